"""Seeded expression tables shared by tests/golden/make_vae_table_fixtures.py and tests/test_rna_tables_cpu.py: two tables of 23
and 17 rows x 9 ``rna_`` columns plus ``wsi_file_name`` and one more non-RNA column, with zeros, one constant column and one
column that is constant within the train split (under SEED) only."""
import math

import numpy as np
import pandas as pd

SEED = 99
ROWS = (23, 17)
GENES = 9
CONSTANT, TRAIN_CONSTANT = 5, 7


def _train_rows():
    """Row positions of each table that land in the train split under SEED: the split rule on a PRIVATE legacy generator (the
    stream np.random.seed(SEED) starts on the global one), so that building the tables leaves the global generator alone."""
    rs = np.random.RandomState(SEED)
    out = []
    for m in ROWS:
        p = rs.permutation(m)
        nt = int(math.ceil(0.2 * m))
        train = p[nt:nt + int(math.floor(0.8 * m))]
        p2 = rs.permutation(len(train))
        nt2 = int(math.ceil(0.2 * len(train)))
        out.append(train[p2[nt2:nt2 + int(math.floor(0.8 * len(train)))]])
    return out


def make_tables():
    rng = np.random.default_rng(1311)
    train_rows = _train_rows()
    tables = []
    for t, m in enumerate(ROWS):
        rna = np.round(rng.gamma(1.5, 20.0, size=(m, GENES)), 3)
        rna[rng.integers(0, m, size=5), rng.integers(0, GENES, size=5)] = 0.0       # zeros stay 0 after the log
        rna[:, CONSTANT] = 4.0                                                       # a constant gene: the scaler divides by 1
        rna[:, TRAIN_CONSTANT] = np.round(rng.gamma(2.0, 3.0, size=m), 3) + 1.0
        rna[train_rows[t], TRAIN_CONSTANT] = 2.5                                     # constant where the scaler is fitted only
        cols = {"wsi_file_name": ["GTEX-T%d-%04d.svs" % (t, i) for i in range(m)]}
        for j in range(GENES):
            cols["rna_G%d" % j] = rna[:, j]
        cols["tissue"] = ["lung", "brain"][t]
        tables.append(pd.DataFrame(cols))
    return tables


def inverse_input():
    """The seeded fp32 matrix whose inverse_transform the fixture stores."""
    return np.random.default_rng(1312).normal(size=(6, GENES)).astype(np.float32)
