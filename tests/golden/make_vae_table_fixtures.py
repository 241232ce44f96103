#!/usr/bin/env python3
"""Golden fixture F11 for the betaVAE's table pipeline, build container only.

The REFERENCE's src/read_data.py is imported behind the same sys.modules stubs as tests/golden/make_data_fixtures.py (packages
absent here that the table code never touches), and its own sequence (src/betaVAE_training.py:70-105) runs with the real pandas
and scikit-learn on the seeded tables of tests/golden/vae_table_cases.py: ``np.random.seed(99)``, ``train_test_split`` twice per
table, ``pd.concat``, ``normalize_dfs(..., 'standard')``, ``RNADataset``.  Nothing of the reference is re-typed or stored but
what its code computes:

    <part>.wsi      the wsi_file_name list of train / val / test (membership and order of the split)
    <part>.values   the transformed rna_ matrix, fp64
    <part>.rows     the fp32 rows RNADataset hands out
    mean, scale     the fitted StandardScaler's mean_ / scale_
    inverse         scaler.inverse_transform of the seeded fp32 matrix vae_table_cases.inverse_input()

    python tests/golden/make_vae_table_fixtures.py   ->  f11_vae_tables.npz
"""
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

from vae_table_cases import SEED, inverse_input, make_tables  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


for _name in ("lmdb", "lz4framed", "cv2"):
    if _name not in sys.modules:
        try:
            __import__(_name)
        except ImportError:
            _stub(_name)
try:
    import torchvision.io  # noqa: F401
except ImportError:
    _tv = _stub("torchvision")
    _tv.io = _stub("torchvision.io", read_image=None)

import read_data as ref_read_data  # noqa: E402   (reference)
from sklearn.model_selection import train_test_split  # noqa: E402


def main():
    import linecache
    import tempfile
    import textwrap
    # the reference's OWN TEXT (src/betaVAE_training.py:63-105 is inline code of the script, not an importable function),
    # extracted at generation time and executed on the seeded tables written as CSV files -- nothing is re-typed here
    ref_file = os.path.join(REF, "betaVAE_training.py")
    text = "".join(linecache.getline(ref_file, n) for n in range(63, 106))
    assert text.startswith("datasets = {") and text.count("train_test_split(") == 2 and "pd.read_csv(dataset)" in text and \
        "normalize_dfs(train_df, val_df, test_df, norm_type='standard')" in text and \
        text.rstrip().endswith("test_dataset = RNADataset([test_df])"), \
        "src/betaVAE_training.py:63-105 is not the table preparation block any more"
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, df in enumerate(make_tables()):
            paths.append(os.path.join(tmp, "table%d.csv" % i))
            df.to_csv(paths[-1], index=False)
        ns = {"np": np, "pd": pd, "train_test_split": train_test_split, "normalize_dfs": ref_read_data.normalize_dfs,
              "RNADataset": ref_read_data.RNADataset, "path_csv": paths, "quick": 0}
        np.random.seed(SEED)
        exec(compile(textwrap.dedent(text), ref_file + ":63-105", "exec"), ns)
    scaler = ns["scaler"]
    out = {"mean": scaler.mean_.astype(np.float64), "scale": scaler.scale_.astype(np.float64)}
    for name in ("train", "val", "test"):
        df, ds = ns[name + "_df"], ns[name + "_dataset"]
        cols = [c for c in df.columns if "rna_" in c]
        out[name + ".wsi"] = np.array(df["wsi_file_name"].tolist())
        out[name + ".values"] = df[cols].values.astype(np.float64)
        out[name + ".rows"] = np.stack([ds[i]["rna_data"].numpy() for i in range(len(ds))]).astype(np.float32)
    inv = scaler.inverse_transform(inverse_input())
    assert inv.dtype == np.float32
    out["inverse"] = inv
    np.savez_compressed(os.path.join(HERE, "f11_vae_tables.npz"), **out)
    print("wrote f11_vae_tables.npz", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
