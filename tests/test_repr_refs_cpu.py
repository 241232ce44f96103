"""The numpy restatements of tests/repr_refs.py pinned without a GPU against independent formulations, and the CPU-visible side of
the feature: prototypes, header text, ABI version, source list and the parsers of both command lines.

* the sequential chain of group_sums_ref against np.cumsum along the rows of each group (cumsum accumulates sequentially: its
  last row is the chain), general floats over 80 binades (the additions round), bit for bit, starting values included;
* the rank rule against an argsort formulation (position of the target in a stable sort by (d2, index)) on exact-integer cases
  with planted ties on both sides of the target, plus hand-worked NaN cases;
* the scores against hand-worked values."""
import os
import re

import numpy as np
import pytest

from rna_gan_amd import _abi, build
from repr_refs import (dist2_f64, group_sums_ref, integer_rows, match_ranks_ref, ranks_from_d2, retrieval_scores_ref, wide_floats)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,F,G", [(1, 1, 1), (65, 33, 7), (130, 5, 65), (300, 3, 2)])
def test_the_chain_is_cumsum_along_the_rows_of_a_group(n, F, G):
    x = wide_floats(n, F, seed=n + F)
    rng = np.random.default_rng(G)
    ids = rng.integers(-1, G + 1, size=n).astype(np.int32)          # -1 and G: ignored rows
    x[(ids < 0) | (ids >= G)] = np.nan
    start = wide_floats(G, F, seed=9).astype(np.float64) * 1.0000001
    count0 = rng.integers(0, 1 << 40, size=G)
    for s0, c0 in ((None, None), (start, count0)):
        sums, counts = group_sums_ref(x, ids, G, s0, c0)
        for g in range(G):
            rows = x[ids == g].astype(np.float64)
            first = np.zeros((1, F)) if s0 is None else s0[g:g + 1]
            want = np.cumsum(np.concatenate([first, rows]), axis=0)[-1]
            assert np.array_equal(_bits(sums[g]), _bits(want)), (g, s0 is None)
            assert counts[g] == len(rows) + (0 if c0 is None else c0[g])
        assert np.isfinite(sums).all()
    # the order matters in the low bits (so the test above can tell a chain from another order) ...
    if n >= 65:
        rev = group_sums_ref(x[::-1], ids[::-1], G)[0]
        assert not np.array_equal(_bits(rev), _bits(group_sums_ref(x, ids, G)[0]))
    # ... and a split at any boundary is the same chain
    for cut in (1, 63, 64):
        if cut < n:
            part = group_sums_ref(x[:cut], ids[:cut], G)
            both = group_sums_ref(x[cut:], ids[cut:], G, *part)
            whole = group_sums_ref(x, ids, G)
            assert np.array_equal(_bits(both[0]), _bits(whole[0])) and np.array_equal(both[1], whole[1])


@pytest.mark.parametrize("na,nb,F", [(1, 1, 1), (2, 3, 1), (65, 130, 2), (130, 64, 33)])
def test_the_rank_rule_is_the_position_in_a_stable_sort(na, nb, F):
    a, b, target = integer_rows(na, nb, F, seed=na + nb + F)
    d = dist2_f64(a, b)
    assert np.array_equal(d, np.round(d)) and np.array_equal(d, ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))
    rank, dstar = match_ranks_ref(a, b, target)
    for r in range(na):
        order = np.lexsort((np.arange(nb), d[r]))                  # by d2, ties by index
        assert rank[r] == int(np.where(order == target[r])[0][0])
        assert dstar[r] == d[r, target[r]]
    if nb >= 3:                                                    # the planted ties: b[0] == b[t] == b[nb - 1]
        t = nb // 2
        assert d[0, 0] == d[0, t] == d[0, nb - 1] and rank[0] >= 1
        assert rank[0] == int((d[0] < d[0, t]).sum() + (d[0, :t] == d[0, t]).sum())
    if na <= nb:
        r0, _ = match_ranks_ref(a, b, None)
        assert np.array_equal(r0, match_ranks_ref(a, b, np.arange(na))[0])


def test_nan_never_counts_and_a_nan_target_ranks_last():
    d = np.array([[4.0, np.nan, 1.0, 4.0],
                  [np.nan, 2.0, 2.0, 0.0],
                  [3.0, 3.0, 3.0, 3.0]])
    rank, dstar = ranks_from_d2(d, [3, 0, 2])
    assert rank.tolist() == [2, 3, 2] and rank.dtype == np.int32
    assert dstar[0] == 4.0 and np.isnan(dstar[1]) and dstar[2] == 3.0
    assert ranks_from_d2(d, [0, 1, 0])[0].tolist() == [1, 1, 0]
    # the brackets of the general-float test: a scaled threshold, no tie-break
    assert ranks_from_d2(d, [3, 0, 2], 1.5)[0].tolist() == [2, 3, 3]
    assert ranks_from_d2(d, [3, 0, 2], 0.5)[0].tolist() == [1, 3, 0]


def test_scores_by_hand():
    s = retrieval_scores_ref([0, 0, 1, 4, 5, 9], 10)
    assert s["top1"] == 2 / 6 and s["top5"] == 4 / 6 and s["median_rank"] == 2.5 and s["chance_top1"] == 0.1
    assert s["mrr"] == float(np.mean([1.0, 1.0, 0.5, 0.2, 1 / 6, 0.1]))
    s = retrieval_scores_ref([0, 2, 1], 3)                          # top5 is capped at the number of reference rows
    assert s["top5"] == 1.0 and s["top1"] == 1 / 3 and s["chance_top1"] == 1 / 3
    from rna_gan_amd.representation import retrieval_scores
    for ranks, n_ref in (([0, 0, 1, 4, 5, 9], 10), ([0, 2, 1], 3), ([7], 8)):
        assert retrieval_scores(np.array(ranks, dtype=np.int32), n_ref) == retrieval_scores_ref(ranks, n_ref)


# ------------------------------------------------------------------ the boundary
def test_prototypes_header_version_and_sources():
    assert _abi.ABI_VERSION == 618
    p, i = _abi._p, _abi._i
    assert _abi.PROTOTYPES["rg_group_sums_update"] == (i, [p, i, i, i, p, i, p, p, p])
    assert _abi.PROTOTYPES["rg_match_ranks"] == (i, [p, i, i, p, i, i, i, p, p, p, p])
    assert "rg_groupstat.hip" in build.SOURCES and "rg_groupstat.hip" not in build.BF16_ONLY
    assert os.path.exists(os.path.join(ROOT, "rna_gan_amd", "csrc", "rg_groupstat.hip"))
    header = open(os.path.join(ROOT, "include", "rnagan_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int rg_group_sums_update(const float* x, int ldx, int n, int F, const int32_t* group, int G, double* sums, "
            "long long* counts, void* stream);") in flat
    assert ("int rg_match_ranks(const double* a, int lda, int na, const double* b, int ldb, int nb, int F, const int32_t* target, "
            "int32_t* rank, double* dtarget, void* stream);") in flat
    for phrase in ("ascending r", "no atomics", "neither summed nor counted", "ties are broken by index", "rank[r] = nb - 1", "CLAMPED"):
        assert phrase in flat, phrase
    src = open(os.path.join(ROOT, "rna_gan_amd", "csrc", "rg_api.hip")).read()
    assert re.search(r"rg_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+618\s*;", src), "rg_version() stays equal to ABI_VERSION"


def test_training_cli_flags():
    import histopathology_gan as H
    base = ["--config", "c.json"]
    off = H.parse_args(base)
    assert (off.cf_patients, off.cf_tiles, off.cf_report) == (0, 8, "top1")
    plain = H.parse_args(base + ["--loss_type", "wganvae"])
    on = H.parse_args(base + ["--loss_type", "wganvae", "--cf_patients", "4", "--cf_tiles", "3", "--cf_report", "mrr"])
    assert (on.cf_patients, on.cf_tiles, on.cf_report) == (4, 3, "mrr")
    changed = {k for k in vars(on) if vars(on)[k] != vars(plain)[k]}
    assert changed == {"cf_patients", "cf_tiles", "cf_report"}, "the defaults change nothing else"
    for bad in (["--loss_type", "wganvae", "--cf_patients", "1"], ["--loss_type", "wgangp", "--cf_patients", "4"],
                ["--cf_patients", "4"], ["--loss_type", "wgan", "--cf_patients", "2"], ["--loss_type", "wganvae", "--cf_patients", "-2"],
                ["--loss_type", "wganvae", "--cf_patients", "4", "--cf_tiles", "0"],
                ["--loss_type", "wganvae", "--cf_patients", "4", "--cf_report", "top3"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)


def test_representation_cli_flags(tmp_path):
    import compute_representation as CR
    base = ["--config", "c.json", "--path_to_save", str(tmp_path / "rep"), "--sample_size", "4"]
    a = CR.parse_args(base + ["--synthetic"])
    assert (a.seed, a.gan, a.vaegan, a.vae_checkpoint, a.multiprocessing, a.extractor, a.synthetic) == \
        (99, None, None, None, False, "discriminator", True)
    b = CR.parse_args(base + ["--gan", "g.model", "--vaegan", "v.model", "--vae_checkpoint", "b.pt", "--seed", "5", "--multiprocessing"])
    assert (b.gan, b.vaegan, b.vae_checkpoint, b.seed, b.multiprocessing, b.synthetic, b.sample_size) == \
        ("g.model", "v.model", "b.pt", 5, True, False, 4)
    for bad in (base, base + ["--synthetic", "--extractor", str(tmp_path / "no_such_file")], base[:4] + ["--synthetic"],
                base[2:] + ["--synthetic"], base[:4] + ["--sample_size", "0", "--synthetic"]):
        with pytest.raises(SystemExit):
            CR.parse_args(bad)
