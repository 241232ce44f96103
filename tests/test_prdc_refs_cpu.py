"""Precision / recall / density / coverage, checked without a GPU: the numpy restatements of tests/prdc_refs.py against a
brute-force pure-Python definition in exact rational arithmetic (fractions.Fraction) and hand-worked cases, the binding's
prototypes, the host side of rna_gan_amd.prdc, and the PrecisionRecall plumbing (constructor, pickle with history, CLI flags)."""
import pickle
from fractions import Fraction

import numpy as np
import pytest
import torch

import rna_gan_amd as P
from rna_gan_amd import _abi
from rna_gan_amd import prdc as PR
from rna_gan_amd.metrics import EvaluationMetric, FrechetDistance, KernelDistance, PrecisionRecall
from prdc_refs import GAMMA, U, dist2, hits_ref, integer_case, prdc_ref, radii2_ref


# ------------------------------------------------------------------ the definitions, brute force in exact arithmetic
def _d2_exact(a, b):
    return sum((Fraction(float(p)) - Fraction(float(q))) ** 2 for p, q in zip(a, b))


def _radii_exact(a, k):
    return [sorted(_d2_exact(a[i], a[j]) for j in range(len(a)) if j != i)[k - 1] for i in range(len(a))]


def _prdc_exact(x, y, k):
    m, n = len(x), len(y)
    rx, ry = _radii_exact(x, k), _radii_exact(y, k)
    in_real = [sum(_d2_exact(x[i], y[j]) <= rx[i] for i in range(m)) for j in range(n)]
    in_fake = [sum(_d2_exact(x[i], y[j]) <= ry[j] for j in range(n)) for i in range(m)]
    nearest = [min(_d2_exact(x[i], y[j]) for j in range(n)) for i in range(m)]
    return {"precision": Fraction(sum(c > 0 for c in in_real), n), "recall": Fraction(sum(c > 0 for c in in_fake), m),
            "density": Fraction(sum(in_real), k * n), "coverage": Fraction(sum(nearest[i] <= rx[i] for i in range(m)), m)}


def _dyadic_case(m, n, F, seed):
    """multiples of 1 / 8 in [-4, 4]: every difference, square and sum is exact in fp64"""
    rng = np.random.default_rng(seed)
    return ((rng.integers(-32, 33, size=(m, F)) / 8.0).astype(np.float32), (rng.integers(-32, 33, size=(n, F)) / 8.0).astype(np.float32))


@pytest.mark.parametrize("m,n,F,k,seed", [(7, 6, 1, 1, 0), (7, 6, 3, 2, 1), (9, 12, 5, 3, 2), (6, 6, 2, 5, 3), (12, 5, 4, 4, 4)])
def test_restatement_against_exact_arithmetic(m, n, F, k, seed):
    for x, y in (integer_case(m, n, F, seed), _dyadic_case(m, n, F, seed)):
        d = dist2(x, y)
        assert all(Fraction(float(d[i, j])) == _d2_exact(x[i], y[j]) for i in range(m) for j in range(n))
        assert [Fraction(float(v)) for v in radii2_ref(x, k)] == _radii_exact(x, k)
        assert [Fraction(float(v)) for v in radii2_ref(y, k)] == _radii_exact(y, k)
        ry = radii2_ref(y, k)
        count, mind2 = hits_ref(x, y, ry)
        assert count.dtype == np.int32
        assert list(count) == [sum(_d2_exact(x[i], y[j]) <= Fraction(float(ry[j])) for j in range(n)) for i in range(m)]
        assert [Fraction(float(v)) for v in mind2] == [min(_d2_exact(x[i], y[j]) for j in range(n)) for i in range(m)]
        none, again = hits_ref(x, y)
        assert none is None and np.array_equal(again, mind2)
        got, want = prdc_ref(x, y, k), _prdc_exact(x, y, k)
        assert {key: Fraction(v) for key, v in got.items()} == {key: Fraction(float(v)) for key, v in want.items()}


def test_integer_case_has_ties_and_duplicates():
    a, b = integer_case(130, 65, 33, seed=3)
    assert np.array_equal(a[129], a[0]) and np.array_equal(b[32], a[0]) and np.array_equal(b[64], b[0])
    d = dist2(a, a)
    assert d[0, 129] == 0.0 and np.array_equal(d, d.T) and np.all(d == np.round(d)) and np.all(np.diagonal(d) == 0.0)
    r1 = radii2_ref(a, 1)
    assert r1[0] == 0.0 and r1[129] == 0.0 and r1[1] > 0.0      # index exclusion: the duplicate counts, the row itself does not
    assert len(np.unique(d)) < d.size // 50                     # exact ties everywhere


def test_order_of_the_features_does_not_matter_on_integers_but_is_the_contract_on_floats():
    a, b = integer_case(5, 4, 70, seed=1)
    assert np.array_equal(dist2(a, b), dist2(a[:, ::-1], b[:, ::-1]))
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((8, 70)).astype(np.float32), rng.standard_normal((6, 70)).astype(np.float32)
    d, e = dist2(x, y), dist2(x[:, ::-1], y[:, ::-1])
    exact = np.array([[float(_d2_exact(p, q)) for q in y] for p in x])
    g = GAMMA(70)
    assert np.all(np.abs(d - exact) <= g * exact) and np.all(np.abs(e - exact) <= g * exact)
    assert np.array_equal(d.T, dist2(y, x)) and np.all(d >= 0.0) and np.all(np.diagonal(dist2(x, x)) == 0.0)
    assert 0 < GAMMA(70) < 73 * U


# ------------------------------------------------------------------ hand-worked cases
def _col(*v):
    return np.array(v, dtype=np.float32)[:, None]


def test_duplicate_rows_give_radius_zero():
    a = _col(0, 0, 1)
    assert list(radii2_ref(a, 1)) == [0.0, 0.0, 1.0]
    assert list(radii2_ref(a, 2)) == [1.0, 1.0, 1.0]
    # three copies: the radius stays 0 at k = 2
    assert list(radii2_ref(_col(5, 5, 5, 9), 2)) == [0.0, 0.0, 0.0, 16.0]


def test_an_exact_tie_hits():
    x, y = _col(0, 2), _col(4, 10)
    assert list(radii2_ref(x, 1)) == [4.0, 4.0] and list(radii2_ref(y, 1)) == [36.0, 36.0]
    # d2(y_0, x_1) = 4 = r2_X[1]: a hit under <=; under < it would not be, and precision and coverage would be 0
    assert prdc_ref(x, y, 1) == {"precision": 0.5, "recall": 1.0, "density": 0.5, "coverage": 0.5}
    count, mind2 = hits_ref(y, x, radii2_ref(x, 1))
    assert list(count) == [1, 0] and list(mind2) == [4.0, 64.0]
    # the interval of the general-float test brackets the tie from both sides
    assert list(hits_ref(y, x, radii2_ref(x, 1), 1 + 2 * GAMMA(1))[0]) == [0, 0]
    assert list(hits_ref(y, x, radii2_ref(x, 1), 1 - 2 * GAMMA(1))[0]) == [1, 0]


def test_k_equal_to_n_minus_one_is_the_farthest_row():
    a = _col(0, 1, 3, 7)
    assert list(radii2_ref(a, 3)) == [49.0, 36.0, 16.0, 49.0]


def test_fidelity_without_diversity_and_the_reverse():
    wide, narrow = _col(0, 100, 200, 300), _col(49, 50, 51)
    assert list(radii2_ref(wide, 1)) == [10000.0] * 4 and list(radii2_ref(narrow, 1)) == [1.0, 1.0, 1.0]
    # a collapsed generator inside the real manifold: every generated row is inside a real ball, no real row inside a generated one
    assert prdc_ref(wide, narrow, 1) == {"precision": 1.0, "recall": 0.0, "density": 2.0, "coverage": 0.5}
    # the roles swapped: the generated set covers the real one, and none of it lies inside the (tiny) real balls
    assert prdc_ref(narrow, wide, 1) == {"precision": 0.0, "recall": 1.0, "density": 0.0, "coverage": 0.0}
    # two disjoint clusters
    assert prdc_ref(_col(0, 1, 2), _col(1000, 1001, 1002), 1) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}


def test_identical_sets():
    x = _col(0, 1, 3, 7, 15)                                  # all ten pairwise distances differ
    # every row lies in its own ball and in those of the rows that count it among their k nearest... the balls of x_i hold
    # exactly k + 1 rows (itself and its k nearest): density = (k + 1) / k
    assert prdc_ref(x, x.copy(), 2) == {"precision": 1.0, "recall": 1.0, "density": 1.5, "coverage": 1.0}
    assert prdc_ref(x, x.copy(), 1) == {"precision": 1.0, "recall": 1.0, "density": 2.0, "coverage": 1.0}


def test_a_nan_row_never_hits_and_has_an_infinite_radius():
    a = np.array([[0, 0], [1, 0], [np.nan, 0], [0, 2]], dtype=np.float32)
    r = radii2_ref(a, 1)
    assert list(r) == [1.0, 1.0, np.inf, 4.0]
    assert list(radii2_ref(a, 3)) == [np.inf] * 4                # only two finite neighbours each
    b = np.array([[0, 1], [np.nan, np.nan]], dtype=np.float32)
    count, mind2 = hits_ref(a, b, np.array([np.inf, np.inf]))
    assert list(count) == [1, 1, 0, 1] and list(mind2) == [1.0, 2.0, np.inf, 1.0]


# ------------------------------------------------------------------ the binding
def test_abi_carries_the_three_symbols():
    assert _abi.ABI_VERSION == 618
    p, i, z = _abi._p, _abi._i, _abi._z
    assert _abi.PROTOTYPES["rg_pairdist_ws_bytes"] == (z, [i, i, i])
    assert _abi.PROTOTYPES["rg_knn_radii2"] == (i, [p, i, i, i, i, p, z, p, p])
    assert _abi.PROTOTYPES["rg_radius_hits"] == (i, [p, i, i, p, i, i, i, p, p, z, p, p, p])
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnagan_hip.h")).read()
    for name in ("rg_pairdist_ws_bytes(", "rg_knn_radii2(", "rg_radius_hits("):
        assert name in header


# ------------------------------------------------------------------ rna_gan_amd.prdc, host side
def test_prdc_argument_checks():
    x = torch.zeros(8, 4)
    for fn in (lambda: PR.knn_radii2(x, 3), lambda: PR.radius_hits(x, x), lambda: PR.prdc(x, x)):
        with pytest.raises(TypeError):
            fn()                                                # host tensors: there is no CPU fallback
    for k in (0, 17, -1):
        with pytest.raises(ValueError):
            PR._check_k(k, 100, "x")
    with pytest.raises(ValueError):
        PR._check_k(5, 5, "x")
    assert PR._check_k(5, 6, "x") == 5 and PR._check_k(16, 17, "x") == 16
    assert callable(PR.precision_recall) and callable(PR.density_coverage) and callable(PR.calculate_prdc)


# ------------------------------------------------------------------ PrecisionRecall plumbing (no device)
def test_precision_recall_is_exported_and_validates():
    assert P.PrecisionRecall is PrecisionRecall and "PrecisionRecall" in P.__all__ and issubclass(PrecisionRecall, EvaluationMetric)
    real = torch.zeros(8, 3, 32, 32, dtype=torch.uint8)
    m = PrecisionRecall(real)
    assert (m.n_fake, m.nearest_k, m.report, m.last, m.history) == (8, 5, "recall", None, [])
    for bad in (dict(nearest_k=0), dict(nearest_k=17), dict(nearest_k=8), dict(report="fidelity"), dict(n_fake=5),
                dict(extractor="inception"), dict(noise=torch.ones(7, 16)), dict(batch_size=0)):
        with pytest.raises(ValueError):
            PrecisionRecall(real, **bad)
    assert PrecisionRecall(real, nearest_k=7, n_fake=8, report="density").report == "density"
    with pytest.raises(ValueError):
        m.set_real(real[:5])
    with pytest.raises(TypeError):
        PrecisionRecall(real.to(torch.int32))
    import inspect
    assert list(inspect.signature(m.metric_ops).parameters) == list(inspect.signature(FrechetDistance(real).metric_ops).parameters)


def test_precision_recall_pickles_settings_and_history_only():
    real = torch.randint(0, 256, (64, 3, 64, 64), dtype=torch.uint8)
    m = PrecisionRecall(real, n_fake=48, seed=3, batch_size=16, encoding_dims=128, nearest_k=3, report="coverage")
    m.set_arg_map({"generator": "generator_ema"})
    m._real_stats = torch.zeros(64, 2048)
    m._real_radii = torch.zeros(64, dtype=torch.float64)
    four = {"precision": 0.5, "recall": 0.25, "density": 1.5, "coverage": 0.75}
    m.last = dict(four)
    m.history.append(dict(four))
    blob = pickle.dumps(m)
    assert len(blob) < 64 * 1024, len(blob)
    back = pickle.loads(blob)
    assert (back.n_fake, back.seed, back.batch_size, back.extractor, back.nearest_k, back.report) == (48, 3, 16, "discriminator", 3, "coverage")
    assert back.arg_map == {"generator": "generator_ema"} and back.history == [four] and back.history is not m.history
    assert back.real is None and back.noise is None and back._real_stats is None and back._real_radii is None and back.last is None
    with pytest.raises(RuntimeError, match="PrecisionRecall"):
        back.metric_ops(None, None, torch.device("cpu"))
    back.set_real(real)
    assert back.real is real
    # the neighbouring metrics' pickle states are what they were
    assert sorted(FrechetDistance(real).__getstate__()) == ["arg_map", "batch_size", "extractor", "n_fake", "seed"]
    assert "history" not in KernelDistance(real).__getstate__()
    # one seed, one noise for all three metrics
    assert torch.equal(FrechetDistance(real, seed=3, n_fake=48, encoding_dims=128).noise, m.noise)


# ------------------------------------------------------------------ CLI
def test_cli_flags(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json"]
    a = H.parse_args(base)
    assert (a.pr_samples, a.pr_k, a.pr_report) == (0, 5, "recall")
    a = H.parse_args(base + ["--pr_samples", "2048", "--pr_k", "3", "--pr_report", "precision"])
    assert (a.pr_samples, a.pr_k, a.pr_report) == (2048, 3, "precision")
    assert H.parse_args(base + ["--pr_samples", "6"]).pr_samples == 6
    for bad in (["--pr_samples", "-1"], ["--pr_samples", "5"], ["--pr_samples", "3", "--pr_k", "3"], ["--pr_samples", "many"],
                ["--pr_k", "0"], ["--pr_k", "17"], ["--pr_report", "fidelity"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()


def test_cli_metrics_share_the_real_set_and_the_extractor():
    import histopathology_gan as H
    args = H.parse_args(["--config", "c.json", "--fd_samples", "6", "--kid_samples", "6", "--pr_samples", "6", "--pr_k", "2",
                         "--pr_report", "density", "--loss_type", "wgan", "--seed", "5"])
    ds = H.SyntheticTiles(8, 32, 4, False, 0)
    holder = {}
    fd = H.build_fd_metric(args, ds, [], torch.device("cpu"), holder)
    kd = H.build_kid_metric(args, ds, [], torch.device("cpu"), holder)
    pr = H.build_pr_metric(args, ds, [], torch.device("cpu"), holder)
    assert isinstance(pr, PrecisionRecall)
    assert pr.real is fd.real and pr.real is kd.real and pr.noise is fd.noise and pr.extractor == fd.extractor == kd.extractor
    assert (pr.nearest_k, pr.report, pr.seed, pr.batch_size, pr.n_fake) == (2, "density", 5, 6, 6)
    args.pr_samples = 4
    other = H.build_pr_metric(args, ds, [], torch.device("cpu"), holder)
    assert other.real is not fd.real and other.real.shape[0] == 4
