"""Pins tests/linprobe_refs.py -- the numpy restatements the GPU tests hold rg_linprobe.hip to -- without a GPU.

* ``fma`` (error-free transformations, rounding to odd) against exact rational arithmetic: float(Fraction) is correctly rounded.
* The chains of scores_ref and colsums_ref against the same chains walked one Python step at a time in exact rationals (so the
  ORDER is pinned, block structure included), and against plain fp64 references within the summation bounds: the matrix product
  within F eps sum |terms|, math.fsum within (rows of a block + blocks) eps sum |terms|.
* softmax_residual_ref against scipy.special.log_softmax.
* The whole fit against sklearn's LogisticRegression(C = 1 / (l2 n), tol = 1e-10) on the same standardised features, through
  strong convexity (lambda = l2): f(ours) - f(sklearn's) <= |grad f(ours)|^2 / (2 lambda) + a few eps |f| -- derived, not tuned --
  and identical predictions wherever the margin exceeds what the implied parameter distance can move the logits."""
import math
from fractions import Fraction

import numpy as np
import pytest

import linprobe_refs as R
from rna_gan_amd import linprobe as LP

EPS = np.finfo(np.float64).eps


def _exact_fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma_is_correctly_rounded():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(4000) * np.exp(rng.uniform(-20, 20, 4000))
    c = rng.standard_normal(4000) * np.exp(rng.uniform(-20, 20, 4000))
    c[:1000] = -(a[:1000] * b[:1000])                        # the addend cancels the rounded product: the low part IS the result
    c[1000:1500] = -(a[1000:1500] * b[1000:1500]) * (1 + 2.0 ** -30)
    got = R.fma(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.count_nonzero(got != a * b + c) > 500, "the operands must be able to tell an fma from multiply-then-add"
    assert np.isnan(R.fma(np.array([np.nan]), np.array([1.0]), np.array([0.0]))[0])
    assert R.fma(np.array([0.0]), np.array([0.0]), np.array([1.5]))[0] == 1.5


def _chain_scores(x, w, bias):
    z = np.empty((x.shape[0], w.shape[0]))
    for r in range(x.shape[0]):
        for c in range(w.shape[0]):
            acc = 0.0
            for f in range(x.shape[1]):
                acc = _exact_fma(x[r, f], w[c, f], acc)
            z[r, c] = acc + bias[c] if bias is not None else acc
    return z


def test_scores_ref_is_the_stated_chain_and_close_to_the_matrix_product():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((9, 37)).astype(np.float32)
    w, bias = rng.standard_normal((3, 37)), rng.standard_normal(3)
    for b in (bias, None):
        got = R.scores_ref(x, w, b)
        assert np.array_equal(got.view(np.uint64), _chain_scores(x, w, b).view(np.uint64))
    x = rng.standard_normal((70, 100)).astype(np.float32)
    w, bias = rng.standard_normal((5, 100)), rng.standard_normal(5)
    xd = x.astype(np.float64)
    got, plain = R.scores_ref(x, w, bias), xd @ w.T + bias
    bound = (100 + 1) * EPS * (np.abs(xd) @ np.abs(w).T + np.abs(bias))
    assert np.all(np.abs(got - plain) <= bound)
    assert not np.array_equal(got, plain), "general floats: the order of the chain must be visible"


def _chain_colsums(x, r, power):
    n, F = x.shape
    C = r.shape[1]
    out = np.zeros((C, F))
    for c in range(C):
        for f in range(F):
            total = 0.0
            for b0 in range(0, n, R.COLSUM_ROWS):
                acc = 0.0
                for row in range(b0, min(n, b0 + R.COLSUM_ROWS)):
                    t = float(x[row, f]) * float(x[row, f]) if power == 2 else float(x[row, f])
                    acc = _exact_fma(r[row, c], t, acc)
                total = total + acc
            out[c, f] = total
    return out


@pytest.mark.parametrize("power", [1, 2])
def test_colsums_ref_is_the_stated_blocked_chain_and_close_to_fsum(power):
    rng = np.random.default_rng(3 + power)
    for n, F, C in ((5, 3, 2), (256, 2, 1), (257, 3, 2), (600, 2, 3)):
        x = rng.standard_normal((n, F)).astype(np.float32)
        r = rng.standard_normal((n, C))
        got = R.colsums_ref(x, r, power)
        assert np.array_equal(got.view(np.uint64), _chain_colsums(x, r, power).view(np.uint64)), (n, F, C)
        t = x.astype(np.float64) ** power
        blocks = -(-n // R.COLSUM_ROWS)
        for c in range(C):
            for f in range(F):
                terms = r[:, c] * t[:, f]
                want = math.fsum(terms)                      # (each term itself carries one rounding: + 1)
                assert abs(got[c, f] - want) <= (min(n, R.COLSUM_ROWS) + blocks + 1) * EPS * math.fsum(np.abs(terms)), (n, c, f)
    ones = np.ones((300, 1), dtype=np.float32)               # the column of ones: plain sums, the same blocked order
    r = rng.standard_normal((300, 2))
    assert np.array_equal(R.colsums_ref(ones, r, power), _chain_colsums(ones, r, power))


def test_softmax_residual_ref_against_scipy():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(5)
    n, C = 200, 7
    z = rng.standard_normal((n, C)) * 5.0
    z[0] = [1000.0, -1000.0, 0.0, 999.0, -3.0, 2.0, 1000.0]
    label = rng.integers(0, C, size=n)
    label[3], label[4] = -1, C                               # masked rows
    wt = rng.uniform(0.5, 2.0, size=n)
    lp = special.log_softmax(z, axis=1)
    ok = (label >= 0) & (label < C)
    y = np.where(ok, label, 0)
    onehot = np.arange(C)[None, :] == y[:, None]
    for weight in (None, wt):
        w = np.ones(n) if weight is None else weight
        for dtype in (np.float64, np.longdouble):
            resid, loss = R.softmax_residual_ref(z, label, weight, dtype)
            assert resid.dtype == dtype and np.isfinite(resid).all() and np.isfinite(loss).all()
            want_r = np.where(ok[:, None], w[:, None] * (np.exp(lp) - onehot), 0.0)
            want_l = np.where(ok, -w * lp[np.arange(n), y], 0.0)
            assert np.allclose(np.asarray(resid, dtype=np.float64), want_r, rtol=1e-12, atol=1e-15)
            assert np.allclose(np.asarray(loss, dtype=np.float64), want_l, rtol=1e-12, atol=1e-13)
            assert not resid[3].any() and not resid[4].any() and loss[3] == 0 and loss[4] == 0
    z[7, 2] = np.nan
    resid, loss = R.softmax_residual_ref(z, np.where(ok, label, 0), None)
    assert np.isnan(resid[7]).all() and np.isnan(loss[7]) and np.isfinite(np.delete(resid, 7, axis=0)).all()


def test_optimiser_minimises_a_quadratic_and_reports_convergence():
    rng = np.random.default_rng(6)
    A = rng.standard_normal((12, 12))
    A = A @ A.T + 0.1 * np.eye(12)
    b = rng.standard_normal(12)
    x, f, g, it, ok = LP.lbfgs(lambda v: (0.5 * v @ A @ v - b @ v, A @ v - b), np.zeros(12), max_iter=200, gtol=1e-6)
    assert ok and it < 100 and np.allclose(x, np.linalg.solve(A, b), atol=1e-4)      # |x - x*| <= |g| / lambda_min, 0.1 here
    _, _, _, it, ok = LP.lbfgs(lambda v: (0.5 * v @ A @ v - b @ v, A @ v - b), np.zeros(12), max_iter=2, gtol=1e-12)
    assert it == 2 and not ok


_FIT = {}


def _fitted():
    if not _FIT:
        x, y = R.blobs(300, 16, 3, sep=4.0, seed=1)
        _FIT.update(x=x, y=y, probe=R.fit(x, y, 3, l2=1e-3))
    return _FIT


def test_fit_reaches_sklearns_optimum_within_the_strong_convexity_bound():
    linear_model = pytest.importorskip("sklearn.linear_model")
    pytest.importorskip("scipy.special")
    ref = _fitted()
    x, y, probe, l2 = ref["x"], ref["y"], ref["probe"], 1e-3
    n = x.shape[0]
    assert probe.converged and probe.n_iter < 200
    f_ours, g_ours = R.objective(x, y, probe.W_std, probe.b_std, probe.mean, probe.scale, l2)
    assert abs(f_ours - probe.objective) <= 64 * EPS * abs(f_ours), "the chained and the vectorised objective are one function"
    assert abs(np.sqrt(g_ours @ g_ours) - probe.grad_norm) <= 1e-9
    xs = (x.astype(np.float64) - probe.mean) / probe.scale
    sk = linear_model.LogisticRegression(C=1.0 / (l2 * n), tol=1e-10, max_iter=10000).fit(xs, y)
    assert sk.coef_.shape == (3, 16)
    f_sk, g_sk = R.objective(x, y, sk.coef_, sk.intercept_, probe.mean, probe.scale, l2)
    gap, bound = f_ours - f_sk, R.strong_convexity_gap(probe, l2)
    print("f(ours) - f(sklearn) = %.3e, bound %.3e; |grad| ours %.3e sklearn %.3e; iterations %d" % (
        gap, bound, probe.grad_norm, np.sqrt(g_sk @ g_sk), probe.n_iter))
    assert gap <= bound
    # both solutions lie within |grad| / lambda of the minimiser: their logits at a point differ by at most D |(x, 1)|
    D = (probe.grad_norm + float(np.sqrt(g_sk @ g_sk))) / l2
    z = xs @ probe.W_std.T + probe.b_std
    top = np.sort(z, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2.0 * D * np.sqrt((xs * xs).sum(axis=1) + 1.0)
    assert clear.mean() > 0.9, "the bound must leave most points to compare (%.2f)" % clear.mean()
    assert np.array_equal(z.argmax(axis=1)[clear], sk.predict(xs)[clear])
    assert LP.accuracy(z.argmax(axis=1), y) > 0.9


def test_fit_arguments_are_checked():
    x, y = R.blobs(40, 4, 2, seed=2)
    with pytest.raises(ValueError, match="l2"):
        R.fit(x, y, 2, l2=0.0)
    with pytest.raises(ValueError, match="l2"):
        R.fit(x, y, 2, l2=float("nan"))
    with pytest.raises(ValueError, match="no training row"):
        R.fit(x, y, 3)
    with pytest.raises(ValueError, match="no training row"):
        R.fit(x, y, 2, mask=y == 0)
    with pytest.raises(ValueError, match="outside"):
        R.fit(x, y + 1, 2)
    with pytest.raises(ValueError):
        R.fit(x, y[:-1], 2)
    const = x.copy()
    const[:, 1] = 3.25                                       # a zero-variance column gets scale 1 and a zero weight
    probe = R.fit(const, y, 2)
    assert probe.scale[1] == 1.0 and probe.converged and abs(probe.W[:, 1]).max() < 1e-9


def test_folds_and_scores_helpers():
    y = np.array([0] * 11 + [1] * 7 + [2] * 5)
    fold = LP.stratified_folds(y, 5, seed=3)
    assert np.array_equal(fold, LP.stratified_folds(y, 5, seed=3)) and not np.array_equal(fold, LP.stratified_folds(y, 5, seed=4))
    for c in range(3):
        per = np.bincount(fold[y == c], minlength=5)
        assert per.max() - per.min() <= 1 and per.sum() == (y == c).sum()
    rng = np.random.default_rng([3, 0xC257])                 # the stated scheme, restated
    want = np.empty(len(y), dtype=np.int64)
    for c in range(3):
        idx = np.nonzero(y == c)[0]
        want[idx[rng.permutation(len(idx))]] = np.arange(len(idx)) % 5
    assert np.array_equal(fold, want)
    with pytest.raises(ValueError, match="fewer"):
        LP.stratified_folds(y, 6)
    pred = np.array([0, 0, 1, 1, 2, 2])
    true = np.array([0, 1, 1, 1, 2, 0])
    assert LP.accuracy(pred, true) == 4 / 6
    assert LP.balanced_accuracy(pred, true, 3) == pytest.approx((1 / 2 + 2 / 3 + 1) / 3)
    assert LP.confusion_matrix(pred, true, 3).tolist() == [[1, 0, 1], [1, 2, 0], [0, 0, 1]]
    metrics = pytest.importorskip("sklearn.metrics")
    assert LP.weighted_f1(pred, true, 3) == pytest.approx(metrics.f1_score(true, pred, average="weighted"))
