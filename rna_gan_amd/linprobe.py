"""Linear-probe scores on feature rows that stay on the device: the classifier two-sample test and train-on-synthetic.

Both are multinomial logistic regression on (n, F) fp32 features:

``c2st``   (Lopez-Paz & Oquab 2017) the held-out accuracy of a classifier trained to tell real from generated features,
           cross-validated: 0.5 = indistinguishable, 1.0 = trivially separable.
``tstr``   (Ravuri & Vinyals 2019, the "classification accuracy score") a tissue classifier trained on GENERATED features, each
           labelled with the tissue of the expression row that conditioned it, tested on the real ones -- next to the same
           classifier cross-validated on the real features (``trtr``, the ceiling) and their ratio.  It collapses when the
           generator ignores the tissue, drops one, or produces tiles whose class evidence is not the real one.

It is the counterpart, on frozen features, of the question src/ml_experiments.py asks by fine-tuning a ResNet-50 (that script
does not parse: SURVEY.md 2, row 15); see tissue_probe.py.  These are functions of feature sets; they are not attached to the
Trainer as per-epoch metrics (rna_gan_amd.metrics) yet.

The fit.  The objective is  (1 / sum wt) sum_rows wt * cross-entropy + (l2 / 2) |W|^2  in STANDARDISED coordinates (column mean
and standard deviation of the training rows; the bias is not penalised), minimised by a plain L-BFGS on the host in numpy fp64
over C x (F + 1) numbers.  One evaluation of loss and gradient is, on the device and in fp64 with a fixed summation order
(include/rnagan_hip.h): rg_linear_scores_f64 (the standardisation folded into W and b on the host), rg_softmax_residual_f64,
rg_rows_weighted_colsums_f64 of the residual against the features (the gradient), against a column of ones (the bias gradient)
and of the row losses (the loss), then ONE download of C F + C + 1 doubles.  Rows are held out by label -1: the kernels mask
them, the feature matrix is never gathered or copied.  The features must be finite (0 * NaN is NaN: a masked row still enters the
column sums as an exact zero times its features).

The optimiser takes its loss-and-gradient function as a parameter and the fit takes its three device operations as an object:
tests/linprobe_refs.py runs the same code on numpy restatements of the kernels.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from .kid import _rows

FOLD_STREAM = 0xC257         # second word of the fold generator's seed: default_rng([seed, FOLD_STREAM])


@dataclass
class LinearProbe:
    """A fitted probe.  ``W`` (C, F) and ``b`` (C,) act on RAW features (logits = x W^T + b); ``mean`` and ``scale`` (F,) are the
    standardisation of the training rows they were fitted under, ``W_std`` / ``b_std`` the same classifier in standardised
    coordinates (the ones the objective and its penalty are stated in).  ``objective`` and ``grad_norm`` (the Euclidean norm of
    the gradient over all C (F + 1) parameters) are those of the last iterate, ``converged`` says max |gradient| <= gtol."""
    W: np.ndarray
    b: np.ndarray
    mean: np.ndarray
    scale: np.ndarray
    W_std: np.ndarray
    b_std: np.ndarray
    n_iter: int
    converged: bool
    objective: float
    grad_norm: float

    @property
    def n_classes(self):
        return self.W.shape[0]


# ---------------------------------------------------------------------------------------------------------------- optimiser
def lbfgs(fun, x0, max_iter=200, gtol=1e-6, memory=10, c1=1e-4, max_halvings=25):
    """Plain L-BFGS with a backtracking Armijo line search, numpy fp64.  fun(x) -> (f, g).  Stops when max |g| <= gtol
    (converged), after max_iter iterations, or when the line search finds no decrease (the iterate is then as good as fp64
    evaluates f).  The first step is 1 / max(1, |g|), later ones start from 1 (the two-loop direction is scaled by s.y / y.y);
    a pair with s.y <= 0 is not stored.  Returns (x, f, g, iterations, converged)."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    S, Y = [], []
    it = 0
    while it < max_iter and not np.max(np.abs(g)) <= gtol:
        q = g.copy()
        alpha = []
        for s, y in zip(reversed(S), reversed(Y)):
            a = float(s @ q) / float(y @ s)
            alpha.append(a)
            q -= a * y
        if S:
            q *= float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])
        for (s, y), a in zip(zip(S, Y), reversed(alpha)):
            q += (a - float(y @ q) / float(y @ s)) * s
        d = -q
        slope = float(g @ d)
        if not slope < 0.0:                                  # not a descent direction (rounding): restart from steepest descent
            S, Y = [], []
            d, slope = -g, -float(g @ g)
        t = 1.0 if S else 1.0 / max(1.0, math.sqrt(-slope))
        for _ in range(max_halvings):
            xn = x + t * d
            fn, gn = fun(xn)
            if fn <= f + c1 * t * slope:
                break
            t *= 0.5
        else:
            break
        s, y = xn - x, gn - g
        if float(s @ y) > 1e-300:
            S.append(s); Y.append(y)
            if len(S) > memory:
                S.pop(0); Y.pop(0)
        x, f, g = xn, fn, gn
        it += 1
    return x, float(f), g, it, bool(np.max(np.abs(g)) <= gtol)


# ---------------------------------------------------------------------------------------------------------------- the fit
def standardisation(s1, s2, count):
    """(mean, scale) of the training rows from their column sums, sums of squares and number: mean = s1 / count, variance =
    s2 / count - mean^2, scale = its square root.  A zero-variance column gets scale 1; a variance at the rounding level of its
    own subtraction (<= 64 eps s2 / count) counts as zero -- its square root would be noise that the fit would divide by."""
    mean = s1 / count
    m2 = s2 / count
    var = m2 - mean * mean
    scale = np.sqrt(np.maximum(var, 0.0))
    scale[var <= 64.0 * np.finfo(np.float64).eps * m2] = 1.0
    return mean, scale


def fit_with_ops(ops, n, F, y, n_classes, l2=1e-3, sample_weight=None, mask=None, max_iter=200, gtol=1e-6):
    """``fit`` on an object that supplies the operations: ``ops.moments(mask01) -> (s1, s2)`` (column sums and sums of squares
    of the rows with mask01 == 1, host fp64), ``ops.set_rows(label, weight)`` -- called once per fit with the int32 labels (-1 on
    the rows left out) and the per-row weights or None -- and ``ops.evaluate(W, b) -> (G, rs, loss)`` for raw-coordinate weights
    W (C, F), b (C,): G = resid^T x (C, F), rs = the column sums of resid (C,), loss = the sum of the row losses, host fp64."""
    C = int(n_classes)
    l2 = float(l2)
    if not (math.isfinite(l2) and l2 > 0.0):
        raise ValueError("l2 must be finite and > 0")
    if C < 1:
        raise ValueError("n_classes must be >= 1")
    y = np.asarray(y)
    if y.ndim != 1 or y.shape[0] != n or not np.issubdtype(y.dtype, np.integer):
        raise ValueError("y must hold one integer label per row (%d), got %s %s" % (n, y.dtype, tuple(y.shape)))
    if mask is None:
        mask = np.ones(n, dtype=bool)
    else:
        mask = np.asarray(mask)
        if mask.shape != (n,) or mask.dtype != np.bool_:
            raise ValueError("mask must be %d booleans" % n)
    if n < 1 or not mask.any():
        raise ValueError("no training rows")
    if (y[mask] < 0).any() or (y[mask] >= C).any():
        raise ValueError("a training label lies outside [0, %d)" % C)
    counts = np.bincount(y[mask], minlength=C)
    if (counts == 0).any():
        raise ValueError("class %d has no training row" % int(np.argmin(counts != 0)))
    label = np.where(mask, y, -1).astype(np.int32)
    weight = None
    total = float(mask.sum())
    if sample_weight is not None:
        weight = np.asarray(sample_weight, dtype=np.float64)
        if weight.shape != (n,) or not np.isfinite(weight).all() or (weight < 0).any():
            raise ValueError("sample_weight must be %d finite values >= 0" % n)
        total = math.fsum(weight[mask])
        if not total > 0.0:
            raise ValueError("the training rows carry no weight")
    mean, scale = standardisation(*ops.moments(mask.astype(np.float64)), float(mask.sum()))
    ops.set_rows(label, weight)

    def fun(theta):
        Ws, bs = theta[:C * F].reshape(C, F), theta[C * F:]
        W = Ws / scale
        b = bs - W @ mean
        G, rs, loss = ops.evaluate(W, b)
        gW = (G - rs[:, None] * mean[None, :]) / scale / total + l2 * Ws
        f = loss / total + 0.5 * l2 * float(np.sum(Ws * Ws))
        return f, np.concatenate([gW.reshape(-1), rs / total])

    theta, f, g, it, ok = lbfgs(fun, np.zeros(C * F + C), max_iter=max_iter, gtol=gtol)
    Ws, bs = theta[:C * F].reshape(C, F).copy(), theta[C * F:].copy()
    W = Ws / scale
    return LinearProbe(W=W, b=bs - W @ mean, mean=mean, scale=scale, W_std=Ws, b_std=bs, n_iter=it, converged=ok, objective=f,
                       grad_norm=float(np.sqrt(g @ g)))


class _DeviceOps:
    """the three entry points on one (n, F) fp32 device tensor, read where it lies; every buffer is allocated once and serves
    any number of fits on these rows (the folds of a cross-validation)"""

    def __init__(self, x, ldx, C):
        self.x, self.ldx, self.C = x, ldx, C
        self.n, self.F = x.shape
        n, F, dev = self.n, self.F, x.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.z, self.resid, self.row_loss = torch.empty(n, C, **f64), torch.empty(n, C, **f64), torch.empty(n, **f64)
        self.ones = torch.ones(n, 1, dtype=torch.float32, device=dev)
        self.params = torch.empty(C * F + C, **f64)
        self.out = torch.empty(max(C * F + C + 1, 2 * F), **f64)
        ws_bytes = _abi.load().rg_colsums_ws_bytes
        need = max(ws_bytes(n, F, C), ws_bytes(n, 1, C))
        self.ws = torch.empty(max(need, 8) // 8, **f64)
        self.label = torch.full((n,), -1, dtype=torch.int32, device=dev)       # until set_rows: every row left out
        self.weight, self.weighted = torch.empty(n, **f64), False

    def _colsums(self, x, ldx, F, r, ldr, C, power, out):
        _abi.launch("rg_rows_weighted_colsums_f64", self.x.device, x.data_ptr(), ldx, self.n, F, r.data_ptr(), ldr, C, power,
                    self.ws.data_ptr(), self.ws.numel() * 8, out.data_ptr())

    def moments(self, mask01):
        F = self.F
        r = torch.from_numpy(np.ascontiguousarray(mask01, dtype=np.float64)).to(self.x.device)
        self._colsums(self.x, self.ldx, F, r, 1, 1, 1, self.out[:F])
        self._colsums(self.x, self.ldx, F, r, 1, 1, 2, self.out[F:2 * F])
        host = self.out[:2 * F].cpu().numpy()
        return host[:F].copy(), host[F:].copy()

    def logits(self, W, b):
        """z = x W^T + b into self.z (the (n, C) fp64 device buffer of this object)"""
        C, F = self.C, self.F
        self.params.copy_(torch.from_numpy(np.concatenate([np.ascontiguousarray(W, dtype=np.float64).reshape(-1),
                                                           np.ascontiguousarray(b, dtype=np.float64)])))
        p = self.params.data_ptr()
        _abi.launch("rg_linear_scores_f64", self.x.device, self.x.data_ptr(), self.ldx, self.n, F, p, F, C, p + 8 * C * F,
                    self.z.data_ptr(), C)
        return self.z

    def set_rows(self, label, weight):
        """upload the labels (int32, -1 = left out) and the weights (fp64 or None) that every later ``evaluate`` uses"""
        self.label.copy_(torch.from_numpy(np.ascontiguousarray(label, dtype=np.int32)))
        self.weighted = weight is not None
        if self.weighted:
            self.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float64)))

    def evaluate(self, W, b):
        C, F, n = self.C, self.F, self.n
        self.logits(W, b)
        _abi.launch("rg_softmax_residual_f64", self.x.device, self.z.data_ptr(), C, n, C, self.label.data_ptr(),
                    self.weight.data_ptr() if self.weighted else None, self.resid.data_ptr(), C, self.row_loss.data_ptr())
        self._colsums(self.x, self.ldx, F, self.resid, C, C, 1, self.out[:C * F])
        self._colsums(self.ones, 1, 1, self.resid, C, C, 1, self.out[C * F:C * F + C])
        self._colsums(self.ones, 1, 1, self.row_loss, 1, 1, 1, self.out[C * F + C:C * F + C + 1])
        host = self.out[:C * F + C + 1].cpu().numpy()
        return host[:C * F].reshape(C, F).copy(), host[C * F:C * F + C].copy(), float(host[C * F + C])


def _labels(y, n, what="y"):
    """integer labels (tensor or array) as a host int64 vector of n"""
    if torch.is_tensor(y):
        if y.is_floating_point() or y.dtype == torch.bool:
            raise TypeError("%s must hold integers" % what)
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if not np.issubdtype(y.dtype, np.integer):
        raise TypeError("%s must hold integers" % what)
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError("%s must hold one label per row (%d), got %s" % (what, n, tuple(y.shape)))
    return y.astype(np.int64)


def _host_vector(v, n, what, dtype):
    if v is None:
        return None
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    if v.shape != (n,):
        raise ValueError("%s must hold one value per row (%d), got %s" % (what, n, tuple(v.shape)))
    return v.astype(dtype)


def fit(x, y, n_classes, l2=1e-3, sample_weight=None, mask=None, max_iter=200, gtol=1e-6, ops=None):
    """Fit the probe on the rows of ``x`` (n, F) fp32 on the device, read where they lie (a row or column slice of a wider tensor
    is not copied).  y: n integer labels in [0, n_classes); mask: n booleans selecting the training rows (the others enter every
    launch with label -1 and come out as exact zeros: no copy of x); sample_weight: n finite values >= 0.  See the module
    docstring for the objective; returns a ``LinearProbe``.  TypeError for a host tensor or a wrong dtype; ValueError for shape
    mismatches, a class with no training row and an l2 that is not finite and > 0.
    ops: ``device_ops(x, n_classes)`` of these rows, to share its buffers between several fits (``cross_validated`` does)."""
    x, ldx = _rows(x, "x")
    n, F = x.shape
    y = _labels(y, n)
    mask = _host_vector(mask, n, "mask", np.bool_)
    sample_weight = _host_vector(sample_weight, n, "sample_weight", np.float64)
    if int(n_classes) < 1:
        raise ValueError("n_classes must be >= 1")
    if n < 1:
        raise ValueError("no training rows")
    if ops is None:
        ops = _DeviceOps(x, ldx, int(n_classes))
    elif ops.x.data_ptr() != x.data_ptr() or (ops.n, ops.F, ops.ldx, ops.C) != (n, F, ldx, int(n_classes)):
        raise ValueError("ops was built for other rows or another number of classes")
    return fit_with_ops(ops, n, F, y, n_classes, l2, sample_weight, mask, max_iter, gtol)


def device_ops(x, n_classes):
    """the device buffers of ``fit`` on the rows of x, for ``fit(x, ..., ops=...)``"""
    x, ldx = _rows(x, "x")
    if int(n_classes) < 1 or x.shape[0] < 1:
        raise ValueError("device_ops needs at least one row and one class")
    return _DeviceOps(x, ldx, int(n_classes))


# ---------------------------------------------------------------------------------------------------------------- using a probe
def scores(probe, x):
    """(n, C) fp64 logits of the rows of x (n, F) fp32 on the device: rg_linear_scores_f64 with the probe's raw-coordinate W, b"""
    x, ldx = _rows(x, "x")
    if x.shape[1] != probe.W.shape[1]:
        raise ValueError("x has %d features, the probe was fitted on %d" % (x.shape[1], probe.W.shape[1]))
    n, F, C = x.shape[0], x.shape[1], probe.W.shape[0]
    z = torch.empty(n, C, dtype=torch.float64, device=x.device)
    params = torch.from_numpy(np.concatenate([probe.W.reshape(-1), probe.b]).astype(np.float64)).to(x.device)
    p = params.data_ptr()
    _abi.launch("rg_linear_scores_f64", x.device, x.data_ptr(), ldx, n, F, p, F, C, p + 8 * C * F, z.data_ptr(), C)
    return z


def predict(probe, x):
    """(n,) int64 host array: the class of the largest logit, ties going to the LOWER class (a row of NaN logits: class 0)"""
    z = scores(probe, x)
    C = z.shape[1]
    cls = torch.arange(C, device=z.device)[None, :].expand_as(z)
    first = torch.where(z == z.max(dim=1, keepdim=True).values, cls, torch.full_like(cls, C)).min(dim=1).values
    return torch.where(first == C, torch.zeros_like(first), first).cpu().numpy().astype(np.int64)


def confusion_matrix(pred, y, n_classes):
    """(C, C) int64: entry [t][p] counts the rows of true class t predicted as p"""
    pred, y = np.asarray(pred).astype(np.int64), np.asarray(y).astype(np.int64)
    if pred.shape != y.shape or pred.ndim != 1:
        raise ValueError("pred and y must be two vectors of one length")
    C = int(n_classes)
    if pred.size and (min(pred.min(), y.min()) < 0 or max(pred.max(), y.max()) >= C):
        raise ValueError("a label lies outside [0, %d)" % C)
    return np.bincount(y * C + pred, minlength=C * C).reshape(C, C)


def accuracy(pred, y):
    pred, y = np.asarray(pred), np.asarray(y)
    if pred.shape != y.shape or pred.ndim != 1 or pred.size < 1:
        raise ValueError("pred and y must be two non-empty vectors of one length")
    return float(np.mean(pred == y))


def balanced_accuracy(pred, y, n_classes):
    """the mean over the classes PRESENT in y of the per-class recall"""
    cm = confusion_matrix(pred, y, n_classes)
    support = cm.sum(axis=1)
    if not support.any():
        raise ValueError("pred and y must be non-empty")
    return float(np.mean(np.diag(cm)[support > 0] / support[support > 0]))


def weighted_f1(pred, y, n_classes):
    """sklearn's f1_score(average="weighted"): the per-class F1 averaged with the class supports as weights"""
    cm = confusion_matrix(pred, y, n_classes).astype(np.float64)
    tp, support, called = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    denom = support + called
    f1 = np.where(denom > 0, 2.0 * tp / np.where(denom > 0, denom, 1.0), 0.0)
    return float(np.sum(f1 * support) / support.sum())


def stratified_folds(y, folds, seed=0):
    """(n,) int64 fold index per row.  Counter-based: ONE ``default_rng([seed, 0xC257])``; the classes are taken in ascending
    order, the rows of a class are permuted by ``rng.permutation`` and dealt round-robin to the folds.  ValueError for fewer rows
    of a class than folds."""
    y = np.asarray(y)
    folds = int(folds)
    if folds < 2:
        raise ValueError("folds must be >= 2")
    rng = np.random.default_rng([int(seed), FOLD_STREAM])
    fold = np.empty(y.shape[0], dtype=np.int64)
    for c in np.unique(y):
        idx = np.nonzero(y == c)[0]
        if idx.size < folds:
            raise ValueError("class %d has %d rows, fewer than the %d folds" % (int(c), idx.size, folds))
        fold[idx[rng.permutation(idx.size)]] = np.arange(idx.size) % folds
    return fold


def row_tissues(labels, row_of, n_rows, folds=None):
    """The tissue of every expression row from the labels of its tiles: ``(classes, tile_label, row_label)`` -- the distinct
    label codes in ascending order, every tile's label and every row's label as indices into them (host int64).  A row's tissue
    is the label of its tiles.  ValueError for ids outside the rows, a row without a tile, a row whose tiles disagree, fewer than
    two distinct tissues and -- with ``folds`` -- a tissue with fewer tiles than folds."""
    P = int(n_rows)
    lab = _labels(labels, len(labels), "labels")
    rows = _labels(row_of, lab.shape[0], "row_of")
    if lab.size == 0 or rows.min() < 0 or rows.max() >= P:
        raise ValueError("row_of points outside the %d expression rows" % P)
    classes, lab = np.unique(lab, return_inverse=True)
    if classes.size < 2:
        raise ValueError("the tiles carry %d distinct tissue(s): a tissue probe needs at least two" % classes.size)
    row_label = np.full(P, -1, dtype=np.int64)
    row_label[rows] = lab
    if (row_label < 0).any():
        raise ValueError("every expression row needs at least one tile (its tissue is the label of its tiles)")
    if (row_label[rows] != lab).any():
        raise ValueError("the tiles of expression row %d carry different tissue labels" % int(rows[np.argmax(row_label[rows] != lab)]))
    if folds is not None and np.bincount(lab).min() < int(folds):
        raise ValueError("a tissue has %d tiles, fewer than the %d folds" % (int(np.bincount(lab).min()), int(folds)))
    return classes, lab.astype(np.int64), row_label


def cross_validated(x, y, n_classes, folds=5, seed=0, l2=1e-3, extra=None, **fit_args):
    """held-out predictions of every row of x: one fit per fold on the other folds (rows held out by mask, x never copied).
    extra = (x2, y2): rows added to EVERY training fold and never tested (x is then concatenated with them once).
    Returns (pred (n,) int64, fold (n,) int64, iterations per fold)."""
    x, _ = _rows(x, "x")
    n = x.shape[0]
    y = _labels(y, n)
    fold = stratified_folds(y, folds, seed)
    xa, ya = x, y
    if extra is not None:
        x2, _ = _rows(extra[0], "extra x")
        if x2.shape[1] != x.shape[1] or x2.device != x.device:
            raise ValueError("the extra rows are %s on %s, x is %s on %s" % (tuple(x2.shape), x2.device, tuple(x.shape), x.device))
        xa, ya = torch.cat([x, x2]), np.concatenate([y, _labels(extra[1], x2.shape[0], "extra y")])
    pred = np.empty(n, dtype=np.int64)
    iters = []
    ops = device_ops(xa, n_classes)                          # one set of buffers for all folds
    for k in range(int(folds)):
        train = np.ones(xa.shape[0], dtype=bool)
        train[:n] = fold != k
        probe = fit(ops.x, ya, n_classes, l2=l2, mask=train, ops=ops, **fit_args)
        iters.append(probe.n_iter)
        held = np.nonzero(fold == k)[0]                      # only the held-out rows are scored (gathered once: n rows over all folds)
        pred[held] = predict(probe, x.index_select(0, torch.from_numpy(held).to(x.device)))
    return pred, fold, iters


def c2st(real_feats, fake_feats, folds=5, seed=0, l2=1e-3):
    """Classifier two-sample test between two (n, F) fp32 device feature sets: {"accuracy" (pooled over all held-out
    predictions), "balanced_accuracy", "per_fold" (held-out accuracy of each fold), "n_iter" (L-BFGS iterations per fold)}.
    Label 0 = real, 1 = generated; folds by ``stratified_folds``."""
    real_feats, _ = _rows(real_feats, "real_feats")
    fake_feats, _ = _rows(fake_feats, "fake_feats")
    if real_feats.shape[1] != fake_feats.shape[1] or real_feats.device != fake_feats.device:
        raise ValueError("real_feats is %s on %s, fake_feats is %s on %s" % (tuple(real_feats.shape), real_feats.device,
                                                                            tuple(fake_feats.shape), fake_feats.device))
    x = torch.cat([real_feats, fake_feats])
    y = np.concatenate([np.zeros(real_feats.shape[0], dtype=np.int64), np.ones(fake_feats.shape[0], dtype=np.int64)])
    pred, fold, iters = cross_validated(x, y, 2, folds, seed, l2)
    return {"accuracy": accuracy(pred, y), "balanced_accuracy": balanced_accuracy(pred, y, 2),
            "per_fold": [accuracy(pred[fold == k], y[fold == k]) for k in range(int(folds))], "n_iter": iters}


def tstr(fake_feats, fake_labels, real_feats, real_labels, n_classes, folds=5, seed=0, l2=1e-3):
    """Train on synthetic, test on real.  "tstr": a probe fitted on ALL generated rows, tested on ALL real rows; "trtr": the probe
    cross-validated on the real rows (``stratified_folds``); "ratio" = tstr / trtr.  Also "tstr_balanced", "trtr_balanced",
    "tstr_confusion", "trtr_confusion" ((C, C) lists, [true][predicted], over the real rows) and "n_iter"."""
    fake_feats, _ = _rows(fake_feats, "fake_feats")
    real_feats, _ = _rows(real_feats, "real_feats")
    if real_feats.shape[1] != fake_feats.shape[1] or real_feats.device != fake_feats.device:
        raise ValueError("real_feats is %s on %s, fake_feats is %s on %s" % (tuple(real_feats.shape), real_feats.device,
                                                                            tuple(fake_feats.shape), fake_feats.device))
    C = int(n_classes)
    yf, yr = _labels(fake_labels, fake_feats.shape[0], "fake_labels"), _labels(real_labels, real_feats.shape[0], "real_labels")
    if yr.size and (yr.min() < 0 or yr.max() >= C):
        raise ValueError("a real label lies outside [0, %d)" % C)
    probe = fit(fake_feats, yf, C, l2=l2)
    p_syn = predict(probe, real_feats)
    p_real, _, iters = cross_validated(real_feats, yr, C, folds, seed, l2)
    a_syn, a_real = accuracy(p_syn, yr), accuracy(p_real, yr)
    return {"tstr": a_syn, "trtr": a_real, "ratio": a_syn / a_real if a_real > 0 else float("inf"),
            "tstr_balanced": balanced_accuracy(p_syn, yr, C), "trtr_balanced": balanced_accuracy(p_real, yr, C),
            "tstr_confusion": confusion_matrix(p_syn, yr, C).tolist(), "trtr_confusion": confusion_matrix(p_real, yr, C).tolist(),
            "n_iter": [probe.n_iter] + iters}
