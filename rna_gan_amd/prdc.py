"""Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between two sets of
feature vectors, evaluated on the device.

X is the real set (m rows), Y the generated set (n rows), d2(a, b) = sum_f (a_f - b_f)^2.  The radius of row i of a set A is
r2_A[i] = the k-th smallest of { d2(a_i, a_j) : j != i } (row i excluded by INDEX: a duplicate row counts, a radius can be 0);
b_s *hits* a_r when d2(a_r, b_s) <= r2_B[s].  Then

    precision = (1 / n)     #{ j : some x_i hits y_j }            (generated rows inside the real manifold: fidelity)
    density   = (1 / (k n)) sum_j #{ i : x_i hits y_j }           (its outlier-robust sibling; can exceed 1)
    recall    = (1 / m)     #{ i : some y_j hits x_i }            (real rows inside the generated manifold: diversity)
    coverage  = (1 / m)     #{ i : min_j d2(x_i, y_j) <= r2_X[i] }

The comparison is ``<=`` on squared distances, as in the original precision / recall code, with no square root anywhere (the
``prdc`` package compares with ``<``; the two differ only on exact ties).  Radii and hits are rg_knn_radii2 and rg_radius_hits
(include/rnagan_hip.h): all-pairs fp64 distances in the direct form, never the m x n matrix in memory; a call of ``prdc`` is
four launch pairs, a few reductions over length-m / length-n vectors on the device and one download of four numbers.

The reference (src/fid.py) has no such metric; the definitions are pinned against an fp64 numpy restatement under tests/.
"""
from __future__ import annotations

import torch

from . import _abi
from .kid import _row_pair, _rows

KMAX = 16
_WS = {}            # device -> the cached workspace (one uint8 buffer per device, grown on demand)


def _workspace(device, nbytes):
    key = _abi.device_key(device)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    return ws


def _check_k(k, n, what):
    k = int(k)
    if not 1 <= k <= KMAX:
        raise ValueError("k must be in 1..%d, got %d" % (KMAX, k))
    if n < k + 1:
        raise ValueError("%s has %d rows: k = %d needs at least %d" % (what, n, k, k + 1))
    return k


def knn_radii2(x, k):
    """(n,) fp64 device tensor of the SQUARED k-th nearest-neighbour radii of the rows of x (n, F) fp32 on the device: the k-th
    smallest squared distance to the OTHER rows (by index).  1 <= k <= 16, n >= k + 1.  Rows are read where they lie."""
    x, ldx = _rows(x, "x")
    n, F = x.shape
    k = _check_k(k, n, "x")
    ws = _workspace(x.device, _abi.load().rg_pairdist_ws_bytes(n, n, k))
    r2 = torch.empty(n, dtype=torch.float64, device=x.device)
    _abi.launch("rg_knn_radii2", x.device, x.data_ptr(), ldx, n, F, k, ws.data_ptr(), ws.numel(), r2.data_ptr())
    return r2


def radius_hits(a, b, rb2=None):
    """``(count, mind2)`` for the rows of a (na, F) against the rows of b (nb, F), fp32 on one device: count[r] (int32) =
    #{ s : d2(a_r, b_s) <= rb2[s] } with rb2 the (nb,) fp64 squared radii of b's rows, mind2[r] (fp64) = min_s d2(a_r, b_s).
    rb2=None: count is None, only the minima are computed.  Rows are read where they lie."""
    a, lda, b, ldb = _row_pair(a, b)
    na, nb, F = a.shape[0], b.shape[0], a.shape[1]
    if na < 1 or nb < 1:
        raise ValueError("radius_hits needs at least one row in each set, got %d and %d" % (na, nb))
    if rb2 is not None:
        if not (torch.is_tensor(rb2) and rb2.dtype == torch.float64 and rb2.device == a.device and rb2.shape == (nb,)):
            raise ValueError("rb2 must be an (nb,) float64 tensor on the device of a and b")
        rb2 = rb2.contiguous()
    ws = _workspace(a.device, _abi.load().rg_pairdist_ws_bytes(na, nb, 0))
    count = None if rb2 is None else torch.empty(na, dtype=torch.int32, device=a.device)
    mind2 = torch.empty(na, dtype=torch.float64, device=a.device)
    _abi.launch("rg_radius_hits", a.device, a.data_ptr(), lda, na, b.data_ptr(), ldb, nb, F, None if rb2 is None else rb2.data_ptr(),
                ws.data_ptr(), ws.numel(), None if count is None else count.data_ptr(), mind2.data_ptr())
    return count, mind2


def prdc(real_feats, fake_feats, k=5, real_radii2=None):
    """{"precision", "recall", "density", "coverage"} (Python floats) of the (m, F) real and (n, F) generated fp32 device feature
    sets at neighbourhood size k.  Four launch pairs -- radii of the real set (skipped when ``real_radii2``, an earlier
    ``knn_radii2(real_feats, k)``, is passed in), radii of the generated set, the generated rows in the real balls, the real rows
    in the generated balls (whose minima give coverage) -- then reductions over length-m / length-n vectors on the device and
    ONE download of the four values.  Comparisons are ``<=`` on squared distances (see the module docstring on ties)."""
    x, _, y, _ = _row_pair(real_feats, fake_feats, ("real_feats", "fake_feats"))
    m, n = x.shape[0], y.shape[0]
    k = _check_k(k, min(m, n), "the smaller set")
    if real_radii2 is None:
        rx2 = knn_radii2(x, k)
    else:
        rx2 = real_radii2
        if not (torch.is_tensor(rx2) and rx2.dtype == torch.float64 and rx2.device == x.device and rx2.shape == (m,)):
            raise ValueError("real_radii2 must be knn_radii2(real_feats, k): an (m,) float64 tensor on the features' device")
    ry2 = knn_radii2(y, k)
    in_real, _ = radius_hits(y, x, rx2)               # per generated row: the number of real balls it lies in
    in_fake, nearest = radius_hits(x, y, ry2)         # per real row: the number of generated balls, the nearest generated row
    # four integer totals come back; each ratio is ONE correctly rounded host division (a device division by a scalar may be
    # a multiplication by its reciprocal)
    inside, covering, balls, covered = torch.stack([(in_real > 0).sum(), (in_fake > 0).sum(), in_real.sum(dtype=torch.int64),
                                                    (nearest <= rx2).sum()]).cpu().tolist()
    return {"precision": inside / float(n), "recall": covering / float(m), "density": balls / (float(k) * n),
            "coverage": covered / float(m)}


def precision_recall(real_feats, fake_feats, k=3):
    """(precision, recall) at the neighbourhood size of Kynkaanniemi et al. (k = 3)"""
    out = prdc(real_feats, fake_feats, k)
    return out["precision"], out["recall"]


def density_coverage(real_feats, fake_feats, k=5):
    """(density, coverage) at the neighbourhood size of Naeem et al. (k = 5)"""
    out = prdc(real_feats, fake_feats, k)
    return out["density"], out["coverage"]


def calculate_prdc(images1, images2, feature_extractor, batch_size=2, device=None, **kwargs):
    """Counterpart of kid.calculate_kid: images (N, H, W, 3) uint8 / float in [0, 1] are uploaded once, resized to 299 and
    extracted on the device (``feature_extractor`` returns device tensors, e.g. fid.inception_features_device); images1 is the
    real set.  Returns prdc(features1, features2, **kwargs)."""
    from .fid import device_feature_pair
    return prdc(*device_feature_pair(images1, images2, feature_extractor, batch_size, device), **kwargs)
