"""Timings of the linear-probe scores (rna_gan_amd.linprobe, rg_linprobe.hip) on one MI355X: one C2ST and one TSTR evaluation
against the same optimiser on downloaded features in vectorised numpy, one evaluation of loss and gradient, and the three kernels
against the time to stream their bytes at the copy rate of the same process.  ``--json PATH`` writes the result
(profiles/linprobe.json); it is printed either way.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rna_gan_amd import _abi, linprobe as LP  # noqa: E402

DEV = torch.device("cuda:0")


class HostOps:
    """the fit's three operations in vectorised numpy fp64 on downloaded features (BLAS matrix products)"""

    def __init__(self, x):
        self.x = x.astype(np.float64)

    def moments(self, m):
        return m @ self.x, m @ (self.x * self.x)

    def set_rows(self, label, weight):
        self.label, self.weight = label, weight

    def evaluate(self, W, b):
        label, weight = self.label, self.weight
        z = self.x @ W.T + b
        z -= z.max(axis=1, keepdims=True)
        e = np.exp(z)
        s = e.sum(axis=1)
        ok = label >= 0
        y = np.where(ok, label, 0)
        wt = (np.ones(len(y)) if weight is None else weight) * ok
        r = e / s[:, None]
        r[np.arange(len(y)), y] -= 1.0
        r *= wt[:, None]
        loss = float((wt * (np.log(s) - z[np.arange(len(y)), y])).sum())
        return r.T @ self.x, r.sum(axis=0), loss


def host_cv(x, y, C, folds, seed, l2, extra=None):
    fold = LP.stratified_folds(y, folds, seed)
    xa, ya = (x, y) if extra is None else (np.concatenate([x, extra[0]]), np.concatenate([y, extra[1]]))
    ops = HostOps(xa)
    pred = np.empty(len(y), dtype=np.int64)
    iters = []
    for k in range(folds):
        train = np.ones(len(ya), dtype=bool)
        train[:len(y)] = fold != k
        p = LP.fit_with_ops(ops, xa.shape[0], xa.shape[1], ya, C, l2, None, train)
        iters.append(p.n_iter)
        held = fold == k
        pred[held] = (x[held].astype(np.float64) @ p.W.T + p.b).argmax(axis=1)
    return pred, iters


def timed(fn, repeat=3):
    fn()                                                     # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def events(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--json", type=str, default=None, help="write the result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_linprobe.py measures on the GPU: none found")
    out = {"device": torch.cuda.get_device_name(0), "note": "seconds; host clock around synchronised work (evaluations), device "
           "events over 50 back-to-back calls (kernels); median of 3 after a warm-up (min, max kept)"}
    F = 2048                                                 # the trunk width of the reference-size critic
    rng = np.random.default_rng([11, 0])
    real = rng.standard_normal((2048, F)).astype(np.float32)
    fake = rng.standard_normal((2048, F)).astype(np.float32)
    fake[:, :64] += 0.25
    rd, fd = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    # ---- one C2ST evaluation, 2048 + 2048 rows, 5 folds
    med, lo, hi, res = timed(lambda: LP.c2st(rd, fd, 5, 0, 1e-3))

    def host_c2st():
        x = np.concatenate([rd.cpu().numpy(), fd.cpu().numpy()])       # the download is part of the host path
        y = np.concatenate([np.zeros(2048, dtype=np.int64), np.ones(2048, dtype=np.int64)])
        pred, iters = host_cv(x, y, 2, 5, 0, 1e-3)
        return {"accuracy": float(np.mean(pred == y)), "n_iter": iters}
    hmed, hlo, hhi, hres = timed(host_c2st)
    out["c2st_2048x2048_F2048_5fold"] = {"device_s": med, "device_min_max": [lo, hi], "host_s": hmed, "host_min_max": [hlo, hhi],
                                         "device": res, "host": hres}
    # one objective evaluation of that problem, and its parts
    x = torch.cat([rd, fd])
    ops = LP.device_ops(x, 2)
    label = np.concatenate([np.zeros(2048), np.ones(2048)]).astype(np.int32)
    W, b = rng.standard_normal((2, F)) * 0.01, np.zeros(2)
    ops.set_rows(label, None)
    ev = timed(lambda: ops.evaluate(W, b), 20)
    out["one_evaluation_n4096_F2048_C2_s"] = {"median": ev[0], "min": ev[1], "max": ev[2],
                                              "launches": 8, "uploads": 1, "downloads": 1}
    # ---- one TSTR evaluation, 64 rows x 32 tiles, two tissues
    yr = (np.arange(2048) % 64 % 2).astype(np.int64)
    real2 = real.copy(); real2[yr == 1, :32] += 0.5
    fake2 = fake.copy(); fake2[yr == 1, :32] += 0.4
    r2, f2 = torch.from_numpy(real2).to(DEV), torch.from_numpy(fake2).to(DEV)
    med, lo, hi, res = timed(lambda: LP.tstr(f2, yr, r2, yr, 2, 5, 0, 1e-3))

    def host_tstr():
        xr, xf = r2.cpu().numpy(), f2.cpu().numpy()
        p = LP.fit_with_ops(HostOps(xf), 2048, F, yr, 2, 1e-3)
        a = float(np.mean((xr.astype(np.float64) @ p.W.T + p.b).argmax(axis=1) == yr))
        pred, iters = host_cv(xr, yr, 2, 5, 0, 1e-3)
        return {"tstr": a, "trtr": float(np.mean(pred == yr)), "n_iter": [p.n_iter] + iters}
    hmed, hlo, hhi, hres = timed(host_tstr)
    res = {k: res[k] for k in ("tstr", "trtr", "ratio", "n_iter")}
    out["tstr_64rows_x32tiles_F2048"] = {"device_s": med, "device_min_max": [lo, hi], "host_s": hmed, "host_min_max": [hlo, hhi],
                                         "device": res, "host": hres}
    # ---- the kernels alone, n = 4096, F = 2048, against the copy rate of this process
    lib = _abi.load()
    n = 4096
    big = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(big)
    t = events(lambda: dst.copy_(big), 20)
    copy_rate = 2 * big.numel() / t                           # bytes read + bytes written per second
    out["copy_rate_GBps"] = copy_rate / 1e9
    st = torch.cuda.current_stream().cuda_stream
    kern = {}
    for C in (2, 8):
        w = torch.randn(C, F, dtype=torch.float64, device=DEV)
        bias = torch.zeros(C, dtype=torch.float64, device=DEV)
        z = torch.empty(n, C, dtype=torch.float64, device=DEV)
        resid, loss = torch.empty_like(z), torch.empty(n, dtype=torch.float64, device=DEV)
        lab = torch.from_numpy((np.arange(n) % C).astype(np.int32)).to(DEV)
        need = lib.rg_colsums_ws_bytes(n, F, C)
        ws, g = torch.empty(need // 8, dtype=torch.float64, device=DEV), torch.empty(C, F, dtype=torch.float64, device=DEV)
        t_sc = events(lambda: lib.rg_linear_scores_f64(x.data_ptr(), F, n, F, w.data_ptr(), F, C, bias.data_ptr(), z.data_ptr(), C, st))
        t_rs = events(lambda: lib.rg_softmax_residual_f64(z.data_ptr(), C, n, C, lab.data_ptr(), None, resid.data_ptr(), C,
                                                          loss.data_ptr(), st))
        t_cs = events(lambda: lib.rg_rows_weighted_colsums_f64(x.data_ptr(), F, n, F, resid.data_ptr(), C, C, 1, ws.data_ptr(), need,
                                                               g.data_ptr(), st))
        b_sc = n * F * 4 + C * F * 8 + n * C * 8
        b_rs = 2 * n * C * 8 + n * 12
        b_cs = n * F * 4 + n * C * 8 + 2 * (n // 256) * C * F * 8 + C * F * 8
        kern["C%d" % C] = {
            "linear_scores": {"s": t_sc, "bytes": b_sc, "stream_s": b_sc / copy_rate, "fma": n * F * C},
            "softmax_residual": {"s": t_rs, "bytes": b_rs, "stream_s": b_rs / copy_rate},
            "colsums_two_launches": {"s": t_cs, "bytes": b_cs, "stream_s": b_cs / copy_rate, "fma": n * F * C}}
    out["kernels_n4096_F2048"] = kern
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
