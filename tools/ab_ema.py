#!/usr/bin/env python3
"""Interleaved A/B of the benchmarked training iteration without and with the averaged generator (rna_gan_amd.ema.ParamEMA on
optimizer_generator: one rg_ema_update launch inside the generator's optimizer step), inside ONE process, with
tools/ab_step.py's timing scheme: every workload owns its models, optimizers, plug-ins and step graphs, the timed regions
alternate  off ema off#control  (order reversed every other round), and the EMA-off workload is built twice -- the difference
of the two identically configured copies is the noise floor a delta has to exceed.  bench.py is used as it stands
(bench.hip_workload; the average is attached to the optimizer it hands back).

    python tools/ab_ema.py --rounds 5 --steps 20 [--json profiles/g_ema_step.json]
    python tools/ab_ema.py --json profiles/g_ema_step.json --merge-trees out.json      (no measurement: see below)

Afterwards rg_ema_update alone is timed on the generator's flat buffer next to rg_adam_step_dev alone on the same buffer (both
pure fp32 streams with 16-byte accesses: 12 and 28 bytes per parameter; the product's bf16 step also writes the 2-byte shadow,
timed as a third row), with rna_gan_amd.probe's protocol and its stream-copy ceiling from the same process.
--merge-trees FILE: the EMA-off variant IS the code of the commit before the feature plus an untaken branch; the comparison with
that commit's own tree needs two builds and fresh processes, which is tools/ab_trees.py's job (--trees parent=<extracted parent
commit>,head=.).  This option puts that tool's result line into the --json file under "parent_tree_ab", next to this tool's A/A
noise floor, and does nothing else.
Nothing here is imported by the product or the tests.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402


def build(bench, bargs, device, decay, prime):
    step, flush, _, info = bench.hip_workload(bargs, 0, 1, device)
    ema = None
    if decay is not None:
        from rna_gan_amd.ema import ParamEMA
        h = info["handles"]
        ema = ParamEMA(h["G"], decay=decay, warmup=True)
        h["og"].attach_ema(ema)
    for _ in range(prime):
        step()
    torch.cuda.synchronize(device)
    return step, flush, info["handles"], ema


def kernel_bandwidth(device, handles, ema):
    """Achieved GB/s (bytes read + written) of the two streaming kernels on the generator's flat buffer.  Run after the A/B:
    the buffers' contents no longer matter (Adam keeps stepping from the last gradient)."""
    from rna_gan_amd import _abi, probe
    G, og = handles["G"], handles["og"]
    flat, twin = G.flat, ema.module.flat
    lib = G.runtime()[0].lib
    st = torch.cuda.current_stream(device).cuda_stream
    n = flat.numel
    p, g, m, v, e = flat.data.data_ptr(), flat.grad.data_ptr(), og._m.data_ptr(), og._v.data_ptr(), twin.data.data_ptr()
    hyper, step_dev = og._hyper.data_ptr(), og._step_dev.data_ptr()
    shadow = 0 if flat.shadow is None else flat.shadow.data_ptr()
    rows = []
    for name, launch, per in (
            ("rg_ema_update", lambda: _abi.check(lib.rg_ema_update(p, e, n, 0.999, step_dev, hyper, st), "rg_ema_update"), 12),
            ("rg_adam_step_dev", lambda: _abi.check(lib.rg_adam_step_dev(p, g, m, v, n, hyper, None, None, st), "rg_adam_step_dev"), 28),
            ("rg_adam_step_dev+shadow", (lambda: _abi.check(lib.rg_adam_step_dev(p, g, m, v, n, hyper, shadow, None, st),
                                                            "rg_adam_step_dev")) if shadow else None, 30)):
        if launch is None:
            continue
        ms = probe._timed(launch, 0.5, 32, device)
        rows.append({"kernel": name, "elements": n, "bytes_per_element": per, "us": round(ms * 1e3, 2),
                     "gbps": round(per * n / (ms * 1e-3) / 1e9, 1)})
    ceil = probe.measure_ceilings(device, settle_s=1.0)
    by = {r["kernel"]: r for r in rows}
    ratio = by["rg_ema_update"]["gbps"] / by["rg_adam_step_dev"]["gbps"]
    return {"kernels": rows, "ema_over_adam_gbps": round(ratio, 3), "within_15_percent": bool(ratio >= 0.85),
            "stream_copy_gbps": ceil["stream_copy_gbps"], "stream_copy_what": ceil["stream_copy_what"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prime", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge-trees", default=None)
    a = ap.parse_args()
    if a.merge_trees:
        res = json.loads(open(a.json).read())
        trees = json.loads(open(a.merge_trees).read())
        d = trees["trees"][1]["delta_vs_first"]["mean"]
        res["parent_tree_ab"] = dict(trees, tool="tools/ab_trees.py", head_minus_parent_ms=d,
                                     within_noise_floor=bool(abs(d) <= res["noise_floor_ms"]))
        with open(a.json, "w") as f:
            f.write(json.dumps(res) + "\n")
        return
    import bench
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    bargs = bench.parse_args(["--batch", str(a.batch), "--precision", a.precision, "--no-cpu-baseline", "--no-roofline", "--no-extras"])
    names = ["off", "ema", "off#control"]
    work, times, last = {}, {n: [] for n in names}, {}
    for n in names:
        t0 = time.perf_counter()
        work[n] = build(bench, bargs, device, a.decay if n == "ema" else None, a.prime)
        print("[ab_ema] built + primed %-12s in %.1f s" % (n, time.perf_counter() - t0), file=sys.stderr, flush=True)
    for r in range(a.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            step, flush = work[n][:2]
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ls = step()
            flush()
            torch.cuda.synchronize(device)
            times[n].append((time.perf_counter() - t0) / a.steps * 1e3)
            last[n] = [float(x.item()) for x in ls]
        print("[ab_ema] round %d: %s" % (r, "  ".join("%s %.3f" % (n, times[n][-1]) for n in names)), file=sys.stderr, flush=True)
    from rna_gan_amd.ops_hip import check_handoffs
    check_handoffs()
    res = {"what": "ms per training iteration (G-loss, D-loss, penalty train_ops), interleaved in one process", "batch": a.batch,
           "precision": a.precision, "steps": a.steps, "rounds": a.rounds, "decay": a.decay, "variants": []}
    for n in names:
        d = [x - y for x, y in zip(times[n], times["off"])]
        res["variants"].append({"name": n, "ms": [round(x, 3) for x in times[n]], "mean": round(sum(times[n]) / len(times[n]), 3),
                                "min": round(min(times[n]), 3), "delta_vs_off": {"mean": round(sum(d) / len(d), 3),
                                                                                 "min": round(min(d), 3), "max": round(max(d), 3)},
                                "losses_last_step": [round(x, 5) for x in last[n]]})
    res["noise_floor_ms"] = abs(res["variants"][2]["delta_vs_off"]["mean"])
    res["ema_minus_off_ms"] = res["variants"][1]["delta_vs_off"]["mean"]
    twin = work["ema"][3].module
    res["twin_finite"] = bool(torch.isfinite(twin.flat.data).all())
    res["kernel_bandwidth"] = kernel_bandwidth(device, work["ema"][2], work["ema"][3])
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
