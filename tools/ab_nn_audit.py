#!/usr/bin/env python3
"""The memorisation audit (rg_nn.hip, rna_gan_amd.nearest, metrics.Memorisation) measured on one device.

    python tools/ab_nn_audit.py [--queries 2048 --refs 65536 --size 256 --factor 4] [--json profiles/nn_audit.json]

Sections:
  descriptor  rg_tile_descriptor_i8 on --desc_tiles uint8 tiles [3][--size][--size] (sets rotated beyond the 256 MiB Infinity Cache):
              device events around --reps back-to-back calls, median over --rounds; next to it the time to move its bytes (the
              tiles read, the descriptors and norms written) at the stream-copy rate measured in this process.
  topk        rg_nn_topk_i8, --queries x --refs random int8 descriptors of D = 3 (size / factor)^2 bytes, k = 4: one call per
              round behind one warm-up call.  Yardsticks: (a) the same search with torch -- fp32 matmul over chunks of --chunk
              reference rows (the fp32 copies of both operands made BEFORE the clock starts), d2 from the norms, torch.topk per
              chunk and over the chunks' winners; a TIMING yardstick only, fp32 is not exact at these magnitudes (how many of
              its nearest rows differ is reported); (b) twice the bf16 MFMA ceiling of rna_gan_amd.probe.
  metric      metrics.Memorisation at --queries samples end to end (generate, export, descriptors, search under the 8 symmetries,
              leave-one-out search, host arithmetic) against --refs resident training tiles, next to TissueYield and
              KernelDistance on the same seeded generator in the same run; the index build is timed apart (it happens once).
  clock       the device's current and maximum engine clock as torch reports them, before and after.
Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


def event_ms(fn, reps, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def stats(v, digits=3):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def clock(device):
    try:
        return {"mhz": torch.cuda.clock_rate(device)}
    except Exception as e:                                    # noqa: BLE001 -- a report, not a product path
        return {"mhz": None, "why": str(e)[:80]}


def descriptor_section(device, N, S, f, reps, rounds):
    from rna_gan_amd import _abi, nearest as NN
    lib = _abi.load()
    D, ldd = NN.descriptor_shape(3, S, f)
    sets = max(2, -(-(320 << 20) // (N * 3 * S * S)) + 1)
    g = torch.Generator(device=device).manual_seed(1)
    data = [torch.randint(0, 256, (N, 3, S, S), dtype=torch.uint8, device=device, generator=g) for _ in range(sets)]
    desc = torch.empty((N, ldd), dtype=torch.int8, device=device)
    norm2 = torch.empty((N,), dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    k = [0]

    def call():
        k[0] += 1
        _abi.check(lib.rg_tile_descriptor_i8(data[k[0] % sets].data_ptr(), N, 3, S, f, desc.data_ptr(), ldd, norm2.data_ptr(), st), "desc")
    for _ in range(sets):
        call()
    got = NN.descriptors(data[0][:8].cpu(), f)
    call_d = NN.descriptors(data[0][:8], f)
    assert torch.equal(got[0], call_d[0].cpu()) and torch.equal(got[1], call_d[1].cpu()), "device and CPU descriptors differ"
    t = [event_ms(call, reps, device) * 1e3 for _ in range(rounds)]
    moved = N * 3 * S * S + N * ldd + N * 4
    return dict(stats(t, 2), unit="us per call (device events over %d back-to-back calls, %d rounds)" % (reps, rounds), tiles=N, size=S,
                factor=f, D=D, ldd=ldd, bytes_moved=moved, buffer_sets=sets)


def torch_search(a32, na, b32, nb, k, chunk):
    """the yardstick: (d2 fp32 [Q][k], index int64 [Q][k])"""
    best_d, best_i = None, None
    for r0 in range(0, b32.shape[0], chunk):
        d2 = na[:, None] + nb[None, r0:r0 + chunk] - 2.0 * (a32 @ b32[r0:r0 + chunk].t())
        d, i = torch.topk(d2, k, dim=1, largest=False, sorted=True)
        i = i + r0
        if best_d is None:
            best_d, best_i = d, i
        else:
            d, j = torch.topk(torch.cat([best_d, d], dim=1), k, dim=1, largest=False, sorted=True)
            best_d, best_i = d, torch.cat([best_i, i], dim=1).gather(1, j)
    return best_d, best_i


def topk_section(device, Q, N, D, k, chunk, rounds):
    from rna_gan_amd import nearest as NN
    g = torch.Generator(device=device).manual_seed(2)
    a = torch.randint(-128, 128, (Q, D), dtype=torch.int8, device=device, generator=g)
    b = torch.randint(-128, 128, (N, D), dtype=torch.int8, device=device, generator=g)
    na = (a.to(torch.int32) ** 2).sum(dim=1, dtype=torch.int32)
    nb = torch.cat([(b[i:i + 4096].to(torch.int32) ** 2).sum(dim=1, dtype=torch.int32) for i in range(0, N, 4096)])
    res = {"queries": Q, "refs": N, "D": D, "k": k, "multiply_adds": Q * N * D,
           "unit": "ms per search (device events, one call per round behind one warm-up call, %d rounds)" % rounds}
    out = {}

    def ours():
        out["ours"] = NN.nearest((a, na), (b, nb), k)
    ours()
    t = [event_ms(ours, 1, device) for _ in range(rounds)]
    res["rg_nn_topk_i8"] = dict(stats(t), tops=round(2.0 * Q * N * D / (statistics.median(t) * 1e-3) / 1e12, 1))
    # exactness of the kernel on a slice, against integer torch ops on the device
    qs = slice(0, min(Q, 64))
    a64, keys = a[qs].double(), None
    for r0 in range(0, N, chunk):                             # fp64 holds these integers exactly
        d2 = na[qs].long()[:, None] + nb[r0:r0 + chunk].long()[None, :] - 2 * (a64 @ b[r0:r0 + chunk].double().t()).long()
        part = (d2 << 32) | torch.arange(r0, min(r0 + chunk, N), device=device)[None, :]
        keys = torch.topk(part if keys is None else torch.cat([keys, part], dim=1), k, dim=1, largest=False, sorted=True).values
    assert torch.equal(keys >> 32, out["ours"][0][qs]) and torch.equal(keys & 0xffffffff, out["ours"][1][qs]), "kernel and fp64 torch differ"
    res["checked"] = "the first %d queries equal an fp64 torch search key for key" % (qs.stop,)
    del a64, keys, d2, part
    try:
        a32, b32 = a.float(), b.float()
        na32, nb32 = na.float(), nb.float()

        def theirs():
            out["torch"] = torch_search(a32, na32, b32, nb32, k, chunk)
        theirs()
        t2 = [event_ms(theirs, 1, device) for _ in range(rounds)]
        res["torch_fp32"] = dict(stats(t2), chunk=chunk, tflops=round(2.0 * Q * N * D / (statistics.median(t2) * 1e-3) / 1e12, 1),
                                 nearest_rows_that_differ=int((out["torch"][1][:, 0] != out["ours"][1][:, 0]).sum()),
                                 what="fp32 matmul + topk over chunks of reference rows; fp32 copies made before the clock starts")
        res["torch_over_kernel"] = round(statistics.median(t2) / statistics.median(t), 2)
        del a32, b32
    except Exception as e:                                    # noqa: BLE001
        res["torch_fp32"] = {"unavailable": str(e)[:200]}
    return res


def metric_section(device, samples, refs, S, f, rounds):
    import rna_gan_amd as P
    from rna_gan_amd import synth
    from rna_gan_amd.metrics import KernelDistance, Memorisation, TissueYield
    from rna_gan_amd.nearest import TrainIndex
    G = P.DCGANGenerator(2048, S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
    Dn = P.DCGANDiscriminator(S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2))
    synth.seeded_fill_(G, 5)
    synth.seeded_fill_(Dn, 6)
    G, Dn = G.set_precision("bf16").to(device), Dn.set_precision("bf16").to(device)
    g = torch.Generator(device=device).manual_seed(3)
    train = torch.cat([torch.randint(0, 256, (min(4096, refs - i), 3, S, S), dtype=torch.uint8, device=device, generator=g)
                       for i in range(0, refs, 4096)])
    res = {"samples": samples, "train_tiles": refs, "size": S, "factor": f,
           "unit": "ms per evaluation (host clock around metric_ops with a device synchronisation, one warm-up, %d rounds)" % rounds}

    def timed(fn):
        fn()
        t = []
        for _ in range(rounds):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(device)
            t.append((time.perf_counter() - t0) * 1e3)
        return stats(t, 1)
    res["index_build"] = timed(lambda: TrainIndex(train, factor=f))
    for name, d4 in (("memorisation_d4", True), ("memorisation_plain", False)):
        m = Memorisation(train, samples, factor=f, k=1, d4=d4, seed=1)
        res[name] = dict(timed(lambda: m.metric_ops(G, device)), last=m.last)      # (the warm-up builds and keeps the index)
        print("[ab_nn_audit] %s %s" % (name, json.dumps(res[name])), file=sys.stderr, flush=True)
    ty = TissueYield(samples, seed=1)
    res["tissue_yield"] = timed(lambda: ty.metric_ops(G, device))
    kd = KernelDistance(train[:samples], extractor="discriminator", seed=1)
    res["kernel_distance"] = timed(lambda: kd.metric_ops(G, Dn, device))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--refs", type=int, default=65536)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--desc_tiles", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sections", default="descriptor,topk,probe,metric")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    from rna_gan_amd.nearest import descriptor_shape
    D, ldd = descriptor_shape(3, a.size, a.factor)
    sections = a.sections.split(",")
    res = {"what": "memorisation audit on one device; sections run one after another in one process",
           "device": torch.cuda.get_device_name(device), "clock_before": clock(device)}
    if "descriptor" in sections:
        res["descriptor"] = descriptor_section(device, a.desc_tiles, a.size, a.factor, a.reps, a.rounds)
        torch.cuda.empty_cache()
        print("[ab_nn_audit] descriptor %s" % json.dumps(res["descriptor"]), file=sys.stderr, flush=True)
    if "topk" in sections:
        res["topk"] = topk_section(device, a.queries, a.refs, ldd, a.k, a.chunk, min(a.rounds, 3))
        torch.cuda.empty_cache()
        print("[ab_nn_audit] topk %s" % json.dumps(res["topk"]), file=sys.stderr, flush=True)
    if "probe" in sections:
        from rna_gan_amd.probe import measure_ceilings
        c = measure_ceilings(device, settle_s=0.5, n_timed=4, copy_mb=1024)
        bf16 = max(v for n, v in c.items() if n.startswith("mfma_bare_"))
        res["probe"] = {"stream_copy_gbps": c["stream_copy_gbps"], "stream_copy_what": c["stream_copy_what"], "bf16_mfma_bare_tflops": bf16,
                        "i8_ceiling_tops": round(2 * bf16, 1), "protocol": c["protocol"]}
        if "descriptor" in res:
            d = res["descriptor"]
            d["us_at_copy_rate"] = round(d["bytes_moved"] / (c["stream_copy_gbps"] * 1e9) * 1e6, 2)
            d["over_copy_rate"] = round(d["median"] / d["us_at_copy_rate"], 2)
        if "topk" in res:
            res["topk"]["rg_nn_topk_i8"]["share_of_i8_ceiling"] = round(res["topk"]["rg_nn_topk_i8"]["tops"] / (2 * bf16), 3)
        print("[ab_nn_audit] probe %s" % json.dumps(res["probe"]), file=sys.stderr, flush=True)
    if "metric" in sections:
        res["metric"] = metric_section(device, a.queries, a.refs, a.size, a.factor, min(a.rounds, 3))
    res["clock_after"] = clock(device)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
