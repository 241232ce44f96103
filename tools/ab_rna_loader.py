#!/usr/bin/env python3
"""The resident expression table (rg_rows_gather_f32, rna_gan_amd.rna_tables) measured on one device.

    python tools/ab_rna_loader.py [--batch 64 --features 19198] [--json profiles/rna_table_loader.json]

Sections:
  kernel   one batch [--batch][--features] gathered from a --table_rows x --features fp32 table (8 192 x 19 198 = 629 MB, larger
           than the 256 MiB Infinity Cache), device events around --reps back-to-back calls, every variant timed once per round,
           the order reversed every other round, (g) timed twice per round (the difference of its two identically configured
           timings is the run's noise floor):
             (g) rg_rows_gather_f32 into a dense [--batch][--features] destination
             (t) torch.index_select(rows, 0, idx, out=the same destination) on the same table
           The calls rotate over --sets index sets and destinations (64 x 64 rows = 314 MB of source rows and as much of
           destinations, so neither side is served from the cache).  Condition: (g) not slower than (t) by more than the noise
           floor; the two move the same bytes.
  train    train_betaVAE iterations per second: the reference-size model (19 198 -> [6000, 4000, 2048] -> 2048 -> [4000, 6000]),
           bf16, batch --batch, ONE model and optimizer for all variants, a synthetic --rows-row table written to two CSV files
           and read back through the real path (pandas read_csv, split_tables, RnaScaler), its train split as the epoch:
             host_w0    DataLoader(RNADataset), shuffle, drop_last, 0 workers
             host_w4    the same with 4 workers (the reference's setting; the workers start with every pass, as there)
             resident   RnaTableLoader over the table on the device
           A warm-up pass each, then --train_rounds interleaved timed passes of --epochs epochs (host clock around a pass that
           ends in a device synchronise; the validation phase is empty and torch.save is replaced by a no-op during the passes:
           a 1.1 GB checkpoint per pass is not what is being measured).  No ratio is demanded; the loop reads three scalars back
           per iteration, which bounds what any loader can win.
Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402


def event_us(fn, reps, device):
    """microseconds per call over `reps` back-to-back calls between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def interleave(variants, rounds, measure, tag):
    names = list(variants)
    out = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            out[n].append(measure(variants[n]))
        print("[ab_rna_loader] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)),
              file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--features", type=int, default=19198)
    ap.add_argument("--table_rows", type=int, default=8192, help="rows of the kernel section's table")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=4096, help="rows of the train section's CSV tables (two files of half each)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--train_rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    from rna_gan_amd import _abi
    from rna_gan_amd import rna_tables as RT
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    N, F = a.batch, a.features
    res = {"what": "resident expression table on one device; variants interleaved in one process", "batch": N, "features": F,
           "device": torch.cuda.get_device_name(device)}

    if "kernel" not in skip:
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        M = a.table_rows
        gen = torch.Generator(device=device).manual_seed(0)
        rows = torch.randn((M, F), dtype=torch.float32, device=device, generator=gen)
        rng = np.random.default_rng(0)
        index = [torch.from_numpy(rng.integers(0, M, size=N).astype(np.int32)).to(device) for _ in range(a.sets)]
        index64 = [i.long() for i in index]
        dsts = [torch.empty(N, F, dtype=torch.float32, device=device) for _ in range(a.sets)]
        k = [0]

        def nxt():
            k[0] += 1
            return k[0] % a.sets

        def gather():
            j = nxt()
            _abi.check(lib.rg_rows_gather_f32(rows.data_ptr(), M, F, F, index[j].data_ptr(), dsts[j].data_ptr(), N, F, st),
                       "rows_gather_f32")
            return dsts[j]

        def index_select():
            j = nxt()
            torch.index_select(rows, 0, index64[j], out=dsts[j])
            return dsts[j]

        variants = {"g_rows_gather": gather, "t_index_select": index_select, "g#control": gather}
        k[0] = 0
        y = gather().clone()
        k[0] = 0
        assert torch.equal(y.view(torch.int32), index_select().view(torch.int32)), "the kernel and index_select differ"
        for fn in variants.values():
            for _ in range(a.sets):
                fn()
        t = interleave(variants, a.rounds, lambda fn: event_us(fn, a.reps, device), "kernel us")
        kern = {n: stats(v) for n, v in t.items()}
        moved = 2 * N * F * 4
        for n in ("g_rows_gather", "t_index_select"):
            kern[n]["tb_per_s"] = round(moved / (kern[n]["median"] * 1e-6) / 1e12, 2)
        gm, tm = kern["g_rows_gather"]["median"], kern["t_index_select"]["median"]
        floor = round(abs(kern["g#control"]["median"] - gm), 2)
        res["kernel"] = dict(kern, unit="us per call (device events over %d back-to-back calls, %d rounds)" % (a.reps, a.rounds),
                             table_rows=M, table_mib=round(rows.numel() * 4 / 2 ** 20, 1), index_sets=a.sets,
                             destinations_mib=round(a.sets * N * F * 4 / 2 ** 20, 1), bytes_moved_per_call=moved,
                             noise_floor_us=floor, g_over_t=round(gm / tm, 3), g_not_slower_than_t=bool(gm <= tm + floor))
        del rows, dsts
        torch.cuda.empty_cache()

    if "train" not in skip:
        import pandas as pd
        import rna_gan_amd as P
        from rna_gan_amd import vae_train as VT
        scratch = tempfile.mkdtemp(prefix="ab_rna_loader_")
        rng = np.random.default_rng(1)
        t0 = time.perf_counter()
        paths = []
        cols = ["rna_G%d" % j for j in range(F)]
        for i in range(2):
            m = a.rows // 2
            df = pd.DataFrame(np.round(rng.gamma(1.5, 20.0, size=(m, F)), 2), columns=cols)
            df.insert(0, "wsi_file_name", ["GTEX-T%d-%05d.svs" % (i, r) for r in range(m)])
            paths.append(os.path.join(scratch, "tissue%d.csv" % i))
            df.to_csv(paths[-1], index=False)
        t1 = time.perf_counter()
        config = {"path_csv": paths, "rna_features": F, "save_dir": scratch}
        np.random.seed(99)
        frames = RT.read_tables(config)
        t2 = time.perf_counter()
        rows, scaler, indices, parts = RT.prepare_tables(frames, 99)
        t3 = time.perf_counter()
        for p in paths:
            os.remove(p)
        del frames, parts
        table = RT.RnaTableSet.from_array(np.concatenate([rows[k] for k in RT.PARTS], axis=0), device)
        torch.cuda.synchronize(device)
        t4 = time.perf_counter()
        n_train = rows["train"].shape[0]
        res["table"] = {"rows": a.rows, "train_rows": n_train, "bytes_resident": table.nbytes,
                        "seconds": {"write_csv": round(t1 - t0, 1), "read_csv": round(t2 - t1, 1),
                                    "split_fit_transform": round(t3 - t2, 1), "upload": round(t4 - t3, 2)}}
        print("[ab_rna_loader] table: %s" % json.dumps(res["table"]), file=sys.stderr, flush=True)
        torch.manual_seed(0)
        model = RT.model_from_config({}, F)
        model = model.set_precision("bf16").cuda()
        opt = P.Adam(model.parameters(), lr=1e-4, weight_decay=1e-5).bind(model)
        host = RT.RNADataset([rows["train"]])
        loaders = {"host_w0": DataLoader(host, batch_size=N, shuffle=True, drop_last=True, num_workers=0),
                   "host_w4": DataLoader(host, batch_size=N, shuffle=True, drop_last=True, num_workers=4),
                   "resident": RT.RnaTableLoader(table, np.arange(n_train), N, shuffle=True, seed=99, drop_last=True)}
        steps = a.epochs * (n_train // N)
        real_save = torch.save

        def one_pass(loader):
            torch.save = lambda *args, **kw: None                 # the passes time iterations, not a 1.1 GB checkpoint
            try:
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                VT.train_betaVAE(model, opt, {"train": loader, "val": []}, save_dir=scratch, num_epochs=a.epochs, verbose=False)
                torch.cuda.synchronize(device)
                return steps / (time.perf_counter() - t0)
            finally:
                torch.save = real_save
        for loader in loaders.values():
            one_pass(loader)
        t = interleave(loaders, a.train_rounds, one_pass, "train it/s")
        tr = {n: stats(v) for n, v in t.items()}
        res["train"] = dict(tr, unit="train_betaVAE iterations per second", iterations_per_pass=steps, epochs_per_pass=a.epochs,
                            resident_over_host_w0=round(tr["resident"]["median"] / tr["host_w0"]["median"], 3),
                            resident_over_host_w4=round(tr["resident"]["median"] / tr["host_w4"]["median"], 3),
                            ms_per_iteration={n: round(1e3 / tr[n]["median"], 2) for n in tr},
                            note="one model and optimizer for all variants; validation phase empty; no checkpoint written")

    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
