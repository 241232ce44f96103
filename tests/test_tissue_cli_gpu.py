"""generate_tissue_images.py --qc off|report|filter and the qc= path under it (export.synthesize_u8, gan_utils.generate_tiles), on
the tiny generator (32 x 32, 64 step channels) and tiny betaVAE of tests/test_export_tiles_gpu.py."""
import csv
import filecmp
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from rna_gan_amd import data as PD
from rna_gan_amd import export as EX
from rna_gan_amd import synth
from rna_gan_amd import tissue as TQ
from rna_gan_amd.gan_utils import generate_tiles

DEV = torch.device("cuda:0")
ENC, SIZE, FEATURES = 64, 32, 48
PATIENTS, T = ["2", "7", "11"], 5
_MODELS = {}


def _models():
    if not _MODELS:
        G = P.DCGANGenerator(ENC, SIZE, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
        synth.seeded_fill_(G, 91)
        G = G.set_precision("bf16").to(DEV).train()
        bv = P.betaVAE(FEATURES, ENC, [40, 36, ENC], [36, 40], beta=0.005)
        synth.seeded_fill_(bv, 92)
        _MODELS["m"] = (SimpleNamespace(generator=G, device=DEV), bv.to(DEV).eval())
    return _MODELS["m"]


def _args(out, *extra):
    import generate_tissue_images as G
    return G.parse_args(["--synthetic", "--rna_features", str(FEATURES), "--patients", ",".join(PATIENTS), "--tiles_per_patient",
                         str(T), "--out_dir", out, "--chunk", "4", "--group", "8", "--seed", "3"] + list(extra))


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = p
    return out


def _stored_tiles(out):
    """{patient: (k, H, W, 3) uint8 RGB} read back through PatchDataset"""
    import pandas as pd
    table = pd.DataFrame({"wsi_file_name": PATIENTS, "rna_0": [0.0] * 3, "patch_data_path": [out] * 3, "labels": [0] * 3})
    ds = PD.PatchDataset(out, table, SIZE, max_patches_total=T)
    got = {q: {} for q in PATIENTS}
    for j in range(len(ds)):
        img, _ = ds[j]
        got[ds.filenames[j]][int(ds.keys[j])] = img.numpy().transpose(1, 2, 0)
    return {q: np.stack([v[k] for k in sorted(v)]) if v else np.zeros((0, SIZE, SIZE, 3), np.uint8) for q, v in got.items()}


def _read_csv(path):
    import generate_tissue_images as G
    with open(path) as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == G.QC_COLUMNS
    return rows[1:]


def test_qc_rows_travel_with_the_chunks():
    """synthesize_u8(qc=...) yields, beside each chunk, the rows the CPU path computes from that chunk's bytes; the tiles are the
    bytes of a run without qc."""
    tr, _ = _models()
    z = torch.from_numpy(np.random.default_rng(93).standard_normal((13, ENC)).astype(np.float32)).to(DEV)
    plain = EX.synthesize_u8_all(tr.generator, z, chunk=5)
    for qc, kw in (({}, {}), ({"dilate": 1, "rgb_min": 10, "percentiles": (5, 95)}, {"layout": "nchw", "order": "bgr"})):
        want_tiles = plain if not kw else EX.synthesize_u8_all(tr.generator, z, chunk=5, **kw)
        seen = []
        for start, a, rows in EX.synthesize_u8(tr.generator, z, chunk=5, qc=qc, **kw):
            assert rows.dtype == np.int32 and rows.shape == (a.shape[0], 12)
            assert np.array_equal(a, want_tiles[start:start + a.shape[0]])
            cpu = TQ.tile_stats(torch.from_numpy(a.copy()), **dict(qc, **kw))
            assert np.array_equal(rows, cpu.stats), start
            seen.append((start, a.shape[0]))
        assert seen == [(0, 5), (5, 5), (10, 3)]
    with pytest.raises(ValueError):
        list(EX.synthesize_u8(tr.generator, z, qc={"min_tissue": 0.2}))
    with pytest.raises(ValueError):
        EX.synthesize_u8_all(tr.generator, z, qc={})


def test_qc_off_is_byte_identical_report_describes_and_filter_keeps_the_accepted(tmp_path, capsys):
    import generate_tissue_images as G
    tr, bv = _models()
    outs = {name: str(tmp_path / name) for name in ("none", "off", "report", "filter")}
    G.run(_args(outs["none"]), tr, bv)
    G.run(_args(outs["off"], "--qc", "off"), tr, bv)
    # 32 x 32 tiles: three dilations fill nearly every tile, so the runs below take --qc_dilate 0, and --qc_min_tissue is chosen
    # between the tiles' tissue fractions, so that some are kept and some are not
    _, rows = G.load_rna(_args(outs["none"]))
    every = {}
    for p, t, a, r in generate_tiles(tr, rows[[2, 7, 11]], T, bv, seed=3, chunk=64, group=8, qc={"dilate": 0}):
        for k in range(a.shape[0]):
            every[(int(p[k]), int(t[k]))] = (a[k].copy(), r[k].copy())
    assert len(every) == 3 * T
    tiles = np.stack([every[(q, t)][0] for q in range(3) for t in range(T)])
    cpu = TQ.tile_stats(torch.from_numpy(tiles), dilate=0)
    assert np.array_equal(cpu.stats, np.stack([every[(q, t)][1] for q in range(3) for t in range(T)]))
    frac = np.sort(np.unique(TQ.tissue_fraction(cpu)))
    assert len(frac) > 1 and not TQ.low_contrast(cpu).any(), (frac, TQ.low_contrast(cpu))
    cut = float(frac[len(frac) // 2 - 1] + frac[len(frac) // 2]) / 2.0 if len(frac) > 1 else 0.2
    rule = ["--qc_min_tissue", repr(cut), "--qc_dilate", "0"]
    written = G.run(_args(outs["report"], "--qc", "report", *rule), tr, bv)
    capsys.readouterr()
    G.run(_args(outs["filter"], "--qc", "filter", *rule), tr, bv)
    printed = capsys.readouterr().out

    # off: the same files with the same bytes as a run without the flag, and no report
    none, off = _tree(outs["none"]), _tree(outs["off"])
    assert sorted(none) == sorted(off) and len(none) == 3 * (T + 1) and "qc.csv" not in off
    assert all(filecmp.cmp(none[k], off[k], shallow=False) for k in none)

    # report: the same store, plus qc.csv whose rows equal the CPU path on the stored tiles
    rep = _tree(outs["report"])
    assert sorted(rep) == sorted(list(none) + ["qc.csv"]) and os.path.join(outs["report"], "qc.csv") in written
    assert all(filecmp.cmp(none[k], rep[k], shallow=False) for k in none)
    stored = _stored_tiles(outs["report"])
    table = _read_csv(rep["qc.csv"])
    assert [(r[0], int(r[1])) for r in table] == [(q, t) for q in PATIENTS for t in range(T)]
    accepted = {}
    for q in PATIENTS:
        assert stored[q].shape == (T, SIZE, SIZE, 3)
        st = TQ.tile_stats(torch.from_numpy(stored[q].copy()), dilate=0)
        fr, pct, low, ok = TQ.tissue_fraction(st), TQ.luma_percentiles(st), TQ.low_contrast(st), TQ.accept(st, min_tissue=cut)
        for t in range(T):
            r = table[PATIENTS.index(q) * T + t]
            assert int(r[2]) == t and [int(v) for v in r[3:7]] == st.thresholds[t].tolist()
            assert (float(r[7]), float(r[8]), float(r[9])) == (float(fr[t]), float(pct[t, 0]), float(pct[t, 1]))
            assert (int(r[10]), int(r[11])) == (int(low[t]), int(ok[t]))
        accepted[q] = [t for t in range(T) if ok[t]]
    kept = sum(len(v) for v in accepted.values())
    assert 0 < kept < 3 * T, "the cut must separate the tiles: %r" % accepted

    # filter: exactly the accepted tiles, in tile order, renumbered; the same decisions in its qc.csv; the counts printed
    filt = _stored_tiles(outs["filter"])
    ftable = _read_csv(os.path.join(outs["filter"], "qc.csv"))
    for q in PATIENTS:
        assert np.array_equal(filt[q], stored[q][accepted[q]]), q
        assert "patient %s: %d of %d tiles rejected" % (q, T - len(accepted[q]), T) in printed
        for t in range(T):
            r, f = table[PATIENTS.index(q) * T + t], ftable[PATIENTS.index(q) * T + t]
            assert r[:2] == f[:2] and r[3:] == f[3:]
            assert int(f[2]) == (accepted[q].index(t) if t in accepted[q] else -1)
    # npy under filter carries the same tiles
    npy = str(tmp_path / "npy")
    G.run(_args(npy, "--qc", "filter", *rule, "--out_format", "npy"), tr, bv)
    for q in PATIENTS:
        assert np.array_equal(np.load(os.path.join(npy, q + ".npy")), filt[q])
    for bad in (["--qc", "maybe"], ["--qc_min_tissue", "1.5"], ["--qc_dilate", "9"], ["--qc_rgb_min", "256"]):
        with pytest.raises(SystemExit):
            _args(str(tmp_path / "x"), *bad)
