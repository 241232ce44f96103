"""rna_gan_amd.stain on the device against its own numpy path (the same integers, so the same StainFit and the same bytes), and the
two programs end to end: tile_slides.py --synthetic --stain_norm macenko writes stores that PatchDataset reads plus a stain.json,
--stain_norm none writes what a run without the flag writes, stain_normalize.py normalises those stores."""
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import stain_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = "cuda:0"


@pytest.mark.parametrize("layout,order", [("nhwc", "rgb"), ("nchw", "bgr")])
def test_fit_and_normalize_equal_the_cpu_path(layout, order):
    from rna_gan_amd import stain
    rgb = R.synthetic_set(11, stains=1, n=5, size=48)
    cpu = torch.from_numpy(R.store_as(rgb, layout, order))
    dev = cpu.to(DEV)
    f_cpu = stain.fit(cpu, layout, order)
    f_dev = stain.fit(dev, layout, order)
    assert f_dev == f_cpu, (f_dev, f_cpu)
    assert np.array_equal(f_dev.he, f_cpu.he) and np.array_equal(f_dev.max_conc, f_cpu.max_conc)
    for batch in (1, 2, 5, 7):
        assert stain.fit(dev, layout, order, batch=batch) == f_cpu, batch
    want = stain.normalize(cpu, f_cpu, layout=layout, order=order)
    got = stain.normalize(dev, f_dev, layout=layout, order=order)
    assert got.device == dev.device and torch.equal(got.cpu(), want)
    assert torch.equal(dev.cpu(), cpu)                                             # the source is untouched
    out = torch.empty_like(dev)
    assert stain.normalize(dev, f_dev, out=out, layout=layout, order=order) is out and torch.equal(out.cpu(), want)
    same = dev.clone()
    stain.normalize(same, f_dev, out=same, layout=layout, order=order)
    assert torch.equal(same.cpu(), want)
    both, f2 = stain.normalize_tiles(dev, layout=layout, order=order, batch=2)
    assert f2 == f_cpu and torch.equal(both.cpu(), want)
    other = stain.StainFit([[0.6, 0.15], [0.7, 0.95], [0.35, 0.25]], [1.4, 0.8])
    assert torch.equal(stain.normalize(dev, f_dev, other, layout=layout, order=order).cpu(),
                       stain.normalize(cpu, f_cpu, other, layout=layout, order=order))


def test_unfittable_set_raises_on_the_device_too():
    from rna_gan_amd import stain
    white = torch.full((2, 16, 16, 3), 255, dtype=torch.uint8, device=DEV)
    with pytest.raises(stain.StainFitError) as e:
        stain.fit(white)
    assert e.value.counts == {"n_pixels": 512, "n_stained": 0}


def test_normalising_a_set_to_its_own_fit_is_the_identity_within_the_gate():
    """The method is the identity only up to what it discards.  (a) The textbook form reads the optical density of I + 1 and renders
    Io exp(-od): every byte comes back one higher, in the fp64 form too.  (b) A pixel's component outside the fitted plane is dropped;
    for noise-free Beer-Lambert bytes that component is the byte rounding, 0.5 / (v + 1) in optical density per channel, and it comes
    back multiplied by (v_c + 1) / (v_d + 1) between a bright channel c and a dark one d.  So the property is asked of a noise-free,
    weakly stained set (strength 0.3: the darkest byte stays above 30, the ratio below 8, the expected excess about one byte), where
    1 + (b) lies inside the textbook-agreement gate; with sensor noise or dark pixels the fp64 form itself moves bytes by more."""
    from rna_gan_amd import stain
    for s in range(2):
        rgb = R.synthetic_set(5 + s, stains=s, n=4, size=64, noise=0.0, strength=0.3)
        assert int(rgb.min()) > 30
        dev = torch.from_numpy(rgb).to(DEV)
        f = stain.fit(dev)
        out = stain.normalize(dev, f, target=f)
        d = (out.cpu().numpy().astype(np.int64) - rgb.astype(np.int64))
        print("self-normalisation, stains %d: byte differences %d .. %d" % (s, d.min(), d.max()))
        assert int(np.abs(d).max()) <= R.TEXTBOOK_GATE


def _stores(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for base, _, files in os.walk(root):
        for name in files:
            p = os.path.join(base, name)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def test_tile_slides_and_stain_normalize_end_to_end(tmp_path):
    import pandas as pd

    import stain_normalize
    import tile_slides
    from rna_gan_amd import data as PD
    from rna_gan_amd import stain

    def tile(name, extra):
        patches = str(tmp_path / name)
        args = ["--synthetic", "--synthetic_slides", "2", "--synthetic_size", "1024x1280", "--seed", "3", "--patch_path", patches,
                "--mask_path", str(tmp_path / "masks"), "--patch_size", "64", "--app_mag", "40", "--thumb_factor", "8",
                "--max_patches_per_slide", "9", "--batch", "4"] + extra
        return patches, tile_slides.run(tile_slides.parse_args(args))

    plain, w0 = tile("plain", [])
    none, w1 = tile("none", ["--stain_norm", "none"])
    mac, w2 = tile("macenko", ["--stain_norm", "macenko"])
    a, b = _stores(plain), _stores(none)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)             # none: the same files, the same bytes
    assert not any(k.endswith("stain.json") for k in a)
    ids = ["synthetic_0.svs", "synthetic_1.svs"]
    assert [p for p in w2 if p.endswith("stain.json")] == [os.path.join(mac, q, "stain.json") for q in ids]
    table = pd.DataFrame({"wsi_file_name": ids, "rna_0": [0.0] * 2, "patch_data_path": [mac] * 2, "labels": [0] * 2})
    ds = PD.PatchDataset(mac, table, 64, max_patches_total=100)
    raw_ds = PD.PatchDataset(plain, table.assign(patch_data_path=[plain] * 2), 64, max_patches_total=100)
    assert len(ds) == len(raw_ds) > 0
    for q in ids:
        rows = [j for j in range(len(ds)) if ds.filenames[j] == q]
        rows.sort(key=lambda j: int(ds.keys[j]))
        raw_rows = sorted((j for j in range(len(raw_ds)) if raw_ds.filenames[j] == q), key=lambda j: int(raw_ds.keys[j]))
        got = np.stack([ds[j][0].numpy().transpose(1, 2, 0) for j in rows])
        raw = np.stack([raw_ds[j][0].numpy().transpose(1, 2, 0) for j in raw_rows])
        rep = json.load(open(os.path.join(mac, q, "stain.json")))
        assert rep["normalized"] is True and rep["method"] == "macenko" and rep["target"]["max_conc"] == [1.9705, 1.0308]
        f = stain.StainFit.from_json(json.dumps(rep))
        raw_t = torch.from_numpy(np.ascontiguousarray(raw))
        assert f == stain.fit(raw_t) and f.n_pixels == raw.size // 3                # the slide's tiles fitted together, as one set
        assert np.array_equal(got, stain.normalize(raw_t, f).numpy()) and not np.array_equal(got, raw)
    # a cohort normalised to one of its own slides: the stain.json of slide 0 as the target
    own = os.path.join(mac, ids[0], "stain.json")
    out = str(tmp_path / "renormalised")
    written = stain_normalize.run(stain_normalize.parse_args(["--patch_path", plain, "--out_path", out, "--stain_target", own, "--batch", "4"]))
    assert written == [os.path.join(out, q, name) for q in ids for name in (q.replace(".svs", ".db"), "stain.json")]
    target = stain.load_target(own)
    for q in ids:
        names, tiles = stain_normalize.read_store(os.path.join(out, q, q.replace(".svs", ".db")))
        raw_names, raw = stain_normalize.read_store(os.path.join(plain, q, q.replace(".svs", ".db")))
        assert names == raw_names and tiles.shape == raw.shape
        raw_t = torch.from_numpy(raw)                                               # the records hold B, G, R
        f = stain.fit(raw_t, order="bgr")
        assert np.array_equal(tiles, stain.normalize(raw_t, f, target, order="bgr").numpy())
        assert stain.StainFit.from_json(open(os.path.join(out, q, "stain.json")).read()) == f
    assert stain_normalize.run(stain_normalize.parse_args(["--patch_path", plain, "--out_path", out])) == []      # skipped: they exist
    assert filecmp.dircmp(plain, none).diff_files == []
