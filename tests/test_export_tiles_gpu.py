"""The bulk output path on the GPU: export.tiles_u8 / synthesize_u8 / synthesize_u8_all, gan_utils.generate_tiles and the
generation CLI's run(), on the tiny generator (32 x 32, 64 step channels) and tiny betaVAE of the trainer and metric tests."""
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
from rna_gan_amd.gan_utils import generate_tiles, synthesize
import export_refs as X

DEV = torch.device("cuda:0")
ENC, SIZE, FEATURES = 64, 32, 48
_MODELS = {}


def _models():
    """(trainer stand-in, betaVAE), built once: seeded weights, generator in train mode (as a freshly loaded trainer leaves it)."""
    if not _MODELS:
        G = P.DCGANGenerator(ENC, SIZE, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
        synth.seeded_fill_(G, 91)
        G = G.set_precision("bf16").to(DEV).train()
        bv = P.betaVAE(FEATURES, ENC, [40, 36, ENC], [36, 40], beta=0.005)
        synth.seeded_fill_(bv, 92)
        _MODELS["m"] = (SimpleNamespace(generator=G, device=DEV), bv.to(DEV).eval())
    return _MODELS["m"]


def _noise(n, seed=93):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, ENC)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("kw", [{}, {"layout": "nchw", "order": "bgr", "rounding": "trunc"},
                                {"sub": -0.75, "div": 1.7}])
def test_synthesize_u8_equals_tiles_u8_equals_the_restatement(kw):
    """N = 13 with chunk 5: a ragged last chunk, each slot used twice (fp8=False: the tiny layers have no fp8 kernel)."""
    tr, _ = _models()
    z = _noise(13)
    img = synthesize(tr.generator, z, chunk=5)
    want = X.tile_export_ref(img.cpu().numpy(), **kw)
    assert np.array_equal(EX.tiles_u8(img, **kw).cpu().numpy(), want)
    seen = []
    held = []
    for start, a in EX.synthesize_u8(tr.generator, z, chunk=5, fp8=False, **kw):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and not a.flags.owndata
        assert np.array_equal(a, want[start:start + a.shape[0]]), "wrong bytes at the moment of the yield (chunk at %d)" % start
        seen.append((start, a.shape[0]))
        held.append(a)
    assert seen == [(0, 5), (5, 5), (10, 3)]
    # two slots: the first and the third chunk shared one buffer
    assert held[0].__array_interface__["data"][0] == held[2].__array_interface__["data"][0] != held[1].__array_interface__["data"][0]
    allb = EX.synthesize_u8_all(tr.generator, z, chunk=5, **kw)
    assert allb.flags.owndata and allb.shape == want.shape and np.array_equal(allb, want)
    assert tr.generator.training                                   # synthesize restored the mode
    # the synthesis batch held fixed: the download chunk does not change a byte
    one = EX.synthesize_u8_all(tr.generator, z, chunk=4, synth_chunk=13, **kw)
    assert np.array_equal(one, EX.synthesize_u8_all(tr.generator, z, chunk=13, synth_chunk=13, **kw))
    assert np.array_equal(one, X.tile_export_ref(synthesize(tr.generator, z, chunk=13).cpu().numpy(), **kw))


def test_synthesize_u8_refusals():
    tr, _ = _models()
    for bad in (dict(noise=_noise(4).cpu()), dict(noise=_noise(4), chunk=0), dict(noise=_noise(4), layout="hwc"),
                dict(noise=_noise(4), out=torch.empty(1))):
        with pytest.raises(ValueError):
            list(EX.synthesize_u8(tr.generator, **bad))
    with pytest.raises(ValueError):
        EX.synthesize_u8_all(tr.generator, _noise(4)[:0])


def _collect(gen, T, Pn):
    out, keys = None, []
    for p, t, a in gen:
        assert p.shape == t.shape == (a.shape[0],) and a.dtype == np.uint8 and a.shape[1:] == (SIZE, SIZE, 3)
        if out is None:
            out = np.zeros((Pn, T) + a.shape[1:], dtype=np.uint8)
        out[p, t] = a
        keys += list(zip(p.tolist(), t.tolist()))
    return out, keys


def test_generate_tiles():
    tr, bv = _models()
    rna = synth.synthetic_rna(3, FEATURES, seed=94, distinct=3)
    T = 7                                                           # 21 rows, tile-major: groups of 8, 8, 5
    for g_train, v_train in ((True, False), (False, True)):
        tr.generator.train(g_train); bv.train(v_train)
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
        a3, keys = _collect(generate_tiles(tr, rna, T, bv, seed=5, chunk=3, group=8), T, 3)
        assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(DEV), dev_state)
        assert tr.generator.training == g_train and bv.training == v_train          # modes restored
        assert sorted(keys) == [(p, t) for p in range(3) for t in range(T)] and len(set(keys)) == len(keys)
    tr.generator.train(); bv.eval()
    a64, _ = _collect(generate_tiles(tr, rna, T, bv, seed=5, chunk=64, group=8), T, 3)
    assert np.array_equal(a3, a64), "the output depends on chunk"
    other, _ = _collect(generate_tiles(tr, rna, T, bv, seed=6, chunk=64, group=8), T, 3)
    assert not np.array_equal(a3, other)
    assert len(np.unique(a3.reshape(21, -1), axis=0)) == 21         # no two tiles alike
    # what a group computes, restated: tile-major rows, one latent_prep per group, the private uniform stream
    ops, _ = tr.generator.runtime()
    with torch.no_grad():
        z = bv.encode(rna.to(DEV))[0].float()
    private = torch.Generator().manual_seed(5)
    rows = torch.arange(0, 8)
    u = torch.empty(8, ENC).uniform_(-0.3, 0.3, generator=private).to(DEV)
    noise = ops.latent_prep(u.contiguous(), z[(rows % 3).to(DEV)].contiguous())
    want = X.tile_export_ref(synthesize(tr.generator, noise.float(), chunk=512).cpu().numpy())
    assert np.array_equal(a3[(rows % 3).numpy(), (rows // 3).numpy()], want)
    # a trailing single row joins the previous group; fewer than two rows in all is refused
    b, keys = _collect(generate_tiles(tr, rna, 3, bv, seed=5, group=4), 3, 3)          # 9 rows: groups of 4 and 5
    assert len(keys) == 9
    with pytest.raises(ValueError):
        list(generate_tiles(tr, rna[:1], 1, bv))
    with pytest.raises(ValueError):
        list(generate_tiles(tr, rna, 2, bv, ema=True))              # no averaged generator on this trainer


def test_cli_store_round_trip_and_grid(tmp_path):
    import pandas as pd
    from PIL import Image
    import generate_tissue_images as G
    tr, bv = _models()
    out = str(tmp_path / "tiles")
    args = G.parse_args(["--synthetic", "--rna_features", str(FEATURES), "--patients", "2,7,11", "--tiles_per_patient", "5",
                         "--out_dir", out, "--out_format", "store", "--chunk", "4", "--group", "8", "--seed", "3"])
    written = G.run(args, tr, bv)
    assert sorted(os.path.basename(w) for w in written) == ["11", "2", "7"]
    ids, rows = G.load_rna(args)
    want, _ = _collect(generate_tiles(tr, rows[[2, 7, 11]], 5, bv, seed=3, chunk=64, group=8), 5, 3)
    table = pd.DataFrame({"wsi_file_name": ["2", "7", "11"], "rna_0": [0.0] * 3, "patch_data_path": [out] * 3, "labels": [0] * 3})
    ds = PD.PatchDataset(out, table, SIZE, max_patches_total=5)
    assert len(ds) == 15
    for j in range(len(ds)):
        img, _ = ds[j]
        q = ["2", "7", "11"].index(ds.filenames[j])
        assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), want[q, int(ds.keys[j])].transpose(2, 0, 1))   # RGB CHW
    # npy and png carry the same tiles
    for fmt in ("npy", "png"):
        a2 = G.parse_args(["--synthetic", "--rna_features", str(FEATURES), "--patients", "2,7,11", "--tiles_per_patient", "5",
                           "--out_dir", str(tmp_path / fmt), "--out_format", fmt, "--chunk", "4", "--group", "8", "--seed", "3"])
        G.run(a2, tr, bv)
    assert np.array_equal(np.load(str(tmp_path / "npy" / "7.npy")), want[1])
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "png" / "11" / "4.png"))), want[2, 4])
    # --random_patient: one 8 x 8 grid
    png = str(tmp_path / "grid" / "g.png")
    a3 = G.parse_args(["--synthetic", "--rna_features", str(FEATURES), "--random_patient", "--sample_size", "10", "--save_path", png])
    assert G.run(a3, tr, bv) == [png]
    im = Image.open(png)
    assert im.size == (8 * SIZE, 8 * SIZE) and im.mode == "RGB"
    g = np.asarray(im)
    assert g[:SIZE].max() > 0 and g[2 * SIZE:].max() == 0 and g[SIZE:2 * SIZE, 2 * SIZE:].max() == 0      # 10 tiles: 8 + 2
