"""Tile quality control without a GPU: the numpy restatement of rg_tile_qc (tests/tissue_refs.py) pinned against scipy's binary
dilation, an exact rational Otsu argmax and numpy's percentile; the CPU-tensor path of rna_gan_amd.tissue against the restatement;
the host decisions (tissue_fraction, luma_percentiles, low_contrast, accept); the ABI rows."""
import os

import numpy as np
import pytest
import torch

from rna_gan_amd import _abi
from rna_gan_amd import tissue as TQ
import tissue_refs as T


# ------------------------------------------------------------------ dilation
def test_dilation_equals_scipy_on_random_masks():
    from scipy.ndimage import binary_dilation
    rng = np.random.default_rng(7)
    for (H, W, p) in ((8, 8, 0.1), (16, 20, 0.02), (33, 7, 0.05), (64, 64, 0.003), (1, 30, 0.1), (30, 1, 0.1)):
        m = rng.random((H, W)) < p
        for d in (1, 2, 3, 8):
            assert np.array_equal(T.dilate_ref(m, d), binary_dilation(m, iterations=d)), (H, W, d)
            assert np.array_equal(TQ._dilate(m, d), binary_dilation(m, iterations=d)), (H, W, d)
        assert np.array_equal(T.dilate_ref(m, 0), m) and np.array_equal(TQ._dilate(m, 0), m)


@pytest.mark.parametrize("where,count", [((8, 10), 25), ((0, 10), 16), ((8, 0), 16), ((0, 0), 10), ((15, 19), 10)])
def test_single_pixel_dilates_to_the_l1_ball(where, count):
    from scipy.ndimage import binary_dilation
    m = np.zeros((16, 20), dtype=bool)
    m[where] = True
    got = T.dilate_ref(m, 3)
    assert int(got.sum()) == count and np.array_equal(got, binary_dilation(m, iterations=3))
    rr, cc = np.mgrid[0:16, 0:20]
    assert np.array_equal(got, np.abs(rr - where[0]) + np.abs(cc - where[1]) <= 3)
    # the same through the whole rule: the tile whose raw mask is that pixel
    row, raw, dil = T.tile_ref(T.single_pixel_tile(16, 20, *where)[0])
    assert np.array_equal(raw, m) and row[4] == 1 and row[5] == count and np.array_equal(dil, got)


# ------------------------------------------------------------------ Otsu
def test_fp64_otsu_picks_the_exact_bin_on_every_histogram_the_gpu_tests_use():
    hs = T.all_test_histograms()
    assert len(hs) >= 80
    for i, h in enumerate(hs):
        want = T.otsu_exact(h)
        assert T.otsu_ref(h) == want, i
        assert TQ._otsu(h) == want, i


def test_otsu_edge_cases():
    h = np.zeros(256, dtype=np.int64)
    h[37] = 65536
    assert T.otsu_ref(h) == T.otsu_exact(h) == TQ._otsu(h) == 37            # a constant channel: lo
    h[:] = 0
    h[10] = h[200] = 160
    assert T.otsu_ref(h) == T.otsu_exact(h) == TQ._otsu(h) == 10            # every candidate ties exactly: the first
    h[:] = 0
    h[0], h[255] = 1, 1 << 26                                               # the ceiling on H W: w1 w2 is still exact
    assert T.otsu_ref(h) == T.otsu_exact(h) == TQ._otsu(h) == 0
    h[:] = 1
    assert T.otsu_ref(h) == T.otsu_exact(h) == TQ._otsu(h) == 127


def test_s8_and_luma():
    rgb = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [200, 100, 150], [1, 0, 0], [3, 2, 2]]], dtype=np.uint8)
    assert T.s8_ref(rgb).tolist() == [[0, 0, 255, 127, 255, 85]]
    assert T.luma_ref(rgb).tolist() == [[0, 2550000, 541875, 1248550, 2125, 22125]]


# ------------------------------------------------------------------ percentiles
@pytest.mark.parametrize("shape", [(8, 8), (16, 20), (33, 7), (256, 256), (1, 1)])
def test_luma_percentiles_equal_numpy(shape):
    H, W = shape
    rgb = T.tissue_like(2, H, W, 5)
    st = TQ.tile_stats(torch.from_numpy(rgb))
    assert st.ranks == T.ranks_ref(H * W) == TQ.percentile_ranks(H * W)[0]
    got = TQ.luma_percentiles(st)
    for n in range(2):
        want = np.percentile(T.luma_ref(rgb[n]).reshape(-1).astype(np.float64), [1, 99]) / (10000.0 * 255.0)
        assert np.allclose(got[n], want, rtol=1e-12, atol=0.0), (got[n], want)
    for q in ((0, 100), (50, 50), (2.5, 97.5)):
        st = TQ.tile_stats(torch.from_numpy(rgb), percentiles=q)
        want = np.percentile(T.luma_ref(rgb[0]).reshape(-1).astype(np.float64), list(q)) / (10000.0 * 255.0)
        assert np.allclose(TQ.luma_percentiles(st)[0], want, rtol=1e-12, atol=0.0)
        assert all(0 <= r < H * W for r in st.ranks)


# ------------------------------------------------------------------ the CPU-tensor path
@pytest.mark.parametrize("N,H,W", [s for s in T.SHAPES if s[1] * s[2] <= 64 * 64])
def test_cpu_path_equals_the_restatement(N, H, W):
    rgb = T.random_tiles(N, H, W)
    for d in T.DILATES:
        want, wmask = T.batch_ref(rgb, dilate=d, key=("random", N, H, W))
        for layout in ("nhwc", "nchw"):
            for order in ("rgb", "bgr"):
                st = TQ.tile_stats(torch.from_numpy(T.stored(rgb, layout, order)), layout=layout, order=order, dilate=d,
                                   return_mask=True)
                assert np.array_equal(st.stats, want), (layout, order, d)
                assert st.mask.dtype == torch.uint8 and np.array_equal(st.mask.numpy(), wmask)
                assert (st.H, st.W, len(st)) == (H, W, N)
    assert TQ.tile_stats(torch.from_numpy(T.stored(rgb, "nhwc", "rgb"))).mask is None


def test_cpu_path_on_the_special_tiles():
    for t in T.special_tiles():
        for rgb_min in (50, 0, 229):
            want, wmask = T.batch_ref(t, rgb_min=rgb_min)
            st = TQ.tile_stats(torch.from_numpy(t), rgb_min=rgb_min, return_mask=True)
            assert np.array_equal(st.stats, want) and np.array_equal(st.mask.numpy(), wmask)
    black = TQ.tile_stats(torch.from_numpy(T.constant_tile(16, 20, (0, 0, 0))))
    assert black.stats[0].tolist() == [0] * 12
    const = TQ.tile_stats(torch.from_numpy(T.constant_tile(256, 256, (201, 201, 201))))
    assert const.stats[0].tolist() == [201, 201, 201, 0, 0, 0] + [201 * 10000] * 4 + [0, 0]


def test_decisions():
    rgb = T.random_tiles(3, 16, 20).copy()
    st = TQ.tile_stats(torch.from_numpy(rgb))
    frac = TQ.tissue_fraction(st)
    assert frac.dtype == np.float64 and np.array_equal(frac, st.dilated_count / 320.0)
    p = TQ.luma_percentiles(st)
    lc = TQ.low_contrast(st)
    assert np.array_equal(lc, (p[:, 1] - p[:, 0]) / 2.0 < 0.05)
    ok = TQ.accept(st)
    assert ok.dtype == bool and np.array_equal(ok, (st.dilated_count > 0.2 * 320) & ~lc)
    # the reference's comparison is strict: exactly min_tissue of the tile is not enough
    one = T.single_pixel_tile(16, 20, 8, 10)
    s1 = TQ.tile_stats(torch.from_numpy(one))
    assert int(s1.dilated_count[0]) == 25
    assert not TQ.accept(s1, min_tissue=25 / 320.0, fraction=0.0)[0] and TQ.accept(s1, min_tissue=24.5 / 320.0, fraction=0.0)[0]
    # a washed-out tile is low-contrast whatever its mask; a black / white checkerboard is not
    assert TQ.low_contrast(TQ.tile_stats(torch.from_numpy(T.constant_tile(16, 20))))[0]
    assert not TQ.accept(TQ.tile_stats(torch.from_numpy(T.constant_tile(16, 20))))[0]
    chk = T.two_level_tile(16, 20, (255, 255, 255), (0, 0, 0))
    assert not TQ.low_contrast(TQ.tile_stats(torch.from_numpy(chk)))[0]
    assert TQ.low_contrast(TQ.tile_stats(torch.from_numpy(chk)), fraction=0.51)[0]


def test_refusals():
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    for kw in (dict(layout="hwc"), dict(order="gbr"), dict(dilate=9), dict(dilate=-1), dict(rgb_min=256), dict(rgb_min=-1),
               dict(percentiles=(1, 101)), dict(percentiles=(1,)), dict(layout="nchw")):
        with pytest.raises(ValueError):
            TQ.tile_stats(x, **kw)
    with pytest.raises(ValueError):
        TQ.tile_stats(x.float())
    with pytest.raises(ValueError):
        TQ.tile_stats(x[0])
    empty = TQ.tile_stats(x[:0], return_mask=True)
    assert len(empty) == 0 and tuple(empty.mask.shape) == (0, 8, 8) and TQ.accept(empty).shape == (0,)


# ------------------------------------------------------------------ the boundary
def test_abi_rows():
    i, p, z = _abi._i, _abi._p, _abi._z
    assert _abi.PROTOTYPES["rg_tile_qc"] == (i, [p, i, i, i, i, i, i, p, p, p, p, z, p])
    assert _abi.PROTOTYPES["rg_tile_qc_workspace_bytes"] == (z, [i, i, i])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnagan_hip.h")).read()
    assert "int rg_tile_qc(" in header and "size_t rg_tile_qc_workspace_bytes(int N, int H, int W);" in header
    assert (T.PLANAR, T.REVERSE) == (TQ.RG_EXPORT_PLANAR, TQ.RG_EXPORT_REVERSE) == (1, 2)
    assert "rg_tissue.hip" in __import__("rna_gan_amd.build", fromlist=["SOURCES"]).SOURCES
    for half in ("bf16", "f16"):
        lib = _abi.load(half)
        assert lib.rg_tile_qc_workspace_bytes(0, 8, 8) == 0 and lib.rg_tile_qc_workspace_bytes(3, 8, 8) % 4 == 0
        assert lib.rg_tile_qc_workspace_bytes(3, 8, 8) == 3 * lib.rg_tile_qc_workspace_bytes(1, 300, 260) > 0


# ------------------------------------------------------------------ flags and the metric's settings (no device needed)
def test_cli_flags_and_metric_settings(capsys):
    import pickle
    import generate_tissue_images as G
    import histopathology_gan as H
    from rna_gan_amd.metrics import TissueYield
    bulk = ["--synthetic", "--patients", "1,2", "--tiles_per_patient", "3", "--out_dir", "x"]
    a = G.parse_args(bulk)
    assert (a.qc, a.qc_min_tissue, a.qc_dilate, a.qc_rgb_min) == ("off", 0.2, 3, 50)
    a = G.parse_args(bulk + ["--qc", "filter", "--qc_min_tissue", "0.35", "--qc_dilate", "0", "--qc_rgb_min", "10"])
    assert (a.qc, a.qc_min_tissue, a.qc_dilate, a.qc_rgb_min) == ("filter", 0.35, 0, 10)
    for bad in (bulk + ["--qc", "on"], bulk + ["--qc_min_tissue", "-0.1"], bulk + ["--qc_dilate", "9"], bulk + ["--qc_rgb_min", "-1"],
                ["--synthetic", "--random_patient", "--save_path", "g.png", "--qc", "report"]):
        with pytest.raises(SystemExit):
            G.parse_args(bad)
    assert G.QC_COLUMNS[:3] == ("patient", "tile", "stored_index") and len(G.QC_COLUMNS) == 12
    base = ["--config", "c.json", "--loss_type", "wgan"]
    assert H.parse_args(base).qc_samples == 0 and H.parse_args(base + ["--qc_samples", "64"]).qc_samples == 64
    with pytest.raises(SystemExit):
        H.parse_args(base + ["--qc_samples", "1"])
    capsys.readouterr()
    m = TissueYield(6, min_tissue=0.3, dilate=2, rgb_min=40, seed=9, batch_size=4, encoding_dims=8)
    assert tuple(m.noise.shape) == (6, 8) and torch.equal(m.noise, torch.randn(6, 8, generator=torch.Generator().manual_seed(9)))
    m.history.append({"accepted": 0.5, "tissue_fraction": 0.4, "low_contrast": 0.1})
    back = pickle.loads(pickle.dumps(m))
    assert (back.n_fake, back.min_tissue, back.dilate, back.rgb_min, back.seed, back.batch_size) == (6, 0.3, 2, 40, 9, 4)
    assert back.history == m.history and back.noise is None and back.last is None
    st = TQ.tile_stats(torch.from_numpy(T.stored(T.random_tiles(3, 16, 20), "nhwc", "rgb")))
    score = m.calculate_score(st)
    assert score == {"accepted": float(TQ.accept(st, 0.3).sum()) / 3, "tissue_fraction": float(TQ.tissue_fraction(st).sum()) / 3,
                     "low_contrast": float(TQ.low_contrast(st).sum()) / 3}
    rows = TQ.stats_from_rows(st.stats.tolist(), 16, 20)
    assert np.array_equal(rows.stats, st.stats) and (rows.ranks, rows.weights) == (st.ranks, st.weights)
    with pytest.raises(ValueError):
        TQ.tile_stats_device(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
