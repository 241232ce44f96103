"""The tiler without a GPU: the numpy restatements of tests/tiler_refs.py pinned against PIL.Image.resize, scipy's binary erosion
and dilation and plain loops; the CPU-tensor path of rna_gan_amd.tiler against the restatements; tile_raster on a CPU tensor against
a sequential per-window loop (crop, tile_stats, accept, Pillow resize); the ABI rows and the refusals that need no device."""
import os

import numpy as np
import pytest
import torch

from rna_gan_amd import _abi
from rna_gan_amd import tiler as TL
from rna_gan_amd import tissue as TQ
import tiler_refs as R


# ------------------------------------------------------------------ the resize
@pytest.mark.parametrize("case", R.SIZE_CASES + R.BIG_CASES + [(128, 128, 256, 256)])
def test_resize_restatement_equals_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    h, w, oh, ow = case
    for kind in R.CONTENTS:
        img = R.content(kind, h, w)
        want = np.asarray(Image.fromarray(img).resize((ow, oh)))
        stats = {}
        got = R.resize_ref(img, oh, ow, stats)
        assert np.array_equal(got, want), (case, kind, int((got != want).sum()))
        cpu = TL.resize_windows(torch.from_numpy(img), [(0, 0)], (h, w), (oh, ow))
        assert cpu.dtype == torch.uint8 and np.array_equal(cpu.numpy()[0], want), (case, kind)
        if kind == "white":
            assert bool((got == 255).all())
        if kind == "binary" and (h, w) != (oh, ow) and h * w > 1:
            assert stats["below"] > 0 and stats["above"] > 0, "the 0 / 255 content must overshoot and clip at both ends: %r" % stats


def test_pillow_tables_are_the_contract():
    for n_in, n_out in ((512, 256), (768, 256), (37, 16), (53, 16), (12, 16), (1, 4), (100, 16), (40, 48), (70, 35), (8192, 1024)):
        bounds, coef = TL.pillow_tables(n_in, n_out)
        K = R.ksize_ref(n_in, n_out)
        assert bounds.dtype == coef.dtype == np.int32 and bounds.shape == (n_out, 2) and coef.shape == (n_out, K)
        assert np.array_equal(np.concatenate([bounds, coef], axis=1), R.table_ref(n_in, n_out))
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= K).all()
    assert R.ksize_ref(8192, 1024) == 33 and R.ksize_ref(68, 8) == 35 and R.ksize_ref(69, 8) == 37 and R.ksize_ref(512, 256) == 9 and R.ksize_ref(768, 256) == 13 and R.ksize_ref(12, 16) == 5
    with pytest.raises(ValueError):
        TL.pillow_tables(0, 4)


def test_windows_on_the_cpu_path():
    """zeros outside the raster, negative origins, overlap, the reversed order, a subset"""
    rng = np.random.default_rng(5)
    raster = rng.integers(0, 256, (45, 61, 3), dtype=np.uint8)
    for (h, w, oh, ow) in ((8, 8, 8, 8), (32, 32, 16, 16), (37, 53, 16, 16), (12, 12, 16, 16)):
        pos = R.window_positions(45, 61, h, w)
        want = R.windows_ref(raster, pos, h, w, oh, ow)
        got = TL.resize_windows(torch.from_numpy(raster), pos, (h, w), (oh, ow)).numpy()
        assert np.array_equal(got, want), (h, w, oh, ow)
        bgr = TL.resize_windows(torch.from_numpy(raster), np.array(pos), (h, w), (oh, ow), order="bgr").numpy()
        assert np.array_equal(bgr, want[..., ::-1])
        sub = TL.resize_windows(torch.from_numpy(raster), pos[3:9:2], (h, w), (oh, ow)).numpy()
        assert np.array_equal(sub, want[3:9:2])
        assert not want[-1].any() and not want[-2].any() and want[0].any()
    assert tuple(TL.resize_windows(torch.from_numpy(raster), [], 8, 4).shape) == (0, 4, 4, 3)


# ------------------------------------------------------------------ erosion and the closing
@pytest.mark.parametrize("shape", R.ERODE_SHAPES)
def test_erode_equals_scipy(shape):
    from scipy.ndimage import binary_dilation, binary_erosion
    H, W = shape
    for name, m in R.mask_cases(H, W).items():
        for r in range(9):
            want = binary_erosion(m, iterations=r).astype(np.uint8) if r else m
            ref = R.erode_ref(m, r)
            assert np.array_equal(ref, want), (name, shape, r)
            if H > 2 * r and W > 2 * r and H * W > 1:
                assert want.any() and not want.all(), "case %s %s r %d must keep both values" % (name, shape, r)
            got = TL.erode(torch.from_numpy(m), r)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (name, shape, r)
        # the closing: dilation, then erosion
        sparse = 1 - m if name == "dense" else m
        for r in (1, 3):
            dil = binary_dilation(sparse, iterations=r)
            assert np.array_equal(R.dilate_l1_ref(sparse, r), dil)
            assert np.array_equal(R.erode_ref(dil, r), binary_erosion(dil, iterations=r))
            assert np.array_equal(TL.erode(torch.from_numpy(TQ._dilate(sparse != 0, r).astype(np.uint8)), r).numpy(),
                                  binary_erosion(dil, iterations=r))
    stack = np.stack(list(R.mask_cases(H, W).values())[:3])
    got = TL.erode(torch.from_numpy(stack), 2).numpy()
    assert np.array_equal(got, np.stack([R.erode_ref(m, 2) for m in stack]))


def test_slide_mask_is_the_closing_of_the_tile_mask():
    from scipy.ndimage import binary_dilation, binary_erosion
    thumb = TL.thumbnail(torch.from_numpy(R.slide().copy()), 8)
    st = TQ.tile_stats(thumb[None], dilate=0, return_mask=True)
    raw = st.mask.numpy()[0] != 0
    want = binary_erosion(binary_dilation(raw, iterations=3), iterations=3)
    got = TL.slide_mask(thumb).numpy()
    assert got.shape == raw.shape and np.array_equal(got != 0, want) and want.any() and not want.all()


# ------------------------------------------------------------------ the box thumbnail
def test_box_reduce_equals_a_loop():
    rng = np.random.default_rng(9)
    for (RH, RW) in ((1, 1), (13, 29), (64, 64), (130, 67)):
        a = rng.integers(0, 256, (RH, RW, 3), dtype=np.uint8)
        for f in R.BOX_FACTORS:
            want = R.box_ref(a, f)
            got = TL.thumbnail(torch.from_numpy(a), f).numpy()
            assert got.shape == (-(-RH // f), -(-RW // f), 3) and np.array_equal(got, want), (RH, RW, f)
    white = np.full((70, 33, 3), 255, dtype=np.uint8)
    assert bool((TL.thumbnail(torch.from_numpy(white), 32).numpy() == 255).all())
    assert np.array_equal(TL.thumbnail(torch.from_numpy(white), 1).numpy(), white)
    for f in (0, 65):
        with pytest.raises(ValueError):
            TL.thumbnail(torch.from_numpy(white), f)


# ------------------------------------------------------------------ the grid
def test_grid_origins_follow_the_reference():
    for (RW, RH, read) in ((1280, 1024, (128, 128)), (1000, 700, (96, 96)), (50, 300, (64, 32)), (10, 10, (64, 64))):
        xmax, ymax, patch_size_resized = RW, RH, read
        indices = [(x, y) for x in range(0, xmax, patch_size_resized[0]) for y in
                   range(0, ymax, patch_size_resized[0])]
        state = np.random.get_state()
        np.random.seed(5)
        np.random.shuffle(indices)
        np.random.set_state(state)
        got = TL.grid_origins(RW, RH, read)
        assert got.dtype == np.int32 and got.tolist() == [list(t) for t in indices]
    assert TL.grid_origins(1280, 1024, 128, seed=6).tolist() != TL.grid_origins(1280, 1024, 128).tolist()


# ------------------------------------------------------------------ tile_raster
_SEQ = {}


def _sequential(max_patches):
    """the reference's loop, one window at a time: slide mask, crop, tile_stats, accept, Pillow resize"""
    from PIL import Image
    if max_patches in _SEQ:
        return _SEQ[max_patches]
    a = R.slide()
    RH, RW = a.shape[:2]
    read = int(R.SLIDE_KW["app_mag"] / 20 * 1.0 * R.SLIDE_KW["patch_size"])
    p = R.SLIDE_KW["patch_size"]
    thumb = R.box_ref(a, R.SLIDE_KW["thumb_factor"])
    mask = TL.slide_mask(torch.from_numpy(thumb)).numpy()
    ratio_x, ratio_y = RW / mask.shape[1], RH / mask.shape[0]
    tiles, origins, rows = [], [], []
    off_mask = rejected = 0
    for x, y in TL.grid_origins(RW, RH, (read, read)).tolist():
        if len(tiles) >= max_patches:
            break
        if not mask[int(y / ratio_y), int(x / ratio_x)]:
            off_mask += 1
            continue
        patch = R.crop_ref(a, x, y, read, read)
        st = TQ.tile_stats(torch.from_numpy(patch[None]))
        if not TQ.accept(st)[0]:
            rejected += 1
            continue
        tiles.append(np.asarray(Image.fromarray(patch).resize((p, p))))
        origins.append((x, y))
        rows.append(st.stats[0])
    _SEQ[max_patches] = (np.stack(tiles), np.array(origins, dtype=np.int32), np.stack(rows), mask, off_mask, rejected)
    return _SEQ[max_patches]


def test_the_synthetic_slide_exercises_every_branch():
    pytest.importorskip("PIL.Image")
    tiles, origins, rows, mask, off_mask, rejected = _sequential(10 ** 6)
    n_cand = len(TL.grid_origins(1280, 1024, 128))
    assert n_cand == 80 and 0 < len(tiles) < n_cand
    assert off_mask > 0 and rejected > 0 and off_mask + rejected + len(tiles) == n_cand
    few = _sequential(5)
    assert len(few[0]) == 5 and np.array_equal(few[0], tiles[:5]) and few[4] + few[5] + 5 < n_cand
    # 1024 and 1280 are multiples of 128, so no window hangs over the raster's edge here: edges are test_windows_on_the_cpu_path's
    assert (origins[:, 0] + 128 <= 1280).all() and (origins[:, 1] + 128 <= 1024).all()


@pytest.mark.parametrize("batch", [1, 7, 256])
def test_tile_raster_on_a_cpu_tensor_equals_the_sequential_loop(batch):
    pytest.importorskip("PIL.Image")
    raster = torch.from_numpy(R.slide().copy())
    for max_patches in (10 ** 6, 5):
        tiles, origins, rows, mask, off_mask, rejected = _sequential(max_patches)
        got = TL.tile_raster(raster, max_patches=max_patches, batch=batch, **R.SLIDE_KW)
        assert np.array_equal(got.tiles.numpy(), tiles), (batch, max_patches)
        assert np.array_equal(got.origins, origins) and np.array_equal(got.qc, rows) and got.qc.dtype == np.int32
        assert np.array_equal(got.mask.numpy(), mask) and got.read == 128 and len(got) == len(tiles)
        assert got.candidates == 80 and got.in_mask == 80 - _sequential(10 ** 6)[4]
        assert got.examined == len(tiles) + rejected
    bgr = TL.tile_raster(raster, max_patches=5, batch=batch, order="bgr", **R.SLIDE_KW)
    assert np.array_equal(bgr.tiles.numpy(), _sequential(5)[0][..., ::-1])


def test_tile_raster_takes_a_supplied_thumbnail_or_mask_and_an_equal_read_size():
    raster = torch.from_numpy(R.slide().copy())
    base = TL.tile_raster(raster, max_patches=5, **R.SLIDE_KW)
    thumb = TL.thumbnail(raster, 8)
    a = TL.tile_raster(raster, thumbnail=thumb, max_patches=5, patch_size=64, app_mag=40.0)
    b = TL.tile_raster(raster, mask=base.mask, max_patches=5, patch_size=64, app_mag=40.0)
    for other in (a, b):
        assert torch.equal(other.tiles, base.tiles) and np.array_equal(other.origins, base.origins)
    same = TL.tile_raster(raster, mask=base.mask, max_patches=3, patch_size=128, app_mag=20.0)          # read == patch: crops
    assert same.read == 128 and len(same) == 3
    for k, (x, y) in enumerate(same.origins.tolist()):
        assert np.array_equal(same.tiles[k].numpy(), R.crop_ref(R.slide(), x, y, 128, 128))
    none = TL.tile_raster(raster, mask=torch.zeros_like(base.mask), **R.SLIDE_KW)
    assert len(none) == 0 and tuple(none.tiles.shape) == (0, 64, 64, 3) and none.qc.shape == (0, 12) and none.in_mask == 0
    assert len(TL.tile_raster(raster, max_patches=0, **R.SLIDE_KW)) == 0


# ------------------------------------------------------------------ the boundary
def test_abi_rows_and_refusals():
    i, p = _abi._i, _abi._p
    assert _abi.PROTOTYPES["rg_window_resize_u8"] == (i, [p, i, i, p, i, i, i, i, i, p, i, p, i, p, i, p])
    assert _abi.PROTOTYPES["rg_mask_erode"] == (i, [p, p, i, i, i, i, p])
    assert _abi.PROTOTYPES["rg_box_reduce_u8"] == (i, [p, i, i, i, p, p])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnagan_hip.h")).read()
    for text in ("int rg_window_resize_u8(", "int rg_mask_erode(", "int rg_box_reduce_u8(", "STORED AS A BYTE"):
        assert text in header
    assert "rg_tiler.hip" in __import__("rna_gan_amd.build", fromlist=["SOURCES"]).SOURCES
    assert (TL.MAX_K, TL.PRECISION_BITS, R.REVERSE) == (35, 22, TL.RG_EXPORT_REVERSE)
    for half in ("bf16", "f16"):
        lib = _abi.load(half)
        # refused before any launch, so no device is needed: NULL buffers, bad shapes, flags, limits
        assert lib.rg_window_resize_u8(None, 8, 8, None, 1, 8, 8, 8, 8, None, 0, None, 0, None, 0, None) == -1
        assert lib.rg_last_error()
        assert lib.rg_mask_erode(None, None, 1, 8, 8, 3, None) == -1
        assert lib.rg_box_reduce_u8(None, 8, 8, 2, None, None) == -1
        buf = torch.zeros(4096, dtype=torch.uint8)
        a, o, out = buf.data_ptr(), buf.data_ptr() + 1024, buf.data_ptr() + 2048
        assert lib.rg_window_resize_u8(a, 8, 8, o, -1, 8, 8, 8, 8, None, 0, None, 0, out, 0, None) == -1
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 8, 8, None, 0, None, 0, out, 1, None) == -1          # the planar bit
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 4, 4, None, 0, None, 0, out, 0, None) == -1          # no tables
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 4, 4, o, 8, o, 9, out, 0, None) == -1                # K = 9 needed
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 4, 4, o, 9, o, 36, out, 0, None) == -1
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 8, 8, None, 0, None, 0, a + 100, 0, None) == -1      # out inside the raster
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 8, 1025, 8, o, 9, o, 9, out, 0, None) == -2
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8193, 8, 8, 8, o, 9, o, 9, out, 0, None) == -2
        assert lib.rg_window_resize_u8(a, 8, 8, o, 1, 8, 69, 8, 8, o, 35, o, 9, out, 0, None) == -2              # 69 -> 8 needs K = 37
        assert lib.rg_window_resize_u8(a, 8, 8, o, 0, 8, 8, 8, 8, None, 0, None, 0, out, 0, None) == 0           # N == 0: no launch
        assert lib.rg_mask_erode(a, out, 1, 8, 8, 9, None) == -1 and lib.rg_mask_erode(a, out, 1, 8, 8, -1, None) == -1
        assert lib.rg_mask_erode(a, a + 8, 1, 8, 8, 1, None) == -1 and lib.rg_mask_erode(a, out, -1, 8, 8, 1, None) == -1
        assert lib.rg_mask_erode(a, out, 0, 8, 8, 1, None) == 0
        assert lib.rg_box_reduce_u8(a, 8, 8, 0, out, None) == -1 and lib.rg_box_reduce_u8(a, 8, 8, 65, out, None) == -1
        assert lib.rg_box_reduce_u8(a, 0, 8, 2, out, None) == -1 and lib.rg_box_reduce_u8(a, 8, 8, 2, a + 16, None) == -1
        assert not buf.any()


def test_cli_flags_and_slide_listing(tmp_path):
    import json
    import tile_slides as S
    base = ["--wsi_path", str(tmp_path), "--patch_path", "p", "--mask_path", "m"]
    a = S.parse_args(base)
    assert (a.patch_size, a.max_patches_per_slide, a.dezoom_factor, a.app_mag, a.thumb_factor, a.out_format, a.qc_report) == \
        (768, 2000, 1.0, 20.0, 32, "store", False)
    a = S.parse_args(base + ["--patch_size", "256", "--max_patches_per_slide", "7", "--dezoom_factor", "2.0", "--num_process", "3",
                             "--thumbnail_suffix", "_thumb.npy", "--qc_report"])
    assert (a.patch_size, a.max_patches_per_slide, a.dezoom_factor, a.qc_report) == (256, 7, 2.0, True)
    for bad in (["--patch_path", "p", "--mask_path", "m"], ["--wsi_path", "w", "--patch_path", "p"], base + ["--patch_size", "1025"],
                base + ["--thumb_factor", "65"], base + ["--dezoom_factor", "0"], base + ["--out_format", "png"], base + ["--batch", "0"],
                base + ["--synthetic_size", "12"], base + ["--min_tissue", "1.5"]):
        with pytest.raises(SystemExit):
            S.parse_args(bad)
    syn = S.parse_args(["--synthetic", "--patch_path", "p", "--mask_path", "m", "--synthetic_size", "64x96", "--seed", "4"])
    assert syn.synthetic_shape == (64, 96)
    assert S.list_slides(syn) == [("synthetic_0.svs", 4, 20.0), ("synthetic_1.svs", 5, 20.0)]
    assert S.slide_id("GTEX-14A5I-0925.svs") == "GTEX-14A5I-0925.svs" and S.slide_id("a.b.c.npy") == "a.b" and S.slide_id("x") == "x"
    for name in ("s1.npy", "s1_thumb.npy", "s2.png", "notes.txt", "s1.npy.json"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "s1.npy.json").write_text(json.dumps({"app_mag": 40}))
    assert S.list_slides(a) == [("s1.npy", str(tmp_path / "s1.npy"), 40.0), ("s2.png", str(tmp_path / "s2.png"), 20.0)]
    np.save(str(tmp_path / "s1.npy"), np.zeros((4, 5, 3), dtype=np.uint8))
    assert S._open_raster(str(tmp_path / "s1.npy")).shape == (4, 5, 3)
    np.save(str(tmp_path / "s1.npy"), np.zeros((4, 5), dtype=np.uint8))
    with pytest.raises(SystemExit):
        S._open_raster(str(tmp_path / "s1.npy"))


def test_python_refusals():
    raster = torch.zeros((16, 16, 3), dtype=torch.uint8)
    for bad in (dict(order="gbr"), dict(read_size=0), dict(out_size=(4, 0)), dict(out_size=1025), dict(read_size=8193),
                dict(read_size=69, out_size=8), dict(origins=[(0.5, 1.0)]), dict(origins=[(1, 2, 3)]), dict(origins=[(1 << 31, 0)])):
        kw = dict(dict(origins=[(0, 0)], read_size=8, out_size=4), **bad)
        with pytest.raises(ValueError):
            TL.resize_windows(raster, **kw)
    for t in (raster.float(), raster[0], torch.zeros((4, 4, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            TL.resize_windows(t, [(0, 0)], 8, 4)
        with pytest.raises(ValueError):
            TL.thumbnail(t, 2)
    m = torch.ones((4, 4), dtype=torch.uint8)
    for r in (-1, 9):
        with pytest.raises(ValueError):
            TL.erode(m, r)
    with pytest.raises(ValueError):
        TL.erode(m.float(), 1)
    for kw in (dict(order="x"), dict(batch=0), dict(patch_size=0), dict(max_patches=-1), dict(mask=torch.ones(4))):
        with pytest.raises(ValueError):
            TL.tile_raster(raster, **kw)
