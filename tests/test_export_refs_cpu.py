"""The tile export without a GPU: the numpy restatement of rg_tile_export_u8 (tests/export_refs.py) pinned against torch's own
chains, the round-trip facts over all 256 bytes, the CPU path of export.tiles_u8, stored LZ4 frames and the store round trip,
the ABI entry and the generation CLI's argument checks."""
import ctypes
import hashlib
import os
import pickle

import numpy as np
import pytest
import torch

from rna_gan_amd import _abi
from rna_gan_amd import data as PD
from rna_gan_amd import export as EX
import export_refs as X
from test_lz4_system_cpu import _lib_decompress_frame, needs_lz4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS, ORDERS, RULES = ("nhwc", "nchw"), ("rgb", "bgr"), ("round", "trunc")


def _draws(n=10 ** 6, seed=1):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def test_restatement_equals_the_save_image_chain():
    """((x - lo) / max(hi - lo, 1e-5)).mul(255).add_(0.5).clamp_(0, 255).to(uint8) with a data-dependent (lo, hi): what
    Trainer.save_image_grid computes."""
    x = _draws()
    t = torch.from_numpy(x)
    lo, hi = float(t.min()), float(t.max())
    want = ((t - lo) / max(hi - lo, 1e-5)).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    got = X.export_byte_ref(x, lo, X.denominator(lo, hi), "round")
    assert np.array_equal(got, want)
    # a range smaller than the floor: the denominator is fp32(1e-5)
    assert X.denominator(0.25, 0.25) == np.float32(1e-5)
    y = np.full(100, 0.25, dtype=np.float32)
    ty = torch.from_numpy(y)
    want = ((ty - 0.25) / max(0.0, 1e-5)).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(X.export_byte_ref(y, 0.25, X.denominator(0.25, 0.25)), want)


def test_value_equals_export_images_nhwc_and_the_reference_script():
    """(x - (-1)) / 2 and x * 0.5 + 0.5 are the same bits; the truncating rule is ``img *= 255; img.astype(uint8)`` on it."""
    x = np.concatenate([_draws(seed=2) * np.float32(0.7), X.edge_values()])
    v = X.export_value_ref(x, -1.0, 2.0)
    w = (x * np.float32(0.5) + np.float32(0.5)).astype(np.float32)
    ok = ~np.isnan(v)
    assert np.array_equal(v[ok].view(np.uint32), w[ok].view(np.uint32)) and np.isnan(w[~ok]).all()
    inside = ok & (v >= 0) & (v * np.float32(255.0) < 256)            # where numpy's float -> uint8 cast is defined
    img = v[inside].copy()
    img *= 255
    assert np.array_equal(X.export_byte_ref(x[inside], rounding="trunc")[img < 255], img.astype(np.uint8)[img < 255])
    assert (X.export_byte_ref(x[inside], rounding="trunc")[img >= 255] == 255).all()


def test_round_trip_over_all_bytes():
    b = np.arange(256, dtype=np.uint8)
    x = X.host_transform(b)
    assert np.array_equal(X.export_byte_ref(x, -1.0, 2.0, "round"), b)
    t = X.export_byte_ref(x, -1.0, 2.0, "trunc")
    lower = b[t != b]
    assert tuple(int(k) for k in lower) == X.TRUNC_ONE_LOWER and len(X.TRUNC_ONE_LOWER) == 63
    assert np.array_equal(t[lower].astype(np.int64), lower.astype(np.int64) - 1)


def test_specials():
    x = np.array([np.nan, -np.inf, np.inf, -1.5, 1.5, -1.0, 1.0, 0.0, -0.0], dtype=np.float32)
    assert X.export_byte_ref(x).tolist() == [0, 0, 255, 0, 255, 0, 255, 128, 128]
    assert X.export_byte_ref(x, rounding="trunc").tolist() == [0, 0, 255, 0, 255, 0, 255, 127, 127]
    assert X.export_byte_ref(np.array([-0.0], dtype=np.float32), 0.0, 1.0, "trunc").tolist() == [0]      # t = -0.0


@pytest.mark.parametrize("C", [1, 3, 4])
def test_cpu_path_of_tiles_u8_equals_the_restatement(C):
    e = X.edge_values()
    rng = np.random.default_rng(C)
    x = np.concatenate([e, (rng.standard_normal(2 * C * 7 * 6 * 60 - e.size % (C * 7 * 6)) * 0.7).astype(np.float32)])
    x = x[:x.size // (C * 7 * 6) * (C * 7 * 6)].reshape(-1, C, 7, 6)
    fin = x[np.isfinite(x)]
    lo, hi = float(fin.min()), float(fin.max())
    for sub, div in ((-1.0, 2.0), (lo, max(hi - lo, 1e-5))):
        for layout in LAYOUTS:
            for order in ORDERS:
                for rule in RULES:
                    got = EX.tiles_u8(torch.from_numpy(x), layout, order, rule, sub, div)
                    assert got.dtype == torch.uint8 and got.is_contiguous()
                    assert np.array_equal(got.numpy(), X.tile_export_ref(x, layout, order, rule, sub, div)), (layout, order, rule)
    out = torch.empty(x.shape[0], 7, 6, C, dtype=torch.uint8)
    assert EX.tiles_u8(torch.from_numpy(x), out=out) is out
    assert np.array_equal(out.numpy(), X.tile_export_ref(x))
    assert tuple(EX.tiles_u8(torch.empty(0, C, 7, 6)).shape) == (0, 7, 6, C)


def test_tiles_u8_refusals():
    x = torch.zeros(2, 3, 4, 4)
    for kw in ({"layout": "hwc"}, {"order": "grb"}, {"rounding": "floor"}, {"div": 0.0}, {"div": float("nan")}, {"div": 1e-60},
               {"out": torch.empty(2, 4, 4, 3)}, {"out": torch.empty(2, 3, 4, 4, dtype=torch.uint8)},
               {"out": torch.empty(2, 4, 4, 6, dtype=torch.uint8)[..., ::2]}):
        with pytest.raises(ValueError):
            EX.tiles_u8(x, **kw)
    for bad in (x.double(), x[0], x.to(torch.uint8), np.zeros((2, 3, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            EX.tiles_u8(bad)
    assert EX.export_flags("nchw", "bgr", "trunc") == 7 and EX.export_flags() == 0
    assert (EX.RG_EXPORT_PLANAR, EX.RG_EXPORT_REVERSE, EX.RG_EXPORT_TRUNC) == (X.PLANAR, X.REVERSE, X.TRUNC) == (1, 2, 4)


# ------------------------------------------------------------------------------------- the argument layer of the uint8 image side
def test_tile_args_refuses_what_stain_and_tissue_refused():
    from rna_gan_amd import stain, tissue
    ok = torch.zeros((2, 5, 7, 3), dtype=torch.uint8)
    assert EX.tile_args(ok, "nhwc", "bgr", "f") == (2, 5, 7) and EX.tile_args(ok.permute(0, 3, 1, 2), "nchw", "rgb", "f") == (2, 5, 7)
    takes = "%s takes a uint8 (N, H, W, 3) or (N, 3, H, W) tensor"
    cases = [((ok.float(), "nhwc", "rgb"), takes),                                                           # a wrong dtype
             ((ok[0], "nhwc", "rgb"), takes),                                                                # a wrong rank
             ((ok.numpy(), "nhwc", "rgb"), takes),
             ((ok, "nchw", "rgb"), "%s needs 3 channels in layout nchw, got (2, 5, 7, 3)"),                 # a wrong channel count
             ((ok[..., :2], "nhwc", "rgb"), "%s needs 3 channels in layout nhwc, got (2, 5, 7, 2)"),
             ((ok, "hwc", "rgb"), "layout must be one of ('nhwc', 'nchw')"),
             ((ok, "nhwc", "grb"), "order must be one of ('rgb', 'bgr')"),
             ((ok.float(), "hwc", "grb"), "layout must be one of ('nhwc', 'nchw')")]                        # the order of the checks
    for (tiles, layout, order), text in cases:
        for what, call in (("f", lambda: EX.tile_args(tiles, layout, order, "f")),
                           ("stain.fit", lambda: stain.fit(tiles, layout, order)),
                           ("stain.normalize", lambda: stain.normalize(tiles, stain.REFERENCE_TARGET, layout=layout, order=order)),
                           ("tile_stats", lambda: tissue.tile_stats(tiles, layout, order))):
            with pytest.raises(ValueError) as e:
                call()
            assert type(e.value) is ValueError and str(e.value) == (text % what if "%s" in text else text), (what, text)
    empty = torch.zeros((2, 0, 7, 3), dtype=torch.uint8)                       # each module keeps its own rule for H W = 0
    assert EX.tile_args(empty, "nhwc", "rgb", "f") == (2, 0, 7)
    with pytest.raises(ValueError, match="stain.fit needs H, W >= 1"):
        stain.fit(empty)
    with pytest.raises(ValueError, match="tile_stats needs 1 <= H W <= 2\\^26, got H 0 W 7"):
        tissue.tile_stats(empty)


def test_rgb_numpy_equals_the_four_views():
    rgb = np.random.default_rng(8).integers(0, 256, (2, 3, 5, 3), dtype=np.uint8)
    stored = {("nhwc", "rgb"): rgb, ("nhwc", "bgr"): rgb[..., ::-1], ("nchw", "rgb"): rgb.transpose(0, 3, 1, 2),
              ("nchw", "bgr"): rgb[..., ::-1].transpose(0, 3, 1, 2)}
    for (layout, order), a in stored.items():
        t = torch.from_numpy(np.ascontiguousarray(a))
        got = EX.rgb_numpy(t, layout, order)
        assert got.shape == (2, 3, 5, 3) and np.array_equal(got, rgb), (layout, order)
        assert np.shares_memory(got, t.numpy()), "a view, not a copy"


def test_a_ctypes_array_reaches_a_void_pointer_parameter():
    """what _abi.launch relies on for small host operands: no cast in front of a c_void_p parameter"""
    memcpy = ctypes.CDLL(None).memcpy
    memcpy.restype, memcpy.argtypes = ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    for ctype, values in ((ctypes.c_int, [3, -30000, 2 ** 31 - 1, -2 ** 31]), (ctypes.c_longlong, [1 << 40, -(1 << 40) - 1, 0, 7])):
        src, dst = (ctype * 4)(*values), (ctype * 4)()
        memcpy(dst, src, ctypes.sizeof(src))
        assert list(dst) == values


# ---------------------------------------------------------------------------------------------------------------- stored frames
def _sizes():
    header = len(pickle.dumps(("slide_patch_0", b"", (256, 256, 3))))
    return [0, 1, 65535, 65536, 65537, 196608 + header]


def test_stored_frames_round_trip():
    rng = np.random.default_rng(4)
    for n in _sizes():
        b = rng.bytes(n)
        f = PD.lz4f_compress(b, stored=True)
        assert PD.lz4f_decompress(f) == b
        blocks = (n + 65535) // 65536
        assert len(f) == 4 + 2 + 8 + 1 + 4 * blocks + n + 4            # magic, FLG BD, content size, HC, block sizes, data, EndMark
        assert f[:15] == PD.lz4f_compress(b)[:15] and f[6:14] == n.to_bytes(8, "little")        # same header, content size recorded
        pos = 15
        for k in range(blocks):
            size = int.from_bytes(f[pos:pos + 4], "little")
            assert size >> 31 == 1 and size & 0x7FFFFFFF == min(65536, n - 65536 * k)               # high bit: uncompressed
            pos += 4 + (size & 0x7FFFFFFF)
    z = bytes(100000)                                                   # compressible: only stored=True keeps it verbatim
    assert len(PD.lz4f_compress(z)) < 2000 < len(PD.lz4f_compress(z, stored=True))
    assert PD.lz4f_decompress(PD.lz4f_compress(z, block_size=1 << 18, stored=True)) == z


@needs_lz4
def test_liblz4_reads_stored_frames():
    rng = np.random.default_rng(5)
    for n in _sizes():
        b = rng.bytes(n)
        assert _lib_decompress_frame(PD.lz4f_compress(b, stored=True), n) == b
    tile = np.arange(32 * 32 * 3, dtype=np.uint8).reshape(32, 32, 3)
    name, raw, shape = pickle.loads(_lib_decompress_frame(PD.encode_record("s_patch_1", tile, stored=True), 1 << 16))
    assert name == "s_patch_1" and tuple(shape) == (32, 32, 3) and raw == tile.tobytes()


def test_default_records_keep_their_bytes():
    """stored=False is the default and writes what the parent wrote: digests taken from the code before the keyword existed."""
    rng = np.random.default_rng(3)
    tile = (rng.integers(0, 256, (40, 40, 3)) // 16 * 16).astype(np.uint8)
    rec = PD.encode_record("s_patch_0", tile)
    assert hashlib.sha256(rec).hexdigest() == "88288ed3aafd4039b3a2f93a1e806f6eb40b6be13daa5ff2fa17f3e6dd92290f"
    assert hashlib.sha256(PD.encode_keys(7)).hexdigest() == "564c911e3b03934003949c80db7eca5ce23c2d521d3d98326ca4c1d0cb5e349b"
    assert rec == PD.encode_record("s_patch_0", tile, stored=False) == PD.serialize_and_compress(("s_patch_0", tile.tobytes(), tile.shape),
                                                                                                 stored=False)
    b = rng.bytes(1000) + bytes(3000)
    assert PD.lz4f_compress(b) == PD.lz4f_compress(b, stored=False) != PD.lz4f_compress(b, stored=True)


def test_store_round_trip_rgb(tmp_path):
    rng = np.random.default_rng(6)
    tiles = rng.integers(0, 256, (5, 12, 10, 3), dtype=np.uint8)               # RGB HWC, as tiles_u8 delivers them
    path = str(tmp_path / "p0" / "p0")
    assert PD.write_tile_store(path, tiles, slide_id="p0", stored=True, channel_order="rgb") == 5
    store = PD.open_tile_store(path)
    assert isinstance(store, PD.DirStore) and len(store) == 6
    keys = pickle.loads(PD.lz4f_decompress(store[b"__keys__"]))
    assert keys == [b"0", b"1", b"2", b"3", b"4"]
    for i, k in enumerate(keys):
        img = PD.decompress_and_deserialize(store[k])
        assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), tiles[i].transpose(2, 0, 1))      # RGB CHW
        name, raw, shape = pickle.loads(PD.lz4f_decompress(store[k]))
        assert name == "p0_patch_%d" % i and raw == tiles[i][:, :, ::-1].tobytes() and tuple(shape) == (12, 10, 3)   # stored BGR
    # the default keeps today's behaviour: tiles are written as given, the reader reverses them
    d = str(tmp_path / "plain")
    PD.write_tile_store(d, tiles)
    got = PD.decompress_and_deserialize(PD.open_tile_store(d)[b"3"])
    assert np.array_equal(got.numpy(), tiles[3][:, :, ::-1].transpose(2, 0, 1))
    with open(os.path.join(d, "3"), "rb") as f:
        assert f.read() == PD.encode_record("slide_patch_3", tiles[3])
    with pytest.raises(ValueError):
        PD.write_tile_store(d, tiles, channel_order="gbr")
    # and through the dataset itself
    import pandas as pd
    table = pd.DataFrame({"wsi_file_name": ["p0"], "rna_0": [0.5], "patch_data_path": [str(tmp_path)], "labels": [0]})
    ds = PD.PatchDataset(str(tmp_path), table, 12, max_patches_total=5)
    assert len(ds) == 5
    for j in range(5):
        img, _ = ds[j]
        assert np.array_equal(img.numpy(), tiles[int(ds.keys[j])].transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------- ABI, CLI
def test_abi_prototype_present():
    i, p, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _abi.PROTOTYPES["rg_tile_export_u8"] == (i, [p, p, i, i, i, i, f, f, i, p])
    assert _abi.ABI_VERSION == 618
    header = open(os.path.join(ROOT, "include", "rnagan_hip.h")).read()
    assert "rg_tile_export_u8(" in header
    for name, value in (("RG_EXPORT_PLANAR", 1), ("RG_EXPORT_REVERSE", 2), ("RG_EXPORT_TRUNC", 4)):
        assert "#define %s %d" % (name, value) in header
    from rna_gan_amd import build
    assert "rg_export.hip" in build.SOURCES and "rg_export.hip" not in build.BF16_ONLY


def test_tile_groups():
    from rna_gan_amd.gan_utils import _tile_groups
    assert _tile_groups(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert _tile_groups(9, 4) == [(0, 4), (4, 9)]                       # a trailing single row joins the previous group
    assert _tile_groups(1, 4) == [(0, 1)] and _tile_groups(8, 4) == [(0, 4), (4, 8)] and _tile_groups(3, 4096) == [(0, 3)]


def test_cli_defaults_and_refusals(capsys):
    import generate_tissue_images as G
    a = G.parse_args(["--synthetic", "--patients", "all", "--tiles_per_patient", "4", "--out_dir", "o"])
    assert (a.out_format, a.quantize, a.chunk, a.group, a.seed, a.precision, a.g_ema, a.fp8, a.prepare_rna, a.rna_features,
            a.sample_size, a.random_patient) == ("store", "round", 512, 4096, 0, "bf16", 0, 0, 0, 19198, 64, False)
    a = G.parse_args(["--synthetic", "--random_patient", "--save_path", "g.png"])
    assert a.random_patient and a.patients is None and a.sample_size == 64
    a = G.parse_args(["--synthetic", "--patient1", "TCGA-1", "--tiles_per_patient", "2", "--out_dir", "o"])
    assert a.patients == "TCGA-1"
    a = G.parse_args(["--checkpoint", "c", "--rna_file", "r", "--vae_checkpoint", "v", "--random_patient", "--save_path", "g",
                      "--config", "x.json", "--checkpoint2", "c2", "--sample_size", "16", "--rna_features", "100"])
    assert (a.checkpoint, a.checkpoint2, a.rna_file, a.vae_checkpoint, a.config, a.sample_size, a.rna_features) == \
        ("c", "c2", "r", "v", "x.json", 16, 100)
    bulk = ["--synthetic", "--patients", "all", "--tiles_per_patient", "4", "--out_dir", "o"]
    rnd = ["--synthetic", "--random_patient", "--save_path", "g.png"]
    bad = [["--synthetic"],                                                                    # neither mode
           rnd + ["--patients", "all"], rnd + ["--patient1", "x"],                                # both modes
           ["--synthetic", "--random_patient"],                                                # no --save_path
           rnd + ["--sample_size", "1"], rnd + ["--sample_size", "65"],
           ["--synthetic", "--patients", "all", "--tiles_per_patient", "4"],                    # no --out_dir
           ["--synthetic", "--patients", "all", "--out_dir", "o"],                              # no --tiles_per_patient
           ["--synthetic", "--patients", " ", "--tiles_per_patient", "4", "--out_dir", "o"],
           bulk + ["--out_format", "lmdb"], bulk + ["--quantize", "floor"], bulk + ["--prepare_rna", "2"], bulk + ["--g_ema", "2"],
           bulk + ["--fp8", "-1"], bulk + ["--chunk", "0"], bulk + ["--group", "1"], bulk + ["--precision", "fp64"],
           bulk + ["--fp8", "1", "--precision", "fp32"], bulk + ["--rna_features", "0"], bulk + ["--img_size", "0"],
           bulk[1:],                                                                             # the three files are missing
           ["--checkpoint", "c", "--rna_file", "r"] + bulk[1:], ["--checkpoint", "c", "--vae_checkpoint", "v"] + bulk[1:],
           ["--rna_file", "r", "--vae_checkpoint", "v"] + bulk[1:]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            G.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    assert G.select_patients("all", ["a", "b", "c"]) == [0, 1, 2] and G.select_patients("c, a", ["a", "b", "c"]) == [2, 0]
    for spec in ("d", "a,a"):
        with pytest.raises(SystemExit):
            G.select_patients(spec, ["a", "b", "c"])
    g = G.compose_grid(np.full((3, 4, 5, 3), 7, dtype=np.uint8))
    assert g.shape == (32, 40, 3) and (g[:4, :15] == 7).all() and g[:4, 15:].max() == 0 and g[4:].max() == 0
