"""Stain normalisation without a GPU: the tables of the contract pinned, the monotonicity that lets the kernel search for the angle
bin, the percentile rule, StainFit, the argument handling of the two programs, rna_gan_amd.stain's numpy path against the
restatement of tests/stain_refs.py, and the agreement of the integer form with the fp64 textbook form of Macenko's method.

``python tests/test_stain_refs_cpu.py`` writes profiles/stain_textbook_agreement.txt; the test recomputes its figures.
No parity with staintools, torchstain or histomicstk is claimed: none of them was installed where this was written.
"""
import ast
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stain_refs as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PROFILE = os.path.join(ROOT, "profiles", "stain_textbook_agreement.txt")


# ------------------------------------------------------------------ tables
def test_tables_are_pinned_and_the_module_builds_the_same():
    from rna_gan_amd import stain
    od = R.od_lut()
    assert od.dtype == np.int32 and od.shape == (256,)
    assert [int(od[v]) for v in (0, 1, 119, 239, 240, 255)] == [22449, 19610, 2839, 0, -17, -264]
    assert np.all(np.diff(od) < 0) and int(np.abs(od).max()) <= 23170            # the bound the kernels' int32 quad sums rest on
    assert R.BETA_Q == 614 == stain.beta_q()
    assert np.array_equal(od, stain.od_table())
    table, off = R.out_lut()
    assert (len(table), off, int(table[0]), int(table[1]), int(table[off]), int(table[-2]), int(table[-1])) == (1598, 16, 255, 254, 240, 1, 0)
    assert np.all(np.diff(table.astype(int)) <= 0) and len(table) <= 8192
    mt, moff = stain.output_table()
    assert moff == off and np.array_equal(mt, table) and mt.dtype == np.uint8
    d = R.dirs()
    assert d.shape == (R.K - 1, 2) and np.array_equal(d, stain.direction_table())
    assert d[0].tolist() == [50, -16384] and d[R.K // 2 - 1].tolist() == [16384, 0] and d[-1].tolist() == [50, 16384]
    assert np.array_equal(d[::-1, 0], d[:, 0]) and np.array_equal(d[::-1, 1], -d[:, 1])
    assert (R.K, R.QP, R.CB, R.CSH, R.SHIFT) == (stain.K, stain.QP, stain.CB, stain.CSH, stain.QH + stain.QOD - stain.QO)
    assert (stain.IO, stain.BETA, stain.ALPHA, stain.QOD, stain.QV, stain.QS, stain.QH, stain.QO) == (240, 0.15, 1, 12, 14, 16, 14, 8)


def test_bin_predicate_is_monotone_so_binary_search_equals_the_count():
    """For p1 > 0 the predicate cos_k p2 - sin_k p1 >= 0 says that p lies on or counter-clockwise of direction k.  Every quantised
    direction has cos_k > 0 and consecutive ones are STRICTLY counter-clockwise of each other (positive cross product): inside the
    half-plane x > 0 the angular order is total, so once the predicate fails at k it fails at every later k.  Checked over the whole
    table, then binary search against the count on random pixels and on pixels exactly on and next to a direction."""
    from rna_gan_amd import stain
    for k in (R.K, 2, 3, 4, 2048):
        d = R.dirs(k).astype(np.int64)
        assert np.all(d[:, 0] > 0)
        assert np.all(d[:-1, 0] * d[1:, 1] - d[:-1, 1] * d[1:, 0] > 0)
    d = R.dirs()
    rng = np.random.default_rng(0)
    p1 = rng.integers(1, 1 << 30, 3000)
    p2 = rng.integers(-(1 << 30), 1 << 30, 3000)
    ks = rng.integers(0, R.K - 1, 600)
    m = rng.integers(1, 60000, 600)
    on1, on2 = d[ks, 0].astype(np.int64) * m, d[ks, 1].astype(np.int64) * m                # exactly on direction k: the >= counts it
    p1 = np.concatenate([p1, on1, on1, on1, [1, 1, 1, 1 << 30, 1 << 30]])
    p2 = np.concatenate([p2, on2, on2 + 1, on2 - 1, [0, 1 << 30, -(1 << 30), 1 << 30, -(1 << 30)]])
    count = R.angle_bin_count(p1, p2, d)
    assert count.min() == 0 and count.max() == R.K - 1
    assert np.array_equal(count, np.array([R.angle_bin_search(a, b, d) for a, b in zip(p1, p2)]))
    assert np.array_equal(count, stain._angle_bins_numpy(p1.astype(np.int64), p2.astype(np.int64), d))
    assert np.array_equal(count[3000:3600], ks + 1)                                        # on direction k (1-based k + 1): bin k + 1
    # the float angle falls into the same bin, away from the bin edges
    phi = np.arctan2(p2[:3000].astype(np.float64), p1[:3000].astype(np.float64))
    pos = (phi + np.pi / 2) / (np.pi / R.K)
    clear = np.abs(pos - np.rint(pos)) > 0.05
    assert np.array_equal(count[:3000][clear], np.floor(pos[clear]).astype(np.int64))


def test_percentile_rule_on_hand_made_histograms():
    from rna_gan_amd import stain
    for f in (stain.histogram_percentile, R.percentile_bin):
        assert f([0, 0, 5, 0], 0) == 2 and f([0, 0, 5, 0], 100) == 2
        h = [1] * 100                                       # rank = q * 99 // 100
        assert [f(h, q) for q in (0, 1, 2, 50, 99, 100)] == [0, 0, 1, 49, 98, 99]
        h = [10, 0, 0, 90, 0, 1]                            # total 101: rank = q
        assert [f(h, q) for q in (0, 9, 10, 99, 100)] == [0, 0, 3, 3, 5]
        assert f([3], 99) == 0
        assert f(np.array([2 ** 40, 1], dtype=np.int64), 99) == 0 and f(np.array([1, 2 ** 40], dtype=np.int64), 1) == 1
    with pytest.raises(ValueError):
        stain.histogram_percentile([0, 0], 50)
    with pytest.raises(ValueError):
        stain.histogram_percentile([1], 1.5)
    assert stain.angle_of_bin(0) == -np.pi / 2 + 0.5 * np.pi / 1024 and stain.conc_of_bin(3) == 3.5 * 8 / 4096


# ------------------------------------------------------------------ StainFit
def test_stainfit_json_round_trip_and_the_reference_target():
    from rna_gan_amd import stain
    f = stain.StainFit([[0.1 + 1e-17, 0.2], [1 / 3, 0.4], [0.5, 2 / 3]], [1.2345678901234567, 0.7], 10, 7, 2)
    g = stain.StainFit.from_json(f.to_json())
    assert g == f and g.he.shape == (3, 2) and g.he.dtype == np.float64 and (g.n_pixels, g.n_stained, g.n_outside) == (10, 7, 2)
    assert stain.StainFit.from_json(stain.stain_report(f, stain.REFERENCE_TARGET, True)) == f            # a stain.json names the fit
    rep = json.loads(stain.stain_report(None, stain.REFERENCE_TARGET, False, "why"))
    assert rep["normalized"] is False and rep["fit"] is None and rep["message"] == "why" and rep["method"] == "macenko"
    t = stain.REFERENCE_TARGET
    assert t.he.tolist() == [[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]] and t.max_conc.tolist() == [1.9705, 1.0308]
    assert stain.load_target("reference") is t and f != t


def test_sets_that_cannot_be_fitted_raise_with_the_counts():
    from rna_gan_amd import stain
    white = torch.full((2, 8, 8, 3), 255, dtype=torch.uint8)
    with pytest.raises(stain.StainFitError) as e:
        stain.fit(white)
    assert e.value.counts == {"n_pixels": 128, "n_stained": 0} and "128" in str(e.value)
    few = white.clone()
    few.view(-1, 3)[:15] = torch.tensor([60, 30, 90], dtype=torch.uint8)            # 15 stained pixels: one short
    with pytest.raises(stain.StainFitError) as e:
        stain.fit(few)
    assert e.value.counts["n_stained"] == 15
    flat = torch.empty((1, 8, 8, 3), dtype=torch.uint8)
    flat[...] = torch.tensor([60, 30, 90], dtype=torch.uint8)                  # one colour: a zero covariance
    with pytest.raises(stain.StainFitError, match="rank-deficient"):
        stain.fit(flat)
    line = flat.clone()
    line[0, :4] = torch.tensor([30, 12, 51], dtype=torch.uint8)                # two colours: rank one
    with pytest.raises(stain.StainFitError, match="rank-deficient"):
        stain.fit(line)
    with pytest.raises(stain.StainFitError):
        stain.fit(torch.empty((0, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(stain.StainFitError):
        stain.normalize(white, stain.StainFit(stain.REFERENCE_TARGET.he, [0.0, 1.0]))
    assert issubclass(stain.StainFitError, ValueError)
    for bad in (white.float(), white[0], white[..., :2]):
        with pytest.raises(ValueError):
            stain.fit(bad)
    with pytest.raises(ValueError):
        stain.fit(white, layout="hwc")
    with pytest.raises(ValueError):
        stain.normalize(white, stain.REFERENCE_TARGET, out=torch.empty(3, dtype=torch.uint8))


# ------------------------------------------------------------------ the numpy path of the module against the restatement
@pytest.mark.parametrize("layout,order", [("nhwc", "rgb"), ("nhwc", "bgr"), ("nchw", "rgb"), ("nchw", "bgr")])
def test_module_numpy_path_equals_the_restatement(layout, order):
    from rna_gan_amd import stain
    rgb = R.synthetic_set(3, stains=1, n=3, size=40)
    want = R.fit(rgb.reshape(-1, 3))
    tiles = torch.from_numpy(R.store_as(rgb, layout, order))
    f = stain.fit(tiles, layout, order)
    assert np.array_equal(f.he, want["he"]) and np.array_equal(f.max_conc, want["max_conc"])
    assert (f.n_pixels, f.n_stained, f.n_outside) == (rgb.size // 3, want["n_stained"], want["n_outside"])
    assert stain.fit(tiles, layout, order, batch=2) == f and stain.fit(tiles, layout, order, batch=1) == f
    t = stain.REFERENCE_TARGET
    ops = R.operands(want["he"], want["max_conc"], t.he, t.max_conc)
    assert stain.apply_operands(f, t) == tuple(ops) and stain.quantize_pinv(f.he) == want["pinv6"]
    y = R.apply(rgb.reshape(-1, 3), *ops).reshape(rgb.shape)
    out = stain.normalize(tiles, f, layout=layout, order=order)
    assert out.shape == tiles.shape and out.dtype == torch.uint8
    assert np.array_equal(R.rgb_of(out.numpy(), layout, order).reshape(rgb.shape), y)
    got, f2 = stain.normalize_tiles(tiles, layout=layout, order=order)
    assert f2 == f and torch.equal(got, out)
    same = tiles.clone()
    assert stain.normalize(same, f, out=same, layout=layout, order=order) is same and torch.equal(same, out)
    # the passes one by one
    px = rgb.reshape(-1, 3)
    assert np.array_equal(stain._moments_numpy(rgb), want["moments"])
    assert np.array_equal(stain._angle_hist_numpy(rgb, want["basis6"], stain.direction_table()), want["angle_hist"])
    assert np.array_equal(stain._conc_hist_numpy(rgb, want["pinv6"]), want["conc_hist"])
    assert int(want["conc_hist"].sum()) == 2 * px.shape[0] and int(want["angle_hist"].sum()) == want["n_stained"]


# ------------------------------------------------------------------ the boundary
def test_prototypes_and_header():
    from rna_gan_amd import _abi
    i, p = _abi._i, _abi._p
    assert _abi.PROTOTYPES["rg_stain_moments"] == (i, [p, i, i, i, i, p, i, p, i, p])
    assert _abi.PROTOTYPES["rg_stain_angle_hist"] == (i, [p, i, i, i, i, p, i, p, p, i, p, i, p])
    assert _abi.PROTOTYPES["rg_stain_conc_hist"] == (i, [p, i, i, i, i, p, p, i, i, i, p, i, p])
    assert _abi.PROTOTYPES["rg_stain_apply"] == (i, [p, p, i, i, i, i, p, p, i, p, i, p, i, p, i, i, p])
    assert _abi.ABI_VERSION == 618
    header = open(os.path.join(ROOT, "include", "rnagan_hip.h")).read()
    for name in ("rg_stain_moments", "rg_stain_angle_hist", "rg_stain_conc_hist", "rg_stain_apply"):
        assert "int %s(const uint8_t* " % name in header
    from rna_gan_amd import build, stain
    assert "rg_stain.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "rna_gan_amd", "csrc", "rg_stain.hip")).read()
    assert "SN_CHUNK = %d;" % stain.STAT_CHUNK in src and "SN_APPLY_CHUNK = %d;" % stain.APPLY_CHUNK in src
    for half in ("bf16", "f16"):                    # host-side refusals need no device: nothing is launched
        lib = _abi.load(half)
        assert lib.rg_stain_moments(None, 1, 4, 4, 0, None, 614, None, 0, None) == -1
        assert lib.rg_stain_moments(0x1000, (1 << 31) - 1, 8, 1, 0, 0x1000, 614, 0x1000, 0, None) == -2
        assert b"2^33" in lib.rg_last_error()
        assert lib.rg_stain_moments(0x1000, 0, 8, 1, 0, 0x1000, 614, 0x1000, 0, None) == 0


# ------------------------------------------------------------------ the programs
def test_tile_slides_arguments(tmp_path):
    import tile_slides
    base = ["--patch_path", "p", "--mask_path", "m", "--synthetic"]
    a = tile_slides.parse_args(base)
    assert a.stain_norm == "none" and a.stain_target == "reference"
    a = tile_slides.parse_args(base + ["--stain_norm", "macenko"])
    assert a.stain_norm == "macenko" and a.stain_target == "reference"
    from rna_gan_amd import stain
    f = tmp_path / "target.json"
    f.write_text(stain.StainFit([[0.6, 0.1], [0.7, 0.9], [0.3, 0.2]], [1.5, 0.9], 5, 4, 0).to_json())
    a = tile_slides.parse_args(base + ["--stain_norm", "macenko", "--stain_target", str(f)])
    assert stain.load_target(a.stain_target).max_conc.tolist() == [1.5, 0.9]
    for bad in (["--stain_norm", "reinhard"], ["--stain_norm", "macenko", "--stain_target", str(tmp_path / "missing.json")],
                ["--stain_target", str(f)]):
        with pytest.raises(SystemExit):
            tile_slides.parse_args(base + bad)


def test_stain_norm_none_touches_no_stain_code():
    """Without a GPU, by parsing: in tile_slides.run every use of the stain module, the target and the fit sits inside an
    ``if args.stain_norm == "macenko":`` block, and the default of the flag is none."""
    import tile_slides
    tree = ast.parse(open(os.path.join(ROOT, "tile_slides.py")).read())
    run = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run")
    guards = [n for n in ast.walk(run) if isinstance(n, ast.If) and ast.unparse(n.test) == "args.stain_norm == 'macenko'"]
    assert len(guards) == 2 and all(not g.orelse for g in guards)
    spans = [(g.body[0].lineno, g.body[-1].end_lineno) for g in guards]
    uses = [n for n in ast.walk(run) if isinstance(n, ast.Name) and n.id in ("stain", "target", "fitted", "message")]
    assert len(uses) >= 8
    for n in uses:
        assert any(lo <= n.lineno <= hi for lo, hi in spans), "line %d uses %s outside the macenko blocks" % (n.lineno, n.id)
    assert not any(isinstance(n, (ast.Import, ast.ImportFrom)) and "stain" in ast.unparse(n) for n in tree.body)
    assert tile_slides.parse_args(["--patch_path", "p", "--mask_path", "m", "--synthetic"]).stain_norm == "none"


def test_stain_normalize_arguments_and_store_round_trip(tmp_path):
    import stain_normalize
    from rna_gan_amd.data import decompress_and_deserialize, open_tile_store
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    a = stain_normalize.parse_args(["--patch_path", src, "--out_path", out])
    assert (a.stain_target, a.batch, a.synthetic, a.device) == ("reference", 256, False, 0)
    for bad in ([], ["--patch_path", src], ["--patch_path", src, "--out_path", src], ["--patch_path", src, "--out_path", out, "--batch", "0"],
                ["--patch_path", src, "--out_path", out, "--stain_target", str(tmp_path / "none.json")],
                ["--patch_path", str(tmp_path / "absent"), "--out_path", out]):
        with pytest.raises(SystemExit):
            stain_normalize.parse_args(bad)
    assert stain_normalize.parse_args(["--patch_path", str(tmp_path / "absent"), "--out_path", out, "--synthetic"]).synthetic
    # the store helpers, without a device: what is read is what was written, names and channel order included
    stain_normalize.write_synthetic(src, slides=2, tiles=3, size=16)
    stores = stain_normalize.list_stores(src)
    assert [(s, n) for s, n, _ in stores] == [("synthetic_0.svs", "synthetic_0.db"), ("synthetic_1.svs", "synthetic_1.db")]
    names, tiles = stain_normalize.read_store(stores[0][2])
    assert names == ["synthetic_0.svs_patch_%d" % k for k in range(3)] and tiles.shape == (3, 16, 16, 3)
    copy = os.path.join(out, "synthetic_0.svs", "synthetic_0.db")
    os.makedirs(os.path.dirname(copy))
    stain_normalize.write_store(copy, names, tiles)
    a, b = open_tile_store(stores[0][2]), open_tile_store(copy)
    assert all(a[k] == b[k] for k in (b"0", b"1", b"2", b"__keys__"))
    rgb = decompress_and_deserialize(b[b"1"]).permute(1, 2, 0).numpy()
    assert np.array_equal(rgb, tiles[1][:, :, ::-1])                     # the records hold B, G, R


# ------------------------------------------------------------------ agreement with the textbook form
def measure_agreement():
    """Over AGREEMENT_SEEDS x the two source stain matrices: fit and normalise to the published target with the integer form
    (rna_gan_amd.stain's numpy path, equal to the restatement) and with the fp64 textbook form -> rows and totals."""
    from rna_gan_amd import stain
    t = stain.REFERENCE_TARGET
    rows, worst, differing, total = [], 0, 0, 0
    for s in range(len(R.SOURCE_STAINS)):
        for seed in R.AGREEMENT_SEEDS:
            rgb = R.synthetic_set(seed, s)
            tiles = torch.from_numpy(rgb)
            f = stain.fit(tiles)
            y = stain.normalize(tiles, f).numpy().reshape(-1, 3).astype(np.int64)
            he, mc = R.textbook_fit(rgb.reshape(-1, 3))
            ty = R.textbook_apply(rgb.reshape(-1, 3), he, mc, t.he, t.max_conc).astype(np.int64)
            d = np.abs(y - ty)
            rows.append((s, seed, int(d.max()), float((d > 0).mean()), float(np.abs(he - f.he).max()),
                         float(np.abs(f.max_conc / mc - 1).max())))
            worst, differing, total = max(worst, int(d.max())), differing + int((d > 0).sum()), total + d.size
    return rows, worst, differing / total


def agreement_text(rows, worst, share):
    lines = ["# integer form (rna_gan_amd.stain) against the fp64 textbook form (tests/stain_refs.py), normalised to the published target",
             "# sets: 8 x 64 x 64 Beer-Lambert tiles, gamma concentrations, 25 %% background, sigma 1.5 noise; seeds %d..%d, two stain matrices"
             % (R.AGREEMENT_SEEDS[0], R.AGREEMENT_SEEDS[-1]),
             "# written by python tests/test_stain_refs_cpu.py",
             "stains seed max_byte_diff share_differing max_abs_diff_HE max_rel_diff_max_conc"]
    lines += ["%d %d %d %.4f %.2e %.2e" % r for r in rows]
    lines += ["largest byte difference %d" % worst, "share of differing bytes %.4f (recorded, not gated)" % share,
              "gate of the tests: %d (the largest difference + 1)" % (worst + 1)]
    return "\n".join(lines) + "\n"


def test_integer_form_agrees_with_the_textbook_form():
    rows, worst, share = measure_agreement()
    print("largest byte difference %d, share of differing bytes %.4f" % (worst, share))
    assert len(rows) >= 40
    assert worst <= R.TEXTBOOK_GATE
    assert max(r[4] for r in rows) < 5e-3 and max(r[5] for r in rows) < 1e-2        # stain vectors to ~1e-3, max_conc to ~0.5 %
    recorded = open(PROFILE).read()
    assert "largest byte difference %d\n" % R.TEXTBOOK_MEASURED in recorded            # the gate rests on the recorded figure


if __name__ == "__main__":
    text = agreement_text(*measure_agreement())
    with open(PROFILE, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
