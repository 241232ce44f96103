"""The host-side launch planner, pinned row by row: what rg_conv_split / rg_conv_slab_dtype / rg_conv_stats_rows /
rg_conv_workspace_bytes / rg_conv_up_maskbits_supported / rg_conv_wgrad_workspace_bytes / rg_conv_wgrad_adam_supported (and
the two linear workspace queries that share the planner) answer for a grid of shapes, in both builds and under the
kernel-selection options, against tests/golden/conv_plans.json.  That table was recorded from the planner as it stood BEFORE
the queries and the launchers were made to read one plan struct (tests/golden/make_plan_fixture.py; never regenerated from
the code under test).  The queries are host code: no GPU is needed."""
import importlib.util
import json
import os

import pytest

from rna_gan_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_plan_fixture", os.path.join(GOLDEN, "make_plan_fixture.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "conv_plans.json")) as f:
        return json.load(f)


def _lib(half):
    path = _abi.LIB_PATH if half == "bf16" else _abi.LIB_PATH_F16
    if not os.path.exists(path):
        from rna_gan_amd.build import build_library
        build_library(half=half)
    return _abi.load(half)


def _expected(build, setting):
    """The recorded tables of one setting: the default rows with the setting's differing rows put in."""
    want = {t: [list(r) for r in build["default"][t]] for t in gen.TABLES}
    if setting != "default":
        for t in gen.TABLES:
            for i, row in build["diff"][setting][t].items():
                want[t][int(i)] = row
    return want


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_every_plan_query_answers_as_recorded(recorded, half):
    lib = _lib(half)
    build = recorded["builds"][half]
    assert sorted(build["diff"]) == sorted(n for n, _ in gen.SETTINGS[1:])
    for name, options in gen.SETTINGS:
        got = gen.query_setting(lib, half, options)
        want = _expected(build, name)
        for t in gen.TABLES:
            assert len(got[t]) == len(want[t]) == len(gen.shapes(t)), (half, name, t)
            for i, (g, w) in enumerate(zip(got[t], want[t])):
                assert g == w, "%s build, options %s, table %s, row %d %r: got %r, recorded %r (columns %r)" % (
                    half, name, t, i, gen.shapes(t)[i], g, w,
                    {"conv": gen.CONV_COLUMNS, "wgrad": gen.WGRAD_COLUMNS}.get(t, ("workspace_bytes",)))
    # every option was cleared again: the default answers are back
    assert gen.query_setting(lib, half, {}) == _expected(build, "default")


def test_the_recorded_table_exercises_the_planner(recorded):
    """The fixture itself: it must reach every kind of plan, or equality with it says little."""
    assert os.path.getsize(os.path.join(GOLDEN, "conv_plans.json")) < 200 * 1024
    bf16 = recorded["builds"]["bf16"]
    conv, wgrad = bf16["default"]["conv"], bf16["default"]["wgrad"]
    shapes = gen.shapes("conv")
    assert len(conv) == len(shapes) == 840 and len(wgrad) == len(gen.shapes("wgrad")) == 420
    split, slab_dtype, stats_rows, ws_bytes, maskbits = (gen.CONV_COLUMNS.index(c) for c in gen.CONV_COLUMNS)
    # what the issue that asked for this test measured on the planner before the refactor
    assert [sum(r[split] == s for r in conv) for s in (1, 2, 4, 8)] == [543, 129, 87, 81]
    assert sum(r[slab_dtype] != _abi.RG_F32 for r in conv) == 170
    assert all(r[slab_dtype] == _abi.RG_BF16 and r[split] > 1 for r in conv if r[slab_dtype] != _abi.RG_F32)
    assert sum(r[stats_rows] > 0 for r in conv) == 412
    assert sum(r[maskbits] == 1 for r in conv) == 18
    assert all(r[ws_bytes] > 0 for r in conv if r[split] > 1)
    assert [sum(r[k] == 1 for r in wgrad) for k in (1, 2)] == [31, 33]
    assert len({r[0] for r in wgrad}) > 10                  # (workspace bytes: many different plans, not one constant)
    changed = {n: sum(len(d[t]) for t in gen.TABLES) for n, d in bf16["diff"].items()}
    for name, rows in (("conv8=0", 229), ("conv8=1", 170), ("convp=0", 18), ("convd=0", 3), ("slab16=0", 170),
                       ("conv_v1=1", 748), ("conv8_blocks=512", 71), ("wgrad8=0", 39), ("wgrad8_blocks=512", 124)):
        assert changed[name] == rows, (name, changed[name])
    assert changed["conv8=0,conv_tile=0"] > 0 and changed["conv8=0,conv_tile=5"] > 0
    assert bf16["diff"]["conv8=0,conv_tile=0"] != bf16["diff"]["conv8=0,conv_tile=5"] != bf16["diff"]["conv8=0"]
    # behind the 2 GB guard (N = 256, 256 x 256 input of 64 channels = 2^31 bytes): the legacy kernel -- no split, no
    # statistics, and the same answer whether or not conv_v1 forces that kernel; its neighbour at N = 128 is a planned launch
    for n, guarded in ((256, True), (128, False)):
        i = shapes.index(dict(up=0, N=n, low=128, O=128, I=64))
        assert (conv[i][split] == 1 and conv[i][stats_rows] == 0) == guarded, conv[i]
        assert (str(i) not in bf16["diff"]["conv_v1=1"]["conv"]) == guarded
    # the fp16 build: the same plans, except that its split-K slabs stay fp32
    f16 = recorded["builds"]["f16"]
    assert all(r[slab_dtype] == _abi.RG_F32 for r in f16["default"]["conv"])
    assert [r[:slab_dtype] + r[slab_dtype + 1:] for r in f16["default"]["conv"]] == \
           [r[:slab_dtype] + r[slab_dtype + 1:] for r in conv]
    assert f16["default"]["wgrad"] == wgrad and sum(len(d) for d in f16["diff"]["slab16=0"].values()) == 0
