"""rg_ema_update (include/rnagan_hip.h) op by op through ctypes, on both builds of the library, bit for bit against the numpy
reference of tests/ema_refs.py (pinned without a GPU by tests/test_ema_refs_cpu.py).

The average e lives inside a SENTINEL-filled allocation (a write outside [e, e + n) changes the pattern), the parameters p inside
a NaN-filled one (a read outside [p, p + n) makes a result non-finite); both overruns stay inside the allocations, so nothing
can fault.  Sizes: every path of the launch plan -- scalar tail only (1, 3), one vector and a tail (4, 5), less than a
workgroup (255), whole workgroups (1024), whole workgroups and a tail (1027), and two full passes of the capped grid plus a tail
(2 x 2048 workgroups x 256 threads x 4 elements + 3: the grid-stride loop runs twice for every thread)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from ema_refs import ema_update_ref
from guarded import Guarded, SBITS
from vae_fid_refs import SENTINEL

GRID_PASS = 2048 * 256 * 4
SIZES = [1, 3, 4, 5, 255, 1024, 1027, 2 * GRID_PASS + 3]
AFTER = 8192


def _special(n):
    """+-0, fp32 denormals and +-large values whose update stays finite (same-sign neighbours at 3e38, opposite signs at 1e37)."""
    p = np.array([0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1e-45, 1.0, 3e38, -3e38, 1e37, -1e37, 3.4e38, 1e-38],
                 dtype=np.float32)
    e = np.array([0.0, 0.0, -0.0, -0.0, -1e-45, 1e-45, 3e-39, 1e-45, 1.0, 1e-45, 2.5e38, -3.4e38, -1e37, 1e37, 3.4e38, -1e-38],
                 dtype=np.float32)
    reps = -(-n // p.size)
    return np.tile(p, reps)[:n].copy(), np.tile(e, reps)[:n].copy()


_DATA = {}


def _data(n, kind):
    """(p, e) as numpy float32, computed once per (n, kind) and never modified."""
    if (n, kind) not in _DATA:
        if kind == "special":
            p, e = _special(n)
        else:
            g = torch.Generator().manual_seed(1000 + n % 997)
            p = torch.randn(n, generator=g).numpy()
            e = torch.randn(n, generator=g).numpy()
        p.setflags(write=False); e.setflags(write=False)
        _DATA[(n, kind)] = (p, e)
    return _DATA[(n, kind)]


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _nan_surroundings(g):
    head, tail = g.flat[:g.before], g.flat[g.before + g.n:]
    return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())


def _call(lib, p, e, n, decay, step_dev=None, hyper=None, p_off=0, e_off=0):
    return lib.rg_ema_update(None if p is None else p.t.data_ptr() + p_off, None if e is None else e.t.data_ptr() + e_off, n,
                             decay, None if step_dev is None else step_dev.data_ptr(),
                             None if hyper is None else hyper.data_ptr(), None)


def _run(lib, n, kind, decay, t, hyper_word=None):
    p_np, e_np = _data(n, kind)
    p = Guarded(torch.from_numpy(p_np.copy()), float("nan"), after=AFTER)
    e = Guarded(torch.from_numpy(e_np.copy()), SENTINEL, after=AFTER)
    step_dev = None if t is None else torch.tensor([t], dtype=torch.int32, device="cuda")
    hyper = None
    if hyper_word is not None:
        hyper = torch.full((12,), float("nan"), device="cuda")     # only hyper[9] may be read
        hyper[9] = hyper_word
    rc = _call(lib, p, e, n, decay, step_dev, hyper)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert e.surroundings_keep(SBITS), "rg_ema_update wrote outside [e, e + n)"
    assert _nan_surroundings(p) and np.array_equal(_bits(p.t.cpu().numpy()), _bits(p_np)), "rg_ema_update wrote to p"
    if step_dev is not None:
        assert int(step_dev.item()) == t
    return e.t.cpu().numpy(), p_np, e_np


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("n", SIZES)
def test_bit_exact(half, kind, n):
    lib = _abi.load(half)
    # every decay with every warm-up state at the small sizes; the 4.2 M-element size (the second pass of the grid-stride loop)
    # with one plain and one warmed-up case
    cases = [(d, t) for d in (0.5, 0.999, 0.9999) for t in (None, 1, 8, 26, 10 ** 6)] if n < GRID_PASS else \
        [(0.999, None), (0.9999, 26)]
    for decay, t in cases:
        got, p_np, e_np = _run(lib, n, kind, decay, t)
        want = ema_update_ref(p_np, e_np, decay, t)
        assert np.isfinite(want).all()
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, "decay %g t %s: %d of %d elements differ, first at %d: got %r want %r (p %r e %r)" % (
            decay, t, bad.size, n, bad[0], got[bad[0]], want[bad[0]], p_np[bad[0]], e_np[bad[0]])
        if kind == "normal" and n >= 4:
            assert not np.array_equal(_bits(got), _bits(e_np))     # the update happened


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("n", [5, 1027])
def test_skip_word(half, n):
    lib = _abi.load(half)
    for t in (None, 8):
        got, p_np, e_np = _run(lib, n, "normal", 0.999, t, hyper_word=1.0)
        assert np.array_equal(_bits(got), _bits(e_np)), "a skipped step moved the average"
        want = ema_update_ref(p_np, e_np, 0.999, t)
        got, _, _ = _run(lib, n, "normal", 0.999, t, hyper_word=0.0)
        assert np.array_equal(_bits(got), _bits(want))
        got, _, _ = _run(lib, n, "normal", 0.999, t, hyper_word=None)          # hyper == NULL: never skipped
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_rejected_arguments_launch_nothing(half):
    lib = _abi.load(half)
    n = 1027
    p_np, e_np = _data(n, "normal")
    p = Guarded(torch.from_numpy(p_np.copy()), float("nan"), after=AFTER)
    e = Guarded(torch.from_numpy(e_np.copy()), SENTINEL, after=AFTER)
    bad_calls = {
        "decay = 1": lambda: _call(lib, p, e, n, 1.0),
        "decay < 0": lambda: _call(lib, p, e, n, -0.25),
        "decay = NaN": lambda: _call(lib, p, e, n, float("nan")),
        "e off by 4 bytes": lambda: _call(lib, p, e, n - 1, 0.5, e_off=4),
        "p off by 4 bytes": lambda: _call(lib, p, e, n - 1, 0.5, p_off=4),
        "e = NULL": lambda: _call(lib, p, None, n, 0.5),
        "p = NULL": lambda: _call(lib, None, e, n, 0.5),
    }
    for what, fn in bad_calls.items():
        assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0      # (a good call in between: the message is this call's)
        rc = fn()
        torch.cuda.synchronize()
        assert rc != 0, what
        msg = lib.rg_last_error()
        assert msg and b"ema_update" in msg, (what, msg)
        assert np.array_equal(_bits(e.t.cpu().numpy()), _bits(e_np)), what
        assert e.surroundings_keep(SBITS), what
        assert np.array_equal(_bits(p.t.cpu().numpy()), _bits(p_np)), what


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_n_zero_is_a_no_op(half):
    lib = _abi.load(half)
    p_np, e_np = _data(5, "normal")
    e = Guarded(torch.from_numpy(e_np.copy()), SENTINEL, after=AFTER)
    p = Guarded(torch.from_numpy(p_np.copy()), float("nan"), after=AFTER)
    assert _call(lib, p, e, 0, 0.5) == 0
    assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0          # no buffer is needed for nothing
    assert _call(lib, p, e, 0, 0.5, e_off=4) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(e.t.cpu().numpy()), _bits(e_np)) and e.surroundings_keep(SBITS)
