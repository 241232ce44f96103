"""The optimizer-step kernels (include/rnagan_hip.h: rg_adam_hyper_dev / _dev2 / _dev3, rg_adam_step_dev and its scalar form,
rg_adam_step, rg_adam_step_slabs, rg_grad_to_wire, and the Adam epilogues of rg_g0_wgrad_adam / rg_linear_wgrad_adam /
rg_conv_wgrad_adam) op by op through ctypes, on both builds of the library, BIT FOR BIT against the numpy restatements of
tests/adam_refs.py (pinned without a GPU by tests/test_adam_refs_cpu.py).

Everything a kernel writes (p, m, v, shadow, wire, hyper, the step counter) lives inside a SENTINEL-filled allocation: a write
outside the range changes the pattern.  Everything it only reads (g, the wire it reads, the slabs) lives inside a NaN-filled one:
a read outside the range makes a result non-finite.  Both overruns stay inside the allocations, so nothing can fault.  Every step
kernel test writes the REFERENCE's hyper values into the device buffer (the one-ulp allowance of the device's double pow / sqrt
stays in the hyper tests); one test chains the product's pairing hyper launch -> step launch on the read-back values."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from adam_refs import (F32, HYPER, SLAB_NSPLITS, adam_hyper_ref, adam_table_ref, adam_upd_ref, normal_inputs, round_h16_ref,
                       slab_inputs, slab_inputs_h16, special_inputs, widen_h16_ref, wire_table_ref)
from guarded import DEV, Guarded, SBITS
from vae_fid_refs import SENTINEL

HALVES = ["bf16", "f16"]
AFTER = 4096
S16 = 0x5E59                                        # the 16-bit sentinel (a finite value in both types)
NAN16 = 0x7FFF                                      # a NaN in both 16-bit types
NAN = float("nan")
GRID_PASS = 8192 * 256 * 4                          # elements one pass of rg_adam_step_dev's capped grid covers
SIZES = [1, 3, 4, 5, 255, 1024, 1027]
BIG = 2 * GRID_PASS + 3
TORCH16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def _h16code(half):
    return _abi.RG_F16 if half == "f16" else _abi.RG_BF16


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32buf(a, fill, after=AFTER):
    return Guarded(torch.from_numpy(np.array(a, dtype=np.float32)), fill, after=after)


def _get(gd):
    return gd.t.cpu().numpy().reshape(-1)


def _nan_around(gd):
    head, tail = gd.flat[:gd.before], gd.flat[gd.before + gd.n:]
    return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())


class G16:
    """tests/guarded.py's Guarded for a 16-bit buffer, given and read back as bits (uint16)."""

    def __init__(self, bits, fill, before=128, after=AFTER):
        bits = np.asarray(bits, dtype=np.uint16).reshape(-1)
        flat = np.full(before + bits.size + after, fill, dtype=np.uint16)
        flat[before:before + bits.size] = bits
        self.flat = torch.from_numpy(flat.view(np.int16)).to(DEV)
        self.before, self.n, self.fill = before, bits.size, fill

    def ptr(self, off=0):
        return self.flat.data_ptr() + 2 * (self.before + off)

    def get(self):
        return self.flat[self.before:self.before + self.n].cpu().numpy().view(np.uint16)

    def surroundings_keep(self):
        h = self.flat.cpu().numpy().view(np.uint16)
        return bool((h[:self.before] == self.fill).all()) and bool((h[self.before + self.n:] == self.fill).all())


def _same(what, got, want, as16=False):
    g = np.asarray(got).view(np.uint16) if as16 else _u32(got)
    w = np.asarray(want).view(np.uint16) if as16 else _u32(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r (%#x) want %r (%#x)" % (
        what, bad.size, g.size, bad[0], np.asarray(got).reshape(-1)[bad[0]], g[bad[0]], np.asarray(want).reshape(-1)[bad[0]], w[bad[0]])


def _refused(lib, rc, name, what):
    torch.cuda.synchronize()
    assert rc != 0, what
    msg = lib.rg_last_error()
    assert msg and name in msg, (what, msg)


def _hyper(step=7, wd=1e-2, ginv=0.125, skip=0):
    return adam_hyper_ref(step, wd=wd, ginv=ginv, skip=skip, **HYPER)


def _hyper_buf(h):
    return _f32buf(h, SENTINEL, after=64)


# ============================================================================================== (a) the hyper kernels
PARAMS = [(4e-4, 0.5, 0.999, 1e-8, 0.0), (1e-3, 0.9, 0.999, 1e-8, 1e-2)]
FLAG, LATCH, SLOTS = 8, 4, 4
DIFFER = {"n": 0, "of": 0}                           # hyper[5] / hyper[6] values that differ at all from the Python doubles'


class _HyperState:
    def __init__(self, t):
        self.step = torch.full((64,), SBITS, dtype=torch.int32, device=DEV)
        self.step[32] = t
        self.hyper = _f32buf(np.full(12, SENTINEL, np.float32), SENTINEL, after=64)

    def sp(self):
        return self.step.data_ptr() + 4 * 32

    def hp(self):
        return self.hyper.t.data_ptr()

    def read(self):
        torch.cuda.synchronize()
        s = self.step.cpu().numpy()
        assert (np.delete(s, 32) == SBITS).all(), "a hyper kernel wrote around the step counter"
        assert self.hyper.surroundings_keep(SBITS), "a hyper kernel wrote outside hyper[0..11]"
        return int(s[32]), _get(self.hyper)


def _amp_state(slot, latch, flag):
    """the words of the other slots (and the scaler's own) hold values that would show if they were read"""
    st = np.full(12, 99, dtype=np.int32)
    for s in range(SLOTS):
        st[LATCH + s] = latch if s == slot else 31 - s
        st[FLAG + s] = flag if s == slot else (0 if flag else 1)
    return torch.from_numpy(st).to(DEV)


def _check_hyper(h, want, what):
    for i in (0, 1, 2, 3, 4, 7, 8, 9):
        assert _u32(h[i:i + 1])[0] == _u32(want[i:i + 1])[0], "%s: hyper[%d] = %r, want %r" % (what, i, h[i], want[i])
    for i in (5, 6):
        d = abs(int(_u32(h[i:i + 1])[0]) - int(_u32(want[i:i + 1])[0]))
        DIFFER["of"] += 1
        DIFFER["n"] += d != 0
        assert d <= 1, "%s: hyper[%d] = %r is %d ulp from %r" % (what, i, h[i], d, want[i])
    assert (_u32(h[10:12]) == SBITS).all(), what + ": hyper[10..11] written"


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("t", [0, 1, 9, 999, 10 ** 5])
def test_hyper_kernels(half, t):
    lib = _abi.load(half)
    before = dict(DIFFER)
    for lr, b1, b2, eps, wd in PARAMS:
        s = _HyperState(t)
        assert lib.rg_adam_hyper_dev(s.sp(), lr, b1, b2, eps, wd, s.hp(), None) == 0, lib.rg_last_error()
        step, h = s.read()
        assert step == t + 1
        _check_hyper(h, adam_hyper_ref(t + 1, lr, b1, b2, eps, wd), "rg_adam_hyper_dev t=%d" % t)
        for ginv in (1.0, 2.0 ** -3, 2.0 ** -12):
            s = _HyperState(t)
            assert lib.rg_adam_hyper_dev2(s.sp(), lr, b1, b2, eps, wd, ginv, s.hp(), None) == 0, lib.rg_last_error()
            step, h = s.read()
            assert step == t + 1
            _check_hyper(h, adam_hyper_ref(t + 1, lr, b1, b2, eps, wd, ginv), "rg_adam_hyper_dev2 t=%d ginv=%g" % (t, ginv))
        for slot, latch in ((0, 0), (1, 12), (3, 24), (2, -3)):
            s = _HyperState(t)
            amp = _amp_state(slot, latch, 0)
            assert lib.rg_adam_hyper_dev3(s.sp(), lr, b1, b2, eps, wd, amp.data_ptr(), slot, s.hp(), None) == 0, lib.rg_last_error()
            step, h = s.read()
            assert step == t + 1                                   # flag clear: rg_adam_hyper_dev2 with ginv = 2^-latch
            _check_hyper(h, adam_hyper_ref(t + 1, lr, b1, b2, eps, wd, 2.0 ** -latch), "rg_adam_hyper_dev3 t=%d latch=%d" % (t, latch))
            assert h[8] == F32(2.0 ** -latch)
            # flag set, another latch and decay: [7], [8], [9] are this call's, the counter and [0..6] the previous call's
            amp2 = _amp_state(slot, latch + 1, 1)
            assert lib.rg_adam_hyper_dev3(s.sp(), lr * 3, 0.25, 0.75, eps * 2, 0.5, amp2.data_ptr(), slot, s.hp(), None) == 0
            step2, h2 = s.read()
            assert step2 == t + 1, "a skipped step advanced the counter"
            _same("hyper[0..6] after a skipped step", h2[:7], h[:7])
            assert h2[7] == F32(0.5) and h2[8] == F32(2.0 ** -(latch + 1)) and h2[9] == 1.0
            assert (_u32(h2[10:12]) == SBITS).all()
            assert np.array_equal(amp2.cpu().numpy(), _amp_state(slot, latch + 1, 1).cpu().numpy())      # the state is only read
    print("hyper[5] / hyper[6] read back (%s build, t = %d): %d of %d values differ from the Python doubles'" % (
        half, t, DIFFER["n"] - before["n"], DIFFER["of"] - before["of"]))


@pytest.mark.parametrize("half", HALVES)
def test_hyper_kernels_reject(half):
    lib = _abi.load(half)
    s = _HyperState(5)
    amp = _amp_state(0, 3, 0)
    a = (4e-4, 0.5, 0.999, 1e-8, 0.0)
    calls = {
        "dev: step NULL": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev(None, *a, s.hp(), None)),
        "dev: hyper NULL": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev(s.sp(), *a, None, None)),
        "dev2: step NULL": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev2(None, *a, 1.0, s.hp(), None)),
        "dev2: hyper NULL": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev2(s.sp(), *a, 1.0, None, None)),
        "dev2: ginv 0": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev2(s.sp(), *a, 0.0, s.hp(), None)),
        "dev2: ginv < 0": (b"adam_hyper_dev", lambda: lib.rg_adam_hyper_dev2(s.sp(), *a, -0.125, s.hp(), None)),
        "dev3: step NULL": (b"adam_hyper_dev3", lambda: lib.rg_adam_hyper_dev3(None, *a, amp.data_ptr(), 0, s.hp(), None)),
        "dev3: hyper NULL": (b"adam_hyper_dev3", lambda: lib.rg_adam_hyper_dev3(s.sp(), *a, amp.data_ptr(), 0, None, None)),
        "dev3: state NULL": (b"adam_hyper_dev3", lambda: lib.rg_adam_hyper_dev3(s.sp(), *a, None, 0, s.hp(), None)),
        "dev3: slot -1": (b"adam_hyper_dev3", lambda: lib.rg_adam_hyper_dev3(s.sp(), *a, amp.data_ptr(), -1, s.hp(), None)),
        "dev3: slot 4": (b"adam_hyper_dev3", lambda: lib.rg_adam_hyper_dev3(s.sp(), *a, amp.data_ptr(), SLOTS, s.hp(), None)),
    }
    for what, (name, fn) in calls.items():
        assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0      # (a good call in between: the message is this call's)
        _refused(lib, fn(), name, what)
        step, h = s.read()
        assert step == 5 and (_u32(h) == SBITS).all(), what


# ============================================================================================== (c) rg_adam_step_dev
_DATA = {}


def _data(n, kind, later, wd, ginv, clip=False):
    """(p, g, m, v), computed once and never modified; the gradient carries 1 / ginv (exact: a power of two)"""
    key = (n, kind, later, wd if kind == "special" else 0.0, ginv, clip and kind == "special")
    if key not in _DATA:
        p, g, m, v = special_inputs(n, wd) if kind == "special" else normal_inputs(n, later)
        if kind == "special" and not later:
            m, v = np.zeros_like(m), np.zeros_like(v)
        if kind == "special" and clip:
            g = np.clip(g, -4096.0, 4096.0).astype(np.float32)     # an fp16 wire: 8 x the large gradient must stay below 65504
        g = g * F32(1.0 / ginv)
        assert np.isfinite(g).all()
        for a in (p, g, m, v):
            a.setflags(write=False)
        _DATA[key] = (p, g, m, v)
    return _DATA[key]


class _Step:
    """the buffers of one rg_adam_step_dev call; `lead` elements (1..3) in front of the data move every fp32 pointer off the
    16-byte boundary (the scalar form), the rest of that 4-element frame belongs to the surroundings; a 4-tuple gives p, g, m and
    v a lead each"""

    def __init__(self, p, g, m, v, hyper, half, wire, shadow, lead=0):
        n = p.size
        self.n, self.half = n, half
        self.leads = lp, lg, lm, lv = (lead,) * 4 if isinstance(lead, int) else lead
        frame = lambda a, fill, ld: np.concatenate([np.full(ld, fill, np.float32), a, np.full((4 - ld) % 4, fill, np.float32)])
        self.p, self.m, self.v = (_f32buf(frame(a, SENTINEL, ld), SENTINEL) for a, ld in ((p, lp), (m, lm), (v, lv)))
        self.g_np = g
        self.wire_np = round_h16_ref(g, half) if wire else None
        # with a wire, g is never read: all NaN
        self.g = _f32buf(frame(np.full(n, NAN, np.float32) if wire else g, NAN, lg), NAN)
        self.wire = G16(self.wire_np, NAN16) if wire else None
        self.shadow = G16(np.full(n, S16, np.uint16), S16) if shadow else None
        self.hyper = _hyper_buf(hyper)
        self.hyper_np = np.array(hyper, np.float32)

    def ptrs(self):
        lp, lg, lm, lv = self.leads
        return (self.p.t.data_ptr() + 4 * lp, self.g.t.data_ptr() + 4 * lg, self.m.t.data_ptr() + 4 * lm, self.v.t.data_ptr() + 4 * lv)

    def call(self, lib, n=None):
        p, g, m, v = self.ptrs()
        return lib.rg_adam_step_dev(p, g, m, v, self.n if n is None else n, self.hyper.t.data_ptr(),
                                    None if self.shadow is None else self.shadow.ptr(),
                                    None if self.wire is None else self.wire.ptr(), None)

    def gradient(self):
        return self.g_np if self.wire_np is None else widen_h16_ref(self.wire_np, self.half)

    def results(self, what):
        """(p, m, v, shadow bits) after checking that nothing around them, and nothing that is only read, has changed"""
        torch.cuda.synchronize()
        out = []
        lp, lg, lm, lv = self.leads
        for name, b, ld in (("p", self.p, lp), ("m", self.m, lm), ("v", self.v, lv)):
            assert b.surroundings_keep(SBITS), "%s: wrote outside %s" % (what, name)
            a = _get(b)
            fr = np.concatenate([a[:ld], a[ld + self.n:]])
            assert (_u32(fr) == SBITS).all(), "%s: wrote next to %s" % (what, name)
            out.append(a[ld:ld + self.n])
        assert _nan_around(self.g), what
        ga = _get(self.g)
        if self.wire is None:
            _same(what + ": g changed", ga[lg:lg + self.n], self.g_np)
        else:
            assert np.isnan(ga).all(), what + ": g written"
            _same(what + ": the wire changed", self.wire.get(), self.wire_np, as16=True)
            assert self.wire.surroundings_keep(), what
        _same(what + ": hyper changed", _get(self.hyper), self.hyper_np)
        assert self.hyper.surroundings_keep(SBITS)
        sh = None
        if self.shadow is not None:
            assert self.shadow.surroundings_keep(), what + ": wrote outside the shadow"
            sh = self.shadow.get()
        return out[0], out[1], out[2], sh


def _check_step(st, got, what, p, m, v):
    want = adam_upd_ref(p, st.gradient(), m, v, st.hyper_np)
    for a in want:
        assert np.isfinite(a).all(), what
    for name, g_, w_ in zip("pmv", got[:3], want):
        _same("%s: %s" % (what, name), g_, w_)
    if got[3] is not None:
        _same(what + ": shadow", got[3], round_h16_ref(want[0], st.half), as16=True)
    return want


VARIANTS = [(False, False), (False, True), (True, False), (True, True)]          # (wire, shadow)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("wire,shadow", VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_step_dev_bit_exact(half, wire, shadow, n):
    lib = _abi.load(half)
    for kind in ("normal", "special"):
        for later in (False, True):
            for wd in (0.0, 1e-2):
                for ginv in (1.0, 0.125):
                    p, g, m, v = _data(n, kind, later, wd, ginv, clip=wire and half == "f16")
                    st = _Step(p, g, m, v, _hyper(7 if later else 1, wd, ginv), half, wire, shadow)
                    what = "n %d %s %s wd %g ginv %g wire %d shadow %d" % (n, kind, "later" if later else "first", wd, ginv, wire, shadow)
                    assert st.call(lib) == 0, lib.rg_last_error()
                    want = _check_step(st, st.results(what), what, p, m, v)
                    if kind == "normal" and n >= 4:
                        assert not np.array_equal(_u32(want[0]), _u32(p))      # the update happened


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("wire,shadow", [(False, False), (True, True)])
def test_step_dev_two_passes_of_the_capped_grid(half, wire, shadow):
    """2 x 8192 workgroups x 256 threads x 4 elements + 3: the grid-stride loop runs twice for every thread, then the tail"""
    lib = _abi.load(half)
    p, g, m, v = _data(BIG, "normal", True, 1e-2, 0.125)
    st = _Step(p, g, m, v, _hyper(7, 1e-2, 0.125), half, wire, shadow)
    assert st.call(lib) == 0, lib.rg_last_error()
    _check_step(st, st.results("two passes"), "two passes", p, m, v)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("wire,shadow", VARIANTS)
def test_step_dev_skip_word(half, wire, shadow):
    lib = _abi.load(half)
    for n in (5, 1027):
        p, g, m, v = _data(n, "normal", True, 1e-2, 0.125)
        st = _Step(p, g, m, v, _hyper(7, skip=1), half, wire, shadow)
        assert st.call(lib) == 0, lib.rg_last_error()
        got = st.results("skipped")
        for name, a, b in zip("pmv", got[:3], (p, m, v)):
            _same("a skipped step moved " + name, a, b)
        if shadow:
            assert (got[3] == S16).all(), "a skipped step wrote the shadow"
        st = _Step(p, g, m, v, _hyper(7, skip=0), half, wire, shadow)
        assert st.call(lib) == 0
        _check_step(st, st.results("not skipped"), "not skipped", p, m, v)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_step_dev_scalar_form(half, n):
    """all four pointers 4, 8 and 12 bytes off the 16-byte boundary: the element-per-thread kernel, bit-equal to the aligned one"""
    lib = _abi.load(half)
    for kind in ("normal", "special"):
        p, g, m, v = _data(n, kind, True, 1e-2, 0.125)
        hy = _hyper(7, 1e-2, 0.125)
        al = _Step(p, g, m, v, hy, half, False, False)
        assert al.call(lib) == 0
        aligned = _check_step(al, al.results("aligned"), "aligned", p, m, v)
        # ... and p, g, m, v off by different amounts (one of them aligned): the same kernel takes any 4-byte aligned pointers
        for lead in (1, 2, 3, (1, 2, 3, 0), (0, 0, 0, 2), (0, 3, 0, 0)):
            st = _Step(p, g, m, v, hy, half, False, False, lead=lead)
            assert st.call(lib) == 0, lib.rg_last_error()
            got = st.results("lead %r" % (lead,))
            for name, a, b in zip("pmv", got[:3], aligned):
                _same("scalar form, lead %r, %s: %s" % (lead, kind, name), a, b)
        # the skip word holds for the scalar kernel too
        st = _Step(p, g, m, v, _hyper(7, skip=1), half, False, False, lead=1)
        assert st.call(lib) == 0
        got = st.results("scalar skipped")
        for a, b in zip(got[:3], (p, m, v)):
            _same("a skipped scalar step", a, b)


@pytest.mark.parametrize("half", HALVES)
def test_step_dev_refusals_and_n_zero(half):
    lib = _abi.load(half)
    n = 1027
    p, g, m, v = _data(n, "normal", True, 1e-2, 0.125)
    hy = _hyper(7)

    def untouched(st, what):
        got = st.results(what)
        for a, b in zip(got[:3], (p, m, v)):
            _same(what, a, b)
        if got[3] is not None:
            assert (got[3] == S16).all(), what

    # misaligned with a shadow or a wire: refused
    for lead in (1, 2, 3):
        for wire, shadow in ((True, False), (False, True), (True, True)):
            st = _Step(p, g, m, v, hy, half, wire, shadow, lead=lead)
            what = "lead %d wire %d shadow %d" % (lead, wire, shadow)
            _refused(lib, st.call(lib), b"adam_step_dev", what)
            untouched(st, what)
    st = _Step(p, g, m, v, hy, half, False, False)
    pp, gp, mp, vp = st.ptrs()
    # NULL arguments
    st2 = _Step(p, g, m, v, hy, half, True, True)
    hp, sp, wp = st2.hyper.t.data_ptr(), st2.shadow.ptr(), st2.wire.ptr()
    pp2, gp2, mp2, vp2 = st2.ptrs()
    for what, args in {"p NULL": (None, gp2, mp2, vp2, n, hp, sp, wp), "m NULL": (pp2, gp2, None, vp2, n, hp, sp, wp),
                       "v NULL": (pp2, gp2, mp2, None, n, hp, sp, wp), "hyper NULL": (pp2, gp2, mp2, vp2, n, None, sp, wp),
                       "both gradients NULL": (pp2, None, mp2, vp2, n, hp, sp, None)}.items():
        assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0
        _refused(lib, lib.rg_adam_step_dev(*args, None), b"adam_step_dev", what)
    # n = 0: nothing is launched, aligned or not
    assert st.call(lib, n=0) == 0 and st2.call(lib, n=0) == 0
    assert lib.rg_adam_step_dev(pp + 4, gp + 4, mp + 4, vp + 4, 0, st.hyper.t.data_ptr(), None, None, None) == 0
    untouched(st, "refused / n = 0 calls")
    untouched(st2, "refused / n = 0 calls (wire, shadow)")


# ============================================================================================== (b) the product's pairing
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("dev3", [False, True])
def test_hyper_launch_then_step_launch(half, dev3):
    """three steps of rg_adam_hyper_dev2 (or _dev3 with the middle step skipped) -> rg_adam_step_dev on the same buffers, against
    the reference chain fed the hyper values READ BACK after each hyper launch."""
    lib = _abi.load(half)
    n = 1027
    lr, b1, b2, eps, wd = 4e-4, 0.5, 0.999, 1e-8, 1e-2
    p, _, m, v = normal_inputs(n, later=False)
    s = _HyperState(0)
    P, M, V = (_f32buf(a, SENTINEL) for a in (p, m, v))
    sh = G16(np.full(n, S16, np.uint16), S16)
    shadow_want = np.full(n, S16, np.uint16)
    counter = 0
    for k in range(3):
        g = normal_inputs(n, later=False, seed=k + 1)[1] * F32(8.0)
        G = _f32buf(g, NAN)
        skip = dev3 and k == 1
        if dev3:
            amp = _amp_state(2, 3, int(skip))
            assert lib.rg_adam_hyper_dev3(s.sp(), lr, b1, b2, eps, wd, amp.data_ptr(), 2, s.hp(), None) == 0
        else:
            assert lib.rg_adam_hyper_dev2(s.sp(), lr, b1, b2, eps, wd, 0.125, s.hp(), None) == 0
        assert lib.rg_adam_step_dev(P.t.data_ptr(), G.t.data_ptr(), M.t.data_ptr(), V.t.data_ptr(), n, s.hp(), sh.ptr(), None, None) == 0
        step, h = s.read()
        counter += 0 if skip else 1
        assert step == counter
        _check_hyper(h, adam_hyper_ref(counter, lr, b1, b2, eps, wd, 0.125, skip=int(skip)), "step %d" % k)
        if not skip:
            p, m, v = adam_upd_ref(p, g, m, v, h)
            shadow_want = round_h16_ref(p, half)
        for name, buf, want in (("p", P, p), ("m", M, m), ("v", V, v)):
            _same("step %d: %s" % (k, name), _get(buf), want)
            assert buf.surroundings_keep(SBITS)
        _same("step %d: shadow" % k, sh.get(), shadow_want, as16=True)
    assert counter == (2 if dev3 else 3) and sh.surroundings_keep()


# ============================================================================================== (d) rg_adam_step (host hyper)
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n", SIZES)
def test_step_host_hyper(half, n):
    lib = _abi.load(half)
    for kind in ("normal", "special"):
        for step in (1, 7):
            p, g, m, v = _data(n, kind, step == 7, 0.0, 1.0)
            hy = adam_hyper_ref(step, **HYPER)                     # wd = 0, ginv = 1
            st = _Step(p, g, m, v, hy, half, False, False)
            pp, gp, mp, vp = st.ptrs()
            assert lib.rg_adam_step(pp, gp, mp, vp, n, step, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], None) == 0, lib.rg_last_error()
            what = "rg_adam_step n %d %s step %d" % (n, kind, step)
            _check_step(st, st.results(what), what, p, m, v)


@pytest.mark.parametrize("half", HALVES)
def test_step_host_hyper_refusals(half):
    lib = _abi.load(half)
    n = 1027
    p, g, m, v = _data(n, "normal", True, 0.0, 1.0)
    st = _Step(p, g, m, v, _hyper(7), half, False, False)
    pp, gp, mp, vp = st.ptrs()
    a = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], None)
    calls = {"step 0": (pp, gp, mp, vp, n, 0), "step -1": (pp, gp, mp, vp, n, -1), "p NULL": (None, gp, mp, vp, n, 1),
             "g NULL": (pp, None, mp, vp, n, 1), "p misaligned": (pp + 4, gp, mp, vp, n - 1, 1), "g misaligned": (pp, gp + 8, mp, vp, n - 2, 1),
             "all misaligned": (pp + 4, gp + 4, mp + 4, vp + 4, n - 1, 1)}
    for what, args in calls.items():
        assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0
        _refused(lib, lib.rg_adam_step(*args, *a), b"adam_step", what)
    assert lib.rg_adam_step(pp, gp, mp, vp, 0, 1, *a) == 0
    got = st.results("refused rg_adam_step calls")
    for x, y in zip(got[:3], (p, m, v)):
        _same("refused rg_adam_step calls", x, y)


# ============================================================================================== (e), (f) segment tables
_SLABS = {}


def _slab(nsplit, n, kind, half):
    """fp32 slabs, or the bits of the same values in the build's 16-bit type; computed once, read-only"""
    key = (nsplit, n, kind, half if kind == "h16" else None)
    if key not in _SLABS:
        s = slab_inputs(nsplit, n) if kind == "f32" else slab_inputs_h16(nsplit, n, half)
        s.setflags(write=False)
        _SLABS[key] = s
    return _SLABS[key]


class _Table:
    """spec: a list of (n, kind, nsplit) with kind in plain | f32 | h16 | skip.  Builds the reference's table and the device
    buffers: every slab tensor in a NaN-filled allocation of its own, g NaN under slab and skipped segments."""

    def __init__(self, spec, half, shadow=True, hyper=None):
        self.half, self.spec = half, spec
        offs = np.concatenate([[0], np.cumsum([s[0] for s in spec])]).astype(np.int64)
        self.total = total = int(offs[-1])
        p, g, m, v = normal_inputs(total, later=True, seed=len(spec))
        g = g * F32(8.0)
        self.table, self.slab_bufs = [], []
        for (n, kind, nsplit), off in zip(spec, offs[:-1].tolist()):
            if kind == "plain":
                self.table.append((off, n, None, 0)); self.slab_bufs.append(None)
            elif kind == "skip":
                g[off:off + n] = NAN
                self.table.append((off, n, None, -1)); self.slab_bufs.append(None)
            else:
                g[off:off + n] = NAN
                s = _slab(nsplit, n, kind, half)
                self.table.append((off, n, s, nsplit))
                self.slab_bufs.append(_f32buf(s.reshape(-1), NAN) if kind == "f32" else G16(s, NAN16))
        self.np = (p, g, m, v)
        self.hyper_np = _hyper(7, 1e-2, 0.125) if hyper is None else hyper
        self.P, self.M, self.V = (_f32buf(a, SENTINEL) for a in (p, m, v))
        self.G = _f32buf(g, NAN)
        self.S = G16(np.full(total, S16, np.uint16), S16) if shadow else None
        self.W = G16(np.full(total, S16, np.uint16), S16)
        self.H = _hyper_buf(self.hyper_np)
        k = len(spec)
        self.k = k
        self.c_off = (C.c_ulonglong * k)(*[t[0] for t in self.table])
        self.c_n = (C.c_ulonglong * k)(*[t[1] for t in self.table])
        self.c_slab = (C.c_void_p * k)(*[None if b is None else (b.t.data_ptr() if isinstance(b, Guarded) else b.ptr()) for b in self.slab_bufs])
        self.c_ns = (C.c_int * k)(*[t[3] for t in self.table])
        code = {"f32": _abi.RG_F32, "h16": _h16code(half)}
        self.c_dt = (C.c_int * k)(*[code.get(s[1], 0) for s in spec])

    def tabs(self):
        return (C.addressof(self.c_off), C.addressof(self.c_n), C.addressof(self.c_slab), C.addressof(self.c_ns), C.addressof(self.c_dt))

    def adam(self, lib, n=None, k=None, tabs=None, p_off=0):
        return lib.rg_adam_step_slabs(self.P.t.data_ptr() + p_off, self.G.t.data_ptr(), self.M.t.data_ptr(), self.V.t.data_ptr(),
                                      self.total if n is None else n, self.H.t.data_ptr(), None if self.S is None else self.S.ptr(),
                                      self.k if k is None else k, *(tabs or self.tabs()), None)

    def wire(self, lib, n=None, k=None, tabs=None):
        return lib.rg_grad_to_wire(self.G.t.data_ptr(), self.W.ptr(), self.total if n is None else n, self.k if k is None else k,
                                   *(tabs or self.tabs()), None)

    def inputs_unchanged(self, what):
        assert _nan_around(self.G), what
        _same(what + ": g changed", _get(self.G), self.np[1])
        for b, (_, _, s, _) in zip(self.slab_bufs, self.table):
            if b is None:
                continue
            if isinstance(b, Guarded):
                _same(what + ": a slab changed", _get(b), s.reshape(-1))
                assert _nan_around(b)
            else:
                _same(what + ": a slab changed", b.get(), s.reshape(-1), as16=True)
                assert b.surroundings_keep()

    def adam_results(self, what):
        torch.cuda.synchronize()
        for name, b in (("p", self.P), ("m", self.M), ("v", self.V)):
            assert b.surroundings_keep(SBITS), "%s: wrote outside %s" % (what, name)
        if self.S is not None:
            assert self.S.surroundings_keep(), what + ": wrote outside the shadow"
        self.inputs_unchanged(what)
        _same(what + ": hyper changed", _get(self.H), self.hyper_np)
        assert (self.W.get() == S16).all()
        return _get(self.P), _get(self.M), _get(self.V), None if self.S is None else self.S.get()

    def check_adam(self, what):
        got = self.adam_results(what)
        p, g, m, v = self.np
        want = adam_table_ref(p, g, m, v, self.hyper_np, self.table, self.half, shadow=np.full(self.total, S16, np.uint16))
        for a in want[:3]:
            assert np.isfinite(a).all(), what
        for name, g_, w_ in zip("pmv", got[:3], want[:3]):
            _same("%s: %s" % (what, name), g_, w_)
        if got[3] is not None:
            _same(what + ": shadow", got[3], want[3], as16=True)
        return got

    def check_untouched(self, what):
        got = self.adam_results(what)
        for name, a, b in zip("pmv", got[:3], (self.np[0], self.np[2], self.np[3])):
            _same("%s: %s written" % (what, name), a, b)
        if got[3] is not None:
            assert (got[3] == S16).all(), what + ": shadow written"

    def check_wire(self, what):
        torch.cuda.synchronize()
        assert self.W.surroundings_keep(), what + ": wrote outside the wire"
        self.inputs_unchanged(what)
        want = wire_table_ref(self.np[1], self.table, self.half, wire=np.full(self.total, S16, np.uint16))
        got = self.W.get()
        _same(what + ": wire", got, want, as16=True)
        return got


SEG_SIZES = [4, 60, 64, 1024, 1028]
LONG_NSPLITS = [4, 32, 33, 129]                    # n = 65536: about 16 trips per workgroup at 16 lanes


def _one_slab_specs(n):
    return [[(8, "plain", 0), (n, None, ns), (7, "plain", 0)] for ns in (SLAB_NSPLITS if n < 65536 else LONG_NSPLITS)]


def _with_kind(spec, kind):
    return [(n, kind if k is None else k, ns) for n, k, ns in spec]


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("kind", ["f32", "h16"])
@pytest.mark.parametrize("n", SEG_SIZES + [65536])
def test_slab_segment_adam(half, kind, n):
    """plain | slab | plain (7 elements: not a multiple of 4) for every nsplit: both lane-count boundaries, the unrolled loop's
    entry on either side of z + 7 SL < nsplit for lane 0 and for the last lane, one column, partial and whole trips"""
    lib = _abi.load(half)
    for spec in _one_slab_specs(n):
        for shadow in ((True, False) if n < 65536 else (True,)):
            t = _Table(_with_kind(spec, kind), half, shadow=shadow)
            assert t.adam(lib) == 0, lib.rg_last_error()
            t.check_adam("nsplit %d n %d %s shadow %d" % (spec[1][2], n, kind, shadow))


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("kind", ["f32", "h16"])
@pytest.mark.parametrize("n", SEG_SIZES + [65536])
def test_slab_segment_wire(half, kind, n):
    lib = _abi.load(half)
    for spec in _one_slab_specs(n):
        t = _Table(_with_kind(spec, kind), half, shadow=False)
        assert t.wire(lib) == 0, lib.rg_last_error()
        t.check_wire("nsplit %d n %d %s" % (spec[1][2], n, kind))


def _tables():
    mixed = []
    kinds = ["plain", "f32", "h16", "skip"]
    nsp = [0, 5, 40, -1, 0, 3, 33, -1, 0, 29, 64, -1, 0, 8, 129, -1, 0, 4, 32, -1, 0, 200, 1, 0]
    for i in range(24):
        k = kinds[i % 4]
        n = (4 * (i + 1)) if k in ("plain", "skip") else (60 if i % 8 < 4 else 64)
        mixed.append((n, k, nsp[i]))
    mixed[-1] = (5, "plain", 0)                                    # the last plain segment is not a multiple of 4
    return {
        "16, 1 and 4 lanes in a row": [(1028, "f32", 40), (60, "h16", 3), (1024, "f32", 9)],
        "16, 1 and 4 lanes in a row (other types)": [(1028, "h16", 40), (60, "f32", 3), (1024, "h16", 9)],
        "4, 16, 4 lanes, one column each": [(4, "f32", 5), (4, "f32", 33), (4, "h16", 32)],
        "a skipped segment in the middle": [(64, "plain", 0), (1028, "skip", -1), (64, "f32", 5), (5, "plain", 0)],
        "24 segments": mixed,
        "one plain segment": [(1027, "plain", 0)],
    }


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("name", list(_tables()))
def test_tables_adam(half, name):
    lib = _abi.load(half)
    spec = _tables()[name]
    for shadow in (True, False):
        t = _Table(spec, half, shadow=shadow)
        assert t.adam(lib) == 0, lib.rg_last_error()
        got = t.check_adam("%s, shadow %d" % (name, shadow))
        if name == "one plain segment":                             # ... equals rg_adam_step_dev bit for bit
            p, g, m, v = t.np
            st = _Step(p, g, m, v, t.hyper_np, half, False, shadow)
            assert st.call(lib) == 0
            for nm, a, b in zip(("p", "m", "v", "shadow"), got, st.results("rg_adam_step_dev")):
                if a is not None:
                    _same("rg_adam_step_slabs against rg_adam_step_dev: " + nm, a, b, as16=nm == "shadow")
    # the skip word
    t = _Table(spec, half, shadow=True, hyper=_hyper(7, 1e-2, 0.125, skip=1))
    assert t.adam(lib) == 0
    t.check_untouched(name + ", skipped step")


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("name", list(_tables()))
def test_tables_wire(half, name):
    lib = _abi.load(half)
    t = _Table(_tables()[name], half, shadow=False)
    assert t.wire(lib) == 0, lib.rg_last_error()
    got = t.check_wire(name)
    for (off, n, slabs, nsplit) in t.table:
        if slabs is None and nsplit < 0:
            assert (got[off:off + n] == S16).all()                 # a skipped segment's slice of the wire is left alone


@pytest.mark.parametrize("half", HALVES)
def test_wire_overflow_in_fp16(half):
    """a column whose fp32 sum exceeds 65504 goes onto an fp16 wire as infinity; its neighbours are unaffected"""
    lib = _abi.load(half)
    t = _Table([(8, "plain", 0), (64, "f32", 5), (4, "plain", 0)], half, shadow=False)
    s = np.array(t.table[1][2])
    s[:, 9] = 30000.0; s[:, 33] = -30000.0
    t.table[1] = (8, 64, s, 5)
    t.slab_bufs[1] = _f32buf(s.reshape(-1), NAN)
    t.c_slab[1] = t.slab_bufs[1].t.data_ptr()
    g = np.array(t.np[1]); g[3] = 1e6
    t.np = (t.np[0], g, t.np[2], t.np[3])
    t.G = _f32buf(g, NAN)
    assert t.wire(lib) == 0, lib.rg_last_error()
    got = widen_h16_ref(t.check_wire("overflow"), half)
    if half == "f16":
        assert got[8 + 9] == np.inf and got[8 + 33] == -np.inf and got[3] == np.inf
        assert np.isfinite(np.delete(got, [3, 8 + 9, 8 + 33])).all()
    else:
        assert np.isfinite(got).all()


@pytest.mark.parametrize("half", HALVES)
def test_refused_tables(half):
    lib = _abi.load(half)
    spec = [(8, "plain", 0), (64, "f32", 5), (64, "h16", 3), (12, "skip", -1), (7, "plain", 0)]
    t = _Table(spec, half, shadow=True)
    other16 = _abi.RG_BF16 if half == "f16" else _abi.RG_F16

    def edited(**kw):
        """the table with some entries replaced: name -> (index, value); returns (tabs, keep-alive)"""
        arrs = {"off": (C.c_ulonglong * t.k)(*t.c_off), "n": (C.c_ulonglong * t.k)(*t.c_n), "slab": (C.c_void_p * t.k)(*t.c_slab),
                "ns": (C.c_int * t.k)(*t.c_ns), "dt": (C.c_int * t.k)(*t.c_dt)}
        for name, (i, val) in kw.items():
            arrs[name][i] = val
        return tuple(C.addressof(arrs[k]) for k in ("off", "n", "slab", "ns", "dt")), arrs

    slab1 = t.c_slab[1]
    cases = {
        "a gap": dict(off=(2, 76)),
        "an overlap": dict(off=(2, 68)),
        "an offset that is not a multiple of 4": dict(n=(0, 6), off=(1, 6)),
        "a slab segment whose n is not a multiple of 4": dict(n=(2, 62)),
        "a slab segment with nsplit 0": dict(ns=(1, 0)),
        "a misaligned slab": dict(slab=(1, slab1 + 4)),
        "fp16 slabs in the bf16 build (or the reverse)": dict(dt=(2, other16)),
        "an unknown slab dtype": dict(dt=(1, 7)),
    }
    good = t.tabs()
    for entry, name in ((t.adam, b"adam_step_slabs"), (t.wire, b"grad_to_wire")):
        for what, kw in cases.items():
            tabs, keep = edited(**kw)
            assert lib.rg_ema_update(None, None, 0, 0.5, None, None, None) == 0
            _refused(lib, entry(lib, tabs=tabs), name, what)
        _refused(lib, entry(lib, k=0), name, "nseg 0")
        _refused(lib, entry(lib, k=25), name, "nseg 25")
        _refused(lib, entry(lib, n=t.total + 4), name, "coverage below n")
        _refused(lib, entry(lib, n=t.total - 4), name, "coverage above n")
        _refused(lib, entry(lib, k=t.k - 1), name, "a segment short")
        for i in range(5):
            tabs = list(good); tabs[i] = None
            _refused(lib, entry(lib, tabs=tuple(tabs)), name, "table %d NULL" % i)
    _refused(lib, t.adam(lib, p_off=4), b"adam_step_slabs", "p misaligned")
    t.check_untouched("refused tables")


# ============================================================================================== (g) the fused epilogues
def _ints(shape, seed, lo=-2, hi=2):
    """small integers without zero, as fp64"""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi, size=shape)                           # lo .. hi - 1
    return np.where(a >= 0, a + 1, a).astype(np.float64)


def _h16_tensor(a, half):
    t = torch.from_numpy(np.asarray(a, dtype=np.float32)).to(TORCH16[half])
    assert torch.equal(t.float(), torch.from_numpy(np.asarray(a, dtype=np.float32)))     # exact in the type
    return t


def _exact_f32(dw):
    g = dw.astype(np.float32)
    assert np.array_equal(g.astype(np.float64), dw) and float(np.abs(dw).max()) < 2 ** 24
    assert len(np.unique(dw)) >= 20 and float(np.mean(dw == 0)) <= 0.2        # not a trivial gradient
    return g * F32(8.0)                                            # carries 1 / ginv


def _epilogue_state(n, seed):
    p, _, m, v = normal_inputs(n, later=True, seed=seed)
    assert np.all(m != 0) and np.all(v != 0)
    return p, m, v


EPI_HYPER = dict(step=5, wd=1e-2, ginv=0.125)


def _check_epilogue(what, half, bufs, shadow, p, g, m, v, hy):
    torch.cuda.synchronize()
    want = adam_upd_ref(p, g, m, v, hy)
    for name, b, w in zip("pmv", bufs, want):
        assert b.surroundings_keep(SBITS), "%s: wrote outside %s" % (what, name)
        _same("%s: %s" % (what, name), _get(b), w)
    if shadow is not None:
        assert shadow.surroundings_keep()
        _same(what + ": shadow", shadow.get(), round_h16_ref(want[0], half), as16=True)
    return want


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("N,E,Cc", [(5, 64, 16), (200, 64, 32)])
def test_g0_epilogue_on_an_exact_gradient(half, N, E, Cc):
    lib = _abi.load(half)
    H = _h16code(half)
    assert lib.rg_g0_wgrad_adam_supported(N, E, Cc, H) == 1
    z, gz = _ints((N, E), 1), _ints((N, 4, 4, Cc), 2)
    dw = np.einsum("ne,nhwc->echw", z, gz)                          # fp64 on integers: exact
    g = _exact_f32(dw).reshape(-1)
    # the operands carry the factor 8 (z is fp32; 8 x small integers stay exact in both 16-bit types)
    zt = torch.from_numpy((z * 8.0).astype(np.float32)).to(DEV)
    gzt = _h16_tensor(gz, half).to(DEV)
    p, m, v = _epilogue_state(g.size, 3)
    hy = _hyper(**EPI_HYPER)
    for with_shadow in (True, False):
        P, M, V = (_f32buf(a, SENTINEL) for a in (p, m, v))
        S = G16(np.full(g.size, S16, np.uint16), S16) if with_shadow else None
        Hb = _hyper_buf(hy)
        rc = lib.rg_g0_wgrad_adam(zt.data_ptr(), gzt.data_ptr(), P.t.data_ptr(), M.t.data_ptr(), V.t.data_ptr(), Hb.t.data_ptr(),
                                  None if S is None else S.ptr(), N, E, Cc, H, None)
        assert rc == 0, lib.rg_last_error()
        _check_epilogue("rg_g0_wgrad_adam (%d, %d, %d)" % (N, E, Cc), half, (P, M, V), S, p, g, m, v, hy)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("N,O,I", [(40, 130, 1024), (100, 64, 515)])
def test_linear_epilogue_on_an_exact_gradient(half, pack, N, O, I):
    lib = _abi.load(half)
    gy, x = _ints((N, O), 4), _ints((N, I), 5)
    g = _exact_f32(gy.T @ x).reshape(-1)
    ldn = (N + 63) // 64 * 64
    gT = torch.zeros(O + 3, ldn, dtype=TORCH16[half]); gT[:O, :N] = _h16_tensor(gy.T * 8.0, half)
    xT = torch.zeros(I + 5, ldn, dtype=TORCH16[half]); xT[:I, :N] = _h16_tensor(x.T, half)
    gT, xT = gT.to(DEV), xT.to(DEV)
    p, m, v = _epilogue_state(g.size, 6)
    hy = _hyper(**EPI_HYPER)
    lead = 1 if I % 2 else 0                                        # the odd row pitch starts 4 bytes off the 16-byte boundary
    frame = lambda a: np.concatenate([np.full(lead, SENTINEL, np.float32), a, np.full((4 - lead) % 4, SENTINEL, np.float32)])
    P, M, V = (_f32buf(frame(a), SENTINEL) for a in (p, m, v))
    Kp = (I + 63) // 64 * 64
    W = G16(np.full((O + 2) * Kp, S16, np.uint16), S16) if pack else None
    Hb = _hyper_buf(hy)
    o = 4 * lead
    rc = lib.rg_linear_wgrad_adam(gT.data_ptr(), xT.data_ptr(), ldn, N, P.t.data_ptr() + o, M.t.data_ptr() + o, V.t.data_ptr() + o,
                                  Hb.t.data_ptr(), O, I, None if W is None else W.ptr(), Kp if pack else 0, None)
    assert rc == 0, lib.rg_last_error()
    torch.cuda.synchronize()
    want = adam_upd_ref(p, g, m, v, hy)
    what = "rg_linear_wgrad_adam (%d, %d, %d)" % (N, O, I)
    for name, b, w in zip("pmv", (P, M, V), want):
        assert b.surroundings_keep(SBITS), "%s: wrote outside %s" % (what, name)
        a = _get(b)
        assert (_u32(np.concatenate([a[:lead], a[lead + g.size:]])) == SBITS).all(), "%s: wrote next to %s" % (what, name)
        _same("%s: %s" % (what, name), a[lead:lead + g.size], w)
    if pack:
        assert W.surroundings_keep()
        img = W.get().reshape(O + 2, Kp)
        _same(what + ": packed image", img[:O, :I], round_h16_ref(want[0], half).reshape(O, I), as16=True)
        assert (img[:O, I:] == S16).all() and (img[O:] == S16).all(), what + ": the image's padding was written"


def _conv_shape(lib, H):
    # the smallest of these layer shapes whose weight gradient has a plan without split-K, as tests/test_loss_scaler_gpu.py
    for shape in ((64, 4, 256, 256), (64, 4, 512, 512), (64, 4, 2048, 1024)):
        if lib.rg_conv_wgrad_adam_supported(shape[0], shape[1], shape[1], shape[2], shape[3], 0, H, _abi.ALGO_AUTO) == 1:
            return shape
    return None


def _conv_wgrad_ref(low, high):
    """dw[o, kh, kw, i] = sum over (n, ho, wo) of low[n, ho, wo, o] high_pad[n, 2 ho + kh, 2 wo + kw, i] (4 x 4, stride 2, pad 1),
    fp64 on integers"""
    N, Ho, Wo, O = low.shape
    I = high.shape[-1]
    hp = np.pad(high, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dw = np.zeros((O, 4, 4, I))
    lo = low.reshape(-1, O)
    for kh in range(4):
        for kw in range(4):
            patch = hp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, I)
            dw[:, kh, kw, :] = lo.T @ patch
    return dw


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("two", [False, True])
def test_conv_epilogue_on_an_exact_gradient(half, two):
    lib = _abi.load(half)
    H = _h16code(half)
    shape = _conv_shape(lib, H)
    if shape is None:
        pytest.skip("this build has no single-launch weight-gradient plan")
    N, hs, O, I = shape
    if lib.rg_conv_wgrad_adam_supported(N, hs, hs, O, I, int(two), H, _abi.ALGO_AUTO) != 1:
        pytest.skip("no single-launch plan for %s operand pairs at this shape" % ("two" if two else "one"))
    pairs = [(_ints((N, hs, hs, O), 10 + 2 * k), _ints((N, 2 * hs, 2 * hs, I), 11 + 2 * k)) for k in range(2 if two else 1)]
    dw = sum(_conv_wgrad_ref(lo, hi) for lo, hi in pairs)
    g = _exact_f32(dw).reshape(-1)
    dev = [(_h16_tensor(lo * 8.0, half).to(DEV), _h16_tensor(hi, half).to(DEV)) for lo, hi in pairs]
    ptrs = [t.data_ptr() for pair in dev for t in pair] + [None, None] * (2 - len(dev))
    p, m, v = _epilogue_state(g.size, 7)
    hy = _hyper(**EPI_HYPER)
    P, M, V = (_f32buf(a, SENTINEL) for a in (p, m, v))
    S = G16(np.full(g.size, S16, np.uint16), S16)
    Hb = _hyper_buf(hy)
    rc = lib.rg_conv_wgrad_adam(*ptrs[:4], P.t.data_ptr(), M.t.data_ptr(), V.t.data_ptr(), Hb.t.data_ptr(), S.ptr(), N, hs, hs, O, I, H,
                                _abi.ALGO_AUTO, None)
    assert rc == 0, lib.rg_last_error()
    _check_epilogue("rg_conv_wgrad_adam %r, %d operand pair(s)" % (shape, len(pairs)), half, (P, M, V), S, p, g, m, v, hy)
