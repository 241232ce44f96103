"""Dynamic loss scaling (rna_gan_amd.amp) on the device:

  * exactness: with power-of-two scaling exact (bf16 / fp32 paths), a scale that doubles after EVERY train_op gives losses,
    parameters, BatchNorm buffers and Adam moments bit-identical to the unscaled run, through captured step graphs, without
    new graphs as the scale changes;
  * overflow recovery (fp16): a start at 2^40 overflows; every such train_op is a bit-exact no-op (parameters, moments,
    shadows, the device step counter), the scale backs off, training resumes; the same start as a static scale ends non-finite;
  * kernel level: one inf in a plain gradient range, a split-K slab, the 16-bit wire, the G.0 factors or a fused
    weight-gradient operand skips the whole step; without it the guarded entry points equal the unguarded ones bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R
import rna_gan_amd as P
from rna_gan_amd import _abi
from rna_gan_amd.amp import DynamicLossScaler, FLAG
from test_train_gpu import product_pair


def _models(in_size, step, enc):
    G0 = R.seeded_fill_(R.OracleDCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2),
                                               last_nonlinearity=nn.Tanh()), 7)
    D0 = R.seeded_fill_(R.OracleDCGANDiscriminator(in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2),
                                                   last_nonlinearity=nn.LeakyReLU(0.2)), 8)
    return G0, D0


def _plugins():
    return P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()


def _snapshot(G, D, og, od, shadows=True):
    out = [p.detach().clone() for p in list(G.parameters()) + list(D.parameters())]
    out += [og._m.clone(), og._v.clone(), od._m.clone(), od._v.clone(), og._step_dev.clone(), od._step_dev.clone()]
    if shadows:
        out += [m.flat.shadow.clone() for m in (G, D) if m.flat.shadow is not None]
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dynamic_scale_is_exact_through_graphs(precision):
    in_size, step, enc, n, iters = 32, 64, 128, 16, 5
    G0, D0 = _models(in_size, step, enc)
    res = {}
    for scaled in (False, True):
        torch.manual_seed(11)
        G, D, og, od = product_pair(in_size, step, enc, precision, G0, D0)
        sc = DynamicLossScaler(init_scale=16.0, growth_interval=1).attach(G, D) if scaled else None
        lg, ld, lp = _plugins()
        losses, graphs = [], []
        for it in range(iters):
            real = R.synthetic_images(n, in_size, seed=100 + it).cuda()
            losses.append((lg.train_ops(G, D, og, "cuda", n), ld.train_ops(G, D, od, real, "cuda"),
                           lp.train_ops(G, D, od, real, "cuda")))
            graphs.append(tuple(len(p._runner._graphs) for p in (lg, ld, lp)))
        torch.cuda.synchronize()
        res[scaled] = (losses, [p.detach().clone() for p in list(G.parameters()) + list(D.parameters())],
                       [b.detach().clone() for b in list(G.buffers()) + list(D.buffers())],
                       [og._m.clone(), og._v.clone(), od._m.clone(), od._v.clone()], graphs,
                       any(sg.graph is not None for p in (lg, ld, lp) for sg in p._runner._graphs.values()))
        if scaled:
            assert sc.get_scale() == 16.0 * 2.0 ** (3 * iters)      # doubled after every train_op, below the cap
            assert sc.skipped_steps() == 0
            assert int(og._step_dev.item()) == iters and int(od._step_dev.item()) == 2 * iters
    assert res[True][5], "the step graphs were never captured"
    assert res[False][0] == res[True][0]
    for k in (1, 2, 3):
        for a, b in zip(res[False][k], res[True][k]):
            assert torch.equal(a, b)
    assert res[False][4] == res[True][4]              # no extra graphs while the scale changes


def _fp16_run(iters, scaler_kw=None, static=None):
    in_size, step, enc, n = 32, 64, 128, 16
    G0, D0 = _models(in_size, step, enc)
    torch.manual_seed(5)
    G, D, og, od = product_pair(in_size, step, enc, "fp16", G0, D0)
    sc = DynamicLossScaler(**scaler_kw).attach(G, D) if scaler_kw is not None else None
    og._ensure(); od._ensure()                                    # moment / step buffers exist before the first snapshot
    if static is not None:
        for m in (G, D):
            ops, _ = m.runtime()
            ops.loss_scale, ops.gp_seed_scale, ops.gp_tangent_scale = static
    return G, D, og, od, sc, _plugins(), in_size, n


def test_fp16_overflow_is_skipped_and_training_recovers():
    k0 = 40
    G, D, og, od, sc, (lg, ld, lp), in_size, n = _fp16_run(0, {"init_scale": 2.0 ** k0, "growth_interval": 10 ** 6})
    start = [p.detach().clone() for p in list(G.parameters()) + list(D.parameters())]
    skipped, last_losses = 0, None
    for it in range(16):
        real = R.synthetic_images(n, in_size, seed=300 + it).cuda()
        row = []
        for name, fn in (("g", lambda: lg.train_ops(G, D, og, "cuda", n)), ("d", lambda: ld.train_ops(G, D, od, real, "cuda")),
                         ("gp", lambda: lp.train_ops(G, D, od, real, "cuda"))):
            # (the 16-bit shadows are first written by the first forward pass, not by an optimizer step)
            before = _snapshot(G, D, og, od, shadows=it > 0)
            row.append(fn())
            now = sc.skipped_steps()
            if now > skipped:
                assert now == skipped + 1
                for a, b in zip(before, _snapshot(G, D, og, od, shadows=it > 0)):
                    assert torch.equal(a, b), (it, name)          # bit-exact no-op, replayed steps included
            skipped = now
            assert sc.get_scale() == 2.0 ** (k0 - skipped)        # no growth here: S and the skip count agree
            for t in (og._m, og._v, od._m, od._v):
                assert bool(torch.isfinite(t).all())
        last_losses = row
    assert skipped >= 3
    assert np.all(np.isfinite(last_losses))
    end = [p.detach() for p in list(G.parameters()) + list(D.parameters())]
    assert all(bool(torch.isfinite(p).all()) for p in end)
    assert any(not torch.equal(a, b) for a, b in zip(start, end))
    assert int(og._step_dev.item()) + int(od._step_dev.item()) == 3 * 16 - skipped
    # Adam.state_dict() reports the device counters (skipped steps do not count), not the number of steps enqueued
    for o in (og, od):
        assert float(o.state_dict()["state"][0]["step"]) == float(o._step_dev.item())


def test_fp16_same_start_as_static_scale_goes_non_finite():
    """The control: 2^40 as a STATIC scale (forced, as tests/test_fp16_gpu.py forces its scales) poisons the parameters."""
    G, D, og, od, _, (lg, ld, lp), in_size, n = _fp16_run(0, None, static=(2.0 ** 40, 2.0 ** 20, 2.0 ** 20))
    for it in range(2):
        real = R.synthetic_images(n, in_size, seed=300 + it).cuda()
        lg.train_ops(G, D, og, "cuda", n); ld.train_ops(G, D, od, real, "cuda"); lp.train_ops(G, D, od, real, "cuda")
    assert not all(bool(torch.isfinite(p).all()) for p in list(G.parameters()) + list(D.parameters()))


# ---------------------------------------------------------------------------------------------------------- kernel level
def _probe_and_hyper(lib, st, segs, step_dev, hyper, slot=0):
    k = len(segs)
    ptrs = (C.c_void_p * k)(*[s[0] for s in segs])
    ns = (C.c_ulonglong * k)(*[s[1] for s in segs])
    dts = (C.c_int * k)(*[s[2] for s in segs])
    _abi.check(lib.rg_nonfinite_probe(k, C.addressof(ptrs), C.addressof(ns), C.addressof(dts),
                                      st.data_ptr() + 4 * (FLAG + slot), None), "probe")
    _abi.check(lib.rg_adam_hyper_dev3(step_dev.data_ptr(), 1e-3, 0.5, 0.999, 1e-8, 0.0, st.data_ptr(), slot, hyper.data_ptr(),
                                      None), "hyper3")


def _state(k):
    st = torch.zeros(12, dtype=torch.int32, device="cuda")
    st[0] = k; st[4] = k
    return st


def _adam_buffers(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).cuda()
    m = (torch.randn(n, generator=g) * 0.01).cuda()
    v = (torch.rand(n, generator=g) * 1e-4).cuda()
    return p, m, v


def _conv_shape(lib, H16):
    # the smallest of these layer shapes whose weight gradient has a plan without split-K (rg_conv_wgrad_adam_supported)
    for shape in ((64, 4, 256, 256), (64, 4, 512, 512), (64, 4, 2048, 1024)):
        if lib.rg_conv_wgrad_adam_supported(shape[0], shape[1], shape[1], shape[2], shape[3], 0, H16, _abi.ALGO_AUTO) == 1:
            return shape
    return None


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("source", ["grad", "wire", "slab", "g0", "conv"])
def test_kernel_skip_and_identity(half, source):
    lib = _abi.load(half)
    H16 = _abi.RG_F16 if half == "f16" else _abi.RG_BF16
    h16 = torch.float16 if half == "f16" else torch.bfloat16
    n = 4096 + 12                                                 # a tail that is not a multiple of 4 (plain form)
    gen = torch.Generator().manual_seed(3)
    grad = torch.randn(n, generator=gen).cuda() * 8.0            # scale 8: carries 2^3, removed by hyper[8]
    wire = grad.to(h16)
    nsp, ns_n = 3, 1024
    slab = (torch.randn(nsp, ns_n, generator=gen) * 8.0).cuda()
    E, Cc, K = 64, 16, 64                                         # G.0: [E][C][4][4] fp32 weight, K samples
    z = torch.randn(K, E, generator=gen).cuda()
    gz0 = (torch.randn(K, Cc * 16, generator=gen) * 8.0).cuda().to(h16)
    results = {}
    for guarded, poison in ((False, False), (True, False), (True, True)):
        hyper = torch.zeros(12, device="cuda")
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = _state(3)
        gr, wr, sl, gz = grad.clone(), wire.clone(), slab.clone(), gz0.clone()
        if poison:
            if source != "conv":
                {"grad": gr, "wire": wr, "slab": sl, "g0": gz}[source].view(-1)[17] = float("inf")
        if source == "g0":
            p, m, v = _adam_buffers(E * Cc * 16, 7)
            segs = [(z.data_ptr(), z.numel(), _abi.RG_F32), (gz.data_ptr(), gz.numel(), H16)]
        elif source == "conv":
            shape = _conv_shape(lib, H16)
            if shape is None:
                pytest.skip("this build has no single-launch weight-gradient plan")
            cN, chs, cO, cI = shape
            p, m, v = _adam_buffers(cO * 16 * cI, 7)
            cg = torch.Generator().manual_seed(9)
            low = torch.randn(cN, chs, chs, cO, generator=cg).cuda().to(h16)
            high = torch.randn(cN, 2 * chs, 2 * chs, cI, generator=cg).cuda().to(h16)
            if poison:
                low.view(-1)[17] = float("inf")
            segs = [(low.data_ptr(), low.numel(), H16), (high.data_ptr(), high.numel(), H16)]
        else:
            p, m, v = _adam_buffers(n if source != "slab" else ns_n, 7)
            segs = {"grad": [(gr.data_ptr(), n, _abi.RG_F32)], "wire": [(wr.data_ptr(), n, H16)],
                    "slab": [(sl.data_ptr(), sl.numel(), _abi.RG_F32)]}[source]
        if guarded:
            _probe_and_hyper(lib, st, segs, step_dev, hyper)
        else:
            _abi.check(lib.rg_adam_hyper_dev2(step_dev.data_ptr(), 1e-3, 0.5, 0.999, 1e-8, 0.0, 1.0 / 8.0, hyper.data_ptr(),
                                              None), "hyper2")
        shadow = torch.zeros(p.numel(), dtype=h16, device="cuda") if source != "grad" else None
        sh = 0 if shadow is None else shadow.data_ptr()
        if source == "grad":
            _abi.check(lib.rg_adam_step_dev(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), None,
                                            None, None), "adam")
        elif source == "wire":
            _abi.check(lib.rg_adam_step_dev(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n - 12, hyper.data_ptr(),
                                            sh, wr.data_ptr(), None), "adam wire")
        elif source == "slab":
            offs = (C.c_ulonglong * 1)(0); lens = (C.c_ulonglong * 1)(ns_n)
            slabs = (C.c_void_p * 1)(sl.data_ptr()); nsa = (C.c_int * 1)(nsp); dts = (C.c_int * 1)(_abi.RG_F32)
            _abi.check(lib.rg_adam_step_slabs(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), ns_n, hyper.data_ptr(),
                                              sh, 1, C.addressof(offs), C.addressof(lens), C.addressof(slabs),
                                              C.addressof(nsa), C.addressof(dts), None), "adam slabs")
        elif source == "g0":
            _abi.check(lib.rg_g0_wgrad_adam(z.data_ptr(), gz.data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(),
                                            hyper.data_ptr(), sh, K, E, Cc, H16, None), "g0 adam")
        else:
            _abi.check(lib.rg_conv_wgrad_adam(low.data_ptr(), high.data_ptr(), None, None, p.data_ptr(), m.data_ptr(),
                                              v.data_ptr(), hyper.data_ptr(), sh, cN, chs, chs, cO, cI, H16, _abi.ALGO_AUTO,
                                              None), "conv adam")
        torch.cuda.synchronize()
        results[(guarded, poison)] = (p, m, v, shadow, int(step_dev.item()), int(st[FLAG].item()))
    ref, ok, bad = results[(False, False)], results[(True, False)], results[(True, True)]
    for a, b in zip(ref[:3], ok[:3]):
        assert torch.equal(a, b)                                   # guarded == unguarded without a non-finite value
    assert ok[4] == 1 and ok[5] == 0
    p0, m0, v0 = _adam_buffers(bad[0].numel(), 7)
    assert torch.equal(bad[0], p0) and torch.equal(bad[1], m0) and torch.equal(bad[2], v0)     # whole step: a no-op
    if bad[3] is not None:
        assert not bool(bad[3].float().abs().sum())               # the shadow was not written either
    assert bad[4] == 0 and bad[5] == 1                             # the step counter did not advance


def test_amp_update_kernel_follows_the_rule():
    lib = _abi.load()
    st = _state(10)
    rule_state = (10, 0, 0)
    for found in (False, False, True, False, False, False, True, True):
        if found:
            st[FLAG] = 1
        _abi.check(lib.rg_amp_update(st.data_ptr(), 0, 3, 8, 11, None), "update")
        rule_state = DynamicLossScaler.update_rule(*rule_state, found, 3, 8, 11)
        got = st.cpu().tolist()
        assert (got[0], got[1], got[2]) == rule_state and got[FLAG] == 0


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("dtype", ["f32", "h16"])
def test_probe_head_body_tail(half, dtype):
    """rg_nonfinite_probe on segments that start off a 16-byte boundary and end off one (the product's segments start at flat
    offsets): one inf in the head element, the vector body or the tail element is found; a finite segment is not flagged."""
    lib = _abi.load(half)
    tdt = torch.float32 if dtype == "f32" else (torch.float16 if half == "f16" else torch.bfloat16)
    code = _abi.RG_F32 if dtype == "f32" else (_abi.RG_F16 if half == "f16" else _abi.RG_BF16)
    per16 = 16 // torch.tensor([], dtype=tdt).element_size()
    base = torch.randn(4096, generator=torch.Generator().manual_seed(1)).cuda().to(tdt)
    for start in range(per16):
        for length in (1, per16 - 1, 3 * per16 + 1, 1000 + start):
            if start + length > base.numel():
                continue
            for where in (None, 0, length // 2, length - 1):
                buf = base.clone()
                if where is not None:
                    buf[start + where] = float("inf") if where % 2 == 0 else float("nan")
                # a non-finite value just outside the segment must not be seen
                if start > 0:
                    buf[start - 1] = float("inf")
                if start + length < buf.numel():
                    buf[start + length] = float("nan")
                flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                ptrs = (C.c_void_p * 1)(buf.data_ptr() + start * buf.element_size())
                ns = (C.c_ulonglong * 1)(length)
                dts = (C.c_int * 1)(code)
                _abi.check(lib.rg_nonfinite_probe(1, C.addressof(ptrs), C.addressof(ns), C.addressof(dts), flag.data_ptr(),
                                                  None), "probe")
                assert int(flag.item()) == (0 if where is None else 1), (start, length, where)
