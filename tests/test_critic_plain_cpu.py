"""BatchNorm-free critic, DCGANDiscriminator(batchnorm=False), without a GPU: the product module mirrors the oracle module's
keys, and the engine's sequencing for it (engine.PlainDiscNet) driven by a float64 CPU twin reproduces torch autograd on the
oracle modules -- the three steps, every weight AND bias gradient, the paired / batched / prefix-rest forms of the D step, and
the penalty step, whose bias gradients are exactly zero."""
import copy
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_cpu as R
from oracle.ops_ref import RefOps, _lrelu_mask, _nhwc
from rna_gan_amd import engine as E
from rna_gan_amd import models as M


class PlainRefOps(RefOps):
    """RefOps plus the ops the BatchNorm-free critic adds (rna_gan_amd.ops_hip.HipOps has the same six)."""

    def conv_down_bias_act(self, x, cw, bias, slope):
        y = F.conv2d(self._nchw(x), self._wq(cw.oihw()), bias.to(self.f), stride=2, padding=1)
        return _nhwc(F.leaky_relu(y, slope), self.act_dtype)

    def conv_down_mask(self, x, cw, mask_act, slope):
        y = F.conv2d(self._nchw(x), self._wq(cw.oihw()), None, stride=2, padding=1)
        return _nhwc(y * _lrelu_mask(self._nchw(mask_act), slope), self.act_dtype)

    def conv_up_mask(self, x, cw, mask_act, slope, dbias=None, accumulate=False):
        y = self.conv_up(x, cw, mask_act, slope)
        if dbias is not None:
            self.col_sum(y, dbias, accumulate)
        return y

    def head_fwd_bias(self, a, cw, bias, slope):
        h = torch.einsum("nijc,cij->n", a.to(self.f), self._wq(cw.w)[0]) + bias.to(self.f)
        return h, F.leaky_relu(h, slope)

    def vec_sum(self, v, out, accumulate):
        s = v.to(self.f).sum().reshape(1)
        if accumulate:
            out.add_(s)
        else:
            out.copy_(s)

    def zero_(self, t):
        return t.zero_()


def mk(in_size, step, enc, seed=5):
    G = R.seeded_fill_(R.OracleDCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2),
                                              last_nonlinearity=nn.Tanh()), seed)
    D = R.seeded_fill_(R.OracleDCGANDiscriminator(in_size, 3, step, batchnorm=False, nonlinearity=nn.LeakyReLU(0.2),
                                                  last_nonlinearity=nn.LeakyReLU(0.2)), seed + 1)
    return G.double(), D.double()


def grads_of(mod):
    return {k: p.grad.clone() for k, p in mod.named_parameters()}


def assert_close_dict(a, b, rtol, atol):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_allclose(a[k].double().numpy(), b[k].double().numpy(), rtol=rtol, atol=atol, err_msg=k)


@pytest.mark.parametrize("in_size", [16, 32, 64])
def test_module_keys_and_shapes_equal_the_oracle(in_size):
    ours = M.DCGANDiscriminator(in_size, 3, 4, batchnorm=False)
    ref = R.OracleDCGANDiscriminator(in_size, 3, 4, batchnorm=False)
    so, sr = ours.state_dict(), ref.state_dict()
    assert list(so.keys()) == list(sr.keys())
    assert all(so[k].shape == sr[k].shape and so[k].dtype == sr[k].dtype for k in so)
    reps = in_size.bit_length() - 4
    want = ["model.%d.0.%s" % (i, w) for i in range(reps + 1) for w in ("weight", "bias")] + ["disc.0.weight", "disc.0.bias"]
    assert list(so.keys()) == want
    assert not any(isinstance(m, nn.BatchNorm2d) for m in ours.modules())
    R.seeded_fill_(ref, 3)
    ours.load_state_dict(ref.state_dict())
    ref2 = R.OracleDCGANDiscriminator(in_size, 3, 4, batchnorm=False)
    ref2.load_state_dict(ours.state_dict())
    for k in sr:
        assert torch.equal(ref2.state_dict()[k], ref.state_dict()[k])
    # the weight initialiser zeroes the new biases like every other (torchgan recipe)
    fresh = M.DCGANDiscriminator(in_size, 3, 4, batchnorm=False)
    assert all(float(p.detach().abs().max()) == 0.0 for k, p in fresh.named_parameters() if k.endswith("bias"))
    # tap-major re-homing covers the biased middle convs and keeps the keys
    E.tap_major_(ours)
    assert sum(E.is_tap_major(p.data) for p in ours.parameters()) == reps
    assert isinstance(E.build_disc_net(ours), E.PlainDiscNet)
    assert isinstance(E.build_disc_net(M.DCGANDiscriminator(in_size, 3, 4)), E.DiscNet)
    # generators keep refusing the recipe
    with pytest.raises(NotImplementedError):
        M.DCGANGenerator(16, in_size, 3, 4, batchnorm=False)


@pytest.mark.parametrize("in_size,step,enc,n,tap_major", [(16, 8, 16, 4, False), (32, 8, 16, 4, False),
                                                          (16, 8, 16, 4, True), (32, 8, 16, 4, True)])
def test_three_steps_match_autograd(in_size, step, enc, n, tap_major):
    torch.manual_seed(0)
    G, D = mk(in_size, step, enc)
    G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
    for m in (G, D, G2, D2):
        m.train()
    if tap_major:
        E.tap_major_(G2), E.tap_major_(D2)
        assert any(E.is_tap_major(p.data) for p in D2.parameters())
    real = R.synthetic_images(n, in_size, seed=3).double()
    noise = R.synthetic_normal(n, enc, seed=4).double()
    ops = PlainRefOps(torch.float64)
    Gn, Dn = E.build_gen_net(G2), E.build_disc_net(D2)
    assert isinstance(Dn, E.PlainDiscNet) and len(Dn.blocks) == in_size.bit_length() - 4
    biases = [k for k, _ in D.named_parameters() if k.endswith("bias")]
    assert len(biases) == len(Dn.blocks) + 2

    # ---- G step: generator gradients through the critic's data-gradient chain
    for p in list(G.parameters()) + list(D.parameters()):
        p.grad = None
    loss_o = R.generator_loss(D(G(noise)))
    loss_o.backward()
    loss_e = E.gen_loss_grads(ops, Gn, Dn, noise)
    np.testing.assert_allclose(float(loss_e), float(loss_o), rtol=1e-9)
    assert_close_dict(grads_of(G2), grads_of(G), 1e-7, 1e-10)

    # ---- D step: every weight and bias, in the paired, batched and prefix / rest forms
    for p in D.parameters():
        p.grad = None
    loss_o = R.discriminator_loss(D(real), D(G(noise).detach()))
    loss_o.backward()
    want = grads_of(D)
    # (the head's own bias gradient is sum_n gh_n: it cancels exactly when every h_n has the same sign)
    assert all(float(want[k].abs().max()) > 0 for k in biases if not k.startswith("disc."))

    def poison():
        for p in D2.parameters():
            p.grad.fill_(123.0)                         # the step WRITES: nothing of this may survive
    poison()
    loss_e = E.disc_loss_grads(ops, Gn, Dn, real, noise)           # disc_backward_pair
    np.testing.assert_allclose(float(loss_e), float(loss_o), rtol=1e-9)
    assert_close_dict(grads_of(D2), want, 1e-9, 1e-12)
    poison()
    loss_e = E.disc_loss_grads_batched(ops, Gn, Dn, real, noise)   # one 2N batch
    np.testing.assert_allclose(float(loss_e), float(loss_o), rtol=1e-9)
    assert_close_dict(grads_of(D2), want, 1e-9, 1e-12)
    poison()
    loss_e, fake_next = E.disc_loss_grads_batched(ops, Gn, Dn, real, noise, next_noise=noise.flip(0))
    np.testing.assert_allclose(float(loss_e), float(loss_o), rtol=1e-9)
    assert_close_dict(grads_of(D2), want, 1e-9, 1e-12)
    np.testing.assert_allclose(fake_next.numpy(), G(noise.flip(0)).detach().numpy(), rtol=1e-9, atol=1e-12)
    for backward in ("all", "dgrad"):
        poison()
        pre = E.disc_loss_prefix(ops, Dn, real, backward)
        assert pre.backward == backward and (pre.ctx_r is None) == (backward == "all")
        loss_s = E.disc_loss_rest(ops, Gn, Dn, pre, noise)
        np.testing.assert_allclose(float(loss_s), float(loss_o), rtol=1e-9)
        assert_close_dict(grads_of(D2), want, 1e-9, 1e-12)
    G2.load_state_dict(G.state_dict())                  # undo the generator's extra running-statistics updates

    # ---- penalty step: value, weight gradients, and bias gradients that are exactly zero
    for p in D.parameters():
        p.grad = None
    eps = 0.3
    xhat = eps * real + (1 - eps) * G(noise)
    gp = R.gradient_penalty(xhat, D(xhat))
    (10.0 * gp).backward()
    want = grads_of(D)
    assert all(want[k] is not None and float(want[k].abs().max()) == 0.0 for k in biases)     # what the oracle does
    poison()
    loss_e = E.gp_loss_grads(ops, Gn, Dn, real, noise, eps, 10.0)
    np.testing.assert_allclose(float(loss_e), float(gp), rtol=1e-9)
    got = grads_of(D2)
    assert_close_dict(got, want, 1e-9, 1e-12)
    for k in biases:
        assert torch.equal(got[k], torch.zeros_like(got[k])), k

    # ---- the penalty's pieces: accumulate=True adds nothing to the biases; the input gradient is zeros
    for p in D2.parameters():
        p.grad.fill_(0.5)
    x = xhat.detach().clone()
    _, ctx = E.disc_forward(ops, Dn, x)
    loss, (g, v) = E.disc_gp_first(ops, Dn, ctx, 1.0)
    np.testing.assert_allclose(float(loss), float(gp), rtol=1e-9)
    gx = E.disc_gp_second(ops, Dn, ctx, (g, 10.0 * v), accumulate=True, need_input_grad=True)
    assert gx.shape == x.shape and torch.equal(gx, torch.zeros_like(x))
    got = grads_of(D2)
    for k in biases:
        assert torch.equal(got[k], torch.full_like(got[k], 0.5)), k
    assert_close_dict({k: t - 0.5 for k, t in got.items()}, want, 1e-9, 1e-11)
    # torch agrees that the penalty does not depend on x beyond the mask pattern
    xr = x.clone().requires_grad_(True)
    gx_o, = torch.autograd.grad(R.gradient_penalty(xr, D(xr)), xr, allow_unused=True)
    assert gx_o is None or float(gx_o.abs().max()) == 0.0


def test_autograd_cotangents_features_and_eval():
    """The per-sample cotangent form of disc_backward (what models._DiscForwardFn hands over), the feature-matching
    activation and the eval-mode forward, which equals the train-mode one for this net."""
    torch.manual_seed(0)
    _, D = mk(32, 8, 16)
    D2 = copy.deepcopy(D)
    ops = PlainRefOps(torch.float64)
    Dn = E.build_disc_net(D2)
    x = R.synthetic_images(4, 32, seed=3).double().requires_grad_(True)
    cot = torch.tensor([0.25, -1.5, 0.0, 2.0], dtype=torch.float64)      # (fp32-exact: the engine takes them as fp32)
    out_o = D(x)
    (out_o * cot).sum().backward()
    for p in D2.parameters():
        p.grad.fill_(0.25)
    out, ctx = E.disc_forward(ops, Dn, x.detach().clone())
    np.testing.assert_allclose(out.numpy(), out_o.detach().numpy(), rtol=1e-10, atol=1e-13)
    gx = E.disc_backward(ops, Dn, ctx, cot, wgrad=True, accumulate=True, need_input_grad=True)
    np.testing.assert_allclose(gx.numpy(), x.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert_close_dict({k: t - 0.25 for k, t in grads_of(D2).items()}, grads_of(D), 1e-9, 1e-11)
    feats = E.disc_features_eval(ops, Dn, x.detach().clone())
    want = D.model(x.detach())
    np.testing.assert_allclose(feats.permute(0, 3, 1, 2).numpy(), want.detach().numpy(), rtol=1e-10, atol=1e-13)
    D.eval()
    np.testing.assert_allclose(E.disc_forward_eval(ops, Dn, x.detach().clone()).numpy(), D(x.detach()).detach().numpy(),
                               rtol=1e-10, atol=1e-13)


def test_losses_decline_the_deferred_forms_for_the_plain_net():
    """The deferred-slab / wire forms of rna_gan_amd.train_op gate on engine.DiscNet: PlainDiscNet is not one."""
    from rna_gan_amd import train_op as L
    D2 = M.DCGANDiscriminator(32, 3, 8, batchnorm=False)
    Dn = E.build_disc_net(E.tap_major_(D2))
    assert not isinstance(Dn, (E.GenNet, E.DiscNet))

    class HalfOps:
        act_dtype, stat_reduce = torch.bfloat16, None
    assert not L._local_half_dcgan(HalfOps(), Dn)
    assert L._local_half_dcgan(HalfOps(), E.build_disc_net(E.tap_major_(M.DCGANDiscriminator(32, 3, 8))))


def test_cli_accepts_critic_batchnorm(monkeypatch):
    import histopathology_gan as H
    monkeypatch.setattr(sys, "argv", ["histopathology_gan.py", "--config", "c.json", "--critic_batchnorm", "0"])
    assert H.parse_args().critic_batchnorm == 0
    monkeypatch.setattr(sys, "argv", ["histopathology_gan.py", "--config", "c.json"])
    assert H.parse_args().critic_batchnorm == 1
