"""Wasserstein losses with the reference's ``train_ops`` plugin interface.

Two families, selected by ``--loss_type`` in the reference CLI (src/histopathology_gan.py:265-278):
  * ``wganvae``: WassersteinGeneratorLossVAE / WassersteinDiscriminatorLossVAE /
    WassersteinGradientPenaltyVAE -- reference source src/wgan_loss.py:47-129,131-263,266-389.
    Same constructor arguments, same ``train_ops`` argument names (the Trainer resolves them by
    name), same RNG calls (uniform noise drawn on the CPU generator, ``torch.rand(1)`` for eps), same
    return value (python float; the penalty is returned unweighted).
  * ``wgan``: the stock torchgan losses (third-party, recalled in SURVEY Appendix A): randn noise
    on the device, tensor ``real_inputs``, optional weight clamp.

What differs from the reference, deliberately: the gradient computation is the explicit HIP
sequencing in rna_gan_amd.engine instead of autograd; work the reference computes and throws away
(discriminator weight grads in the G step, generator grads in the GP step, betaVAE grads) is not
computed; in a data-parallel run the flat gradient buffer is all-reduced before the optimizer step.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import engine as E
from .betavae import betaVAE
from .train_op import _dispatch, _g_body, _lookahead_ok, d_train_op, gp_train_op      # the scheduler: how a plugin's train_op runs
# Names others reach through this module.  Of the switches DP_ROUTE alone: a stale ``losses.G0_ADAM`` must raise, not set a dead copy
from .train_op import _Runner                        # loss objects are pickled into checkpoints, which name losses._Runner
from .train_op import flush                          # noqa: F401  callers apply a pending data-parallel step next to the plugins
from .train_op import _g_step, _d_step, _gp_step     # noqa: F401  the eager train_ops that smoke() and the parity tests call
from .train_op import _FAKE                          # new_batch() clears it: never rebound, only mutated
from .train_op import DP_ROUTE                       # noqa: F401  bench.py reads it once, for its config record


def reduce(x, reduction=None):
    if reduction == "mean":
        return torch.mean(x)
    if reduction == "sum":
        return torch.sum(x)
    return x


def wasserstein_generator_loss(fgz, reduction="mean"):
    return reduce(-1.0 * fgz, reduction)


def wasserstein_discriminator_loss(fx, fgz, reduction="mean"):
    return reduce(fgz - fx, reduction)


# the *_vae functional forms ignore their reduction argument (src/wgan_loss.py:24-29)
def wasserstein_generator_loss_vae(fgz, reduction="mean"):
    return reduce(-1.0 * fgz, "mean")


def wasserstein_discriminator_loss_vae(fx, fgz, reduction="mean"):
    return reduce(fgz - fx, "mean")


class _GradientPenaltyFn(torch.autograd.Function):
    """(||d sum(d_interpolate) / d interpolate||_2 - 1)^2 as a differentiable scalar, for discriminator outputs produced
    by the HIP discriminator under autograd (models._DiscForwardFn).  torch cannot differentiate through that node a
    second time, so this Function takes the node's saved forward context and runs the engine's explicit second-order
    pass (engine.disc_gp_first / disc_gp_second: tangent forward + joint reverse) in its own backward: parameter
    gradients are ADDED into the flat gradient buffer, the gradient with respect to ``interpolate`` is returned."""

    @staticmethod
    def forward(ctx, interpolate, d_interpolate, *params):
        node = d_interpolate.grad_fn
        module, dctx = getattr(node, "module", None), getattr(node, "dctx", None)
        if module is None or dctx is None:
            raise RuntimeError("wasserstein_gradient_penalty: d_interpolate must be the direct output of a rna_gan_amd "
                               "discriminator called on `interpolate` with gradients enabled")
        if dctx.x.data_ptr() != interpolate.data_ptr() and not torch.equal(dctx.x, interpolate.detach().float()):
            raise RuntimeError("wasserstein_gradient_penalty: d_interpolate was not computed from this `interpolate`")
        ops, net = module.runtime()
        loss, st = E.disc_gp_first(ops, net, dctx, 1.0)
        ctx.module, ctx.dctx, ctx.st = module, dctx, st
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        ops, net = ctx.module.runtime()
        g, v = ctx.st
        scale = float(gloss)                      # host sync: this is the public functional form, not the hot path
        v = v if scale == 1.0 else v * scale      # v is linear in the upstream gradient (v = dL/dg)
        gx = E.disc_gp_second(ops, net, ctx.dctx, (g, v), accumulate=True, need_input_grad=ctx.needs_input_grad[0])
        return (gx, None) + (None,) * (len(ctx.module._rt_flat.params))


def wasserstein_gradient_penalty(interpolate, d_interpolate, reduction="mean"):
    """torchgan.losses.functional.wasserstein_gradient_penalty / src/wgan_loss.py:32-44: the squared distance from 1 of
    the 2-norm (over the WHOLE batch) of d sum(d_interpolate) / d interpolate.  ``d_interpolate`` must come from a
    rna_gan_amd discriminator applied to ``interpolate`` (requires_grad=True) with gradients enabled; the result is
    a scalar that can be back-propagated (see _GradientPenaltyFn)."""
    fn = d_interpolate.grad_fn
    module = getattr(fn, "module", None)
    if module is None:
        raise RuntimeError("wasserstein_gradient_penalty: d_interpolate carries no rna_gan_amd discriminator graph "
                           "(call the discriminator on an `interpolate` that requires grad, gradients enabled)")
    gp = _GradientPenaltyFn.apply(interpolate, d_interpolate, *module._rt_flat.params)
    return reduce(gp, reduction)


def wasserstein_gradient_penalty_vae(interpolate, d_interpolate, reduction="mean"):
    """src/wgan_loss.py:32-44 (the reduction argument is ignored there: always the mean of the scalar)."""
    return wasserstein_gradient_penalty(interpolate, d_interpolate, "mean")


class GeneratorLoss(nn.Module):
    def __init__(self, reduction="mean", override_train_ops=None):
        super().__init__()
        self.reduction = reduction
        self.override_train_ops = override_train_ops
        self.arg_map = {}

    def set_arg_map(self, value):
        self.arg_map.update(value)


class DiscriminatorLoss(nn.Module):
    def __init__(self, reduction="mean", override_train_ops=None):
        super().__init__()
        self.reduction = reduction
        self.override_train_ops = override_train_ops
        self.arg_map = {}

    def set_arg_map(self, value):
        self.arg_map.update(value)


def _pinned(*shape):
    return torch.empty(*shape, dtype=torch.float32, pin_memory=torch.cuda.is_available())


def _check_labels(generator, discriminator, labels):
    if generator.label_type != "none" or discriminator.label_type != "none":
        raise NotImplementedError("label-conditioned GANs are not on the RNA-GAN DCGAN path")


_NEXT_NOISE = [None]            # Trainer flow: the penalty step's noise, drawn by the D-loss plugin right after its own
TRAINER_LOOKAHEAD = [False]     # set by Trainer when a gradient-penalty plugin directly follows the D-loss plugin


# ------------------------------------------------------------------------------------------------
# stock losses (--loss_type wgan)
# ------------------------------------------------------------------------------------------------
class WassersteinGeneratorLoss(GeneratorLoss):
    def __init__(self, reduction="mean", override_train_ops=None):
        super().__init__(reduction, override_train_ops)
        self._runner = _Runner()

    def forward(self, fgz):
        return wasserstein_generator_loss(fgz, self.reduction)

    def step(self, generator, discriminator, optimizer_generator, noise):
        """The train_op body on explicit inputs; returns the loss as a 1-element device tensor."""
        return _dispatch(self._runner, ("g",), _g_body(generator, discriminator), [noise],
                         generator, discriminator, generator, optimizer_generator)

    def train_ops_async(self, generator, discriminator, optimizer_generator, device, batch_size, labels=None):
        _check_labels(generator, discriminator, labels)
        noise = torch.randn(batch_size, generator.encoding_dims, device=device)
        return self.step(generator, discriminator, optimizer_generator, noise)

    def train_ops(self, generator, discriminator, optimizer_generator, device, batch_size, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_generator, device, batch_size, labels).item()
    train_ops._rg_async = "train_ops_async"


class WassersteinDiscriminatorLoss(DiscriminatorLoss):
    def __init__(self, reduction="mean", clip=None, override_train_ops=None):
        super().__init__(reduction, override_train_ops)
        self.clip = clip if isinstance(clip, (tuple, list)) and len(clip) > 1 else None
        self._runner = _Runner()

    def forward(self, fx, fgz):
        return wasserstein_discriminator_loss(fx, fgz, self.reduction)

    def step(self, generator, discriminator, optimizer_discriminator, real, noise, next_noise=None):
        """next_noise: the noise tensor the gradient-penalty step of this iteration will be called with (train_op.d_train_op)."""
        return d_train_op(self._runner, generator, discriminator, optimizer_discriminator, self.clip, real, [noise], None, next_noise)

    def train_ops_async(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        _check_labels(generator, discriminator, labels)
        batch_size = real_inputs.size(0)
        noise = torch.randn(batch_size, generator.encoding_dims, device=device)
        nxt = None
        if TRAINER_LOOKAHEAD[0] and _lookahead_ok():       # the penalty plugin's randn, drawn now (same generator order)
            nxt = _NEXT_NOISE[0] = torch.randn(batch_size, generator.encoding_dims, device=device)
        return self.step(generator, discriminator, optimizer_discriminator, real_inputs.to(device), noise, nxt)

    def train_ops(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_discriminator, real_inputs, device, labels).item()
    train_ops._rg_async = "train_ops_async"


class WassersteinGradientPenalty(DiscriminatorLoss):
    def __init__(self, reduction="mean", lambd=10.0, override_train_ops=None):
        super().__init__(reduction, override_train_ops)
        self.lambd = lambd
        self._runner = _Runner()

    def forward(self, interpolate, d_interpolate):
        """torchgan WassersteinGradientPenalty.forward: the unweighted penalty as a differentiable scalar."""
        return wasserstein_gradient_penalty(interpolate, d_interpolate, self.reduction)

    def step(self, generator, discriminator, optimizer_discriminator, real, noise, eps):
        """eps: 1-element float32 device tensor (read inside the graph)."""
        return gp_train_op(self._runner, generator, discriminator, optimizer_discriminator, self.lambd, real,
                           lambda: [noise], noise, eps)

    def train_ops_async(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        _check_labels(generator, discriminator, labels)
        batch_size = real_inputs.size(0)
        noise, _NEXT_NOISE[0] = _NEXT_NOISE[0], None       # drawn ahead by the D-loss plugin (Trainer flow), else now
        if noise is None or noise.shape != (batch_size, generator.encoding_dims):
            noise = torch.randn(batch_size, generator.encoding_dims, device=device)
        eps = _pinned(1).uniform_(0.0, 1.0).to(device, non_blocking=True)   # CPU generator, as the reference
        return self.step(generator, discriminator, optimizer_discriminator, real_inputs.to(device), noise, eps)

    def train_ops(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_discriminator, real_inputs, device, labels).item()
    train_ops._rg_async = "train_ops_async"


# ------------------------------------------------------------------------------------------------
# betaVAE-conditioned losses (--loss_type wganvae), src/wgan_loss.py
# ------------------------------------------------------------------------------------------------
class _LatentCache:
    """z_mean = betaVAE.encode(rna)[0] of the CURRENT batch, shared by the three loss plugins.

    The reference builds three frozen betaVAE copies from one checkpoint (src/wgan_loss.py:67-69, :159-161, :289-291)
    and encodes the same RNA rows three times per iteration (:96-97, :223-224, :353-354); the result is the same
    tensor each time.  Here the first train_op of a batch encodes (its own small HIP graph), the other two reuse the
    latent when (a) they are handed the same RNA tensor (the cache keeps a reference to it, so identity by address +
    version counter is sound) and (b) their encoder holds the same weights BY PROVENANCE (betaVAE.signature(): the token of
    the checkpoint file / state_dict the weights were loaded from, valid while no tensor of the module has been written
    since -- not a fingerprint of the values).  ``new_batch()`` (called by
    Trainer.train_iter and by bench.py at the start of every iteration) drops the entry, so a latent is never carried
    from one iteration to the next even when the caller reuses one input tensor."""

    def __init__(self):
        self.key = None
        self.src = None
        self.z = None
        self.hits = 0
        self.misses = 0

    def clear(self):
        self.key, self.src, self.z = None, None, None


_LATENT = _LatentCache()
LATENT_CACHE = os.environ.get("RNAGAN_LATENT_CACHE", "1") != "0"


def new_batch():
    """Start of a new batch: forget the cached conditioning latent (and anything prepared ahead for a step that never ran)."""
    _LATENT.clear()
    _NEXT_NOISE[0] = None
    _FAKE.clear()


class _VAEMixin:
    def _init_vae(self, checkpoint, rna_features, beta):
        self.betavae = betaVAE(rna_features, 2048, [6000, 4000, 2048], [4000, 6000], beta=beta)
        if checkpoint is not None:
            self.betavae.load_checkpoint_file(checkpoint)      # weights token = the file's identity (_LatentCache)
        self.betavae.eval()
        self._runner = _Runner()
        self._enc_runner = _Runner()

    def _inputs(self, generator, real_inputs, device):
        """src/wgan_loss.py:94-101: rna (to the device, once per batch); u ~ U(-0.3, 0.3) drawn on the CPU generator."""
        batch_size = real_inputs["image"].size(0)
        if next(self.betavae.parameters()).device != torch.device(device):
            self.betavae = self.betavae.to(device)
        # same generator consumption as torch.FloatTensor(bs, E).uniform_(-0.3, 0.3); drawn into pinned
        # memory so that the copy to the device is asynchronous
        u = _pinned(batch_size, generator.encoding_dims).uniform_(-0.3, 0.3).to(device, non_blocking=True)
        return real_inputs["rna_data"], u

    def _latent(self, rna):
        """z_mean = betavae.encode(rna)[0] (src/wgan_loss.py:96-97) for this batch: from the per-batch cache, or
        encoded now (rna: host or device tensor)."""
        dev = next(self.betavae.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the betaVAE of a loss plugin must live on the GPU (call train_ops / move it with .to())")
        key = (rna.data_ptr(), rna._version, tuple(rna.shape), rna.dtype, rna.device, self.betavae.signature())
        if LATENT_CACHE and _LATENT.key == key:
            _LATENT.hits += 1
            return _LATENT.z
        _LATENT.misses += 1
        rna_dev = rna.to(dev, non_blocking=True).float().contiguous()
        z = self._enc_runner.run(("enc",), lambda r: self.betavae.encode(r, mean_only=True)[0], [rna_dev], [], [])
        _LATENT.key, _LATENT.src, _LATENT.z = key, rna, z
        return z

    def _noise(self, generator, z, u):
        """src/wgan_loss.py:100-106: noise = standardise_columns(u + z_mean)."""
        ops, _ = generator.runtime()
        return ops.latent_prep(u, z)


class WassersteinGeneratorLossVAE(GeneratorLoss, _VAEMixin):
    def __init__(self, checkpoint, rna_features, beta=0.005):
        # the reference passes (checkpoint, rna_features) positionally to the base class, so the path
        # lands in .reduction and rna_features in .override_train_ops (src/wgan_loss.py:63-66); kept.
        super().__init__(checkpoint, rna_features)
        self._init_vae(checkpoint, rna_features, beta)

    def forward(self, fgz):
        return wasserstein_generator_loss_vae(fgz, self.reduction)

    def step(self, generator, discriminator, optimizer_generator, rna, u):
        return _dispatch(self._runner, ("g",), _g_body(generator, discriminator, lambda z, uu: self._noise(generator, z, uu)),
                         [self._latent(rna), u], generator, discriminator, generator, optimizer_generator)

    def train_ops_async(self, generator, discriminator, optimizer_generator, device, batch_size, real_inputs, labels=None):
        _check_labels(generator, discriminator, labels)
        rna, u = self._inputs(generator, real_inputs, device)
        return self.step(generator, discriminator, optimizer_generator, rna, u)

    def train_ops(self, generator, discriminator, optimizer_generator, device, batch_size, real_inputs, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_generator, device, batch_size, real_inputs, labels).item()
    train_ops._rg_async = "train_ops_async"


class WassersteinDiscriminatorLossVAE(DiscriminatorLoss, _VAEMixin):
    def __init__(self, checkpoint, rna_features, beta=0.005, reduction="mean", clip=None, override_train_ops=None):
        super().__init__(checkpoint, rna_features)
        self.clip = clip if isinstance(clip, (tuple, list)) and len(clip) > 1 else None
        self._init_vae(checkpoint, rna_features, beta)

    def forward(self, fx, fgz):
        return wasserstein_discriminator_loss_vae(fx, fgz, self.reduction)

    def step(self, generator, discriminator, optimizer_discriminator, real, rna, u, next_u=None):
        """next_u: the uniform draw the gradient-penalty step of this iteration will be called with, same RNA batch (d_train_op)."""
        return d_train_op(self._runner, generator, discriminator, optimizer_discriminator, self.clip, real,
                          [self._latent(rna), u], lambda z, uu: self._noise(generator, z, uu), next_u)

    def train_ops_async(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        _check_labels(generator, discriminator, labels)
        rna, u = self._inputs(generator, real_inputs, device)
        nxt = None
        if TRAINER_LOOKAHEAD[0] and _lookahead_ok():       # the penalty plugin's draw, made now (same generator order)
            nxt = _NEXT_NOISE[0] = self._inputs(generator, real_inputs, device)[1]
        real = real_inputs["image"].to(device)
        return self.step(generator, discriminator, optimizer_discriminator, real, rna, u, nxt)

    def train_ops(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_discriminator, real_inputs, device, labels).item()
    train_ops._rg_async = "train_ops_async"


class WassersteinGradientPenaltyVAE(DiscriminatorLoss, _VAEMixin):
    def __init__(self, checkpoint, rna_features, reduction="mean", lambd=10.0, override_train_ops=None, beta=0.005):
        super().__init__(checkpoint, rna_features)
        self.lambd = lambd
        self.override_train_ops = override_train_ops
        self._init_vae(checkpoint, rna_features, beta)

    def forward(self, interpolate, d_interpolate):
        """src/wgan_loss.py:293-312 (``self.reduction`` holds the checkpoint path there and is ignored by the
        functional form, :44)."""
        return wasserstein_gradient_penalty_vae(interpolate, d_interpolate, self.reduction)

    def step(self, generator, discriminator, optimizer_discriminator, real, rna, u, eps):
        return gp_train_op(self._runner, generator, discriminator, optimizer_discriminator, self.lambd, real,
                           lambda: [self._latent(rna), u], u, eps, lambda z, uu: self._noise(generator, z, uu))

    def train_ops_async(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        _check_labels(generator, discriminator, labels)
        ahead, _NEXT_NOISE[0] = _NEXT_NOISE[0], None       # u drawn ahead by the D-loss plugin (Trainer flow), else now
        if ahead is not None and ahead.shape == (real_inputs["image"].size(0), generator.encoding_dims):
            rna, u = real_inputs["rna_data"], ahead
        else:
            rna, u = self._inputs(generator, real_inputs, device)
        real = real_inputs["image"].to(device)
        eps = _pinned(1).uniform_(0.0, 1.0).to(device, non_blocking=True)   # torch.rand(1) in the reference (:376)
        return self.step(generator, discriminator, optimizer_discriminator, real, rna, u, eps)

    def train_ops(self, generator, discriminator, optimizer_discriminator, real_inputs, device, labels=None):
        return self.train_ops_async(generator, discriminator, optimizer_discriminator, real_inputs, device, labels).item()
    train_ops._rg_async = "train_ops_async"
