"""Exponential moving average of a module's parameters (the averaged generator of ProGAN / StyleGAN / BigGAN), kept by ONE HIP
launch inside ``optim.Adam.step()``.

    ema = ParamEMA(generator, decay=0.999, warmup=True)
    optimizer_generator.attach_ema(ema)
    ...train...
    images = gan_utils.synthesize(ema.module, noise)

``ema.module`` is a second module of the same class ("the twin"): own storage, eval mode, no gradients.  Its flat parameter
buffer IS the average: rg_ema_update reads the live module's flat buffer right behind the Adam launches of the same step, on
the same stream, with the same device-side step counter (the warm-up) and skip word (a step dynamic loss scaling skipped moves
neither the weights nor the average).  Being a launch of ``step()`` it is part of every captured step graph, of the deferred
data-parallel tail and of every fused-step form.  No 16-bit shadow of the average is written: the twin is read once per epoch
or at synthesis, and its operand images are rebuilt from the fp32 master on demand (``packs_stale() == 2``).

BatchNorm running statistics are running averages already: they are COPIED from the live module on demand
(``sync_buffers()``), not averaged (StyleGAN's rule).
"""
from __future__ import annotations

import copy

import torch

from . import dist as D_
from . import _abi

_RUNTIME_FIELDS = ("_rt_ops", "_rt_net", "_rt_flat", "_amp_scaler")


def _twin_of(module):
    """A copy of ``module`` with its own storage and no runtime: same class, same state_dict keys and shapes."""
    D_.flush()                                     # a data-parallel train_op may have left the module's step in flight
    memo = {}
    for name in _RUNTIME_FIELDS:                   # backend handles, engine views and flat buffers are rebuilt, never copied
        val = module.__dict__.get(name)
        if val is not None:
            memo[id(val)] = None
    twin = copy.deepcopy(module, memo)
    for name in _RUNTIME_FIELDS[:3]:
        setattr(twin, name, None)
    twin.__dict__.pop("_amp_scaler", None)
    twin.eval()
    twin.requires_grad_(False)
    return twin


class ParamEMA:
    def __init__(self, module, decay=0.999, warmup=True):
        if not hasattr(module, "runtime"):
            raise TypeError("ParamEMA averages a rna_gan_amd HIP module (its flat parameter buffer)")
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError("ParamEMA: decay must be in [0, 1), got %r" % (decay,))
        self.source = module
        self._decay = decay
        self._warmup = bool(warmup)
        self._optimizer = None
        self._gens = None                          # (live flat generation, twin flat generation) the launch was resolved for
        self.module = _twin_of(module)

    # decay / warmup are kernel arguments frozen in captured graphs: fixed while attached
    @property
    def decay(self):
        return self._decay

    @decay.setter
    def decay(self, value):
        self._set("_decay", float(value))

    @property
    def warmup(self):
        return self._warmup

    @warmup.setter
    def warmup(self, value):
        self._set("_warmup", bool(value))

    def _set(self, name, value):
        if self._optimizer is not None:
            raise RuntimeError("ParamEMA: decay / warmup are fixed while attached to an optimizer (detach_ema() first)")
        if name == "_decay" and not 0.0 <= value < 1.0:
            raise ValueError("ParamEMA: decay must be in [0, 1), got %r" % (value,))
        setattr(self, name, value)

    # ------------------------------------------------------------------ the launch (driven by optim.Adam)
    def _resolve(self):
        """Home the twin and check that both flat buffers have the same fp32 layout; remember their generations."""
        fs = self.source.flat
        twin = self.module
        if next(twin.parameters()).device != fs.data.device:
            raise RuntimeError("ParamEMA: the averaged module is on %s, the live module on %s: move both"
                               % (next(twin.parameters()).device, fs.data.device))
        if twin.training:
            twin.eval()
        ft = twin.flat
        if fs.data.dtype != torch.float32 or ft.data.dtype != torch.float32:
            raise TypeError("ParamEMA: rg_ema_update averages fp32 flat buffers (got %s / %s)" % (fs.data.dtype, ft.data.dtype))
        if fs.offsets != ft.offsets or fs.numel != ft.numel:
            raise RuntimeError("ParamEMA: the live and the averaged module lay their parameters out differently")
        self._gens = (fs.gen, ft.gen)

    def _attach(self, optimizer):
        if self._optimizer is not None and self._optimizer is not optimizer:
            raise RuntimeError("ParamEMA: already attached to another optimizer")
        self._optimizer = optimizer
        self._resolve()

    def _detach(self):
        self._optimizer = None
        self._gens = None

    def _rehomed(self) -> bool:
        """True when either module was re-homed since the launch was resolved (then resolved again): the caller bumps its
        buffer generation, so that no captured graph goes on writing to a buffer that was given back."""
        if self._gens == (self.source.flat.gen, self.module.flat.gen):
            return False
        self._resolve()
        return True

    def _launch(self, half, hyper, step_dev):
        fs, ft = self.source._rt_flat, self.module._rt_flat
        if self._gens != (fs.gen, ft.gen):
            raise RuntimeError("ParamEMA: a module was re-homed between the optimizer's buffer check and its step")
        _abi.launch("rg_ema_update", fs.data.device, fs.data.data_ptr(), ft.data.data_ptr(), fs.numel, self._decay,
                    step_dev.data_ptr() if self._warmup else None, hyper.data_ptr(), half=half)
        self.module.weights_changed()              # plain version bump: no shadow was written

    # ------------------------------------------------------------------ on demand
    @torch.no_grad()
    def sync_buffers(self):
        """Copy the live module's buffers (BatchNorm running statistics, num_batches_tracked) into the twin."""
        D_.flush()
        live = dict(self.source.named_buffers())
        for name, b in self.module.named_buffers():
            b.copy_(live[name])
        return self

    @torch.no_grad()
    def reset(self):
        """Re-initialise the average from the live module (parameters and buffers), in place."""
        D_.flush()
        live = dict(self.source.named_parameters())
        for name, p in self.module.named_parameters():
            p.copy_(live[name])
        self.module.weights_changed()
        return self.sync_buffers()

    def state_dict(self):
        self.sync_buffers()
        return self.module.state_dict()

    def load_state_dict(self, state_dict, strict=True):
        return self.module.load_state_dict(state_dict, strict=strict)
