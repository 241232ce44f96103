"""Dynamic loss scaling for the fp16 build: torch.cuda.amp.GradScaler's rule, kept on the device (rna_gan_amd/csrc/rg_amp.hip).

Opt-in (``Trainer(loss_scaling="dynamic")``, ``histopathology_gan.py --loss_scaling dynamic`` or
``RNAGAN_F16_LOSS_SCALE=dynamic``); without it nothing changes: the static scale of ops_hip.HipOps and the same launches.

Per train_op (one seeded backward + its optimizer step), counted like GradScaler:
  * the backward seeds read S = 2^k from the device: the exponent is LATCHED per stepped network at the train_op's first seed
    (rg_amp_latch), and the seeds and that network's Adam unscale read the latch -- in a data-parallel "prefix" train_op the
    other network's pending step (and its scale update) runs between the prefix and the rest, and S must not change inside one
    train_op (a backoff then takes effect one train_op late);
  * the optimizer step probes every gradient value its Adam launches read, and -- in a single process -- the loss
    (rg_nonfinite_probe; data parallel: the loss is rank-local, the reduced / gathered gradients decide alone); a non-finite
    value makes the step a no-op (parameters, moments, shadows, the step counter), S <- max(S / 2, min_scale), the growth
    tracker is reset and the skipped counter goes up; otherwise the tracker goes up and after growth_interval clean steps
    S <- min(2 S, max_scale).
No host synchronisation: only get_scale() / skipped_steps() / state_dict() read the device.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from ._abi import check, CONSTANTS, RG_F32

# include/rnagan_hip.h RG_AMP_*
STATE_INTS, EXP, TRACKER, SKIPPED, LATCH, FLAG, SLOTS = (
    CONSTANTS["RG_AMP_" + k] for k in ("STATE_INTS", "EXP", "TRACKER", "SKIPPED", "LATCH", "FLAG", "SLOTS"))
PROBE_MAX_SEGS = 32


def _exp2(v, what):
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError("DynamicLossScaler: %s must be a positive power of two, got %r" % (what, v))
    m, e = math.frexp(v)
    if m != 0.5:
        raise ValueError("DynamicLossScaler: %s must be a power of two (exact unscaling), got %r" % (what, v))
    return e - 1


class DynamicLossScaler:
    # 2^24: the fp16 seeds stay far below 65504 for any head pre-activation mask (|coef| <= S / batch), and a scale that large
    # already moves gradients of 2^-24 (the smallest fp16 subnormal) to 1; growing further can only create overflow
    def __init__(self, init_scale=4096.0, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24, growth_factor=2.0,
                 backoff_factor=0.5):
        if float(growth_factor) != 2.0 or float(backoff_factor) != 0.5:
            raise ValueError("DynamicLossScaler: growth_factor must be 2 and backoff_factor 0.5 (powers of two keep the "
                             "unscaling exact)")
        if int(growth_interval) != growth_interval or int(growth_interval) < 1:
            raise ValueError("DynamicLossScaler: growth_interval must be a positive integer")
        self.growth_interval = int(growth_interval)
        self.min_exp = _exp2(min_scale, "min_scale")
        self.max_exp = _exp2(max_scale, "max_scale")
        k0 = _exp2(init_scale, "init_scale")
        if not (-126 < self.min_exp <= self.max_exp < 127 and -126 < k0 < 127):
            raise ValueError("DynamicLossScaler: need min_scale <= max_scale, all inside fp32's normal range")
        # the state lives on the host until the scaler is attached to modules on a device (rnagan_hip.h RG_AMP_*); as with
        # GradScaler, the caps bound growth and backoff, not the initial scale
        self._state = torch.zeros(STATE_INTS, dtype=torch.int32)
        self._state[EXP] = k0
        self._slots = {}                 # id(stepped module) -> slot

    # ---------------------------------------------------------------- wiring
    def attach(self, *modules):
        """Scale the backward passes of these modules (G and D share ONE scaler: the seeds of every train_op are issued through
        the generator's HipOps).  Each module's backend must be rna_gan_amd.ops_hip.HipOps."""
        for m in modules:
            ops, _ = m.runtime()
            if not hasattr(ops, "amp"):
                raise TypeError("DynamicLossScaler.attach: %r has no HIP backend" % (m,))
            self.attach_ops(ops)
            m._amp_scaler = self
            self.slot_of(m)
        return self

    def attach_ops(self, ops):
        self._home(ops.device)
        # the static fp16 scale is replaced: seeds and unscale both read the device scale from now on
        ops.loss_scale, ops.gp_seed_scale, ops.gp_tangent_scale = 1.0, 1.0, 1.0
        ops.amp = self

    def _home(self, device):
        if self._state.device != torch.device(device):
            if self._state.is_cuda:
                raise RuntimeError("DynamicLossScaler: one scaler serves the modules of ONE device")
            self._state = self._state.to(device)

    def slot_of(self, module):
        s = self._slots.get(id(module))
        if s is None:
            if len(self._slots) >= SLOTS:
                raise RuntimeError("DynamicLossScaler: at most %d stepped networks per scaler" % SLOTS)
            s = self._slots[id(module)] = len(self._slots)
        return s

    @property
    def state(self):
        return self._state

    # ---------------------------------------------------------------- device steps (enqueued on `stream`)
    def latch(self, ops, module):
        """Before the first backward seed of a train_op that steps `module`: its seeds and its Adam unscale read S as of now."""
        slot = self.slot_of(module)
        check(ops.lib.rg_amp_latch(self._state.data_ptr(), slot, ops.stream), "rg_amp_latch")
        ops.amp_slot = slot

    def probe(self, lib, module, segs, stream):
        """segs: [(address, elements, dtype code)] -- OR "non-finite" into the flag of `module`'s slot."""
        segs = [s for s in segs if s[1] > 0]
        flag = self._state.data_ptr() + 4 * (FLAG + self.slot_of(module))
        for i in range(0, len(segs), PROBE_MAX_SEGS):
            part = segs[i:i + PROBE_MAX_SEGS]
            k = len(part)
            ptrs = (C.c_void_p * k)(*[p for p, _, _ in part])
            ns = (C.c_ulonglong * k)(*[n for _, n, _ in part])
            dts = (C.c_int * k)(*[d for _, _, d in part])
            check(lib.rg_nonfinite_probe(k, C.addressof(ptrs), C.addressof(ns), C.addressof(dts), flag, stream),
                  "rg_nonfinite_probe")

    def probe_loss(self, ops, module, loss):
        if torch.is_tensor(loss) and loss.is_cuda and loss.dtype == torch.float32:
            self.probe(ops.lib, module, [(loss.data_ptr(), loss.numel(), RG_F32)], ops.stream)

    def hyper(self, lib, module, step_dev, group, hyper, stream):
        check(lib.rg_adam_hyper_dev3(step_dev.data_ptr(), float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]),
                                     float(group["eps"]), float(group.get("weight_decay", 0.0)), self._state.data_ptr(),
                                     self.slot_of(module), hyper.data_ptr(), stream), "rg_adam_hyper_dev3")

    def update(self, lib, module, stream):
        check(lib.rg_amp_update(self._state.data_ptr(), self.slot_of(module), self.growth_interval, self.min_exp, self.max_exp,
                                stream), "rg_amp_update")

    # ---------------------------------------------------------------- host view (synchronises)
    def _read(self):
        from . import dist as D_
        D_.flush()                       # a data-parallel train_op may have left its optimizer step (and update) in flight
        return [int(v) for v in self._state.cpu().tolist()]

    def get_scale(self) -> float:
        return 2.0 ** self._read()[EXP]

    def skipped_steps(self) -> int:
        return self._read()[SKIPPED]

    def state_dict(self):
        st = self._read()
        return {"scale": 2.0 ** st[EXP], "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": self.growth_interval,
                "_growth_tracker": st[TRACKER], "skipped_steps": st[SKIPPED]}

    def load_state_dict(self, sd):
        if float(sd.get("growth_factor", 2.0)) != 2.0 or float(sd.get("backoff_factor", 0.5)) != 0.5:
            raise ValueError("DynamicLossScaler.load_state_dict: growth_factor 2 / backoff_factor 0.5 only")
        k = _exp2(sd["scale"], "scale")
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        from . import dist as D_
        D_.flush()
        vals = self._state.cpu()
        vals[EXP] = k
        vals[TRACKER] = int(sd.get("_growth_tracker", 0))
        vals[SKIPPED] = int(sd.get("skipped_steps", 0))
        self._state.copy_(vals)          # in place: captured graphs hold the buffer's address

    # ---------------------------------------------------------------- the rule, on the host (documentation and tests)
    @staticmethod
    def update_rule(exp, tracker, skipped, found_nonfinite, growth_interval, min_exp, max_exp):
        """(exp, tracker, skipped) after one train_op: what rg_amp_update does on the device."""
        if found_nonfinite:
            return max(exp - 1, min_exp), 0, skipped + 1
        if tracker + 1 >= growth_interval:
            return min(exp + 1, max_exp), 0, skipped
        return exp, tracker + 1, skipped


_DEFAULT = {}


def default_scaler(device):
    """The process's scaler for RNAGAN_F16_LOSS_SCALE=dynamic: one per device, shared by every fp16 HipOps on it."""
    key = str(torch.device(device))
    sc = _DEFAULT.get(key)
    if sc is None:
        sc = _DEFAULT[key] = DynamicLossScaler()
        sc._home(device)
    return sc
