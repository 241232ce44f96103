"""The train_op scheduler: how one train_op of a loss plugin (rna_gan_amd.losses) runs.  A train_op is a _Body (prefix / rest over
the engine's gradient passes), armed to leave weight gradients to the optimizer step that consumes them (_armed) and dispatched
(_dispatch) as one captured graph (_Runner.run) or, data parallel, along _Runner.run_dp / flush.  The module-level switches are
read as globals at call time: set them here (train_op.NAME), never on a copy imported elsewhere."""
import contextlib
import os

import torch

from . import dist as D_
from . import engine as E
from . import graphed


def _nets(generator, discriminator):
    og, gn = generator.runtime()
    od, dn = discriminator.runtime()
    if og.act_dtype != od.act_dtype:
        raise RuntimeError("generator and discriminator must use the same precision")
    if og.amp is not od.amp:
        # every seed is issued through the generator's backend and every optimizer unscales with its own network's: a scaler on
        # one of them only would leave the other network's gradients off by the scale
        raise RuntimeError("dynamic loss scaling: attach ONE DynamicLossScaler to both the generator and the discriminator "
                           "(DynamicLossScaler.attach(G, D))")
    return og, gn, dn


def _is_half(ops):
    """The backend runs the 16-bit-storage MFMA kernels (bf16 build, or the fp16 build of the same sources)."""
    return ops.act_dtype in (torch.bfloat16, torch.float16)


def _wire_kind(ops):
    """compress argument of the data-parallel all-reduce: the gradients travel in the build's 16-bit type, or as fp32."""
    if not _is_half(ops) or (ops.half == "f16" and not D_.F16_WIRE):
        return False
    return ops.half


def _local_half_dcgan(ops, net):
    """16-bit kernels on a DCGAN GenNet / DiscNet whose BatchNorm statistics are rank-local: what every deferred weight-gradient
    form below needs."""
    return _is_half(ops) and isinstance(net, (E.GenNet, E.DiscNet)) and ops.stat_reduce is None


def _is_adam(optimizer):
    """rna_gan_amd.optim.Adam (the only optimizer with note_replayed / grad_wire), without importing it here."""
    return hasattr(optimizer, "note_replayed")


def _own_adam(stepped, optimizer):
    """The optimizer is rna_gan_amd.optim.Adam bound to the stepped module (Adam.bind): it consumes what a gradient pass defers."""
    return _is_adam(optimizer) and optimizer._module is stepped


def _grad_scale(ops):
    """Seed scale of the D / G loss: the data-parallel mean over ranks times the (static) fp16 loss scale."""
    return D_.grad_scale() * ops.loss_scale


def _f32(x):
    """A step input as the kernels take it."""
    return x.contiguous().float()


def _finish(module, optimizer):
    """all-reduce (data parallel) -> optimizer step -> invalidate packed weights."""
    _reduce(module)
    _apply(module, optimizer)


def _reduce(module):
    ops, _ = module.runtime()
    D_.allreduce_sum_(module.flat.grad, compress=_wire_kind(ops))


def _apply(module, optimizer):
    ops, _ = module.runtime()
    if (ops.loss_scale != 1.0 or ops.amp is not None) and not _own_adam(module, optimizer):
        # fp16: the gradients in module.flat.grad carry the loss scale; only rna_gan_amd.optim.Adam bound to the module unscales
        raise RuntimeError("fp16 precision needs rna_gan_amd.optim.Adam(...).bind(module): a foreign optimizer would step on "
                           "loss-scaled gradients")
    optimizer.step()
    if not _is_adam(optimizer):      # rna_gan_amd.optim.Adam reports the change itself
        module.weights_changed()
    return module.flat.data[:1]          # a tensor result, so that this half can be a graph of its own


# Dynamic loss scaling (rna_gan_amd.amp): the scale is latched for the STEPPED network right before the first backward seed of its
# train_op -- in the rest, except for a data-parallel D-loss prefix that seeds D(real) -- and the loss is probed for non-finite
# values once the rest has produced it.  In the data-parallel "prefix" route a network's pending optimizer step (which reads
# its latch) is always applied before that network's next train_op seeds: the D step's pending update runs in the flush between
# the penalty step's prefix (which reads G and seeds nothing) and its rest, G's between the D-loss prefix and rest.
def _amp_latch(ops, stepped):
    if ops.amp is not None:
        ops.amp.latch(ops, stepped)


def _amp_loss(ops, stepped, loss):
    # (data parallel: the loss is rank-local, so only the all-reduced gradients decide -- every rank decides alike)
    if ops.amp is not None and not D_.active():
        ops.amp.probe_loss(ops, stepped, loss[0] if isinstance(loss, tuple) else loss)
    return loss


# Every train_op body is  rest(prefix(...))  where the PREFIX reads only ONE of the two networks (engine.*_prefix):
#   G step : prefix = conditioned noise + G(z)            (reads G)   rest = D(G(z)), backward through D and G
#   D step : prefix = (clip) + D(real) [+ noise]          (reads D)   rest = G(z), D(fake), backward through D
#   GP step: prefix = noise + G(z) + interpolation        (reads G)   rest = penalty forward / double backward in D
# In a data-parallel run the previous train_op's all-reduce and optimizer step of the OTHER network stay in flight
# while the prefix runs (run_dp below).
def _g_prefix(generator, discriminator, noise):
    ops, gn, _ = _nets(generator, discriminator)
    return E.gen_loss_prefix(ops, gn, _f32(noise))


def _g_rest(generator, discriminator, pre):
    ops, gn, dn = _nets(generator, discriminator)
    _amp_latch(ops, generator)
    return _amp_loss(ops, generator, E.gen_loss_rest(ops, gn, dn, pre, grad_scale=_grad_scale(ops)))


# data-parallel D-loss step: D(real)'s backward belongs to the prefix too (it reads the discriminator only), so the generator's
# gradient all-reduce -- started by the G-loss step just before -- is covered by a forward and a backward pass
# (RNAGAN_DP_PREFIX_BWD=0: forward only, as in round 2)
# RNAGAN_DP_PREFIX_BWD=2 (default since round 4): forward + data-gradient chain in the prefix, the conv weight gradients of
# both halves as two-segment launches in the rest -- engine.disc_loss_prefix(backward="dgrad").  One rank, same box,
# interleaved: 12.07 ms against 12.21 ms for mode 1 (single-process path 11.24-11.39); the prefix shrinks from ~1.3 to ~0.9 ms, still longer than the
# generator's 90 MB collective at any plausible bus bandwidth.  1: the whole backward of the real half in the prefix (round 3).
# PROVISIONAL default: the only evidence is a one-rank timing and a world-2 run over gloo on a shared GPU; mode 2's shorter
# prefix gives the generator's collective less cover, and tools/dp_first_run.sh A/Bs mode 1 on the first real multi-GPU node.
def _env_int(name, dflt, allowed):
    try:
        v = int(os.environ.get(name, "") or dflt)
    except ValueError:
        v = dflt
    return v if v in allowed else dflt


DP_PREFIX_MODE = _env_int("RNAGAN_DP_PREFIX_BWD", 2, (0, 1, 2))
DP_PREFIX_BWD = DP_PREFIX_MODE != 0
# Data-parallel ROUTE of a train_op.  "prefix" (default): graph(prefix) / graph(rest) / all-reduce started and left in flight
# under the next train_op's prefix, which reads the other network (_Runner.run_dp) -- it HIDES the collectives, and gives up what a
# single process gains from running a train_op as one body: D(real) + D(fake) as one double batch, the penalty step's fake batch
# out of the D-loss step's generator pass, graph boundaries (+0.6 ms of 10.4 at one rank, DESIGN).  "whole": the single
# process's body as ONE graph (gradients onto the wire), then the all-reduce, waited for at once, then the optimizer step --
# nothing is hidden and none of that is lost.  Which of the two is faster depends on the collectives' real duration: the first
# run on a multi-GPU node A/Bs them (tools/dp_first_run.sh).
DP_ROUTE = os.environ.get("RNAGAN_DP_ROUTE", "prefix")
if DP_ROUTE not in ("prefix", "whole"):
    DP_ROUTE = "prefix"


def _single_body():
    """This train_op runs as the single-process body (_Body.whole, if it has one): no data-parallel run, or its route "whole"."""
    return not D_.active() or DP_ROUTE == "whole"


def _clip(ops, discriminator, clip):
    if clip is not None:
        ops.clamp_(discriminator.flat.data, clip[0], clip[1])      # every D parameter (wgan_loss.py:213-215)
        discriminator.weights_changed()


def _d_prefix(generator, discriminator, real, noise, clip):
    ops, _, dn = _nets(generator, discriminator)
    _clip(ops, discriminator, clip)
    backward = None
    if D_.active():
        backward = "dgrad" if DP_PREFIX_MODE == 2 else "all" if DP_PREFIX_BWD else None
    if backward is not None:
        _amp_latch(ops, discriminator)           # D(real)'s backward is seeded here
    return E.disc_loss_prefix(ops, dn, _f32(real), backward, grad_scale=_grad_scale(ops)), _f32(noise)


def _d_batched(generator, discriminator, real, noise, clip, next_noise=None):
    """single process: D(real) and D(fake) as one double batch through the conv layers (engine.disc_loss_grads_batched);
    next_noise: the noise of the penalty step that follows -- its fake batch comes out of the same generator pass"""
    ops, gn, dn = _nets(generator, discriminator)
    _clip(ops, discriminator, clip)
    _amp_latch(ops, discriminator)
    return _amp_loss(ops, discriminator, E.disc_loss_grads_batched(
        ops, gn, dn, _f32(real), _f32(noise), grad_scale=_grad_scale(ops), next_noise=None if next_noise is None else _f32(next_noise)))


class _FakeCache:
    """G(noise) of the penalty step, produced ahead by the D-loss step of the same iteration (both need a fake batch from the
    same generator weights, src/wgan_loss.py:247 and :371; one generator pass over the double batch instead of two).  The
    entry is used only by a penalty step that is handed the very noise tensor it was produced for, with the generator
    unchanged in between."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.key, self.src, self.img = None, None, None

    @staticmethod
    def make_key(generator, noise_tensors):
        _, gn = generator.runtime()
        return (id(generator), gn.g0.version) + tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in noise_tensors)

    def put(self, generator, noise_tensors, img):
        self.key, self.src, self.img = self.make_key(generator, noise_tensors), list(noise_tensors), img

    def take(self, generator, noise_tensors):
        if self.key is None or self.key != self.make_key(generator, noise_tensors):
            return None
        img = self.img
        self.clear()
        return img


_FAKE = _FakeCache()


# (data parallel, route "whole": the generator's pending update is applied before the D-loss step starts, so its weights are
# the same in the D-loss and the penalty step, as in a single process)
_lookahead_ok = _single_body


def _d_step_lookahead(runner, key, generator, discriminator, optimizer, clip, inputs, noise_fn, next_tensors):
    """D-loss step whose generator pass also produces the fake batch of the penalty step that follows (kept in _FAKE)."""
    body = _d_body(generator, discriminator, clip, noise_fn, lookahead=True)
    loss, fake_next = _dispatch(runner, key + ("lookahead",), body, inputs, generator, discriminator, discriminator, optimizer)
    _FAKE.put(generator, next_tensors, fake_next)
    return loss


def _gp_fake_body(generator, discriminator, lambd):
    """penalty step on a fake batch that is already there: inputs (real, fake, eps)"""
    def prefix(real, fake, eps):
        ops, _, _ = _nets(generator, discriminator)
        return E.gp_loss_prefix_fake(ops, _f32(real), fake, eps if torch.is_tensor(eps) else float(eps))
    return _Body(prefix, lambda xhat: _gp_rest(generator, discriminator, xhat, lambd), generator)


def _d_rest(generator, discriminator, pre):
    ops, gn, dn = _nets(generator, discriminator)
    d_real, noise = pre
    if d_real.backward is None:                  # (else the prefix seeded D(real)'s backward: latched there)
        _amp_latch(ops, discriminator)
    return _amp_loss(ops, discriminator, E.disc_loss_rest(ops, gn, dn, d_real, noise, grad_scale=_grad_scale(ops)))


def _gp_prefix(generator, discriminator, real, noise, eps):
    ops, gn, _ = _nets(generator, discriminator)
    return E.gp_loss_prefix(ops, gn, _f32(real), _f32(noise), eps if torch.is_tensor(eps) else float(eps))


def _gp_rest(generator, discriminator, xhat, lambd):
    ops, _, dn = _nets(generator, discriminator)
    _amp_latch(ops, discriminator)
    return _amp_loss(ops, discriminator, E.gp_loss_rest(ops, dn, xhat, float(lambd), grad_scale=D_.gp_grad_scale()))


def _g_step(generator, discriminator, optimizer_generator, noise):
    """Eager G train_op body (gradients + all-reduce + optimizer step)."""
    loss = _g_body(generator, discriminator).grads(noise)
    _finish(generator, optimizer_generator)
    return loss


def _d_step(generator, discriminator, optimizer_discriminator, real, noise, clip):
    loss = _d_body(generator, discriminator, clip).grads(real, noise)
    _finish(discriminator, optimizer_discriminator)
    return loss


def _gp_step(generator, discriminator, optimizer_discriminator, real, noise, eps, lambd):
    """eps: python float or 1-element device tensor."""
    loss = _gp_body(generator, discriminator, lambd).grads(real, noise, eps)
    _finish(discriminator, optimizer_discriminator)
    return loss


class _Body:
    """One train_op: prefix(*inputs) -> pre ; rest(pre) -> loss ; which network the prefix reads.  whole (optional): the
    single-process form of the same train_op when it is not simply rest(prefix(...))."""

    def __init__(self, prefix, rest, prefix_reads, whole=None):
        self.prefix, self.rest, self.prefix_reads, self.whole = prefix, rest, prefix_reads, whole

    def grads(self, *inputs):
        if self.whole is not None and _single_body():
            return self.whole(*inputs)
        return self.rest(self.prefix(*inputs))


def _g_body(generator, discriminator, noise_fn=None):
    nf = noise_fn or (lambda nz: nz)
    return _Body(lambda *a: _g_prefix(generator, discriminator, nf(*a)),
                 lambda pre: _g_rest(generator, discriminator, pre), generator)


def _d_body(generator, discriminator, clip, noise_fn=None, lookahead=False):
    """whole: D(real) + D(fake) as one double batch; the two chains of prefix / rest: what the data-parallel "prefix" route runs"""
    nf = noise_fn or (lambda nz: nz)
    if lookahead:
        # inputs (real, *conditioning, noise, next_noise): the penalty step's fake batch comes out of this step's generator pass
        return _Body(None, None, discriminator,
                     lambda real, *a: _d_batched(generator, discriminator, real, nf(*a[:-1]), clip, nf(*a[:-2], a[-1])))
    return _Body(lambda real, *a: _d_prefix(generator, discriminator, real, nf(*a), clip),
                 lambda pre: _d_rest(generator, discriminator, pre), discriminator,
                 lambda real, *a: _d_batched(generator, discriminator, real, nf(*a), clip))


def _gp_body(generator, discriminator, lambd, noise_fn=None):
    nf = noise_fn or (lambda nz: nz)
    return _Body(lambda real, *a: _gp_prefix(generator, discriminator, real, nf(*a[:-1]), a[-1]),
                 lambda xhat: _gp_rest(generator, discriminator, xhat, lambd), generator)


def _dispatch(runner, key, body, inputs, generator, discriminator, stepped, optimizer):
    """single process: one graph per train_op (gradients + optimizer step); data parallel: see _Runner.run_dp"""
    mods = [generator, discriminator]
    if D_.active():
        return runner.run_dp(key, body, inputs, mods, stepped, optimizer)

    def full(*a):
        sk = _skinny_slab_layer(stepped, optimizer)
        # this gradient pass is followed at once by optimizer.step() (_finish), which consumes what it leaves pending: the split-K
        # weight gradients of the 4 x 4 layers as unreduced slabs, the image-side layer's per-workgroup partials (registered on
        # the HipOps the engine runs BOTH networks on, _nets), G.0's operands
        with _armed(slabs=_slab_layers(stepped, optimizer), skinny=None if sk is None else (generator.runtime()[0], sk),
                    g0=_fusable_g0(stepped, optimizer)):
            loss = body.grads(*a)
        _finish(stepped, optimizer)
        return loss
    return runner.run(key, full, inputs, mods, [optimizer])


def d_train_op(runner, G, D, opt, clip, real, cond_inputs, noise_fn=None, next_draw=None):
    """The D-loss train_op of a plugin.  cond_inputs: what the noise is made of -- [noise], or [latent, u] under noise_fn;
    next_draw: the draw (noise / u) of this iteration's penalty step: its fake batch then comes out of this step's generator pass."""
    if next_draw is not None and _lookahead_ok():
        return _d_step_lookahead(runner, ("d", clip), G, D, opt, clip, [real, *cond_inputs, next_draw], noise_fn, (next_draw,))
    return _dispatch(runner, ("d", clip), _d_body(G, D, clip, noise_fn), [real, *cond_inputs], G, D, D, opt)


def gp_train_op(runner, G, D, opt, lambd, real, cond_inputs, draw, eps, noise_fn=None):
    """The penalty train_op of a plugin.  draw: the noise / u tensor of this step; cond_inputs(): what the noise is made of,
    [noise] or [latent, u] -- called only when this step makes its own fake batch; eps: 1-element device tensor."""
    fake = _FAKE.take(G, (draw,)) if _single_body() else None
    if fake is not None:                  # G(noise) came out of the D-loss step's generator pass
        return _dispatch(runner, ("gpf", lambd), _gp_fake_body(G, D, lambd), [real, fake, eps], G, D, D, opt)
    return _dispatch(runner, ("gp", lambd), _gp_body(G, D, lambd, noise_fn), [real, *cond_inputs(), eps], G, D, D, opt)


@contextlib.contextmanager
def _armed(slabs=(), wired=(), skinny=None, g0=None, factor_stage=None):
    """Arm ONE gradient pass to leave weight gradients unreduced for whoever consumes them right after it, and disarm it again.
      slabs         ConvW handles whose split-K slabs may stay unreduced (ConvW.defer_slabs);
      wired         data parallel: (ConvW, wire slice) pairs -- defer_slabs plus ConvW.wire_slot;
      skinny        (HipOps, ConvW): the image-side layer whose per-workgroup partials may stay (HipOps._skinny_defer);
      g0            generator layer 0's handle: its operands stay on the handle (ConvW.fuse_step), or are copied into this rank's
                    factor_stage = (z slot, gz0 slot) of the gathered factor buffers (ConvW.factor_stage).
    On entry nothing may be pending on these layers from an earlier pass that raised before its consumer ran (a stale
    pending_wgrad would also keep that pass's operand activations alive): dropped.  On exit every flag set here is cleared --
    a stale one is silent: a later eager pass would leave a gradient unreduced and the optimizer would step without it.  When the
    body raises, what it left pending is dropped too: no consumer will run, the next train_op starts clean.
    What is pending after a NORMAL exit is the caller's to consume, and the callers differ: a single process hands it to
    optimizer.step() (_dispatch: _finish right after the with); a data-parallel pass turns pending_slabs into the all-reduce's
    segment table and checks / clears g0.pending_wgrad == "staged" before it leaves the with (_dp_armed)."""
    layers = list(slabs) + [cw for cw, _ in wired] + [c for c in (skinny and skinny[1], g0) if c is not None]

    def drop():
        for cw in layers:
            cw.pending_slabs = cw.pending_bias = cw.pending_wgrad = None
    drop()
    for cw in slabs:
        cw.defer_slabs = True
    for cw, slot in wired:
        cw.defer_slabs, cw.wire_slot = True, slot
    if skinny is not None:
        skinny[0]._skinny_defer = {skinny[1].dw.data_ptr(): skinny[1]}
    if g0 is not None:
        g0.fuse_step, g0.factor_stage = True, factor_stage
    try:
        yield
    except BaseException:
        drop()
        raise
    finally:
        for cw in layers:
            cw.defer_slabs, cw.wire_slot, cw.fuse_step, cw.factor_stage = False, None, False, None
        if skinny is not None:
            skinny[0]._skinny_defer = None


# split-K weight-gradient slabs summed inside the optimizer step instead of by a reduction launch per layer (single process,
# bf16 kernels, rna_gan_amd.optim.Adam bound to the stepped module): ConvW.defer_slabs / ops_hip._wgrad_slabs / rg_adam_step_slabs
SLAB_ADAM = os.environ.get("RNAGAN_SLAB_ADAM", "1") != "0"


def _slab_layers(stepped, optimizer):
    if not SLAB_ADAM or D_.active() or not _own_adam(stepped, optimizer):
        return []
    ops, net = stepped.runtime()
    return [b[0] for b in net.blocks] if _local_half_dcgan(ops, net) else []


SKINNY_SLAB_ADAM = os.environ.get("RNAGAN_SKINNY_SLAB_ADAM", "1") != "0"


def _skinny_slab_layer(stepped, optimizer):
    """The stepped network's image-side 4 x 4 layer (D's first conv / G's last transposed conv: 64 <-> 3 channels, PyTorch-layout
    weight) when its weight gradient's per-workgroup partials may stay unreduced for the optimizer step (conditions of
    _slab_layers; the tensor must sit 16-byte aligned in the flat buffer)."""
    if not SKINNY_SLAB_ADAM or not _slab_layers(stepped, optimizer):
        return None
    _, net = stepped.runtime()
    cw = net.conv0 if isinstance(net, E.DiscNet) else net.last
    flat = stepped.flat
    off = (cw.w.data_ptr() - flat.data.data_ptr()) // 4
    if cw.dw is None or not cw.w.is_contiguous() or off % 4 or cw.w.numel() % 4 or cw.w.shape[0] != 64:
        return None
    if cw.bias is not None and ((cw.bias.data_ptr() - flat.data.data_ptr()) // 4) % 4:
        return None                     # (its bias-gradient partials become a segment of the same step: 16-byte aligned too)
    return cw


G0_ADAM = os.environ.get("RNAGAN_G0_ADAM", "1") != "0"


def _adam_g0(stepped, optimizer):
    """The stepped module's layer-0 weight handle if rna_gan_amd.optim.Adam may form its gradient inside the fused step: the
    generator (DCGAN recipe), stepped by that optimizer bound to it, bf16 kernels."""
    if not G0_ADAM or not _own_adam(stepped, optimizer):
        return None
    ops, net = stepped.runtime()
    return net.g0 if isinstance(net, E.GenNet) and _is_half(ops) else None


def _fusable_g0(stepped, optimizer):
    """Single process: the optimizer step that follows the pass forms the gradient from the operands left on the handle."""
    return None if D_.active() else _adam_g0(stepped, optimizer)


# data-parallel runs: the gradient all-reduce + optimizer step of the last train_op, not yet applied
_PENDING = [None]
OVERLAP = os.environ.get("RNAGAN_DP_OVERLAP", "1") != "0"
FUSED_WIDEN = os.environ.get("RNAGAN_DP_FUSED_WIDEN", "1") != "0"


class _Pending:
    def __init__(self, module, optimizer, handle, factors=None):
        self.module, self.optimizer, self.handle, self.factors = module, optimizer, handle, factors


# data parallel, bf16 wire: the 4 x 4 layers' weight gradients go onto the wire without an fp32 gradient in between -- a split-K
# launch leaves its (bf16) slabs for rg_grad_to_wire, a launch without split-K writes its bf16 tile into the wire slice
# (ConvW.wire_slot / ops_hip._wgrad_slabs); needs ONE weight-gradient launch per layer and pass (the paired prefix form)
DP_WIRE_DIRECT = os.environ.get("RNAGAN_DP_WIRE_DIRECT", "1") != "0"


def _dp_wire_layers(stepped, optimizer):
    """[(ConvW, wire slice)] of the stepped module's layers whose weight gradients may bypass the fp32 gradient buffer."""
    if not (DP_WIRE_DIRECT and SLAB_ADAM and D_.active() and FUSED_WIDEN and (DP_PREFIX_MODE == 2 or DP_ROUTE == "whole")) \
            or D_.sync_stats():
        return []
    if not _own_adam(stepped, optimizer):
        return []
    ops, net = stepped.runtime()
    if not _wire_kind(ops) or not _local_half_dcgan(ops, net):
        return []
    flat = stepped.flat
    wire = D_.wire_for(flat.grad, ops.half)
    if wire is None:
        return []
    out = []
    for cw, _ in net.blocks:
        off = (cw.w.data_ptr() - flat.data.data_ptr()) // 4
        n = cw.w.numel()
        if cw.layout == "OHWI" and off % 8 == 0 and n % 4 == 0 and off >= 0 and off + n <= flat.data.numel():
            out.append((cw, wire[off:off + n]))
    return out


def _dp_wire_table(stepped, layers, head):
    """Segment table over flat[head:] from what the pass left on the layers (pending_slabs), or None when nothing was deferred."""
    flat = stepped.flat
    rows = []
    for cw, _ in layers:
        ps, cw.pending_slabs = cw.pending_slabs, None
        if ps is not None:
            rows.append(((cw.w.data_ptr() - flat.data.data_ptr()) // 4, cw.w.numel(), 0 if ps[0] is None else ps[0].data_ptr(),
                         ps[1], ps[2]))
    if not rows:
        return None
    rows.sort(key=lambda t: t[0])
    total, pos, table = flat.data.numel(), head, []
    for off, n, ptr, ns, sdt in rows:
        if off < pos:
            raise RuntimeError("rna_gan_amd: a deferred weight gradient overlaps the part of the flat buffer that does not travel "
                               "on the wire")
        if off > pos:
            table.append((pos - head, off - pos, 0, 0, 0))
        table.append((off - head, n, ptr, ns, sdt))
        pos = off + n
    if total > pos:
        table.append((pos - head, total - pos, 0, 0, 0))
    return table


def _dp_factor_g0(stepped, optimizer, batch):
    """Data parallel: (g0 handle, gathered-factor buffers) when the stepped module's layer-0 weight gradient can travel as
    FACTORS (dist.G0_FACTORS): DCGAN generator stepped by rna_gan_amd.optim.Adam bound to it, bf16 kernels, rank-local
    statistics, and the fused kernel takes K = world x batch."""
    if not (D_.G0_FACTORS and D_.active()) or D_.sync_stats():
        return None
    g0 = _adam_g0(stepped, optimizer)
    if g0 is None:
        return None
    ops, _ = stepped.runtime()
    En, C = g0.w.shape[0], g0.w.shape[1]
    if (g0.w.data_ptr() - stepped.flat.data.data_ptr()) != 0:
        return None
    if not ops.lib.rg_g0_wgrad_adam_supported(D_.world_size() * batch, En, C, ops.dt):
        return None
    return g0, D_.factor_buffers(id(stepped), batch, En, C, ops.h16, stepped.flat.data.device), ops.dt


def _dp_plan(stepped, optimizer, inputs):
    """(fac, wired, head) of a data-parallel gradient pass.  fac: generator-loss step -- layer 0's weight gradient travels as
    gathered factors (dist.G0_FACTORS): the backward copies z / gz0 into this rank's slices of the gathered buffers instead
    of forming the 67 M-element product (_dp_factor_g0: None for anything but the generator); wired: _dp_wire_layers;
    head: the leading elements of the flat gradient that stay off the all-reduce wire (G.0's, when it travels as factors)."""
    fac = _dp_factor_g0(stepped, optimizer, inputs[0].shape[0]) if inputs else None
    return fac, _dp_wire_layers(stepped, optimizer), fac[0].w.numel() if fac is not None else 0


def _dp_armed(fn, stepped, fac, wired, head, cell):
    """fn as a data-parallel gradient pass: armed for (fac, wired) of _dp_plan, and what the pass left pending consumed."""
    g0 = fac[0] if fac is not None else None

    def armed(*a):
        with _armed(wired=wired, g0=g0, factor_stage=None if fac is None else (fac[1][2], fac[1][3])):
            out = fn(*a)
            # what the weight-gradient launches of this pass left: kept with the graph this call captures (a replay runs
            # no host code, its launches are these)
            cell["wire_table"] = _dp_wire_table(stepped, wired, head)
            if g0 is not None:
                if g0.pending_wgrad != "staged":
                    raise RuntimeError("data-parallel G step: layer 0's weight gradient was not left as factors")
                g0.pending_wgrad = None               # (flush hands the GATHERED factors to the optimizer)
        return out
    return armed


def flush():
    """Apply the optimizer step a data-parallel train_op may have left in flight (all-reduce started, update not
    applied yet).  Called before anything reads parameters outside the train_ops: state_dict(), forward(), save."""
    pend, _PENDING[0] = _PENDING[0], None
    if pend is None:
        return
    # rna_gan_amd.optim.Adam steps straight from the all-reduced bf16 wire buffer (no widening pass; .grad then keeps
    # the rank-local gradient); other optimizers get the averaged gradient back in .grad first
    wire = D_.wire_of(pend.handle) if FUSED_WIDEN and _is_adam(pend.optimizer) else None
    # (with gathered G.0 factors the handle's head is excluded from the wire; the tail is widened like any other gradient
    # when the optimizer does not step from the wire -- RNAGAN_DP_FUSED_WIDEN=0 or a foreign optimizer)
    D_.allreduce_finish(pend.handle, widen=wire is None)
    fac = pend.factors
    if fac is not None:
        g0, (z_all, gy_all, _, _), dt, works = fac
        for w in works:
            if w is not None:
                w.wait()
        g0.pending_wgrad = (z_all, gy_all, dt)     # every rank's samples: the fused step forms sum_r z_r^T gz0_r itself
    if _is_adam(pend.optimizer):
        pend.optimizer.grad_wire = wire
    try:
        _APPLY_RUNNER.run(("apply", id(pend.module), wire is not None, fac is not None),
                          lambda: _apply(pend.module, pend.optimizer), [], [], [pend.optimizer], [pend.module])
    finally:
        if fac is not None:
            fac[0].pending_wgrad = None
    if _is_adam(pend.optimizer):
        pend.optimizer.grad_wire = None


class _Runner:
    """Executes a step body eagerly for the first calls, then from a captured HIP graph
    (rna_gan_amd.graphed.StepGraph).  One graph per (body, modules, optimizer, input shapes)."""

    MAX_GRAPHS = 24

    def __init__(self):
        self._graphs = {}
        self._pre = {}

    def __getstate__(self):          # loss objects are pickled into checkpoints; graphs are not state
        return {}

    def __setstate__(self, state):
        self._graphs = {}
        self._pre = {}

    def run_dp(self, key, body, inputs, modules, stepped, optimizer):
        """Data-parallel form.  Collectives are never captured, so a train_op is graph(prefix) -> graph(rest) ->
        eager all-reduce START; the all-reduce is only waited for -- and the optimizer step applied (a graph of its
        own) -- by the NEXT train_op after it has enqueued its prefix, which reads the other network: the RCCL
        transfer over xGMI overlaps with that compute.  flush() applies a trailing update."""
        if DP_ROUTE == "whole":
            return self._run_dp_whole(key, body, inputs, modules, stepped, optimizer)
        pend = _PENDING[0]
        if pend is not None and (not OVERLAP or pend.module is body.prefix_reads):
            flush()                                   # the prefix needs the updated weights: no overlap possible
        sg_pre = self._step_graph(key + ("pre",), body.prefix, inputs, [body.prefix_reads], [], [])
        pre = sg_pre(*inputs) if sg_pre is not None else body.prefix(*inputs)
        flush()
        # the rest reads the prefix's outputs through a holder: they are the prefix graph's static outputs once it is
        # captured, so the rest graph is tied to that prefix graph and may only be captured after it
        holder = self._pre.setdefault((key, id(sg_pre)), {})
        holder["pre"] = pre
        loss = self._dp_grads(key + ("rest", id(sg_pre)), lambda: body.rest(holder["pre"]), [], inputs, modules, stepped,
                              optimizer, allow_capture=sg_pre is not None and sg_pre.graph is not None)
        if not OVERLAP:
            flush()
        return loss

    def _run_dp_whole(self, key, body, inputs, modules, stepped, optimizer):
        """Route "whole" (DP_ROUTE): graph(the single process's gradient body) -> all-reduce -> wait -> graph(optimizer step)."""
        flush()
        loss = self._dp_grads(key + ("whole",), body.grads, inputs, inputs, modules, stepped, optimizer)
        flush()                                   # nothing to overlap with: wait and apply now
        return loss

    def _dp_grads(self, key, fn, fn_inputs, step_inputs, modules, stepped, optimizer, allow_capture=True):
        """What both data-parallel routes do with the gradient part ``fn(*fn_inputs)`` of a train_op: run it armed (_dp_armed) as
        one graph, START the gradient all-reduce (and the all-gathers of G.0's factors) and leave the optimizer step pending
        for flush().  step_inputs: the train_op's own inputs (their leading dimension is the batch).  Returns the loss."""
        fac, wired, head = _dp_plan(stepped, optimizer, step_inputs)
        # the wire segment table describes the launches of ONE graph: it lives with the StepGraph whose function wrote it
        # (StepGraph.wire_cell), not in a holder that every variant under one prefix (packs_stale, lr, buf_gen) overwrites
        cell = {}
        armed = _dp_armed(fn, stepped, fac, wired, head, cell)
        sg = self._step_graph(key + (fac is not None, len(wired)), armed, fn_inputs, modules, [], [])
        if sg is not None:
            if sg.wire_cell is None:
                sg.wire_cell = cell                   # created by this call: its function is the closure over this cell
            cell = sg.wire_cell                       # (an existing graph runs / replays the closure of the call that created it)
            loss = sg(*fn_inputs, allow_capture=allow_capture)
        else:
            loss = armed(*fn_inputs)
        ops, _ = stepped.runtime()
        handle = D_.allreduce_start(stepped.flat.grad, compress=_wire_kind(ops), head=head,
                                    table=cell.get("wire_table") if wired else None)
        if fac is not None:
            z_all, gy_all, z_mine, gy_mine = fac[1]
            fac = fac + ([D_.allgather_start(z, mine) for z, mine in ((z_all, z_mine), (gy_all, gy_mine))],)
        _PENDING[0] = _Pending(stepped, optimizer, handle, fac)
        return loss

    def run(self, key, fn, inputs, modules, optimizers, stepped=None):
        sg = self._step_graph(key, fn, inputs, modules, optimizers, stepped)
        return sg(*inputs) if sg is not None else fn(*inputs)

    def _step_graph(self, key, fn, inputs, modules, optimizers, stepped=None):
        """The StepGraph for this body / launch-sequence variant, or None when it has to run eagerly."""
        if not graphed.ENABLED or D_.sync_stats():       # synchronised statistics put collectives inside the step
            return None
        if stepped is None:
            stepped = [o._module for o in optimizers if getattr(o, "_module", None) is not None]
        hip_opts = [o for o in optimizers if _is_adam(o)]
        if len(hip_opts) != len(optimizers):
            return None                     # a foreign optimizer keeps host-side state: no capture
        for o in hip_opts:
            o._ensure()                     # moment / step buffers exist (and their generation is final) before keying
        # A captured graph freezes (a) the launch sequence, which depends on which packed weights are stale, (b) the raw
        # addresses of the flat parameter / gradient / shadow buffers and of Adam's moment / step buffers, (c) the
        # optimizer hyper-parameters passed as kernel arguments.  All three are part of the key: a re-homed module
        # (.to(), load into new storage), re-allocated optimizer state or a scheduler's new lr gets a new graph
        # instead of replaying one that updates freed buffers or steps with the old lr.
        key = key + tuple(tuple(t.shape) for t in inputs) + tuple(id(m) for m in modules) + \
            tuple(id(o) for o in optimizers) + tuple(int(m.packs_stale()) for m in modules) + \
            tuple(m.flat.gen for m in modules) + \
            tuple((o.buf_gen, float(o.param_groups[0]["lr"]), tuple(float(b) for b in o.param_groups[0]["betas"]),
                   float(o.param_groups[0]["eps"]), float(o.param_groups[0].get("weight_decay", 0.0))) for o in hip_opts)
        amp = tuple(_amp_key(m) for m in list(modules) + [o._module for o in hip_opts if o._module is not None])
        if any(a is not None for a in amp):
            # dynamic loss scaling: which scaler state the launches read (never its value -- that lives on the device)
            key = key + ("amp",) + amp
        sg = self._graphs.get(key)
        if sg is None:
            while len(self._graphs) >= self.MAX_GRAPHS:          # e.g. one lr value per epoch under a scheduler
                self._graphs.pop(next(iter(self._graphs)))
            sg = self._graphs[key] = graphed.StepGraph(fn, inputs, modules, hip_opts, stepped)
        return sg


def _amp_key(module):
    ops = getattr(module, "_rt_ops", None)
    sc = getattr(ops, "amp", None)
    return None if sc is None else (id(sc), sc.state.data_ptr())


_APPLY_RUNNER = _Runner()
D_.set_flush_hook(flush)
