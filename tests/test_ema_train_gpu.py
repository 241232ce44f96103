"""The averaged generator (rna_gan_amd.ema.ParamEMA, Trainer(ema_decay=...)) through training.

The yardstick is the SNAPSHOT RECURRENCE: after every iteration the live generator's flat buffer and Adam's device step counter
are read back; whenever the counter advanced, a host copy of the average is advanced with the numpy reference of the kernel
(tests/ema_refs.py) from that snapshot and that counter.  The twin's flat buffer must equal the host copy BIT FOR BIT at the end
-- through eager steps, captured and replayed step graphs, skipped steps of dynamic loss scaling, a re-homed twin and the
deferred optimizer step of the data-parallel tail.  Shapes: the smallest the training tests use (in_size 32, step 64, enc 128,
batch 16)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R
import rna_gan_amd as P
from rna_gan_amd import graphed
from rna_gan_amd.amp import DynamicLossScaler
from rna_gan_amd.ema import ParamEMA
from rna_gan_amd.gan_utils import generate_images, synthesize
from ema_refs import ema_update_ref
from test_train_gpu import product_pair
from test_loss_scaler_gpu import _models, _plugins
from test_trainer_gpu import network

IN_SIZE, STEP, ENC, N = 32, 64, 128, 16
DECAY = 0.999


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flat_np(module):
    flat = module.flat
    return flat.data[:flat.numel].detach().cpu().numpy().copy()


class _Recurrence:
    """The host copy of the average, advanced from snapshots."""

    def __init__(self, G, og, ema):
        self.G, self.og, self.ema = G, og, ema
        og._ensure()
        torch.cuda.synchronize()
        self.host = _flat_np(ema.module)
        self.t = int(og._step_dev.item())
        self.advanced = 0

    def observe(self):
        """Call after every iteration (at most one generator step since the last call).  True when the counter advanced."""
        torch.cuda.synchronize()
        t = int(self.og._step_dev.item())
        assert t in (self.t, self.t + 1), (self.t, t)
        moved = t != self.t
        if moved:
            self.host = ema_update_ref(_flat_np(self.G), self.host, self.ema.decay, t if self.ema.warmup else None)
            self.advanced += 1
        self.t = t
        return moved

    def check(self, what=""):
        torch.cuda.synchronize()
        got = _flat_np(self.ema.module)
        bad = np.flatnonzero(_bits(got) != _bits(self.host))
        assert bad.size == 0, "%s: %d of %d elements of the average differ from the snapshot recurrence (first at %d: %r vs %r)" % (
            what, bad.size, got.size, bad[0], got[bad[0]], self.host[bad[0]])


def _setup(precision="bf16", decay=DECAY, warmup=True, seed=11, with_ema=True):
    G0, D0 = _models(IN_SIZE, STEP, ENC)
    torch.manual_seed(seed)
    G, D, og, od = product_pair(IN_SIZE, STEP, ENC, precision, G0, D0)
    ema = None
    if with_ema:
        ema = ParamEMA(G, decay, warmup=warmup)
        og.attach_ema(ema)
    return G, D, og, od, ema


def _iteration(plugins, G, D, og, od, it, g_step=True):
    lg, ld, lp = plugins
    real = R.synthetic_images(N, IN_SIZE, seed=100 + it).cuda()
    row = []
    if g_step:
        row.append(lg.train_ops(G, D, og, "cuda", N))
    row.append(ld.train_ops(G, D, od, real, "cuda"))
    row.append(lp.train_ops(G, D, od, real, "cuda"))
    return row


@pytest.mark.parametrize("mode", ["graphs", "eager", "g_every_2nd"])
def test_recurrence(mode, monkeypatch):
    if mode == "eager":
        monkeypatch.setattr(graphed, "ENABLED", False)             # (restored by monkeypatch)
    elif not graphed.ENABLED:
        pytest.skip("RNAGAN_GRAPHS=0")
    G, D, og, od, ema = _setup()
    assert not ema.module.training and G.training
    plugins = _plugins()
    rec = _Recurrence(G, og, ema)
    assert np.array_equal(_bits(rec.host), _bits(_flat_np(G)))     # the average starts from the live parameters
    iters = graphed.WARMUP_CALLS + 4
    for it in range(iters):
        g_step = mode != "g_every_2nd" or it % 2 == 0
        _iteration(plugins, G, D, og, od, it, g_step)
        assert rec.observe() == g_step
    rec.check(mode)
    assert rec.advanced == (iters if mode != "g_every_2nd" else (iters + 1) // 2)
    assert not np.array_equal(_bits(rec.host), _bits(_flat_np(G)))  # an average, not a copy
    captured = [sg.graph is not None for sg in plugins[0]._runner._graphs.values()]
    if mode == "graphs":
        assert any(captured), "the generator step graph was never captured"
    if mode == "eager":
        assert not captured
    assert not ema.module.training and G.training                  # the loop never touches the twin's mode


def test_observer_changes_nothing():
    """Two runs from the same seeds, without and with the average: identical losses, parameters, buffers and Adam moments, and no
    additional step graph.  Without the average the optimizer's buffer generation is 1 (one bump, when the moments are made):
    the graph keys are what they were before the feature existed."""
    res = {}
    for with_ema in (False, True):
        G, D, og, od, ema = _setup(with_ema=with_ema)
        plugins = _plugins()
        losses = [_iteration(plugins, G, D, og, od, it) for it in range(graphed.WARMUP_CALLS + 3)]
        torch.cuda.synchronize()
        res[with_ema] = (losses, [p.detach().clone() for p in list(G.parameters()) + list(D.parameters())],
                         [b.detach().clone() for b in list(G.buffers()) + list(D.buffers())],
                         [og._m.clone(), og._v.clone(), od._m.clone(), od._v.clone(), og._step_dev.clone()],
                         [len(p._runner._graphs) for p in plugins], og.buf_gen, od.buf_gen)
    off, on = res[False], res[True]
    assert off[0] == on[0]
    for k in (1, 2, 3):
        assert len(off[k]) == len(on[k])
        for a, b in zip(off[k], on[k]):
            assert torch.equal(a, b)
    assert off[4] == on[4]
    assert off[5] == 1 and off[6] == 1 and on[6] == 1 and on[5] > 1


def test_skipped_steps_leave_the_average_alone():
    """fp16 build, dynamic loss scaling started at 2^40 (the recipe of tests/test_loss_scaler_gpu.py: the gradients overflow, the
    step is skipped on the device, the scale backs off; nothing faults)."""
    G, D, og, od, ema = _setup(precision="fp16", seed=5, with_ema=False)
    sc = DynamicLossScaler(init_scale=2.0 ** 40, growth_interval=10 ** 6).attach(G, D)
    ema = ParamEMA(G, DECAY, warmup=True)
    og.attach_ema(ema)
    lg, ld, lp = plugins = _plugins()
    rec = _Recurrence(G, og, ema)
    skipped_g = stepped_g = 0
    # the scale comes down by one binade per skipped step; the generator's gradients (through the critic) stay above fp16's range
    # longest.  Run until three generator steps were taken behind the skipped ones (64 iterations at most: 2^40 -> 2^-24)
    for it in range(64):
        if skipped_g >= 1 and stepped_g >= 3:
            break
        real = R.synthetic_images(N, IN_SIZE, seed=300 + it).cuda()
        before = _flat_np(ema.module)
        seen = sc.skipped_steps()
        lg.train_ops(G, D, og, "cuda", N)
        g_skipped = sc.skipped_steps() > seen
        moved = rec.observe()
        assert moved == (not g_skipped)
        if g_skipped:
            skipped_g += 1
            assert np.array_equal(_bits(before), _bits(_flat_np(ema.module))), "a skipped generator step moved the average (it %d)" % it
        else:
            stepped_g += 1
        ld.train_ops(G, D, od, real, "cuda")
        lp.train_ops(G, D, od, real, "cuda")
        assert not rec.observe()
    print("generator steps: %d skipped, %d taken" % (skipped_g, stepped_g))
    assert skipped_g >= 1, "no generator step was skipped: the run proves nothing about the skip word"
    rec.check("fp16 dynamic")
    assert rec.advanced == stepped_g == int(og._step_dev.item())
    assert stepped_g >= 3, "the generator never recovered: the recurrence was not exercised behind the skipped steps"


def test_twin_is_usable_and_rehomes():
    if not graphed.ENABLED:
        pytest.skip("RNAGAN_GRAPHS=0")
    G, D, og, od, ema = _setup()
    plugins = _plugins()
    rec = _Recurrence(G, og, ema)
    iters = graphed.WARMUP_CALLS + 3
    for it in range(iters):
        _iteration(plugins, G, D, og, od, it)
        rec.observe()
    rec.check("before")
    twin = ema.module
    # no shared storage
    mine = {t.untyped_storage().data_ptr() for t in list(G.parameters()) + list(G.buffers())}
    assert all(t.untyped_storage().data_ptr() not in mine for t in list(twin.parameters()) + list(twin.buffers()))
    assert twin.flat.data.data_ptr() != G.flat.data.data_ptr()
    # buffers: copied on demand
    assert any(not torch.equal(a, b) for a, b in zip(G.buffers(), twin.buffers()))      # G's running statistics moved on
    ema.sync_buffers()
    for (ka, a), (kb, b) in zip(G.named_buffers(), twin.named_buffers()):
        assert ka == kb and torch.equal(a, b)
    # the twin's operand images follow its masters through replayed steps: synthesis from the twin == synthesis from a fresh
    # generator loaded with the twin's state
    noise = R.synthetic_normal(8, ENC, seed=77).cuda()
    got = synthesize(twin, noise).clone()
    fresh = P.DCGANGenerator(ENC, IN_SIZE, 3, STEP, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
    fresh.load_state_dict(ema.state_dict())
    fresh.set_precision("bf16")
    want = synthesize(fresh.cuda(), noise)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert not torch.equal(got, synthesize(G, noise))               # ... and it is not the live generator's output
    # again after one more (replayed) step: stale images would reproduce `got`
    _iteration(plugins, G, D, og, od, iters); rec.observe()
    ema.sync_buffers()                                              # (the live running statistics moved with that iteration)
    got2 = synthesize(twin, noise).clone()
    fresh.load_state_dict(ema.state_dict())
    assert torch.equal(got2, synthesize(fresh, noise)) and not torch.equal(got2, got)
    rec.check("after synthesis")
    # re-homing: the twin goes to the CPU and back -- new storage, the old flat buffer is given back
    old_ptr, gen0 = twin.flat.data.data_ptr(), og.buf_gen
    twin.cpu(); twin.cuda()
    for it in range(iters + 1, iters + 3):
        _iteration(plugins, G, D, og, od, it)
        assert rec.observe()
    assert og.buf_gen > gen0
    rec.check("after re-homing")
    assert not twin.training and not any(p.requires_grad for p in twin.parameters())
    # decay / warm-up are frozen while attached; detaching bumps the generation again and stops the average
    with pytest.raises(RuntimeError):
        ema.decay = 0.5
    gen1 = og.buf_gen
    assert og.detach_ema() is ema and og.buf_gen > gen1
    frozen = _flat_np(twin)
    _iteration(plugins, G, D, og, od, iters + 3)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(frozen), _bits(_flat_np(twin)))
    # reset(): the twin becomes the live module again
    ema.reset()
    assert np.array_equal(_bits(_flat_np(twin)), _bits(_flat_np(G)))


def _loader():
    imgs = R.synthetic_images(3 * N, IN_SIZE, seed=5)
    return DataLoader(TensorDataset(imgs, torch.zeros(3 * N)), batch_size=N)


def _trainer(tmp_path, tag, **kw):
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    return P.Trainer(network(IN_SIZE, ENC), losses, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4, epochs=1,
                     recon=str(tmp_path / ("img" + tag)), nrow=2, **kw)


def test_trainer_checkpoints_and_samples_the_average(tmp_path):
    torch.manual_seed(0)
    tr = _trainer(tmp_path, "a", ema_decay=0.99)
    assert tr.generator_ema is tr.ema.module and "generator_ema" not in tr.model_names
    tr(_loader())
    assert not tr.generator_ema.training
    ck = torch.load(str(tmp_path / "gana0.model"), map_location="cpu", weights_only=False)
    for key in ("epoch", "loss_information", "loss_objects", "metric_objects", "loss_logs", "metric_logs", "generator",
                "discriminator", "optimizer_generator", "optimizer_discriminator"):
        assert key in ck, key
    assert list(ck["generator_ema"].keys()) == list(ck["generator"].keys())
    assert ck["ema_information"] == {"decay": 0.99, "warmup": True}
    assert any(not torch.equal(ck["generator_ema"][k], ck["generator"][k]) for k in ck["generator"] if "weight" in k)
    for k, v in ck["generator"].items():                            # the buffers are the live generator's (copied, not averaged)
        if "running_" in k or "num_batches" in k:
            assert torch.equal(v, ck["generator_ema"][k]), k
    assert os.path.isfile(str(tmp_path / "imga" / "epoch1_generator.png"))
    assert os.path.isfile(str(tmp_path / "imga" / "epoch1_generator_ema.png"))
    # a second trainer restores the average bit for bit
    tr2 = _trainer(tmp_path, "b", ema_decay=0.99)
    tr2.load_model(load_path=str(tmp_path / "gana0.model"))
    for (ka, a), (kb, b) in zip(tr.ema.state_dict().items(), tr2.ema.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    # averaging off: neither key nor file, and such a checkpoint resets the average to the loaded generator
    tr3 = _trainer(tmp_path, "c")
    assert tr3.ema is None and tr3.generator_ema is None
    tr3.load_model(load_path=str(tmp_path / "gana0.model"))       # "generator_ema" present, averaging off: ignored
    tr3.save_model(0)
    tr3.test_noise = tr3.generator.sampler(4, tr3.device)
    tr3.sample_images(0)
    assert os.path.isfile(str(tmp_path / "imgc" / "epoch1_generator.png"))
    ck3 = torch.load(str(tmp_path / "ganc0.model"), map_location="cpu", weights_only=False)
    assert "generator_ema" not in ck3 and "ema_information" not in ck3
    assert not os.path.exists(str(tmp_path / "imgc" / "epoch1_generator_ema.png"))
    tr4 = _trainer(tmp_path, "d", ema_decay=0.99)
    tr4.load_model(load_path=str(tmp_path / "ganc0.model"))
    for (ka, a), (kb, b) in zip(tr4.generator.state_dict().items(), tr4.generator_ema.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    assert torch.equal(tr4.generator.state_dict()["model.0.0.weight"].cpu(), ck["generator"]["model.0.0.weight"])
    # generate_images from the average
    img = generate_images(tr, sample_size=10, ema=True)
    assert img.shape == (10, IN_SIZE, IN_SIZE, 3) and img.dtype == np.float32 and np.isfinite(img).all()
    assert img.min() >= 0.0 and img.max() <= 1.0
    with pytest.raises(ValueError):
        generate_images(tr3, sample_size=10, ema=True)
    # a foreign generator optimizer cannot carry the launch
    net = network(IN_SIZE, ENC)
    net["generator"]["optimizer"] = {"name": torch.optim.SGD, "args": {"lr": 0.1}}
    with pytest.raises(ValueError):
        P.Trainer(net, [P.WassersteinGeneratorLoss()], checkpoints=str(tmp_path / "gane"), recon=str(tmp_path / "imge"),
                  ema_decay=0.99)


WORKER = r'''
import os, sys, numpy as np, torch, torch.nn as nn
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import torch.distributed as dist
from rna_gan_amd import dist as D_, losses as PL
from rna_gan_amd.ema import ParamEMA
import rna_gan_amd as P
from oracle import ref_cpu as R
from ema_refs import ema_update_ref
rank = int(os.environ["RANK"])
torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
D_.init_from_env(backend="gloo")
assert D_.world_size() == 2 and D_.active()
D_.COMPRESS = False                                  # fp32 wire: every gloo build reduces it
in_size, step, enc, n, iters = [int(v) for v in os.environ["SHAPE"].split(",")]
G0 = R.seeded_fill_(R.OracleDCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh()), 7)
D0 = R.seeded_fill_(R.OracleDCGANDiscriminator(in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2)), 8)
G = P.DCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
D = P.DCGANDiscriminator(in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2))
G.load_state_dict(G0.state_dict()); D.load_state_dict(D0.state_dict())
G, D = G.cuda().train(), D.cuda().train()
og = P.Adam(G.parameters(), lr=1e-4, betas=(0.5, 0.999)).bind(G)
od = P.Adam(D.parameters(), lr=4e-4, betas=(0.5, 0.999)).bind(D)
ema = ParamEMA(G, 0.999, warmup=True)
og.attach_ema(ema)
lg, ld, lp = PL.WassersteinGeneratorLoss(), PL.WassersteinDiscriminatorLoss(), PL.WassersteinGradientPenalty()
flat = lambda m: m.flat.data[:m.flat.numel].detach().cpu().numpy().copy()
og._ensure()
host, t0, advanced = flat(ema.module), int(og._step_dev.item()), 0
for it in range(iters):
    real = R.synthetic_images(n, in_size, seed=100 + 10 * it + rank).cuda()
    nz = [R.synthetic_normal(n, enc, seed=200 + 30 * it + 3 * rank + j).cuda() for j in range(3)]
    eps = torch.tensor([0.15 + 0.2 * it + 0.3 * rank], device="cuda")
    lg.step(G, D, og, nz[0]); ld.step(G, D, od, real, nz[1]); lp.step(G, D, od, real, nz[2], eps)
    # the generator's step of this iteration was deferred into the tail that the D-loss train_op flushed
    torch.cuda.synchronize()
    t = int(og._step_dev.item())
    assert t == t0 + 1, (t0, t)
    host = ema_update_ref(flat(G), host, 0.999, t); t0 = t; advanced += 1
PL.flush()
torch.cuda.synchronize()
torch.save({"twin": torch.from_numpy(flat(ema.module)), "host": torch.from_numpy(host), "G": torch.from_numpy(flat(G)),
            "advanced": advanced}, os.environ["OUT"] + str(rank))
dist.barrier()
dist.destroy_process_group()
'''


def test_data_parallel_world_2(tmp_path):
    """Two gloo ranks on one device (the manner of tests/test_dp2_gpu.py), three iterations: the generator's optimizer step --
    and the average's launch inside it -- runs in the deferred data-parallel tail.  The two ranks' averages are bit-identical
    and equal the snapshot recurrence."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "ema_dp2_rank")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, REPO=repo, OUT=out, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                   LOCAL_RANK="0", WORLD_SIZE="2", RNAGAN_FORCE_DP="0", SHAPE="%d,%d,%d,%d,%d" % (IN_SIZE, STEP, ENC, 8, 3))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    for p in procs:
        try:
            _, err = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err[-3000:]
    r0, r1 = [torch.load(out + str(r)) for r in range(2)]
    assert r0["advanced"] == r1["advanced"] == 3
    assert torch.equal(r0["G"].view(torch.int32), r1["G"].view(torch.int32))
    assert torch.equal(r0["twin"].view(torch.int32), r1["twin"].view(torch.int32))
    assert torch.equal(r0["twin"].view(torch.int32), r0["host"].view(torch.int32))
    assert not torch.equal(r0["twin"], r0["G"])
