"""Dynamic loss scaling (rna_gan_amd.amp) under data parallel at WORLD SIZE 2: two rank processes sharing the device and
all-reducing over gloo, as tests/test_dp2_gpu.py runs them.

  * bf16 (power-of-two scaling exact), growth_interval = 1 so that the scale doubles after EVERY train_op, on both routes: the
    parameters are bit-identical to the same world-2 run without a scaler.  In the "prefix" route the generator's pending step
    -- and its scale update -- runs between the D-loss prefix (which seeds D(real)) and its rest: without the per-network latch
    the two halves of that train_op would carry different scales;
  * fp16 with a non-finite input on ONE rank: the all-reduced gradient carries it to both, both ranks skip the same steps and
    keep bit-identical, finite parameters.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_dp2_gpu import _free_port, _require_devices

WORKER = r'''
import os, sys, torch, torch.nn as nn
sys.path.insert(0, os.environ["REPO"])
import torch.distributed as dist
from rna_gan_amd import dist as D_, losses as PL
from rna_gan_amd.amp import DynamicLossScaler
import rna_gan_amd as P
from oracle import ref_cpu as R
rank = int(os.environ["RANK"])
torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
D_.init_from_env(backend="gloo")
assert D_.world_size() == 2 and D_.active()
precision = os.environ["PRECISION"]
if precision == "bf16":                        # does this gloo build all-reduce bf16 device tensors?
    try:
        t = torch.ones(8, dtype=torch.bfloat16, device="cuda")
        dist.all_reduce(t)
        if float(t[0]) != 2.0:
            D_.COMPRESS = False
    except Exception:
        D_.COMPRESS = False
in_size, step, enc, n, iters = 32, 64, 128, 8, 4
G0 = R.seeded_fill_(R.OracleDCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh()), 7)
D0 = R.seeded_fill_(R.OracleDCGANDiscriminator(in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2)), 8)
G = P.DCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
D = P.DCGANDiscriminator(in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2))
G.load_state_dict(G0.state_dict()); D.load_state_dict(D0.state_dict())
G.set_precision(precision); D.set_precision(precision)
G, D = G.cuda().train(), D.cuda().train()
og = P.Adam(G.parameters(), lr=1e-4, betas=(0.5, 0.999)).bind(G)
od = P.Adam(D.parameters(), lr=4e-4, betas=(0.5, 0.999)).bind(D)
sc = None
if os.environ["AMP"] != "0":
    init, interval = os.environ["AMP"].split(",")
    sc = DynamicLossScaler(init_scale=float(init), growth_interval=int(interval)).attach(G, D)
poison = int(os.environ.get("POISON_RANK", "-1"))
lg, ld, lp = PL.WassersteinGeneratorLoss(), PL.WassersteinDiscriminatorLoss(), PL.WassersteinGradientPenalty()
losses, history = [], []
for it in range(iters):
    real = R.synthetic_images(n, in_size, seed=100 + 10 * it + rank).cuda()
    if rank == poison and it == 1:
        real[0, 0, 0, 0] = float("inf")        # this rank's D-loss and penalty gradients turn non-finite
    nz = [R.synthetic_normal(n, enc, seed=200 + 30 * it + 3 * rank + j).cuda() for j in range(3)]
    eps = torch.tensor([0.15 + 0.2 * it + 0.3 * rank], device="cuda")
    losses += [lg.step(G, D, og, nz[0]).item(), ld.step(G, D, od, real, nz[1]).item(), lp.step(G, D, od, real, nz[2], eps).item()]
PL.flush()
if sc is not None:                             # (read once at the end: a read flushes the pending step, the route is left alone)
    history.append((sc.get_scale(), sc.skipped_steps()))
torch.cuda.synchronize()
torch.save({"losses": losses, "history": history, "steps": (int(og._step_dev.item()), int(od._step_dev.item())),
            "G": {k: v.cpu() for k, v in G.state_dict().items()},
            "D": {k: v.cpu() for k, v in D.state_dict().items()}}, os.environ["OUT"] + str(rank))
dist.barrier()
dist.destroy_process_group()
'''


def _run(tmp_path, precision, amp, route, poison=-1):
    _require_devices(2)
    ndev = torch.cuda.device_count()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / ("amp_%s_%s_%s_%d_rank" % (precision, amp.replace(",", "_"), route, poison)))
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, REPO=repo, OUT=out, PRECISION=precision, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   RANK=str(rank), LOCAL_RANK=str(rank % ndev), WORLD_SIZE="2", RNAGAN_FORCE_DP="0", AMP=amp,
                   RNAGAN_DP_ROUTE=route, POISON_RANK=str(poison))
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
    return [torch.load(out + str(r)) for r in range(2)]


def _params(res, net):
    return {k: v for k, v in res[net].items() if "running" not in k and "num_batches" not in k}


@pytest.mark.parametrize("route", ["prefix", "whole"])
def test_dp2_dynamic_scale_is_exact(tmp_path, route):
    plain = _run(tmp_path, "bf16", "0", route)
    scaled = _run(tmp_path, "bf16", "16,1", route)
    # the scale doubled after every train_op of both ranks alike, nothing was skipped
    assert scaled[0]["history"] == scaled[1]["history"] == [(16.0 * 2.0 ** 12, 0)]
    for r in range(2):
        assert scaled[r]["losses"] == plain[r]["losses"]
        for net in ("G", "D"):
            for k, v in plain[r][net].items():
                assert torch.equal(v, scaled[r][net][k]), (route, r, net, k)


@pytest.mark.parametrize("route", ["prefix", "whole"])
def test_dp2_fp16_non_finite_on_one_rank_skips_on_both(tmp_path, route):
    res = _run(tmp_path, "fp16", "4096,1000000", route, poison=1)
    assert res[0]["history"] == res[1]["history"]
    skipped = res[0]["history"][-1][1]
    assert skipped >= 1 and res[0]["history"][-1][0] == 4096.0 / 2 ** skipped
    assert res[0]["steps"] == res[1]["steps"] and sum(res[0]["steps"]) == 3 * 4 - skipped
    for net in ("G", "D"):
        a, b = _params(res[0], net), _params(res[1], net)
        for k, v in a.items():
            assert torch.equal(v, b[k]), (route, net, k)              # rank-identical
            assert bool(torch.isfinite(v).all()), (route, net, k)
