"""Training with the BatchNorm-free critic, DCGANDiscriminator(batchnorm=False), on the GPU: two iterations against the CPU
oracle in the three precisions, the penalty step's exactly-zero bias gradients, graph replay against eager launches, the Trainer
(checkpoint round trip, the CLI flag) and the data-parallel route at world size 2.

The 16-bit gates of the two-iteration test are TWICE the worst figure of 24 consecutive unselected seeds (0..23) at the test's
own shapes, measured with two_iterations() below by tools/critic_plain_tolerance.py and recorded in
profiles/critic_plain_tolerance.txt (the factor 2: a 24-seed maximum understates the tail)."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import Adam
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R
import rna_gan_amd as P
from rna_gan_amd import losses as PL

IN_SIZE, STEP, ENC, N = 32, 64, 128, 16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_pair(seed, in_size=IN_SIZE, step=STEP, enc=ENC):
    G0 = R.seeded_fill_(R.OracleDCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2),
                                               last_nonlinearity=nn.Tanh()), 7 + seed)
    D0 = R.seeded_fill_(R.OracleDCGANDiscriminator(in_size, 3, step, batchnorm=False, nonlinearity=nn.LeakyReLU(0.2),
                                                   last_nonlinearity=nn.LeakyReLU(0.2)), 1008 + seed)
    return G0, D0


def product_pair(precision, G_src, D_src, in_size=IN_SIZE, step=STEP, enc=ENC, lr_d=4e-4):
    G = P.DCGANGenerator(enc, in_size, 3, step, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
    D = P.DCGANDiscriminator(in_size, 3, step, batchnorm=False, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2))
    G.load_state_dict(G_src.state_dict()); D.load_state_dict(D_src.state_dict())
    G.set_precision(precision); D.set_precision(precision)
    G, D = G.cuda().train(), D.cuda().train()
    og = P.Adam(G.parameters(), lr=1e-4, betas=(0.5, 0.999)).bind(G)
    od = P.Adam(D.parameters(), lr=lr_d, betas=(0.5, 0.999)).bind(D)
    return G, D, og, od


def bias_grads(D):
    return {k: p.grad for k, p in D.named_parameters() if k.endswith("bias")}


def update_cosine(du, dr):
    """Cosine between two parameter updates; an update that is exactly zero on the oracle (the head's bias when its gradient
    sum_n gh_n cancels in the D step: the penalty step never moves it) must be exactly zero here too, and then counts as 1."""
    du, dr = du.double().reshape(-1), dr.double().reshape(-1)
    if float(dr.norm()) == 0.0:
        return 1.0 if float(du.norm()) == 0.0 else 0.0
    return float((du * dr).sum() / (du.norm() * dr.norm() + 1e-300))


def numel_of(name):
    """Elements of the parameter `G.<key>` / `D.<key>` at the test's shapes."""
    G0, D0 = oracle_pair(0)
    return dict((G0 if name[0] == "G" else D0).named_parameters())[name[2:]].numel()


def two_iterations(seed, precision):
    """Two iterations (clip on the second) on the HIP path and on the CPU oracle from the same weights and draws.  Returns
    (loss errors [6] as |got - want| / (|want| + 0.5), {parameter: update cosine after iteration 0}, Adam step counts, whether
    every bias gradient was exactly zero after each penalty step)."""
    G0, D0 = oracle_pair(seed)
    Go, Do = copy.deepcopy(G0).train(), copy.deepcopy(D0).train()
    ogo, odo = R.make_adam(Go.parameters(), 1e-4), R.make_adam(Do.parameters(), 4e-4)
    G, D, og, od = product_pair(precision, G0, D0)
    errs, cos, zero_bias = [], {}, True
    for it in range(2):
        real = R.synthetic_images(N, IN_SIZE, seed=100 + it + 10 * seed)
        noises = [R.synthetic_normal(N, ENC, seed=200 + 3 * it + j + 100 * seed) for j in range(3)]
        eps = 0.25 + 0.5 * it
        clip = (-0.01, 0.01) if it == 1 else None
        ref = R.train_iteration(Go, Do, ogo, odo, real, noises, eps, clip=clip)
        rd = real.cuda()
        got = {"g": PL._g_step(G, D, og, noises[0].cuda()).item(),
               "d": PL._d_step(G, D, od, rd, noises[1].cuda(), clip).item(),
               "gp": PL._gp_step(G, D, od, rd, noises[2].cuda(), eps, 10.0).item()}
        bg = bias_grads(D)
        assert len(bg) == len(list(D.model.children())) + 1
        zero_bias = zero_bias and all(bool((g == 0).all()) for g in bg.values())
        errs += [abs(got[k] - ref[k]) / (abs(ref[k]) + 0.5) if np.isfinite(got[k]) else float("inf") for k in ("g", "d", "gp")]
        if it == 0:
            for tag, mod, ref_mod, src in (("G.", G, Go, G0), ("D.", D, Do, D0)):
                for (k, p), (_, q), (_, s) in zip(mod.named_parameters(), ref_mod.named_parameters(), src.named_parameters()):
                    cos[tag + k] = update_cosine(p.detach().cpu() - s.detach(), q.detach() - s.detach())
    steps = ([float(s["step"]) for s in og.state_dict()["state"].values()], [float(s["step"]) for s in od.state_dict()["state"].values()])
    return errs, cos, steps, zero_bias


# precision -> (loss gate, per-tensor update-cosine gate, the same over the tensors with >= LARGE elements).
# fp32: the project's fp32 gates (test_two_iterations_vs_oracle, test_reference_trainops_fixture).
# bf16 / fp16: 2 x the worst of seeds 0..23 (profiles/critic_plain_tolerance.txt, which also says why the loss gates are looser
# than the BatchNorm critic's 4e-2 and why the all-tensor cosine gate is vacuous: on seeds 1, 12 and 15 the oracle's head-bias
# gradient sum_n gh_n cancels exactly while one head pre-activation of the 16-bit run sits on the other side of the LeakyReLU
# kink, and a 1-element tensor's cosine is then 0 -- so the gate that bites is the one over the large tensors).
LARGE = 4096
GATES = {"fp32": (2e-3, 1 - 2e-3, 1 - 2e-3), "bf16": (1.010e-1, -1.0, 0.67604), "fp16": (7.321e-2, -1.0, 0.80455)}


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_two_iterations_vs_oracle(precision):
    tol_loss, min_cos, min_cos_large = GATES[precision]
    errs, cos, steps, zero_bias = two_iterations(0, precision)
    worst = min(cos, key=cos.get)
    big = {k: c for k, c in cos.items() if numel_of(k) >= LARGE}
    worst_big = min(big, key=big.get)
    print("%s: loss errors %s; worst update cosine %.5f (%s), over the large tensors %.5f (%s)"
          % (precision, np.round(errs, 5).tolist(), cos[worst], worst, big[worst_big], worst_big))
    assert max(errs) <= tol_loss, errs
    assert cos[worst] >= min_cos, (worst, cos[worst])
    assert big[worst_big] >= min_cos_large, (worst_big, big[worst_big])
    assert set(steps[0]) == {2.0} and set(steps[1]) == {4.0}           # one G step, two D steps per iteration: biases too
    assert zero_bias, "a bias gradient of the penalty step is not exactly zero"


def test_graph_replay_equals_eager():
    """The three train_ops replayed from captured HIP graphs leave bit-identical parameters to eager launches."""
    from rna_gan_amd import graphed
    n = 8
    G0, D0 = oracle_pair(0)
    results = []
    for use_graphs in (True, False):
        graphed.ENABLED = use_graphs
        try:
            G, D, og, od = product_pair("bf16", G0, D0)
            lg, ld, lp = PL.WassersteinGeneratorLoss(), PL.WassersteinDiscriminatorLoss(clip=(-0.01, 0.01)), \
                PL.WassersteinGradientPenalty()
            losses = []
            for it in range(5):                      # calls 1-2 eager, 3 captures + replays, 4-5 replay
                real = R.synthetic_images(n, IN_SIZE, seed=100 + it).cuda()
                nz = [R.synthetic_normal(n, ENC, seed=200 + 3 * it + j).cuda() for j in range(3)]
                eps = torch.tensor([0.1 + 0.2 * it], device="cuda")
                losses += [lg.step(G, D, og, nz[0]).item(), ld.step(G, D, od, real, nz[1]).item(),
                           lp.step(G, D, od, real, nz[2], eps).item()]
                assert all(bool((g == 0).all()) for g in bias_grads(D).values())
            results.append((losses, G.flat.data.clone(), D.flat.data.clone(), og.state_dict(), od.state_dict()))
        finally:
            graphed.ENABLED = True
    (la, ga, da, oga, oda), (lb, gb, db, ogb, odb) = results
    assert all(np.isfinite(v) for v in la) and la == lb
    assert torch.equal(ga, gb) and torch.equal(da, db)
    assert float(oga["state"][0]["step"]) == float(ogb["state"][0]["step"]) == 5.0
    assert [float(s["step"]) for s in oda["state"].values()] == [float(s["step"]) for s in odb["state"].values()] == [10.0] * 8


def _network(in_size=32, enc=64):
    return {
        "generator": {"name": P.DCGANGenerator,
                      "args": {"encoding_dims": enc, "out_channels": 3, "step_channels": 64, "out_size": in_size,
                               "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.Tanh()},
                      "optimizer": {"name": Adam, "args": {"lr": 0.0001, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": {"in_size": in_size, "in_channels": 3, "step_channels": 64, "batchnorm": False,
                                   "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.LeakyReLU(0.2)},
                          "optimizer": {"name": Adam, "args": {"lr": 0.0004, "betas": (0.5, 0.999)}}},
    }


def _plugins():
    return [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(clip=(-0.01, 0.01)), P.WassersteinGradientPenalty()]


def test_trainer_checkpoint_roundtrip_and_next_iteration(tmp_path):
    torch.manual_seed(0)
    imgs = R.synthetic_images(24, 32, seed=5)
    loader = DataLoader(TensorDataset(imgs, torch.zeros(24)), batch_size=8)
    ck = str(tmp_path / "gan")
    tr = P.Trainer(_network(), _plugins(), checkpoints=ck, sample_size=16, epochs=1, devices=[0], recon=str(tmp_path / "img"), nrow=4)
    tr(loader)                                                           # three iterations, then the checkpoint
    assert tr.loss_information["generator_iters"] == 3 and tr.loss_information["discriminator_iters"] == 6
    assert all(len(v) == 3 and all(np.isfinite(x) for x in v) for v in tr.loss_logs.values())
    sd = torch.load(ck + "0.model", map_location="cpu", weights_only=False)
    Do = R.OracleDCGANDiscriminator(32, 3, 64, batchnorm=False)
    Do.load_state_dict(sd["discriminator"])                              # the ordinary state_dict: the oracle module takes it
    assert list(sd["discriminator"]) == list(Do.state_dict())
    assert [float(s["step"]) for s in sd["optimizer_discriminator"]["state"].values()] == [6.0] * 8
    assert float(tr.discriminator.flat.data.abs().max()) <= 0.01 + 2 * 3 * 4e-4      # the clamp reaches the biases too
    tr2 = P.Trainer(_network(), _plugins(), checkpoints=str(tmp_path / "gan2"), sample_size=16, epochs=1, devices=[0],
                    recon=str(tmp_path / "img2"), nrow=4)
    tr2.load_model(load_path=ck + "0.model")
    assert tr2.start_epoch == 1

    def state(t):
        out = {}
        for name in ("generator", "discriminator", "optimizer_generator", "optimizer_discriminator"):
            sdict = getattr(t, name).state_dict()
            if "state" in sdict:
                for i, s in sdict["state"].items():
                    for k, v in s.items():
                        out["%s.%s.%s" % (name, i, k)] = v.detach().cpu().clone() if torch.is_tensor(v) else torch.tensor(float(v))
            else:
                for k, v in sdict.items():
                    out[name + "." + k] = v.detach().cpu().clone()
        return out
    sa, sb = state(tr), state(tr2)
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    batch = R.synthetic_images(8, 32, seed=6).cuda()
    vals = []
    for t in (tr, tr2):
        t.batch_size = 8
        for name in t.model_names:
            getattr(t, name).train()
        t._store_loss_maps()
        t.real_inputs = batch
        torch.manual_seed(123)
        t.train_iter()
        vals.append([t.loss_logs[k][-1] for k in t.loss_logs])
    assert vals[0] == vals[1] and all(np.isfinite(v) for v in vals[0])
    sa, sb = state(tr), state(tr2)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_cli_critic_batchnorm_flag(tmp_path):
    """Two synthetic steps through the CLI with --critic_batchnorm 0 at 32 x 32: completion, a discriminator checkpoint without
    BatchNorm keys and with biases, finite weights."""
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"path_csv": ["synthetic"], "patch_data_path": ["synthetic"], "img_size": 32, "rna_features": 64,
                               "flag": "critic_plain"}))
    cmd = [sys.executable, os.path.join(REPO, "histopathology_gan.py"), "--config", str(cfg), "--gan_type", "dcgan", "--loss_type",
           "wgan", "--synthetic", "--critic_batchnorm", "0", "--num_epochs", "1", "--steps_per_epoch", "2", "--model_dir",
           str(tmp_path / "model"), "--image_dir", str(tmp_path / "img")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training of the Model is Complete" in r.stdout
    files = sorted(str(p) for p in tmp_path.glob("model*") if str(p).endswith(".model"))
    assert files, "no checkpoint written"
    ck = torch.load(files[0], map_location="cpu", weights_only=False)
    keys = list(ck["discriminator"])
    assert keys == ["model.0.0.weight", "model.0.0.bias", "model.1.0.weight", "model.1.0.bias", "model.2.0.weight",
                    "model.2.0.bias", "disc.0.weight", "disc.0.bias"]
    assert all(bool(torch.isfinite(v).all()) for v in ck["discriminator"].values())
    assert all(len(v) == 2 and all(np.isfinite(x) for x in v) for v in ck["loss_logs"].values())


# ---- data parallel, world 2 over gloo on one device: the generic flat-gradient all-reduce.  The optimizers' learning rate is
# zero, so the weights stay the initial ones and the all-reduced gradient of each step can be compared with gradients the test
# process forms from the same weights.
WORKER = r'''
import os, sys, torch, torch.nn as nn
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import torch.distributed as dist
from rna_gan_amd import dist as D_, losses as PL
from oracle import ref_cpu as R
import test_critic_plain_train_gpu as T
rank = int(os.environ["RANK"])
torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
D_.init_from_env(backend="gloo")
assert D_.world_size() == 2 and D_.active()
G0, D0 = T.oracle_pair(0)
G, D, og, od = T.product_pair("fp32", G0, D0, lr_d=0.0)
ld, lp = PL.WassersteinDiscriminatorLoss(), PL.WassersteinGradientPenalty()
real, nz, eps = T.dp_shard(rank)
out = {}
out["loss_d"] = ld.step(G, D, od, real.cuda(), nz[0].cuda()).item()
PL.flush(); torch.cuda.synchronize()
out["grad_d"] = {k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()}
out["loss_gp"] = lp.step(G, D, od, real.cuda(), nz[1].cuda(), torch.tensor([eps], device="cuda")).item()
PL.flush(); torch.cuda.synchronize()
out["grad_gp"] = {k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()}
out["D"] = {k: v.cpu() for k, v in D.state_dict().items()}
torch.save(out, os.environ["OUT"] + str(rank))
dist.barrier()
dist.destroy_process_group()
'''


def dp_shard(rank, n=8):
    return (R.synthetic_images(n, IN_SIZE, seed=300 + rank), [R.synthetic_normal(n, ENC, seed=400 + 2 * rank + j) for j in range(2)],
            0.2 + 0.5 * rank)


def test_world2_allreduced_gradients_are_the_shard_mean(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "dp2_rank")
    procs = []
    for rank in range(2):
        env = dict(os.environ, REPO=REPO, OUT=out, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK="0",
                   WORLD_SIZE="2", RNAGAN_FORCE_DP="0")
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    # meanwhile: each shard's single-process gradients from the same (initial) weights
    G0, D0 = oracle_pair(0)
    G, D, og, od = product_pair("fp32", G0, D0, lr_d=0.0)
    single = {"grad_d": [], "grad_gp": []}
    for rank in range(2):
        real, nz, eps = dp_shard(rank)
        PL._d_step(G, D, od, real.cuda(), nz[0].cuda(), None)
        single["grad_d"].append({k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()})
        PL._gp_step(G, D, od, real.cuda(), nz[1].cuda(), eps, 10.0)
        single["grad_gp"].append({k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()})
    assert all(torch.equal(v.cpu(), D0.state_dict()[k]) for k, v in D.state_dict().items())      # lr = 0: nothing moved
    for p in procs:
        try:
            _, err = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err[-3000:]
    res = [torch.load(out + str(r)) for r in range(2)]
    for step in ("grad_d", "grad_gp"):
        for k in res[0][step]:
            assert torch.equal(res[0][step][k], res[1][step][k]), (step, k)              # both ranks hold the same reduced gradient
            mean = (single[step][0][k].double() + single[step][1][k].double()) / 2
            got = res[0][step][k].double()
            if step == "grad_gp" and k.endswith("bias"):
                assert bool((got == 0).all()) and bool((mean == 0).all()), k
                continue
            # fp32 sums of up to 2 x 8 x 16 x 16 = 4096 terms in another order (the rank-local pass pairs the two halves'
            # weight gradients, the single process runs one double batch): sqrt(K) eps = 4e-6 typical, K eps = 2.4e-4 worst
            d = float((got - mean).abs().max() / (mean.abs().max() + 1e-30))
            print("%s %s: %.2e" % (step, k, d))
            assert d <= 1e-4, (step, k, d)
    assert all(torch.equal(res[0]["D"][k], res[1]["D"][k]) for k in res[0]["D"])
