"""bench.py's own multi-rank launcher (`python bench.py --gpus 2` outside torchrun) end to end on CPU ranks: the parent
starts 2 fresh rank processes, they rendezvous over gloo on 127.0.0.1, run warm-up + timed steps of the toy plug-in
workload (tests/bench_plugin_cpu.py) bracketed by barriers, take the MAX over ranks, and rank 0 prints ONE JSON line
whose n_gpus comes from the live process group."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, env_extra=None, timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True,
                          text=True, timeout=timeout, cwd=ROOT)


def test_gpus2_launcher_runs_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--step-plugin", "tests.bench_plugin_cpu:make"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["ranks"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["collective_backend"] == "gloo"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 8 and out["value"] > 0
    assert abs(out["value"] - 8 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-2 * out["value"]


def test_gpus_mismatch_is_an_error():
    """Launched under a 1-rank environment but asked for 2 GPUs: refuse instead of printing a 1-GPU number under a 2-GPU label."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--step-plugin", "tests.bench_plugin_cpu:make"],
             env_extra={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                        "MASTER_PORT": "29999"})
    assert r.returncode != 0
    assert "process group has 1 rank" in (r.stderr + r.stdout)


def test_failing_rank_fails_the_launch():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--step-plugin", "tests.bench_plugin_cpu:does_not_exist"])
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_plain_run_leaves_the_full_measurements_out(monkeypatch):
    """Without --full a run does only what its headline figure needs: parse_args turns off every leg main() runs behind the
    timed region (the roofline pass and its ceilings, the extras and parity, the CPU baseline).  --full turns them on, the
    --no-* options still leave single legs out of it, and the timed work is configured the same either way."""
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    monkeypatch.delenv("RNAGAN_BENCH_PRECISION", raising=False)
    import bench
    legs = ("no_roofline", "no_ceilings", "no_extras", "no_cpu_baseline")
    argv = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    plain, full = bench.parse_args(argv), bench.parse_args(argv + ["--full"])
    assert not plain.full and all(getattr(plain, k) for k in legs)
    assert full.full and not any(getattr(full, k) for k in legs)
    part = bench.parse_args(argv + ["--full", "--no-extras", "--no-cpu-baseline"])
    assert [k for k in legs if getattr(part, k)] == ["no_extras", "no_cpu_baseline"]
    timed = ("gpus", "steps", "warmup", "batch", "precision", "seed", "gan_type", "api_path", "sync_stats", "dump_outputs")
    assert [getattr(plain, k) for k in timed] == [getattr(full, k) for k in timed]


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the last timed step's loss values (those of the JSON line) and the trained parameters and buffers
    as float .npy files; two runs with the same arguments write the same arrays, and --steps sets how many steps ran."""
    import numpy as np

    def dump(tag, steps):
        d = tmp_path / tag
        r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--step-plugin", "tests.bench_plugin_cpu:make",
                  "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == steps and out["ms_per_step"] > 0
        arrays = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert np.array_equal(arrays["losses"], np.array(out["config"]["losses_last_step"]))
        assert "G.model.0.0.weight" in arrays and "D.disc.0.weight" in arrays
        return arrays

    a, b, c = dump("a", 3), dump("b", 3), dump("c", 2)
    assert sorted(a) == sorted(b) == sorted(c)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["losses"], c["losses"]) and not np.array_equal(a["G.model.0.0.weight"], c["G.model.0.0.weight"])


def test_dump_outputs_samples_large_tensors(tmp_path, monkeypatch):
    """dump_outputs with DUMP_SAMPLE lowered: a tensor above it is written as DUMP_SAMPLE of its elements at ascending,
    distinct positions, the same positions in every call (the values here ARE the positions); a smaller tensor whole, in its
    shape; float64 stays float64, bf16 and fp32 are written as float32; integer buffers are left out."""
    import numpy as np
    import torch
    # importing bench.py sets this variable in os.environ: the test leaves the environment as it found it
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    G, D = torch.nn.Module(), torch.nn.Module()
    G.big = torch.nn.Parameter(torch.arange(1000, dtype=torch.float32).reshape(10, 100))
    G.register_buffer("small", torch.arange(48, dtype=torch.float64).reshape(6, 8))
    D.register_buffer("h16", torch.arange(200).to(torch.bfloat16))          # integers up to 256 are exact in bf16
    D.register_buffer("count", torch.tensor(3))
    info = {"handles": {"G": G, "D": D}}
    losses = [torch.tensor(1.5), torch.tensor([2.5]), torch.tensor(-0.25)]
    dumps = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        bench.dump_outputs(str(d), losses, info)
        dumps.append({f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))})
    a, b = dumps
    assert sorted(a) == ["D.h16", "G.big", "G.small", "losses"]
    assert a["losses"].dtype == np.float32 and a["losses"].tolist() == [1.5, 2.5, -0.25]
    assert a["G.small"].dtype == np.float64 and np.array_equal(a["G.small"], np.arange(48.0).reshape(6, 8))
    for name, numel in (("G.big", 1000), ("D.h16", 200)):
        v = a[name]
        assert v.dtype == np.float32 and v.shape == (64,)
        assert np.all(np.diff(v) > 0) and v[0] >= 0 and v[-1] < numel and np.array_equal(v, np.round(v))
        assert v[-1] >= 64                                  # spread over the tensor, not its first elements
    assert all(np.array_equal(a[k], b[k]) for k in a)
