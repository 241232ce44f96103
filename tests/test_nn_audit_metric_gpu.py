"""The memorisation audit end to end on the device (rna_gan_amd.metrics.Memorisation -> export.tiles_u8 -> nearest.audit ->
rg_tile_descriptor_i8 / rg_nn_topk_i8): a stub generator whose prescribed output decodes to known bytes, audited against 256 training
tiles; every integer EQUAL to the numpy restatement of tests/nn_audit_refs.py and to the CPU-tensor path on the same inputs.

What must not be flagged is built to be farther from the training set than training tiles are from each other (a sample of the
training distribution itself is flagged about half of the time -- nearest.audit).  With factor 4 a descriptor has 192 block means of
16 bytes.  Training bytes are uniform in [64, 192): two training tiles differ by about 192 * 2 * 1365 / 16 = 32 800, the nearest of
255 by about 23 000.  Fresh tiles are uniform in [0, 256): 192 * (5461 + 1365) / 16 = 81 900 to a training tile, the nearest of 256
above 55 000.  Training tile 11 carries a left / right step of +-60 that survives the block means, so its quarter turn is at least
192 * 3 600 farther from every tile; a +-1 byte copy is within 192 of its source."""
import pickle

import numpy as np
import pytest
import torch

import nn_audit_refs as R

pytestmark = pytest.mark.gpu
CUDA = torch.device("cuda:0")
SOURCES = [7, 11, 100, 200, 255]            # the copied training tiles; the copy of 11 is turned by 90 degrees
FRESH = 6


class _Prescribed(torch.nn.Module):
    """generator(z): image number z[i, 0] of a fixed list, as fp32 in [-1, 1] that the export decodes to the given bytes"""

    def __init__(self, tiles_u8):
        super().__init__()
        self.encoding_dims = 1
        self.register_buffer("images", torch.from_numpy(tiles_u8).float() / 255.0 * 2.0 - 1.0)

    def forward(self, z):
        return self.images[z[:, 0].long()].contiguous()


def _build():
    rng = np.random.default_rng(77)
    train = rng.integers(64, 192, size=(256, 3, 32, 32), dtype=np.uint8)
    train[11, :, :, :16] += 60
    train[11, :, :, 16:] -= 60

    def noisy(t):
        return np.clip(t.astype(np.int16) + rng.integers(-1, 2, size=t.shape), 0, 255).astype(np.uint8)
    gen = [noisy(train[s]) for s in SOURCES]
    gen[1] = R.d4(gen[1], 1)
    gen += [rng.integers(0, 256, size=(3, 32, 32), dtype=np.uint8) for _ in range(FRESH)]
    held = rng.integers(64, 192, size=(9, 3, 32, 32), dtype=np.uint8)
    return train, np.stack(gen), held


@pytest.fixture(scope="module")
def case():
    train, gen, held = _build()
    want = {d4: R.audit(gen, train, 4, 2, d4, held) for d4 in (False, True)}
    return train, gen, held, want


def _metric(train, gen, held, d4, **kw):
    from rna_gan_amd.metrics import Memorisation
    ids = torch.arange(gen.shape[0], dtype=torch.float32)[:, None]
    return Memorisation(torch.from_numpy(train).to(CUDA), gen.shape[0], factor=4, k=2, d4=d4, heldout=torch.from_numpy(held).to(CUDA),
                        noise=ids, batch_size=4, **kw)                    # 4 + 4 + 3: a ragged last batch


@pytest.mark.parametrize("d4", [True, False])
def test_metric_flags_the_copies_and_equals_the_restatement(case, d4):
    train, gen, held, want = case
    G = _Prescribed(gen).to(CUDA)
    G.train()
    metric = _metric(train, gen, held, d4)
    decoded = torch.cat(metric.generated_tiles(G, CUDA))
    assert decoded.dtype == torch.uint8 and np.array_equal(decoded.cpu().numpy(), gen), "the stub's output does not decode to its bytes"
    value = metric.metric_ops(G, CUDA)
    res, w = metric.last_result, want[d4]
    print("Memorisation d4=%s: %r" % (d4, metric.last))
    for name in ("d2", "index", "loo_d2", "copied", "exact"):
        assert np.array_equal(getattr(res, name), w[name]), name
    assert value == res.copy_rate == w["copy_rate"] and res.closer_than_heldout == w["closer_than_heldout"]
    flagged = [True, d4, True, True, True] + [False] * FRESH
    assert res.copied.tolist() == flagged and value == sum(flagged) / len(flagged)
    matched = res.index[:5, 0].tolist()
    assert matched == SOURCES if d4 else (matched[0], matched[2:]) == (SOURCES[0], SOURCES[2:])
    assert (res.d2[[0, 2, 3, 4], 0] <= 192).all() and (res.d2[5:, 0] > 40000).all() and not res.exact.any()
    assert metric.history == [metric.last] and set(metric.last) == {"copy_rate", "exact", "min_d2", "median_d2", "closer_than_heldout"}
    assert metric.last["min_d2"] == int(w["d2"][:, 0].min()) and metric.last["median_d2"] == float(np.median(w["d2"][:, 0]))
    assert G.training
    # a second evaluation reuses the index and gives the same numbers
    index = metric._index
    assert metric.metric_ops(G, CUDA) == value and metric._index is index and metric.history == [metric.last] * 2


def test_device_results_equal_the_cpu_tensor_path(case):
    from rna_gan_amd import nearest as NN
    train, gen, held, _ = case
    out = {}
    for dev in ("cpu", CUDA):
        index = NN.TrainIndex(torch.from_numpy(train).to(dev), factor=4, chunk=100)
        assert index.desc.device.type == torch.device(dev).type and tuple(index.desc.shape) == (256, 192)
        out[dev] = (index, NN.audit(torch.from_numpy(gen).to(dev), index, k=4, d4=True, heldout_u8=torch.from_numpy(held).to(dev)))
    assert torch.equal(out["cpu"][0].desc, out[CUDA][0].desc.cpu()) and torch.equal(out["cpu"][0].norm2, out[CUDA][0].norm2.cpu())
    a, b = out["cpu"][1], out[CUDA][1]
    for name in ("d2", "index", "loo_d2", "copied", "exact", "heldout_d2"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.summary() == b.summary()
    d2, ix = NN.nearest(out[CUDA][0], out[CUDA][0], 3, exclude=torch.arange(256))
    cd2, cix = NN.nearest(out["cpu"][0], out["cpu"][0], 3, exclude=torch.arange(256))
    assert d2.device.type == "cuda" and d2.dtype == torch.int64 and torch.equal(d2.cpu(), cd2) and torch.equal(ix.cpu(), cix)


def test_pickle_keeps_history_and_drops_the_index(case):
    train, gen, held, _ = case
    G = _Prescribed(gen).to(CUDA)
    metric = _metric(train, gen, held, True, seed=5)
    value = metric.metric_ops(G, CUDA)
    blob = pickle.dumps(metric)
    assert len(blob) < 16 * 1024
    back = pickle.loads(blob)
    assert (back.n_fake, back.factor, back.k, back.d4, back.seed, back.batch_size) == (len(gen), 4, 2, True, 5, 4)
    assert back.history == metric.history == [metric.last]
    assert back._index is None and back.train_tiles is None and back.heldout is None and back.noise is None and back.last_result is None
    with pytest.raises(RuntimeError):
        back.metric_ops(G, CUDA)
    from rna_gan_amd.resident import DeviceTileSet
    back.set_train(DeviceTileSet.from_tensors(torch.from_numpy(train), device=CUDA))
    back.noise = metric.noise
    assert back.metric_ops(G, CUDA) == value and "closer_than_heldout" not in back.last and len(back.history) == 2
    from rna_gan_amd.metrics import Memorisation
    ts = DeviceTileSet.from_tensors(torch.from_numpy(train), device=CUDA)
    again = Memorisation.from_tile_set(ts, len(gen), factor=4, k=2, d4=True, noise=metric.noise, batch_size=4)
    assert again.metric_ops(G, CUDA) == value


def test_audit_program_writes_the_table_and_the_sheet(tmp_path):
    """audit_memorisation.run in process with the tiny generator of tests/test_metrics_gpu.py (32 x 32 tiles) and a handed-in
    training set: nearest.csv repeats the AuditResult row by row, nearest.png has 16 rows of 1 + k tiles and a gap"""
    from types import SimpleNamespace
    from PIL import Image
    import audit_memorisation as A
    from rna_gan_amd.resident import DeviceTileSet
    from rna_gan_amd.synth import synthetic_tiles_u8
    from test_metrics_gpu import _models
    G, _ = _models(6)
    ts = DeviceTileSet.from_tensors(synthetic_tiles_u8(70, 32, 3), device=CUDA)
    args = A.parse_args(["--synthetic", "--out_dir", str(tmp_path / "o"), "--samples", "20", "--k", "3", "--factor", "2", "--seed", "4"])
    res, paths = A.run(args, trainer=SimpleNamespace(generator=G, device=CUDA), betavae=None, tile_set=ts)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["nearest.csv", "nearest.png"]
    lines = open(paths[0]).read().splitlines()
    assert lines[0] == "generated,index_0,index_1,index_2,d2_0,d2_1,d2_2,loo_d2,copied,exact" and len(lines) == 21
    table = np.array([[int(v) for v in line.split(",")] for line in lines[1:]], dtype=np.int64)
    assert np.array_equal(table[:, 0], np.arange(20)) and np.array_equal(table[:, 1:4], res.index) and np.array_equal(table[:, 4:7], res.d2)
    assert np.array_equal(table[:, 7], res.loo_d2) and np.array_equal(table[:, 8], res.copied) and np.array_equal(table[:, 9], res.exact)
    assert (np.diff(res.d2, axis=1) >= 0).all() and res.index.min() >= 0 and res.index.max() < 70
    assert Image.open(paths[1]).size == (4 * 32 + 2, 16 * 32)
    for bad in (["--out_dir", "o"], ["--synthetic"], ["--synthetic", "--out_dir", "o", "--k", "9"],
                ["--synthetic", "--out_dir", "o", "--factor", "3"]):
        with pytest.raises(SystemExit):
            A.parse_args(bad)


def test_cli_builds_the_metric_and_hands_it_the_resident_set():
    """histopathology_gan.py --resident 1 --mem_samples N: the metric is built before the resident set exists and receives it
    through set_train; its result equals the CPU-tensor path on the same generated bytes and the same tiles"""
    import histopathology_gan as H
    from rna_gan_amd import nearest as NN
    from rna_gan_amd.augment import InputTransform
    from rna_gan_amd.metrics import Memorisation
    from rna_gan_amd.resident import DeviceTileSet
    from test_metrics_gpu import _models
    args = H.parse_args(["--config", "c.json", "--loss_type", "wgan", "--seed", "5", "--resident", "1", "--mem_samples", "8",
                         "--mem_factor", "2", "--mem_d4", "0"])
    ds = H.SyntheticTiles(24, 32, 4, False, 0, as_u8=True)
    m = H.build_mem_metric(args, ds, [], CUDA, {"input_transform": InputTransform(0.5, 0.5)})
    assert isinstance(m, Memorisation) and (m.n_fake, m.factor, m.d4, m.k, m.seed) == (8, 2, False, 1, 5) and m.train_tiles is None
    G, _ = _models(6)
    with pytest.raises(RuntimeError):
        m.metric_ops(G, CUDA)
    ts = DeviceTileSet.from_dataset(ds, CUDA)
    m.set_train(ts)
    value = m.metric_ops(G, CUDA)
    gen = torch.cat(m.generated_tiles(G, CUDA))
    want = NN.audit(gen.cpu(), NN.TrainIndex(ts.tiles.cpu(), factor=2), k=1)
    assert value == want.copy_rate and m.last == want.summary()
    for name in ("d2", "index", "loo_d2", "copied"):
        assert np.array_equal(getattr(m.last_result, name), getattr(want, name)), name
