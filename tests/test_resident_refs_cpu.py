"""The resident training set (rna_gan_amd.resident), checked without a GPU: the refs of tests/resident_refs.py against the
augment_refs functions on a pre-gathered copy, the CPU-device loader bit for bit against the refs, the order and code streams,
the shard rule against the CLI's, the state dict, from_dataset over in-memory tile stores, the binding, the Trainer's
"data_loader" checkpoint key and the CLI flags."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

import rna_gan_amd as P
from rna_gan_amd import _abi
from rna_gan_amd import data as PD
from rna_gan_amd import losses as PL
from rna_gan_amd.augment import InputTransform
from rna_gan_amd.resident import DeviceTileLoader, DeviceTileSet, epoch_order, shard_indices
from augment_refs import normalize_ref, tile_transform_ref
from resident_refs import epoch_order_ref, gather_transform_ref, shard_ref

CPU = torch.device("cpu")
M, C, S, G = 13, 3, 5, 6
_RNG = np.random.default_rng(41)
STORE = _RNG.integers(0, 256, size=(M, C, S, S), dtype=np.uint8)
RNA = _RNG.standard_normal((4, G)).astype(np.float32)
ROW_OF = (np.arange(M) % 4).astype(np.int32)
LABELS = np.arange(M, dtype=np.float32)
for _a in (STORE, RNA, ROW_OF, LABELS):
    _a.setflags(write=False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _set(form="dict"):
    t = torch.from_numpy(STORE.copy())
    if form == "tensor":
        return DeviceTileSet.from_tensors(t, device=CPU)
    if form == "tuple":
        return DeviceTileSet.from_tensors(t, labels=torch.from_numpy(LABELS.copy()), device=CPU)
    return DeviceTileSet.from_tensors(t, rna=torch.from_numpy(RNA.copy()), row_of=torch.from_numpy(ROW_OF.copy()),
                                      labels=torch.from_numpy(LABELS.copy()), device=CPU)


# ------------------------------------------------------------------ the refs
def test_refs_equal_augment_refs_on_a_pregathered_copy():
    index = np.array([3, 3, 0, 12, 7, 1, 12], dtype=np.int32)
    codes = np.array([0, 5, 7, 2, 1, 6, 3], dtype=np.int32)
    pre = STORE[index]
    assert (_bits(gather_transform_ref(STORE, index, codes)) == _bits(tile_transform_ref(pre, codes))).all()
    assert (_bits(gather_transform_ref(STORE, index)) == _bits(normalize_ref(pre))).all()
    assert (_bits(gather_transform_ref(STORE, index, codes, mean=0.25, std=0.125)) ==
            _bits(tile_transform_ref(pre, codes, 0.25, 0.125))).all()
    assert (_bits(gather_transform_ref(STORE, None, n=4)) == _bits(normalize_ref(STORE[:4]))).all()
    wild = np.array([-1, -2 ** 31, M, 2 ** 31 - 1], dtype=np.int64)                   # clamped to the nearest valid tile
    assert (_bits(gather_transform_ref(STORE, wild)) == _bits(normalize_ref(STORE[[0, 0, M - 1, M - 1]]))).all()


def test_order_and_shard_refs():
    for seed, rank, e, m in ((0, 0, 0, 13), (7, 2, 5, 64), (7, 2, 6, 64), (1, 0, 0, 1)):
        got = epoch_order(seed, rank, e, m)
        assert got.dtype == np.int32 and got.tolist() == epoch_order_ref(seed, rank, e, m)
        assert sorted(got.tolist()) == list(range(m))
    assert epoch_order(0, 0, 0, 0).shape == (0,)


# ------------------------------------------------------------------ the loader on the CPU device
@pytest.mark.parametrize("form", ["tensor", "tuple", "dict"])
@pytest.mark.parametrize("augment", ["none", "d4", None])
def test_cpu_loader_equals_the_refs(form, augment):
    tf = None if augment is None else InputTransform(augment=augment, seed=3, rank=1)
    loader = DeviceTileLoader(_set(form), 4, transform=tf, seed=9, rank=1)
    assert len(loader) == 3 and loader.batch_size == 4
    order = epoch_order_ref(9, 1, 0, M)
    for t, batch in enumerate(loader):
        idx = order[4 * t:4 * t + 4]
        image = batch if form == "tensor" else batch[0] if form == "tuple" else batch["image"]
        codes = None
        if augment == "d4":
            codes = tf.last_codes
            assert (codes == tf.codes_for(t, 4)).all() and tf.batches == t + 1
        assert image.dtype == torch.float32 and image.is_contiguous() and tuple(image.shape) == (4, C, S, S)
        assert (_bits(image.numpy()) == _bits(gather_transform_ref(STORE, idx, codes))).all()
        if form == "tuple":
            assert isinstance(batch, list) and len(batch) == 2 and (batch[1].numpy() == LABELS[idx]).all()
        if form == "dict":
            assert sorted(batch) == ["image", "labels", "rna_data"]
            assert (batch["labels"].numpy() == LABELS[idx]).all()
            assert (_bits(batch["rna_data"].numpy()) == _bits(RNA[ROW_OF[idx]])).all()
    assert loader.epoch == 1
    if augment != "d4" and tf is not None:
        assert tf.batches == 0 and tf.last_codes is None


def test_other_mean_and_std_and_the_last_partial_batch():
    tf = InputTransform(mean=0.25, std=0.125, augment="d4", seed=1, rank=0)
    loader = DeviceTileLoader(_set("tensor"), 4, transform=tf, seed=2, rank=0, drop_last=False)
    assert len(loader) == 4
    order = epoch_order_ref(2, 0, 0, M)
    sizes = []
    for t, image in enumerate(loader):
        idx = order[4 * t:4 * t + 4]
        sizes.append(image.shape[0])
        assert len(tf.last_codes) == len(idx)
        assert (_bits(image.numpy()) == _bits(gather_transform_ref(STORE, idx, tf.last_codes, mean=0.25, std=0.125))).all()
    assert sizes == [4, 4, 4, 1]
    with pytest.raises(ValueError):
        DeviceTileLoader(_set("tensor"), 0)


def _epoch_indices(loader):
    """The tile index of every sample of one epoch, recovered from the labels (label m = tile m)."""
    return [int(v) for batch in loader for v in batch[1].tolist()]


def test_epoch_order_is_a_permutation_and_a_pure_function():
    ts = _set("tuple")
    a = DeviceTileLoader(ts, 4, seed=5, rank=2, drop_last=False)
    first, second = _epoch_indices(a), _epoch_indices(a)
    assert sorted(first) == list(range(M)) and sorted(second) == list(range(M))          # every tile once, no repeat
    assert first != second and a.epoch == 2
    assert first == epoch_order_ref(5, 2, 0, M) and second == epoch_order_ref(5, 2, 1, M)
    b = DeviceTileLoader(ts, 4, seed=5, rank=2, drop_last=False)
    assert _epoch_indices(b) == first
    assert _epoch_indices(DeviceTileLoader(ts, 4, seed=5, rank=3, drop_last=False)) != first
    assert _epoch_indices(DeviceTileLoader(ts, 4, seed=6, rank=2, drop_last=False)) != first
    dropped = _epoch_indices(DeviceTileLoader(ts, 4, seed=5, rank=2))
    assert dropped == first[:12] and len(set(dropped)) == 12


# ------------------------------------------------------------------ shards
def test_shards_are_disjoint_equal_and_the_clis_rule():
    import histopathology_gan as H
    for n_items in (0, 7, 64, 101, 1000):
        for batch in (1, 4, 8):
            for world in (1, 2, 3):
                shards = [shard_indices(n_items, r, world, batch) for r in range(world)]
                for r, sh in enumerate(shards):
                    assert sh == shard_ref(n_items, r, world, batch) == H.shard_indices(n_items, r, world, batch)
                    assert len(sh) % batch == 0 and len(sh) == len(shards[0])
                flat = [i for sh in shards for i in sh]
                assert len(set(flat)) == len(flat) and all(0 <= i < n_items for i in flat)
                batches = {len(DeviceTileLoader(DeviceTileSet.from_tensors(
                    torch.zeros(len(sh), 1, 1, 1, dtype=torch.uint8), device=CPU), batch, rank=r))
                    for r, sh in enumerate(shards)}
                assert len(batches) == 1


# ------------------------------------------------------------------ state
def test_state_dict_round_trip_restores_order_and_codes():
    def make():
        tf = InputTransform(augment="d4", seed=8, rank=0)
        return DeviceTileLoader(_set("tuple"), 4, transform=tf, seed=8, rank=0), tf

    whole, wtf = make()
    runs = []
    for _ in range(3):
        epoch = []
        for batch in whole:
            epoch.append((batch[1].tolist(), wtf.last_codes.copy(), batch[0].numpy().copy()))
        runs.append(epoch)
    first, ftf = make()
    for _ in first:
        pass
    state = first.state_dict()
    assert state == {"seed": 8, "epoch": 1, "transform": {"seed": 8, "augment": "d4", "batches": 3}}
    second, stf = make()
    second.seed = 0
    second.load_state_dict(state)
    assert (second.seed, second.epoch, stf.batches) == (8, 1, 3)
    for e in (1, 2):
        for (labels, codes, image), batch in zip(runs[e], second):
            assert batch[1].tolist() == labels and (stf.last_codes == codes).all()
            assert (_bits(batch[0].numpy()) == _bits(image)).all()
    plain = DeviceTileLoader(_set("tensor"), 4, seed=3)
    assert plain.state_dict() == {"seed": 3, "epoch": 0, "transform": None}
    plain.load_state_dict({"seed": 3, "epoch": 4, "transform": None})
    assert plain.epoch == 4


# ------------------------------------------------------------------ from_dataset
def _stores(tmp_slides=("a.svs", "b.svs"), tiles_per_slide=5, garbage=("b.svs", 2)):
    """In-memory slide databases in the reference's record format; one record is garbage."""
    import pandas as pd
    rng = np.random.default_rng(17)
    stores, rows = {}, []
    for k, wsi in enumerate(tmp_slides):
        st = {b"__keys__": PD.encode_keys(tiles_per_slide)}
        for i in range(tiles_per_slide):
            tile = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
            st[str(i).encode("ascii")] = PD.encode_record("%s_patch_%d" % (wsi, i), tile)
        if wsi == garbage[0]:
            st[str(garbage[1]).encode("ascii")] = b"not an lz4 frame"
        stores[os.path.join("root", wsi, wsi.replace(".svs", ".db"))] = st
        rows.append({"wsi_file_name": wsi, "rna_a": float(k) + 0.5, "rna_b": -float(k), "rna_c": 3.0,
                     "patch_data_path": "root", "labels": k})
    return stores, pd.DataFrame(rows)


def test_from_dataset_drops_the_garbage_record_and_keeps_every_byte():
    stores, table = _stores()
    ds = PD.PatchRNADataset("root", table, 8, transforms=None, stores=stores)
    assert len(ds) == 10
    ts = DeviceTileSet.from_dataset(ds, CPU, chunk=4)
    assert len(ts) == 9 and ts.dropped == 1 and ts.form == "dict"
    assert ts.tiles.dtype == torch.uint8 and tuple(ts.tiles.shape) == (9, 3, 8, 8)
    assert tuple(ts.rna.shape) == (2, 3) and ts.row_of.dtype == torch.int32 and ts.labels.dtype == torch.float32   # one row per slide
    assert ts.nbytes == 9 * 192 + 2 * 3 * 4 + 9 * 4 + 9 * 4 and ts.build_seconds >= 0
    m = 0
    for i in range(len(ds)):
        image = PD.decompress_and_deserialize(stores[ds.lmdbs_path[i]][ds.keys[i]])
        if image is None:
            continue
        assert torch.equal(ts.tiles[m], image)
        assert torch.equal(ts.rna[ts.row_of[m].long()], ds.rna_data_arrays[i])
        assert torch.equal(ts.labels[m], ds.labels[i])
        m += 1
    assert m == 9
    # a rank's shard: the same records, in the order of the list
    # (the dataset draws its per-slide tile order from the global `random`: where the garbage record sits differs from run to run)
    readable = [i for i in range(len(ds)) if PD.decompress_and_deserialize(stores[ds.lmdbs_path[i]][ds.keys[i]]) is not None]
    unreadable = [i for i in range(len(ds)) if i not in readable]
    items = [readable[8], readable[1], readable[4]]
    sub = DeviceTileSet.from_dataset(ds, CPU, items=items, chunk=2)
    assert len(sub) == 3 and sub.dropped == 0
    assert DeviceTileSet.from_dataset(ds, CPU, items=unreadable + items, chunk=2).dropped == 1
    for m, i in enumerate(items):
        assert torch.equal(sub.tiles[m], PD.decompress_and_deserialize(stores[ds.lmdbs_path[i]][ds.keys[i]]))
        assert torch.equal(sub.rna[sub.row_of[m].long()], ds.rna_data_arrays[i])
    # every batch of the loader is full
    assert [b["image"].shape[0] for b in DeviceTileLoader(ts, 4, rank=0)] == [4, 4]
    # PatchDataset: (image, label) items
    pd_set = DeviceTileSet.from_dataset(PD.PatchDataset("root", table, 8, transforms=None, stores=stores), CPU)
    assert pd_set.form == "tuple" and len(pd_set) == 9 and pd_set.rna is None and pd_set.dropped == 1


def test_from_dataset_over_synthetic_tiles():
    import histopathology_gan as H
    for with_rna in (True, False):
        ds = H.SyntheticTiles(20, 8, 5, with_rna, 3, as_u8=True)
        ts = DeviceTileSet.from_dataset(ds, CPU, chunk=7)
        assert len(ts) == 20 and ts.dropped == 0 and ts.form == ("dict" if with_rna else "tuple")
        for i in range(20):
            item = ds[i]
            assert torch.equal(ts.tiles[i], item["image"] if with_rna else item[0])
            if with_rna:
                assert torch.equal(ts.rna[ts.row_of[i].long()], item["rna_data"])
        if with_rna:
            assert ts.rna.shape[0] == 16                                     # the 16 distinct rows, once each


class _Counting(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items, self.reads = items, 0

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.reads += 1
        return self.items[i]


def test_budget_refusal_raises_before_any_upload(monkeypatch):
    ds = _Counting([torch.zeros(3, 8, 8, dtype=torch.uint8) for _ in range(10)])
    uploads = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (uploads.append(a) if k.get("dtype") == torch.uint8 else None,
                                                         real_empty(*a, **k))[1])     # the tile tensor's allocation
    with pytest.raises(MemoryError, match=r"1920 bytes.*budget is 1919 bytes.*--num_patches"):
        DeviceTileSet.from_dataset(ds, CPU, chunk=4, max_bytes=1919)
    assert uploads == [] and ds.reads <= 4                                   # refused inside the first chunk, nothing allocated
    assert len(DeviceTileSet.from_dataset(ds, CPU, chunk=4, max_bytes=1920)) == 10
    assert uploads == [((10, 3, 8, 8),)]                                     # (the probe does see the allocation of a set that fits)


def test_refused_tiles():
    good = torch.zeros(3, 8, 8, dtype=torch.uint8)
    for bad in (torch.zeros(3, 8, 8), torch.zeros(3, 8, 8, dtype=torch.int32), torch.zeros(8, 8, dtype=torch.uint8),
                torch.zeros(3, 8, 4, dtype=torch.uint8), torch.zeros(1, 3, 8, 8, dtype=torch.uint8),
                torch.zeros(3, 4, 4, dtype=torch.uint8), np.zeros((3, 8, 8), dtype=np.uint8)):
        with pytest.raises(ValueError):
            DeviceTileSet.from_dataset(_Counting([good, bad]), CPU)
    with pytest.raises(ValueError):
        DeviceTileSet.from_dataset(_Counting([None, None]), CPU)             # no readable tile at all
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(2, 3, 8, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            DeviceTileSet.from_tensors(bad, device=CPU)
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError):
        DeviceTileSet.from_tensors(u8, rna=torch.zeros(3, 4), device=CPU)                     # no row map, not one row per tile
    with pytest.raises(ValueError):
        DeviceTileSet.from_tensors(u8, rna=torch.zeros(1, 4), row_of=torch.tensor([0, 1]), device=CPU)   # outside the table
    with pytest.raises(ValueError):
        DeviceTileSet.from_tensors(u8, labels=torch.zeros(3), device=CPU)


# ------------------------------------------------------------------ the binding
def test_abi_carries_the_symbol():
    import ctypes
    p, i, f = _abi._p, _abi._i, _abi._f
    assert _abi.PROTOTYPES["rg_tile_gather_transform"] == (i, [p, ctypes.c_longlong, p, p, i, i, i, p, f, f, p])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnagan_hip.h")).read()
    assert "int rg_tile_gather_transform(const uint8_t* store, long long M, const int* index, float* dst, int N, int C, int S," \
        in header
    assert _abi.ABI_VERSION == 618
    from rna_gan_amd import build
    assert "rg_augment.hip" in build.SOURCES and "rg_augment.hip" not in build.BF16_ONLY
    assert hasattr(_abi.load(), "rg_tile_gather_transform") and hasattr(_abi.load("f16"), "rg_tile_gather_transform")


# ------------------------------------------------------------------ the Trainer
SEEN = []


class _Record(PL.DiscriminatorLoss):
    def train_ops(self, real_inputs):
        image = real_inputs["image"] if isinstance(real_inputs, dict) else real_inputs
        SEEN.append(image.detach().numpy().copy())
        return 0.0


def _trainer(tmp_path, tag, epochs=1, **kw):
    net = {
        "generator": {"name": P.DCGANGenerator,
                      "args": dict(encoding_dims=16, out_size=32, out_channels=3, step_channels=4,
                                   nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh()),
                      "optimizer": {"name": torch.optim.Adam, "args": {"lr": 1e-4, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": dict(in_size=32, in_channels=3, step_channels=4,
                                       nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2)),
                          "optimizer": {"name": torch.optim.Adam, "args": {"lr": 4e-4, "betas": (0.5, 0.999)}}}}
    return P.Trainer(net, [_Record()], device=CPU, checkpoints=str(tmp_path / tag), recon=None, epochs=epochs,
                     test_noise=torch.zeros(1, 16), **kw)


def test_trainer_writes_and_reads_the_data_loader_key(tmp_path):
    def loader():
        tf = InputTransform(augment="d4", seed=4, rank=0)
        return DeviceTileLoader(_set("dict"), 4, transform=tf, seed=4, rank=0), tf

    del SEEN[:]
    whole, _ = loader()
    _trainer(tmp_path, "whole", epochs=2)(whole)
    want = list(SEEN)
    assert len(want) == 6
    del SEEN[:]
    first, _ = loader()
    _trainer(tmp_path, "first", epochs=1)(first)
    ck = torch.load(str(tmp_path / "first0.model"), map_location="cpu", weights_only=False)
    assert ck["data_loader"] == {"seed": 4, "epoch": 1, "transform": {"seed": 4, "augment": "d4", "batches": 3}}
    assert "input_transform" not in ck
    second, tf = loader()
    tr = _trainer(tmp_path, "second", epochs=2)
    tr.load_model(load_path=str(tmp_path / "first0.model"))
    assert second.epoch == 0                                  # stashed: applied by train() to the loader it is given
    del SEEN[:]
    tr(second)
    assert second.epoch == 2 and tf.batches == 6 and len(SEEN) == 3
    for a, b in zip(want[3:], SEEN):
        assert (_bits(a) == _bits(b)).all()
    # a plain DataLoader writes no key, and a checkpoint without the key loads into a run with a resident loader
    plain = _trainer(tmp_path, "plain")
    plain(DataLoader(torch.from_numpy(normalize_ref(STORE[:8])), batch_size=4))
    ck = torch.load(str(tmp_path / "plain0.model"), map_location="cpu", weights_only=False)
    assert "data_loader" not in ck
    third, _ = loader()
    tr = _trainer(tmp_path, "third", epochs=2)
    tr.load_model(load_path=str(tmp_path / "plain0.model"))
    del SEEN[:]
    tr(third)
    assert len(SEEN) == 3 and (_bits(SEEN[0]) == _bits(want[0])).all()       # no key: the streams start at 0
    # ... and a checkpoint WITH the key loads into a run with a plain DataLoader, which ignores it
    tr = _trainer(tmp_path, "fourth", epochs=2)
    tr.load_model(load_path=str(tmp_path / "first0.model"))
    tr(DataLoader(torch.from_numpy(normalize_ref(STORE[:8])), batch_size=4))
    assert "data_loader" not in torch.load(str(tmp_path / "fourth0.model"), map_location="cpu", weights_only=False)


def test_trainer_refuses_a_second_transform(tmp_path):
    tr = _trainer(tmp_path, "twice", input_transform=InputTransform(augment="d4"))
    with pytest.raises(ValueError, match="second time"):
        tr(DeviceTileLoader(_set("tensor"), 4, transform=InputTransform(augment="d4"), rank=0))
    with pytest.raises(ValueError, match="second time"):
        tr(DeviceTileLoader(_set("tensor"), 4, rank=0))


# ------------------------------------------------------------------ the CLI
def test_cli_flags(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json"]
    a = H.parse_args(base)
    assert (a.resident, a.resident_max_gb) == (0, 0.0)
    a = H.parse_args(base + ["--resident", "1", "--resident_max_gb", "40.5", "--augment", "d4"])
    assert (a.resident, a.resident_max_gb, a.augment, a.device_transform) == (1, 40.5, "d4", 0)
    for bad in (["--resident", "2"], ["--resident", "-1"], ["--resident", "yes"], ["--resident_max_gb", "-1"],
                ["--resident_max_gb", "lots"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()
