"""The input transform, checked without a GPU: the index table of tests/augment_refs.py against np.rot90 / flips and as a group,
the fp32 normalisation against the host transforms on every byte value, rna_gan_amd.augment.InputTransform on the CPU device
bit for bit against the refs, its counter-based code stream and state dict, the Trainer's batch hook, and the CLI flags."""
import numpy as np
import pytest
import torch

from rna_gan_amd import _abi
from rna_gan_amd import data as PD
from rna_gan_amd.augment import InputTransform, d4_apply
from augment_refs import SOURCE_INDEX, asymmetric_tile, d4_index_ref, d4_plane_ref, normalize_ref, tile_transform_ref

CPU = torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the table
def test_table_is_flip_then_rot90():
    x = asymmetric_tile(5)
    for code in range(8):
        r, f = code & 3, code >> 2
        want = np.rot90(x[..., ::-1] if f else x, r, axes=(-2, -1))
        assert (d4_plane_ref(x, code) == want).all(), code
        assert (d4_apply(torch.from_numpy(x), code).numpy() == want).all(), code
        rows, cols = d4_index_ref(5, code)
        assert (x[rows, cols] == want).all(), code


def test_eight_results_are_pairwise_distinct():
    x = asymmetric_tile(5)
    res = [d4_plane_ref(x, c) for c in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert (res[a] != res[b]).any(), (a, b)


def test_codes_form_a_group():
    x = asymmetric_tile(5)
    res = [d4_plane_ref(x, c) for c in range(8)]

    def which(y):
        hit = [c for c in range(8) if (res[c] == y).all()]
        assert len(hit) == 1
        return hit[0]
    table = [[which(d4_plane_ref(res[a], b)) for b in range(8)] for a in range(8)]      # a, then b
    for a in range(8):
        assert sorted(table[a]) == list(range(8))            # closed, and a row of the table is a permutation
        assert 0 in table[a]                                 # an inverse among the eight
        assert table[a][0] == a and table[0][a] == a         # code 0 is the identity
    assert table[1][1] == 2 and table[1][3] == 0 and table[4][4] == 0


def test_codes_use_the_low_three_bits():
    x = asymmetric_tile(5)
    for code, low in ((-1, 7), (11, 3), (1 << 20, 0), (8, 0)):
        assert (d4_plane_ref(x, code) == d4_plane_ref(x, low)).all()
    assert sorted(SOURCE_INDEX) == list(range(8))


# ------------------------------------------------------------------ the normalisation
def test_normalisation_is_the_host_transform_on_every_byte():
    b = np.arange(256, dtype=np.uint8)
    want = normalize_ref(b)
    t = torch.from_numpy(b)
    assert (_bits(PD.ToFloatNormalize(0.5, 0.5)(t).numpy()) == _bits(want)).all()
    assert (_bits(((t.float() / 255.0 - 0.5) / 0.5).numpy()) == _bits(want)).all()
    assert (_bits(((t.float() / 255.0 - 0.25) / 0.125).numpy()) == _bits(normalize_ref(b, 0.25, 0.125))).all()
    assert want[0] == -1.0 and want[255] == 1.0


# ------------------------------------------------------------------ InputTransform on the CPU device
def _batch(N, C, S, dtype, seed=0):
    rng = np.random.default_rng([seed, N, C, S])
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(N, C, S, S), dtype=np.uint8)
    return rng.standard_normal((N, C, S, S)).astype(np.float32)


@pytest.mark.parametrize("S", [1, 5, 16])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_cpu_transform_equals_the_refs(S, dtype):
    src = _batch(11, 3, S, dtype)
    tf = InputTransform(augment="d4", seed=3, rank=0)
    got = tf(torch.from_numpy(src), CPU)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == src.shape
    assert tf.last_codes.shape == (11,) and tf.batches == 1
    assert (_bits(got.numpy()) == _bits(tile_transform_ref(src, tf.last_codes))).all()
    plain = InputTransform(augment="none")
    if dtype == np.uint8:
        assert (_bits(plain(torch.from_numpy(src), CPU).numpy()) == _bits(tile_transform_ref(src))).all()
    assert (_bits(tf.normalize(torch.from_numpy(src), CPU).numpy()) == _bits(tile_transform_ref(src))).all()
    assert tf.batches == 1                                   # normalize() consumes no draw


def test_other_mean_and_std():
    src = _batch(4, 1, 5, np.uint8)
    tf = InputTransform(mean=0.25, std=0.125, augment="d4", seed=1, rank=0)
    got = tf(torch.from_numpy(src), CPU)
    assert (_bits(got.numpy()) == _bits(tile_transform_ref(src, tf.last_codes, 0.25, 0.125))).all()


def test_code_stream_is_counter_based():
    a, b = InputTransform(augment="d4", seed=7, rank=2), InputTransform(augment="d4", seed=7, rank=2)
    x = torch.zeros(16, 1, 2, 2)
    for t in range(3):
        a(x, CPU)
        b(x, CPU)
        assert (a.last_codes == b.last_codes).all()
        assert (a.last_codes == np.random.default_rng([7, 2, t]).integers(0, 8, size=16)).all()
        assert (a.last_codes == a.codes_for(t, 16)).all()
    assert a.last_codes.dtype == np.int32
    other_rank = InputTransform(augment="d4", seed=7, rank=3)
    other_seed = InputTransform(augment="d4", seed=8, rank=2)
    big = torch.zeros(256, 1, 1, 1)
    streams = []
    for tf in (InputTransform(augment="d4", seed=7, rank=2), other_rank, other_seed):
        tf(big, CPU)
        streams.append(tf.last_codes.copy())
        assert sorted(set(streams[-1].tolist())) == list(range(8))          # all eight codes within 256 draws
    assert (streams[0] != streams[1]).any() and (streams[0] != streams[2]).any() and (streams[1] != streams[2]).any()


def test_rank_defaults_to_the_process_rank():
    assert InputTransform().rank == 0 and InputTransform(rank=5).rank == 5


def test_none_draws_nothing_and_returns_the_tensor_itself():
    tf = InputTransform(augment="none", seed=1)
    x = torch.randn(3, 2, 4, 4)
    assert tf(x, CPU) is x
    assert tf.normalize(x, CPU) is x
    assert tf.batches == 0 and tf.last_codes is None
    assert tf.state_dict() == {"seed": 1, "augment": "none", "batches": 0}


def test_state_dict_round_trip_continues_the_stream():
    x = torch.zeros(9, 1, 3, 3)
    whole = InputTransform(augment="d4", seed=5, rank=1)
    want = []
    for _ in range(5):
        whole(x, CPU)
        want.append(whole.last_codes.copy())
    first = InputTransform(augment="d4", seed=5, rank=1)
    for _ in range(2):
        first(x, CPU)
    state = first.state_dict()
    assert state == {"seed": 5, "augment": "d4", "batches": 2}
    second = InputTransform(augment="d4", seed=5, rank=1)
    second.load_state_dict(state)
    for t in range(2, 5):
        second(x, CPU)
        assert (second.last_codes == want[t]).all()


def test_value_errors():
    tf = InputTransform(augment="d4")
    for bad in (torch.zeros(2, 3, 4, 5), torch.zeros(3, 4, 4), torch.zeros(1, 2, 3, 4, 4),
                torch.zeros(2, 3, 4, 4, dtype=torch.float64), torch.zeros(2, 3, 4, 4, dtype=torch.int32),
                torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            tf(bad, CPU)
        with pytest.raises(ValueError):
            tf.normalize(bad, CPU)
    assert tf.batches == 0                                   # a refused batch draws nothing
    with pytest.raises(ValueError):
        InputTransform(augment="rot")
    with pytest.raises(ValueError):
        InputTransform(std=0.0)


# ------------------------------------------------------------------ the binding
def test_abi_carries_the_symbol():
    import os
    p, i, f = _abi._p, _abi._i, _abi._f
    assert _abi.PROTOTYPES["rg_tile_transform"] == (i, [p, i, p, i, i, i, p, f, f, p])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "rg_tile_transform(" in open(os.path.join(root, "include", "rnagan_hip.h")).read()
    from rna_gan_amd import build
    assert "rg_augment.hip" in build.SOURCES and "rg_augment.hip" not in build.BF16_ONLY


def test_a_library_without_a_bound_symbol_is_refused(monkeypatch):
    """rg_tile_transform was added under the ABI number of the parent: what refuses a library built before it is the symbol check
    of _abi.load, shown here with a name no library exports."""
    monkeypatch.setattr(_abi, "_libs", {})
    monkeypatch.setitem(_abi.PROTOTYPES, "rg_no_such_entry_point", (_abi._i, []))
    with pytest.raises(RuntimeError, match="rg_no_such_entry_point missing"):
        _abi.load()


# ------------------------------------------------------------------ the Trainer's batch hook (no model is needed for it)
def _bare_trainer(tf):
    import rna_gan_amd as P
    t = P.Trainer.__new__(P.Trainer)
    t.device, t.input_transform = CPU, tf
    return t


def test_trainer_hook_replaces_the_image_of_every_batch_form():
    u8 = torch.from_numpy(_batch(4, 3, 5, np.uint8))
    labels = torch.arange(4.0)
    rna = torch.randn(4, 6)
    want = torch.from_numpy(tile_transform_ref(u8.numpy()))
    t = _bare_trainer(InputTransform(augment="none"))
    pair = (u8, labels)
    out = t._transform_batch(pair)
    assert torch.equal(out[0], want) and out[1] is labels and pair[0] is u8
    lst = [u8, labels]
    out = t._transform_batch(lst)
    assert torch.equal(out[0], want) and lst[0] is u8 and out is not lst
    assert torch.equal(t._transform_batch(u8), want)
    d = {"image": u8, "rna_data": rna, "labels": labels}
    out = t._transform_batch(d)
    assert out is not d and d["image"] is u8 and sorted(out) == sorted(d)
    assert torch.equal(out["image"], want) and out["rna_data"] is rna and out["labels"] is labels
    t = _bare_trainer(InputTransform(augment="d4", seed=2, rank=0))
    out = t._transform_batch(d)
    assert (_bits(out["image"].numpy()) == _bits(tile_transform_ref(u8.numpy(), t.input_transform.last_codes))).all()


# ------------------------------------------------------------------ the CLI
def test_cli_flags(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json"]
    a = H.parse_args(base)
    assert (a.device_transform, a.augment) == (0, "none")
    a = H.parse_args(base + ["--device_transform", "1", "--augment", "d4"])
    assert (a.device_transform, a.augment) == (1, "d4")
    assert H.parse_args(base + ["--augment", "d4"]).device_transform == 0
    for bad in (["--device_transform", "2"], ["--device_transform", "-1"], ["--device_transform", "yes"], ["--augment", "flip"],
                ["--augment", "D4"], ["--augment", ""]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()


def test_synthetic_tiles_as_uint8_are_the_same_draws():
    import histopathology_gan as H
    for with_rna in (False, True):
        f32 = H.SyntheticTiles(4, 8, 5, with_rna, 3)
        u8 = H.SyntheticTiles(4, 8, 5, with_rna, 3, as_u8=True)
        for i in range(4):
            a, b = f32[i], u8[i]
            a, b = (a["image"], b["image"]) if with_rna else (a[0], b[0])
            assert b.dtype == torch.uint8 and a.dtype == torch.float32
            assert (_bits(a.numpy()) == _bits(normalize_ref(b.numpy()))).all()


def test_cli_metric_set_is_normalised_and_unaugmented():
    import histopathology_gan as H
    args = H.parse_args(["--config", "c.json", "--fd_samples", "6", "--loss_type", "wgan", "--device_transform", "1",
                         "--augment", "d4"])
    tf = InputTransform(augment="d4", seed=args.seed, rank=0)
    ds = H.SyntheticTiles(8, 8, 4, False, 0, as_u8=True)
    real = H.metric_inputs(args, 6, "--fd_samples", ds, [], CPU, {"input_transform": tf})[0]
    want = torch.stack([H.SyntheticTiles(8, 8, 4, False, 0)[i][0] for i in range(6)])
    assert real.dtype == torch.float32 and torch.equal(real, want)
    assert tf.batches == 0
