"""rna_gan_amd.rna_tables without a GPU: the table pipeline against the reference's own run (tests/golden/f11_vae_tables.npz,
written by tests/golden/make_vae_table_fixtures.py with the real pandas and scikit-learn), bit for bit; the split restatement
against scikit-learn where it is installed; the scaler's file; the loader on a CPU tensor against the plain loops of
tests/rna_table_refs.py; the budget; the binding; the training CLI's argument handling."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from rna_gan_amd import _abi
from rna_gan_amd import rna_tables as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rna_table_refs import batches_ref, epoch_order_ref, rows_gather_ref, split_ref, split_tables_ref  # noqa: E402
from vae_table_cases import GENES, ROWS, SEED, inverse_input, make_tables  # noqa: E402

CPU = torch.device("cpu")
_F11 = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f11(golden_dir):
    """The fixture and this build's pipeline on the same tables, computed once."""
    if not _F11:
        with np.load(os.path.join(golden_dir, "f11_vae_tables.npz")) as z:
            _F11["z"] = {k: z[k] for k in z.files}
        _F11["tables"] = make_tables()
        _F11["got"] = RT.prepare_tables(_F11["tables"], SEED)
    return _F11["z"], _F11["tables"], _F11["got"]


# ------------------------------------------------------------------ the reference's run
def test_split_membership_and_order(golden_dir):
    z, tables, (rows, scaler, indices, parts) = _f11(golden_dir)
    for k in RT.PARTS:
        assert parts[k]["wsi_file_name"].tolist() == z[k + ".wsi"].tolist(), k
    # the indices say the same as the frames, and equal the plain-loop rule
    want = split_tables_ref(ROWS, SEED)
    for i, df in enumerate(tables):
        for k in RT.PARTS:
            assert indices[i][k].tolist() == want[i][k]
    for k in RT.PARTS:
        names = [tables[i]["wsi_file_name"].iloc[j] for i in range(len(tables)) for j in indices[i][k]]
        assert names == z[k + ".wsi"].tolist()
    # every row lands in exactly one part, except the rows the two floors drop (none at these sizes: 23 -> 5 + 18 -> 4 + 14)
    for i, m in enumerate(ROWS):
        got = sorted(sum((indices[i][k].tolist() for k in RT.PARTS), []))
        assert got == list(range(m))


def test_scaler_equals_the_reference(golden_dir):
    z, _tables, (_rows, scaler, _indices, parts) = _f11(golden_dir)
    assert np.array_equal(scaler.mean.view(np.uint64), z["mean"].view(np.uint64))
    assert np.array_equal(scaler.scale.view(np.uint64), z["scale"].view(np.uint64))
    assert scaler.mean.dtype == np.float64 and scaler.scale.dtype == np.float64
    assert scaler.scale[5] == 1.0 and scaler.scale[7] == 1.0          # the constant column, and the one constant in train only
    assert scaler.columns == ["rna_G%d" % j for j in range(GENES)]
    for k in RT.PARTS:
        got = scaler.transform_frame(parts[k])
        assert got.dtype == np.float64
        assert np.array_equal(got.view(np.uint64), z[k + ".values"].view(np.uint64)), k
    assert np.abs(z["test.values"][:, 7]).max() > 0                   # that column does vary outside the train split


def test_rows_are_the_reference_datasets(golden_dir):
    z, _tables, (rows, scaler, _indices, parts) = _f11(golden_dir)
    import pandas as pd
    for k in RT.PARTS:
        assert rows[k].dtype == np.float32 and np.array_equal(_bits(rows[k]), _bits(z[k + ".rows"])), k
        # rna_rows on a frame that already holds the transformed values, as the reference's RNADataset sees it
        df = parts[k].copy()
        cols = RT.rna_columns(df)
        df[cols] = scaler.transform_frame(parts[k])
        assert np.array_equal(_bits(RT.rna_rows(df)), _bits(z[k + ".rows"]))
        ds = RT.RNADataset([df])
        assert len(ds) == df.shape[0] and sorted(ds[0]) == ["rna_data"] and ds[0]["rna_data"].dtype == torch.float32
        assert np.array_equal(_bits(torch.stack([ds[i]["rna_data"] for i in range(len(ds))]).numpy()), _bits(z[k + ".rows"]))
    both = RT.RNADataset([rows["val"], rows["test"]])
    assert np.array_equal(_bits(both.rows.numpy()), _bits(np.concatenate([z["val.rows"], z["test.rows"]])))
    np.random.seed(5)
    quick = RT.RNADataset([pd.DataFrame({"rna_a": np.arange(30.0), "other": 1}), np.arange(40.0).reshape(40, 1)], quick=True)
    assert len(quick) == 20 and len(set(quick.rows[:10, 0].tolist())) == 10 and len(set(quick.rows[10:, 0].tolist())) == 10


def test_inverse_transform_fp32(golden_dir):
    z, _tables, (_rows, scaler, _indices, _parts) = _f11(golden_dir)
    got = scaler.inverse_transform(inverse_input())
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(z["inverse"]))
    y64 = inverse_input().astype(np.float64)
    assert np.array_equal(scaler.inverse_transform(y64), y64 * scaler.scale + scaler.mean)
    with pytest.raises(ValueError):
        scaler.inverse_transform(np.zeros((2, GENES + 1), dtype=np.float32))
    with pytest.raises(RuntimeError):
        RT.RnaScaler().transform(np.zeros((2, GENES)))


def test_log_keeps_zeros_and_nans():
    x = np.array([[0.0, 1.0, np.e, -3.0, np.nan]])
    got = RT.log_rna(x)
    assert got[0, 0] == 0.0 and got[0, 1] == 0.0 and got[0, 2] == 1.0 and got[0, 3] == 0.0 and got[0, 4] == 0.0


@pytest.mark.parametrize("m", [5, 10, 11, 37, 100, 503])
def test_split_rule_is_scikit_learns(m):
    ms = pytest.importorskip("sklearn.model_selection")
    np.random.seed(1000 + m)
    a_train, a_test = ms.train_test_split(np.arange(m), test_size=0.2)
    b_train, b_val = ms.train_test_split(a_train, test_size=0.2)
    np.random.seed(1000 + m)
    train, test = RT.split_indices(m)
    tr2, va2 = RT.split_indices(len(train))
    assert test.tolist() == a_test.tolist() and train.tolist() == a_train.tolist()
    assert train[tr2].tolist() == b_train.tolist() and train[va2].tolist() == b_val.tolist()
    np.random.seed(1000 + m)
    r_train, r_test = split_ref(m)
    assert r_train == a_train.tolist() and r_test == a_test.tolist()


def test_split_needs_rows():
    with pytest.raises(ValueError):
        RT.split_indices(1)


def test_scaler_round_trip(tmp_path, golden_dir):
    _z, _tables, (_rows, scaler, _indices, _parts) = _f11(golden_dir)
    path = str(tmp_path / "scaler.npz")
    scaler.save(path)
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["columns", "mean", "scale"]
    back = RT.RnaScaler.load(path)
    assert np.array_equal(back.mean.view(np.uint64), scaler.mean.view(np.uint64))
    assert np.array_equal(back.scale.view(np.uint64), scaler.scale.view(np.uint64))
    assert back.columns == scaler.columns
    import pandas as pd
    with pytest.raises(ValueError):
        back.transform_frame(pd.DataFrame({"rna_other%d" % j: [1.0] for j in range(GENES)}))
    with pytest.raises(RuntimeError):
        RT.RnaScaler().save(path)


# ------------------------------------------------------------------ the loader on a CPU tensor
def _table(M=37, F=5):
    return np.random.default_rng([41, M, F]).normal(size=(M, F)).astype(np.float32)


@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("shuffle", [True, False])
def test_cpu_loader_equals_the_loops(shuffle, drop_last):
    rows = _table()
    ts = RT.RnaTableSet.from_array(rows, CPU)
    items = np.array([36, 3, 4, 4, 9, 0, 11, 12, 13, 30, 31], dtype=np.int64)        # a subset, one row twice
    loader = RT.RnaTableLoader(ts, items, 4, shuffle=shuffle, seed=7, drop_last=drop_last)
    assert len(loader) == (2 if drop_last else 3)
    for epoch in range(3):
        order = epoch_order_ref(7, epoch, items) if shuffle else items.tolist()
        assert sorted(order) == sorted(items.tolist())                               # a permutation of the items
        want = batches_ref(order, 4, drop_last)
        assert loader.epoch == epoch
        got = list(loader)
        assert loader.epoch == epoch + 1 and len(got) == len(want) == len(loader)
        for b, idx in zip(got, want):
            assert sorted(b) == ["rna_data"]
            x = b["rna_data"]
            assert x.dtype == torch.float32 and x.device.type == "cpu" and x.is_contiguous() and tuple(x.shape) == (len(idx), 5)
            assert np.array_equal(_bits(x.numpy()), _bits(rows_gather_ref(rows, 5, idx)))
    if shuffle:
        assert epoch_order_ref(7, 0, items) != epoch_order_ref(7, 1, items)


def test_order_is_a_pure_function_and_uses_no_torch_rng():
    ts = RT.RnaTableSet.from_array(_table(), CPU)
    items = np.arange(5, 30)
    a = RT.RnaTableLoader(ts, items, 8, shuffle=True, seed=3, drop_last=True)
    b = RT.RnaTableLoader(ts, items, 8, shuffle=True, seed=3, drop_last=True)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    np.random.seed(12)
    first = [x["rna_data"].clone() for x in a]
    assert torch.equal(torch.get_rng_state(), before)
    assert np.random.randint(1 << 30) == np.random.RandomState(12).randint(1 << 30)   # numpy's global generator untouched
    np.random.seed(99)
    torch.manual_seed(1)
    again = [x["rna_data"].clone() for x in b]
    assert len(first) == 3 and all(torch.equal(p, q) for p, q in zip(first, again))
    assert a.order_for(1).tolist() == epoch_order_ref(3, 1, items) and a.order_for(1).dtype == np.int32
    c = RT.RnaTableLoader(ts, items, 8, shuffle=True, seed=4, drop_last=True)
    assert c.order_for(0).tolist() != a.order_for(0).tolist()


def test_state_round_trip():
    ts = RT.RnaTableSet.from_array(_table(), CPU)
    a = RT.RnaTableLoader(ts, np.arange(20), 8, shuffle=True, seed=5, drop_last=False)
    list(a); list(a)
    state = a.state_dict()
    assert state == {"seed": 5, "epoch": 2}
    third = [x["rna_data"].clone() for x in a]
    b = RT.RnaTableLoader(ts, np.arange(20), 8, shuffle=True, seed=0, drop_last=False)
    b.load_state_dict(state)
    assert b.seed == 5 and b.epoch == 2
    assert all(torch.equal(p, q["rna_data"]) for p, q in zip(third, b))
    # a consumer that stops at the last batch has finished the epoch
    it = iter(b)
    for _ in range(len(b)):
        next(it)
    assert b.epoch == 4


def test_loader_arguments():
    ts = RT.RnaTableSet.from_array(_table(), CPU)
    with pytest.raises(IndexError):
        RT.RnaTableLoader(ts, [0, 37], 4)
    with pytest.raises(IndexError):
        RT.RnaTableLoader(ts, [-1], 4)
    with pytest.raises(ValueError):
        RT.RnaTableLoader(ts, [0], 0)
    empty = RT.RnaTableLoader(ts, [], 4, shuffle=True)
    assert len(empty) == 0 and list(empty) == [] and empty.epoch == 1
    for bad in (np.zeros((2, 3)), np.zeros(3, dtype=np.float32), torch.zeros(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            RT.RnaTableSet.from_array(bad, CPU)
    with pytest.raises(ValueError):
        RT.rows_gather(torch.zeros(2, 3), None, n=1)                 # a CPU tensor has no kernel to run


def test_budget_is_refused_before_any_allocation(monkeypatch):
    rows = torch.zeros(10, 6)
    moved = []
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: moved.append(a) or self)
    with pytest.raises(MemoryError) as e:
        RT.RnaTableSet.from_array(rows, CPU, max_bytes=239)
    assert "240" in str(e.value) and "239" in str(e.value)
    assert moved == []
    ts = RT.RnaTableSet.from_array(rows, CPU, max_bytes=240)
    assert len(moved) == 1 and ts.nbytes == 240 and len(ts) == 10 and ts.features == 6


# ------------------------------------------------------------------ the binding
def test_abi_carries_the_symbol():
    import ctypes
    p, i, ll = _abi._p, _abi._i, ctypes.c_longlong
    assert _abi.PROTOTYPES["rg_rows_gather_f32"] == (i, [p, ll, i, ll, p, p, i, ll, p])
    header = open(os.path.join(ROOT, "include", "rnagan_hip.h")).read()
    assert "int rg_rows_gather_f32(const float* table, long long M, int F, long long ld_table, const int* index, float* dst, " \
           "int N,\n                       long long ld_dst, void* stream);" in header
    assert _abi.ABI_VERSION == 618
    from rna_gan_amd import build
    assert "rg_rows.hip" in build.SOURCES and "rg_rows.hip" not in build.BF16_ONLY
    assert hasattr(_abi.load(), "rg_rows_gather_f32") and hasattr(_abi.load("f16"), "rg_rows_gather_f32")


# ------------------------------------------------------------------ the training CLI's arguments (nothing here reaches a device)
def _cli():
    spec = importlib.util.spec_from_file_location("betaVAE_training_cli", os.path.join(ROOT, "betaVAE_training.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_csvs(tmp_path):
    paths = []
    for i, df in enumerate(make_tables()):
        paths.append(str(tmp_path / ("table%d.csv" % i)))
        df.to_csv(paths[-1], index=False)
    return paths


def test_cli_without_tables_says_so(tmp_path):
    cfg = tmp_path / "c.json"
    cfg.write_text(json.dumps({"save_dir": str(tmp_path / "out"), "rna_features": GENES}))
    with pytest.raises(SystemExit) as e:
        _cli().main(["--config", str(cfg)])
    assert "path_csv" in str(e.value) and "out of scope" not in str(e.value)
    assert not os.path.exists(str(tmp_path / "out"))


def test_cli_reports_a_feature_mismatch(tmp_path):
    cfg = tmp_path / "c.json"
    cfg.write_text(json.dumps({"save_dir": str(tmp_path / "out"), "rna_features": GENES + 3, "path_csv": _write_csvs(tmp_path)}))
    with pytest.raises(SystemExit) as e:
        _cli().main(["--config", str(cfg)])
    assert "rna_features" in str(e.value) and str(GENES + 3) in str(e.value) and str(GENES) in str(e.value)


def test_cli_tables_from_csv_files(tmp_path, golden_dir):
    """real_tables on the CSV files: the rows, scaler.npz and split.npz of the fixture's run."""
    z, _tables, (_rows, scaler, indices, _parts) = _f11(golden_dir)
    out = str(tmp_path / "out")
    cfg = {"save_dir": out, "rna_features": GENES, "path_csv": _write_csvs(tmp_path)}

    class Args:
        seed = SEED
    got = _cli().real_tables(Args, cfg)
    for k in RT.PARTS:
        assert np.array_equal(_bits(got["rows"][k]), _bits(z[k + ".rows"]))
    assert got["features"] == GENES and got["train_items"].tolist() == list(range(24))
    assert got["test_ids"].tolist() == z["test.wsi"].tolist() and got["test_labels"].tolist() == [0] * 5 + [1] * 4
    saved = RT.RnaScaler.load(os.path.join(out, "scaler.npz"))
    assert np.array_equal(saved.mean, scaler.mean) and np.array_equal(saved.scale, scaler.scale)
    with np.load(os.path.join(out, "split.npz")) as s:
        assert sorted(s.files) == sorted("%s_%d" % (k, i) for i in (0, 1) for k in RT.PARTS)
        for i in (0, 1):
            for k in RT.PARTS:
                assert s["%s_%d" % (k, i)].tolist() == indices[i][k].tolist()
    cfg["quick"] = 1
    quick = _cli().real_tables(Args, cfg)
    assert len(quick["train_items"]) == 10 and len(set(quick["train_items"].tolist())) == 10
