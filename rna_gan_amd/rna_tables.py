"""Real expression tables for betaVAE training: the reference's CSV pipeline on the host, once per run, and the standardised
table resident on the device, every batch formed there by one launch.

Host side (fp64, once per run; src/betaVAE_training.py:70-101, src/read_data.py:374-410, :467-498):

* ``split_tables``: per CSV an 80/20 train/test split, then an 80/20 train/val split of the train part, the parts concatenated
  across CSVs in the order given.  The reference calls scikit-learn's ``train_test_split(df, test_size=0.2)`` with no
  ``random_state`` after ``np.random.seed(seed)``; for m rows that is ``p = np.random.permutation(m)``, test =
  ``p[:ceil(0.2 m)]``, train = ``p[ceil(0.2 m) : ceil(0.2 m) + floor(0.8 m)]`` on the global legacy generator, restated here in
  numpy so that the run-time path needs no scikit-learn (tests/test_rna_tables_cpu.py compares the two where it is installed).
* ``RnaScaler``: ``log_standardize_rna``'s contract (rna_gan_amd.data), fitted on the train split only and applied to all three:
  ln with zeros (and NaNs) left at 0, fp64 mean and population variance, a scale below 10 eps replaced by 1.
* ``rna_rows`` / ``RNADataset``: the fp32 rows the reference's dataset hands out one dict at a time.

Device side: ``RnaTableSet`` holds the rows [M][F] fp32 on the device -- train, val and test in ONE table, addressed through
index subsets -- and ``RnaTableLoader`` yields ``{"rna_data": x}`` with x the dense [n][F] batch of one rg_rows_gather_f32 launch
(rna_gan_amd/csrc/rg_rows.hip).  The order of epoch e is ``items[np.random.default_rng([seed, 0, e]).permutation(len(items))]``,
uploaded once per epoch as int32; batch t hands the kernel ``order + t * batch_size``: a steady-state batch issues no
host-to-device copy, no collate and no worker.  The loader consumes no torch random numbers.  On a CPU tensor the same bits come
from torch indexing; on a CUDA tensor there is no fallback: the kernel runs or the call raises.

Out of scope: tables larger than the device's memory (no partial residency), ``minmax`` normalisation (commented out in the
reference), data parallel betaVAE training.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _abi
from .resident import RESERVE_BYTES

PARTS = ("train", "val", "test")


# ------------------------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------------------------
def split_indices(m, test_size=0.2):
    """(train, test) row positions of one ``train_test_split(range(m), test_size=0.2)`` call: ONE permutation drawn on numpy's
    global legacy generator."""
    m = int(m)
    n_test = int(math.ceil(test_size * m))
    n_train = int(math.floor((1.0 - test_size) * m))
    if n_train < 1 or n_test < 1:
        raise ValueError("a table of %d rows cannot be split %g / %g" % (m, 1.0 - test_size, test_size))
    p = np.random.permutation(m)
    return p[n_test:n_test + n_train], p[:n_test]


def split_tables(frames, seed=None):
    """frames: one DataFrame per CSV.  Returns (parts, indices): ``parts[k]`` for k in train / val / test is the concatenation,
    in the order given, of every table's share; ``indices[i][k]`` are the row positions of table i that went there, in order.
    seed: seeds numpy's global legacy generator first (None: it is used as it stands, as the reference's training script does
    with its seeding commented out)."""
    import pandas as pd
    if seed is not None:
        np.random.seed(int(seed))
    indices, shares = [], {k: [] for k in PARTS}
    for df in frames:
        m = df.shape[0]
        train, test = split_indices(m)
        tr2, va2 = split_indices(len(train))
        idx = {"train": train[tr2], "val": train[va2], "test": test}
        indices.append(idx)
        for k in PARTS:
            shares[k].append(df.iloc[idx[k]])
    parts = {k: (pd.concat(v) if len(v) > 1 else v[0]) for k, v in shares.items()}
    return parts, indices


def rna_columns(frame):
    return [c for c in frame.columns if "rna_" in c]


def log_rna(x):
    """ln(x) in fp64 with zeros -- and the NaNs of negative or missing entries -- left at 0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lx = np.where(x == 0, 0.0, np.log(x))
    return np.where(np.isnan(lx), 0.0, lx)


def rna_rows(frame):
    """The fp32 matrix [rows][genes] of a frame: the columns whose name contains ``rna_``, in frame order, fp64 -> fp32."""
    return np.ascontiguousarray(frame[rna_columns(frame)].to_numpy(dtype=np.float64).astype(np.float32))


class RnaScaler:
    """StandardScaler on ln-transformed expression, fitted on the train split only."""

    def __init__(self, mean=None, scale=None, columns=None):
        self.mean = None if mean is None else np.asarray(mean, dtype=np.float64)
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        self.columns = None if columns is None else [str(c) for c in columns]

    def fit(self, train_lx, columns=None):
        lx = np.asarray(train_lx, dtype=np.float64)
        if lx.ndim != 2 or lx.shape[0] < 1:
            raise ValueError("RnaScaler.fit takes a [rows][genes] matrix with at least one row")
        self.mean = lx.mean(axis=0)
        scale = np.sqrt(lx.var(axis=0))
        scale[scale < 10 * np.finfo(np.float64).eps] = 1.0          # constant features are not scaled
        self.scale = scale
        if columns is not None:
            self.columns = [str(c) for c in columns]
        return self

    def _fitted(self, width):
        if self.mean is None:
            raise RuntimeError("RnaScaler: fit or load first")
        if width != self.mean.shape[0]:
            raise ValueError("RnaScaler: %d columns, fitted on %d" % (width, self.mean.shape[0]))

    def transform(self, lx):
        lx = np.asarray(lx, dtype=np.float64)
        self._fitted(lx.shape[-1])
        return (lx - self.mean) / self.scale

    def transform_frame(self, frame):
        """fp64 standardised matrix of a raw frame's rna_ columns (ln included)."""
        cols = rna_columns(frame)
        if self.columns is not None and cols != self.columns:
            raise ValueError("RnaScaler: the frame's rna_ columns are not the ones the scaler was fitted on")
        return self.transform(log_rna(frame[cols].to_numpy(dtype=np.float64)))

    def inverse_transform(self, y):
        """fp32 input: fp32(fp32(y scale) + mean), each operation evaluated in fp64 and rounded to fp32 (what scikit-learn's
        in-place ``X *= scale_; X += mean_`` gives for an fp32 array); any other input is computed and returned in fp64."""
        y = np.asarray(y)
        self._fitted(y.shape[-1])
        if y.dtype == np.float32:
            t = (y.astype(np.float64) * self.scale).astype(np.float32)
            return (t.astype(np.float64) + self.mean).astype(np.float32)
        return np.asarray(y, dtype=np.float64) * self.scale + self.mean

    def save(self, path):
        if self.mean is None:
            raise RuntimeError("RnaScaler: nothing to save")
        with open(path, "wb") as f:
            np.savez(f, mean=self.mean, scale=self.scale, columns=np.array(self.columns or [], dtype=str))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cols = [str(c) for c in z["columns"].tolist()]
            return cls(z["mean"], z["scale"], cols or None)


def prepare_tables(frames, seed=None):
    """The reference's sequence up to the datasets: split, fit on train, transform all three.  Returns (rows, scaler, indices,
    parts): rows[k] the standardised fp32 matrix of part k (fp64 -> fp32, what RNADataset hands out), parts[k] the raw frames."""
    parts, indices = split_tables(frames, seed)
    cols = rna_columns(parts["train"])
    for k in PARTS:
        if rna_columns(parts[k]) != cols:
            raise ValueError("the tables do not share their rna_ columns")
    scaler = RnaScaler().fit(log_rna(parts["train"][cols].to_numpy(dtype=np.float64)), cols)
    rows = {k: np.ascontiguousarray(scaler.transform_frame(parts[k]).astype(np.float32)) for k in PARTS}
    return rows, scaler, indices, parts


def read_tables(config):
    """The frames of a config's ``path_csv`` (a list; a single path may be given as a string), read with pandas."""
    import pandas as pd
    path_csv = config.get("path_csv")
    if not path_csv:
        raise SystemExit("the config has no 'path_csv' (the list of RNA-Seq CSV files, one per tissue)")
    if isinstance(path_csv, str):
        path_csv = [path_csv]
    frames = [pd.read_csv(p) for p in path_csv]
    for p, df in zip(path_csv, frames):
        if not rna_columns(df):
            raise SystemExit("%s has no rna_ columns" % p)
    return frames


def check_features(config, width):
    """The config's ``rna_features`` against the tables' width."""
    want = config.get("rna_features")
    if want is not None and int(want) != int(width):
        raise SystemExit("rna_features is %d in the config, but the tables of path_csv have %d rna_ columns" % (int(want), width))
    return int(width)


def model_from_config(config, features):
    """betaVAE(features, z, encoder_dims, decoder_dims, beta) with the reference's sizes unless the config's optional
    ``encoder_dims`` / ``decoder_dims`` say otherwise (z = the last encoder width, as the reference's 2048)."""
    from .betavae import betaVAE
    enc = [int(v) for v in config.get("encoder_dims", [6000, 4000, 2048])]
    dec = [int(v) for v in config.get("decoder_dims", [4000, 6000])]
    return betaVAE(int(features), enc[-1], enc, dec, beta=config.get("beta", 2))


def scaler_for(config, seed, path=None, frames=None):
    """The run's scaler: ``path``, else ``scaler.npz`` in the config's save_dir, else refitted by repeating the split under the
    seed (all the reference does)."""
    import os
    if path is None:
        saved = os.path.join(config.get("save_dir", "."), "scaler.npz")
        path = saved if os.path.exists(saved) else None
    if path is not None:
        return RnaScaler.load(path)
    return prepare_tables(read_tables(config) if frames is None else frames, seed)[1]


class RNADataset(Dataset):
    """src/read_data.py:374-410: items ``{"rna_data": fp32 [G]}`` over a list of frames, CSV paths or fp32 row matrices.
    quick: 10 rows sampled per table (``DataFrame.sample(10)``, numpy's global generator), as the reference does."""

    def __init__(self, frames_or_paths, quick=False):
        import pandas as pd
        mats = []
        for t in frames_or_paths:
            if isinstance(t, np.ndarray):
                mat = np.ascontiguousarray(t, dtype=np.float32)
                if quick:
                    mat = mat[np.random.choice(mat.shape[0], 10, replace=False)]
            else:
                df = pd.read_csv(t) if isinstance(t, str) else t
                if quick:
                    df = df.sample(10)
                mat = rna_rows(df)
            mats.append(mat)
        self.rows = torch.from_numpy(np.concatenate(mats, axis=0) if len(mats) != 1 else mats[0])

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, i):
        return {"rna_data": self.rows[i]}


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
def epoch_order(seed, epoch, items):
    """The order of epoch ``epoch`` over ``items``: a pure function of its arguments."""
    items = np.asarray(items)
    return items[np.random.default_rng([int(seed), 0, int(epoch)]).permutation(len(items))].astype(np.int32)


class RnaTableSet:
    """rows [M][F] fp32 on ``device``: train, val and test rows in one table; loaders address it through index subsets."""

    def __init__(self, rows):
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] < 1:
            raise ValueError("RnaTableSet holds an [M][F] float32 tensor")
        self.rows = rows.contiguous()

    def __len__(self):
        return self.rows.shape[0]

    @property
    def features(self):
        return self.rows.shape[1]

    @property
    def device(self):
        return self.rows.device

    @property
    def nbytes(self):
        return self.rows.numel() * 4

    @classmethod
    def from_array(cls, rows_f32, device, max_bytes=None):
        """rows_f32: numpy or torch [M][F] float32 on the host.  Raises MemoryError -- before anything is allocated on the
        device -- when the table needs more than ``max_bytes`` (default: the device's free memory minus 8 GiB; no limit on a
        CPU device): no partial residency."""
        device = torch.device(device)
        host = torch.from_numpy(np.ascontiguousarray(rows_f32)) if isinstance(rows_f32, np.ndarray) else rows_f32
        if not torch.is_tensor(host) or host.dtype != torch.float32 or host.dim() != 2:
            raise ValueError("RnaTableSet.from_array takes an [M][F] float32 array, got %s" % (
                "%s %s" % (host.dtype, tuple(host.shape)) if torch.is_tensor(host) else type(host).__name__))
        need = host.numel() * 4
        if max_bytes is None and device.type == "cuda":
            max_bytes = torch.cuda.mem_get_info(device)[0] - RESERVE_BYTES
        if max_bytes is not None and need > max_bytes:
            raise MemoryError("RnaTableSet: %d rows of %d floats need %d bytes on %s, the budget is %d bytes (free memory minus "
                              "%d GiB unless given): no partial residency -- raise the budget or train through the host loader "
                              "(--resident 0)" % (host.shape[0], host.shape[1], need, device, max_bytes, RESERVE_BYTES >> 30))
        return cls(host.to(device))


def rows_gather(rows, index, n=None, ld_dst=None):
    """rg_rows_gather_f32 on a dense device table: index a device int32 tensor (None: the first n rows); returns [n][ld_dst]
    (default ld_dst = F).  CUDA tensors only."""
    if rows.device.type != "cuda" or rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows_gather takes a dense [M][F] float32 tensor on a ROCm device")
    M, F = rows.shape
    if index is not None:
        if index.dtype != torch.int32 or index.dim() != 1 or index.device != rows.device or not index.is_contiguous():
            raise ValueError("index is a dense int32 vector on the table's device")
        n = index.shape[0]
    ld = F if ld_dst is None else int(ld_dst)
    out = torch.empty((int(n), ld), dtype=torch.float32, device=rows.device)
    if int(n) == 0:
        return out                       # (an empty tensor has no address to hand over)
    _abi.launch("rg_rows_gather_f32", rows.device, rows.data_ptr(), M, F, F, 0 if index is None else index.data_ptr(), out.data_ptr(),
                int(n), ld)
    return out


class RnaTableLoader:
    """What train_betaVAE / evaluate_betaVAE iterate over an RnaTableSet: ``{"rna_data": x}``, x the dense fp32 [n][F] batch of
    one launch, already on the device.  items: the rows of the table this loader covers (a split).  state_dict() /
    load_state_dict(): ``{"seed", "epoch"}``, epoch = passes completed."""

    def __init__(self, tableset, items, batch_size, shuffle=False, seed=0, drop_last=False):
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        if items.size and not (0 <= int(items.min()) and int(items.max()) < len(tableset)):    # the kernel's clamp is never relied upon
            raise IndexError("RnaTableLoader: an item outside the table of %d rows" % len(tableset))
        self.tableset = tableset
        self.items = items
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.seed = int(seed)
        self.drop_last = bool(drop_last)
        self.epoch = 0
        self._fixed = None               # the device copy of an unshuffled order: uploaded once

    def __len__(self):
        m, b = len(self.items), self.batch_size
        return m // b if self.drop_last else (m + b - 1) // b

    def order_for(self, epoch):
        return epoch_order(self.seed, epoch, self.items) if self.shuffle else self.items.astype(np.int32)

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch}

    def load_state_dict(self, state):
        self.seed = int(state["seed"])
        self.epoch = int(state["epoch"])

    def _upload(self, order):
        t = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32))
        device = self.tableset.device
        return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t

    def __iter__(self):
        ts, B = self.tableset, self.batch_size
        m, nb = len(self.items), len(self)
        if self.shuffle:
            order = self._upload(self.order_for(self.epoch))                  # once per epoch
        else:
            if self._fixed is None:
                self._fixed = self._upload(self.order_for(0))
            order = self._fixed
        for t in range(nb):
            index = order[t * B:min(m, t * B + B)]
            if ts.device.type == "cuda":
                x = rows_gather(ts.rows, index)
            else:
                x = ts.rows.index_select(0, index.long())
            if t == nb - 1:
                self.epoch += 1          # with the last batch handed out, not at exhaustion: a consumer that stops there has finished
            yield {"rna_data": x}
        if nb == 0:
            self.epoch += 1
