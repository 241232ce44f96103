"""The training set resident on the device: decoded once, kept as uint8, every batch formed there by one launch.

The loaders in front of the step are host-bound: LZ4 and pickle decode, collate, pinning and one host-to-device
copy per batch, for tiles that are re-read from disk every epoch.  The working set is small -- at most ``--num_patches`` tiles
of 196 608 bytes per slide -- so ``DeviceTileSet`` reads the dataset ONCE and keeps the tiles on the device as uint8, and
``DeviceTileLoader`` forms each training batch with one launch of rg_tile_gather_transform (rna_gan_amd/csrc/rg_augment.hip):
gather by index, normalise, per-sample D4 symmetry.  The steady-state loop has no loader workers, no pinning thread and no
per-batch host-to-device copy.

Two counter-based streams, no generator object carrying state:

* the ORDER of epoch e on rank r is ``np.random.default_rng([seed, r, e]).permutation(M)``, uploaded once per epoch as int32;
  batch t hands the kernel ``perm + t * batch_size``;
* the D4 CODES are the given ``InputTransform``'s (``codes_for`` and its ``batches`` counter, rna_gan_amd.augment); the whole
  epoch's codes are uploaded once, and ``transform.last_codes`` is set per batch as the transform itself would.

Data parallel: each rank holds only its shard, chosen once by ``shard_indices`` (the rule of the CLI's function of the same name:
strided, truncated to an equal whole number of batches per rank) and permuted per epoch under the rank's own stream, so every rank
yields the same number of full batches and the collectives pair.

On a CPU device the same bits come from torch ops (the rule of InputTransform); on a CUDA device there is no fallback: the
kernel runs or the call raises.  Out of scope: sets larger than the device's memory (no partial residency, no spill), the
evaluation sets, and caching the frozen encoder's per-slide output (``wganvae`` still runs the encoder per batch).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import _abi
from . import dist as D_
from .augment import d4_apply

RESERVE_BYTES = 8 << 30          # what the default budget leaves free on the device: the step's own buffers, graphs, workspaces


def shard_indices(n_items, rank, world, batch_size):
    """Rank ``rank``'s shard of a list of n_items: strided (rank, rank + world, ...), truncated so that every rank gets the same
    number of items and that number is a multiple of the batch size."""
    per_rank = (n_items // world) // batch_size * batch_size
    return list(range(rank, n_items, world))[:per_rank]


def epoch_order(seed, rank, epoch, m):
    """The order of epoch ``epoch`` on rank ``rank`` over m tiles: a pure function of its arguments."""
    return np.random.default_rng([int(seed), int(rank), int(epoch)]).permutation(int(m)).astype(np.int32)


class _Items(Dataset):
    """``ds`` restricted to ``items`` (None: all of it), in that order."""

    def __init__(self, ds, items):
        self.ds, self.items = ds, items

    def __len__(self):
        return len(self.ds) if self.items is None else len(self.items)

    def __getitem__(self, i):
        return self.ds[i if self.items is None else self.items[i]]


def _as_list(batch):
    return batch


def _check_tile(image, shape):
    if not torch.is_tensor(image) or image.dtype != torch.uint8:
        raise ValueError("DeviceTileSet holds uint8 tiles (build the dataset with transforms=None / as_u8), got %s"
                         % (image.dtype if torch.is_tensor(image) else type(image).__name__))
    if image.dim() != 3 or image.shape[1] != image.shape[2]:
        raise ValueError("DeviceTileSet holds square [C][S][S] tiles, got %s" % (tuple(image.shape),))
    if shape is not None and tuple(image.shape) != tuple(shape):
        raise ValueError("DeviceTileSet: a tile of shape %s in a set of %s" % (tuple(image.shape), tuple(shape)))


class DeviceTileSet:
    """tiles [M][C][S][S] uint8, labels [M] fp32 and -- for a set with RNA -- the de-duplicated rows rna [P][G] fp32 with
    row_of [M] int32 (tile m's row is rna[row_of[m]]: a dataset repeats one row per tile of a slide, the table holds it once),
    all on ``device``.  ``form`` is the batch structure of the dataset it came from: "dict", "tuple" or "tensor"."""

    def __init__(self, tiles, rna=None, row_of=None, labels=None, form=None, dropped=0, build_seconds=None):
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[2] != tiles.shape[3]:
            raise ValueError("DeviceTileSet holds [M][C][S][S] uint8 tiles, got %s %s" % (tiles.dtype, tuple(tiles.shape)))
        M = tiles.shape[0]
        if (rna is None) != (row_of is None):
            raise ValueError("rna and row_of go together")
        if rna is not None:
            if rna.dtype != torch.float32 or rna.dim() != 2 or row_of.dtype != torch.int32 or tuple(row_of.shape) != (M,):
                raise ValueError("rna is [P][G] float32 and row_of is [M] int32")
            if M and not (0 <= int(row_of.min()) and int(row_of.max()) < rna.shape[0]):
                raise ValueError("row_of points outside the RNA table")
        if labels is not None and labels.shape[0] != M:
            raise ValueError("one label per tile")
        self.tiles, self.rna, self.row_of, self.labels = tiles.contiguous(), rna, row_of, labels
        self.form = form or ("dict" if rna is not None else "tuple" if labels is not None else "tensor")
        if self.form not in ("dict", "tuple", "tensor") or (self.form == "dict") != (rna is not None) or \
                (self.form != "tensor" and labels is None):
            raise ValueError("form %r does not fit the side data" % (self.form,))
        self.dropped = int(dropped)
        self.build_seconds = build_seconds

    def __len__(self):
        return self.tiles.shape[0]

    @property
    def device(self):
        return self.tiles.device

    @property
    def nbytes(self):
        """Bytes resident on the device."""
        return sum(t.numel() * t.element_size() for t in (self.tiles, self.rna, self.row_of, self.labels) if t is not None)

    @classmethod
    def from_tensors(cls, tiles_u8, rna=None, row_of=None, labels=None, device="cuda:0"):
        """A set from host (or device) tensors.  rna without row_of: one row per tile.  rna -> dict batches (labels default to
        zeros); labels alone -> (image, labels) batches; neither -> bare image tensors."""
        device = torch.device(device)
        if not torch.is_tensor(tiles_u8) or tiles_u8.dtype != torch.uint8 or tiles_u8.dim() != 4:
            raise ValueError("from_tensors takes an [M][C][S][S] uint8 tensor")
        M = tiles_u8.shape[0]
        if rna is not None:
            rna = rna.to(device=device, dtype=torch.float32).contiguous()
            if row_of is None:
                if rna.shape[0] != M:
                    raise ValueError("rna without row_of needs one row per tile")
                row_of = torch.arange(M, dtype=torch.int32)
            row_of = row_of.to(device=device, dtype=torch.int32).contiguous()
            if labels is None:
                labels = torch.zeros(M, dtype=torch.float32)
        elif row_of is not None:
            raise ValueError("row_of without rna")
        if labels is not None:
            labels = labels.to(device=device, dtype=torch.float32).contiguous()
        return cls(tiles_u8.to(device).contiguous(), rna, row_of, labels)

    @classmethod
    def from_dataset(cls, ds, device, items=None, chunk=256, workers=0, max_bytes=None):
        """Read ``ds`` (a PatchDataset, a PatchRNADataset or the CLI's SyntheticTiles, built with transforms=None / as_u8) once,
        in dataset order -- ``items``: the list of dataset indices to read, a rank's shard -- through an unshuffled DataLoader
        over ``chunk`` items with ``workers`` workers; each chunk is uploaded from pinned memory into its slice of the tile
        tensor.  Records whose image is None (unreadable: what the reference's collate_fn drops per batch) are dropped here,
        once, and counted in ``dropped``.  Raises ValueError for a tile that is not uint8 [C][S][S], and MemoryError -- before
        the first upload -- when the set needs more than ``max_bytes`` (default: the device's free memory minus 8 GiB; no
        limit on a CPU device)."""
        import time
        t0 = time.perf_counter()
        device = torch.device(device)
        view = _Items(ds, None if items is None else [int(i) for i in items])
        n = len(view)
        if max_bytes is None and device.type == "cuda":
            max_bytes = torch.cuda.mem_get_info(device)[0] - RESERVE_BYTES
        loader = DataLoader(view, batch_size=max(int(chunk), 1), shuffle=False, num_workers=int(workers), collate_fn=_as_list)
        tiles = None
        shape = None
        form = None
        rows, row_index, row_of, labels = [], {}, [], []
        m = dropped = 0
        for batch in loader:
            keep = []
            for item in batch:
                if form is None:
                    form = "dict" if isinstance(item, dict) else "tuple" if isinstance(item, (tuple, list)) else "tensor"
                image = item["image"] if form == "dict" else item[0] if form == "tuple" else item
                if image is None:
                    dropped += 1
                    continue
                _check_tile(image, shape)
                if shape is None:
                    # the budget, before the first upload: every item counted as readable; of the RNA table (one row per
                    # SLIDE, 1/300 of its tiles' bytes at the default --num_patches) only this first row is known yet
                    shape = tuple(image.shape)
                    need = n * int(np.prod(shape)) + (n * 4 if form != "tensor" else 0)
                    if form == "dict":
                        need += n * 4 + item["rna_data"].numel() * 4
                    if max_bytes is not None and need > max_bytes:
                        raise MemoryError(
                            "DeviceTileSet: %d tiles of %s need %d bytes on %s, the budget is %d bytes (free memory minus %d "
                            "GiB unless given): no partial residency -- lower --num_patches, raise the budget, or train "
                            "through the host loader" % (n, shape, need, device, max_bytes, RESERVE_BYTES >> 30))
                    tiles = torch.empty((n,) + shape, dtype=torch.uint8, device=device)
                keep.append(image)
                if form == "dict":
                    row = item["rna_data"].to(torch.float32).contiguous()
                    key = row.numpy().tobytes()
                    if key not in row_index:
                        row_index[key] = len(rows)
                        rows.append(row)
                    row_of.append(row_index[key])
                if form != "tensor":
                    labels.append(torch.as_tensor(item["labels"] if form == "dict" else item[1], dtype=torch.float32))
            if keep:
                host = torch.stack(keep)
                if device.type == "cuda":
                    # pinned staging from torch's caching host allocator: a block is handed out again only once the copy
                    # that read it has completed
                    host = host.pin_memory()
                tiles[m:m + len(keep)].copy_(host, non_blocking=True)
                m += len(keep)
        if tiles is None:
            raise ValueError("DeviceTileSet: no readable tile among %d items" % n)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        if m < n:
            tiles = tiles[:m]                  # (a view: the unreadable records' share stays allocated, a copy would double the set)
        rna = torch.stack(rows).to(device) if form == "dict" else None
        rmap = torch.tensor(row_of, dtype=torch.int32, device=device) if form == "dict" else None
        lab = torch.stack(labels).to(device) if form != "tensor" else None
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        return cls(tiles, rna, rmap, lab, form=form, dropped=dropped, build_seconds=time.perf_counter() - t0)


class DeviceTileLoader:
    """What Trainer.train iterates over a DeviceTileSet: batches in the dataset's structure -- {"image", "rna_data", "labels"},
    (image, labels) or the bare image -- with ``image`` the FINAL fp32 batch of one rg_tile_gather_transform launch (the Trainer
    must not hold an input_transform of its own) and the side data taken by torch.index_select on the device.

    transform: an rna_gan_amd.augment.InputTransform, whose mean / std, code stream and ``batches`` counter the loader uses
    (None: mean = std = 0.5, no symmetry).  state_dict() / load_state_dict(): the seed, the number of epochs completed and the
    transform's state; the Trainer keeps them in the checkpoint under "data_loader"."""

    final_images = True          # the batches are on the device and transformed: no prefetcher, no second transform

    def __init__(self, tileset, batch_size, transform=None, seed=0, rank=None, drop_last=True):
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        self.tileset = tileset
        self.batch_size = int(batch_size)
        self.transform = transform
        self.seed = int(seed)
        self.rank = D_.rank() if rank is None else int(rank)
        self.drop_last = bool(drop_last)
        self.epoch = 0               # epochs completed: the next pass uses the order of this epoch
        self.mean, self.std = (0.5, 0.5) if transform is None else (transform.mean, transform.std)
        if float(self.std) == 0.0:
            raise ValueError("std must not be 0")

    def __len__(self):
        m, b = len(self.tileset), self.batch_size
        return m // b if self.drop_last else (m + b - 1) // b

    def order_for(self, epoch):
        return epoch_order(self.seed, self.rank, epoch, len(self.tileset))

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch,
                "transform": None if self.transform is None else self.transform.state_dict()}

    def load_state_dict(self, state):
        self.seed = int(state["seed"])
        self.epoch = int(state["epoch"])
        if self.transform is not None and state.get("transform") is not None:
            self.transform.load_state_dict(state["transform"])

    # ------------------------------------------------------------------ one batch
    def _images(self, index, codes, n):
        """index / codes: device int32 views of n entries (codes may be None)."""
        ts = self.tileset
        M, C, S, _ = ts.tiles.shape
        device = ts.device
        if device.type != "cuda":
            x = ts.tiles.index_select(0, index.long())
            x = (x.float() / 255.0 - self.mean) / self.std          # the three fp32 operations of the kernel's contract
            if codes is None or n == 0:
                return x
            return torch.stack([d4_apply(x[k], c) for k, c in enumerate(codes.tolist())]).contiguous()
        out = torch.empty((n, C, S, S), dtype=torch.float32, device=device)
        _abi.launch("rg_tile_gather_transform", device, ts.tiles.data_ptr(), M, index.data_ptr(), out.data_ptr(), n, C, S,
                    0 if codes is None else codes.data_ptr(), self.mean, self.std)
        return out

    def __iter__(self):
        ts, tf, B = self.tileset, self.transform, self.batch_size
        M, device = len(ts), ts.device
        nb = len(self)
        order = self.order_for(self.epoch)
        if M and not (0 <= int(order.min()) and int(order.max()) < M):       # the kernel's clamp is never relied upon
            raise RuntimeError("DeviceTileLoader: an index outside the set")
        sizes = [min(B, M - t * B) for t in range(nb)]
        host_codes = None
        if tf is not None and tf.augment == "d4":
            host_codes = [tf.codes_for(tf.batches + t, sizes[t]) for t in range(nb)]

        def upload(a):
            t = torch.from_numpy(a)
            return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t
        perm = upload(order)                                                  # once per epoch
        codes = upload(np.concatenate(host_codes)) if host_codes and nb else None
        for t in range(nb):
            n = sizes[t]
            index = perm[t * B:t * B + n]
            if host_codes is not None:
                tf.last_codes = host_codes[t]
                tf.batches += 1
            image = self._images(index, None if codes is None else codes[t * B:t * B + n], n)
            if t == nb - 1:
                self.epoch += 1      # with the last batch handed out, not at exhaustion: a consumer that stops there has finished
            if ts.form == "tensor":
                yield image
            elif ts.form == "tuple":
                yield [image, ts.labels.index_select(0, index)]
            else:
                yield {"image": image, "rna_data": ts.rna.index_select(0, ts.row_of.index_select(0, index)),
                       "labels": ts.labels.index_select(0, index)}
        if nb == 0:
            self.epoch += 1
