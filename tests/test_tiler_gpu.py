"""rna_gan_amd.tiler.tile_raster on the device against the same call on a CPU tensor (which tests/test_tiler_refs_cpu.py pins to a
sequential per-window loop through Pillow), and tile_slides.py --synthetic end to end: a child process writes the stores, PatchDataset
reads the same tiles back."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import data as PD
from rna_gan_amd import tiler as TL
import tiler_refs as R

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CPU = {}


def _cpu(max_patches):
    if max_patches not in _CPU:
        _CPU[max_patches] = TL.tile_raster(torch.from_numpy(R.slide().copy()), max_patches=max_patches, **R.SLIDE_KW)
    return _CPU[max_patches]


@pytest.mark.parametrize("batch,max_patches", [(256, 10 ** 6), (7, 10 ** 6), (4, 5), (1, 5)])
def test_tile_raster_on_the_device_equals_the_cpu_tensor(batch, max_patches):
    want = _cpu(max_patches)
    assert 0 < len(want) < want.in_mask < want.candidates
    got = TL.tile_raster(torch.from_numpy(R.slide().copy()).to(DEV), max_patches=max_patches, batch=batch, **R.SLIDE_KW)
    assert got.tiles.is_cuda and got.mask.is_cuda
    assert torch.equal(got.tiles.cpu(), want.tiles), "tiles"
    assert np.array_equal(got.origins, want.origins) and np.array_equal(got.qc, want.qc)
    assert torch.equal(got.mask.cpu(), want.mask)
    assert (got.read, got.candidates, got.in_mask, got.examined) == (want.read, want.candidates, want.in_mask, want.examined)


def test_order_thumbnail_and_mask_on_the_device():
    raster = torch.from_numpy(R.slide().copy()).to(DEV)
    want = _cpu(5)
    bgr = TL.tile_raster(raster, max_patches=5, order="bgr", **R.SLIDE_KW)
    assert torch.equal(bgr.tiles.cpu(), want.tiles.flip(-1))
    thumb = TL.thumbnail(raster, 8)
    a = TL.tile_raster(raster, thumbnail=thumb.cpu(), max_patches=5, patch_size=64, app_mag=40.0)
    b = TL.tile_raster(raster, mask=want.mask, max_patches=5, patch_size=64, app_mag=40.0)
    assert torch.equal(a.tiles.cpu(), want.tiles) and torch.equal(b.tiles.cpu(), want.tiles)


def test_cli_synthetic_in_a_child_process_and_patchdataset_reads_the_tiles_back(tmp_path):
    import pandas as pd
    patches, masks = str(tmp_path / "patches"), str(tmp_path / "masks")
    cmd = [sys.executable, os.path.join(ROOT, "tile_slides.py"), "--synthetic", "--synthetic_slides", "2", "--synthetic_size", "1024x1280",
           "--seed", "3", "--patch_path", patches, "--mask_path", masks, "--patch_size", "64", "--app_mag", "40", "--thumb_factor", "8",
           "--max_patches_per_slide", "9", "--batch", "4", "--qc_report"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ids = ["synthetic_0.svs", "synthetic_1.svs"]
    table = pd.DataFrame({"wsi_file_name": ids, "rna_0": [0.0] * 2, "patch_data_path": [patches] * 2, "labels": [0] * 2})
    ds = PD.PatchDataset(patches, table, 64, max_patches_total=100)
    got = {q: {} for q in ids}
    for j in range(len(ds)):
        img, _ = ds[j]
        got[ds.filenames[j]][int(ds.keys[j])] = img.numpy().transpose(1, 2, 0)
    for k, q in enumerate(ids):
        want = TL.tile_raster(torch.from_numpy(TL.synthetic_slide(1024, 1280, seed=3 + k)), max_patches=9, **R.SLIDE_KW)
        assert 0 < len(want) <= 9 and sorted(got[q]) == list(range(len(want)))
        assert np.array_equal(np.stack([got[q][i] for i in range(len(want))]), want.tiles.numpy()), q
        assert os.path.isdir(os.path.join(patches, q, q.replace(".svs", ".db")))
        mask = np.load(os.path.join(masks, q, "mask.npy"))
        assert mask.dtype == bool and np.array_equal(mask, want.mask.numpy() != 0)
        with open(os.path.join(patches, q, "qc.csv")) as f:
            rows = list(csv.reader(f))
        assert len(rows) == 1 + len(want) and [[int(v) for v in row[2:8]] for row in rows[1:]] == \
            np.concatenate([want.origins, want.qc[:, :4]], axis=1).tolist()
    # a second run (in this process) skips both slides and writes nothing; with a fresh --patch_path it reuses the masks
    import tile_slides
    assert tile_slides.run(tile_slides.parse_args(cmd[2:])) == []
    again = str(tmp_path / "again")
    written = tile_slides.run(tile_slides.parse_args(cmd[2:4] + ["1", "--synthetic_size", "1024x1280", "--seed", "3", "--patch_path", again,
                                                                 "--mask_path", masks, "--patch_size", "64", "--app_mag", "40",
                                                                 "--max_patches_per_slide", "9"]))
    assert written == [os.path.join(again, ids[0], ids[0].replace(".svs", ".db"))]
    store = PD.open_tile_store(written[0])
    back = [PD.decompress_and_deserialize(store[str(i).encode()]).numpy().transpose(1, 2, 0) for i in range(len(got[ids[0]]))]
    assert np.array_equal(np.stack(back), np.stack([got[ids[0]][i] for i in range(len(got[ids[0]]))]))
