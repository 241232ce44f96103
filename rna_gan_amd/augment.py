"""The input transform of the Trainer on the device: uint8 tiles in, normalised fp32 NCHW out, with D4 augmentation.

The reference normalises every tile on the host (src/histopathology_gan.py:106-109), so a batch crosses PCIe as fp32.  With
``InputTransform`` the loader hands over the uint8 tiles (a quarter of the bytes) and ONE launch of rg_tile_transform
(rna_gan_amd/csrc/rg_augment.hip) normalises them -- the same three fp32 operations as the host transform, bit-identical -- and,
under ``augment="d4"``, maps every sample by one of the eight symmetries of the square (four rotations, each with or without
a flip).  H&E tiles have no canonical orientation: the distribution of the real tiles is invariant under D4, so transforming
the reals alone shows the critic nothing the generator should not produce, and D4 needs no interpolation, so it is exact.

Code c = r + 4 f: flip left-right if f, then rotate counter-clockwise by r quarter turns, i.e.
``np.rot90(x[..., ::-1] if f else x, r, axes=(-2, -1))``.  As a source index for output pixel (i, j), T = S - 1:

    0: [i][j]      1: [j][T-i]    2: [T-i][T-j]    3: [T-j][i]
    4: [i][T-j]    5: [j][i]      6: [T-i][j]      7: [T-j][T-i]

The codes are COUNTER-BASED: the t-th augmented batch of N samples on rank ``rank`` uses
``np.random.default_rng([seed, rank, t]).integers(0, 8, size=N)``.  No generator object carries state across batches, so the
state is the batch counter alone and a resumed run continues the exact code stream on every rank from rank 0's checkpoint.

On a CPU device the same result is computed with torch ops (the Trainer stays usable without a GPU); on a CUDA device there
is no fallback: the kernel runs or the call raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi
from . import dist as D_

AUGMENTS = ("none", "d4")


def d4_apply(x, code):
    """The symmetry ``code & 7`` of the square on the last two axes of a torch tensor (a view or a copy; see the table above)."""
    code = int(code) & 7
    if code & 4:
        x = torch.flip(x, dims=(-1,))
    return torch.rot90(x, code & 3, dims=(-2, -1))


class InputTransform:
    def __init__(self, mean=0.5, std=0.5, augment="none", seed=0, rank=None):
        if augment not in AUGMENTS:
            raise ValueError("augment must be one of %s" % (AUGMENTS,))
        if float(std) == 0.0:
            raise ValueError("std must not be 0")
        self.mean, self.std = float(mean), float(std)
        self.augment = augment
        self.seed = int(seed)
        self.rank = D_.rank() if rank is None else int(rank)
        self.batches = 0                # t: augmented batches drawn so far (the whole state of the code stream)
        self.last_codes = None          # the most recent host codes (numpy int32[N]); None before the first draw

    # ------------------------------------------------------------------ the code stream
    def codes_for(self, t, n):
        """Codes of the t-th augmented batch of n samples on this rank (a pure function of seed, rank, t, n)."""
        return np.random.default_rng([self.seed, self.rank, int(t)]).integers(0, 8, size=int(n)).astype(np.int32)

    def state_dict(self):
        return {"seed": self.seed, "augment": self.augment, "batches": self.batches}

    def load_state_dict(self, state):
        self.batches = int(state["batches"])

    # ------------------------------------------------------------------ the transform
    @staticmethod
    def _check(images):
        if not torch.is_tensor(images) or images.dim() != 4:
            raise ValueError("InputTransform takes an [N][C][S][S] tensor")
        if images.shape[2] != images.shape[3]:
            raise ValueError("InputTransform takes square tiles, got %d x %d" % (images.shape[2], images.shape[3]))
        if images.dtype not in (torch.uint8, torch.float32):
            raise ValueError("InputTransform takes uint8 or float32 tiles, got %s" % images.dtype)

    def _run(self, images, device, codes):
        """codes: numpy int32[N] or None (the identity for every sample)."""
        device = torch.device(device)
        if images.dtype == torch.float32 and codes is None:
            return images                # nothing to do: the caller's tensor itself, as without a transform
        if device.type != "cuda":
            x = images.to(device)
            if x.dtype == torch.uint8:
                x = (x.float() / 255.0 - self.mean) / self.std      # the three fp32 operations of the kernel's contract
            if codes is None:
                return x
            return torch.stack([d4_apply(x[n], c) for n, c in enumerate(codes)]).contiguous() if len(codes) else x
        src = images.to(device, non_blocking=True).contiguous()
        N, C, S, _ = src.shape
        out = torch.empty((N, C, S, S), dtype=torch.float32, device=device)
        if N == 0:
            return out
        dcodes = None
        if codes is not None:
            # pinned staging from torch's caching host allocator: a block is handed out again only once the non-blocking copy
            # that read it has completed, so the host never waits and no buffer is overwritten under a copy in flight
            dcodes = torch.from_numpy(codes).pin_memory().to(device, non_blocking=True)
        _abi.launch("rg_tile_transform", device, src.data_ptr(), _abi.RG_U8 if src.dtype == torch.uint8 else _abi.RG_F32,
                    out.data_ptr(), N, C, S, 0 if dcodes is None else dcodes.data_ptr(), self.mean, self.std)
        return out

    def __call__(self, images, device):
        """One training batch: uint8 is normalised (and transformed under ``d4``), float32 is transformed under ``d4`` and
        returned as the same tensor object under ``none``.  Under ``d4`` this draws the batch's codes and advances the counter."""
        self._check(images)
        codes = None
        if self.augment == "d4":
            codes = self.codes_for(self.batches, images.shape[0])
            self.batches += 1
            self.last_codes = codes
        return self._run(images, device, codes)

    def normalize(self, images, device):
        """The code-0 transform (evaluation sets): consumes no draw."""
        self._check(images)
        return self._run(images, device, None)
