"""Sentinel helpers shared by the op-by-op GPU test files (tests/test_vae_fid_ops_gpu.py, tests/test_bn_reduce_ops_gpu.py).

Outputs live inside a larger allocation pre-filled with one finite bit pattern: what a contract leaves untouched must keep it bit
for bit.  Operands live inside a larger allocation whose remainder is NaN: a row or column read past the operand shows up as a
non-finite result.  Those reads stay inside the allocation, so nothing can fault."""
import torch

from vae_fid_refs import SENTINEL, bits

DEV = "cuda:0"
SBITS = 0x5e59e2d3                                  # bits of SENTINEL


class Guarded:
    """A tensor in the middle of a larger allocation filled with `fill` (NaN around operands, SENTINEL around outputs).  The
    offsets keep 256-byte alignment.  `after` is sized by the caller to cover the farthest overrun it wants to see."""

    def __init__(self, t, fill, before=128, after=4096):
        n = t.numel()
        self.flat = torch.full((before + n + after,), fill, dtype=t.dtype, device=DEV)
        self.flat[before:before + n] = t.reshape(-1).to(DEV)
        self.t = self.flat[before:before + n].view(t.shape)
        self.before, self.n = before, n

    def surroundings_keep(self, pattern):
        head, tail = self.flat[:self.before], self.flat[self.before + self.n:]
        return bool((bits(head) == pattern).all()) and bool((bits(tail) == pattern).all())


def _out(shape, after=4096):
    return Guarded(torch.full(shape, SENTINEL, dtype=torch.float32), SENTINEL, after=after)


def _assert_sentinel(t, what):
    assert bool((bits(t) == SBITS).all()), "%s: %d elements that must stay untouched were written" % (
        what, int((bits(t) != SBITS).sum()))
