"""Shared by the op-level GPU test files: the library is built twice from the same sources (bf16 storage and IEEE fp16 storage;
a library, an instruction stream and an option table of its own each), and the 16-bit tests run on both."""
import functools
import inspect

import torch

H16 = [torch.bfloat16, torch.float16]


def ru(dtype, bf16_tol):
    """A tolerance that is "a few rounding units of the storage type": one unit is 2^-8 for bf16 and 2^-11 for fp16, so the
    fp16 build gets the bf16 number divided by 8.  Bounds on fp32 sums, means, statistics and fp32 weight gradients (summation
    order only) do not depend on the storage type and are written as plain numbers."""
    return bf16_tol / 8 if dtype == torch.float16 else bf16_tol


def fp16_twin(fn):
    """Decorator (outermost, above the parametrisations): the test takes the build's 16-bit type as a keyword (`h16` or `dtype`)
    with the bf16 default; a copy that passes torch.float16 is collected next to it as <name>_fp16[...], so the bf16 cases keep
    the ids they always had."""
    key = "h16" if "h16" in inspect.signature(fn).parameters else "dtype"
    assert key in inspect.signature(fn).parameters, fn.__name__

    @functools.wraps(fn)
    def run(*args, **kwargs):
        kwargs[key] = torch.float16
        return fn(*args, **kwargs)
    run.__name__ = run.__qualname__ = fn.__name__ + "_fp16"
    fn.__globals__[run.__name__] = run
    return fn
