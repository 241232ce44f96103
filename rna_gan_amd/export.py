"""The output side of bulk generation on the device: generated fp32 NCHW images -> uint8 tiles in ONE launch, and a
double-buffered pinned download behind it.

``gan_utils.synthesize`` leaves fp32 NCHW images on the device; ``rg_export_images_nhwc`` + ``.cpu()`` then moves 12 bytes per
pixel across the host link and the quantisation to bytes runs in numpy on the host.  ``tiles_u8`` (rg_tile_export_u8,
rna_gan_amd/csrc/rg_export.hip) quantises and lays the batch out on the device, so 3 bytes per pixel cross the link, and
``synthesize_u8`` keeps the link busy with chunk k while chunk k + 1 is synthesised.

The arithmetic contract (include/rnagan_hip.h; restated in tests/export_refs.py), every step a separately rounded fp32 operation:

    v = (x - sub) / div                       (sub, div) = (-1, 2): the value of rg_export_images_nhwc, bit for bit;
                                              (lo, max(hi - lo, 1e-5)): the min-max normalisation of Trainer.save_image_grid
    t = v * 255 + 0.5  (rounding="round", torchvision save_image's rule)      t = v * 255  (rounding="trunc", the reference
                                                                               script's ``img *= 255; astype(uint8)``)
    byte = 0 if not t >= 0 (NaN included), 255 if t >= 255, else t truncated toward zero

Under the rounding rule a tile that went through the input transform ((b / 255 - 0.5) / 0.5) comes back as the same 256 bytes;
the truncating rule returns 63 of them one lower, so rounding is the default everywhere.

On a CPU tensor ``tiles_u8`` computes the same bytes with torch ops (callers stay testable anywhere); on a CUDA tensor there is
no fallback: the kernel runs or the call raises.  Nothing here draws from a random generator.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _abi

RG_EXPORT_PLANAR, RG_EXPORT_REVERSE, RG_EXPORT_TRUNC = (_abi.CONSTANTS["RG_EXPORT_" + k] for k in ("PLANAR", "REVERSE", "TRUNC"))
LAYOUTS = ("nhwc", "nchw")
ORDERS = ("rgb", "bgr")
ROUNDINGS = ("round", "trunc")


def export_flags(layout="nhwc", order="rgb", rounding="round"):
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s" % (LAYOUTS,))
    if order not in ORDERS:
        raise ValueError("order must be one of %s" % (ORDERS,))
    if rounding not in ROUNDINGS:
        raise ValueError("rounding must be one of %s" % (ROUNDINGS,))
    return (RG_EXPORT_PLANAR if layout == "nchw" else 0) | (RG_EXPORT_REVERSE if order == "bgr" else 0) | \
        (RG_EXPORT_TRUNC if rounding == "trunc" else 0)


def tile_args(tiles, layout, order, what):
    """(N, H, W) of uint8 tiles, (N, H, W, 3) ("nhwc") or (N, 3, H, W) ("nchw"), as the image-side functions take them; ``what``
    names the caller in the messages"""
    export_flags(layout, order)
    if not torch.is_tensor(tiles) or tiles.dim() != 4 or tiles.dtype != torch.uint8:
        raise ValueError("%s takes a uint8 (N, H, W, 3) or (N, 3, H, W) tensor" % what)
    if tiles.shape[3 if layout == "nhwc" else 1] != 3:
        raise ValueError("%s needs 3 channels in layout %s, got %s" % (what, layout, tuple(tiles.shape)))
    N = tiles.shape[0]
    H, W = (tiles.shape[1], tiles.shape[2]) if layout == "nhwc" else (tiles.shape[2], tiles.shape[3])
    return N, H, W


def rgb_numpy(tiles, layout, order):
    """a CPU tensor as (N, H, W, 3) numpy in R, G, B order (a view where possible)"""
    a = tiles.numpy()
    if layout == "nchw":
        a = a.transpose(0, 2, 3, 1)
    if order == "bgr":
        a = a[..., ::-1]
    return a


def _out_shape(shape, layout):
    N, C, H, W = shape
    return (N, H, W, C) if layout == "nhwc" else (N, C, H, W)


def tiles_u8(images, layout="nhwc", order="rgb", rounding="round", sub=-1.0, div=2.0, out=None):
    """fp32 [N][C][H][W] -> uint8 on the same device, [N][H][W][C] (layout "nhwc") or [N][C][H][W] ("nchw"); order "bgr":
    destination channel c takes source channel C - 1 - c.  One launch on the current stream, no host synchronisation.
    sub / div: Python scalars, each rounded once to fp32.  out: optional contiguous uint8 tensor of the result's shape."""
    flags = export_flags(layout, order, rounding)
    if not torch.is_tensor(images) or images.dim() != 4 or images.dtype != torch.float32:
        raise ValueError("tiles_u8 takes a float32 [N][C][H][W] tensor")
    sub, div = float(sub), float(div)
    if div == 0.0 or div != div or float(np.float32(div)) == 0.0:
        raise ValueError("div must be neither 0 nor NaN")
    N, C, H, W = images.shape
    if min(C, H, W) < 1:
        raise ValueError("tiles_u8 needs C, H, W >= 1, got %s" % (tuple(images.shape),))
    shape = _out_shape(images.shape, layout)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=images.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != images.device:
        raise ValueError("out must be a contiguous uint8 tensor of shape %s on %s" % (shape, images.device))
    if N == 0:
        return out
    if images.device.type != "cuda":
        x = images
        v = (x - torch.full_like(x, sub)) / torch.full_like(x, div)       # tensor operands: a true fp32 division, no reciprocal
        t = v * 255.0
        if rounding == "round":
            t = t + 0.5
        zero = torch.zeros_like(t)
        b = torch.where(t >= 255.0, torch.full_like(t, 255.0), torch.where(t >= 0.0, t, zero)).to(torch.uint8)
        if order == "bgr":
            b = b.flip(1)
        out.copy_(b.permute(0, 2, 3, 1) if layout == "nhwc" else b)
        return out
    src = images.contiguous()
    _abi.launch("rg_tile_export_u8", src.device, src.data_ptr(), out.data_ptr(), N, C, H, W, sub, div, flags)
    return out


def synthesize_u8(generator, noise, chunk=512, fp8=False, synth_chunk=None, qc=None, **export_kwargs):
    """Bulk synthesis delivered to the host as uint8: a generator function over ``(start, array)``, where ``array`` is a uint8
    numpy VIEW of a pinned buffer holding the tiles of noise rows start .. start + len(array) (at most ``chunk``), laid out as
    ``tiles_u8(..., **export_kwargs)`` lays them out.

    Two pinned slots with one event each and a copy stream: chunk k + 1's synthesis and export are enqueued before the host
    waits for chunk k's copy, so they run while chunk k crosses the link.  A YIELDED VIEW IS VALID ONLY UNTIL THE GENERATOR IS
    ADVANCED AGAIN: the next chunk but one lands in the same slot.  Copy what must be kept (``synthesize_u8_all`` does).
    ``noise``: (N, E) on a CUDA device.  synth_chunk: rows per ``synthesize`` call (default: ``chunk``) -- the conv kernels pick
    their tiling by batch size, so a caller whose bytes must not depend on ``chunk`` fixes this and lets ``chunk`` cut the export
    and the download only (``generate_tiles`` does).  Draws no random numbers.
    qc: None, or a dict of ``tissue.tile_stats`` settings (rgb_min, dilate, percentiles; {} for the defaults): tile quality control
    runs on each uint8 chunk where it lies on the device (rg_tile_qc) and its 12 int32 per tile travel behind the chunk; the
    generator then yields ``(start, array, rows)``, ``rows`` an int32 (len(array), 12) numpy VIEW valid as long as ``array`` is
    (``tissue.stats_from_rows`` makes a TileStats of it)."""
    from .gan_utils import synthesize
    layout = export_kwargs.get("layout", "nhwc")
    export_flags(layout, export_kwargs.get("order", "rgb"), export_kwargs.get("rounding", "round"))
    if "out" in export_kwargs:
        raise ValueError("synthesize_u8 owns its output buffers: out= is not accepted")
    if noise.device.type != "cuda":
        raise ValueError("synthesize_u8 runs the HIP generator: noise must be on a CUDA device")
    chunk = int(chunk)
    synth = chunk if synth_chunk is None else int(synth_chunk)
    if chunk < 1 or synth < 1:
        raise ValueError("chunk and synth_chunk must be >= 1")
    if qc is not None:
        from .tissue import tile_stats_device
        if set(qc) - {"rgb_min", "dilate", "percentiles"}:
            raise ValueError("qc takes rgb_min, dilate and percentiles")
        qc = dict(qc, layout=layout, order=export_kwargs.get("order", "rgb"))
    device = noise.device
    N = noise.shape[0]
    main = torch.cuda.current_stream(device)
    copy = torch.cuda.Stream(device)
    events = [torch.cuda.Event(), torch.cuda.Event()]
    dev = [None, None]            # device uint8 staging, one per slot
    pinned = [None, None]
    dev_rows, pinned_rows = [None, None], [None, None]        # qc: the stats rows of a slot
    pending = None                # (start, n, slot) of the chunk whose copy is in flight
    k = 0
    for b0 in range(0, N, synth):
        img = synthesize(generator, noise[b0:b0 + synth], chunk=synth, fp8=fp8)
        for c0 in range(0, img.shape[0], chunk):
            piece = img[c0:c0 + chunk]
            n, s = piece.shape[0], k & 1
            k += 1
            if dev[s] is None:
                shape = _out_shape((min(chunk, synth, N),) + tuple(img.shape[1:]), layout)
                dev[s] = torch.empty(shape, dtype=torch.uint8, device=device)
                pinned[s] = torch.empty(shape, dtype=torch.uint8).pin_memory()
                if qc is not None:
                    dev_rows[s] = torch.empty((shape[0], 12), dtype=torch.int32, device=device)
                    pinned_rows[s] = torch.empty((shape[0], 12), dtype=torch.int32).pin_memory()
            else:
                main.wait_event(events[s])        # the copy that read this device slot (two chunks ago) is done before it is rewritten
            tiles_u8(piece, out=dev[s][:n], **export_kwargs)
            if qc is not None:
                tile_stats_device(dev[s][:n], out=dev_rows[s][:n], **qc)
            copy.wait_stream(main)
            with torch.cuda.stream(copy):
                pinned[s][:n].copy_(dev[s][:n], non_blocking=True)
                if qc is not None:
                    pinned_rows[s][:n].copy_(dev_rows[s][:n], non_blocking=True)
                events[s].record(copy)
            if pending is not None:
                yield _delivered(pending, events, pinned, pinned_rows, qc)
            pending = (b0 + c0, n, s)
    if pending is not None:
        yield _delivered(pending, events, pinned, pinned_rows, qc)


def _delivered(pending, events, pinned, pinned_rows, qc):
    ps, pn, pslot = pending
    events[pslot].synchronize()
    if qc is None:
        return ps, pinned[pslot][:pn].numpy()
    return ps, pinned[pslot][:pn].numpy(), pinned_rows[pslot][:pn].numpy()


def synthesize_u8_all(generator, noise, chunk=512, fp8=False, synth_chunk=None, **export_kwargs):
    """The chunks of ``synthesize_u8`` copied into ONE numpy array that owns its memory."""
    out = None
    if "qc" in export_kwargs:
        raise ValueError("synthesize_u8_all returns the tiles alone: qc= is not accepted")
    for start, a in synthesize_u8(generator, noise, chunk=chunk, fp8=fp8, synth_chunk=synth_chunk, **export_kwargs):
        if out is None:
            out = np.empty((noise.shape[0],) + a.shape[1:], dtype=np.uint8)
        out[start:start + a.shape[0]] = a
    if out is None:
        raise ValueError("synthesize_u8_all needs at least one noise row")
    return out
