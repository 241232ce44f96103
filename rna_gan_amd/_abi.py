"""ctypes binding of librnagan_hip.so.  include/rnagan_hip.h is the only statement of the ABI: PROTOTYPES and CONSTANTS are
read from it at import, so a new entry point is a declaration in the header and a definition in a .hip file, nothing else.

Everything outside the training-step backend calls a stream-taking entry point through launch(); entry points without a
stream (*_ws_bytes, *_workspace_bytes, rg_msssim_plan) are called as load().name(...).

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librnagan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rnagan_hip.h")

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64,
            "long long": C.c_longlong, "unsigned": C.c_uint}
# the short names the family tests (tests/test_*_refs_cpu.py) spell their pinned prototypes with; nothing in the package uses them
_p, _i, _f, _d, _z, _l = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int64
_TYPE_WORDS = frozenset("void char short int long unsigned signed float double size_t int64_t const".split())


def _ctype(text, named, decl):
    """the ctypes type of one C parameter (``named``) or return type; anything but a pointer, an array or a _SCALARS type raises"""
    words = text.replace("*", " * ").replace("[", " [ ").split()
    if "*" in words or "[" in words:
        return C.c_char_p if words[:3] == ["const", "char", "*"] and "*" not in words[3:] and "[" not in words else C.c_void_p
    if named and (len(words) < 2 or words[-1] in _TYPE_WORDS):
        raise ValueError("rnagan_hip.h: parameter %r without a name in: %s" % (text.strip(), decl))
    ctype = _SCALARS.get(" ".join(w for w in (words[:-1] if named else words) if w != "const"))
    if ctype is None:
        raise ValueError("rnagan_hip.h: no ctypes mapping for %r in: %s" % (text.strip(), decl))
    return ctype


def parse_header(text):
    """(PROTOTYPES, CONSTANTS) of the header's text: every ``<ret> rg_name(<params>);`` as name -> (restype, [argtypes]) and every
    ``#define RG_NAME <integer literal>`` as name -> int.  A use of an rg_ name that is not such a declaration raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2).replace(" ", ""), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(RG_\w+)[ \t]+\(?[ \t]*(-?[ \t]*(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for m in re.finditer(r"([A-Za-z_][\w\s*]*?)\b(rg_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = " ".join(m.group(0).split())
        if m.group(2) in prototypes:
            raise ValueError("rnagan_hip.h: declared twice: %s" % decl)
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        prototypes[m.group(2)] = (_ctype(m.group(1), False, decl), [_ctype(p, True, decl) for p in params])
    for name in re.findall(r"\b(rg_\w+)\s*\(", text):
        if name not in prototypes:
            raise ValueError("rnagan_hip.h: %s( is not a declaration of the form `<ret> rg_name(<params>);`" % name)
    return prototypes, constants


with open(HEADER_PATH) as _header:
    PROTOTYPES, CONSTANTS = parse_header(_header.read())

RG_F32, RG_BF16, RG_F16 = CONSTANTS["RG_F32"], CONSTANTS["RG_BF16"], CONSTANTS["RG_F16"]
RG_U8 = CONSTANTS["RG_U8"]            # a source type only (rg_resize_bilinear01, rg_tile_transform)
ALGO_AUTO, ALGO_GENERIC, ALGO_MFMA = CONSTANTS["RG_ALGO_AUTO"], CONSTANTS["RG_ALGO_GENERIC"], CONSTANTS["RG_ALGO_MFMA"]

# must equal rg_version() of the library (rna_gan_amd/csrc/rg_api.hip): bumped when an existing entry point changes; one that is
# only ADDED keeps the number -- load() refuses a library that lacks it.  The one literal here: it has to disagree with a stale library
ABI_VERSION = 618

_libs = {}
LIB_PATH_F16 = os.path.join(_HERE, "librnagan_hip_f16.so")
# entry points that exist only in the bf16 build (measurement probes; the fp32 mode's bf16-plane kernels)
BF16_ONLY_PREFIXES = ("rg_probe_", "rg_split_planes", "rg_f32p_")


def load(half: str = "bf16"):
    """Load the HIP library (once per build).  half = "bf16": librnagan_hip.so; "f16": librnagan_hip_f16.so (the same sources,
    IEEE fp16 as the 16-bit storage type).  Raises RuntimeError if it cannot be loaded."""
    if half in _libs:
        return _libs[half]
    if half not in ("bf16", "f16"):
        raise ValueError("half must be 'bf16' or 'f16'")
    path = LIB_PATH if half == "bf16" else LIB_PATH_F16
    if not os.path.exists(path):
        raise RuntimeError(
            "rna_gan_amd: %s not found. Build it with `python -m rna_gan_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU / eager fallback." % path)
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise RuntimeError("rna_gan_amd: cannot load %s: %s" % (path, e))
    for name, (res, args) in PROTOTYPES.items():
        if half == "f16" and name.startswith(BF16_ONLY_PREFIXES):
            continue
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError("rna_gan_amd: symbol %s missing from %s: the library is older than this package -- rebuild "
                               "it with `python -m rna_gan_amd.build`" % (name, path))
        fn.restype = res
        fn.argtypes = args
    got = lib.rg_version()
    if got != ABI_VERSION:
        raise RuntimeError("rna_gan_amd: %s reports ABI version %d, this package binds version %d (a stale or swapped "
                           "build): rebuild it with `python -m rna_gan_amd.build`" % (path, got, ABI_VERSION))
    want = RG_BF16 if half == "bf16" else RG_F16
    if lib.rg_storage_dtype() != want:
        raise RuntimeError("rna_gan_amd: %s stores dtype code %d, expected %d (a swapped build)" % (path, lib.rg_storage_dtype(), want))
    _libs[half] = lib
    return lib


_LAST_ERR_LIBS = ("bf16", "f16")


def check(rc: int, what: str):
    if rc != 0:
        # (the error string is thread-local per library: take it from whichever loaded build has one)
        msgs = []
        for h in _LAST_ERR_LIBS:
            if h in _libs:
                m = _libs[h].rg_last_error()
                if m:
                    msgs.append(m.decode() if len(_libs) == 1 else "[%s build] %s" % (h, m.decode()))
        raise RuntimeError("rna_gan_amd: %s failed (%d): %s" % (what, rc, " | ".join(msgs) if msgs else "?"))


def launch(name: str, device, *args, half: str = "bf16"):
    """One call of the entry point ``name`` of the ``half`` build, whose LAST parameter is the stream: ``args`` are all the others,
    the call is made with ``device`` current and on torch's current stream of it, and its return code is checked under ``name``.
    A small host operand goes in as a ctypes array where the prototype says c_void_p."""
    import torch
    with torch.cuda.device(device):
        check(getattr(load(half), name)(*args, torch.cuda.current_stream(device).cuda_stream), name)


def device_key(device):
    """(type, index) of a torch device, the current device's index where it has none: the key of a per-device cache"""
    import torch
    return device.type, device.index if device.index is not None else torch.cuda.current_device()
