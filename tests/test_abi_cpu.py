"""CPU checks of the boundary: the library builds/loads and exports every symbol the header declares;
the ctypes prototype table covers exactly the header.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

from rna_gan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "rnagan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", src)))


def test_header_and_prototypes_agree():
    assert header_symbols() == sorted(_abi.PROTOTYPES.keys())
    # the type half: the table is derived from the header, every declared symbol has an entry and every type was mapped
    for name, (res, args) in _abi.PROTOTYPES.items():
        assert res in (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p), name
        assert None not in args and all(isinstance(a, type(ctypes.c_int)) for a in args), name
    # the scalar types and strings that no family's own test pins
    p, i, f, d, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    assert _abi.PROTOTYPES["rg_set_option"] == (i, [ctypes.c_char_p, i])
    assert _abi.PROTOTYPES["rg_last_error"] == (ctypes.c_char_p, [])
    i64 = ctypes.c_int64
    assert _abi.PROTOTYPES["rg_resize_bilinear01"] == (i, [p, i, i64, i64, i64, i64, f, f, p, i, i, i, i, i, i, p])
    assert _abi.PROTOTYPES["rg_probe_fill_bf16"] == (i, [p, z, ctypes.c_uint, p])
    assert _abi.PROTOTYPES["rg_adam_step"] == (i, [p, p, p, p, z, i, d, d, d, d, p])


def test_parser_maps_declarations_given_as_text():
    protos, consts = _abi.parse_header("""
        /* a comment with int rg_hidden(int a); inside */
        #define RG_A 7
        #define RG_B (-3)   // trailing
        #define RG_C 0x1F
        #define RG_NOT_AN_INTEGER 1.5
        #define OTHER 4
        size_t rg_a_bytes(long long n, const int dims[4], unsigned seed);
        const char* rg_b(void);
        int rg_c(const void* const* rows, const char* name,
                 int64_t stride, double x, float y, size_t n, void* stream);
    """)
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos == {"rg_a_bytes": (ctypes.c_size_t, [ctypes.c_longlong, p, ctypes.c_uint]), "rg_b": (ctypes.c_char_p, []),
                      "rg_c": (i, [p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_double, ctypes.c_float, ctypes.c_size_t, p])}
    assert consts == {"RG_A": 7, "RG_B": -3, "RG_C": 31}


@pytest.mark.parametrize("text", [
    "int rg_x(unsigned long n, void* stream);",          # a scalar type outside the list: nothing defaults to int
    "short rg_x(int n);",                                # ... as the return type
    "int rg_x(int n, char c);",
    "int rg_x(int, float slope);",                       # a parameter without a name
    "int rg_x(int n, void (*fn)(int), void* stream);",   # not of the form <ret> rg_name(<params>);
    "int rg_x(int n, void* stream)",                     # the semicolon is missing
    "int rg_x(int n);  int rg_x(float n);",              # declared twice
])
def test_parser_refuses_what_it_cannot_map(text):
    with pytest.raises(ValueError) as e:
        _abi.parse_header(text)
    assert "rg_x" in str(e.value)                        # the message carries the declaration


def test_constants_are_the_headers():
    """the values the modules had as literals before they were read from the header, written out"""
    from rna_gan_amd import amp, export, msssim
    assert (_abi.RG_F32, _abi.RG_BF16, _abi.RG_F16, _abi.RG_U8) == (0, 1, 2, 3)
    assert (_abi.ALGO_AUTO, _abi.ALGO_GENERIC, _abi.ALGO_MFMA) == (0, 1, 2)
    assert (export.RG_EXPORT_PLANAR, export.RG_EXPORT_REVERSE, export.RG_EXPORT_TRUNC) == (1, 2, 4)
    assert (msssim.BAND, msssim.COLS) == (32, 16)
    assert (amp.STATE_INTS, amp.EXP, amp.TRACKER, amp.SKIPPED, amp.LATCH, amp.FLAG, amp.SLOTS) == (12, 0, 1, 2, 4, 8, 4)
    for name, value in (("RG_OK", 0), ("RG_EINVAL", -1), ("RG_EUNSUPPORTED", -2), ("RG_EWORKSPACE", -3), ("RG_EHIP", -4),
                        ("RG_AMP_STATE_INTS", 12), ("RG_MSSSIM_BAND", 32), ("RG_EXPORT_TRUNC", 4)):
        assert _abi.CONSTANTS[name] == value and type(_abi.CONSTANTS[name]) is int, name
    assert _abi.ABI_VERSION == 618


def test_one_call_path():
    """outside the training-step backend (and dist's debug call) no module takes a stream by hand: _abi.launch does"""
    allowed = {"ops_hip.py", "vae_train.py", "amp.py", "optim.py", "train_op.py", "dist.py", "_abi.py"}
    pkg = os.path.join(ROOT, "rna_gan_amd")
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py") and fn not in allowed:
            assert ".cuda_stream" not in open(os.path.join(pkg, fn)).read(), fn
    assert ".cuda_stream" not in open(os.path.join(ROOT, "histopathology_gan.py")).read()
    assert open(os.path.join(pkg, "dist.py")).read().count(".cuda_stream") == 1      # _debug_hold's, not part of the ABI


def test_library_loads_and_exports_all():
    if not os.path.exists(_abi.LIB_PATH):
        from rna_gan_amd.build import build_library
        build_library()
    lib = _abi.load()
    assert lib.rg_version() == _abi.ABI_VERSION
    assert lib.rg_storage_dtype() == _abi.RG_BF16
    for name in header_symbols():
        assert hasattr(lib, name), name


def test_fp16_build_loads_and_exports_all_but_the_probes():
    """librnagan_hip_f16.so: the same sources with IEEE fp16 as the 16-bit storage type (BASELINE configs[3]); it reports
    RG_F16 and exports every entry point of the header except the bf16-only measurement probes."""
    if not os.path.exists(_abi.LIB_PATH_F16):
        from rna_gan_amd.build import build_library
        build_library(half="f16")
    lib = _abi.load("f16")
    assert lib.rg_version() == _abi.ABI_VERSION
    assert lib.rg_storage_dtype() == _abi.RG_F16
    for name in header_symbols():
        if name.startswith(_abi.BF16_ONLY_PREFIXES):
            continue
        assert hasattr(lib, name), name


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "rna_gan_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            txt = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in txt and "from oracle" not in txt, fn


def test_kernel_selection_options_are_known():
    """rg_set_option is host-only: every knob the header, the tools and the tests name is accepted (and cleared again),
    an unknown name is RG_EINVAL with a message."""
    lib = _abi.load()
    for name in (b"conv8", b"conv8_blocks", b"conv_tile", b"xcd", b"class_fast", b"wgrad_blocks", b"wgrad8", b"korder",
                 b"convp", b"convp_blocks", b"convd", b"convd_blocks", b"fp8_mx", b"wgrad8n", b"f32mma", b"skinny128", b"slab16", b"wslab16", b"bn_rev", b"wgrad8_mfma", b"narrow32", b"upimg", b"upimg_blocks"):
        assert lib.rg_set_option(name, 1) == 0, name
        assert lib.rg_set_option(name, -1) == 0, name
    assert lib.rg_set_option(b"no_such_knob", 1) != 0
    assert b"no_such_knob" in lib.rg_last_error()
