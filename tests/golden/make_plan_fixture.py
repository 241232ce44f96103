#!/usr/bin/env python3
"""Record what the host-side launch planner answers: tests/golden/conv_plans.json (read by tests/test_conv_plan_cpu.py).

The plan queries of the stride-2 convs, the transposed convs and their weight gradients are host code: the library loads
and answers them on a machine without a GPU.  The committed table was recorded ONCE, from the commit before the planner was
refactored into one plan struct per launch; the test holds every later planner to it.  Regenerating it from the code under
test would make the test vacuous -- rerun this only for a deliberate change of a plan, and say so in that commit.

    python tests/golden/make_plan_fixture.py            # writes tests/golden/conv_plans.json

Layout of the file: per build ("bf16", "f16") the tables under default options in full, and per option setting only the rows
that differ from the default ({"table": {"<row index>": row}}).  Row i of a table belongs to the i-th shape of shapes(): the
shapes themselves are not stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_plans.json")

BATCH = (1, 2, 8, 64, 128, 256)
LOW = (2, 4, 8, 16, 32, 64, 128)                 # low-side height = width
CHANNELS = ((64, 128), (128, 64), (128, 256), (256, 512), (512, 1024), (1024, 512), (1024, 2048), (64, 64), (192, 128),
            (128, 3))                            # (O, I) of the Conv2d(I -> O) / ConvTranspose2d(O -> I) pair
# (M, K, Nout) of rg_linear_workspace_bytes: the betaVAE's layers at 19 198 genes, G.0 (128 -> 4 x 4 x 1024) at three batches
LINEAR = ((64, 19198, 6000), (64, 6000, 4000), (64, 4000, 2000), (64, 2000, 19198), (8, 19198, 6000), (8, 128, 16384),
          (64, 128, 16384), (128, 128, 16384), (256, 2048, 2000))
# (M, K_pad, Nout) of rg_gemm_nt_bf16_workspace_bytes: the same layers with K padded to 64, and a weight-gradient product
GEMM_NT = ((64, 19200, 6000), (64, 6016, 4000), (64, 2048, 19198), (6000, 64, 19200), (64, 128, 16384), (8, 128, 16384))

# name -> options set through rg_set_option (and cleared again with -1)
SETTINGS = (
    ("default", {}),
    ("conv8=0", {"conv8": 0}), ("conv8=1", {"conv8": 1}),
    ("convp=0", {"convp": 0}), ("convd=0", {"convd": 0}), ("slab16=0", {"slab16": 0}), ("conv_v1=1", {"conv_v1": 1}),
    ("conv8_blocks=512", {"conv8_blocks": 512}),
    ("wgrad8=0", {"wgrad8": 0}), ("wgrad8_blocks=512", {"wgrad8_blocks": 512}),
    ("conv8=0,conv_tile=0", {"conv8": 0, "conv_tile": 0}), ("conv8=0,conv_tile=5", {"conv8": 0, "conv_tile": 5}),
    # these changed no answer when the table was recorded (they choose between kernels whose plans answer alike): kept so
    # that they go on changing none
    ("narrow8=1", {"narrow8": 1}), ("conv_tile=0", {"conv_tile": 0}), ("conv_tile=5", {"conv_tile": 5}),
    ("wgrad8n=0", {"wgrad8n": 0}), ("wgrad8n=2", {"wgrad8n": 2}), ("wgrad_blocks=256", {"wgrad_blocks": 256}),
)

CONV_COLUMNS = ("split", "slab_dtype", "stats_rows", "workspace_bytes", "maskbits_supported")
WGRAD_COLUMNS = ("workspace_bytes", "adam_supported_1seg", "adam_supported_2seg")


def shapes(table):
    """The shapes of a table, in row order, as dicts (for messages) -- conv: both directions of every (N, low, O, I)."""
    if table == "conv":
        return [dict(up=up, N=n, low=s, O=o, I=i) for up in (0, 1) for n in BATCH for s in LOW for o, i in CHANNELS]
    if table == "wgrad":
        return [dict(N=n, low=s, O=o, I=i) for n in BATCH for s in LOW for o, i in CHANNELS]
    if table == "linear":
        return [dict(M=m, K=k, Nout=n) for m, k, n in LINEAR]
    if table == "gemm_nt":
        return [dict(M=m, K_pad=k, Nout=n) for m, k, n in GEMM_NT]
    raise KeyError(table)


TABLES = ("conv", "wgrad", "linear", "gemm_nt")


def query(lib, half):
    """All four tables under the options that are set right now."""
    dt = 1 if half == "bf16" else 2               # RG_BF16 / RG_F16: the build's 16-bit storage type
    conv = []
    for s in shapes("conv"):
        a = (s["up"], s["N"], s["low"], s["low"], s["O"], s["I"], dt, 0)
        conv.append([lib.rg_conv_split(*a), lib.rg_conv_slab_dtype(*a), lib.rg_conv_stats_rows(*a),
                     lib.rg_conv_workspace_bytes(*a),
                     lib.rg_conv_up_maskbits_supported(*a[1:]) if s["up"] else 0])
    wgrad = []
    for s in shapes("wgrad"):
        a = (s["N"], s["low"], s["low"], s["O"], s["I"])
        wgrad.append([lib.rg_conv_wgrad_workspace_bytes(*a, dt, 0), lib.rg_conv_wgrad_adam_supported(*a, 0, dt, 0),
                      lib.rg_conv_wgrad_adam_supported(*a, 1, dt, 0)])
    return {"conv": conv, "wgrad": wgrad,
            "linear": [[lib.rg_linear_workspace_bytes(m, k, n, 0)] for m, k, n in LINEAR],
            "gemm_nt": [[lib.rg_gemm_nt_bf16_workspace_bytes(m, k, n)] for m, k, n in GEMM_NT]}


def query_setting(lib, half, options):
    for k, v in options.items():
        assert lib.rg_set_option(k.encode(), v) == 0, k
    try:
        return query(lib, half)
    finally:
        for k in options:
            lib.rg_set_option(k.encode(), -1)


def record(lib, half):
    default = query_setting(lib, half, {})
    diffs = {}
    for name, options in SETTINGS[1:]:
        got = query_setting(lib, half, options)
        diffs[name] = {t: {str(i): r for i, (r, d) in enumerate(zip(got[t], default[t])) if r != d} for t in TABLES}
    return {"default": default, "diff": diffs}


def main():
    sys.path.insert(0, ROOT)
    from rna_gan_amd import _abi
    doc = {"conv_columns": CONV_COLUMNS, "wgrad_columns": WGRAD_COLUMNS,
           "builds": {half: record(_abi.load(half), half) for half in ("bf16", "f16")}}
    with open(OUT, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('"default"', '\n"default"').replace('},"', '},\n"') + "\n")
    for half, b in doc["builds"].items():
        print(half, {n: sum(len(d[t]) for t in TABLES) for n, d in b["diff"].items()})
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
