#!/usr/bin/env python3
"""Worst |err| / bound per op and build from the output of an op-level GPU test file run with `-s`.

    python -m pytest tests/test_bn_reduce_ops_gpu.py -q -s > log.txt
    python tools/op_error_table.py log.txt > table.txt

Reads the lines the tests print as "RATIO <op> <case> <value>" (and "RECORD ..." lines, copied as they are) and prints one row
per (op, build) with the case of the worst ratio: the body of profiles/bn_reduce_op_errors.txt.  The bounds are derived in the
tests; this table only documents the headroom."""
import collections
import re
import sys


def main(path):
    worst, records = collections.OrderedDict(), []
    for line in open(path):
        for m in re.finditer(r"RATIO (\S+) (\S+) ([0-9.eE+-]+)", line):
            op, case, v = m.group(1), m.group(2), float(m.group(3))
            build = next((b for b in ("bf16", "fp16", "f32") if b in re.split(r"[/ ]", case)), "f32")
            if (op, build) not in worst or v > worst[(op, build)][0]:
                worst[(op, build)] = (v, case)
        m = re.search(r"RECORD (.*)", line)
        if m:
            records.append(m.group(1).strip())
    print("# columns: op   build   worst ratio   case")
    for (op, build), (v, case) in worst.items():
        print("%-34s %-5s %8.4f  %s" % (op, build, v, case))
    for r in records:
        print("record  " + r)


if __name__ == "__main__":
    main(sys.argv[1])
