#!/usr/bin/env python3
"""Where the 16-bit gates of tests/test_critic_plain_train_gpu.py::test_two_iterations_vs_oracle come from: its own protocol
(two iterations against the CPU oracle at in_size 32 / step 64 / enc 128 / batch 16, clip on the second) over consecutive
unselected seeds, per precision the loss error |hip - oracle| / (|oracle| + 0.5) and the per-tensor update cosine of every seed,
the worst of each, and twice the worst -- the gate.

    python tools/critic_plain_tolerance.py [--seeds 24] [--precisions bf16,fp16] [--out profiles/critic_plain_tolerance.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=24)
ap.add_argument("--precisions", default="bf16,fp16")
ap.add_argument("--out", default=None)
a = ap.parse_args()
import test_critic_plain_train_gpu as T      # noqa: E402  (the protocol lives next to the test that asserts the gate)

lines = ["BatchNorm-free critic, two iterations vs the CPU oracle, seeds 0..%d, in_size %d / step %d / enc %d / batch %d"
         % (a.seeds - 1, T.IN_SIZE, T.STEP, T.ENC, T.N),
         "loss error = |hip - oracle| / (|oracle| + 0.5), worst of the 6 losses; cosine = per-tensor update cosine after iteration 0"]
LARGE = 4096      # a cosine over fewer elements counts sign agreements of a handful of Adam steps: +-1 for the 1-element head bias
for precision in a.precisions.split(","):
    lines.append("")
    lines.append("%s  seed  loss_err  (which)  min_cos  (tensor)            min_cos >= %d elements  (tensor)       zero penalty bias grads"
                 % (precision, LARGE))
    worst_e, worst_c, worst_l = 0.0, 1.0, 1.0
    for seed in range(a.seeds):
        errs, cos, steps, zero_bias = T.two_iterations(seed, precision)
        k = min(cos, key=cos.get)
        big = {n: c for n, c in cos.items() if T.numel_of(n) >= LARGE}
        kl = min(big, key=big.get)
        which = ["g0", "d0", "gp0", "g1", "d1", "gp1"][errs.index(max(errs))]
        lines.append("%s  %4d  %.3e  %-7s  %.5f  %-20s %.5f  %-20s %s" % (precision, seed, max(errs), which, cos[k], k, big[kl], kl, zero_bias))
        print(lines[-1], flush=True)
        worst_e, worst_c, worst_l = max(worst_e, max(errs)), min(worst_c, cos[k]), min(worst_l, big[kl])
    lines.append("%s  worst loss error %.3e -> gate %.3e;  worst cosine %.5f -> gate cos >= %.5f;  worst cosine of the tensors with >= %d "
                 "elements %.5f -> gate cos >= %.5f"
                 % (precision, worst_e, 2 * worst_e, worst_c, 1 - 2 * (1 - worst_c), LARGE, worst_l, 1 - 2 * (1 - worst_l)))
    print(lines[-1], flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
