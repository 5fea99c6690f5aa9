#!/usr/bin/env python3
"""tools/multistart_rate.py [--out profiles/multistart_rate.txt] [--pairs A S]: what a multi-start LM costs per chain.

For each pair and M in {1, 16, 64, 256}: wall time of one nid_multistart_lm call (M chains from seeded perturbations of
pose_init, sigma 1e-3 rad / 2e-3 m, 10 iterations; best of 5, the pair's setup excluded), rounds done, us per chain --
and, in the same process on the same device, the existing baseline: M serial nid_host_run_lm(fused=3) from the same
starts (the sum of their optimize() times, setup excluded as well).

Without --pair this is the driver: one child process per pair, each under its own time limit, the next one only if the
one before ended well (what `timeout 300 ... --pair A && timeout 300 ... --pair S` does from a shell); the children's
tables go to --out.  With --pair X: that pair's table on stdout."""
import argparse
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINS = 8
ITER = 10
CHAINS = (1, 16, 64, 256)


def starts(synth, pair, n):
    rng = np.random.default_rng(2024)
    return np.stack([synth.perturb_pose7(pair.pose_init, rng.normal(0, 1e-3, 3), rng.normal(0, 2e-3, 3)) for _ in range(n)])


def measure(cfg):
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    hostlib = importlib.import_module("nid-pose-estimation_amd.hostlib")
    pair = synth.make_pair(cfg)
    print(f"pair {cfg} ({pair.cols}x{pair.rows}, {pair.cell * pair.cell} cells, {BINS} bins), {ITER} iterations")
    print("   M | multistart call ms | rounds | us/chain | serial fused=3 ms (sum of optimize()) | us/chain | serial / multistart")
    for m in CHAINS:
        p = starts(synth, pair, m)
        hostlib.run_multistart_lm(pair, BINS, p, iterations=ITER)  # (first call: buffers)
        best, rounds = 1e9, 0
        for _ in range(5):
            res, _, rounds = hostlib.run_multistart_lm(pair, BINS, p, iterations=ITER)
            best = min(best, hostlib.last_optimize_seconds())
        assert (res["status"] != 0).all()
        hostlib.run_lm(pair, BINS, p[0], ITER, fused=3)
        serial = 1e9
        for _ in range(2):
            t = 0.0
            for k in range(m):
                hostlib.run_lm(pair, BINS, p[k], ITER, fused=3)
                t += hostlib.last_optimize_seconds()
            serial = min(serial, t)
        print(f"{m:4d} | {best * 1e3:18.3f} | {rounds:6d} | {best / m * 1e6:8.1f} | {serial * 1e3:37.3f} | {serial / m * 1e6:8.1f} | {serial / best:6.2f} x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair")
    ap.add_argument("--pairs", nargs="+", default=["A", "S"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistart_rate.txt"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per pair")
    a = ap.parse_args()
    if a.pair:
        measure(a.pair)
        return 0
    text = ["# tools/multistart_rate.py: nid_multistart_lm against M serial nid_host_run_lm(fused=3), same process, same device\n"]
    for cfg in a.pairs:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pair", cfg], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"pair {cfg}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        if r.returncode != 0:  # nothing more is started on the device behind a step that failed
            sys.stderr.write(r.stderr)
            return r.returncode
        text.append(r.stdout)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
