#!/usr/bin/env python3
"""tools/refmask_cost.py [--out profiles/refmask_cost.txt]: what a masking call of include/nid/nid_refmask.h costs beside its
yardstick, config A (640x480, 16 / 8 / 4 cells), 3 levels, 8 bins, ONE process on one device.

Two numbers, each the median of 20 runs behind a warm-up, every run a blocking call with a device synchronisation before
and after it, timed with the host clock:
  nid_pyr_mask_occluded with dilate 2 (both classes, accumulate off), and
  nid_pyr_promote_target -- the yardstick: a masking call runs the same reference half (k_pyr_down_depth per coarser level,
  the depth conversion and the tiling per level) plus two light kernels, a device-to-device copy fewer and 64 bytes home.
If masking costs more than twice the promotion, the file says which kernel the excess sits in: the two kernels' own times
are then estimated from calls that differ in one kernel only (dilate 0 / 8, and a clear, which runs no classification)."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINS, LEVELS = 8, 3
F = 1.0 / 5000
WARMUP, RUNS = 5, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refmask_cost.txt"))
    a = ap.parse_args()
    capi = importlib.import_module("nid-pose-estimation_amd.capi")
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    if capi.load().nid_device_count() < 1:
        print("tools/refmask_cost.py: no HIP device visible", file=sys.stderr)
        return 1
    device_synchronize = C.CDLL("libamdhip64.so").hipDeviceSynchronize  # (the runtime libnid_hip.so is linked against)

    pair = synth.make_pair("A")
    T0 = synth.matrix_colmajor16(pair.T_wc0)
    # the target's depth: the keyframe's own with a near plate and a far hole, so that both classes and the dilation have work
    dep1 = pair.depth_u16.copy()
    dep1[100:220, 150:330] = 5000
    dep1[300:400, 400:560] = 30000
    T_cw0 = np.linalg.inv(pair.T_wc0)
    pose = synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])
    pyr = capi.Pyramid.create(pair, BINS, levels=LEVELS)
    pyr.set_pair_u16(pair.depth_u16, F, pair.im0, pair.im1, T0)
    pyr.set_target_depth(dep1, F)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        t = []
        for _ in range(RUNS):
            device_synchronize()
            t0 = time.perf_counter()
            fn()
            device_synchronize()
            t.append(time.perf_counter() - t0)
        return statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3

    counts = {}

    def mask(dilate=2):
        counts["last"] = pyr.mask_occluded(pose, 0.01, 0.02, 6, dilate, False)

    t_mask = timed(mask)
    n = counts["last"]
    t_prom = timed(lambda: pyr.promote_resident_target(T0))
    lines = [f"# tools/refmask_cost.py: config A ({pair.cols}x{pair.rows}, {pair.cell}x{pair.cell} cells at level 0), {LEVELS} levels, {BINS} bins; one process, one device",
             f"# host clock around blocking calls, a device synchronisation before and after each; medians of {RUNS} runs behind {WARMUP} (min ... max), ms",
             f"nid_pyr_mask_occluded, dilate 2   {t_mask[0]:7.3f} ({t_mask[1]:.3f} ... {t_mask[2]:.3f})   "
             f"[{int(n['n_occluded'])} occluded, {int(n['n_through'])} through, {int(n['n_dilated'])} dilated of {int(n['n_valid'])} valid pixels]",
             f"nid_pyr_promote_target            {t_prom[0]:7.3f} ({t_prom[1]:.3f} ... {t_prom[2]:.3f})",
             f"ratio                             {t_mask[0] / t_prom[0]:7.2f}"]
    if t_mask[0] > 2 * t_prom[0]:
        # calls that differ in one kernel: a clear of a masked plane runs k_refmask_dilate_apply (dilate 0) and the reference
        # half but no k_refmask_classify; dilate 0 against dilate 8 moves k_refmask_dilate_apply alone
        def clear_masked():
            mask(2)
            pyr.clear_reference_mask()

        t_pair = timed(clear_masked)
        t_d0, t_d8 = timed(lambda: mask(0)), timed(lambda: mask(8))
        t_clear = t_pair[0] - t_mask[0]
        lines += ["masking costs more than twice the promotion; calls that differ in one kernel, medians in ms:",
                  f"  nid_pyr_clear_reference_mask of a masked plane (no k_refmask_classify)   {t_clear:7.3f}",
                  f"  nid_pyr_mask_occluded, dilate 0 / 8                                     {t_d0[0]:7.3f} / {t_d8[0]:7.3f}",
                  f"  k_refmask_classify: about {t_d0[0] - t_clear:.3f} ms; k_refmask_dilate_apply's dilation: about {t_d8[0] - t_d0[0]:.3f} ms for 8 pixels; "
                  f"the rest beyond the promotion ({t_clear - t_prom[0]:+.3f} ms) is k_refmask_dilate_apply's pass over the plane and the counts' way home",
                  "  the excess sits in " + ("k_refmask_classify" if t_d0[0] - t_clear > max(t_clear - t_prom[0], t_d8[0] - t_d0[0]) else "k_refmask_dilate_apply")]
    pyr.close()
    for s in lines:
        print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
