#!/usr/bin/env python3
"""tools/reffill_cost.py [--out profiles/reffill_cost.txt]: what a fill of include/nid/nid_reffill.h costs beside its
yardsticks, config A (640x480, 16 / 8 / 4 cells), 3 levels, 8 bins, ONE process on one device.

Each number is the median of 20 runs behind a warm-up, every run a blocking call with a device synchronisation before and
after it, timed with the host clock:
  nid_pyr_fill_reference_depth with guard 1 (accumulate off) on a keyframe with 16 % of its depth missing,
  nid_pyr_mask_occluded with dilate 2 and nid_pyr_promote_target -- a fill runs the masking call's chain behind two
  kernels and three in-stream fills or copies of its own --, and
  whole frames through nid_track_push_u16 at 16 starts under on-demand keyframes with verification, filling on and off.
If the fill costs more than twice the masking call, the file says where the excess sits: calls that differ in one part only
(a clear of a filled plane runs the chain without the two kernels and the z-buffer's fill; guard 0 against guard 2 moves
k_reffill_apply's window alone)."""
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
GUARD_ABS, GUARD_REL = 50, 20
STARTS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reffill_cost.txt"))
    a = ap.parse_args()
    capi = importlib.import_module("nid-pose-estimation_amd.capi")
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    if capi.load().nid_device_count() < 1:
        print("tools/reffill_cost.py: no HIP device visible", file=sys.stderr)
        return 1
    device_synchronize = C.CDLL("libamdhip64.so").hipDeviceSynchronize  # (the runtime libnid_hip.so is linked against)

    pair = synth.make_pair("A")
    T0 = synth.matrix_colmajor16(pair.T_wc0)
    dep0 = pair.depth_u16.copy()
    for r in range(20, pair.rows - 40, 100):  # the sensor's holes: 40 x 40 blocks, 16 % of the keyframe
        for c in range(30, pair.cols - 40, 100):
            dep0[r:r + 40, c:c + 40] = 0
    # the target's depth: the keyframe's complete depth with a near plate and a far hole (tools/refmask_cost.py's)
    dep1 = pair.depth_u16.copy()
    dep1[100:220, 150:330] = 5000
    dep1[300:400, 400:560] = 30000
    T_cw0 = np.linalg.inv(pair.T_wc0)
    pose = synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])
    pyr = capi.Pyramid.create(pair, BINS, levels=LEVELS)

    def fresh():
        pyr.set_pair_u16(dep0, F, pair.im0, pair.im1, T0)
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

    def fill(guard=1):
        counts["last"] = pyr.fill_reference_depth(pose, guard, GUARD_ABS, GUARD_REL, False)

    fresh()
    t_fill = timed(fill)
    n = counts["last"]
    t_mask = timed(lambda: pyr.mask_occluded(pose, 0.01, 0.02, 6, 2, False))
    t_prom = timed(lambda: pyr.promote_resident_target(T0))
    fmt = lambda t: f"{t[0]:7.3f} ({t[1]:.3f} ... {t[2]:.3f})"
    lines = [f"# tools/reffill_cost.py: config A ({pair.cols}x{pair.rows}, {pair.cell}x{pair.cell} cells at level 0), {LEVELS} levels, {BINS} bins; one process, one device",
             f"# host clock around blocking calls, a device synchronisation before and after each; medians of {RUNS} runs behind {WARMUP} (min ... max), ms",
             f"nid_pyr_fill_reference_depth, guard 1   {fmt(t_fill)}   "
             f"[{int(n['n_filled'])} filled, {int(n['n_refused'])} refused of {int(n['n_holes'])} holes; {int(n['n_splat'])} splats on {int(n['n_hit'])} pixels]",
             f"nid_pyr_mask_occluded, dilate 2         {fmt(t_mask)}",
             f"nid_pyr_promote_target                  {fmt(t_prom)}",
             f"fill / mask                             {t_fill[0] / t_mask[0]:7.2f}"]
    if t_fill[0] > 2 * t_mask[0]:
        fresh()

        def clear_filled():
            fill(1)
            pyr.clear_reference_fill()

        t_pair = timed(clear_filled)
        t_one = timed(fill)
        t_g0, t_g2 = timed(lambda: fill(0)), timed(lambda: fill(2))
        t_clear = t_pair[0] - t_one[0]
        lines += ["the fill costs more than twice the masking call; calls that differ in one part, medians in ms:",
                  f"  nid_pyr_clear_reference_fill of a filled plane (the chain, no fill kernel, no z-buffer)   {t_clear:7.3f}",
                  f"  nid_pyr_fill_reference_depth, guard 0 / 2                                              {t_g0[0]:7.3f} / {t_g2[0]:7.3f}",
                  f"  the z-buffer's fill, k_reffill_splat and k_reffill_apply without a window: about {t_g0[0] - t_clear:.3f} ms; "
                  f"the guard's window: about {t_g2[0] - t_g0[0]:.3f} ms for 2 pixels; the chain behind them {t_clear:.3f} ms against {t_mask[0]:.3f} ms for the masking call"]
    pyr.close()

    # whole frames: the keyframe, then the same second frame over and over (it never ages out and always overlaps)
    rng = np.random.default_rng(7)
    twists = rng.uniform(-1, 1, size=(STARTS - 2, 6)) * np.array([1e-3, 1e-3, 1e-3, 2e-3, 2e-3, 2e-3])
    pol = capi.track_policy_default()
    pol.keyframe_mode, pol.min_overlap, pol.max_age = 1, 0.1, 0
    pol.min_consistent, pol.min_samples = 0.5, 1000
    frames = {}
    for filling in (False, True):
        trk = capi.Tracker.create(pair, BINS, levels=LEVELS)
        trk.set_lm(10, float(np.sqrt(0.95)), [STARTS] * LEVELS)
        trk.set_twists(twists)
        trk.set_policy(pol)
        trk.set_filling(filling, 1, GUARD_ABS, GUARD_REL)
        trk.push(pair.im0, dep0, F, T_wc_first=T0)
        ran = {"fills": 0, "ok": 0}

        def push():
            r = trk.push(pair.im1, dep1, F)
            ran["ok"] += r["status"] == capi.TRACK_OK and not r["promoted"]
            ran["fills"] += int(trk.last_fill()["n_target_valid"]) > 0

        frames[filling] = (timed(push), dict(ran))
        trk.close()
    for filling in (False, True):
        t, ran = frames[filling]
        lines.append(f"nid_track_push_u16, {STARTS} starts, filling {'on ' if filling else 'off'}   {fmt(t)}   "
                     f"[{ran['ok']} of {WARMUP + RUNS} frames tracked on the keyframe, {ran['fills']} ran a fill]")
    lines.append(f"filling on - off                        {frames[True][0][0] - frames[False][0][0]:+7.3f}")
    for s in lines:
        print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
