#!/usr/bin/env python3
"""tools/refgather_cost.py [--out profiles/refgather_cost.txt]: what a bilinear gather of include/nid/nid_refgather.h costs
beside the nearest-splat fusion and the fill, and what it buys, ONE process on one device.

1. Config A (640x480, 16 / 8 / 4 cells), 3 levels, 8 bins, tools/reffuse_cost.py's keyframe and target.  Each number is
   the median of 20 runs behind a warm-up of 5, every run a blocking call with a device synchronisation before and after
   it, timed with the host clock: nid_pyr_fuse_reference_depth_bilinear beside nid_pyr_fuse_reference_depth and
   nid_pyr_fill_reference_depth (guard 1) -- one kernel in front of the masking chain where they run two and a memset.
2. What it buys: tools/reffuse_cost.py's keyframe's life on noisy depth (120 x 168, twelve views, seeded noise of +-20
   counts), per frame with fusing off, with nearest sampling and with bilinear sampling: the tracked pose's error and the
   RMS of the keyframe's level-0 depth against its noise-free depth.  Beside it the same twelve maps fused by both host
   twins at the TRUE poses: what either observation is worth when the pose is not in the way.
(3., the benchmark against the parent's library, is bench.py's own output: profiles/refgather_cost.txt quotes it.)"""
import argparse
import ctypes as C
import importlib
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("reffuse_cost", os.path.join(ROOT, "tools", "reffuse_cost.py"))
rc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rc)

BINS, LEVELS, F = rc.BINS, rc.LEVELS, rc.F
WARMUP, RUNS = rc.WARMUP, rc.RUNS
GATE_ABS, GATE_REL, MAX_OBS = rc.GATE_ABS, rc.GATE_REL, rc.MAX_OBS
TAP_ABS, TAP_REL = 50, 20
FRAMES, NOISE = rc.FRAMES, rc.NOISE
MODES = ("off", "nearest", "bilinear")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refgather_cost.txt"))
    a = ap.parse_args()
    capi = importlib.import_module("nid-pose-estimation_amd.capi")
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    if capi.load().nid_device_count() < 1:
        print("tools/refgather_cost.py: no HIP device visible", file=sys.stderr)
        return 1
    device_synchronize = C.CDLL("libamdhip64.so").hipDeviceSynchronize  # (the runtime libnid_hip.so is linked against)

    pair = synth.make_pair("A")
    T0 = synth.matrix_colmajor16(pair.T_wc0)
    dep0 = pair.depth_u16.copy()
    for r in range(20, pair.rows - 40, 100):  # the sensor's holes: 40 x 40 blocks, 16 % of the keyframe
        for c in range(30, pair.cols - 40, 100):
            dep0[r:r + 40, c:c + 40] = 0
    dep1 = pair.depth_u16.copy()  # the target's depth: the keyframe's complete depth with a near plate and a far hole
    dep1[100:220, 150:330] = 5000
    dep1[300:400, 400:560] = 30000
    T_cw0 = np.linalg.inv(pair.T_wc0)
    pose = synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])
    pyr = capi.Pyramid.create(pair, BINS, levels=LEVELS)

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

    def gather():
        counts["gather"] = pyr.fuse_reference_depth_bilinear(pose, GATE_ABS, GATE_REL, MAX_OBS, TAP_ABS, TAP_REL)

    def fuse():
        counts["fuse"] = pyr.fuse_reference_depth(pose, GATE_ABS, GATE_REL, MAX_OBS)

    def fill():
        counts["fill"] = pyr.fill_reference_depth(pose, 1, GATE_ABS, GATE_REL, False)

    pyr.set_pair_u16(dep0, F, pair.im0, pair.im1, T0)
    pyr.set_target_depth(dep1, F)
    t_gather = timed(gather)
    t_fuse = timed(fuse)
    t_fill = timed(fill)
    t_gather2 = timed(gather)  # (once more behind the others: the order of the calls in this process does not decide)
    t_fuse2 = timed(fuse)
    g, n, nf = counts["gather"], counts["fuse"], counts["fill"]
    fmt = lambda t: f"{t[0]:7.3f} ({t[1]:.3f} ... {t[2]:.3f})"
    lines = [f"# tools/refgather_cost.py: config A ({pair.cols}x{pair.rows}, {pair.cell}x{pair.cell} cells at level 0), {LEVELS} levels, {BINS} bins; one process, one device",
             f"# host clock around blocking calls, a device synchronisation before and after each; medians of {RUNS} runs behind {WARMUP} (min ... max), ms",
             f"nid_pyr_fuse_reference_depth_bilinear          {fmt(t_gather)}   "
             f"[{int(g['n_sampled'])} sampled, {int(g['n_outside'])} outside, {int(g['n_tap_refused'])} tap-refused of {int(g['n_valid'])} valid; "
             f"{int(g['n_fused'])} fused, {int(g['n_gated'])} gated, {int(g['n_saturated'])} saturated]",
             f"nid_pyr_fuse_reference_depth                   {fmt(t_fuse)}   "
             f"[{int(n['n_fused'])} fused, {int(n['n_gated'])} gated, {int(n['n_saturated'])} saturated of {int(n['n_valid'])} valid]",
             f"nid_pyr_fill_reference_depth, guard 1          {fmt(t_fill)}   [{int(nf['n_filled'])} filled of {int(nf['n_holes'])} holes]",
             f"nid_pyr_fuse_reference_depth_bilinear, again   {fmt(t_gather2)}",
             f"nid_pyr_fuse_reference_depth, again            {fmt(t_fuse2)}",
             f"bilinear - nearest                             {t_gather[0] - t_fuse[0]:+7.3f}   again {t_gather2[0] - t_fuse2[0]:+7.3f}   "
             f"(min ... max spread: bilinear {t_gather[2] - t_gather[1]:.3f}, nearest {t_fuse[2] - t_fuse[1]:.3f})"]
    pyr.close()

    # what it buys: a keyframe's life on noisy depth maps, tracked
    rng = np.random.default_rng(7)
    rng.uniform(-1, 1, size=(rc.STARTS - 2, 6))  # (tools/reffuse_cost.py's draws up to here: the same small twists behind them)
    pol = capi.track_policy_default()
    pol.keyframe_mode, pol.min_overlap, pol.max_age = 1, 0.1, 0
    pol.min_consistent, pol.min_samples = 0.5, 1000
    spair, poses, ims, deps, clean0, sT0 = rc.noisy_sequence(synth)
    small = rng.uniform(-1, 1, size=(3, 6)) * np.array([1e-3, 1e-3, 1e-3, 2e-3, 2e-3, 2e-3])

    def rms_of(plane):
        kept = plane.astype(np.int64)
        ok = (kept > 0) & (clean0 > 0)
        return float(np.sqrt(np.mean((kept[ok] - clean0[ok]) ** 2)))

    life = {}
    for mode in MODES:
        trk = capi.Tracker.create(spair, 16, levels=3)
        trk.set_lm(10, float(np.sqrt(0.95)), [2 + len(small)] * 3)
        trk.set_twists(small)
        trk.set_policy(pol)
        trk.set_fusing(mode != "off", GATE_ABS, GATE_REL, MAX_OBS)
        trk.set_fusion_sampling(capi.REFFUSE_BILINEAR if mode == "bilinear" else capi.REFFUSE_NEAREST, TAP_ABS, TAP_REL)
        rows = []
        for k in range(FRAMES):
            r = trk.push(ims[k], deps[k], F, T_wc_first=sT0)
            err_t = float(np.linalg.norm(r["pose7"][4:] - poses[k][4:]))
            fused = int(trk.last_gather()["n_fused"]) if mode == "bilinear" else int(trk.last_fusion()["n_fused"])
            rows.append((int(r["status"]), int(r["promoted"]), err_t, rms_of(trk.pyramid.get_level_inputs(0)[0]), fused))
        life[mode] = rows
        trk.close()
    # ... and the same maps at the TRUE poses, through the two host twins
    cfg = capi.NidConfig(spair.rows, spair.cols, spair.cell, 16, 3, 0, 0, 0, spair.fx, spair.fy, spair.cx, spair.cy)
    true_rows = [(rms_of(deps[0]), 0, rms_of(deps[0]), 0)]
    Sn = Kn = Sb = Kb = None
    for k in range(1, FRAMES):
        Sn, Kn, fn_, cn = capi.reffuse_host(cfg, deps[0], F, sT0, deps[k], F, poses[k], GATE_ABS, GATE_REL, MAX_OBS, Sn, Kn)
        Sb, Kb, fb_, cb = capi.refgather_host(cfg, deps[0], F, sT0, deps[k], F, poses[k], GATE_ABS, GATE_REL, MAX_OBS, TAP_ABS, TAP_REL, Sb, Kb)
        true_rows.append((rms_of(np.where(fn_ != 0, fn_, deps[0])), int(cn["n_fused"]), rms_of(np.where(fb_ != 0, fb_, deps[0])), int(cb["n_fused"])))
    lines += [f"# a keyframe's life: {spair.cols}x{spair.rows}, 3 levels, 16 bins, {FRAMES} views, every depth map with seeded integer noise uniform in [-{NOISE}, {NOISE}] counts of 1/5000 m;",
              f"# gate {GATE_ABS} / {GATE_REL}, tap gate {TAP_ABS} / {TAP_REL}, cap {MAX_OBS}.  |t - t_true| in mm of the tracked pose7; RMS of the keyframe's level-0 depth against its noise-free depth in counts",
              "# (pixels valid in both).  The last four columns: the same maps fused by nid_reffuse_host / nid_refgather_host at the TRUE poses, all on frame 0's keyframe",
              "frame | off: status promoted   |dt|  depth RMS | nearest: status promoted   |dt|  depth RMS   fused | bilinear: status promoted   |dt|  depth RMS   fused | true poses: nearest RMS   fused  bilinear RMS   fused"]
    for k in range(FRAMES):
        o, f, b, t = life["off"][k], life["nearest"][k], life["bilinear"][k], true_rows[k]
        lines.append(f"{k:5d} | {o[0]:11d} {o[1]:8d} {o[2] * 1e3:6.3f} {o[3]:10.3f} | {f[0]:15d} {f[1]:8d} {f[2] * 1e3:6.3f} {f[3]:10.3f} {f[4]:7d} | "
                     f"{b[0]:16d} {b[1]:8d} {b[2] * 1e3:6.3f} {b[3]:10.3f} {b[4]:7d} | {t[0]:23.3f} {t[1]:7d} {t[2]:13.3f} {t[3]:7d}")
    later = [k for k in range(1, FRAMES) if all(life[m][k][0] == capi.TRACK_OK for m in MODES)]
    if later:
        mean = lambda m: statistics.mean(life[m][k][2] for k in later) * 1e3
        lines.append(f"means over the {len(later)} later frames tracked OK in all three runs: |dt| off {mean('off'):.3f}, nearest {mean('nearest'):.3f}, "
                     f"bilinear {mean('bilinear'):.3f} mm; depth RMS at the last frame off {life['off'][-1][3]:.3f}, nearest {life['nearest'][-1][3]:.3f}, "
                     f"bilinear {life['bilinear'][-1][3]:.3f} counts; at the true poses nearest {true_rows[-1][0]:.3f}, bilinear {true_rows[-1][2]:.3f} counts")
    for s in lines:
        print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
