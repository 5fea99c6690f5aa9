"""What tests/test_refgather_cpu.py and tests/test_refgather_gpu.py share (no test in here): a numpy restatement of the rule
of include/nid/nid_refgather.h -- one ufunc per IEEE operation, written from the header, not from
csrc/nid_refgather_rule.h; both matrices go through 4 x 4 matrices and numpy's inverse, not through the library's
quaternion product.  Part B is tests/reffuse_restate.py's arithmetic (refined) restated on the gather's observation.  The
scene is tests/reffill_restate.py's Scene, unchanged."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("reffuse_restate", os.path.join(ROOT, "tests", "reffuse_restate.py"))
ur = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ur)
fr, rr = ur.fr, ur.rr

F5000 = fr.F5000
Scene = fr.Scene
COUNT_NAMES = ("n_valid", "n_sampled", "n_outside", "n_tap_refused", "n_fused", "n_gated", "n_saturated", "n_changed")
GATE_ABS, GATE_REL = ur.GATE_ABS, ur.GATE_REL
base, completed, refined = ur.base, ur.completed, ur.refined


def keyframe_to_target(T16, pose7):
    """rows of [R|t] of x_t = T_cw(target) T_wc(keyframe) x_k, through 4 x 4 matrices"""
    T_wc0 = np.asarray(T16, dtype=np.float64).reshape(4, 4).T  # (column-major 16)
    T_cw1 = np.eye(4)
    T_cw1[:3, :] = rr.pose_M(pose7).reshape(3, 4)
    return (T_cw1 @ T_wc0)[:3, :].reshape(12)


def _valid(z):
    return ~((z < 0.01) | (z > 100))


def observe(cfg, d0, factor0, T16, d1, factor1, pose7, tap_abs, tap_rel_1024):
    """steps G.0 - G.6: (q [rows, cols] i64 with 0 where the pixel has no observation, valid, outside, tap_refused, margin).
    margin: the smallest distance of any decision from its threshold -- ut, vt (pixels) and zk' / factor0 + 0.5 (counts)
    from an integer, zt from 0 and every depth that is tested for validity from 0.01 and 100 (metres).  (The tap gate is
    integer arithmetic: it has no margin.)"""
    rows, cols = cfg.rows, cfg.cols
    d0 = np.asarray(d0, dtype=np.uint16).reshape(rows, cols)
    d1 = np.asarray(d1, dtype=np.uint16).reshape(rows, cols)
    K = keyframe_to_target(T16, pose7)
    M = fr.target_to_keyframe(T16, pose7)
    r = np.arange(rows, dtype=np.float64)[:, None] * np.ones((1, cols))
    c = np.arange(cols, dtype=np.float64)[None, :] * np.ones((rows, 1))
    with np.errstate(all="ignore"):
        zk = d0.astype(np.float64) * factor0                                  # G.0, G.1
        valid = _valid(zk)
        x = zk * (c - cfg.cx) / cfg.fx
        y = zk * (r - cfg.cy) / cfg.fy
        xt = ((K[0] * x + K[1] * y) + K[2] * zk) + K[3]                       # G.2
        yt = ((K[4] * x + K[5] * y) + K[6] * zk) + K[7]
        zt = ((K[8] * x + K[9] * y) + K[10] * zk) + K[11]
        front = valid & (zt > 0)
        ut = (cfg.fx * xt) / zt + cfg.cx                                      # G.3
        vt = (cfg.fy * yt) / zt + cfg.cy
        c0, r0 = np.floor(ut), np.floor(vt)
        inframe = front & (c0 >= 0) & (c0 <= cols - 2) & (r0 >= 0) & (r0 <= rows - 2)
        a, b = ut - c0, vt - r0
        ci = np.where(inframe, c0, 0).astype(np.int64)
        ri = np.where(inframe, r0, 0).astype(np.int64)
        if rows >= 2 and cols >= 2:
            taps = [d1[ri + dr, ci + dc].astype(np.int64) for dr in (0, 1) for dc in (0, 1)]   # G.4: t00, t01, t10, t11
        else:
            taps = [np.zeros((rows, cols), dtype=np.int64)] * 4
        tz = [t.astype(np.float64) * factor1 for t in taps]
        taps_valid = _valid(tz[0]) & _valid(tz[1]) & _valid(tz[2]) & _valid(tz[3])
        lo, hi = np.minimum.reduce(taps), np.maximum.reduce(taps)
        close = (hi - lo) * 1024 <= tap_abs * 1024 + tap_rel_1024 * lo
        tap_refused = inframe & ~(taps_valid & close)
        go = inframe & taps_valid & close
        t00, t01, t10, t11 = [t.astype(np.float64) for t in taps]
        top = t00 + a * (t01 - t00)                                           # G.5
        bot = t10 + a * (t11 - t10)
        zo = (top + b * (bot - top)) * factor1
        xo = zo * (ut - cfg.cx) / cfg.fx                                      # G.6
        yo = zo * (vt - cfg.cy) / cfg.fy
        zk2 = ((M[8] * xo + M[9] * yo) + M[10] * zo) + M[11]
        qd = np.floor(zk2 / factor0 + 0.5)
        inrange = go & (qd >= 1) & (qd <= 65535)
        q = np.where(inrange, qd, 1).astype(np.int64)
        zq = q.astype(np.float64) * factor0
        sampled = inrange & _valid(zq)
        outside = valid & ~tap_refused & ~sampled
        margins = [fr._to_bounds(zk), np.abs(zt[valid]), fr._to_integer(ut)[front], fr._to_integer(vt)[front]]
        margins += [fr._to_bounds(z[inframe]) for z in tz]
        margins += [fr._to_integer(zk2 / factor0 + 0.5)[go], fr._to_bounds(zq[inrange])]
    margin = min([float(m.min()) for m in margins if m.size] or [np.inf])
    return np.where(sampled, q, 0), valid, outside, tap_refused, margin


def restate(cfg, d0, factor0, T16, d1, factor1, pose7, gate_abs, gate_rel_1024, max_obs, tap_abs, tap_rel_1024, sums=None, obs=None):
    """(SUM plane u32, OBS plane u8, FUSED plane u16, counts dict, margin): the whole rule of nid_refgather.h"""
    rows, cols = cfg.rows, cfg.cols
    d0 = np.asarray(d0, dtype=np.uint16).reshape(rows, cols)
    S = np.zeros((rows, cols), dtype=np.int64) if sums is None else np.asarray(sums).astype(np.int64).reshape(rows, cols)
    k = np.zeros((rows, cols), dtype=np.int64) if obs is None else np.asarray(obs).astype(np.int64).reshape(rows, cols)
    q, valid, outside, tap_refused, margin = observe(cfg, d0, factor0, T16, d1, factor1, pose7, tap_abs, tap_rel_1024)
    u = d0.astype(np.int64)
    before = refined(u, S, k)
    cand = q != 0                                                             # B: the cap before the gate
    saturated = cand & (k >= max_obs)
    inside = np.abs(q - u) * 1024 <= gate_abs * 1024 + gate_rel_1024 * u
    fuse = cand & ~saturated & inside
    gated = cand & ~saturated & ~inside
    S2 = S + np.where(fuse, q, 0)
    k2 = k + fuse
    e = refined(u, S2, k2)
    fused = np.where(valid & (k2 > 0), e, 0)
    counts = dict(n_valid=int(valid.sum()), n_sampled=int(cand.sum()), n_outside=int(outside.sum()), n_tap_refused=int(tap_refused.sum()),
                  n_fused=int(fuse.sum()), n_gated=int(gated.sum()), n_saturated=int(saturated.sum()),
                  n_changed=int((valid & (e != before)).sum()))
    return S2.astype(np.uint32), k2.astype(np.uint8), fused.astype(np.uint16), counts, margin


def counts_dict(rec):
    return {k: int(rec[k]) for k in COUNT_NAMES}
