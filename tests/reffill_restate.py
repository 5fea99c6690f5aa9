"""What tests/test_reffill_cpu.py and tests/test_reffill_gpu.py share (no test in here): a numpy restatement of the rule of
include/nid/nid_reffill.h -- one ufunc per IEEE operation, written from the header, not from csrc/nid_reffill_rule.h; the
matrix M goes through 4 x 4 matrices and numpy's inverse, not through the library's quaternion product -- and the scene both
files fill: tests/refmask_restate.py's, with more holes in the keyframe's depth."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("refmask_restate", os.path.join(ROOT, "tests", "refmask_restate.py"))
rr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rr)

F5000 = rr.F5000
COUNT_NAMES = ("n_target_valid", "n_splat", "n_hit", "n_holes", "n_refused", "n_new", "n_filled")
GUARD_ABS, GUARD_REL = 50, 20  # counts of the depth factor (1 cm at 1/5000 m); 1024ths: about 2 %
NONE = -1


def target_to_keyframe(T16, pose7):
    """rows of [R|t] of x_k = T_cw(keyframe) T_wc(target) x_t, through 4 x 4 matrices"""
    T_wc0 = np.asarray(T16, dtype=np.float64).reshape(4, 4).T  # (column-major 16)
    T_cw1 = np.eye(4)
    T_cw1[:3, :] = rr.pose_M(pose7).reshape(3, 4)
    return (np.linalg.inv(T_wc0) @ np.linalg.inv(T_cw1))[:3, :].reshape(12)


def _to_integer(x):
    """distance of x from the nearest integer"""
    f = x - np.floor(x)
    return np.minimum(f, 1 - f)


def _to_bounds(z):
    """distance of a depth in metres from the validity test's two bounds"""
    return np.minimum(np.abs(z - 0.01), np.abs(z - 100))


def restate(cfg, d0, factor0, T16, d1, factor1, pose7, guard, guard_abs, guard_rel_1024, accumulate, fill=None):
    """(final plane [rows, cols] u16, counts dict, margin): parts A - C of nid_reffill.h.  margin: the smallest distance of
    any decision from its threshold -- u + 0.5, v + 0.5 (pixels) and zk / factor0 + 0.5 (counts) from an integer, zk from 0
    and every depth that is tested for validity from 0.01 and 100 (metres) --, so that a caller can see that no decision of
    the scene hangs on a last bit.  (The guard is integer arithmetic: it has no margin.)"""
    rows, cols = cfg.rows, cfg.cols
    d0 = np.asarray(d0, dtype=np.uint16).reshape(rows, cols)
    d1 = np.asarray(d1, dtype=np.uint16).reshape(rows, cols)
    old = np.zeros((rows, cols), dtype=np.uint16) if fill is None else np.asarray(fill, dtype=np.uint16).reshape(rows, cols)
    M = target_to_keyframe(T16, pose7)
    r1 = np.arange(rows, dtype=np.float64)[:, None] * np.ones((1, cols))
    c1 = np.arange(cols, dtype=np.float64)[None, :] * np.ones((rows, 1))
    with np.errstate(all="ignore"):
        zt = d1.astype(np.float64) * factor1                                  # A 1.
        tvalid = ~((zt < 0.01) | (zt > 100))
        x = zt * (c1 - cfg.cx) / cfg.fx                                       # 2.
        y = zt * (r1 - cfg.cy) / cfg.fy
        xk = ((M[0] * x + M[1] * y) + M[2] * zt) + M[3]                       # 3.
        yk = ((M[4] * x + M[5] * y) + M[6] * zt) + M[7]
        zk = ((M[8] * x + M[9] * y) + M[10] * zt) + M[11]
        front = tvalid & (zk > 0)
        u = (cfg.fx * xk) / zk + cfg.cx                                       # 4.
        v = (cfg.fy * yk) / zk + cfg.cy
        c, r = np.floor(u + 0.5), np.floor(v + 0.5)
        inframe = front & (c >= 0) & (c <= cols - 1) & (r >= 0) & (r <= rows - 1)
        qd = np.floor(zk / factor0 + 0.5)                                     # 5.
        inrange = inframe & (qd >= 1) & (qd <= 65535)
        q = np.where(inrange, qd, 1).astype(np.int64)
        zq = q.astype(np.float64) * factor0
        splat = inrange & ~((zq < 0.01) | (zq > 100))
        z0 = d0.astype(np.float64) * factor0
        valid0 = ~((z0 < 0.01) | (z0 > 100))
        margins = [_to_bounds(zt), np.abs(zk[tvalid]), _to_integer(u + 0.5)[front], _to_integer(v + 0.5)[front],
                   _to_integer(zk / factor0 + 0.5)[inframe], _to_bounds(zq[inrange]), _to_bounds(z0)]
    margin = min([float(m.min()) for m in margins if m.size] or [np.inf])
    big = np.iinfo(np.int64).max
    zbuf = np.full(rows * cols, big, dtype=np.int64)                          # 6.
    idx = (np.where(splat, r, 0).astype(np.int64) * cols + np.where(splat, c, 0).astype(np.int64))[splat]
    np.minimum.at(zbuf, idx, q[splat])
    zbuf = zbuf.reshape(rows, cols)
    hit = zbuf != big
    S = np.where(hit, zbuf, np.where(valid0, d0.astype(np.int64), NONE))      # B.
    refused = np.zeros((rows, cols), dtype=bool)
    if guard > 0:
        pad = np.full((rows + 2 * guard, cols + 2 * guard), NONE, dtype=np.int64)
        pad[guard:guard + rows, guard:guard + cols] = S
        zq_ = np.where(hit, zbuf, 0)
        for dr in range(2 * guard + 1):
            for dc in range(2 * guard + 1):
                if dr == guard and dc == guard:
                    continue
                qn = pad[dr:dr + rows, dc:dc + cols]
                refused |= hit & (qn != NONE) & ((zq_ - qn) * 1024 > guard_abs * 1024 + guard_rel_1024 * qn)
    kept = ~valid0 & bool(accumulate) & (old != 0)                            # C.
    new = np.where(valid0, 0, np.where(kept, old, np.where(hit & ~refused, np.where(hit, zbuf, 0), 0))).astype(np.uint16)
    counts = dict(n_target_valid=int(tvalid.sum()), n_splat=int(splat.sum()), n_hit=int(hit.sum()), n_holes=int((~valid0).sum()),
                  n_refused=int((~valid0 & ~kept & hit & refused).sum()), n_new=int(((old == 0) & (new != 0)).sum()),
                  n_filled=int((new != 0).sum()))
    return new, counts, margin


def counts_dict(rec):
    assert int(rec["reserved"]) == 0
    return {k: int(rec[k]) for k in COUNT_NAMES}


def completed(fill, dep0):
    """the depth plane a filled pyramid is the pyramid of"""
    return np.where(fill != 0, fill, dep0).astype(np.uint16)


class Scene(rr.Scene):
    """tests/refmask_restate.py's scene with holes in the keyframe's depth: under the second view's near occluder, across
    that occluder's corner (where the guard decides), under the far surface, on plain surface, and at two image corners
    (the guard's window is clipped there)."""

    def __init__(self, synth, rows, cols, cell):
        super().__init__(synth, rows, cols, cell)
        d = self.dep0
        d[30:44, 40:60] = 0
        d[44:60, 60:90] = 0
        d[80:90, 100:120] = 0
        d[100:110, 20:40] = 0
        d[0:2, 0:3] = 0
        d[rows - 2:, cols - 5:] = 0
