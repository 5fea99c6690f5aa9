"""What tests/test_reffuse_cpu.py and tests/test_reffuse_gpu.py share (no test in here): a numpy restatement of part B of the
rule of include/nid/nid_reffuse.h, written from the header, not from csrc/nid_reffuse_rule.h.  Part A is
tests/reffill_restate.py's text as it is: its restate() over a keyframe without a single valid sample, guard 0 and a fresh
plane fills every hit pixel with the z-buffer's entry -- a count of 1 ... 65535 -- and leaves 0 where nothing hit.  The scene
is that file's Scene, unchanged."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("reffill_restate", os.path.join(ROOT, "tests", "reffill_restate.py"))
fr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fr)
rr = fr.rr

F5000 = fr.F5000
Scene = fr.Scene
COUNT_NAMES = ("n_target_valid", "n_splat", "n_hit", "n_valid", "n_fused", "n_gated", "n_saturated", "n_changed")
GATE_ABS, GATE_REL = fr.GUARD_ABS, fr.GUARD_REL


def zbuffer(cfg, factor0, T16, d1, factor1, pose7):
    """(z-buffer [rows, cols] i64 with 0 where nothing hit, part A's three counts, its margin): parts A.1 - 6 of nid_reffill.h"""
    holes = np.zeros((cfg.rows, cfg.cols), dtype=np.uint16)
    plane, cnt, margin = fr.restate(cfg, holes, factor0, T16, d1, factor1, pose7, 0, 0, 0, False, None)
    assert cnt["n_filled"] == cnt["n_hit"] == int((plane != 0).sum())
    return plane.astype(np.int64), {k: cnt[k] for k in COUNT_NAMES[:3]}, margin


def refined(u, S, k):
    """e: the round-half-up mean of the uploaded count and the fused ones, in integer division"""
    return (2 * (u + S) + (k + 1)) // (2 * (k + 1))


def restate(cfg, d0, factor0, T16, d1, factor1, pose7, gate_abs, gate_rel_1024, max_obs, sums=None, obs=None):
    """(SUM plane u32, OBS plane u8, FUSED plane u16, counts dict, margin): parts A and B of nid_reffuse.h.  margin: part A's
    (tests/reffill_restate.py) and the distance of the keyframe's depths from the validity test's bounds; part B is integer
    arithmetic and has none."""
    rows, cols = cfg.rows, cfg.cols
    d0 = np.asarray(d0, dtype=np.uint16).reshape(rows, cols)
    S = np.zeros((rows, cols), dtype=np.int64) if sums is None else np.asarray(sums).astype(np.int64).reshape(rows, cols)
    k = np.zeros((rows, cols), dtype=np.int64) if obs is None else np.asarray(obs).astype(np.int64).reshape(rows, cols)
    q, counts, margin = zbuffer(cfg, factor0, T16, d1, factor1, pose7)
    hit = q != 0
    u = d0.astype(np.int64)
    with np.errstate(all="ignore"):
        z0 = d0.astype(np.float64) * factor0
        valid = ~((z0 < 0.01) | (z0 > 100))
        margin = min(margin, float(fr._to_bounds(z0).min()))
    before = refined(u, S, k)
    cand = valid & hit
    saturated = cand & (k >= max_obs)
    inside = np.abs(q - u) * 1024 <= gate_abs * 1024 + gate_rel_1024 * u
    fuse = cand & ~saturated & inside
    gated = cand & ~saturated & ~inside
    S2 = S + np.where(fuse, q, 0)
    k2 = k + fuse
    e = refined(u, S2, k2)
    assert int((2 * (u + S2) + (k2 + 1))[valid].max(initial=0)) < 1 << 26
    fused = np.where(valid & (k2 > 0), e, 0)
    counts.update(n_valid=int(valid.sum()), n_fused=int(fuse.sum()), n_gated=int(gated.sum()), n_saturated=int(saturated.sum()),
                  n_changed=int((valid & (e != before)).sum()))
    return S2.astype(np.uint32), k2.astype(np.uint8), fused.astype(np.uint16), counts, margin


def counts_dict(rec):
    return {k: int(rec[k]) for k in COUNT_NAMES}


def base(fused, dep0):
    """the BASE plane: the keyframe's own samples as a fill on a fused pyramid reads them"""
    return np.where(fused != 0, fused, dep0).astype(np.uint16)


def completed(fill, fused, dep0):
    """the depth plane a filled and refined pyramid is the pyramid of"""
    return np.where(fill != 0, fill, np.where(fused != 0, fused, dep0)).astype(np.uint16)
