"""What tests/test_refmask_cpu.py and tests/test_refmask_gpu.py share (no test in here): a numpy restatement of the rule of
include/nid/nid_refmask.h -- one ufunc per IEEE operation, written from the header, not from csrc/nid_depth_check.h --
and the scene both files classify."""
import numpy as np

F5000 = 1.0 / 5000
CALLER, OCCLUDED, THROUGH, DILATED = 1, 2, 4, 8
COUNT_NAMES = ("n_valid", "n_caller", "n_occluded", "n_through", "n_dilated", "n_masked")


def pose_M(p):
    """the rows of [R|t] as lm::pose_record makes them (csrc/nid_lm_step.h), operation for operation"""
    p = np.asarray(p, dtype=np.float64)
    x, y, z, w = p[0], p[1], p[2], p[3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1 - (tyy + tzz), txy - twz, txz + twy, p[4],
                     txy + twz, 1 - (txx + tzz), tyz - twx, p[5],
                     txz - twy, tyz + twx, 1 - (txx + tyy), p[6]])


def dilate_any(S, d):
    """pixels with a pixel of S within Chebyshev distance d, the window clipped at the image"""
    rows, cols = S.shape
    pad = np.zeros((rows + 2 * d, cols + 2 * d), dtype=bool)
    pad[d:d + rows, d:d + cols] = S
    out = np.zeros_like(S)
    for dr in range(2 * d + 1):
        for dc in range(2 * d + 1):
            out |= pad[dr:dr + rows, dc:dc + cols]
    return out


def restate(cfg, d0, factor0, T16, d1, factor1, pose7, tol_abs, tol_rel, classes, dilate, accumulate, mask=None):
    """(final plane [rows, cols] u8, counts dict, margin): steps 1 - 4 of nid_refmask.h.  margin: the smallest distance of
    any valid pixel from a threshold its class depends on -- zc from 0, u + 0.5 and v + 0.5 from an integer (pixels), dz from
    +-tol (metres) --, so that a caller can see that no decision of the scene hangs on a last bit."""
    rows, cols = cfg.rows, cfg.cols
    T = np.asarray(T16, dtype=np.float64).reshape(16)
    d0 = np.asarray(d0, dtype=np.uint16).reshape(rows, cols)
    d1f = np.asarray(d1, dtype=np.uint16).reshape(-1)
    old = np.zeros((rows, cols), dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8).reshape(rows, cols)
    M = pose_M(pose7)
    r = np.arange(rows, dtype=np.float64)[:, None] * np.ones((1, cols))
    c = np.arange(cols, dtype=np.float64)[None, :] * np.ones((rows, 1))
    with np.errstate(all="ignore"):
        z = d0.astype(np.float64) * factor0                                   # 1.
        valid = ~((z < 0.01) | (z > 100))
        x0 = z * (c - cfg.cx) / cfg.fx
        y0 = z * (r - cfg.cy) / cfg.fy
        X = ((T[0] * x0 + T[4] * y0) + T[8] * z) + T[12]
        Y = ((T[1] * x0 + T[5] * y0) + T[9] * z) + T[13]
        Z = ((T[2] * x0 + T[6] * y0) + T[10] * z) + T[14]
        xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3]                        # 2. (nid_keyframe.h's steps 2 - 5)
        yc = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7]
        zc = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11]
        front = valid & (zc > 0)
        u = (cfg.fx * xc) / zc + cfg.cx
        v = (cfg.fy * yc) / zc + cfg.cy
        cc, rr = np.floor(u + 0.5), np.floor(v + 0.5)
        inframe = front & (cc >= 0) & (cc <= cols - 1) & (rr >= 0) & (rr <= rows - 1)
        ci, ri = np.where(inframe, cc, 0).astype(np.int64), np.where(inframe, rr, 0).astype(np.int64)
        zt = d1f[ri * cols + ci].astype(np.float64) * factor1
        both = inframe & ~((zt < 0.01) | (zt > 100))
        tol = tol_abs + tol_rel * zt
        dz = zc - zt
        occluded = both & (dz > tol)
        through = both & ~occluded & (dz < -tol)
        frac_u, frac_v = (u + 0.5) - np.floor(u + 0.5), (v + 0.5) - np.floor(v + 0.5)
        margins = [np.abs(zc[valid]), np.minimum(frac_u, 1 - frac_u)[front], np.minimum(frac_v, 1 - frac_v)[front],
                   np.abs(dz - tol)[both], np.abs(dz + tol)[both]]
    margin = min([float(m.min()) for m in margins if m.size] or [np.inf])
    b = old & np.uint8(15 if accumulate else CALLER)                          # 3.
    if classes & OCCLUDED:
        b = b | (occluded.astype(np.uint8) * np.uint8(OCCLUDED))
    if classes & THROUGH:
        b = b | (through.astype(np.uint8) * np.uint8(THROUGH))
    S = (b & (OCCLUDED | THROUGH)) != 0                                       # 4.
    near = dilate_any(S, dilate) if dilate > 0 else np.zeros_like(S)
    b = np.where(S, b & np.uint8(~DILATED & 0xff), np.where(near, b | np.uint8(DILATED), b)).astype(np.uint8)
    counts = dict(n_valid=int(valid.sum()), n_caller=int(((b & CALLER) != 0).sum()), n_occluded=int(((b & OCCLUDED) != 0).sum()),
                  n_through=int(((b & THROUGH) != 0).sum()), n_dilated=int(((b & DILATED) != 0).sum()), n_masked=int((valid & (b != 0)).sum()))
    return b, counts, margin


def counts_dict(rec):
    assert int(rec["reserved"][0]) == 0 and int(rec["reserved"][1]) == 0
    return {k: int(rec[k]) for k in COUNT_NAMES}


class Scene:
    """A keyframe (the suite's small synthetic pair: image, depth with zero-depth holes, camera -> world matrix) and the
    depth map of a second, nearby view of the same surface with a NEAR OCCLUDER (1 m in front of a scene at 1.5 - 2.8 m),
    a FAR HOLE (6 m) and INVALID samples (zeros, and counts just below the validity bound) painted in.  pose: the second
    view's; pose_out: one that moves part of the keyframe out of view."""

    def __init__(self, synth, rows, cols, cell):
        pair = synth.make_pair("S", texture="analytic", rows=rows, cols=cols, cell=cell)
        self.pair, self.rows, self.cols = pair, rows, cols
        T_cw0 = np.linalg.inv(pair.T_wc0)
        self.pose0 = synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])
        self.pose = synth.perturb_pose7(self.pose0, [5e-4, -8e-4, 3e-4], [3e-3, -1.5e-3, 2e-3])
        # (with a rotation: under a pure translation u + 0.5 lands on integers exactly, the depth being counts of 1/5000 m)
        self.pose_out = synth.perturb_pose7(self.pose0, [2e-3, -3e-3, 1e-3], [0.45, 0.0, -0.35])
        self.T0 = synth.matrix_colmajor16(pair.T_wc0)
        self.dep0 = pair.depth_u16.copy()
        self.dep0[3:6, 10:50] = 0           # invalid keyframe samples
        self.dep0[rows - 1, cols - 3:] = 0  # ... also among the pixels of no cell where the shape has any
        self.dep0[60, 70:74] = [49, 0, 49, 1]
        # the second view's depth: every keyframe pixel's depth in that view, splatted like an image
        r = np.arange(rows, dtype=np.float64)[:, None]
        c = np.arange(cols, dtype=np.float64)[None, :]
        z = pair.depth_m
        P0 = np.stack([z * (c - pair.cx) / pair.fx, z * (r - pair.cy) / pair.fy, z, np.ones_like(z)], axis=-1).reshape(-1, 4)
        T_cw = synth.pose7_to_matrix(self.pose)
        zc = (P0 @ (T_cw @ pair.T_wc0).T)[:, 2].reshape(rows, cols)
        self.im1 = np.clip(np.rint(synth.render_second_view(pair.im0, z, pair.fx, pair.fy, pair.cx, pair.cy, pair.T_wc0, T_cw)), 0, 255).astype(np.uint8)
        dep1 = np.rint(synth.render_second_view(zc, z, pair.fx, pair.fy, pair.cx, pair.cy, pair.T_wc0, T_cw) * 5000.0).astype(np.uint16)
        dep1[20:52, 30:75] = 5000             # the near occluder
        dep1[70:100, 90:150] = 30000          # the far hole
        dep1[0:12, cols - 20:] = 5000         # an occluder at the image's corner: its dilation is clipped
        dep1[56:60, :] = 0                    # invalid target samples
        dep1[62, 5:11] = [49, 48, 0, 49, 1, 0]
        self.dep1 = dep1

    def cfg(self, capi, nb=16):
        p = self.pair
        return capi.NidConfig(p.rows, p.cols, p.cell, nb, 3, 0, 0, 0, p.fx, p.fy, p.cx, p.cy)
