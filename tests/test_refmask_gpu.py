"""include/nid/nid_refmask.h on the device: the plane and the counts of nid_pyr_mask_occluded equal nid_refmask_host's and a
numpy restatement's; a masked pyramid is the pyramid of the pair with those depth samples set to 0, bit for bit; a mask
is reversible and classification reads pristine depth; the state rules; the tracker with masking is the composition its
header states.  120 x 168 with 4 x 4 cells and three levels (cells of 30 x 42 pixels, a coarsest level of one cell), and
122 x 174 with 4 x 4 cells and two levels: two rows and six columns of level 0 belong to no cell.  Sixteen bins, the smooth
texture (tests/test_keyframe_gpu.py's reasons)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("refmask_restate", os.path.join(ROOT, "tests", "refmask_restate.py"))
rr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rr)

DELTA = float(np.sqrt(0.95))
NB = 16
F5000 = rr.F5000
TOL_ABS, TOL_REL = 0.01, 0.02
GEOMETRY = {"W": (120, 168, 4, 3), "O": (122, 174, 4, 2)}  # rows, cols, cell_num, levels


@pytest.fixture(scope="module")
def scenes(synth):
    return {k: rr.Scene(synth, r, c, cell) for k, (r, c, cell, _) in GEOMETRY.items()}


@pytest.fixture(scope="module")
def pyramids(capi, scenes):
    """two pyramids per geometry, shared by the tests that need no tracker"""
    held = {(w, k): capi.Pyramid.create(s.pair, NB, levels=GEOMETRY[w][3]) for w, s in scenes.items() for k in "XY"}
    yield held
    for p in held.values():
        p.close()


def _inputs(pyr):
    return [tuple(x.tobytes() for x in pyr.get_level_inputs(l)) for l in range(pyr.levels)]


def _fresh(pyr, s, dep0=None):
    """the scene's pair (a new reference: unmasked) and the second view's depth on the target"""
    pyr.set_pair_u16(s.dep0 if dep0 is None else dep0, F5000, s.pair.im0, s.im1, s.T0)
    pyr.set_target_depth(s.dep1, F5000)


def _evaluations(pyr, pose):
    """every level's N_c, Href, entropies, error and Jacobian at `pose`, as bytes"""
    out = []
    for l in range(pyr.levels):
        ctx = pyr.level(l)
        out.append(tuple(a.tobytes() for a in ctx.compute_href(pose) + ctx.evaluate(pose, True)))
    return out


def _starts(synth, pose):
    return np.stack([pose, synth.perturb_pose7(pose, [1e-3, 0, 0], [0, 2e-3, 0]), synth.perturb_pose7(pose, [0, -1e-3, 0], [2e-3, 0, 0]),
                     synth.perturb_pose7(pose, [0, 0, 1e-3], [0, 0, -2e-3])])


# ---- 1. the mask equals the host twin and the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_mask_equals_the_host(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    pyr = pyramids[which, "X"]
    _fresh(pyr, s)
    assert not pyr.get_reference_mask().any()
    caller = np.zeros((s.rows, s.cols), dtype=np.uint8)
    caller[35:60, 60:90] = 200      # overlaps the occluder's footprint and reaches past it
    caller[s.rows - 2:, :] = 1      # the last rows: pixels of no cell where the shape has any
    pyr.set_reference_mask(caller)
    plane = pyr.get_reference_mask()
    assert np.array_equal(plane, (caller != 0).astype(np.uint8))
    # (pose, classes, dilate, accumulate), each on top of the plane the one before left
    calls = [(s.pose, 6, 0, 0), (s.pose, 2, 1, 0), (s.pose, 4, 8, 0), (s.pose, 6, 8, 0), (s.pose, 2, 0, 0), (s.pose_out, 6, 1, 0),
             (s.pose, 2, 0, 1), (s.pose_out, 4, 8, 1), (s.pose, 6, 1, 1), (s.pose, 4, 1, 0), (s.pose_out, 2, 8, 0), (s.pose, 0, 8, 0)]
    worst = np.inf
    most = dict(n_occluded=0, n_through=0, n_dilated=0)
    for k, (pose, classes, dilate, acc) in enumerate(calls):
        what = f"{which}, call {k}: classes {classes}, dilate {dilate}, accumulate {acc}"
        cnt = pyr.mask_occluded(pose, TOL_ABS, TOL_REL, classes, dilate, acc)
        got = pyr.get_reference_mask()
        args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, pose, TOL_ABS, TOL_REL, classes, dilate, bool(acc), plane)
        host, host_cnt = capi.refmask_host(*args)
        want, want_cnt, margin = rr.restate(*args)
        worst = min(worst, margin)
        print(f"{what}: {rr.counts_dict(cnt)}, smallest margin {margin:.3e}")
        assert np.array_equal(host, want) and rr.counts_dict(host_cnt) == want_cnt, f"{what}: the host twin and the restatement"
        assert np.array_equal(got, host), f"{what}: {int((got != host).sum())} bytes of the plane differ from the host's"
        assert cnt.tobytes() == host_cnt.tobytes(), f"{what}: counts {cnt} / {host_cnt}"
        assert np.array_equal(got & 1, plane & 1), f"{what}: the caller's bit moved"
        # the effective reference: level 0's depth is pristine-or-0
        assert np.array_equal(pyr.get_level_inputs(0)[0], np.where(got != 0, 0, s.dep0).astype(np.uint16)), what
        for name in most:
            most[name] = max(most[name], want_cnt[name])
        plane = got
    assert worst > 1e-9, "a decision of the scene hangs on a last bit"
    assert most["n_occluded"] > 500 and most["n_through"] > 500 and most["n_dilated"] > 100, most
    assert np.array_equal(plane, (caller != 0).astype(np.uint8)), "classes 0 without accumulate leaves the caller's bit alone"


# ---- 2. a masked pyramid is the pyramid of the zeroed depth ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_masked_pyramid_equals_the_zeroed_depth(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    caller = np.zeros((s.rows, s.cols), dtype=np.uint8)
    caller[90:, 150:] = 1  # (reaches the pixels of no cell where the shape has any)
    X.set_reference_mask(caller)
    cnt = X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    plane = X.get_reference_mask()
    assert int(cnt["n_masked"]) > 2000 and (plane & 1).any() and (plane & 2).any() and (plane & 4).any() and (plane & 8).any()
    zeroed = np.where(plane != 0, 0, s.dep0).astype(np.uint16)
    z0 = s.dep0.astype(np.float64) * F5000
    assert int(((plane != 0) & ~((z0 < 0.01) | (z0 > 100))).sum()) == int(cnt["n_masked"]), "n_masked: the valid samples the mask takes out"
    _fresh(Y, s, zeroed)
    assert _inputs(X) == _inputs(Y)
    for pose in (s.pose, s.pair.pose_init):
        ex, ey = _evaluations(X, pose), _evaluations(Y, pose)
        for l in range(X.levels):
            for name, a, b in zip(("N_c", "Href", "Hc", "Hj", "err", "J"), ex[l], ey[l]):
                assert a == b, f"{which}, level {l}: {name}"
    n_c = X.level(0).compute_href(s.pose)[0]
    assert (n_c >= 300).any() and n_c.sum() < s.rows * s.cols - int(cnt["n_masked"]) + 1
    starts = _starts(synth, s.pose)
    rx, ry = X.multistart_lm(starts, 5, DELTA), Y.multistart_lm(starts, 5, DELTA)
    assert rx[0].tobytes() == ry[0].tobytes() and rx[1].tobytes() == ry[1].tobytes() and rx[2].tobytes() == ry[2].tobytes()
    assert rx[3] == ry[3] and rx[4].tobytes() == ry[4].tobytes() and np.isfinite(rx[0]["chi2"]).any()


# ---- 3. reversible; classification reads pristine depth ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_mask_is_reversible(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    _fresh(Y, s)  # never masked
    never = _inputs(Y)
    ev_never = _evaluations(Y, s.pose)
    Y.clear_reference_mask()  # nothing masked: a no-op, the reference stage stays
    for l in range(Y.levels):
        ctx = Y.level(l)
        assert tuple(a.tobytes() for a in ctx.evaluate(s.pose, True)) == ev_never[l][2:]
    first = X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    plane = X.get_reference_mask()
    assert plane.any() and _inputs(X) != never
    again = X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)  # on the masked pyramid: the rule reads pristine depth
    assert np.array_equal(X.get_reference_mask(), plane) and again.tobytes() == first.tobytes()
    X.clear_reference_mask()
    assert not X.get_reference_mask().any()
    assert _inputs(X) == never
    assert _evaluations(X, s.pose) == ev_never
    X.clear_reference_mask()  # twice
    assert _inputs(X) == never
    third = X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    assert np.array_equal(X.get_reference_mask(), plane) and third.tobytes() == first.tobytes()
    X.set_reference_mask(np.zeros_like(plane))  # a caller's empty mask clears the derived bits too
    assert not X.get_reference_mask().any() and _inputs(X) == never


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------
def test_state_rules(capi, synth, scenes, pyramids):
    s = scenes["W"]
    levels = GEOMETRY["W"][3]
    zeros = np.zeros((s.rows, s.cols), dtype=np.uint8)
    fresh = capi.Pyramid.create(s.pair, NB, levels=levels)
    try:
        for call in (lambda: fresh.mask_occluded(s.pose), lambda: fresh.set_reference_mask(zeros), fresh.clear_reference_mask, fresh.get_reference_mask):
            with pytest.raises(capi.NidError, match="call order"):
                call()  # no reference
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        ctx = fresh.level(0)
        ctx.compute_href(s.pose)
        want = ctx.evaluate(s.pose, True)
        before = _inputs(fresh)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.mask_occluded(s.pose)  # no target depth
        assert _inputs(fresh) == before and not fresh.get_reference_mask().any()
        for a, b in zip(want, ctx.evaluate(s.pose, True)):  # the refused call left the reference, its reference stage included
            assert a.tobytes() == b.tobytes()
        # a promotion and a new pair drop the mask, the caller's bit included
        T1 = capi.pose_to_Twc16(s.pose)
        caller = zeros.copy()
        caller[10:20, 10:20] = 1

        def masked():
            fresh.set_target_depth(s.dep1, F5000)
            fresh.set_reference_mask(caller)
            cnt = fresh.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 1, 0)
            assert int(cnt["n_masked"]) > 100 + 1000 and fresh.get_reference_mask().any()

        masked()
        fresh.promote_resident_target(T1)
        assert not fresh.get_reference_mask().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        masked()
        fresh.promote_target(s.dep1, F5000, T1)
        assert not fresh.get_reference_mask().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.clear_reference_mask()  # nothing to clear behind a promotion: the promoted depth stays
        assert np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        masked()
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        assert not fresh.get_reference_mask().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep0)
        # ... and the first mask behind the new reference starts from its depth, not from an older pristine copy
        fresh.set_target(s.im1)
        fresh.set_target_depth(s.dep1, F5000)
        fresh.promote_resident_target(T1)
        fresh.set_target_depth(s.dep1, F5000)
        cnt = fresh.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 0, 0)
        host, host_cnt = capi.refmask_host(s.cfg(capi, NB), s.dep1, F5000, T1, s.dep1, F5000, s.pose, TOL_ABS, TOL_REL, 6, 0)
        assert np.array_equal(fresh.get_reference_mask(), host) and cnt.tobytes() == host_cnt.tobytes()
    finally:
        fresh.close()

    # an uncollected launch on a level: the four calls refuse and change nothing; the public slots are untouched by a mask
    X = pyramids["W", "X"]
    _fresh(X, s)
    X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 2, 1, 0)
    plane = X.get_reference_mask()
    ctx = X.level(1)
    ctx.compute_href(s.pose)
    want = ctx.normal_equations(s.pose, DELTA)
    before = _inputs(X)
    ctx.launch(5, s.pose, DELTA)
    for call in (lambda: X.mask_occluded(s.pose), lambda: X.set_reference_mask(zeros), X.clear_reference_mask, X.get_reference_mask):
        with pytest.raises(capi.NidError, match="call order"):
            call()
    got = ctx.wait(5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert _inputs(X) == before and np.array_equal(X.get_reference_mask(), plane)
    reduced_dev, cellout_dev = ctx.slot_buffers(5)
    slot = (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    X.clear_reference_mask()
    assert slot == (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    with pytest.raises(capi.NidError, match="call order"):
        ctx.evaluate(s.pose, True)  # as behind a promotion: a reference, no reference stage
    ctx.compute_href(s.pose)
    got = ctx.normal_equations(s.pose, DELTA)
    assert np.isfinite(got[2])

    # the argument rules behind a good handle
    lib = capi.load()
    q =np.ascontiguousarray(s.pose)
    dp = lambda a: a.ctypes.data_as(capi.c_dp)
    before = _inputs(X)  # (cleared above: the never-masked pyramid's)
    for classes, dilate in ((1, 0), (8, 0), (7, 0), (-2, 0), (6, -1), (6, 9)):
        assert lib.nid_pyr_mask_occluded(X.h, dp(q), 0.01, 0.02, classes, dilate, 0, None) == -1
    for bad in (-1e-9, np.nan, np.inf):
        assert lib.nid_pyr_mask_occluded(X.h, dp(q), bad, 0.02, 6, 0, 0, None) == -1
        assert lib.nid_pyr_mask_occluded(X.h, dp(q), 0.01, bad, 6, 0, 0, None) == -1
    assert lib.nid_pyr_mask_occluded(X.h, None, 0.01, 0.02, 6, 0, 0, None) == -1
    assert lib.nid_pyr_set_reference_mask_u8(X.h, None) == -1 and lib.nid_pyr_get_reference_mask_u8(X.h, None) == -1
    assert _inputs(X) == before, "a refused argument touched the pyramid"
    assert lib.nid_pyr_mask_occluded(X.h, dp(q), 0.01, 0.02, 6, 8, 1, None) == 0  # counts are optional
    trk = capi.Tracker.create(s.pair, NB, levels=levels)
    try:
        for classes, dilate in ((1, 0), (8, 0), (-2, 0), (6, -1), (6, 9)):
            assert lib.nid_track_set_masking(trk.h, classes, dilate) == -1
        assert lib.nid_track_set_masking(trk.h, 6, 8) == 0 and lib.nid_track_set_masking(trk.h, 0, 0) == 0
        assert lib.nid_track_last_mask(trk.h, None) == -1
        assert not any(rr.counts_dict(trk.last_mask()).values())
    finally:
        trk.close()


# ---- 5. the tracker is its composition ------------------------------------------------------------------------------------------
TRACK_ITER = 10
TWISTS = np.array([[1e-3, 0, 0, 0, 2e-3, 0], [0, -1e-3, 0, 2e-3, 0, 0], [0, 0, 1e-3, 0, 0, -2e-3]], dtype=np.float64)
STEP = ([5e-4, -8e-4, 3e-4], [3e-3, -1.5e-3, 2e-3])  # the motion from one view to the next, as a twist
MIN_OVERLAP, MIN_CONSISTENT = 0.75, 0.5
MASK_CLASSES, MASK_DILATE = 6, 2


class Seq:
    """Six views of one textured surface a few millimetres apart: frame 0 is the keyframe; from frame 3 on an occluder --
    a bright plate 1 m from the camera, in front of a scene 1.5 - 2.8 m away -- stands in the image and in the depth map."""

    def __init__(self, synth, rows, cols, cell):
        pair = synth.make_pair("S", texture="analytic", rows=rows, cols=cols, cell=cell)
        self.pair = pair
        T_cw0 = np.linalg.inv(pair.T_wc0)
        self.pose = [synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])]
        for _ in range(5):
            self.pose.append(synth.perturb_pose7(self.pose[-1], *STEP))
        self.im, self.dep = [pair.im0], [pair.depth_u16]
        r = np.arange(rows, dtype=np.float64)[:, None]
        c = np.arange(cols, dtype=np.float64)[None, :]
        z = pair.depth_m
        P0 = np.stack([z * (c - pair.cx) / pair.fx, z * (r - pair.cy) / pair.fy, z, np.ones_like(z)], axis=-1).reshape(-1, 4)
        args = (pair.depth_m, pair.fx, pair.fy, pair.cx, pair.cy, pair.T_wc0)
        for k, p in enumerate(self.pose[1:], start=1):
            T_cw = synth.pose7_to_matrix(p)
            im = np.clip(np.rint(synth.render_second_view(pair.im0, *args, T_cw)), 0, 255).astype(np.uint8)
            zc = (P0 @ (T_cw @ pair.T_wc0).T)[:, 2].reshape(rows, cols)
            dep = np.rint(synth.render_second_view(zc, *args, T_cw) * 5000.0).astype(np.uint16)
            if k >= 3:
                c0 = 40 + 6 * (k - 3)  # it moves on between the frames
                im[44:76, c0:c0 + 36] = 230
                dep[44:76, c0:c0 + 36] = 5000
            self.im.append(im)
            self.dep.append(dep)
        self.T0 = synth.matrix_colmajor16(pair.T_wc0)


class Restated:
    """nid_track_push_u16's schedule under an active policy with masking (nid_keyframe.h's steps, nid_refmask.h's step 5e),
    from the Pyramid's public calls and the pose helpers"""

    def __init__(self, capi, pyr, policy, classes, dilate, keep):
        self.capi, self.pyr, self.pol, self.classes, self.dilate, self.keep = capi, pyr, policy, classes, dilate, keep
        self.cur, self.prev, self.have_ref, self.frame, self.age = None, None, False, 0, 0
        self.check = (np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0, 0)
        self.mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]

    def push(self, im, dep, T_first):
        capi, pyr, pol, L = self.capi, self.pyr, self.pol, self.pyr.levels
        out = dict(chi2=0.0, n_active=0, best_origin=-1, promoted=0, frame=self.frame, rounds=np.zeros(L, dtype=np.int32))
        chosen, n_checked = np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0
        mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]
        pyr.set_target(im)
        if not self.have_ref:
            pyr.promote_target(dep, F5000, T_first)
            self.cur, self.prev, self.have_ref = capi.pose_from_Twc16(T_first), None, True
            out.update(status=capi.TRACK_FIRST, promoted=1)
        else:
            assert dep is not None and (pol.keyframe_mode != 0 or pol.min_consistent > 0)  # (the other branches: tests/test_keyframe_gpu.py)
            pyr.set_target_depth(dep, F5000)
            cur = self.cur
            pred = cur if self.prev is None else capi.pose_compose(capi.pose_compose(cur, capi.pose_inverse(self.prev)), cur)
            starts = np.stack([pred, cur] + [capi.pose_perturb(pred, tw) for tw in TWISTS])
            res, origin, rounds, best, _ = pyr.multistart_lm(starts, TRACK_ITER, DELTA, keep=self.keep)
            out.update(rounds=rounds, best_origin=best)
            res0, org0 = res[L - 1], origin[L - 1]
            if best >= 0:
                ok = [k for k in range(len(res0)) if res0["n_active"][k] > 0 and np.isfinite(res0["chi2"][k])]
                order = sorted(ok, key=lambda k: (res0["chi2"][k] / float(res0["n_active"][k]), k))
                m = len(order) if pol.min_consistent > 0 else 1
                tot, _ = pyr.depth_check(res0["pose7"][order[:m]], pol.tol_abs, pol.tol_rel, cells=False)
                n_checked = m
                passes = [int(t["n_both"]) >= pol.min_samples and float(t["n_consistent"]) >= pol.min_consistent * float(t["n_both"]) for t in tot]
                pick = (passes.index(True) if True in passes else None) if pol.min_consistent > 0 else 0
                if pick is None:
                    out.update(status=capi.TRACK_REJECTED, best_origin=int(org0[order[0]]))
                    self.prev, chosen = None, tot[0]
                else:
                    k, t = order[pick], tot[pick]
                    chosen = t
                    pose = res0["pose7"][k].copy()
                    promote = (pol.keyframe_mode == 0 or float(t["n_inframe"]) < pol.min_overlap * float(t["n_ref"])
                               or (pol.max_age > 0 and self.age + 1 >= pol.max_age))
                    if promote:
                        pyr.promote_resident_target(capi.pose_to_Twc16(pose))
                    elif self.classes:  # 5e.
                        mask = pyr.mask_occluded(pose, pol.tol_abs, pol.tol_rel, self.classes, self.dilate, 0)
                    out.update(status=capi.TRACK_OK, best_origin=int(org0[k]), chi2=float(res0["chi2"][k]), n_active=int(res0["n_active"][k]),
                               promoted=int(promote))
                    self.prev, self.cur = cur, pose
            else:
                out.update(status=capi.TRACK_LOST)
                self.prev = None
        if out["promoted"]:
            self.age = 0
        elif out["status"] == capi.TRACK_OK:
            self.age += 1
        self.check = (chosen, n_checked, self.age)
        self.mask = mask
        out["pose7"] = self.cur.copy()
        self.frame += 1
        return out


def _assert_same_result(got, want, what):
    assert got["pose7"].tobytes() == want["pose7"].tobytes(), f"{what}: pose7\n{got['pose7']}\n{want['pose7']}"
    assert np.float64(got["chi2"]).tobytes() == np.float64(want["chi2"]).tobytes(), f"{what}: chi2 {got['chi2']!r} / {want['chi2']!r}"
    for name in ("n_active", "best_origin", "status", "promoted", "frame"):
        assert got[name] == want[name], f"{what}: {name} {got[name]} / {want[name]}"
    assert got["rounds"].tobytes() == want["rounds"].tobytes(), f"{what}: rounds {got['rounds']} / {want['rounds']}"


def _policy(capi, verified):
    pol = capi.track_policy_default()
    pol.keyframe_mode, pol.min_overlap = 1, MIN_OVERLAP
    if verified:
        pol.min_consistent, pol.min_samples = MIN_CONSISTENT, 1000
    return pol


def _tracker(capi, pair, levels, pol):
    trk = capi.Tracker.create(pair, NB, levels=levels)
    trk.set_lm(TRACK_ITER, DELTA, [2 + len(TWISTS)] * levels)
    trk.set_twists(TWISTS)
    trk.set_policy(pol)
    return trk


# (levels 2: the geometry on which tests/test_keyframe_gpu.py's chains hold the pose; levels 3: this file's)
@pytest.mark.parametrize("levels,verified", [(3, False), (3, True), (2, False), (2, True)])
def test_tracker_is_its_composition(capi, synth, levels, verified):
    """Six pushes under on-demand keyframes, an occluder from frame 3 on: every result, last check, last mask, mask plane and
    level input equal to the restatement's, whatever the status."""
    s = Seq(synth, 120, 168, 4)
    pol = _policy(capi, verified)
    trk = _tracker(capi, s.pair, levels, pol)
    pyr = capi.Pyramid.create(s.pair, NB, levels=levels)
    try:
        trk.set_masking(MASK_CLASSES, MASK_DILATE)
        ref = Restated(capi, pyr, pol, MASK_CLASSES, MASK_DILATE, [2 + len(TWISTS)] * levels)
        masked_frames = 0
        for k in range(6):
            got = trk.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            want = ref.push(s.im[k], s.dep[k], s.T0)
            mask, plane = trk.last_mask(), trk.pyramid.get_reference_mask()
            print(f"levels {levels}, verified {verified}, push {k}: status {got['status']}, promoted {got['promoted']}, mask {rr.counts_dict(mask)}, "
                  f"|pose7 - true| {np.abs(got['pose7'] - s.pose[k]).max():.3e}")
            what = f"levels {levels}, verified {verified}, push {k}"
            _assert_same_result(got, want, what)
            chk = trk.last_check()
            assert chk[0].tobytes() == ref.check[0].tobytes() and chk[1:] == ref.check[1:], f"{what}: last check"
            assert mask.tobytes() == ref.mask.tobytes(), f"{what}: last mask {mask} / {ref.mask}"
            assert np.array_equal(plane, pyr.get_reference_mask()), f"{what}: the mask plane"
            assert _inputs(trk.pyramid) == _inputs(pyr), f"{what}: level inputs"
            ran = got["status"] == capi.TRACK_OK and not got["promoted"]
            assert ran or not any(rr.counts_dict(mask).values()), f"{what}: counts without a step 5e"
            if got["promoted"]:
                assert not plane.any(), f"{what}: a promoted frame starts unmasked"
            if ran:
                masked_frames += 1
                assert int(mask["n_valid"]) > 0 and int((plane != 0).sum()) >= int(mask["n_masked"])
                if k >= 3 and np.abs(got["pose7"] - s.pose[k]).max() < 5e-3:  # tracked near the truth: the plate's footprint is masked
                    assert int(mask["n_occluded"]) > 500, f"{what}: the occluder was not masked"
        if levels == 2:
            assert masked_frames >= 1, "no frame was tracked on the keyframe: nothing of step 5e was shown"
    finally:
        pyr.close()
        trk.close()


def test_masking_off_is_the_tracker_of_nid_keyframe(capi, synth):
    """classes == 0 -- set back, or never set -- gives the bytes of nid_keyframe.h's tracker and no mask"""
    s = Seq(synth, 120, 168, 4)
    pol = _policy(capi, False)
    a, b = _tracker(capi, s.pair, 2, pol), _tracker(capi, s.pair, 2, pol)
    try:
        b.set_masking(MASK_CLASSES, MASK_DILATE)
        b.set_masking(0, 0)
        for k in range(6):
            ra, rb = a.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0), b.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            _assert_same_result(ra, rb, f"push {k}")
            assert _inputs(a.pyramid) == _inputs(b.pyramid)
            ca, cb = a.last_check(), b.last_check()
            assert ca[0].tobytes() == cb[0].tobytes() and ca[1:] == cb[1:]
            for t in (a, b):
                assert not any(rr.counts_dict(t.last_mask()).values()) and not t.pyramid.get_reference_mask().any()
    finally:
        a.close()
        b.close()
