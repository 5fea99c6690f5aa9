"""include/nid/nid_reffill.h on the device: the plane and the counts of nid_pyr_fill_reference_depth equal nid_reffill_host's
and a numpy restatement's; a filled pyramid is the pyramid of the pair with those depth samples written in, bit for bit; a
fill is reversible and composes with the mask of nid_refmask.h; the state rules; the tracker with filling is the
composition its header states.  120 x 168 with 4 x 4 cells and three levels, and 122 x 174 with 4 x 4 cells and two levels
(two rows and six columns of level 0 belong to no cell): neither is a multiple of the kernels' 16 x 64 tile.  Sixteen bins,
the smooth texture (tests/test_keyframe_gpu.py's reasons)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("reffill_restate", os.path.join(ROOT, "tests", "reffill_restate.py"))
fr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fr)
rr = fr.rr

DELTA = float(np.sqrt(0.95))
NB = 16
F5000 = fr.F5000
GA, GR = fr.GUARD_ABS, fr.GUARD_REL
TOL_ABS, TOL_REL = 0.01, 0.02
GEOMETRY = {"W": (120, 168, 4, 3), "O": (122, 174, 4, 2)}  # rows, cols, cell_num, levels


@pytest.fixture(scope="module")
def scenes(synth):
    return {k: fr.Scene(synth, r, c, cell) for k, (r, c, cell, _) in GEOMETRY.items()}


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
    """the scene's pair (a new reference: unmasked, unfilled) and the second view's depth on the target"""
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


def _caller(s):
    """a caller's mask over part of the hole across the occluder's corner, valid pixels beside it and the last rows"""
    caller = np.zeros((s.rows, s.cols), dtype=np.uint8)
    caller[50:70, 80:100] = 7
    caller[s.rows - 2:, :] = 1
    return caller


# ---- 1. the fill equals the host twin and the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_fill_equals_the_host(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    pyr = pyramids[which, "X"]
    _fresh(pyr, s)
    assert not pyr.get_reference_fill().any()
    pyr.set_reference_mask(_caller(s))
    pyr.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 1, 0)
    mask = pyr.get_reference_mask()
    assert (mask & 1).any() and (mask & 2).any() and (mask & 8).any()
    # (pose, guard, accumulate), each on top of the plane the one before left
    calls = [(s.pose, 1, 0), (s.pose_out, 0, 1), (s.pose_out, 2, 0), (s.pose, 2, 1), (s.pose, 0, 0), (s.pose_out, 1, 0), (s.pose, 1, 1),
             (s.pose, 2, 0), (s.pose_out, 0, 0), (s.pose_out, 2, 1), (s.pose, 0, 1)]
    plane = np.zeros((s.rows, s.cols), dtype=np.uint16)
    worst = np.inf
    most = dict(n_filled=0, n_refused=0, n_new=0, collisions=0)
    for k, (pose, guard, acc) in enumerate(calls):
        what = f"{which}, call {k}: guard {guard}, accumulate {acc}"
        cnt = pyr.fill_reference_depth(pose, guard, GA, GR, acc)
        got = pyr.get_reference_fill()
        args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, pose, guard, GA, GR, bool(acc), plane)
        host, host_cnt = capi.reffill_host(*args)
        want, want_cnt, margin = fr.restate(*args)
        worst = min(worst, margin)
        print(f"{what}: {fr.counts_dict(cnt)}, smallest margin {margin:.3e}")
        assert np.array_equal(host, want) and fr.counts_dict(host_cnt) == want_cnt, f"{what}: the host twin and the restatement"
        assert np.array_equal(got, host), f"{what}: {int((got != host).sum())} entries of the plane differ from the host's"
        assert cnt.tobytes() == host_cnt.tobytes(), f"{what}: counts {cnt} / {host_cnt}"
        assert np.array_equal(pyr.get_reference_mask(), mask), f"{what}: the mask plane moved"
        # the effective reference: level 0's depth is mask ? 0 : (fill ? fill : uploaded)
        assert np.array_equal(pyr.get_level_inputs(0)[0], np.where(mask != 0, 0, np.where(got != 0, got, s.dep0)).astype(np.uint16)), what
        most = dict(n_filled=max(most["n_filled"], want_cnt["n_filled"]), n_refused=max(most["n_refused"], want_cnt["n_refused"]),
                    n_new=max(most["n_new"], want_cnt["n_new"]), collisions=max(most["collisions"], want_cnt["n_splat"] - want_cnt["n_hit"]))
        plane = got
    assert worst > 1e-9, "a decision of the scene hangs on a last bit"
    assert most["n_filled"] > 1000 and most["n_refused"] > 100 and most["n_new"] > 500 and most["collisions"] > 5000, most
    assert ((mask != 0) & (plane != 0)).any(), "no masked pixel was filled: the mask's hold on a pixel that became valid was not shown"


# ---- 2. a filled pyramid is the pyramid of the completed depth -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_filled_pyramid_equals_the_completed_depth(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    _fresh(Y, s)  # never filled
    # the second view's pose, and one that moves half of the keyframe's lower left cell out of view: what is left of that cell
    # is under 300 samples without the hole in it ([100:110, 20:40]) and over 300 with it
    poses = (s.pose, synth.perturb_pose7(s.pose0, [0, 0, 0], [-0.45, 0.3, 0]))
    unfilled = [[Y.level(l).compute_href(pose)[0].copy() for l in range(Y.levels)] for pose in poses]
    cnt = X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    fill = X.get_reference_fill()
    assert int(cnt["n_filled"]) == int((fill != 0).sum()) > 1000 and int(cnt["n_refused"]) > 0
    comp = fr.completed(fill, s.dep0)
    _fresh(Y, s, comp)
    assert _inputs(X) == _inputs(Y)
    grew, crossed = 0, 0
    for k, pose in enumerate(poses):
        ex, ey = _evaluations(X, pose), _evaluations(Y, pose)
        for l in range(X.levels):
            for name, a, b in zip(("N_c", "Href", "Hc", "Hj", "err", "J"), ex[l], ey[l]):
                assert a == b, f"{which}, level {l}: {name}"
            n_c = X.level(l).compute_href(pose)[0]
            print(f"{which}, pose {k}, level {l}: N_c unfilled {unfilled[k][l].tolist()}, filled {n_c.tolist()}")
            assert l > 0 or (n_c >= unfilled[k][l]).all()  # (level 0: a fill moves no sample that was there)
            grew += int((n_c > unfilled[k][l]).sum())
            crossed += int(((unfilled[k][l] < 300) & (n_c >= 300)).sum())
    assert grew > 0, "no cell gained a sample"
    assert crossed > 0, "no cell came back over the 300-sample threshold"
    starts = _starts(synth, s.pose)
    rx, ry = X.multistart_lm(starts, 5, DELTA), Y.multistart_lm(starts, 5, DELTA)
    assert rx[0].tobytes() == ry[0].tobytes() and rx[1].tobytes() == ry[1].tobytes() and rx[2].tobytes() == ry[2].tobytes()
    assert rx[3] == ry[3] and rx[4].tobytes() == ry[4].tobytes() and np.isfinite(rx[0]["chi2"]).any()


# ---- 3. reversible; composes with the mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_fill_is_reversible_and_composes_with_the_mask(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    _fresh(Y, s)  # never filled
    never = _inputs(Y)
    ev_never = _evaluations(Y, s.pose)
    Y.clear_reference_fill()  # nothing filled: a no-op, the reference stage stays
    for l in range(Y.levels):
        assert tuple(a.tobytes() for a in Y.level(l).evaluate(s.pose, True)) == ev_never[l][2:]
    first = X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    plane = X.get_reference_fill()
    assert plane.any() and _inputs(X) != never
    X.clear_reference_fill()
    assert not X.get_reference_fill().any() and _inputs(X) == never
    assert _evaluations(X, s.pose) == ev_never
    X.clear_reference_fill()  # twice
    assert _inputs(X) == never
    again = X.fill_reference_depth(s.pose, 1, GA, GR, 1)
    assert np.array_equal(X.get_reference_fill(), plane) and again.tobytes() == first.tobytes()
    # a new reference starts unfilled
    _fresh(X, s)
    assert not X.get_reference_fill().any() and _inputs(X) == never
    # fill, then mask == the pyramid of the completed depth, masked alike; the host's mask over the completed depth too
    X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    assert np.array_equal(X.get_reference_fill(), plane)
    comp = fr.completed(plane, s.dep0)
    _fresh(Y, s, comp)
    caller = _caller(s)
    for pyr in (X, Y):
        pyr.set_reference_mask(caller)
    cx, cy = (pyr.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0) for pyr in (X, Y))
    mask = X.get_reference_mask()
    assert np.array_equal(mask, Y.get_reference_mask()) and cx.tobytes() == cy.tobytes() and _inputs(X) == _inputs(Y)
    host, host_cnt = capi.refmask_host(cfg, comp, F5000, s.T0, s.dep1, F5000, s.pose, TOL_ABS, TOL_REL, 6, 2, False, (caller != 0).astype(np.uint8))
    assert np.array_equal(mask, host) and cx.tobytes() == host_cnt.tobytes()
    # (the filled pixels are consistent with the frame they were filled from: the mask sees them as valid samples, without a class)
    _, unfilled_cnt = capi.refmask_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, s.pose, TOL_ABS, TOL_REL, 6, 2, False, (caller != 0).astype(np.uint8))
    assert int(cx["n_valid"]) == int(unfilled_cnt["n_valid"]) + int((plane != 0).sum()), "the mask did not see the fill"
    assert np.array_equal(X.get_reference_fill(), plane), "a masking call moved the fill"
    assert np.array_equal(X.get_level_inputs(0)[0], np.where(mask != 0, 0, comp).astype(np.uint16))
    assert ((mask != 0) & (plane != 0)).any()
    # clearing the mask keeps the fill; clearing the fill keeps the mask
    X.clear_reference_mask()
    assert not X.get_reference_mask().any() and np.array_equal(X.get_reference_fill(), plane)
    assert np.array_equal(X.get_level_inputs(0)[0], comp)
    X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    X.clear_reference_fill()
    want, _ = capi.refmask_host(cfg, comp, F5000, s.T0, s.dep1, F5000, s.pose, TOL_ABS, TOL_REL, 6, 2)
    assert np.array_equal(X.get_reference_mask(), want) and not X.get_reference_fill().any()
    assert np.array_equal(X.get_level_inputs(0)[0], np.where(want != 0, 0, s.dep0).astype(np.uint16))


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------
def test_state_rules(capi, synth, scenes, pyramids):
    s = scenes["W"]
    cfg = s.cfg(capi, NB)
    levels = GEOMETRY["W"][3]
    fresh = capi.Pyramid.create(s.pair, NB, levels=levels)
    try:
        for call in (lambda: fresh.fill_reference_depth(s.pose), fresh.clear_reference_fill, fresh.get_reference_fill):
            with pytest.raises(capi.NidError, match="call order"):
                call()  # no reference
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        ctx = fresh.level(0)
        ctx.compute_href(s.pose)
        want = ctx.evaluate(s.pose, True)
        before = _inputs(fresh)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.fill_reference_depth(s.pose)  # no target depth
        assert _inputs(fresh) == before and not fresh.get_reference_fill().any()
        for a, b in zip(want, ctx.evaluate(s.pose, True)):  # the refused call left the reference, its reference stage included
            assert a.tobytes() == b.tobytes()
        # both promotions and a new pair drop the fill
        T1 = capi.pose_to_Twc16(s.pose)

        def filled():
            fresh.set_target_depth(s.dep1, F5000)
            cnt = fresh.fill_reference_depth(s.pose, 1, GA, GR, 0)
            assert int(cnt["n_filled"]) > 1000 and fresh.get_reference_fill().any()

        filled()
        fresh.promote_resident_target(T1)
        assert not fresh.get_reference_fill().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        filled()
        fresh.promote_target(s.dep1, F5000, T1)
        assert not fresh.get_reference_fill().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.clear_reference_fill()  # nothing to clear behind a promotion: the promoted depth stays
        assert np.array_equal(fresh.get_level_inputs(0)[0], s.dep1)
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        filled()
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        assert not fresh.get_reference_fill().any() and np.array_equal(fresh.get_level_inputs(0)[0], s.dep0)
        # ... and the first fill behind a promotion starts from ITS depth and matrix: the old keyframe's depth on the target
        fresh.set_target(s.im1)
        fresh.set_target_depth(s.dep1, F5000)
        fresh.promote_resident_target(T1)
        fresh.set_target_depth(s.dep0, F5000)
        cnt = fresh.fill_reference_depth(s.pose0, 1, GA, GR, 0)
        host, host_cnt = capi.reffill_host(cfg, s.dep1, F5000, T1, s.dep0, F5000, s.pose0, 1, GA, GR)
        assert np.array_equal(fresh.get_reference_fill(), host) and cnt.tobytes() == host_cnt.tobytes() and int(cnt["n_filled"]) > 100
    finally:
        fresh.close()

    # an uncollected launch on a level: the three calls refuse and change nothing; the public slots are untouched by a fill
    X = pyramids["W", "X"]
    _fresh(X, s)
    X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    plane = X.get_reference_fill()
    ctx = X.level(1)
    ctx.compute_href(s.pose)
    want = ctx.normal_equations(s.pose, DELTA)
    before = _inputs(X)
    ctx.launch(5, s.pose, DELTA)
    for call in (lambda: X.fill_reference_depth(s.pose), X.clear_reference_fill, X.get_reference_fill):
        with pytest.raises(capi.NidError, match="call order"):
            call()
    got = ctx.wait(5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert _inputs(X) == before and np.array_equal(X.get_reference_fill(), plane)
    reduced_dev, cellout_dev = ctx.slot_buffers(5)
    slot = (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    X.fill_reference_depth(s.pose_out, 2, GA, GR, 1)
    X.clear_reference_fill()
    assert slot == (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    with pytest.raises(capi.NidError, match="call order"):
        ctx.evaluate(s.pose, True)  # as behind a promotion: a reference, no reference stage
    ctx.compute_href(s.pose)
    assert np.isfinite(ctx.normal_equations(s.pose, DELTA)[2])

    # the argument rules behind a good handle
    lib = capi.load()
    q = np.ascontiguousarray(s.pose)
    dp = lambda a: a.ctypes.data_as(capi.c_dp)
    before = _inputs(X)  # (cleared above: the never-filled pyramid's)
    for guard, ga, gr in ((-1, 50, 20), (3, 50, 20), (1, -1, 20), (1, 65536, 20), (1, 50, -1), (1, 50, 1025)):
        assert lib.nid_pyr_fill_reference_depth(X.h, dp(q), guard, ga, gr, 0, None) == -1
    assert lib.nid_pyr_fill_reference_depth(X.h, None, 1, 50, 20, 0, None) == -1
    assert lib.nid_pyr_get_reference_fill_u16(X.h, None) == -1
    assert _inputs(X) == before and not X.get_reference_fill().any(), "a refused argument touched the pyramid"
    assert lib.nid_pyr_fill_reference_depth(X.h, dp(q), 2, 65535, 1024, 1, None) == 0  # counts are optional
    trk = capi.Tracker.create(s.pair, NB, levels=levels)
    try:
        for guard, ga, gr in ((-1, 50, 20), (3, 50, 20), (1, -1, 20), (1, 65536, 20), (1, 50, -1), (1, 50, 1025)):
            assert lib.nid_track_set_filling(trk.h, 1, guard, ga, gr) == -1
        assert lib.nid_track_set_filling(trk.h, 1, 2, 65535, 1024) == 0 and lib.nid_track_set_filling(trk.h, 0, 0, 0, 0) == 0
        assert lib.nid_track_last_fill(trk.h, None) == -1
        assert not any(fr.counts_dict(trk.last_fill()).values())
    finally:
        trk.close()


# ---- 5. the tracker is its composition ------------------------------------------------------------------------------------------
TRACK_ITER = 10
TWISTS = np.array([[1e-3, 0, 0, 0, 2e-3, 0], [0, -1e-3, 0, 2e-3, 0, 0], [0, 0, 1e-3, 0, 0, -2e-3]], dtype=np.float64)
STEP = ([5e-4, -8e-4, 3e-4], [3e-3, -1.5e-3, 2e-3])  # the motion from one view to the next, as a twist
MIN_OVERLAP, MIN_CONSISTENT = 0.75, 0.5
# the frame that brings a keyframe to this age is promoted, and the keyframe's fills end with it.  Three levels: 2 -- the
# second frame fills, the third is promoted (from the fourth on the occluder has these chains rejected).  Two levels: 3 --
# two frames fill one keyframe, the second on top of the first
MAX_AGE = {3: 2, 2: 3}
MASK_CLASSES, MASK_DILATE = 6, 2
FILL_GUARD = 1


class Seq:
    """tests/test_refmask_gpu.py's six views of one textured surface a few millimetres apart, an occluder from frame 3 on --
    here with holes in every frame's depth map, so that every keyframe has something to fill."""

    def __init__(self, synth, rows, cols, cell):
        pair = synth.make_pair("S", texture="analytic", rows=rows, cols=cols, cell=cell)
        self.pair = pair
        T_cw0 = np.linalg.inv(pair.T_wc0)
        self.pose = [synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])]
        for _ in range(5):
            self.pose.append(synth.perturb_pose7(self.pose[-1], *STEP))
        self.im, self.dep = [pair.im0], [pair.depth_u16.copy()]
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
        for k, dep in enumerate(self.dep):  # the sensor's holes, elsewhere in every frame
            dep[20 + 5 * k:34 + 5 * k, 100 + 4 * k:124 + 4 * k] = 0
            dep[90:100, 30 + 10 * k:50 + 10 * k] = 0
        self.T0 = synth.matrix_colmajor16(pair.T_wc0)


class Restated:
    """nid_track_push_u16's schedule under an active policy with filling and masking (nid_keyframe.h's steps, nid_reffill.h's
    fill behind the choice, nid_refmask.h's step 5e), from the Pyramid's public calls and the pose helpers"""

    def __init__(self, capi, pyr, policy, filling, classes, dilate, keep):
        self.capi, self.pyr, self.pol, self.filling, self.classes, self.dilate, self.keep = capi, pyr, policy, filling, classes, dilate, keep
        self.cur, self.prev, self.have_ref, self.frame, self.age = None, None, False, 0, 0
        self.check = (np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0, 0)
        self.mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]
        self.fill = np.zeros(1, dtype=capi.REFFILL_COUNTS_DTYPE)[0]

    def push(self, im, dep, T_first):
        capi, pyr, pol, L = self.capi, self.pyr, self.pol, self.pyr.levels
        out = dict(chi2=0.0, n_active=0, best_origin=-1, promoted=0, frame=self.frame, rounds=np.zeros(L, dtype=np.int32))
        chosen, n_checked = np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0
        mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]
        fill = np.zeros(1, dtype=capi.REFFILL_COUNTS_DTYPE)[0]
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
                    else:
                        if self.filling:  # behind the choice, in front of the mask; the first fill of a pixel stays
                            fill = pyr.fill_reference_depth(pose, FILL_GUARD, GA, GR, 1)
                        if self.classes:  # 5e.
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
        self.mask, self.fill = mask, fill
        out["pose7"] = self.cur.copy()
        self.frame += 1
        return out


def _assert_same_result(got, want, what):
    assert got["pose7"].tobytes() == want["pose7"].tobytes(), f"{what}: pose7\n{got['pose7']}\n{want['pose7']}"
    assert np.float64(got["chi2"]).tobytes() == np.float64(want["chi2"]).tobytes(), f"{what}: chi2 {got['chi2']!r} / {want['chi2']!r}"
    for name in ("n_active", "best_origin", "status", "promoted", "frame"):
        assert got[name] == want[name], f"{what}: {name} {got[name]} / {want[name]}"
    assert got["rounds"].tobytes() == want["rounds"].tobytes(), f"{what}: rounds {got['rounds']} / {want['rounds']}"


def _policy(capi, levels):
    pol = capi.track_policy_default()
    pol.keyframe_mode, pol.min_overlap, pol.max_age = 1, MIN_OVERLAP, MAX_AGE[levels]
    pol.min_consistent, pol.min_samples = MIN_CONSISTENT, 1000  # verification on: a fill trusts the chosen pose
    return pol


def _tracker(capi, pair, levels, pol):
    trk = capi.Tracker.create(pair, NB, levels=levels)
    trk.set_lm(TRACK_ITER, DELTA, [2 + len(TWISTS)] * levels)
    trk.set_twists(TWISTS)
    trk.set_policy(pol)
    return trk


@pytest.mark.parametrize("levels,masking", [(3, False), (3, True), (2, False), (2, True)])
def test_tracker_is_its_composition(capi, synth, levels, masking):
    """Six pushes under on-demand keyframes with a maximal age, verification on, an occluder from frame 3 on: every result,
    last check, last mask, last fill, fill plane, mask plane and level input equal to the restatement's, whatever the status."""
    s = Seq(synth, 120, 168, 4)
    pol = _policy(capi, levels)
    trk = _tracker(capi, s.pair, levels, pol)
    pyr = capi.Pyramid.create(s.pair, NB, levels=levels)
    classes = MASK_CLASSES if masking else 0
    try:
        assert not any(fr.counts_dict(trk.last_fill()).values())
        trk.set_filling(True, FILL_GUARD, GA, GR)
        if masking:
            trk.set_masking(MASK_CLASSES, MASK_DILATE)
        ref = Restated(capi, pyr, pol, True, classes, MASK_DILATE, [2 + len(TWISTS)] * levels)
        filled_frames, later_promotions, carried = 0, 0, 0
        for k in range(6):
            got = trk.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            want = ref.push(s.im[k], s.dep[k], s.T0)
            fill, mask = trk.last_fill(), trk.last_mask()
            plane, mplane = trk.pyramid.get_reference_fill(), trk.pyramid.get_reference_mask()
            what = f"levels {levels}, masking {masking}, push {k}"
            print(f"{what}: status {got['status']}, promoted {got['promoted']}, fill {fr.counts_dict(fill)}, mask {rr.counts_dict(mask)}, "
                  f"|pose7 - true| {np.abs(got['pose7'] - s.pose[k]).max():.3e}")
            _assert_same_result(got, want, what)
            chk = trk.last_check()
            assert chk[0].tobytes() == ref.check[0].tobytes() and chk[1:] == ref.check[1:], f"{what}: last check"
            assert mask.tobytes() == ref.mask.tobytes(), f"{what}: last mask {mask} / {ref.mask}"
            assert fill.tobytes() == ref.fill.tobytes(), f"{what}: last fill {fill} / {ref.fill}"
            assert np.array_equal(plane, pyr.get_reference_fill()), f"{what}: the fill plane"
            assert np.array_equal(mplane, pyr.get_reference_mask()), f"{what}: the mask plane"
            assert _inputs(trk.pyramid) == _inputs(pyr), f"{what}: level inputs"
            ran = got["status"] == capi.TRACK_OK and not got["promoted"]
            assert ran or not any(fr.counts_dict(fill).values()), f"{what}: counts without a fill"
            if got["promoted"]:
                assert not plane.any() and not mplane.any(), f"{what}: a promoted frame starts unfilled and unmasked"
                later_promotions += k > 0
            if ran:
                assert int(fill["n_holes"]) > 0 and int((plane != 0).sum()) == int(fill["n_filled"])
                filled_frames += int(fill["n_filled"]) > 0
                carried += int(fill["n_filled"]) > int(fill["n_new"]) > 0  # fills of an earlier frame kept beside this frame's
                lvl0 = trk.pyramid.get_level_inputs(0)[0]
                assert np.array_equal(lvl0[(plane != 0) & (mplane == 0)], plane[(plane != 0) & (mplane == 0)]), f"{what}: a fill is not in use"
            elif not got["promoted"]:
                assert np.array_equal(plane, before_plane), f"{what}: a frame without a fill moved the plane"
            before_plane = plane
        assert filled_frames >= 1, "no frame was tracked on the keyframe and filled it: nothing of the fill was shown"
        assert later_promotions >= 1, "no later frame was promoted: a keyframe's fills were never dropped"
        if levels == 2:
            assert carried >= 1, "no frame filled on top of an earlier frame's fills: accumulate was not shown"
        print(f"levels {levels}, masking {masking}: {filled_frames} frames filled, {carried} kept earlier fills, {later_promotions} later promotions")
    finally:
        pyr.close()
        trk.close()


def test_filling_off_is_the_tracker_of_nid_refmask(capi, synth):
    """filling off -- set back, or never set -- gives the bytes of nid_refmask.h's tracker and no fill"""
    s = Seq(synth, 120, 168, 4)
    pol = _policy(capi, 2)
    a, b = _tracker(capi, s.pair, 2, pol), _tracker(capi, s.pair, 2, pol)
    try:
        for t in (a, b):
            t.set_masking(MASK_CLASSES, MASK_DILATE)
        b.set_filling(True, FILL_GUARD, GA, GR)
        b.set_filling(False)
        for k in range(6):
            ra, rb = a.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0), b.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            _assert_same_result(ra, rb, f"push {k}")
            assert _inputs(a.pyramid) == _inputs(b.pyramid)
            assert np.array_equal(a.pyramid.get_reference_mask(), b.pyramid.get_reference_mask()) and a.last_mask().tobytes() == b.last_mask().tobytes()
            for t in (a, b):
                assert not any(fr.counts_dict(t.last_fill()).values()) and not t.pyramid.get_reference_fill().any()
    finally:
        a.close()
        b.close()
