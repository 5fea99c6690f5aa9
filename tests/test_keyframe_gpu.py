"""include/nid/nid_keyframe.h on the device: nid_pyr_depth_check equals nid_depth_check_host record for record, leaves the
evaluations alone and obeys its state rules; nid_pyr_promote_target equals nid_pyr_promote_target_u16; the tracker under a
policy is the composition of public calls its header states, keeps a keyframe while the overlap lasts and refuses a frame
whose depth contradicts its pose.  120 x 160 (one case 120 x 168), 4 x 4 cells, TWO levels: three would make the coarsest
level one cell, on which LM wanders.  Sixteen bins, the smooth texture, no illumination change and a
few millimetres of motion between near views: measured, 16 cells of 30 x 40 pixels hold a chain at the true pose only
then, and only from a start within about 5e-3 of it -- with eight bins or the illumination change LM leaves the true pose
for a false minimum of lower cost, which is what the verification is for but not what a behaviour test can stand on."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = float(np.sqrt(0.95))
NB = 16
LEVELS = 2
F5000 = 1.0 / 5000
TRACK_ITER = 10
TWISTS = np.array([[1e-3, 0, 0, 0, 2e-3, 0], [0, -1e-3, 0, 2e-3, 0, 0], [0, 0, 1e-3, 0, 0, -2e-3]], dtype=np.float64)
KEEP = [2 + len(TWISTS), 2 + len(TWISTS)]
STEP = ([5e-4, -8e-4, 3e-4], [3e-3, -1.5e-3, 2e-3])  # the motion from one near view to the next, as a twist
TOL_ABS, TOL_REL = 0.01, 0.02  # nid_track_policy_default's
# The far view's motion against the second near view (a twist on its pose): 0.45 m to the side and 0.35 m forward in front of
# a scene 1.5 ... 2.8 m away.  MIN_OVERLAP lies between the overlaps n_inframe / n_ref nid_depth_check_host gives at the
# ground-truth poses against frame 0 (computed on the CPU when this test was written): the three near views 1.0000 each
# -- 0.25 above --, the far view 0.5845 -- 0.17 below (120 x 168: 1.0000 and 0.5913).
# Against MIN_CONSISTENT: the consistent fraction n_consistent / n_both of the second near view with its own depth map is
# 1.0000, with the far view's depth map 0.1102 (120 x 168: 0.1049) -- the far camera stands 0.35 m nearer to everything.
FAR_TWIST = ([0.0, 0.0, 0.0], [0.45, 0.0, -0.35])
MIN_OVERLAP = 0.75
MIN_CONSISTENT = 0.5


class Seq:
    """Views of one textured surface: frame 0 is the pair's reference (image, depth, camera -> world matrix); frames 1 - 3
    are near views, frame 4 the far view, each with its image, ITS OWN depth map -- the surface's depth in that view,
    splatted like the image -- and its true world -> camera pose."""

    def __init__(self, synth, pair):
        self.pair = pair
        T_cw0 = np.linalg.inv(pair.T_wc0)
        self.pose = [synth.pose7_from_Rt(T_cw0[:3, :3], T_cw0[:3, 3])]
        for _ in range(3):
            self.pose.append(synth.perturb_pose7(self.pose[-1], *STEP))
        self.pose.append(synth.perturb_pose7(self.pose[2], *FAR_TWIST))
        self.im, self.dep = [pair.im0], [pair.depth_u16]
        rows, cols = pair.rows, pair.cols
        r = np.arange(rows, dtype=np.float64)[:, None]
        c = np.arange(cols, dtype=np.float64)[None, :]
        z = pair.depth_m
        P0 = np.stack([z * (c - pair.cx) / pair.fx, z * (r - pair.cy) / pair.fy, z, np.ones_like(z)], axis=-1).reshape(-1, 4)
        args = (pair.depth_m, pair.fx, pair.fy, pair.cx, pair.cy, pair.T_wc0)
        for p in self.pose[1:]:
            T_cw = synth.pose7_to_matrix(p)
            self.im.append(np.clip(np.rint(synth.render_second_view(pair.im0, *args, T_cw)), 0, 255).astype(np.uint8))
            zc = (P0 @ (T_cw @ pair.T_wc0).T)[:, 2].reshape(rows, cols)  # every reference pixel's depth in this view
            self.dep.append(np.rint(synth.render_second_view(zc, *args, T_cw) * 5000.0).astype(np.uint16))
        self.T0 = synth.matrix_colmajor16(pair.T_wc0)

    def cfg(self, capi):
        p = self.pair
        return capi.NidConfig(p.rows, p.cols, p.cell, NB, 3, 0, 0, 0, p.fx, p.fy, p.cx, p.cy)


@pytest.fixture(scope="module")
def seqs(synth):
    return {"S": Seq(synth, synth.make_pair("S", texture="analytic")),
            "W": Seq(synth, synth.make_pair("S", texture="analytic", rows=120, cols=168, cell=4))}


@pytest.fixture(scope="module")
def pyramids(capi, seqs):
    """two pyramids per geometry, shared by the tests that need no tracker"""
    held = {(w, k): capi.Pyramid.create(s.pair, NB, levels=LEVELS) for w, s in seqs.items() for k in "XY"}
    yield held
    for p in held.values():
        p.close()


def _inputs(pyr):
    return [tuple(x.tobytes() for x in pyr.get_level_inputs(l)) for l in range(LEVELS)]


def _batch(synth, s, n, seed):
    """n poses around the second frame's: small and large motions, a NaN pose and a pose that looks away from the scene"""
    rng = np.random.default_rng(seed)
    poses = [s.pose[1]]
    while len(poses) < n:
        scale = (1.0, 10.0, 60.0)[len(poses) % 3]
        poses.append(synth.perturb_pose7(s.pose[1], rng.normal(0, 2e-3 * scale, 3), rng.normal(0, 5e-3 * scale, 3)))
    poses = np.array(poses)
    if n >= 3:
        poses[n // 2] = np.array([0, 1.0, 0, 0, 0, 0, 0.0])  # half a turn about y: the scene is behind the camera
        poses[n - 1, 2] = np.nan
    return poses


def _host(capi, s, points, dep, poses, tol_abs=TOL_ABS, tol_rel=TOL_REL):
    cfg = s.cfg(capi)
    got = [capi.depth_check_host(cfg, points, dep, F5000, q, tol_abs, tol_rel) for q in poses]
    return np.array([t for t, _ in got]), np.stack([c for _, c in got])


# ---- 1. the device's counts are the host's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n", [("S", 1), ("S", 17), ("S", 256), ("W", 17)])
def test_depth_check_equals_the_host(capi, synth, seqs, pyramids, which, n):
    assert capi.NID_MAX_BATCH == 256
    s = seqs[which]
    pyr = pyramids[which, "X"]
    pyr.set_pair_u16(s.dep[0], F5000, s.im[0], s.im[1], s.T0)
    dep1 = s.dep[1].copy()
    dep1[10:30, 20:60] = 4000    # a nearer and a farther patch, zeros, and counts on both sides of 0.01 m
    dep1[70:90, 90:140] = 30000
    dep1[40:44, :] = 0
    dep1[44, 0:9] = [48, 49, 50, 51, 52, 49, 50, 51, 65535]
    pyr.set_target_depth(dep1, F5000)
    points = pyr.level(0).get_points3d()
    poses = _batch(synth, s, n, 7 + n)
    tot, cel = pyr.depth_check(poses)
    want_tot, want_cel = _host(capi, s, points, dep1, poses)
    for name in capi.DEPTH_CELL_DTYPE.names:
        assert np.array_equal(cel[name], want_cel[name]), f"{which}, n = {n}: cells' {name}"
    assert cel.tobytes() == want_cel.tobytes() and tot.tobytes() == want_tot.tobytes()
    for name in capi.DEPTH_CELL_DTYPE.names:  # a total is the exact sum of the pose's cells
        assert np.array_equal(tot[name].astype(np.uint64), cel[name].astype(np.uint64).sum(axis=1))
    assert tot["n_consistent"][0] > 0 and tot["n_occluded"][0] > 0 and tot["n_through"][0] > 0 and tot["n_both"][0] < tot["n_inframe"][0]
    if n >= 3:
        for k in (n // 2, n - 1):  # behind the camera, NaN: reference samples and nothing else
            assert tot["n_ref"][k] == tot["n_ref"][0] > 0 and tot["n_inframe"][k] == 0 and tot["sum_abs_um"][k] == 0
    # two runs give the same bytes; a pose gives the same records alone and at any position of a batch; totals alone
    again = pyr.depth_check(poses)
    assert again[0].tobytes() == tot.tobytes() and again[1].tobytes() == cel.tobytes()
    assert pyr.depth_check(poses, cells=False)[0].tobytes() == tot.tobytes()
    for k in sorted({0, n // 3, n - 1}):
        alone = pyr.depth_check(poses[k])
        assert alone[0].tobytes() == tot[k:k + 1].tobytes() and alone[1].tobytes() == cel[k:k + 1].tobytes(), f"pose {k} alone"
    if n > 1:
        back = pyr.depth_check(poses[::-1])
        assert back[0].tobytes() == tot[::-1].tobytes() and back[1].tobytes() == cel[::-1].tobytes()
    # other tolerances
    t2, c2 = pyr.depth_check(poses[:2], tol_abs=0.0, tol_rel=0.001)
    w2 = _host(capi, s, points, dep1, poses[:2], 0.0, 0.001)
    assert t2.tobytes() == w2[0].tobytes() and c2.tobytes() == w2[1].tobytes() and t2["n_consistent"][0] < tot["n_consistent"][0]


# ---- 2. evaluations are unaffected -------------------------------------------------------------------------------------------
def test_evaluations_are_unaffected(capi, synth, seqs, pyramids):
    s = seqs["S"]
    pyr = pyramids["S", "X"]
    pyr.set_pair_u16(s.dep[0], F5000, s.im[0], s.im[1], s.T0)
    pyr.set_target_depth(s.dep[1], F5000)
    ctx = pyr.level(0)
    p = s.pair.pose_init
    href = ctx.compute_href(p)
    before = ctx.evaluate(p, True)
    ne = ctx.normal_equations(p, DELTA)
    pyr.depth_check(_batch(synth, s, 17, 3))
    after = ctx.evaluate(p, True)  # (no reference stage in between: the level stayed evaluable)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    ne2 = ctx.normal_equations(p, DELTA)
    assert ne[0].tobytes() == ne2[0].tobytes() and ne[1].tobytes() == ne2[1].tobytes() and ne[2] == ne2[2] and ne[3] == ne2[3]
    href2 = ctx.compute_href(p)
    assert href[0].tobytes() == href2[0].tobytes() and href[1].tobytes() == href2[1].tobytes()
    for a, b in zip(before, ctx.evaluate(p, True)):
        assert a.tobytes() == b.tobytes()
    assert (href[0] >= 300).any() and np.isfinite(ne[2])


# ---- 3. a promotion from the resident depth equals one with the depth uploaded ---------------------------------------------------
@pytest.mark.parametrize("which", ["S", "W"])
def test_promote_target_equals_promote_target_u16(capi, synth, seqs, pyramids, which):
    s = seqs[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    T1 = capi.pose_to_Twc16(s.pose[1])
    dep = s.dep[1].copy()
    dep[5:9, 5:40] = 0
    dep[50, 60:68] = [49, 50, 51, 65535, 0, 1, 50, 49]
    for pyr in (X, Y):
        pyr.set_pair_u16(s.dep[0], F5000, s.im[0], s.im[2], s.T0)
        pyr.set_target(s.im[1])
    X.set_target_depth(dep, F5000)
    X.promote_resident_target(T1)
    Y.promote_target(dep, F5000, T1)
    assert _inputs(X) == _inputs(Y)
    assert X.get_level_inputs(0)[0].tobytes() == dep.tobytes()
    p = s.pose[2]
    for pyr in (X, Y):
        pyr.set_target(s.im[2])
    for l in range(LEVELS):
        a, b = X.level(l), Y.level(l)
        ha, hb = a.compute_href(p), b.compute_href(p)
        assert ha[0].tobytes() == hb[0].tobytes() and ha[1].tobytes() == hb[1].tobytes() and (l > 0 or (ha[0] >= 300).any())
        for x, y in zip(a.evaluate(p, True), b.evaluate(p, True)):
            assert x.tobytes() == y.tobytes(), f"{which}: level {l}"
    # the depth stayed with the target it came with ... until the target was replaced
    with pytest.raises(capi.NidError, match="call order"):
        X.depth_check(p)
    X.set_target_depth(s.dep[2], F5000)
    X.promote_resident_target(capi.pose_to_Twc16(p))  # twice in a row
    Y.promote_target(s.dep[2], F5000, capi.pose_to_Twc16(p))
    assert _inputs(X) == _inputs(Y)


# ---- 4. state and argument rules -------------------------------------------------------------------------------------------------
def test_state_rules(capi, synth, seqs, pyramids):
    s = seqs["S"]
    p = s.pose[1]
    lib = capi.load()
    fresh = capi.Pyramid.create(s.pair, NB, levels=LEVELS)
    try:
        with pytest.raises(capi.NidError, match="call order"):
            fresh.set_target_depth(s.dep[0], F5000)  # no target
        with pytest.raises(capi.NidError, match="call order"):
            fresh.depth_check(p)  # nothing at all
        fresh.set_target(s.im[0])
        fresh.set_target_depth(s.dep[0], F5000)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.depth_check(p)  # a target depth and no reference
        fresh.promote_resident_target(s.T0)
        tot, _ = fresh.depth_check(s.pose[0])  # the keyframe against its own depth
        assert tot["n_consistent"][0] == tot["n_ref"][0] > 0 and tot["sum_abs_um"][0] < 100 * tot["n_ref"][0]
        ctx = fresh.level(0)
        ctx.compute_href(p)
        want = ctx.normal_equations(p, DELTA)
        before = _inputs(fresh)
        fresh.set_target(s.im[1])  # drops the target depth
        with pytest.raises(capi.NidError, match="call order"):
            fresh.depth_check(p)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.promote_resident_target(s.T0)
        got = ctx.normal_equations(p, DELTA)  # the refused promotion left the reference, its reference stage included
        assert np.isfinite(got[2]) and [lv[:2] for lv in _inputs(fresh)] == [lv[:2] for lv in before]
        fresh.set_target(s.im[0])
        got = ctx.normal_equations(p, DELTA)
        assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2]
        fresh.set_pair_u16(s.dep[0], F5000, s.im[0], s.im[1], s.T0)  # a new pair has no target depth either
        with pytest.raises(capi.NidError, match="call order"):
            fresh.depth_check(p)
    finally:
        fresh.close()

    # an uncollected launch on a level: the three calls refuse and change nothing
    X = pyramids["S", "X"]
    X.set_pair_u16(s.dep[0], F5000, s.im[0], s.im[1], s.T0)
    X.set_target_depth(s.dep[1], F5000)
    good = X.depth_check(p)
    ctx = X.level(1)
    ctx.compute_href(p)
    want = ctx.normal_equations(p, DELTA)
    before = _inputs(X)
    ctx.launch(5, p, DELTA)
    with pytest.raises(capi.NidError, match="call order"):
        X.depth_check(p)
    with pytest.raises(capi.NidError, match="call order"):
        X.set_target_depth(s.dep[2], F5000)
    with pytest.raises(capi.NidError, match="call order"):
        X.promote_resident_target(s.T0)
    got = ctx.wait(5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert _inputs(X) == before
    again = X.depth_check(p)  # the refused calls cleared no flag and replaced no depth
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()

    # the argument rules behind a good handle
    dp, vp = (lambda a: a.ctypes.data_as(capi.c_dp)), (lambda a: a.ctypes.data_as(C.c_void_p))
    poses = np.tile(p, (capi.NID_MAX_BATCH + 1, 1))
    tot = np.zeros(capi.NID_MAX_BATCH + 1, dtype=capi.DEPTH_COUNTS_DTYPE)
    for n in (0, -1, capi.NID_MAX_BATCH + 1):
        assert lib.nid_pyr_depth_check(X.h, dp(poses), n, 0.01, 0.02, vp(tot), None) == -1
    assert lib.nid_pyr_depth_check(X.h, None, 1, 0.01, 0.02, vp(tot), None) == -1
    assert lib.nid_pyr_depth_check(X.h, dp(poses), 1, 0.01, 0.02, None, None) == -1
    for bad in (-1e-9, np.nan, np.inf):
        assert lib.nid_pyr_depth_check(X.h, dp(poses), 1, bad, 0.02, vp(tot), None) == -1
        assert lib.nid_pyr_depth_check(X.h, dp(poses), 1, 0.01, bad, vp(tot), None) == -1
    assert lib.nid_pyr_set_target_depth_u16(X.h, None, F5000) == -1 and lib.nid_pyr_promote_target(X.h, None) == -1
    assert lib.nid_pyr_depth_check(X.h, dp(poses), capi.NID_MAX_BATCH, 0.01, 0.02, vp(tot), None) == 0
    trk = capi.Tracker.create(s.pair, NB, levels=LEVELS)
    try:
        assert lib.nid_track_set_policy(trk.h, None) == -1
        for name, bad in (("keyframe_mode", 2), ("keyframe_mode", -1), ("max_age", -1), ("min_samples", -1), ("reserved", 1), ("min_overlap", 1.5),
                          ("min_overlap", float("nan")), ("min_consistent", -0.1), ("min_consistent", float("inf")), ("tol_abs", -1.0),
                          ("tol_rel", float("nan"))):
            pol = capi.track_policy_default()
            setattr(pol, name, bad)
            assert lib.nid_track_set_policy(trk.h, C.byref(pol)) == -1, name
        chosen, n_checked, age = trk.last_check()
        assert (n_checked, age) == (0, 0) and not any(chosen.tolist())
    finally:
        trk.close()


# ---- 5. the tracker under a policy is its composition ------------------------------------------------------------------------------
class Restated:
    """nid_track_push_u16's schedule under a policy (nid_keyframe.h), from the Pyramid's public calls and the pose helpers"""

    def __init__(self, capi, pyr, policy, twists=TWISTS, keep=KEEP):
        self.capi, self.pyr, self.pol, self.twists, self.keep = capi, pyr, policy, twists, keep
        self.cur, self.prev, self.have_ref, self.frame, self.age = None, None, False, 0, 0
        self.check = (np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0, 0)

    def set_pose(self, pose7):
        self.cur, self.prev = np.array(pose7, dtype=np.float64), None

    def push(self, im, dep, T_first=None):
        capi, pyr, pol = self.capi, self.pyr, self.pol
        out = dict(chi2=0.0, n_active=0, best_origin=-1, promoted=0, frame=self.frame, rounds=np.zeros(LEVELS, dtype=np.int32))
        chosen, n_checked = np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0
        pyr.set_target(im)
        if not self.have_ref:
            T = np.eye(4).reshape(16) if T_first is None else T_first
            pyr.promote_target(dep, F5000, T)
            self.cur, self.prev, self.have_ref = capi.pose_from_Twc16(T), None, True
            out.update(status=capi.TRACK_FIRST, promoted=1)
        else:
            with_policy = dep is not None and (pol.keyframe_mode != 0 or pol.min_consistent > 0)
            if with_policy:
                pyr.set_target_depth(dep, F5000)
            cur = self.cur
            pred = cur if self.prev is None else capi.pose_compose(capi.pose_compose(cur, capi.pose_inverse(self.prev)), cur)
            starts = np.stack([pred, cur] + [capi.pose_perturb(pred, tw) for tw in self.twists])
            res, origin, rounds, best, best_pose = pyr.multistart_lm(starts, TRACK_ITER, DELTA, keep=self.keep)
            out.update(rounds=rounds, best_origin=best)
            res0, org0 = res[LEVELS - 1], origin[LEVELS - 1]
            if best >= 0 and with_policy:
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
                    out.update(status=capi.TRACK_OK, best_origin=int(org0[k]), chi2=float(res0["chi2"][k]), n_active=int(res0["n_active"][k]),
                               promoted=int(promote))
                    self.prev, self.cur = cur, pose
            elif best >= 0:
                k = int(np.flatnonzero(org0 == best)[0])
                out.update(status=capi.TRACK_OK, chi2=float(res0["chi2"][k]), n_active=int(res0["n_active"][k]))
                self.prev, self.cur = cur, best_pose.copy()
                if dep is not None:
                    pyr.promote_target(dep, F5000, capi.pose_to_Twc16(self.cur))
                    out.update(promoted=1)
            else:
                out.update(status=capi.TRACK_LOST)
                self.prev = None
        if out["promoted"]:
            self.age = 0
        elif out["status"] == capi.TRACK_OK:
            self.age += 1
        self.check = (chosen, n_checked, self.age)
        out["pose7"] = self.cur.copy()
        self.frame += 1
        return out


def _assert_same_result(got, want, what):
    assert got["pose7"].tobytes() == want["pose7"].tobytes(), f"{what}: pose7\n{got['pose7']}\n{want['pose7']}"
    assert np.float64(got["chi2"]).tobytes() == np.float64(want["chi2"]).tobytes(), f"{what}: chi2 {got['chi2']!r} / {want['chi2']!r}"
    for name in ("n_active", "best_origin", "status", "promoted", "frame"):
        assert got[name] == want[name], f"{what}: {name} {got[name]} / {want[name]}"
    assert got["rounds"].tobytes() == want["rounds"].tobytes(), f"{what}: rounds {got['rounds']} / {want['rounds']}"


def _assert_same_check(trk, ref, what):
    got, want = trk.last_check(), ref.check
    assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], f"{what}: last check {got} / {want}"


def _policy(capi, **members):
    pol = capi.track_policy_default()
    for k, v in members.items():
        setattr(pol, k, v)
    return pol


def _tracker(capi, s, pol=None):
    trk = capi.Tracker.create(s.pair, NB, levels=LEVELS)
    trk.set_lm(TRACK_ITER, DELTA, KEEP)
    trk.set_twists(TWISTS)
    if pol is not None:
        trk.set_policy(pol)
    return trk


def _near_start(synth, pose):
    """a start a frame's motion away from `pose`, for a frame the tracker could not reach from the last one"""
    return synth.perturb_pose7(pose, [1e-3, -1e-3, 5e-4], [4e-3, -3e-3, 2e-3])


# frames of a run: (index into the sequence's images, index of the depth map or None, jump to the frame's neighbourhood first)
RUN = ((0, 0, False), (1, 1, False), (2, 2, False), (3, None, False), (4, 4, True), (3, 3, True), (2, 2, False))


@pytest.mark.parametrize("which,policy", [("S", "on_demand"), ("S", "max_age"), ("S", "verified"), ("W", "verified")])
def test_tracker_is_its_composition(capi, synth, seqs, pyramids, which, policy):
    """Seven pushes -- the first frame, two near views, one without depth, the far view, and back --, every result, last
    check and level input equal to the restatement's, whatever the status."""
    s = seqs[which]
    pol = {"on_demand": _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP),
           "max_age": _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP, max_age=2),
           "verified": _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP, min_consistent=MIN_CONSISTENT, min_samples=1000)}[policy]
    trk = _tracker(capi, s, pol)
    try:
        ref = Restated(capi, pyramids[which, "Y"], pol)
        ref.have_ref = False
        statuses, promoted = [], []
        for k, (i, d, jump) in enumerate(RUN):
            dep = s.dep[d] if d is not None else None
            if jump:
                start = _near_start(synth, s.pose[i])
                trk.set_pose(start)
                ref.set_pose(start)
            got = trk.push(s.im[i], dep, F5000, T_wc_first=s.T0)
            want = ref.push(s.im[i], dep, T_first=s.T0)
            chosen, n_checked, age = trk.last_check()
            print(f"{which} {policy}, push {k} (view {i}): status {got['status']}, best_origin {got['best_origin']}, promoted {got['promoted']}, "
                  f"checked {n_checked}, age {age}, in frame {chosen['n_inframe']} / {chosen['n_ref']}, consistent {chosen['n_consistent']} / "
                  f"{chosen['n_both']}, |pose7 - true| {np.abs(got['pose7'] - s.pose[i]).max():.3e}")
            _assert_same_result(got, want, f"{which} {policy}, push {k}")
            _assert_same_check(trk, ref, f"{which} {policy}, push {k}")
            assert _inputs(trk.pyramid) == _inputs(ref.pyr), f"{which} {policy}, push {k}: level inputs"
            assert got["status"] != capi.TRACK_OK or dep is None or n_checked >= 1 or k == 0
            statuses.append(got["status"])
            promoted.append(got["promoted"])
        assert statuses[0] == capi.TRACK_FIRST and capi.TRACK_LOST not in statuses[1:3], statuses
        if policy == "verified":
            assert capi.TRACK_REJECTED in statuses or capi.TRACK_OK in statuses
        if policy == "max_age" and statuses[1:3] == [capi.TRACK_OK] * 2:
            assert promoted[1:3] == [0, 1], "the second frame tracked on a keyframe promotes it at max_age = 2"
    finally:
        trk.close()


def test_default_policy_set_back_is_no_policy(capi, synth, seqs):
    """a tracker whose policy was set and then set back to nid_track_policy_default gives the bytes of one that never had
    one -- the schedule of nid_pyr_stream.h: a promotion with every frame that has depth, nothing checked"""
    s = seqs["S"]
    a, b = _tracker(capi, s), _tracker(capi, s, _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP, min_consistent=MIN_CONSISTENT))
    try:
        b.set_policy(capi.track_policy_default())
        for k, (i, d, jump) in enumerate(RUN[:5]):
            dep = s.dep[d] if d is not None else None
            if jump:
                for t in (a, b):
                    t.set_pose(_near_start(synth, s.pose[i]))
            ra, rb = a.push(s.im[i], dep, F5000, T_wc_first=s.T0), b.push(s.im[i], dep, F5000, T_wc_first=s.T0)
            _assert_same_result(ra, rb, f"push {k}")
            assert _inputs(a.pyramid) == _inputs(b.pyramid)
            for t in (a, b):
                chosen, n_checked, age = t.last_check()
                assert n_checked == 0 and not any(chosen.tolist())
                assert not ra["promoted"] or age == 0
            if ra["status"] == capi.TRACK_OK:
                assert ra["promoted"] == int(dep is not None)
    finally:
        a.close()
        b.close()


# ---- 6. behaviour ------------------------------------------------------------------------------------------------------------------
def test_on_demand_keeps_the_keyframe_until_the_overlap_falls(capi, synth, seqs):
    s = seqs["S"]
    trk = _tracker(capi, s, _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP))
    try:
        first = trk.push(s.im[0], s.dep[0], F5000, T_wc_first=s.T0)
        assert (first["status"], first["promoted"]) == (capi.TRACK_FIRST, 1)
        points = trk.pyramid.level(0).get_points3d()
        cfg = s.cfg(capi)
        overlap = []
        for i in range(1, 5):  # the condition this test stands on, from the host function at the ground-truth poses
            t, _ = capi.depth_check_host(cfg, points, s.dep[i], F5000, s.pose[i], TOL_ABS, TOL_REL)
            overlap.append(int(t["n_inframe"]) / int(t["n_ref"]))
        print("overlap with frame 0 at the true poses:", [f"{o:.4f}" for o in overlap])
        assert min(overlap[:3]) >= MIN_OVERLAP + 0.05 and overlap[3] <= MIN_OVERLAP - 0.05
        keyframe = [lv[:2] for lv in _inputs(trk.pyramid)]
        tracked = 0
        for i in (1, 2, 3):
            got = trk.push(s.im[i], s.dep[i], F5000)
            chosen, n_checked, age = trk.last_check()
            print(f"near view {i}: status {got['status']}, promoted {got['promoted']}, in frame {chosen['n_inframe']} / {chosen['n_ref']}, age {age}")
            if got["status"] == capi.TRACK_OK:
                tracked += 1
                assert got["promoted"] == 0 and n_checked == 1 and age == tracked
                assert int(chosen["n_inframe"]) >= MIN_OVERLAP * int(chosen["n_ref"])
            assert [lv[:2] for lv in _inputs(trk.pyramid)] == keyframe, "a near view replaced the keyframe"
        assert tracked >= 2, "the near views did not track: nothing was shown"
        trk.set_pose(_near_start(synth, s.pose[4]))
        got = trk.push(s.im[4], s.dep[4], F5000)
        chosen, n_checked, age = trk.last_check()
        print(f"far view: status {got['status']}, promoted {got['promoted']}, in frame {chosen['n_inframe']} / {chosen['n_ref']}, age {age}")
        if got["status"] == capi.TRACK_OK:
            assert got["promoted"] == 1 and age == 0 and int(chosen["n_inframe"]) < MIN_OVERLAP * int(chosen["n_ref"])
            now = _inputs(trk.pyramid)
            assert now[0][0] == s.dep[4].tobytes() and now[0][1] == s.im[4].tobytes(), "the far view is the keyframe now"
    finally:
        trk.close()


def test_verification_rejects_a_depth_map_of_another_view(capi, synth, seqs):
    s = seqs["S"]
    pol = _policy(capi, keyframe_mode=1, min_overlap=MIN_OVERLAP, min_consistent=MIN_CONSISTENT, min_samples=1000)
    trk = _tracker(capi, s, pol)
    try:
        trk.push(s.im[0], s.dep[0], F5000, T_wc_first=s.T0)
        points = trk.pyramid.level(0).get_points3d()
        cfg = s.cfg(capi)
        frac = {}
        for name, d in (("right", s.dep[2]), ("wrong", s.dep[4])):  # view 2's image with its own depth / with the far view's
            t, _ = capi.depth_check_host(cfg, points, d, F5000, s.pose[2], TOL_ABS, TOL_REL)
            assert int(t["n_both"]) >= pol.min_samples
            frac[name] = int(t["n_consistent"]) / int(t["n_both"])
        print("consistent fraction at the true pose:", frac)
        assert frac["right"] >= MIN_CONSISTENT + 0.2 and frac["wrong"] <= MIN_CONSISTENT - 0.2
        one = trk.push(s.im[1], s.dep[1], F5000)
        assert one["status"] == capi.TRACK_OK and one["promoted"] == 0
        keyframe = _inputs(trk.pyramid)
        bad = trk.push(s.im[2], s.dep[4], F5000)
        chosen, n_checked, age = trk.last_check()
        print(f"wrong depth: status {bad['status']}, checked {n_checked}, consistent {chosen['n_consistent']} / {chosen['n_both']}")
        assert bad["status"] == capi.TRACK_REJECTED and bad["promoted"] == 0 and bad["best_origin"] >= 0 and n_checked >= 1
        assert bad["chi2"] == 0 and bad["n_active"] == 0 and bad["frame"] == 2 and age == 1
        assert bad["pose7"].tobytes() == one["pose7"].tobytes(), "a rejected frame moved the pose"
        assert float(chosen["n_consistent"]) < MIN_CONSISTENT * float(chosen["n_both"])
        assert [lv[:2] for lv in _inputs(trk.pyramid)] == [lv[:2] for lv in keyframe], "a rejected frame touched the keyframe"
        good = trk.push(s.im[2], s.dep[2], F5000)
        chosen, n_checked, age = trk.last_check()
        print(f"right depth: status {good['status']}, checked {n_checked}, consistent {chosen['n_consistent']} / {chosen['n_both']}")
        assert good["status"] == capi.TRACK_OK and good["frame"] == 3 and age == 2
        assert float(chosen["n_consistent"]) >= MIN_CONSISTENT * float(chosen["n_both"]) and int(chosen["n_both"]) >= pol.min_samples
    finally:
        trk.close()
