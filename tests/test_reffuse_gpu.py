"""include/nid/nid_reffuse.h on the device: the planes and the counts of nid_pyr_fuse_reference_depth equal nid_reffuse_host's
and a numpy restatement's; a refined pyramid is the pyramid of the pair with the refined samples written in, bit for bit; a
fusion is reversible and composes with the fill of nid_reffill.h and the mask of nid_refmask.h; the state rules; the tracker
with fusing is the composition its header states.  The geometries, the scene, the six-frame sequence and the helpers are
tests/test_reffill_gpu.py's: 120 x 168 with three levels and 122 x 174 with two -- 20 160 and 21 228 pixels, neither a
multiple of k_reffuse_apply's 1024-pixel span, both multiples of a lane's four pixels: the lane that makes a plane's last
one to three pixels one by one is run by test_plane_sizes_around_a_lane."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ur = _load("reffuse_restate")
fg = _load("test_reffill_gpu")  # (its helpers and its sequence; its tests are not collected from here)
fr, rr = ur.fr, ur.rr

DELTA, NB, F5000 = fg.DELTA, fg.NB, fg.F5000
GA, GR = ur.GATE_ABS, ur.GATE_REL
TOL_ABS, TOL_REL = fg.TOL_ABS, fg.TOL_REL
GEOMETRY = fg.GEOMETRY
_inputs, _fresh, _evaluations, _starts, _caller = fg._inputs, fg._fresh, fg._evaluations, fg._starts, fg._caller


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


# ---- 1. the fusion equals the host twin and the restatement -----------------------------------------------------------------
# (pose, gate_abs, gate_rel_1024, max_obs) or "fill": each on the planes the one before left
CALLS = (("pose", GA, GR, 1), ("pose", GA, GR, 1), ("pose_out", 0, 0, 2), "fill", ("pose", 10, 0, 2), ("pose", GA, GR, 2), ("pose_out", GA, GR, 255),
         ("pose", 0, 0, 255), ("pose_out", 10, 0, 255), ("pose", 10, 0, 255), ("pose_out", 10, 0, 1))


@pytest.mark.parametrize("which", ["W", "O"])
def test_fusion_equals_the_host(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    pyr = pyramids[which, "X"]
    _fresh(pyr, s)
    assert not pyr.get_reference_fused().any() and not pyr.get_reference_fusion_obs().any()
    pyr.set_reference_mask(_caller(s))
    pyr.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 1, 0)
    mask = pyr.get_reference_mask()
    assert (mask & 1).any() and (mask & 2).any() and (mask & 8).any()
    S = np.zeros((s.rows, s.cols), dtype=np.uint32)
    K = np.zeros((s.rows, s.cols), dtype=np.uint8)
    fused = np.zeros((s.rows, s.cols), dtype=np.uint16)
    fill = np.zeros((s.rows, s.cols), dtype=np.uint16)
    worst = np.inf
    seen = dict(n_fused=0, n_gated=0, n_saturated=0, n_changed=0)
    for k, call in enumerate(CALLS):
        if call == "fill":  # in between: on the BASE plane, and the fusion's planes stay
            cnt = pyr.fill_reference_depth(s.pose_out, 1, GA, GR, 0)
            fill, host_cnt = capi.reffill_host(cfg, ur.base(fused, s.dep0), F5000, s.T0, s.dep1, F5000, s.pose_out, 1, GA, GR)
            assert np.array_equal(pyr.get_reference_fill(), fill) and cnt.tobytes() == host_cnt.tobytes() and fill.any()
            assert np.array_equal(pyr.get_reference_fused(), fused) and np.array_equal(pyr.get_reference_fusion_obs(), K)
        else:
            name, ga, gr, mo = call
            what = f"{which}, call {k}: {name}, gate {ga} / {gr}, max_obs {mo}"
            cnt = pyr.fuse_reference_depth(getattr(s, name), ga, gr, mo)
            args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, getattr(s, name), ga, gr, mo, S, K)
            S, K, fused, host_cnt = capi.reffuse_host(*args)
            wS, wK, wF, want_cnt, margin = ur.restate(*args)
            worst = min(worst, margin)
            print(f"{what}: {ur.counts_dict(cnt)}, smallest margin {margin:.3e}")
            assert np.array_equal(S, wS) and np.array_equal(K, wK) and np.array_equal(fused, wF) and ur.counts_dict(host_cnt) == want_cnt, \
                f"{what}: the host twin and the restatement"
            got = pyr.get_reference_fused()
            assert np.array_equal(got, fused), f"{what}: {int((got != fused).sum())} entries of the FUSED plane differ from the host's"
            assert np.array_equal(pyr.get_reference_fusion_obs(), K), f"{what}: the OBS plane"
            assert cnt.tobytes() == host_cnt.tobytes(), f"{what}: counts {cnt} / {host_cnt}"
            seen = {n: max(seen[n], want_cnt[n]) for n in seen}
        assert np.array_equal(pyr.get_reference_mask(), mask), f"call {k}: the mask plane moved"
        assert np.array_equal(pyr.get_reference_fill(), fill), f"call {k}: the fill plane moved"
        # the effective reference: level 0's depth is mask ? 0 : (fill ? fill : (fused ? fused : uploaded))
        assert np.array_equal(pyr.get_level_inputs(0)[0], np.where(mask != 0, 0, ur.completed(fill, fused, s.dep0)).astype(np.uint16)), f"call {k}"
    assert worst > 1e-9, "a decision of the scene hangs on a last bit"
    assert all(v > 0 for v in seen.values()), f"a branch of the rule was never reached: {seen}"
    assert seen["n_fused"] > 10000 and seen["n_gated"] > 10000 and seen["n_saturated"] > 5000 and seen["n_changed"] > 10000, seen
    assert ((mask != 0) & (fused != 0)).any() and int(K.max()) > 2


def test_plane_sizes_around_a_lane(capi, synth):
    """k_reffuse_apply's last lane: planes of 4 n + 3, 4 n + 2 and 4 n + 1 pixels (a lane makes four) and one of exactly five
    workgroups' spans -- each against the host twin, twice on the same state."""
    for rows, cols, rest in ((65, 75, 3), (65, 78, 2), (65, 77, 1), (64, 80, 0)):
        assert (rows * cols) % 4 == rest and (rest or (rows * cols) % 1024 == 0)
        s = rr.Scene(synth, rows, cols, 4)
        cfg = s.cfg(capi, NB)
        pyr = capi.Pyramid.create(s.pair, NB, levels=1)
        try:
            _fresh(pyr, s)
            S = K = None
            for ga, mo in ((GA, 255), (5, 2)):
                cnt = pyr.fuse_reference_depth(s.pose, ga, GR, mo)
                S, K, fused, host_cnt = capi.reffuse_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, s.pose, ga, GR, mo, S, K)
                assert np.array_equal(pyr.get_reference_fused(), fused) and np.array_equal(pyr.get_reference_fusion_obs(), K), (rows, cols)
                assert cnt.tobytes() == host_cnt.tobytes() and int(cnt["n_fused"]) + int(cnt["n_saturated"]) > 0, (rows, cols, cnt)
                assert np.array_equal(pyr.get_level_inputs(0)[0], ur.base(fused, s.dep0)), (rows, cols)
        finally:
            pyr.close()


# ---- 2. a refined pyramid is the pyramid of the refined depth ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_refined_pyramid_equals_the_refined_depth(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    poses = (s.pose, synth.perturb_pose7(s.pose0, [0, 0, 0], [-0.45, 0.3, 0]))
    X.fuse_reference_depth(s.pose_out, GA, GR, 255)
    X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    cnt = X.fuse_reference_depth(s.pose, GA, GR, 255)
    fused, fill = X.get_reference_fused(), X.get_reference_fill()
    assert int(cnt["n_fused"]) > 10000 and int((fused != 0).sum()) > 10000 and int((fill != 0).sum()) > 1000
    comp = ur.completed(fill, fused, s.dep0)
    assert int((comp != s.dep0).sum()) > 10000
    _fresh(Y, s, comp)
    assert _inputs(X) == _inputs(Y)
    for k, pose in enumerate(poses):
        ex, ey = _evaluations(X, pose), _evaluations(Y, pose)
        for l in range(X.levels):
            for name, a, b in zip(("N_c", "Href", "Hc", "Hj", "err", "J"), ex[l], ey[l]):
                assert a == b, f"{which}, pose {k}, level {l}: {name}"
    starts = _starts(synth, s.pose)
    rx, ry = X.multistart_lm(starts, 5, DELTA), Y.multistart_lm(starts, 5, DELTA)
    assert rx[0].tobytes() == ry[0].tobytes() and rx[1].tobytes() == ry[1].tobytes() and rx[2].tobytes() == ry[2].tobytes()
    assert rx[3] == ry[3] and rx[4].tobytes() == ry[4].tobytes() and np.isfinite(rx[0]["chi2"]).any()


# ---- 3. reversible; composes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_fusion_is_reversible_and_composes(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    _fresh(Y, s)  # never fused
    never = _inputs(Y)
    ev_never = _evaluations(Y, s.pose)
    Y.clear_reference_fusion()  # nothing fused: a no-op, the reference stage stays
    for l in range(Y.levels):
        assert tuple(a.tobytes() for a in Y.level(l).evaluate(s.pose, True)) == ev_never[l][2:]
    first = X.fuse_reference_depth(s.pose, GA, GR, 255)
    fused = X.get_reference_fused()
    assert int(first["n_changed"]) > 10000 and _inputs(X) != never
    X.clear_reference_fusion()
    assert not X.get_reference_fused().any() and not X.get_reference_fusion_obs().any() and _inputs(X) == never
    assert _evaluations(X, s.pose) == ev_never
    X.clear_reference_fusion()  # twice
    assert _inputs(X) == never
    again = X.fuse_reference_depth(s.pose, GA, GR, 255)
    assert np.array_equal(X.get_reference_fused(), fused) and again.tobytes() == first.tobytes()
    # with a fill and a mask: the clear keeps both and gives the never-fused pyramid's bits
    caller = _caller(s)
    for pyr in (X, Y):
        pyr.set_reference_mask(caller)
    Y.fill_reference_depth(s.pose_out, 0, GA, GR, 0)  # (guard 0: the fill reads no neighbour's BASE)
    X.fill_reference_depth(s.pose_out, 0, GA, GR, 0)
    assert _inputs(X) != _inputs(Y)
    X.clear_reference_fusion()
    assert np.array_equal(X.get_reference_fill(), Y.get_reference_fill()) and X.get_reference_fill().any()
    assert np.array_equal(X.get_reference_mask(), Y.get_reference_mask()) and X.get_reference_mask().any()
    assert _inputs(X) == _inputs(Y)

    # fill then fuse == fuse then fill on the device; a fill on a fused pyramid is nid_reffill_host on the BASE plane
    for guard in (1, 2):
        _fresh(X, s)
        _fresh(Y, s)
        fx = X.fill_reference_depth(s.pose_out, guard, GA, GR, 0)
        ux = X.fuse_reference_depth(s.pose_out, GA, GR, 255)
        uy = Y.fuse_reference_depth(s.pose_out, GA, GR, 255)
        fy = Y.fill_reference_depth(s.pose_out, guard, GA, GR, 0)
        assert fx.tobytes() == fy.tobytes() and ux.tobytes() == uy.tobytes() and int(fx["n_refused"]) > 0 and int(ux["n_changed"]) > 500
        assert np.array_equal(X.get_reference_fill(), Y.get_reference_fill()) and np.array_equal(X.get_reference_fused(), Y.get_reference_fused())
        assert np.array_equal(X.get_reference_fusion_obs(), Y.get_reference_fusion_obs()) and _inputs(X) == _inputs(Y)
        base = ur.base(Y.get_reference_fused(), s.dep0)
        host, host_cnt = capi.reffill_host(cfg, base, F5000, s.T0, s.dep1, F5000, s.pose_out, guard, GA, GR)
        assert np.array_equal(Y.get_reference_fill(), host) and fy.tobytes() == host_cnt.tobytes()
        # ... and at another pose than the fusion's, where BASE differs from the uploaded depth under the guard's window
        Y.fuse_reference_depth(s.pose, GA, GR, 255)
        fy = Y.fill_reference_depth(s.pose, guard, GA, GR, 1)
        base = ur.base(Y.get_reference_fused(), s.dep0)
        host2, host_cnt = capi.reffill_host(cfg, base, F5000, s.T0, s.dep1, F5000, s.pose, guard, GA, GR, True, host)
        assert np.array_equal(Y.get_reference_fill(), host2) and fy.tobytes() == host_cnt.tobytes()
    # clearing the fill on a fused pyramid leaves the fused samples in the effective depth
    fused = Y.get_reference_fused()
    Y.clear_reference_fill()
    assert not Y.get_reference_fill().any() and np.array_equal(Y.get_reference_fused(), fused) and fused.any()
    assert np.array_equal(Y.get_level_inputs(0)[0], ur.base(fused, s.dep0))
    # a mask behind a fusion classifies the refined samples: the host's mask over the completed depth
    cnt = Y.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 2, 0)
    want, want_cnt = capi.refmask_host(cfg, ur.base(fused, s.dep0), F5000, s.T0, s.dep1, F5000, s.pose, TOL_ABS, TOL_REL, 6, 2)
    assert np.array_equal(Y.get_reference_mask(), want) and cnt.tobytes() == want_cnt.tobytes()
    assert np.array_equal(Y.get_reference_fused(), fused), "a masking call moved the fusion"

    # a new reference starts unfused: the pair call and both promotions
    T1 = capi.pose_to_Twc16(s.pose)
    for renew in (lambda: _fresh(X, s), lambda: X.promote_resident_target(T1), lambda: X.promote_target(s.dep1, F5000, T1)):
        _fresh(X, s)
        assert int(X.fuse_reference_depth(s.pose, GA, GR, 255)["n_fused"]) > 10000 and X.get_reference_fused().any()
        renew()
        assert not X.get_reference_fused().any() and not X.get_reference_fusion_obs().any()
        X.clear_reference_fusion()  # nothing to clear behind a new reference
        assert not X.get_reference_fused().any()
    assert np.array_equal(X.get_level_inputs(0)[0], s.dep1)
    # ... and the first fusion behind a promotion starts from ITS depth and matrix: the old keyframe's depth on the target
    X.set_target(s.pair.im0)
    X.set_target_depth(s.dep0, F5000)
    cnt = X.fuse_reference_depth(s.pose0, GA, GR, 255)
    _, K, host, host_cnt = capi.reffuse_host(cfg, s.dep1, F5000, T1, s.dep0, F5000, s.pose0, GA, GR, 255)
    assert np.array_equal(X.get_reference_fused(), host) and np.array_equal(X.get_reference_fusion_obs(), K) and cnt.tobytes() == host_cnt.tobytes()
    assert int(cnt["n_fused"]) > 1000


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------
def test_state_rules(capi, synth, scenes, pyramids):
    s = scenes["W"]
    levels = GEOMETRY["W"][3]
    fresh = capi.Pyramid.create(s.pair, NB, levels=levels)
    try:
        for call in (lambda: fresh.fuse_reference_depth(s.pose), fresh.clear_reference_fusion, fresh.get_reference_fused, fresh.get_reference_fusion_obs):
            with pytest.raises(capi.NidError, match="call order"):
                call()  # no reference
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        ctx = fresh.level(0)
        ctx.compute_href(s.pose)
        want = ctx.evaluate(s.pose, True)
        before = _inputs(fresh)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.fuse_reference_depth(s.pose)  # no target depth
        assert _inputs(fresh) == before and not fresh.get_reference_fused().any() and not fresh.get_reference_fusion_obs().any()
        for a, b in zip(want, ctx.evaluate(s.pose, True)):  # the refused call left the reference, its reference stage included
            assert a.tobytes() == b.tobytes()
    finally:
        fresh.close()

    # an uncollected launch on a level: the four calls refuse and change nothing; the public slots are untouched by a fusion
    X = pyramids["W", "X"]
    _fresh(X, s)
    X.fuse_reference_depth(s.pose, GA, GR, 255)
    fused, obs = X.get_reference_fused(), X.get_reference_fusion_obs()
    ctx = X.level(1)
    ctx.compute_href(s.pose)
    want = ctx.normal_equations(s.pose, DELTA)
    before = _inputs(X)
    ctx.launch(5, s.pose, DELTA)
    for call in (lambda: X.fuse_reference_depth(s.pose), X.clear_reference_fusion, X.get_reference_fused, X.get_reference_fusion_obs):
        with pytest.raises(capi.NidError, match="call order"):
            call()
    got = ctx.wait(5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert _inputs(X) == before and np.array_equal(X.get_reference_fused(), fused) and np.array_equal(X.get_reference_fusion_obs(), obs)
    reduced_dev, cellout_dev = ctx.slot_buffers(5)
    slot = (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    X.fuse_reference_depth(s.pose_out, GA, GR, 255)
    X.clear_reference_fusion()
    assert slot == (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    with pytest.raises(capi.NidError, match="call order"):
        ctx.evaluate(s.pose, True)  # as behind a promotion: a reference, no reference stage
    ctx.compute_href(s.pose)
    assert np.isfinite(ctx.normal_equations(s.pose, DELTA)[2])

    # the argument rules behind a good handle
    lib = capi.load()
    q = np.ascontiguousarray(s.pose)
    dp = lambda a: a.ctypes.data_as(capi.c_dp)
    before = _inputs(X)  # (cleared above: the never-fused pyramid's)
    bad = ((-1, 20, 255), (65536, 20, 255), (50, -1, 255), (50, 1025, 255), (50, 20, 0), (50, 20, 256), (50, 20, -1))
    for ga, gr, mo in bad:
        assert lib.nid_pyr_fuse_reference_depth(X.h, dp(q), ga, gr, mo, None) == -1
    assert lib.nid_pyr_fuse_reference_depth(X.h, None, 50, 20, 255, None) == -1
    assert lib.nid_pyr_get_reference_fused_u16(X.h, None) == -1 and lib.nid_pyr_get_reference_fusion_obs_u8(X.h, None) == -1
    assert _inputs(X) == before and not X.get_reference_fused().any(), "a refused argument touched the pyramid"
    assert lib.nid_pyr_fuse_reference_depth(X.h, dp(q), 65535, 1024, 255, None) == 0  # counts are optional
    trk = capi.Tracker.create(s.pair, NB, levels=levels)
    try:
        for ga, gr, mo in bad:
            assert lib.nid_track_set_fusing(trk.h, 1, ga, gr, mo) == -1
        assert lib.nid_track_set_fusing(trk.h, 1, 65535, 1024, 255) == 0 and lib.nid_track_set_fusing(trk.h, 0, 0, 0, 1) == 0
        assert lib.nid_track_last_fusion(trk.h, None) == -1
        assert not any(ur.counts_dict(trk.last_fusion()).values())
    finally:
        trk.close()


# ---- 5. the tracker is its composition ------------------------------------------------------------------------------------------
TRACK_ITER, TWISTS, MASK_CLASSES, MASK_DILATE, FILL_GUARD = fg.TRACK_ITER, fg.TWISTS, fg.MASK_CLASSES, fg.MASK_DILATE, fg.FILL_GUARD
FUSE_MAX_OBS = 1  # on the two-level sequence the keyframe's second frame meets the cap


class Restated:
    """nid_track_push_u16's schedule under an active policy with filling, fusing and masking (nid_keyframe.h's steps,
    nid_reffill.h's fill behind the choice, nid_reffuse.h's fusion behind the fill, nid_refmask.h's step 5e), from the
    Pyramid's public calls and the pose helpers"""

    def __init__(self, capi, pyr, policy, filling, fusing, classes, dilate, keep):
        self.capi, self.pyr, self.pol, self.filling, self.fusing = capi, pyr, policy, filling, fusing
        self.classes, self.dilate, self.keep = classes, dilate, keep
        self.cur, self.prev, self.have_ref, self.frame, self.age = None, None, False, 0, 0
        self.check = (np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0, 0)
        self.mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]
        self.fill = np.zeros(1, dtype=capi.REFFILL_COUNTS_DTYPE)[0]
        self.fusion = np.zeros(1, dtype=capi.REFFUSE_COUNTS_DTYPE)[0]

    def push(self, im, dep, T_first):
        capi, pyr, pol, L = self.capi, self.pyr, self.pol, self.pyr.levels
        out = dict(chi2=0.0, n_active=0, best_origin=-1, promoted=0, frame=self.frame, rounds=np.zeros(L, dtype=np.int32))
        chosen, n_checked = np.zeros(1, dtype=capi.DEPTH_COUNTS_DTYPE)[0], 0
        mask = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)[0]
        fill = np.zeros(1, dtype=capi.REFFILL_COUNTS_DTYPE)[0]
        fusion = np.zeros(1, dtype=capi.REFFUSE_COUNTS_DTYPE)[0]
        pyr.set_target(im)
        if not self.have_ref:
            pyr.promote_target(dep, F5000, T_first)
            self.cur, self.prev, self.have_ref = capi.pose_from_Twc16(T_first), None, True
            out.update(status=capi.TRACK_FIRST, promoted=1)
        else:
            assert dep is not None and (pol.keyframe_mode != 0 or pol.min_consistent > 0)
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
                        if self.filling:  # 5d'.
                            fill = pyr.fill_reference_depth(pose, FILL_GUARD, GA, GR, 1)
                        if self.fusing:  # 5d''.
                            fusion = pyr.fuse_reference_depth(pose, GA, GR, FUSE_MAX_OBS)
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
        self.mask, self.fill, self.fusion = mask, fill, fusion
        out["pose7"] = self.cur.copy()
        self.frame += 1
        return out


@pytest.mark.parametrize("levels,filling,masking", [(3, False, False), (3, True, True), (2, False, True), (2, True, False), (2, True, True)])
def test_tracker_is_its_composition(capi, synth, levels, filling, masking):
    """Six pushes under on-demand keyframes with a maximal age, verification on, an occluder from frame 3 on: every result,
    last check, last mask, last fill, last fusion, every plane and level input equal to the restatement's, whatever the status."""
    s = fg.Seq(synth, 120, 168, 4)
    pol = fg._policy(capi, levels)
    trk = fg._tracker(capi, s.pair, levels, pol)
    pyr = capi.Pyramid.create(s.pair, NB, levels=levels)
    classes = MASK_CLASSES if masking else 0
    try:
        assert not any(ur.counts_dict(trk.last_fusion()).values())
        trk.set_fusing(True, GA, GR, FUSE_MAX_OBS)
        if filling:
            trk.set_filling(True, FILL_GUARD, GA, GR)
        if masking:
            trk.set_masking(MASK_CLASSES, MASK_DILATE)
        ref = Restated(capi, pyr, pol, filling, True, classes, MASK_DILATE, [2 + len(TWISTS)] * levels)
        most = dict(n_fused=0, n_gated=0, n_saturated=0, n_changed=0)
        fused_frames, later_promotions = 0, 0
        for k in range(6):
            got = trk.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            want = ref.push(s.im[k], s.dep[k], s.T0)
            fusion, fill, mask = trk.last_fusion(), trk.last_fill(), trk.last_mask()
            what = f"levels {levels}, filling {filling}, masking {masking}, push {k}"
            print(f"{what}: status {got['status']}, promoted {got['promoted']}, fusion {ur.counts_dict(fusion)}")
            fg._assert_same_result(got, want, what)
            chk = trk.last_check()
            assert chk[0].tobytes() == ref.check[0].tobytes() and chk[1:] == ref.check[1:], f"{what}: last check"
            assert mask.tobytes() == ref.mask.tobytes(), f"{what}: last mask {mask} / {ref.mask}"
            assert fill.tobytes() == ref.fill.tobytes(), f"{what}: last fill {fill} / {ref.fill}"
            assert fusion.tobytes() == ref.fusion.tobytes(), f"{what}: last fusion {fusion} / {ref.fusion}"
            plane, obs = trk.pyramid.get_reference_fused(), trk.pyramid.get_reference_fusion_obs()
            assert np.array_equal(plane, pyr.get_reference_fused()) and np.array_equal(obs, pyr.get_reference_fusion_obs()), f"{what}: the fusion's planes"
            assert np.array_equal(trk.pyramid.get_reference_fill(), pyr.get_reference_fill()), f"{what}: the fill plane"
            assert np.array_equal(trk.pyramid.get_reference_mask(), pyr.get_reference_mask()), f"{what}: the mask plane"
            assert _inputs(trk.pyramid) == _inputs(pyr), f"{what}: level inputs"
            ran = got["status"] == capi.TRACK_OK and not got["promoted"]
            assert ran or not any(ur.counts_dict(fusion).values()), f"{what}: counts without a fusion"
            if got["promoted"]:
                assert not plane.any() and not obs.any(), f"{what}: a promoted frame starts unfused"
                later_promotions += k > 0
            if ran:
                assert int(fusion["n_valid"]) > 0
                fused_frames += int(fusion["n_fused"]) > 0
                most = {n: max(most[n], int(fusion[n])) for n in most}
                mplane = trk.pyramid.get_reference_mask()
                use = (plane != 0) & (mplane == 0)
                assert np.array_equal(trk.pyramid.get_level_inputs(0)[0][use], plane[use]), f"{what}: a refined sample is not in use"
            elif not got["promoted"]:
                assert np.array_equal(plane, before_plane), f"{what}: a frame without a fusion moved the plane"
            before_plane = plane
        assert fused_frames >= 1, "no frame was tracked on the keyframe and fused into it: nothing of the fusion was shown"
        assert later_promotions >= 1, "no later frame was promoted: a keyframe's fusion was never dropped"
        assert most["n_fused"] > 0 and most["n_changed"] > 0, most
        if levels == 2:
            assert most["n_saturated"] > 0, "no frame met the cap on top of an earlier frame's observations"
        print(f"levels {levels}, filling {filling}, masking {masking}: {fused_frames} frames fused, {later_promotions} later promotions, {most}")
    finally:
        pyr.close()
        trk.close()


def test_fusing_off_is_the_tracker_of_nid_reffill(capi, synth):
    """fusing off -- set back, or never set -- gives the bytes of nid_reffill.h's tracker and no fusion"""
    s = fg.Seq(synth, 120, 168, 4)
    pol = fg._policy(capi, 2)
    a, b = fg._tracker(capi, s.pair, 2, pol), fg._tracker(capi, s.pair, 2, pol)
    try:
        for t in (a, b):
            t.set_masking(MASK_CLASSES, MASK_DILATE)
            t.set_filling(True, FILL_GUARD, GA, GR)
        b.set_fusing(True, GA, GR, 255)
        b.set_fusing(False)
        for k in range(6):
            ra, rb = a.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0), b.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            fg._assert_same_result(ra, rb, f"push {k}")
            assert _inputs(a.pyramid) == _inputs(b.pyramid)
            assert np.array_equal(a.pyramid.get_reference_mask(), b.pyramid.get_reference_mask()) and a.last_mask().tobytes() == b.last_mask().tobytes()
            assert np.array_equal(a.pyramid.get_reference_fill(), b.pyramid.get_reference_fill()) and a.last_fill().tobytes() == b.last_fill().tobytes()
            for t in (a, b):
                assert not any(ur.counts_dict(t.last_fusion()).values()) and not t.pyramid.get_reference_fused().any()
    finally:
        a.close()
        b.close()
