"""include/nid/nid_refgather.h on the device: the planes and the counts of nid_pyr_fuse_reference_depth_bilinear equal
nid_refgather_host's and a numpy restatement's; a gathered pyramid is the pyramid of the pair with the refined samples
written in, bit for bit, with a fill and a mask present; nid_pyr_clear_reference_fusion serves a gather; the state rules;
the tracker with bilinear sampling is the composition its header states, and with nearest sampling it is
nid_reffuse.h's.  The geometries, the scene, the six-frame sequence and the helpers are tests/test_reffill_gpu.py's and
tests/test_reffuse_gpu.py's: 120 x 168 with three levels and 122 x 174 with two -- 20 160 and 21 228 pixels, neither a
multiple of k_refgather_apply's 1024-pixel span, both multiples of a lane's four pixels: the lane that makes a plane's last
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


gr = _load("refgather_restate")
ug = _load("test_reffuse_gpu")  # (its helpers and its restated tracker; its tests are not collected from here)
fg = ug.fg
ur, fr, rr = gr.ur, gr.fr, gr.rr

DELTA, NB, F5000 = fg.DELTA, fg.NB, fg.F5000
GA, GR = gr.GATE_ABS, gr.GATE_REL
TA, TR = 50, 20  # the tap gate: counts of the depth factor, 1024ths of the smallest tap
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


# ---- 1. the gather equals the host twin and the restatement -------------------------------------------------------------------
# ("g", pose, gate_abs, gate_rel_1024, max_obs, tap_abs, tap_rel_1024), ("f", pose, gate_abs, gate_rel_1024, max_obs): a
# nearest-splat fusion, or "fill": each on the planes the one before left
CALLS = (("g", "pose", GA, GR, 1, TA, TR), ("g", "pose", GA, GR, 1, TA, TR), ("f", "pose_out", GA, GR, 2), "fill", ("g", "pose_out", 0, 0, 2, TA, TR),
         ("g", "pose", 10, 0, 255, 5, 0), ("g", "pose_out", GA, GR, 255, TA, TR))


@pytest.mark.parametrize("which", ["W", "O"])
def test_gather_equals_the_host(capi, synth, scenes, pyramids, which):
    """five gathers at both poses with a nearest-splat fusion and a fill among them, under a mask: FUSED, OBS and the counts
    from the device equal the host twin's (and the restatement's); the mask and the fill plane do not move"""
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
    seen = {n: 0 for n in gr.COUNT_NAMES}
    for k, call in enumerate(CALLS):
        what = f"{which}, call {k}: {call}"
        if call == "fill":  # in between: on the BASE plane, and the fusion's planes stay
            cnt = pyr.fill_reference_depth(s.pose_out, 1, GA, GR, 0)
            fill, host_cnt = capi.reffill_host(cfg, gr.base(fused, s.dep0), F5000, s.T0, s.dep1, F5000, s.pose_out, 1, GA, GR)
            assert np.array_equal(pyr.get_reference_fill(), fill) and cnt.tobytes() == host_cnt.tobytes() and fill.any()
            assert np.array_equal(pyr.get_reference_fused(), fused) and np.array_equal(pyr.get_reference_fusion_obs(), K)
        elif call[0] == "f":
            _, name, ga, g_rel, mo = call
            cnt = pyr.fuse_reference_depth(getattr(s, name), ga, g_rel, mo)
            S, K, fused, host_cnt = capi.reffuse_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, getattr(s, name), ga, g_rel, mo, S, K)
            assert cnt.tobytes() == host_cnt.tobytes() and int(cnt["n_fused"]) > 0, what
            assert np.array_equal(pyr.get_reference_fused(), fused) and np.array_equal(pyr.get_reference_fusion_obs(), K), what
        else:
            _, name, ga, g_rel, mo, ta, tr = call
            cnt = pyr.fuse_reference_depth_bilinear(getattr(s, name), ga, g_rel, mo, ta, tr)
            args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, getattr(s, name), ga, g_rel, mo, ta, tr, S, K)
            S, K, fused, host_cnt = capi.refgather_host(*args)
            wS, wK, wF, want_cnt, margin = gr.restate(*args)
            worst = min(worst, margin)
            print(f"{what}: {gr.counts_dict(cnt)}, smallest margin {margin:.3e}")
            assert np.array_equal(S, wS) and np.array_equal(K, wK) and np.array_equal(fused, wF) and gr.counts_dict(host_cnt) == want_cnt, \
                f"{what}: the host twin and the restatement"
            got = pyr.get_reference_fused()
            assert np.array_equal(got, fused), f"{what}: {int((got != fused).sum())} entries of the FUSED plane differ from the host's"
            assert np.array_equal(pyr.get_reference_fusion_obs(), K), f"{what}: the OBS plane"
            assert cnt.tobytes() == host_cnt.tobytes(), f"{what}: counts {cnt} / {host_cnt}"
            seen = {n: max(seen[n], want_cnt[n]) for n in seen}
        assert np.array_equal(pyr.get_reference_mask(), mask), f"call {k}: the mask plane moved"
        assert np.array_equal(pyr.get_reference_fill(), fill), f"call {k}: the fill plane moved"
        # the effective reference: level 0's depth is mask ? 0 : (fill ? fill : (fused ? fused : uploaded))
        assert np.array_equal(pyr.get_level_inputs(0)[0], np.where(mask != 0, 0, gr.completed(fill, fused, s.dep0)).astype(np.uint16)), f"call {k}"
    assert worst > 1e-9, "a decision of the scene hangs on a last bit"
    assert all(v > 0 for v in seen.values()), f"a branch of the rule was never reached: {seen}"
    assert seen["n_fused"] > 10000 and seen["n_gated"] > 5000 and seen["n_saturated"] > 5000 and seen["n_tap_refused"] > 10000, seen
    assert ((mask != 0) & (fused != 0)).any() and int(K.max()) > 2


def test_plane_sizes_around_a_lane(capi, synth):
    """k_refgather_apply's last lane: planes of 4 n + 3, 4 n + 2 and 4 n + 1 pixels (a lane makes four) and one of exactly
    five workgroups' spans -- each against the host twin, twice on the same state."""
    for rows, cols, rest in ((65, 75, 3), (65, 78, 2), (65, 77, 1), (64, 80, 0)):
        assert (rows * cols) % 4 == rest and (rest or rows * cols == 5 * 1024)
        s = rr.Scene(synth, rows, cols, 4)
        cfg = s.cfg(capi, NB)
        pyr = capi.Pyramid.create(s.pair, NB, levels=1)
        try:
            _fresh(pyr, s)
            S = K = None
            for ga, mo in ((GA, 255), (5, 2)):
                cnt = pyr.fuse_reference_depth_bilinear(s.pose, ga, GR, mo, TA, TR)
                S, K, fused, host_cnt = capi.refgather_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, s.pose, ga, GR, mo, TA, TR, S, K)
                assert np.array_equal(pyr.get_reference_fused(), fused) and np.array_equal(pyr.get_reference_fusion_obs(), K), (rows, cols)
                assert cnt.tobytes() == host_cnt.tobytes() and int(cnt["n_fused"]) + int(cnt["n_saturated"]) > 0, (rows, cols, cnt)
                assert np.array_equal(pyr.get_level_inputs(0)[0], gr.base(fused, s.dep0)), (rows, cols)
        finally:
            pyr.close()


# ---- 2. a gathered pyramid is the pyramid of the refined depth ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_gathered_pyramid_equals_the_refined_depth(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    poses = (s.pose, synth.perturb_pose7(s.pose0, [0, 0, 0], [-0.45, 0.3, 0]))
    caller = _caller(s)
    X.set_reference_mask(caller)
    X.fuse_reference_depth_bilinear(s.pose_out, GA, GR, 255, TA, TR)
    X.fill_reference_depth(s.pose, 1, GA, GR, 0)
    mask, fill = X.get_reference_mask(), X.get_reference_fill()
    cnt = X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)
    fused = X.get_reference_fused()
    assert np.array_equal(X.get_reference_mask(), mask) and np.array_equal(X.get_reference_fill(), fill), "the call moved the mask or the fill plane"
    assert int(cnt["n_fused"]) > 10000 and int((fused != 0).sum()) > 10000 and int((fill != 0).sum()) > 1000 and mask.any()
    comp = gr.completed(fill, fused, s.dep0)
    assert int((comp != s.dep0).sum()) > 2000
    _fresh(Y, s, comp)
    Y.set_reference_mask(caller)
    assert np.array_equal(Y.get_reference_mask(), mask) and _inputs(X) == _inputs(Y)
    for k, pose in enumerate(poses):
        ex, ey = _evaluations(X, pose), _evaluations(Y, pose)
        for l in range(X.levels):
            for name, a, b in zip(("N_c", "Href", "Hc", "Hj", "err", "J"), ex[l], ey[l]):
                assert a == b, f"{which}, pose {k}, level {l}: {name}"
    starts = _starts(synth, s.pose)
    rx, ry = X.multistart_lm(starts, 5, DELTA), Y.multistart_lm(starts, 5, DELTA)
    assert rx[0].tobytes() == ry[0].tobytes() and rx[1].tobytes() == ry[1].tobytes() and rx[2].tobytes() == ry[2].tobytes()
    assert rx[3] == ry[3] and rx[4].tobytes() == ry[4].tobytes() and np.isfinite(rx[0]["chi2"]).any()
    # a mask behind a gather classifies the refined samples, on either pyramid
    cx, cy = X.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 1, 0), Y.mask_occluded(s.pose, TOL_ABS, TOL_REL, 6, 1, 0)
    assert cx.tobytes() == cy.tobytes() and np.array_equal(X.get_reference_mask(), Y.get_reference_mask()) and _inputs(X) == _inputs(Y)
    assert np.array_equal(X.get_reference_fused(), fused), "a masking call moved the fusion"


# ---- 3. the clear serves a gather; a new reference starts unfused -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["W", "O"])
def test_clear_behind_gathers_alone(capi, synth, scenes, pyramids, which):
    s = scenes[which]
    cfg = s.cfg(capi, NB)
    X, Y = pyramids[which, "X"], pyramids[which, "Y"]
    _fresh(X, s)
    _fresh(Y, s)  # never fused
    never = _inputs(Y)
    ev_never = _evaluations(Y, s.pose)
    first = X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)
    fused = X.get_reference_fused()
    assert int(first["n_changed"]) > 1000 and _inputs(X) != never
    X.fuse_reference_depth_bilinear(s.pose_out, GA, GR, 255, TA, TR)
    X.clear_reference_fusion()  # behind gathers alone: not a no-op
    assert not X.get_reference_fused().any() and not X.get_reference_fusion_obs().any() and _inputs(X) == never
    assert _evaluations(X, s.pose) == ev_never
    X.clear_reference_fusion()  # twice
    assert _inputs(X) == never
    again = X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)
    assert np.array_equal(X.get_reference_fused(), fused) and again.tobytes() == first.tobytes()
    # with a fill and a mask: the clear keeps both and gives the never-fused pyramid's bits
    caller = _caller(s)
    _fresh(X, s)
    for pyr in (X, Y):
        pyr.set_reference_mask(caller)
        pyr.fill_reference_depth(s.pose_out, 0, GA, GR, 0)  # (guard 0: the fill reads no neighbour's BASE)
    X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)
    assert _inputs(X) != _inputs(Y)
    X.clear_reference_fusion()
    assert np.array_equal(X.get_reference_fill(), Y.get_reference_fill()) and X.get_reference_fill().any()
    assert np.array_equal(X.get_reference_mask(), Y.get_reference_mask()) and X.get_reference_mask().any()
    assert _inputs(X) == _inputs(Y)

    # a new reference starts unfused: the pair call and both promotions
    T1 = capi.pose_to_Twc16(s.pose)
    for renew in (lambda: _fresh(X, s), lambda: X.promote_resident_target(T1), lambda: X.promote_target(s.dep1, F5000, T1)):
        _fresh(X, s)
        assert int(X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)["n_fused"]) > 10000 and X.get_reference_fused().any()
        renew()
        assert not X.get_reference_fused().any() and not X.get_reference_fusion_obs().any()
        X.clear_reference_fusion()  # nothing to clear behind a new reference
        assert not X.get_reference_fused().any()
    assert np.array_equal(X.get_level_inputs(0)[0], s.dep1)
    # ... and the first gather behind a promotion starts from ITS depth and matrix: the old keyframe's depth on the target
    X.set_target(s.pair.im0)
    X.set_target_depth(s.dep0, F5000)
    cnt = X.fuse_reference_depth_bilinear(s.pose0, GA, GR, 255, TA, TR)
    _, K, host, host_cnt = capi.refgather_host(cfg, s.dep1, F5000, T1, s.dep0, F5000, s.pose0, GA, GR, 255, TA, TR)
    assert np.array_equal(X.get_reference_fused(), host) and np.array_equal(X.get_reference_fusion_obs(), K) and cnt.tobytes() == host_cnt.tobytes()
    assert int(cnt["n_fused"]) > 1000


# ---- 4. state rules -------------------------------------------------------------------------------------------------------------
def test_state_rules(capi, synth, scenes, pyramids):
    s = scenes["W"]
    levels = GEOMETRY["W"][3]
    fresh = capi.Pyramid.create(s.pair, NB, levels=levels)
    try:
        with pytest.raises(capi.NidError, match="call order"):
            fresh.fuse_reference_depth_bilinear(s.pose)  # no reference
        fresh.set_pair_u16(s.dep0, F5000, s.pair.im0, s.im1, s.T0)
        ctx = fresh.level(0)
        ctx.compute_href(s.pose)
        want = ctx.evaluate(s.pose, True)
        before = _inputs(fresh)
        with pytest.raises(capi.NidError, match="call order"):
            fresh.fuse_reference_depth_bilinear(s.pose)  # no target depth
        assert _inputs(fresh) == before and not fresh.get_reference_fused().any() and not fresh.get_reference_fusion_obs().any()
        for a, b in zip(want, ctx.evaluate(s.pose, True)):  # the refused call left the reference, its reference stage included
            assert a.tobytes() == b.tobytes()
    finally:
        fresh.close()

    # an uncollected launch on a level: the call refuses and changes nothing; the public slots are untouched by a gather
    X = pyramids["W", "X"]
    _fresh(X, s)
    X.fuse_reference_depth_bilinear(s.pose, GA, GR, 255, TA, TR)
    fused, obs = X.get_reference_fused(), X.get_reference_fusion_obs()
    ctx = X.level(1)
    ctx.compute_href(s.pose)
    want = ctx.normal_equations(s.pose, DELTA)
    before = _inputs(X)
    ctx.launch(5, s.pose, DELTA)
    with pytest.raises(capi.NidError, match="call order"):
        X.fuse_reference_depth_bilinear(s.pose)
    got = ctx.wait(5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert _inputs(X) == before and np.array_equal(X.get_reference_fused(), fused) and np.array_equal(X.get_reference_fusion_obs(), obs)
    reduced_dev, cellout_dev = ctx.slot_buffers(5)
    slot = (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    X.fuse_reference_depth_bilinear(s.pose_out, GA, GR, 255, TA, TR)
    assert slot == (ctx.read_device(reduced_dev, capi.NID_REDUCED_LEN).tobytes(), ctx.read_device(cellout_dev, (ctx.ncell, capi.NID_CELL_OUT)).tobytes())
    with pytest.raises(capi.NidError, match="call order"):
        ctx.evaluate(s.pose, True)  # as behind a promotion: a reference, no reference stage
    ctx.compute_href(s.pose)
    assert np.isfinite(ctx.normal_equations(s.pose, DELTA)[2])

    # the argument rules behind a good handle
    lib = capi.load()
    q = np.ascontiguousarray(s.pose)
    dp = lambda a: a.ctypes.data_as(capi.c_dp)
    X.clear_reference_fusion()
    before = _inputs(X)
    bad = ((-1, 20, 255, 50, 20), (65536, 20, 255, 50, 20), (50, -1, 255, 50, 20), (50, 1025, 255, 50, 20), (50, 20, 0, 50, 20), (50, 20, 256, 50, 20),
           (50, 20, 255, -1, 20), (50, 20, 255, 65536, 20), (50, 20, 255, 50, -1), (50, 20, 255, 50, 1025))
    for a in bad:
        assert lib.nid_pyr_fuse_reference_depth_bilinear(X.h, dp(q), *a, None) == -1, a
    assert lib.nid_pyr_fuse_reference_depth_bilinear(X.h, None, 50, 20, 255, 50, 20, None) == -1
    assert _inputs(X) == before and not X.get_reference_fused().any(), "a refused argument touched the pyramid"
    assert lib.nid_pyr_fuse_reference_depth_bilinear(X.h, dp(q), 65535, 1024, 255, 65535, 1024, None) == 0  # counts are optional
    trk = capi.Tracker.create(s.pair, NB, levels=levels)
    try:
        for mode, ta, tr in ((-1, 50, 20), (2, 50, 20), (1, -1, 20), (1, 65536, 20), (0, 50, -1), (0, 50, 1025)):
            assert lib.nid_track_set_fusion_sampling(trk.h, mode, ta, tr) == -1, (mode, ta, tr)
        assert lib.nid_track_set_fusion_sampling(trk.h, 1, 65535, 1024) == 0 and lib.nid_track_set_fusion_sampling(trk.h, 0, 0, 0) == 0
        assert lib.nid_track_last_gather(trk.h, None) == -1
        assert not any(gr.counts_dict(trk.last_gather()).values())
    finally:
        trk.close()


# ---- 5. the tracker is its composition ------------------------------------------------------------------------------------------
MASK_CLASSES, MASK_DILATE, FILL_GUARD, TWISTS = fg.MASK_CLASSES, fg.MASK_DILATE, fg.FILL_GUARD, fg.TWISTS
FUSE_MAX_OBS = ug.FUSE_MAX_OBS


class _Bilinear:
    """a Pyramid whose step 5d'' gathers: tests/test_reffuse_gpu.py's Restated schedule calls fuse_reference_depth with
    nid_track_set_fusing's gate and cap; here that call is nid_pyr_fuse_reference_depth_bilinear with the tap gate, its counts
    kept aside, and what the schedule records as the push's nearest-splat fusion is zeros"""

    def __init__(self, capi, pyr):
        self._capi, self._pyr = capi, pyr
        self.gather = np.zeros(1, dtype=capi.REFGATHER_COUNTS_DTYPE)[0]

    def __getattr__(self, name):
        return getattr(self._pyr, name)

    def fuse_reference_depth(self, pose7, gate_abs, gate_rel_1024, max_obs):
        self.gather = self._pyr.fuse_reference_depth_bilinear(pose7, gate_abs, gate_rel_1024, max_obs, TA, TR)
        return np.zeros(1, dtype=self._capi.REFFUSE_COUNTS_DTYPE)[0]


@pytest.mark.parametrize("levels,filling,masking", [(3, False, False), (3, True, True), (2, False, False), (2, True, True)])
def test_tracker_is_its_composition(capi, synth, levels, filling, masking):
    """Six pushes under on-demand keyframes with a maximal age, verification on, an occluder from frame 3 on, sampling
    BILINEAR: every result, last check, last mask, last fill, last gather, every plane and level input equal to the
    restatement's from public calls, whatever the status; nid_track_last_fusion reads zeros."""
    s = fg.Seq(synth, 120, 168, 4)
    pol = fg._policy(capi, levels)
    trk = fg._tracker(capi, s.pair, levels, pol)
    pyr = capi.Pyramid.create(s.pair, NB, levels=levels)
    classes = MASK_CLASSES if masking else 0
    try:
        assert not any(gr.counts_dict(trk.last_gather()).values())
        trk.set_fusing(True, GA, GR, FUSE_MAX_OBS)
        trk.set_fusion_sampling(capi.REFFUSE_BILINEAR, TA, TR)
        if filling:
            trk.set_filling(True, FILL_GUARD, GA, GR)
        if masking:
            trk.set_masking(MASK_CLASSES, MASK_DILATE)
        proxy = _Bilinear(capi, pyr)
        ref = ug.Restated(capi, proxy, pol, filling, True, classes, MASK_DILATE, [2 + len(TWISTS)] * levels)
        most = {n: 0 for n in gr.COUNT_NAMES}
        gathered_frames, later_promotions = 0, 0
        for k in range(6):
            got = trk.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            proxy.gather = np.zeros(1, dtype=capi.REFGATHER_COUNTS_DTYPE)[0]
            want = ref.push(s.im[k], s.dep[k], s.T0)
            gather, fusion, fill, mask = trk.last_gather(), trk.last_fusion(), trk.last_fill(), trk.last_mask()
            what = f"levels {levels}, filling {filling}, masking {masking}, push {k}"
            print(f"{what}: status {got['status']}, promoted {got['promoted']}, gather {gr.counts_dict(gather)}")
            fg._assert_same_result(got, want, what)
            chk = trk.last_check()
            assert chk[0].tobytes() == ref.check[0].tobytes() and chk[1:] == ref.check[1:], f"{what}: last check"
            assert mask.tobytes() == ref.mask.tobytes(), f"{what}: last mask {mask} / {ref.mask}"
            assert fill.tobytes() == ref.fill.tobytes(), f"{what}: last fill {fill} / {ref.fill}"
            assert gather.tobytes() == proxy.gather.tobytes(), f"{what}: last gather {gather} / {proxy.gather}"
            assert not any(ur.counts_dict(fusion).values()), f"{what}: nid_track_last_fusion reads {fusion} with sampling BILINEAR"
            plane, obs = trk.pyramid.get_reference_fused(), trk.pyramid.get_reference_fusion_obs()
            assert np.array_equal(plane, pyr.get_reference_fused()) and np.array_equal(obs, pyr.get_reference_fusion_obs()), f"{what}: the fusion's planes"
            assert np.array_equal(trk.pyramid.get_reference_fill(), pyr.get_reference_fill()), f"{what}: the fill plane"
            assert np.array_equal(trk.pyramid.get_reference_mask(), pyr.get_reference_mask()), f"{what}: the mask plane"
            assert _inputs(trk.pyramid) == _inputs(pyr), f"{what}: level inputs"
            ran = got["status"] == capi.TRACK_OK and not got["promoted"]
            assert ran or not any(gr.counts_dict(gather).values()), f"{what}: counts without a gather"
            if got["promoted"]:
                assert not plane.any() and not obs.any(), f"{what}: a promoted frame starts unfused"
                later_promotions += k > 0
            if ran:
                assert int(gather["n_valid"]) > 0
                gathered_frames += int(gather["n_fused"]) > 0
                most = {n: max(most[n], int(gather[n])) for n in most}
        assert gathered_frames >= 1, "no frame was tracked on the keyframe and gathered into it: nothing of the feature was shown"
        assert later_promotions >= 1, "no later frame was promoted: a keyframe's fusion was never dropped"
        assert most["n_fused"] > 0 and most["n_sampled"] > 0, most
        print(f"levels {levels}, filling {filling}, masking {masking}: {gathered_frames} frames gathered, {later_promotions} later promotions, {most}")
    finally:
        pyr.close()
        trk.close()


def test_sampling_nearest_is_the_tracker_of_nid_reffuse(capi, synth):
    """sampling NEAREST -- never set, set with mode 0 and a tap gate, or set to BILINEAR and back -- gives the bytes of
    nid_reffuse.h's tracker, its fusion counts included, and no gather"""
    s = fg.Seq(synth, 120, 168, 4)
    pol = fg._policy(capi, 2)
    a, b, c = (fg._tracker(capi, s.pair, 2, pol) for _ in range(3))
    try:
        for t in (a, b, c):
            t.set_masking(MASK_CLASSES, MASK_DILATE)
            t.set_filling(True, FILL_GUARD, GA, GR)
            t.set_fusing(True, GA, GR, 255)
        b.set_fusion_sampling(capi.REFFUSE_NEAREST, 7, 3)
        c.set_fusion_sampling(capi.REFFUSE_BILINEAR, TA, TR)
        c.set_fusion_sampling(capi.REFFUSE_NEAREST, TA, TR)
        fused_frames = 0
        for k in range(6):
            ra = a.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
            for t in (b, c):
                rt = t.push(s.im[k], s.dep[k], F5000, T_wc_first=s.T0)
                fg._assert_same_result(ra, rt, f"push {k}")
                assert _inputs(a.pyramid) == _inputs(t.pyramid)
                assert np.array_equal(a.pyramid.get_reference_mask(), t.pyramid.get_reference_mask()) and a.last_mask().tobytes() == t.last_mask().tobytes()
                assert np.array_equal(a.pyramid.get_reference_fill(), t.pyramid.get_reference_fill()) and a.last_fill().tobytes() == t.last_fill().tobytes()
                assert np.array_equal(a.pyramid.get_reference_fused(), t.pyramid.get_reference_fused())
                assert np.array_equal(a.pyramid.get_reference_fusion_obs(), t.pyramid.get_reference_fusion_obs())
                assert a.last_fusion().tobytes() == t.last_fusion().tobytes()
            for t in (a, b, c):
                assert not any(gr.counts_dict(t.last_gather()).values())
            fused_frames += int(a.last_fusion()["n_fused"]) > 0
        assert fused_frames >= 1, "no frame was fused: the comparison showed nothing"
    finally:
        for t in (a, b, c):
            t.close()
