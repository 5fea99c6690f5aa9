"""nid_pyr on the device (include/nid/nid_pyr.h): the levels k_pyr_down makes are the host pyramid's byte for byte, a level
context is the context the host route would have made, a pyramid is reusable, nid_pyr_multistart_lm is the composition of
public calls its header states, and one chain takes the decisions of the shipped coarse-to-fine LM.  8 bins, 3 levels."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = float(np.sqrt(0.95))
NB = 8
LEVELS = 3
ITER = 4
F5000, F500 = 1.0 / 5000, 1.0 / 500

# Test 5's bound on |pose7(one chain of run_pyramid_multistart_lm) - pose7(run_pyramid_lm(fused=1))|, max over the seven
# components, both with 128-thread cost + Jacobian launches.  Measured, not chosen -- the yardstick is the shipped LM's own
# spread: the final-pose difference of run_pyramid_lm(fused=1) between the 128- and the 256-thread shape (last-bit changes
# in H and b, amplified by three levels of LM) over PYR_PARITY_SEEDS on pair A, 10 iterations per level; the chain differs
# from run_pyramid_lm at 128 threads through y*y*y against pow and the written-out sin / cos against libm, compounding
# over three levels: 10 x (the reasoning of test_multistart_gpu.PARITY_TOL).  Never more than 1e-9, the pose tolerance
# of the sharded pyramid in tests/test_multi_gpu.py.  Figures: profiles/pyr_parity.txt.
# Measured on an MI355X, seeds 0 ... 3: spread 3.671e-15, 6.505e-17, 4.718e-16, 1.081e-14; |chain - run_pyramid_lm(128)|
# 2.678e-15, 1.943e-16, 7.459e-17, 1.086e-14 -- the chain is as far from the shipped LM as the shipped LM is from itself.
PYR_PARITY_SPREAD = 1.081e-14  # max over PYR_PARITY_SEEDS, seed 103
PYR_PARITY_SEEDS = (0, 1, 2, 3)  # _starts(seed=100 + s): run_pyramid_lm takes the same decisions at 128 and 256 threads for each
PYR_PARITY_CAP = 1e-9


@pytest.fixture(scope="module")
def hostlib():
    return importlib.import_module("nid-pose-estimation_amd.hostlib")


@pytest.fixture(scope="module")
def pair_W(synth):
    """168 columns: 84 and 42 on the coarser levels -- rows that are no multiple of 4 or 8 elements; 4 / 2 / 1 cells"""
    return synth.make_pair("S", rows=120, cols=168, cell=4)


def _T(synth, pair):
    return synth.matrix_colmajor16(pair.T_wc0)


_HOST_LEVELS = {}


def _host_levels(hostlib, key, dep, im0, im1, factor):
    """[(depth_u16, im0, im1) per level]: host/nid_pyramid.cpp's own down-sampling, made once per input"""
    if key not in _HOST_LEVELS:
        out = [(np.ascontiguousarray(dep, dtype=np.uint16), np.ascontiguousarray(im0, dtype=np.uint8), np.ascontiguousarray(im1, dtype=np.uint8))]
        for _ in range(1, LEVELS):
            d, a, b = out[-1]
            out.append((hostlib.pyr_down_depth_u16(d, factor), hostlib.pyr_down_u8(a), hostlib.pyr_down_u8(b)))
        _HOST_LEVELS[key] = out
    return _HOST_LEVELS[key]


def _constructed_depth(shape):
    """counts on both sides of the validity bounds -- 0.01 m is 50 counts at 1/5000, 100 m is 50 000 counts at 1/500 --,
    the largest count and ordinary values, mixed pixel by pixel so that 2x2 blocks hold every combination"""
    rng = np.random.default_rng(20240607)
    special = np.array([0, 49, 50, 51, 49999, 50000, 50001, 65535], dtype=np.uint16)
    dep = rng.integers(1000, 30000, size=shape).astype(np.uint16)
    pick = rng.random(shape) < 0.6
    dep[pick] = special[rng.integers(0, special.size, size=int(pick.sum()))]
    return dep


@pytest.fixture(scope="module")
def pyramids(capi):
    """one pyramid per geometry, shared: {(rows, cols): [Pyramid, name of the pair it holds]}"""
    held = {}
    yield held
    for pyr, _ in held.values():
        pyr.close()


def _pyr_with(capi, synth, pyramids, pair, name, factor=F5000, dep=None, im0=None, im1=None):
    key = (pair.rows, pair.cols)
    if key not in pyramids:
        pyramids[key] = [capi.Pyramid.create(pair, NB, levels=LEVELS), None]
    slot = pyramids[key]
    if slot[1] != name:
        slot[0].set_pair_u16(pair.depth_u16 if dep is None else dep, factor, pair.im0 if im0 is None else im0,
                             pair.im1 if im1 is None else im1, _T(synth, pair))
        slot[1] = name
        for l in range(LEVELS):  # the library's defaults, whatever an earlier test set
            ctx = slot[0].level(l)
            ctx.set_math_mode(capi.MATH_FAST)
            ctx.set_options(capi.JACBOUND_CPU, capi.XFORM_QUAT)
            ctx.set_launch_shape(0, 0)
    return slot[0]


# ---- 1. the device-built inputs are the host's ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["S_edge", "W", "constructed_5000", "constructed_500", "white", "black"])
def test_levels_equal_the_host_pyramid(capi, synth, hostlib, pyramids, pair_S_edge, pair_W, case):
    pair = pair_S_edge if case == "S_edge" else pair_W
    dep, im0, im1, factor = pair.depth_u16, pair.im0, pair.im1, F5000
    if case.startswith("constructed"):
        dep, factor = _constructed_depth(pair.depth_u16.shape), (F5000 if case.endswith("5000") else F500)
    elif case in ("white", "black"):
        im0 = np.full_like(pair.im0, 255 if case == "white" else 0)
        im1 = im0.copy()
    if case == "S_edge":  # the 2x2 depth blocks of this pair hold every number of valid samples
        z = dep.astype(np.float64) * factor
        valid = ~((z < 0.01) | (z > 100))
        counts = valid[0::2, 0::2].astype(int) + valid[0::2, 1::2] + valid[1::2, 0::2] + valid[1::2, 1::2]
        assert np.bincount(counts.ravel(), minlength=5).tolist() == [255, 5, 62, 764, 3714]
    pyr = _pyr_with(capi, synth, pyramids, pair, case, factor, dep, im0, im1)
    host = _host_levels(hostlib, case, dep, im0, im1, factor)
    for l in range(LEVELS):
        got = pyr.get_level_inputs(l)
        for what, g, h in zip(("depth", "im0", "im1"), got, host[l]):
            assert g.shape == h.shape and g.dtype == h.dtype
            if g.tobytes() != h.tobytes():
                bad = np.argwhere(g != h)
                r, c = bad[0]
                raise AssertionError(f"{case}, level {l}, {what}: {len(bad)} of {g.size} elements differ, first at ({r}, {c}): "
                                     f"{g[r, c]} (device) / {h[r, c]} (host)")
    if case.startswith("constructed"):  # the case is what it says: blocks with 0 ... 4 valid samples on level 1
        z = dep.astype(np.float64) * factor
        valid = ~((z < 0.01) | (z > 100))
        counts = valid[0::2, 0::2].astype(int) + valid[0::2, 1::2] + valid[1::2, 0::2] + valid[1::2, 1::2]
        assert (np.bincount(counts.ravel(), minlength=5) > 0).all()


# ---- 2. a level context is the context the host route would have made -------------------------------------------------
def _fresh_level_context(capi, synth, pair, pyr, l, host, math, pose0):
    c = pyr.level_config(l)
    ctx = capi.Context(c.rows, c.cols, c.cell_num, NB, c.fx, c.fy, c.cx, c.cy)
    ctx.set_math_mode(math)
    d, a, b = host[l]
    cnt, href = ctx.set_pair_u16(d, F5000, a, b, _T(synth, pair), pose0)
    return ctx, cnt, href


def _same_outputs(a, b, what):
    for name, x, y in zip(("Hc", "Hj", "err", "J"), a, b):
        assert x.tobytes() == y.tobytes(), f"{what}: per-cell output {name} differs"


@pytest.mark.parametrize("math", ["FAST", "STRICT"])
@pytest.mark.parametrize("which", ["S_edge", "W"])
def test_level_context_equals_host_route(capi, synth, hostlib, pair_S_edge, pair_W, which, math):
    pair = pair_S_edge if which == "S_edge" else pair_W
    mode = capi.MATH_STRICT if math == "STRICT" else capi.MATH_FAST
    host = _host_levels(hostlib, which, pair.depth_u16, pair.im0, pair.im1, F5000)
    pyr = capi.pyramid_from_pair(pair, NB, levels=LEVELS)
    p = pair.pose_init
    poses = [p, synth.perturb_pose7(p, [1e-3, -2e-3, 5e-4], [3e-3, 1e-3, -2e-3])]
    for l in range(LEVELS):
        ctx = pyr.level(l)
        ctx.set_math_mode(mode)
        with pytest.raises(capi.NidError):  # before the reference stage: href is not set
            ctx.normal_equations(p, DELTA)
        cnt, href = ctx.compute_href(p)
        ref, cnt_r, href_r = _fresh_level_context(capi, synth, pair, pyr, l, host, mode, p)
        assert cnt.tobytes() == cnt_r.tobytes(), f"{which} {math} level {l}: in-frame counts differ\n{cnt}\n{cnt_r}"
        assert href.tobytes() == href_r.tobytes(), f"{which} {math} level {l}: reference entropies differ"
        assert (cnt >= 300).any(), "a level without an active cell checks nothing"
        for k, q in enumerate(poses):
            _same_outputs(ctx.evaluate(q, True), ref.evaluate(q, True), f"{which} {math} level {l} pose {k}")
        ref.close()
    pyr.close()


# ---- 3. a pyramid is reusable ----------------------------------------------------------------------------------------
def test_pyramid_is_reusable(capi, synth, pair_S, pair_S_edge):
    used = capi.pyramid_from_pair(pair_S_edge, NB, levels=LEVELS)
    for l in range(LEVELS):
        used.level(l).compute_href(pair_S_edge.pose_init)
    used.set_pair_u16(pair_S.depth_u16, F5000, pair_S.im0, pair_S.im1, _T(synth, pair_S))
    fresh = capi.pyramid_from_pair(pair_S, NB, levels=LEVELS)
    p = pair_S.pose_init
    for l in range(LEVELS):
        a, b = used.level(l), fresh.level(l)
        with pytest.raises(capi.NidError):  # the new pair has had no reference stage
            a.normal_equations(p, DELTA)
        for x, y in zip(used.get_level_inputs(l), fresh.get_level_inputs(l)):
            assert x.tobytes() == y.tobytes()
        ra, rb = a.compute_href(p), b.compute_href(p)
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes(), f"level {l}"
        _same_outputs(a.evaluate(p, True), b.evaluate(p, True), f"level {l}")
    # an uncollected launch on a level context: refused, nothing is overwritten under it
    ctx = used.level(1)
    before = ctx.normal_equations(p, DELTA)
    ctx.launch(5, p, DELTA)
    with pytest.raises(capi.NidError):
        used.set_pair_u16(pair_S_edge.depth_u16, F5000, pair_S_edge.im0, pair_S_edge.im1, _T(synth, pair_S_edge))
    got = ctx.wait(5)
    assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes() and got[2] == before[2]
    used.set_pair_u16(pair_S_edge.depth_u16, F5000, pair_S_edge.im0, pair_S_edge.im1, _T(synth, pair_S_edge))
    again = capi.pyramid_from_pair(pair_S_edge, NB, levels=LEVELS)
    for l in range(LEVELS):
        ra, rb = used.level(l).compute_href(p), again.level(l).compute_href(p)
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes(), f"level {l} after the refused call"
    for pyr in (used, fresh, again):
        pyr.close()


# ---- 4. nid_pyr_multistart_lm is its stated composition --------------------------------------------------------------
def _starts(synth, pair, n, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([synth.perturb_pose7(pair.pose_init, rng.normal(0, 1e-3, 3), rng.normal(0, 2e-3, 3)) for _ in range(n)])


def _out_of_frame_start(synth, pair, ctx):
    """a pose further and further off until no cell has a sample in frame: n_active counts the cells the REFERENCE stage
    left active, so such a pose shows as a chi2 that is not finite (ctx: a context with its reference stage done)"""
    for k in (2, 4, 8, 16, 32):
        p = synth.perturb_pose7(pair.pose_init, [0.0, 0.03, 0.0], [0.25 * k, -0.15 * k, 0.0])
        if not np.isfinite(ctx.normal_equations(p, DELTA)[2]):
            return p
    raise AssertionError("no start without a cell in frame found")


def _composition(capi, pyr, starts, iterations, pose_ref, keep):
    """the schedule of nid_pyr.h from public calls on the pyramid's own level contexts"""
    L, n = pyr.levels, len(starts)
    kp = [n] * L if keep is None else list(keep)
    res = np.zeros((L, n), dtype=capi.MS_RESULT_DTYPE)
    origin = np.full((L, n), -1, dtype=np.int32)
    rounds = np.zeros(L, dtype=np.int32)
    best_origin, best_pose = -1, np.zeros(7)
    cur, cur_o = np.array(starts, dtype=np.float64), np.arange(n, dtype=np.int32)
    for l in range(L - 1, -1, -1):
        ctx, row, m = pyr.level(l), L - 1 - l, len(cur)
        ctx.compute_href(pose_ref if (l == L - 1 and pose_ref is not None) else cur[0])
        r, _, rd = ctx.multistart_lm(cur, iterations, DELTA)
        res[row, :m], origin[row, :m], rounds[row] = r, cur_o, rd
        idx = np.flatnonzero((r["n_active"] > 0) & np.isfinite(r["chi2"]))
        if idx.size == 0:
            break
        order = idx[np.argsort(r["chi2"][idx] / r["n_active"][idx].astype(np.float64), kind="stable")]
        if l == 0:
            best_origin, best_pose = int(cur_o[order[0]]), r["pose7"][order[0]].copy()
            break
        order = order[:kp[l - 1]]
        cur, cur_o = r["pose7"][order].copy(), cur_o[order]
    return res, origin, rounds, best_origin, best_pose


def _assert_same_run(dev, ref, what):
    for name, d, r in zip(("results", "origin", "rounds"), dev[:3], ref[:3]):
        assert d.tobytes() == r.tobytes(), f"{what}: {name} differ\n{d}\n{r}"
    assert dev[3] == ref[3], f"{what}: best_origin {dev[3]} / {ref[3]}"
    assert dev[4].tobytes() == ref[4].tobytes(), f"{what}: best_pose7"


@pytest.mark.parametrize("keep", ["none", "1_2_n", "n_n_n"])
@pytest.mark.parametrize("n", [1, 5, 17])
@pytest.mark.parametrize("which", ["S_edge", "S"])
def test_multistart_is_its_composition(capi, synth, pyramids, pair_S, pair_S_edge, which, n, keep):
    pair = pair_S_edge if which == "S_edge" else pair_S
    pyr = _pyr_with(capi, synth, pyramids, pair, which)
    starts = np.concatenate([pair.pose_init[None], _starts(synth, pair, n)])[:n]
    # (a second level cannot start more chains than the one below ran: with one chain `[1, 2, n]` is a bad argument)
    kp = {"none": None, "1_2_n": [1, min(2, n), n], "n_n_n": [n, n, n]}[keep]
    if keep == "1_2_n" and n == 1:
        with pytest.raises(capi.NidError):
            pyr.multistart_lm(starts, ITER, DELTA, keep=[1, 2, n])
    ref_pose = None if n == 5 else pair.pose_init
    dev = pyr.multistart_lm(starts, ITER, DELTA, pose_ref=ref_pose, keep=kp)
    ref = _composition(capi, pyr, starts, ITER, ref_pose, kp)
    _assert_same_run(dev, ref, f"{which}, n = {n}, keep = {kp}")
    res, origin, rounds, best, best_pose = dev
    assert best >= 0 and (rounds >= 2).all()
    want = [n, n, n] if kp is None else kp[::-1]
    assert [(origin[row] >= 0).sum() for row in range(LEVELS)] == want, "every start of this cloud is eligible on every level"
    assert (res["status"][origin >= 0] != capi.MS_RUNNING).all()


def test_multistart_out_of_frame_start_and_side_effects(capi, synth, pyramids, pair_S):
    pyr = _pyr_with(capi, synth, pyramids, pair_S, "S")
    probe = _starts(synth, pair_S, 3, seed=3)

    def slots():
        out = []
        for l in range(LEVELS):
            ctx = pyr.level(l)
            ctx.compute_href(pair_S.pose_init)
            ctx.launch_batch(0, probe, DELTA)
            out.append([ctx.wait(k) for k in range(len(probe))])
        return out

    before = slots()
    # (found on the coarsest level, whose one cell is the whole image: out of frame there is out of frame on every level)
    far = _out_of_frame_start(synth, pair_S, pyr.level(LEVELS - 1))
    assert not any(np.isfinite(pyr.level(l).normal_equations(far, DELTA)[2]) for l in range(LEVELS))
    n = 6
    starts = np.concatenate([_starts(synth, pair_S, 2), far[None], _starts(synth, pair_S, 3, seed=12)])
    dev = pyr.multistart_lm(starts, ITER, DELTA, pose_ref=pair_S.pose_init)
    _assert_same_run(dev, _composition(capi, pyr, starts, ITER, pair_S.pose_init, None), "with an out-of-frame start")
    res, origin, rounds, best, best_pose = dev
    assert origin[0].tolist() == list(range(n)) and not np.isfinite(res["chi2"][0, 2])
    assert 2 not in origin[1] and 2 not in origin[2], "the out-of-frame start is never carried to a finer level"
    assert (origin[1] >= 0).sum() == n - 1 and (origin[2] >= 0).sum() == n - 1 and best not in (-1, 2)
    # alone: no eligible chain on the coarsest level -- NID_OK, no best, the finer levels' rows untouched zeros
    res, origin, rounds, best, best_pose = pyr.multistart_lm(far[None], ITER, DELTA)
    assert best == -1 and origin.tolist() == [[0], [-1], [-1]] and rounds[0] >= 1 and rounds[1:].tolist() == [0, 0]
    assert res[1:].tobytes() == bytes(res[1:].nbytes) and best_pose.tobytes() == bytes(56)
    assert res["status"][0, 0] != capi.MS_RUNNING
    _assert_same_run((res, origin, rounds, best, best_pose), _composition(capi, pyr, far[None], ITER, None, None), "the out-of-frame start alone")
    # the public slots of every level context: the same bytes as before
    after = slots()
    for l in range(LEVELS):
        for a, b in zip(before[l], after[l]):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3], f"level {l}"
    # bad arguments
    five = _starts(synth, pair_S, 5)
    for bad in (np.zeros((0, 7)), np.tile(pair_S.pose_init, (257, 1))):
        with pytest.raises(capi.NidError):
            pyr.multistart_lm(bad, ITER, DELTA)
    for bad_keep in ([5, 2, 5], [1, 2, 4], [0, 2, 5], [1, 6, 5]):
        with pytest.raises(capi.NidError):
            pyr.multistart_lm(five, ITER, DELTA, keep=bad_keep)
    with pytest.raises(capi.NidError):
        pyr.multistart_lm(five, 0, DELTA)
    ctx = pyr.level(1)
    ctx.launch(5, pair_S.pose_init, DELTA)
    with pytest.raises(capi.NidError):
        pyr.multistart_lm(five, ITER, DELTA)
    ctx.wait(5)
    pyr.multistart_lm(five, ITER, DELTA)


# ---- 5. one chain against the shipped coarse-to-fine LM ----------------------------------------------------------------
def _trials_per_outer(tr_k):
    out, n = [], 0
    for t in tr_k:
        if t["flags"] & 1 or not t["flags"] & (2 | 4):
            continue
        n += 1
        if t["flags"] & 8:
            out.append(n)
            n = 0
        if t["flags"] & 32:
            break
    return out


def test_one_chain_against_the_shipped_pyramid_lm(capi, synth, hostlib, pair_A):
    """hostlib.run_pyramid_multistart_lm with one start against hostlib.run_pyramid_lm(fused=1) from the same start, both
    with 128-thread launches (pair A, 16 / 8 / 4 cells, 10 iterations per level): the same lm_trials per outer iteration
    on every level, the final pose within 10 x the shipped LM's own 128- / 256-thread spread (at most 1e-9)."""
    iters = 10
    starts = np.stack([_starts(synth, pair_A, 1, seed=100 + s)[0] for s in PYR_PARITY_SEEDS])
    # the per-round detail of the chain comes from a pyramid of the test's own with the host layer's options
    pyr = capi.pyramid_from_pair(pair_A, NB, levels=LEVELS)
    for l in range(LEVELS):
        ctx = pyr.level(l)
        ctx.set_options(capi.JACBOUND_CPU, capi.XFORM_MATRIX)
        ctx.set_launch_shape(128, 0)
    worst, spread_max = 0.0, 0.0
    try:
        for k, p0 in enumerate(starts):
            seed = PYR_PARITY_SEEDS[k]
            runs = {}
            for nt in (128, 256):
                hostlib.set_launch_shape(nt, 0)
                runs[nt] = hostlib.run_pyramid_lm(pair_A, NB, p0, levels=LEVELS, iterations=iters, fused=1)
            trials = {nt: [[r["lm_trials"] for r in lv] for lv in runs[nt][1]] for nt in runs}
            # a start on a decision edge of the shipped LM itself is replaced, not tolerated
            assert trials[128] == trials[256], f"seed {seed}: run_pyramid_lm decides differently at 128 and 256 threads: choose another start"
            hostlib.set_launch_shape(128, 0)
            res, origin, rounds, best, best_pose = hostlib.run_pyramid_multistart_lm(pair_A, NB, p0[None], levels=LEVELS, iterations=iters)
            assert best == 0 and origin.tolist() == [[0]] * LEVELS
            start = p0
            for row in range(LEVELS):
                l = LEVELS - 1 - row
                assert res["outer_iterations"][row, 0] == len(trials[128][row]) and res["trials"][row, 0] == sum(trials[128][row]), \
                    f"seed {seed}, level {l}: {res['outer_iterations'][row, 0]} outer iterations / {res['trials'][row, 0]} trials, run_pyramid_lm {trials[128][row]}"
                ctx = pyr.level(l)
                ctx.compute_href(start)
                one, _, rd, tr = ctx.multistart_lm(start[None], iters, DELTA, trace=True)
                assert one.tobytes() == res[row].tobytes() and rd == rounds[row], f"seed {seed}, level {l}: the host layer's level contexts are not set up like the operators'"
                assert _trials_per_outer(tr[:, 0]) == trials[128][row], f"seed {seed}, level {l}"
                start = res["pose7"][row, 0]
            assert best_pose.tobytes() == res["pose7"][LEVELS - 1, 0].tobytes()
            d = float(np.abs(best_pose - runs[128][0]).max())
            spread = float(np.abs(runs[128][0] - runs[256][0]).max())
            print(f"seed {seed}: |pyramid multistart - run_pyramid_lm(128)| = {d:.3e}, run_pyramid_lm 128 / 256 spread {spread:.3e}, "
                  f"trials per level {trials[128]}")
            worst, spread_max = max(worst, d), max(spread_max, spread)
    finally:
        hostlib.set_launch_shape(-1, 0)
        hostlib.release_pyramid()
        pyr.close()
    print(f"largest spread {spread_max:.3e}, largest difference {worst:.3e}")
    tol = 10 * PYR_PARITY_SPREAD
    assert tol <= PYR_PARITY_CAP, f"10 x the measured spread ({tol:.3e}) is above the project's pose tolerance {PYR_PARITY_CAP:.0e}"
    assert worst <= tol, f"final poses differ by {worst:.3e} > {tol:.3e}"
