"""nid_multistart_lm on the device: many Levenberg-Marquardt chains advanced by one evaluation grid per round and stepped
by k_lm_step (include/nid/nid_multistart.h).  The reference of the bit-for-bit tests is a loop of existing public calls:
launch_batch(want_jac) + wait per round, capi.lm_step_host (the same function, compiled for the host) per chain."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = float(np.sqrt(0.95))
NB = 8
ITER = 6

# Test 4's bound on |pose7(multi-start chain) - pose7(run_lm(fused=1))|, max over the seven components.  Measured, not
# assumed: the final-pose spread of run_lm(fused=1) itself between the cost + Jacobian shapes 128 and 256 -- the LM's own
# amplification of last-bit changes in H and b -- over the starts below (pair S, 10 iterations) is PARITY_SPREAD
# (profiles/multistart_parity.txt); the multi-start path differs from run_lm at 128 threads through y*y*y against pow
# and the written-out sin / cos against libm, a perturbation of another source and the same amplification: 10 x.
PARITY_SPREAD = 5.065e-16  # measured on an MI355X: max over PARITY_SEEDS, seed 104
PARITY_TOL = 10 * PARITY_SPREAD
PARITY_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)  # _starts(seed=100 + s): run_lm takes the same decisions at 128 and 256 threads for each


@pytest.fixture(scope="module")
def hostlib():
    return importlib.import_module("nid-pose-estimation_amd.hostlib")


def _starts(synth, pair, n, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([synth.perturb_pose7(pair.pose_init, rng.normal(0, 1e-3, 3), rng.normal(0, 2e-3, 3)) for _ in range(n)])


def _out_of_frame_start(synth, pair, ctx):
    """test_parity_gpu's "far" pose taken further until every cell is out of frame.  n_active of normal_equations does not
    fall with the pose -- it counts the cells the REFERENCE stage left active (16 of 16 on this pair at any pose); a cell
    without a sample in frame has no joint entropy and the pose's chi2 is not finite -- so "no cell contributes" shows
    as a non-finite chi2, and that is what keeps such a chain from ever being `best`."""
    for k in (2, 4, 8, 16):
        p = synth.perturb_pose7(pair.pose_init, [0.0, 0.03, 0.0], [0.25 * k, -0.15 * k, 0.0])
        if not np.isfinite(ctx.normal_equations(p, DELTA)[2]):
            return p
    raise AssertionError("no start without a cell in frame found")


def _exhausting_start(pair):
    """a start whose first outer iteration rejects ten trials in a row: the pose a 30-iteration chain on pair S converged
    to (found by restarting converged chains: about one in five of them ends like this), at the bottom of its basin,
    where no damped step gains anything.  The test asserts the status."""
    return np.array([0.02646331065551744, 0.051377935024499014, -0.0023497854829923554, 0.9983258383363379,
                     -0.10847660958551704, 0.022101975958659967, -0.25447934635468106])


def _mixed(synth, pair, ctx):
    good = _starts(synth, pair, 1, seed=5)[0]
    return np.stack([good, pair.pose_init, _out_of_frame_start(synth, pair, ctx), _exhausting_start(pair)])


def _block(H, b, chi2, na):
    r = np.zeros(32)
    r[0] = chi2
    r[1:7] = b
    r[7:28] = H[np.triu_indices(6)]
    r[28] = na
    return r


def _host_stepped(capi, ctx, starts, iterations, max_rounds=0):
    """the round loop on the host from public calls; (results, best, rounds, trace) as Context.multistart_lm gives them"""
    n = len(starts)
    cap = max_rounds if max_rounds > 0 else 1 + 10 * iterations
    states = [capi.new_ms_state(p, iterations) for p in starts]
    poses = np.array(starts, dtype=np.float64).copy()
    trace = np.zeros((cap, n), dtype=capi.MS_TRACE_DTYPE)
    rounds = cap
    for r in range(cap):
        ctx.launch_batch(0, poses, DELTA, want_jac=True)
        running = 0
        for k in range(n):
            blk = _block(*ctx.wait(k))
            st = states[k]
            if capi.lm_step_host(st, blk):
                running += 1
                poses[k] = np.array(st.rec_q)
            t = trace[r, k]
            t["trial_chi2"], t["lambda_"], t["rho"], t["pose7"] = st.trial_chi2, st.lambda_, st.rho, np.array(st.pose7)
            t["flags"], t["status"] = st.flags, st.status
        if running == 0:
            rounds = r + 1
            break
    res = np.zeros(n, dtype=capi.MS_RESULT_DTYPE)
    best, best_v = -1, 0.0
    for k, st in enumerate(states):
        res[k]["pose7"] = np.array(st.pose7)
        res[k]["chi2"], res[k]["lambda_"], res[k]["n_active"] = st.chi2, st.lambda_, st.n_active
        res[k]["outer_iterations"], res[k]["trials"], res[k]["status"] = st.outer_done, st.trials_total, st.status
        if st.n_active > 0 and np.isfinite(st.chi2) and (best < 0 or st.chi2 / st.n_active < best_v):
            best, best_v = k, st.chi2 / st.n_active
    return res, best, rounds, trace[:rounds]


def _assert_same(dev, ref, what):
    res_d, best_d, rounds_d, tr_d = dev
    res_r, best_r, rounds_r, tr_r = ref
    assert rounds_d == rounds_r, f"{what}: rounds {rounds_d} (device) / {rounds_r} (host-stepped)"
    for name in tr_d.dtype.names:
        same = tr_d[name].tobytes() == tr_r[name].tobytes()
        if not same:
            bad = np.argwhere(tr_d[name].view(np.uint8).reshape(tr_d.shape + (-1,)) != tr_r[name].view(np.uint8).reshape(tr_r.shape + (-1,)))[0]
            raise AssertionError(f"{what}: trace field {name} differs first at round {bad[0]}, chain {bad[1]}: "
                                 f"{tr_d[name][bad[0], bad[1]]!r} (device) / {tr_r[name][bad[0], bad[1]]!r} (host-stepped)")
    assert res_d.tobytes() == res_r.tobytes(), f"{what}: results differ\n{res_d}\n{res_r}"
    assert best_d == best_r


@pytest.fixture(scope="module")
def ctx_S(capi, pair_S):
    ctx = capi.from_pair(pair_S, NB)
    ctx.compute_href(pair_S.pose_init)
    return ctx


@pytest.mark.parametrize("m", [1, 2, 16, 17, 64, 256])
def test_device_equals_host_stepped(capi, synth, pair_S, ctx_S, m):
    """every round, every chain: trial chi2, lambda, rho, decision flags, pose7 -- and the results -- are the bits of the
    host-stepped loop, for chain counts on both sides of the kernel-argument limit (16) and up to the largest grid"""
    mixed = _mixed(synth, pair_S, ctx_S)
    starts = np.concatenate([_starts(synth, pair_S, m), mixed])[:m] if m < 8 else np.concatenate([mixed, _starts(synth, pair_S, m - 4)])
    dev = ctx_S.multistart_lm(starts, ITER, DELTA, trace=True)
    ref = _host_stepped(capi, ctx_S, starts, ITER)
    _assert_same(dev, ref, f"M = {m}")
    assert all(s != capi.MS_RUNNING for s in dev[0]["status"])
    assert dev[2] >= 3 and (dev[0]["outer_iterations"] >= 1).all()


def test_chains_do_not_interact_and_freeze(capi, synth, pair_S, ctx_S, monkeypatch):
    starts = _mixed(synth, pair_S, ctx_S)
    res, best, rounds, tr = ctx_S.multistart_lm(starts, ITER, DELTA, trace=True)
    st = res["status"]
    # the out-of-frame chain: chi2 is not finite, rho is NaN, every outer iteration ends with its first (rejected) trial
    assert not np.isfinite(res["chi2"][2]) and st[2] == capi.MS_ITERATIONS and res["trials"][2] == ITER
    assert res["pose7"][2].tobytes() == starts[2].tobytes(), "a chain that never accepts keeps its start pose"
    assert st[3] == capi.MS_TRIALS_EXHAUSTED and res["trials"][3] == 10, f"the exhausting start ended with status {st[3]} after {res['trials'][3]} trials"
    assert st[0] != capi.MS_RUNNING and st[1] != capi.MS_RUNNING
    assert rounds > 2 + 1, "the chains end at different rounds: some are frozen while others run"
    # alone
    for k in range(len(starts)):
        one, b1, r1 = ctx_S.multistart_lm(starts[k:k + 1], ITER, DELTA)
        assert one.tobytes() == res[k:k + 1].tobytes(), f"chain {k} alone differs from the same start in the mixed batch"
        assert r1 <= rounds
    # rounds enqueued past the last chain's end, and other chunkings of them
    again = ctx_S.multistart_lm(starts, ITER, DELTA, max_rounds=rounds + 7, trace=True)
    assert again[0].tobytes() == res.tobytes() and again[2] == rounds and again[3].tobytes() == tr.tobytes()
    for chunk in ("1", "3", "64"):
        monkeypatch.setenv("NID_MS_CHUNK", chunk)
        other = ctx_S.multistart_lm(starts, ITER, DELTA, trace=True)
        assert other[0].tobytes() == res.tobytes() and other[2] == rounds and other[3].tobytes() == tr.tobytes(), f"chunk {chunk}"
    monkeypatch.delenv("NID_MS_CHUNK")
    # buffers and tickets are left clean
    second = ctx_S.multistart_lm(starts, ITER, DELTA, trace=True)
    assert second[0].tobytes() == res.tobytes() and second[1] == best and second[3].tobytes() == tr.tobytes()
    # too few rounds: not finished
    short, _, r_short = ctx_S.multistart_lm(starts, ITER, DELTA, max_rounds=2)
    assert r_short == 2 and (short["status"] == capi.MS_RUNNING).all() and (short["trials"] == 1).all()


def test_repairs_are_in_before_the_step_reads(capi, synth):
    pair = synth.make_pair("A", flash=True)
    ctx = capi.from_pair(pair, NB)
    ctx.compute_href(pair.pose_init)
    starts = _starts(synth, pair, 17)
    ctx.repair_count(reset=True)
    dev = ctx.multistart_lm(starts, 3, DELTA, trace=True)
    assert ctx.repair_count() > 0, "the flash pair must send cells through k_repair"
    ref = _host_stepped(capi, ctx, starts, 3)
    _assert_same(dev, ref, "flash pair, M = 17")


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


def test_against_the_shipped_lm(capi, synth, hostlib, pair_S):
    """chain k against hostlib.run_lm(fused=1) from the same start with 128-thread cost + Jacobian launches: the same
    lm_trials per outer iteration, the final pose within PARITY_TOL"""
    starts = np.stack([_starts(synth, pair_S, 1, seed=100 + s)[0] for s in PARITY_SEEDS])
    worst = 0.0
    try:
        for k, p0 in enumerate(starts):
            runs = {}
            for nt in (128, 256):
                hostlib.set_launch_shape(nt, 0)
                runs[nt] = hostlib.run_lm(pair_S, NB, p0, iterations=10, fused=1)
            # a start on a decision edge of the shipped LM itself is replaced, not tolerated
            assert [r["lm_trials"] for r in runs[128][1]] == [r["lm_trials"] for r in runs[256][1]], f"seed {PARITY_SEEDS[k]}: run_lm decides differently at 128 and 256 threads: choose another start"
            hostlib.set_launch_shape(128, 0)
            res, best, rounds, tr = hostlib.run_multistart_lm(pair_S, NB, starts, iterations=10, pose_ref=p0, trace=True)
            assert _trials_per_outer(tr[:, k]) == [r["lm_trials"] for r in runs[128][1]], f"seed {PARITY_SEEDS[k]}"
            d = float(np.abs(res["pose7"][k] - runs[128][0]).max())
            spread = float(np.abs(runs[128][0] - runs[256][0]).max())
            print(f"seed {PARITY_SEEDS[k]}: |multistart - run_lm(128)| = {d:.3e}, run_lm 128 / 256 spread {spread:.3e}, {len(runs[128][1])} iterations, status {res['status'][k]}")
            worst = max(worst, d)
    finally:
        hostlib.set_launch_shape(-1, 0)
    assert worst <= PARITY_TOL, f"final poses differ by {worst:.3e} > {PARITY_TOL:.3e}"


def test_best_and_side_effects(capi, synth, pair_S):
    ctx = capi.from_pair(pair_S, NB)
    ctx.compute_href(pair_S.pose_init)
    starts = _mixed(synth, pair_S, ctx)
    probe = _starts(synth, pair_S, 20, seed=3)
    before = [ctx.normal_equations(p, DELTA) for p in probe[:3]]
    seq_before = ctx.run_sequence(probe, DELTA, batch=8)
    res, best, rounds = ctx.multistart_lm(starts, ITER, DELTA)
    score = [r["chi2"] / r["n_active"] if r["n_active"] > 0 and np.isfinite(r["chi2"]) else np.inf for r in res]
    assert best == int(np.argmin(score)) and best != 2 and np.isfinite(score[best])
    only_inactive = ctx.multistart_lm(starts[2:3], ITER, DELTA)
    assert only_inactive[1] == -1
    ctx.launch_batch(0, probe[:3], DELTA)
    after = [ctx.wait(k) for k in range(3)]
    for a, b in zip(before, after):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3]
    assert ctx.run_sequence(probe, DELTA, batch=8).tobytes() == seq_before.tobytes()
    for bad in (np.zeros((0, 7)), np.tile(pair_S.pose_init, (257, 1))):
        with pytest.raises(capi.NidError):
            ctx.multistart_lm(bad, ITER, DELTA)
    ctx.launch(5, pair_S.pose_init, DELTA)
    with pytest.raises(capi.NidError):
        ctx.multistart_lm(starts, ITER, DELTA)
    ctx.wait(5)
    again = ctx.multistart_lm(starts, ITER, DELTA)
    assert again[0].tobytes() == res.tobytes() and again[1] == best


def test_strict_math(capi, synth, pair_S):
    ctx = capi.from_pair(pair_S, NB, math=capi.MATH_STRICT)
    ctx.compute_href(pair_S.pose_init)
    starts = np.concatenate([_mixed(synth, pair_S, ctx), _starts(synth, pair_S, 13)])
    dev = ctx.multistart_lm(starts, ITER, DELTA, trace=True)
    ref = _host_stepped(capi, ctx, starts, ITER)
    _assert_same(dev, ref, "STRICT, M = 17")
