"""The host layer's one launch path on ONE context (pair S, 8 bins): a single awaited pose given to nid_launch_batch takes
the route of nid_launch (DIRECT records, GROUP-DIRECT, the resident kernel) and must give its bits; and the three owners of
per-pose buffers -- the public slots, the fused pipeline's pool, nid_multistart_lm's pool -- do not disturb each other when
used in turn.  Bit equality only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = float(np.sqrt(0.95))
NPOSES = 41   # pose k of a sequence is pose k % 41: no period of a batch or a grid
ITER = 6


def _pack(ne):
    H, b, chi2, na = ne
    r = np.zeros(29)
    r[0] = chi2
    r[1:7] = b
    r[7:28] = H[np.triu_indices(6)]
    r[28] = na
    return r


def _same(a, b):
    """bit for bit; a NaN is a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _poses(synth, pair, count, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.perturb_pose7(pair.pose_init, rng.normal(0, 1e-3, 3), rng.normal(0, 2e-3, 3)) for _ in range(count)])


@pytest.fixture(scope="module")
def one(capi, synth, pair_S):
    ctx = capi.from_pair(pair_S, 8)
    ctx.compute_href(pair_S.pose_init)
    yield ctx, _poses(synth, pair_S, NPOSES, 11)
    ctx.close()


def test_one_awaited_pose_in_a_batch_is_the_single_launch(one):
    """launch_batch(slot, [pose]) against launch(slot, pose) and normal_equations(pose): H, b, chi2 and count, cost + Jacobian
    and cost only, in every result mode, through the resident kernel, and timed -- each with a 17-pose launch_batch on other
    slots in flight.  (The Jacobian's last bits depend on the workgroup shape: every comparison is within one shape.)"""
    ctx, poses = one
    others = poses[20:37]

    def case(what, pose, jac, ref, other_ref, batch_first):
        want = ref[jac]
        assert _same(_pack(ctx.normal_equations(pose, DELTA, want_jac=jac)), want), f"{what}: normal_equations"
        ctx.launch(3, pose, DELTA, want_jac=jac)
        assert _same(_pack(ctx.wait(3)), want), f"{what}: launch + wait"
        if batch_first:
            ctx.launch_batch(8, others, DELTA, want_jac=jac)
        ctx.launch_batch(3, [pose], DELTA, want_jac=jac)
        if not batch_first:
            ctx.launch_batch(8, others, DELTA, want_jac=jac)
        got = _pack(ctx.wait(3))
        assert _same(got, want), f"{what}: launch_batch of one pose + wait"
        for k in range(len(others)):
            assert _same(_pack(ctx.wait(8 + k)), other_ref[jac][k]), f"{what}: pose {k} of the 17-pose batch"

    def references(shape):
        """in-launch reduction, nothing resident, untimed: what every mode must reproduce at this shape"""
        ctx.set_launch_shape(shape, 0)
        ctx.set_direct_results(0)
        ref = {p: {jac: _pack(ctx.normal_equations(poses[p], DELTA, want_jac=jac)) for jac in (True, False)} for p in (0, 5)}
        oth = {jac: [_pack(ctx.normal_equations(q, DELTA, want_jac=jac)) for q in others] for jac in (True, False)}
        return ref, oth

    ref, oth = references(0)
    for mode in (0, 1, 2):
        ctx.set_direct_results(mode)
        for jac in (True, False):
            for p, batch_first in ((0, False), (5, True)):
                case(f"direct_results({mode}) jac={jac}", poses[p], jac, ref[p], oth, batch_first)
        # nid_launch_chain with one trial of each kind: two awaited single poses, the cost-only one on the second stream
        ctx.launch_chain(3, [poses[0], poses[5]], 1, DELTA)
        assert _same(_pack(ctx.wait(3)), ref[0][True]) and _same(_pack(ctx.wait(4)), ref[5][False]), f"direct_results({mode}): chain"
    # timed: launches keep the in-launch reduction and record events around the evaluation kernel
    ctx.set_direct_results(1)
    ctx.enable_timing(True)
    for jac in (True, False):
        case(f"timed jac={jac}", poses[0], jac, ref[0], oth, False)
        assert ctx.last_kernel_ms(3)[0] > 0 and ctx.last_kernel_ms(8)[0] > 0
    ctx.enable_timing(False)
    # the resident evaluator at the 512-thread shape: the single pose is a request to it (the 17-pose launch behind it
    # collects the request and retires the kernel; the next request starts another)
    ref512, oth512 = references(512)
    ctx.set_direct_results(1)
    ctx.set_resident(True)
    s0 = ctx.resident_stats()
    for jac in (True, False):
        case(f"resident jac={jac}", poses[0], jac, ref512[0], oth512, False)
    s1 = ctx.resident_stats()
    assert s1["served"] - s0["served"] >= 6 and s1["fallbacks"] == s0["fallbacks"], (s0, s1)   # three requests per case
    ctx.set_resident(False)
    ctx.set_launch_shape(0, 0)


def test_private_pools_and_public_slots_in_turn(capi, pair_S, one):
    """fused sequence (batch 16), multi-start with 17 then 3 chains (the pool is larger than the call), fused sequence
    (batch 64), a 256-pose launch_batch, the first sequence again: every row is its pose's single launch; the multi-start
    results are those of the same calls on a fresh context."""
    ctx, poses = one
    ref = np.stack([_pack(ctx.normal_equations(p, DELTA)) for p in poses])
    idx = np.arange(2 * 64 * 16) % NPOSES

    def sequence(batch):
        out = ctx.run_sequence(poses[idx], DELTA, batch=batch)
        bad = [k for k in range(len(idx)) if not _same(out[k, :29], ref[idx[k]])]
        assert not bad, f"batch {batch}: {len(bad)} rows differ from the single launch, first at {bad[0]}"
        return out

    first = sequence(16)                                     # n = 2 F batch with F = 64: two fused grids of 1024 poses
    ms = [ctx.multistart_lm(poses[:n], ITER, DELTA, trace=True) for n in (17, 3)]
    sequence(64)                                             # n = 2 F batch with F = 16
    seq = poses[np.arange(256) % NPOSES]
    ctx.launch_batch(0, seq, DELTA)
    for k in range(256):
        assert _same(_pack(ctx.wait(k)), ref[k % NPOSES]), k
    assert _same(sequence(16), first)

    fresh = capi.from_pair(pair_S, 8)
    fresh.compute_href(pair_S.pose_init)
    for n, got in zip((17, 3), ms):
        want = fresh.multistart_lm(poses[:n], ITER, DELTA, trace=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1:3] == want[1:3], f"{n} chains: results, best or rounds differ"
        assert got[3].tobytes() == want[3].tobytes(), f"{n} chains: traces differ"
    fresh.close()


def test_growable_buffers_small_large_small(capi, synth, pair_S):
    """Every buffer that grows with the request -- the pipelined loop's result rings and the fused pool, nid_multistart_lm's
    pool, round words and trace, nid_multi_run_sequence's rings -- asked for small, then large, then small again on ONE
    context (one nid_multi of two shards on device 0): every result equals, bit for bit, the same call on a context that
    has made no other call.  Then everything is closed and a new context is used once: a release that took something
    still in use would show there."""
    poses = _poses(synth, pair_S, NPOSES, 23)

    def context():
        c = capi.from_pair(pair_S, 8)
        c.compute_href(pair_S.pose_init)
        return c

    def multi():
        m = capi.multi_from_pair(pair_S, 8, devices=(0, 0))
        m.compute_href(pair_S.pose_init)
        return m

    def fresh(make, call):
        c = make()
        try:
            return call(c)
        finally:
            c.close()

    short, long_ = poses[np.arange(12) % NPOSES], poses[np.arange(2 * 64 * 16) % NPOSES]
    calls = [("run_sequence batch 2", lambda c: c.run_sequence(short, DELTA, batch=2).tobytes()),      # 6 launches, ring of 2
             ("run_sequence batch 16, fused", lambda c: c.run_sequence(long_, DELTA, batch=16).tobytes()),  # two grids of 1024: rings and pool grow
             ("run_sequence batch 2 again", lambda c: c.run_sequence(short, DELTA, batch=2).tobytes())]

    def ms(n, iterations, trace):
        def call(c):
            got = c.multistart_lm(poses[:n], iterations, DELTA, trace=trace)
            return (got[0].tobytes(), got[1], got[2]) + ((got[3].tobytes(),) if trace else ())
        return call
    calls += [("multistart 2 chains", ms(2, 3, False)), ("multistart 6 chains, traced, more rounds", ms(6, 7, True)),
              ("multistart 2 chains again", ms(2, 3, False))]

    ctx = context()
    for what, call in calls:
        assert call(ctx) == fresh(context, call), what
    ctx.close()

    seq = poses[np.arange(40) % NPOSES]
    m = multi()
    for batch, group in ((2, 2), (4, 4), (2, 2)):  # group * batch 4, 16, 4: the shards' device rings and the pinned landing zones
        call = lambda c: c.run_sequence(seq, DELTA, batch=batch, group=group).tobytes()
        assert call(m) == fresh(multi, call), f"multi run_sequence batch {batch} group {group}"
    m.close()

    again = context()
    assert _same(again.run_sequence(short, DELTA, batch=2)[:, :29], np.stack([_pack(again.normal_equations(p, DELTA)) for p in short]))
    again.close()
