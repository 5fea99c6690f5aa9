"""One corpus of (chain state, reduced block) pairs for lm::lm_step (csrc/nid_lm_step.h), shared by tests/test_lm_step_cpu.py
and tests/test_lm_step_gpu.py.  A plain module: import it, call corpus(capi).

Synthetic chains are stepped with capi.lm_step_host and (state before, block) is recorded at every step.  If the device
build equals the host build on every recorded pair it equals it on every one of these chains, by induction -- so ONE launch
of k_lm_step over the recorded pairs covers whole chains in every phase: first blocks, accepted and rejected trials, failed
solves, the end of each kind and what a finished chain does with further blocks.

Every input is one lm_step is specified for.  In particular r[28] (n_active) is always an integral count in 0..65536:
(int32_t)r[28] of a NaN or an out-of-range double is undefined in C++, and the reduction kernels never produce one -- the
NaN / infinite blocks below keep r[28] a count.  Start poses are unit quaternions with w >= 0, as nid_ms_state asks.

A pair's CATEGORY says what it was built for.  NAN_CATEGORIES are the ones built to make NaNs (a rotation of more than
1e6 rad, or 1e200; a non-finite H; a non-finite chi2): IEEE fixes neither the sign nor the payload of a NaN that
arithmetic produced (generated: 0/0, inf - inf; or passed through an operation: a NaN chi2 through the subtraction in rho), so
only there may a device double differ from the host's in its bits while both are NaN."""
import ctypes as C
import math
from decimal import Decimal, getcontext

import numpy as np

F_FIRST, F_ACCEPT, F_REJECT, F_OUTER_END, F_SOLVE_FAILED, F_FINISHED = 1, 2, 4, 8, 16, 32
NAN_CATEGORIES = ("theta > 1e6", "theta = 1e200", "H non-finite", "chi2 non-finite")
DBL_MAX, DBL_MIN = np.finfo(np.float64).max, np.finfo(np.float64).tiny

# nid_ms_state as a numpy record (capi.MsState field for field)
STATE_DTYPE = np.dtype([("pose7", "f8", 7), ("chi2", "f8"), ("H", "f8", 21), ("b", "f8", 6), ("lambda_", "f8"), ("ni", "f8"),
                        ("ini_chi2", "f8"), ("x", "f8", 6), ("trial7", "f8", 7), ("trial_chi2", "f8"), ("rho", "f8"),
                        ("rec_q", "f8", 7), ("rec_M", "f8", 12),
                        ("iterations", "i4"), ("xform_mode", "i4"), ("started", "i4"), ("n_active", "i4"), ("n_bad", "i4"),
                        ("trials", "i4"), ("outer_done", "i4"), ("trials_total", "i4"), ("solve_ok", "i4"), ("status", "i4"),
                        ("flags", "i4"), ("rec_mode", "i4")])
assert STATE_DTYPE.itemsize == 624

getcontext().prec = 60
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])
POSE0 = np.array([0.01, -0.02, 0.03, 0.0, 0.4, -0.2, 1.5])
POSE0[3] = np.sqrt(1.0 - (POSE0[:3] ** 2).sum())
# quaternions with w within 1e-16 of zero (unit to rounding): exp(x) * pose comes out with w < 0 for half of all x
POSES_W0 = [np.array([1.0, 0, 0, 0.0, 0.1, 0.2, 0.3]), np.array([0.6, 0.8, 0, 1e-17, -1.0, 2.0, 0.5]),
            np.array([0, 0.6, -0.8, 5e-17, 0, 0, 0]), np.array([0.48, -0.6, 0.64, 1e-16, 3.0, -4.0, 5.0])]
POSE_FAR = np.array([POSE0[0], POSE0[1], POSE0[2], POSE0[3], 1e6, -1e6, 1e6])
A_UNIT = 1.0 + 1e-5  # H = I: lambda = 1e-5, the damped diagonal


def block(H, b, chi2, na=16):
    r = np.zeros(32)
    r[0] = chi2
    r[1:7] = b
    r[7:28] = np.asarray(H)[np.triu_indices(6)]
    r[28] = na
    return r


def filled_block(v, na=16):
    r = np.full(32, v)
    r[28] = na  # (a count, whatever else the block holds)
    return r


def spd(rng, scale=1.0, cond=1e3):
    """symmetric positive definite, eigenvalues from scale to scale * cond (downwards from scale where that would overflow)"""
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    ev = np.geomspace(1.0, cond, 6) if scale * cond < 1e301 else np.geomspace(1.0 / cond, 1.0, 6)
    H = (Q * ev) @ Q.T
    return (H + H.T) * (0.5 * scale)


def full(H21):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = H21
    return H + np.triu(H, 1).T


def ldlt_pivots(H21, lam):
    """ldlt6_solve's pivoting restated on Python floats (IEEE doubles, no contraction): per k the index exchanged with
    (p != k: an exchange) and the pivot.  -> (exchanges [6], pivots [6], positive)"""
    A = [[float(v) for v in row] for row in full(np.asarray(H21, dtype=np.float64))]
    for i in range(6):
        A[i][i] = A[i][i] + lam
    ex, piv, positive = [], [], True
    for k in range(6):
        p, best = k, abs(A[k][k])
        for i in range(k + 1, 6):
            if abs(A[i][i]) > best:
                best, p = abs(A[i][i]), i
        if p != k:
            A[k], A[p] = A[p], A[k]
            for row in A:
                row[k], row[p] = row[p], row[k]
        dk = A[k][k]
        ex.append(p)
        piv.append(dk)
        if not dk >= 0:
            positive = False
        usable = abs(dk) > DBL_MIN
        for i in range(k + 1, 6):
            A[i][k] = A[i][k] / dk if usable else 0.0
        for i in range(k + 1, 6):
            for j in range(k + 1, 6):
                A[i][j] = A[i][j] - (A[i][k] * dk) * A[j][k]
    return ex, piv, positive


def theta_of(x):
    """se3_exp's theta, operation for operation"""
    with np.errstate(all="ignore"):
        o = np.asarray(x, dtype=np.float64)
        return float(np.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]))


def quadrant_of(theta):
    """sincos_pos's quadrant, operation for operation (theta <= 1e6)"""
    kd = (theta * float.fromhex("0x1.45F306DC9C883p-1") + float.fromhex("0x1.8p52")) - float.fromhex("0x1.8p52")
    return int(kd) & 3


def around(t, ulps):
    """the doubles b for which b / A_UNIT takes every value within about `ulps` of t (x = b / (1 + 1e-5) in the same binade
    steps no wider than b does), t itself among them"""
    b0 = t * A_UNIT
    out = [b0]
    lo = hi = b0
    for _ in range(ulps + 1):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [float(lo), float(hi)]
    return out


def rotation_rhs():
    """right-hand sides b (rotation part, along +x) whose solve with H = I gives the angles of the corpus; (class, b)"""
    out = [("zero", 0.0), ("small", 9.99e-6 * A_UNIT), ("small", 1.01e-5 * A_UNIT)]
    out += [("threshold", b) for b in around(1e-5, 3)]
    for k in range(1, 9):
        out += [("k pi/2", b) for b in around(float(Decimal(k) * PI / 2), 3)]
    out += [("trace sign", float(t) * A_UNIT) for t in np.linspace(2.0, 2.2, 11)] + [("trace sign", float(2 * PI / 3) * A_UNIT)]
    out += [("half turn", float(t) * A_UNIT) for t in np.linspace(3.0, 3.3, 16)]
    out += [("large", 40.0 * A_UNIT), ("large", 1e3 * A_UNIT)] + [("1e6", b) for b in around(1e6, 3)]
    out += [("1e200", 1e200)]
    return out


AXES = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), np.array([0, 0, -1.0]),
        np.array([0.48, -0.6, 0.64]), np.array([-0.36, 0.48, 0.8])]


class Corpus:
    def __init__(self, capi):
        self.capi = capi
        self._before, self._blocks, self.cats = [], [], []

    def fresh(self, pose=POSE0, iterations=10, mode=0):
        return self.capi.new_ms_state(pose, iterations, mode)

    def step(self, cat, st, blk):
        """record (st, blk), then step st on the host"""
        self._before.append(bytes(memoryview(st)))
        self._blocks.append(np.array(blk, dtype=np.float64))
        self.cats.append(cat)
        return self.capi.lm_step_host(st, blk)

    # ---- what the tests read ------------------------------------------------------------------------------------
    def finish(self):
        self.n = len(self.cats)
        self.blocks = np.array(self._blocks)
        self.blocks.setflags(write=False)
        self._raw = b"".join(self._before)
        after = self.states()
        self.running = np.zeros(self.n, dtype=bool)
        for k in range(self.n):
            self.running[k] = self.capi.lm_step_host(after[k], self.blocks[k])
        self.before = np.frombuffer(self._raw, dtype=STATE_DTYPE)
        self.after = np.frombuffer(bytes(memoryview(after)), dtype=STATE_DTYPE)  # the host twin's answer, read-only
        self.nan_ok = np.array([c in NAN_CATEGORIES for c in self.cats])
        return self

    def states(self, n=None):
        """a fresh ctypes array of the first n states as they were BEFORE their step"""
        n = self.n if n is None else n
        arr = (self.capi.MsState * n)()
        C.memmove(arr, self._raw, n * C.sizeof(self.capi.MsState))
        return arr


def sentinel_records(n):
    """pose records no step writes: what a finished chain's record must still hold"""
    rec19 = -(1000.0 + np.arange(n))[:, None] - np.arange(19)[None, :] / 32.0
    return np.ascontiguousarray(rec19), (0x1234000 + np.arange(n)).astype(np.int32)


def expected_records(cp, n):
    """the records behind a launch over the first n pairs that started from sentinel_records(n)"""
    rec19, mode = sentinel_records(n)
    run = cp.running[:n]
    rec19[run, :7] = cp.after["rec_q"][:n][run]
    rec19[run, 7:] = cp.after["rec_M"][:n][run]
    mode[run] = cp.after["rec_mode"][:n][run]
    return rec19, mode


def _first_blocks(c, rng):
    # SPD, condition 1 .. 1e12, scale 1e-300 .. 1e300; two accepted trials behind each (lambda shrinks: less damping)
    for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
        for scale in (1e-300, 1e-200, 1e-100, 1e-10, 1.0, 1e10, 1e100, 1e200, 1e300):
            for rep in range(2):
                H = spd(rng, scale, cond)
                xs = rng.standard_normal(6) * 1e-2
                st = c.fresh(mode=rep)
                c.step("spd", st, block(H, H @ xs, 10.0))
                for chi2 in (9.0, 8.5):
                    if st.status == 0:
                        H = spd(rng, scale, cond)
                        c.step("spd", st, block(H, H @ (rng.standard_normal(6) * 1e-2), chi2, na=9))
    off = rng.standard_normal((6, 6)) * 0.05
    off = off + off.T
    np.fill_diagonal(off, 0.0)
    bb = rng.standard_normal(6) * 1e-2
    # equal diagonals: the tie goes to the lower index (with and without off-diagonals; a rank-one matrix of ones)
    for H in (2.0 * np.eye(6), 2.0 * np.eye(6) + off, np.ones((6, 6)), 3.0 * np.eye(6) + 10 * off):
        c.step("ties", c.fresh(), block(H, bb, 10.0))
    # diagonals ordered so that every k exchanges: (1, 6, 5, 4, 3, 2); and the other orders of interest
    for d in ([1, 6, 5, 4, 3, 2], [6, 5, 4, 3, 2, 1], [1, 2, 3, 4, 5, 6], [2, 1, 4, 3, 6, 5], [3, 6, 1, 5, 2, 4]):
        for s in (1.0, 1e-3):
            c.step("exchanges", c.fresh(), block(np.diag(np.array(d, dtype=float)) * s + off * s, bb * s, 10.0))
    # rank 0 .. 5: zero rows and columns; all-zero H: lambda = 0, every pivot zero
    for rank in range(6):
        for rep in range(3):
            H = spd(rng, 1.0, 10.0)
            dead = rng.permutation(6)[: 6 - rank]
            H[dead, :] = 0.0
            H[:, dead] = 0.0
            b = H @ (rng.standard_normal(6) * 1e-2)
            if rep == 2:
                b = b + 1e-3  # (a right-hand side outside the range too)
            st = c.fresh()
            c.step("rank", st, block(H, b, 10.0 if rank else 0.0, na=rank))
            c.step("rank", st, block(H, b, 9.0 if rank else 0.0, na=rank))  # rank 0: x = 0, rho == 0
    # denormal diagonals: pivots at or below DBL_MIN count as zero
    for d in ([1e-310] * 6, [1e-305, 1e-310, 1e-305, 1e-310, 1e-305, 1e-310], [DBL_MIN * 1e5, DBL_MIN, 0, 5e-324, 1e-310, 1e-320]):
        st = c.fresh()
        c.step("denormal", st, block(np.diag(d), np.array([1e-310, 1e-306, 0, 1e-320, 1e-307, 5e-324]), 10.0))
        c.step("denormal", st, block(np.diag(d), np.zeros(6), 9.0))
    # a negative pivot first met at k = 0 .. 5 (pivots come by |diagonal|): the solve fails until lambda has grown past it;
    # the blocks behind a failed solve carry a BETTER chi2, which must not be accepted
    for k in range(6):
        for o in (0.0, 1.0):
            d = np.array([6.0, 5, 4, 3, 2, 1])
            d[k] = -d[k]
            H = np.diag(d) + o * off
            st = c.fresh()
            c.step("negative pivot", st, block(H, bb, 10.0))
            for _ in range(12):
                if st.status != 0:
                    break
                c.step("negative pivot", st, block(H, bb, 1.0 if not st.solve_ok else 9.0))
    # a later solve that fails: an accepted trial brings an indefinite H
    st = c.fresh()
    c.step("later solve", st, block(spd(rng), bb, 10.0))
    Hbad = np.diag([4.0, 3, 2, 1, 1, -0.5])
    c.step("later solve", st, block(Hbad, bb, 9.0))
    for _ in range(4):
        c.step("later solve", st, block(Hbad, bb, 1.0))
    # an infinite and a NaN entry, in H and in b
    for what in range(6):
        H, b = spd(rng), bb.copy()
        if what == 0: H[0, 0] = np.inf
        if what == 1: H[2, 3] = H[3, 2] = np.inf
        if what == 2: H[4, 4] = np.nan
        if what == 3: H[1, 5] = H[5, 1] = np.nan
        if what == 4: b[2] = np.inf
        if what == 5: b[3] = np.nan
        st = c.fresh()
        c.step("H non-finite", st, block(H, b, 10.0))
        for chi2 in (9.0, 11.0):
            if st.status == 0:
                c.step("H non-finite", st, block(spd(rng), bb, chi2))


def _rotations(c, rng):
    poses = [IDENTITY, POSE0] + POSES_W0 + [POSE_FAR]
    trans = np.array([0.3, -0.7, 0.2]) * A_UNIT
    k = 0
    for cls, b in rotation_rhs():
        for axis in AXES:
            for pose in (IDENTITY, poses[k % len(poses)]):
                st = c.fresh(pose, mode=k & 1)
                k += 1
                u = np.concatenate([axis * b, trans])
                if cls == "1e200":
                    cat = "theta = 1e200"
                else:  # (by the theta the solve will produce: x = b / (1 + 1e-5) component by component)
                    cat = "theta > 1e6" if not theta_of(u / A_UNIT) <= 1e6 else "rotation: " + cls
                c.step(cat, st, block(np.eye(6), u, 10.0))
                if k % 5 == 0:  # the trial is accepted: a pose far round becomes the current one
                    c.step(cat, st, block(spd(rng), rng.standard_normal(6) * 1e-2, 9.0))


def _one_in(c, cat, iterations=10, seed=7, mode=0, pose=POSE0):
    """a chain one step in on a fixed system; chi2_for(rho) is the trial chi2 that gives that gain ratio (to rounding)"""
    rng = np.random.default_rng(seed)
    H, b = spd(rng), rng.standard_normal(6) * 1e-2
    st = c.fresh(pose, iterations, mode)
    c.step(cat, st, block(H, b, 10.0))
    x = np.array(st.x)
    scale = float(x @ (st.lambda_ * x + b)) + 1e-3
    return st, H, b, (lambda rho: 10.0 - rho * scale)


def _later_blocks(c, rng):
    # ten rejections in a row: the ninth goes on, the tenth ends the chain (status 2)
    st, H, b, _ = _one_in(c, "rejections")
    for k in range(10):
        c.step("rejections", st, block(H, b, 11.0 + k))
    done = [st]
    # three flat iterations (status 4); a gain in between resets the count
    st, H, b, _ = _one_in(c, "flat")
    for k in range(3):
        c.step("flat", st, block(H, b, 10.0 - 1e-6 * (k + 1)))
    done.append(st)
    st, H, b, _ = _one_in(c, "flat")
    for chi2 in (10.0 - 1e-6, 9.0, 9.0 - 1e-6, 9.0 - 2e-6):
        c.step("flat", st, block(H, b, chi2))
    # the last of `iterations` (status 1)
    for its in (1, 2):
        st, H, b, _ = _one_in(c, "iterations", iterations=its)
        for k in range(its):
            c.step("iterations", st, block(H, b, 9.0 - k))
        done.append(st)
    st, H, b, _ = _one_in(c, "rho zero")
    c.step("rho zero", st, block(H, b, 10.0))
    done.append(st)
    # finished chains of every status, handed ordinary, NaN and infinite blocks: frozen
    assert sorted({s.status for s in done}) == [1, 2, 3, 4]
    for st in done:
        for blk in (block(H, b, 1.0), filled_block(np.nan), filled_block(np.inf), filled_block(-np.inf)):
            c.step("frozen", st, blk)
    for rho in (0.05, 0.5, 0.84, 0.85, 0.9, 0.93, 0.94, 3.0):  # both lambda clamps from both sides
        for mode in (0, 1):
            st, H, b, chi2_for = _one_in(c, "rho", mode=mode)
            c.step("rho", st, block(2 * H, -b, chi2_for(rho), na=9))
    st, H, b, chi2_for = _one_in(c, "rho zero")
    c.step("rho zero", st, block(H, b, 10.0))  # rho == 0 exactly: status 3
    for v in (np.nan, np.inf, -np.inf):
        st, H, b, _ = _one_in(c, "chi2 non-finite")
        c.step("chi2 non-finite", st, block(H, b, v))
        c.step("chi2 non-finite", st, block(H, b, 9.0))
        c.step("chi2 non-finite", st, block(H, b, v))
    st, H, b, _ = _one_in(c, "chi2 DBL_MAX")
    c.step("chi2 DBL_MAX", st, block(H, b, DBL_MAX))
    c.step("chi2 DBL_MAX", st, block(H, b, 9.0))


def _ordinary(c, rng):
    """chains on a quadratic cost, as tests/test_multistart_cpu.py runs them, from near and far poses in both modes"""
    for k in range(48):
        H = spd(rng, scale=10.0 ** rng.integers(-2, 3), cond=10.0 ** rng.integers(1, 5))
        xs = rng.standard_normal(6) * 10.0 ** rng.uniform(-4, -1)
        cost = lambda d: 5.0 + 0.5 * (d - xs) @ H @ (d - xs)
        st = c.fresh([POSE0, POSE_FAR, IDENTITY, POSES_W0[k % 4]][k % 4], iterations=4 + k % 5, mode=k & 1)
        c.step("ordinary", st, block(H, H @ xs, cost(np.zeros(6))))
        for _ in range(14):
            if st.status != 0:
                break
            x = np.array(st.x)
            c.step("ordinary", st, block(H, H @ (xs - x), cost(x)))
            if st.flags & F_ACCEPT:
                xs = xs - x


_CORPUS = None


def corpus(capi):
    """the corpus, built once per process: .n, .blocks [n, 32], .cats [n], .states(n) (fresh ctypes copies of the states
    before), .before / .after (STATE_DTYPE records: the inputs, the host twin's answers), .running [n], .nan_ok [n]"""
    global _CORPUS
    if _CORPUS is None:
        c = Corpus(capi)
        rng = np.random.default_rng(20240521)
        # the head of the corpus mixes running, finishing and frozen chains: the launches over its first 1, 64 and 65
        # pairs see all three
        _later_blocks(c, rng)
        _first_blocks(c, rng)
        _rotations(c, rng)
        _ordinary(c, rng)
        _CORPUS = c.finish()
    return _CORPUS
