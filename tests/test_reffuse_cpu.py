"""include/nid/nid_reffuse.h without a device: the export table, the argument rules (checked before any device is touched),
known answers of nid_reffuse_host, the host function against a numpy restatement of the header's rule on the scene the GPU
tests fuse -- planes and counts compared for equality over sequences of calls, and no decision of part A within 1e-9 of a
threshold --, fill and fusion in either order, what the feature is for on a noisy plane, and the rule alone in a program of
its own under the host sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("reffuse_restate", os.path.join(ROOT, "tests", "reffuse_restate.py"))
ur = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ur)
fr = ur.fr

INVALID_ARG = -1
F5000 = ur.F5000
F12 = 2.0 ** -12
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0.0])
EYE16 = np.eye(4).reshape(16)
GA, GR = ur.GATE_ABS, ur.GATE_REL


def _declared():
    txt = open(os.path.join(ROOT, "include", "nid", "nid_reffuse.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nid_[A-Za-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported(capi):
    lib = capi.load()
    declared = _declared()
    assert len(declared) == 7 and sorted(capi.REFFUSE_SYMBOLS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nid_[A-Za-z0-9_]+)", nm))
    for name in declared:
        assert hasattr(lib, name) and name in exported, f"{name} declared in nid_reffuse.h but not exported"
    for other in (capi.SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PYR_SYMBOLS, capi.STREAM_SYMBOLS, capi.KEYFRAME_SYMBOLS, capi.REFMASK_SYMBOLS,
                  capi.REFFILL_SYMBOLS, capi.MULTI_SYMBOLS):
        assert not set(declared) & set(other)
    assert lib.nid_abi_version() == 4, "nid_reffuse.h is a header of its own: the C-ABI of nid_c.h has not changed"
    assert capi.REFFUSE_MAX_OBS == 255 and capi.REFFUSE_COUNTS_DTYPE.itemsize == 64
    assert capi.REFFUSE_COUNTS_DTYPE.names == ur.COUNT_NAMES
    assert ur.COUNT_NAMES == ("n_target_valid", "n_splat", "n_hit", "n_valid", "n_fused", "n_gated", "n_saturated", "n_changed")


def _cfg(capi, rows=24, cols=32, fx=128.0, fy=-128.0, cx=15.5, cy=11.5):
    return capi.NidConfig(rows, cols, 4, 8, 3, 0, 0, 0, fx, fy, cx, cy)


def test_argument_rules_before_any_device(capi):
    lib = capi.load()
    cfg = _cfg(capi)
    N = 24 * 32
    d0, d1 = np.full(N, 10000, dtype=np.uint16), np.full(N, 10010, dtype=np.uint16)
    S, K, Fu = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint16)
    cnt = np.zeros(1, dtype=capi.REFFUSE_COUNTS_DTYPE)
    dp, u16p, vp = (lambda a: a.ctypes.data_as(capi.c_dp)), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))), \
        (lambda a: a.ctypes.data_as(C.c_void_p))
    u32p, u8p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(capi.c_u8p))
    opt = lambda fn, a: fn(a) if a is not None else None

    def host(c=cfg, D0=d0, T=EYE16, D1=d1, Q=IDENTITY, ga=50, gr=20, mo=255, Sm=None, Kb=None, Fp=Fu, Cn=cnt):
        Sm = S.copy() if Sm is None else Sm  # (an unfused state unless the caller brings one)
        Kb = K.copy() if Kb is None else Kb
        return lib.nid_reffuse_host(C.byref(c) if c is not None else None, opt(u16p, D0), F5000, opt(dp, T), opt(u16p, D1), F5000, opt(dp, Q),
                                    ga, gr, mo, opt(u32p, Sm), opt(u8p, Kb), opt(u16p, Fp), opt(vp, Cn))

    assert host() == 0 and host(Cn=None) == 0 and host(ga=0, gr=0, mo=1) == 0 and host(ga=65535, gr=1024, mo=255) == 0
    for name in ("c", "D0", "T", "D1", "Q", "Fp"):
        assert host(**{name: None}) == INVALID_ARG, name
    assert lib.nid_reffuse_host(C.byref(cfg), u16p(d0), F5000, dp(EYE16), u16p(d1), F5000, dp(IDENTITY), 50, 20, 255, None, u8p(K.copy()), u16p(Fu),
                                vp(cnt)) == INVALID_ARG
    assert lib.nid_reffuse_host(C.byref(cfg), u16p(d0), F5000, dp(EYE16), u16p(d1), F5000, dp(IDENTITY), 50, 20, 255, u32p(S.copy()), None, u16p(Fu),
                                vp(cnt)) == INVALID_ARG
    for bad in (-1, 65536, 1 << 30):
        assert host(ga=bad) == INVALID_ARG, bad
    for bad in (-1, 1025, 1 << 30):
        assert host(gr=bad) == INVALID_ARG, bad
    for bad in (-1, 0, 256, 1 << 30):
        assert host(mo=bad) == INVALID_ARG, bad
    assert host(c=_cfg(capi, rows=0)) == INVALID_ARG and host(c=_cfg(capi, cols=0)) == INVALID_ARG
    assert host(c=_cfg(capi, rows=1 << 16, cols=1 << 15)) == INVALID_ARG  # rows x cols above INT32_MAX: refused before a byte is read
    # planes no sequence of calls leaves: a sum above 65535 a fused observation
    bad_sum = S.copy()
    bad_sum[5] = 1
    assert host(Sm=bad_sum) == INVALID_ARG
    one = K.copy()
    one[5] = 1
    bad_sum[5] = 65536
    assert host(Sm=bad_sum, Kb=one) == INVALID_ARG
    bad_sum[5] = 65535
    assert host(Sm=bad_sum, Kb=one) == 0
    # the pyramid's and the tracker's entry points: a null handle or pointer and the ranges are refused first
    assert lib.nid_pyr_fuse_reference_depth(None, dp(IDENTITY), 50, 20, 255, vp(cnt)) == INVALID_ARG
    assert lib.nid_pyr_clear_reference_fusion(None) == INVALID_ARG
    assert lib.nid_pyr_get_reference_fused_u16(None, u16p(Fu)) == INVALID_ARG
    assert lib.nid_pyr_get_reference_fusion_obs_u8(None, u8p(K)) == INVALID_ARG
    assert lib.nid_track_set_fusing(None, 1, 50, 20, 255) == INVALID_ARG
    assert lib.nid_track_last_fusion(None, vp(cnt)) == INVALID_ARG


# ---- known answers ------------------------------------------------------------------------------------------------------
def _one(capi, cfg, d0, d1, gate_abs=64, gate_rel=0, max_obs=255, sums=None, obs=None):
    args = (cfg, d0, F12, EYE16, d1, F12, IDENTITY, gate_abs, gate_rel, max_obs, sums, obs)
    S, K, Fu, cnt = capi.reffuse_host(*args)
    wS, wK, wF, wcnt, _ = ur.restate(*args)
    assert np.array_equal(S, wS) and np.array_equal(K, wK) and np.array_equal(Fu, wF) and ur.counts_dict(cnt) == wcnt
    return S, K, Fu, ur.counts_dict(cnt)


def test_known_answers(capi):
    """identity pose and matrix, depth factor 2^-12: a target pixel lands on the keyframe pixel of its own index and every
    quantity is exact.  The keyframe is a plane at 2 m (8192 counts)."""
    capi.load()
    rows, cols = 24, 32
    N = rows * cols
    cfg = _cfg(capi)
    flat = np.full((rows, cols), 8192, dtype=np.uint16)
    # a plane fused with itself: every pixel takes an observation and none changes
    S, K, Fu, cnt = _one(capi, cfg, flat, flat)
    assert (S == 8192).all() and (K == 1).all() and (Fu == 8192).all()
    assert cnt == dict(n_target_valid=N, n_splat=N, n_hit=N, n_valid=N, n_fused=N, n_gated=0, n_saturated=0, n_changed=0)

    # one pixel: u = 8192, q = 8200 -> 8196 (k = 1); then q = 8201 -> 8198 (the mean is 8197.67); a mean that ends in .5 goes up
    alone = np.zeros_like(flat)
    alone[10, 12] = 8200
    S, K, Fu, cnt = _one(capi, cfg, flat, alone)
    assert (S[10, 12], K[10, 12], Fu[10, 12]) == (8200, 1, 8196) and int((Fu != 0).sum()) == 1 and int(K.sum()) == 1
    assert cnt == dict(n_target_valid=1, n_splat=1, n_hit=1, n_valid=N, n_fused=1, n_gated=0, n_saturated=0, n_changed=1)
    alone[10, 12] = 8201
    S, K, Fu, cnt = _one(capi, cfg, flat, alone, sums=S, obs=K)
    assert (S[10, 12], K[10, 12], Fu[10, 12]) == (16401, 2, 8198) and (cnt["n_fused"], cnt["n_changed"]) == (1, 1)
    for q, want in ((8193, 8193), (8191, 8192), (8195, 8194), (8189, 8191)):  # 8192.5, 8191.5, 8193.5, 8190.5
        alone[10, 12] = q
        assert _one(capi, cfg, flat, alone)[2][10, 12] == want, q

    # the gate (abs 8 counts, rel 16 / 1024 of the uploaded 8192 counts = 128: 136 counts), on both sides: a hit exactly on
    # the bound is fused, one count beyond is gated
    for q, inside in ((8192 + 136, True), (8192 + 137, False), (8192 - 136, True), (8192 - 137, False)):
        alone[10, 12] = q
        S, K, Fu, cnt = _one(capi, cfg, flat, alone, gate_abs=8, gate_rel=16)
        assert (int(K[10, 12]), cnt["n_fused"], cnt["n_gated"], cnt["n_changed"]) == ((1, 1, 0, 1) if inside else (0, 0, 1, 0)), q
        assert Fu[10, 12] == ((8192 + q + 1) // 2 if inside else 0)
    alone[10, 12] = 8193
    assert _one(capi, cfg, flat, alone, gate_abs=0, gate_rel=0)[3]["n_gated"] == 1
    alone[10, 12] = 8192
    assert _one(capi, cfg, flat, alone, gate_abs=0, gate_rel=0)[3]["n_fused"] == 1

    # a hole is never fused, whatever the target shows, and its S and k stay
    d0 = flat.copy()
    d0[10, 12] = 0
    d0[3, 3] = 40  # 0.00977 m: invalid
    S, K, Fu, cnt = _one(capi, cfg, d0, flat, gate_abs=65535)
    assert (Fu[10, 12], K[10, 12], S[10, 12], Fu[3, 3], K[3, 3]) == (0, 0, 0, 0, 0)
    assert cnt == dict(n_target_valid=N, n_splat=N, n_hit=N, n_valid=N - 2, n_fused=N - 2, n_gated=0, n_saturated=0, n_changed=0)

    # max_obs reached: saturated, S and k unchanged -- and a smaller cap than the k a pixel has holds it as well
    d1 = np.full((rows, cols), 8200, dtype=np.uint16)
    S1, K1, F1, cnt = _one(capi, cfg, flat, d1, max_obs=1)
    assert cnt["n_fused"] == N and (F1 == 8196).all()
    S2, K2, F2, cnt = _one(capi, cfg, flat, d1, max_obs=1, sums=S1, obs=K1)
    assert np.array_equal(S2, S1) and np.array_equal(K2, K1) and np.array_equal(F2, F1)
    assert (cnt["n_fused"], cnt["n_gated"], cnt["n_saturated"], cnt["n_changed"]) == (0, 0, N, 0)
    S3, K3, F3, cnt = _one(capi, cfg, flat, d1, max_obs=2, sums=S2, obs=K2)
    assert (K3 == 2).all() and (F3 == 8197).all() and (cnt["n_fused"], cnt["n_saturated"], cnt["n_changed"]) == (N, 0, N)
    S4, K4, F4, cnt = _one(capi, cfg, flat, d1, max_obs=1, sums=S3, obs=K3)
    assert np.array_equal(S4, S3) and np.array_equal(K4, K3) and np.array_equal(F4, F3) and cnt["n_saturated"] == N
    # a saturated pixel is not gated: the cap is asked first
    far = np.full((rows, cols), 4096, dtype=np.uint16)
    assert _one(capi, cfg, flat, far, max_obs=2, sums=S3, obs=K3)[3]["n_saturated"] == N
    assert _one(capi, cfg, flat, far, max_obs=3, sums=S3, obs=K3)[3]["n_gated"] == N


# ---- the host function against the restatement on the GPU tests' scene ----------------------------------------------------------
TABLE = {  # (rows, cols): valid keyframe pixels, {pose: (hit and valid, within gate 50 / 20, gated, within gate 0 / 0)}
    (120, 168): (18860, dict(pose=(18302, 15422, 2880, 401), pose_out=(10963, 1027, 9936, 4))),
    (122, 174): (None, dict(pose=(19346, 16466, 2880, 445), pose_out=(11578, 1036, 10542, 4))),
}
# (pose, gate_abs, gate_rel_1024, max_obs), each on the planes the one before left
SEQUENCE = (("pose", GA, GR, 1), ("pose", GA, GR, 1), ("pose_out", 0, 0, 2), ("pose", 10, 0, 2), ("pose", GA, GR, 2), ("pose_out", GA, GR, 255),
            ("pose", 0, 0, 255), ("pose_out", 10, 0, 255), ("pose", 10, 0, 255), ("pose_out", 10, 0, 1))


@pytest.mark.parametrize("rows,cols", [(120, 168), (122, 174)])
def test_host_equals_the_restatement(capi, synth, rows, cols):
    capi.load()
    s = fr.Scene(synth, rows, cols, 4)
    cfg = s.cfg(capi)
    worst = np.inf
    n_valid, table = TABLE[rows, cols]
    for name in ("pose", "pose_out"):  # the scene's branches from an unfused state
        hit_valid, inside, gated, exact = table[name]
        pose = getattr(s, name)
        _, _, fused, cnt = capi.reffuse_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, pose, GA, GR, 255)
        cnt = ur.counts_dict(cnt)
        print(f"{rows} x {cols}, {name}: {cnt}")
        assert n_valid is None or cnt["n_valid"] == n_valid
        assert (cnt["n_fused"] + cnt["n_gated"], cnt["n_fused"], cnt["n_gated"], cnt["n_saturated"]) == (hit_valid, inside, gated, 0)
        assert capi.reffuse_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, pose, 0, 0, 255)[3]["n_fused"] == exact
        if name == "pose":  # (14 649 and 15 601 values change: a mean within half a count of u rounds back to u)
            assert cnt["n_fused"] >= cnt["n_changed"] > 12000 and 12 <= _median_abs(ur, cfg, s, pose) <= 13
    S = np.zeros((rows, cols), dtype=np.uint32)
    K = np.zeros((rows, cols), dtype=np.uint8)
    seen = dict(n_fused=0, n_gated=0, n_saturated=0, n_changed=0)
    for k, (name, ga, gr, mo) in enumerate(SEQUENCE):
        args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, getattr(s, name), ga, gr, mo, S, K)
        S2, K2, fused, cnt = capi.reffuse_host(*args)
        wS, wK, wF, wcnt, margin = ur.restate(*args)
        what = f"{rows} x {cols}, call {k}: {name}, gate {ga} / {gr}, max_obs {mo}"
        print(f"{what}: {wcnt}, margin {margin:.3e}")
        assert np.array_equal(S2, wS) and np.array_equal(K2, wK) and np.array_equal(fused, wF), what
        assert ur.counts_dict(cnt) == wcnt, what
        assert np.array_equal(fused != 0, K2 != 0) and not (fused != 0)[~_valid(s.dep0)].any(), what
        worst = min(worst, margin)
        seen = {n: max(seen[n], wcnt[n]) for n in seen}
        S, K = S2, K2
    assert worst > 1e-9, "a decision of the scene hangs on a last bit: move the scene"
    assert all(v > 0 for v in seen.values()), f"a branch of the rule was never reached: {seen}"
    assert int(K.max()) > 2, "no pixel went beyond the small caps"


def _valid(dep, factor=F5000):
    z = dep.astype(np.float64) * factor
    return ~((z < 0.01) | (z > 100))


def _median_abs(ur, cfg, s, pose):
    q, _, _ = ur.zbuffer(cfg, F5000, s.T0, s.dep1, F5000, pose)
    both = (q != 0) & _valid(s.dep0)
    return float(np.median(np.abs(q[both] - s.dep0[both].astype(np.int64))))


# ---- fill and fusion commute --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(120, 168), (122, 174)])
def test_fill_and_fusion_commute(capi, synth, rows, cols):
    """host twins only: for one target depth and pose, fill then fuse == fuse then fill, where the later fill reads BASE"""
    capi.load()
    s = fr.Scene(synth, rows, cols, 4)
    cfg = s.cfg(capi)
    moved = 0
    for pose in (s.pose, s.pose_out):
        for guard in (0, 1, 2):
            view = (s.T0, s.dep1, F5000, pose)
            # fill, then fuse: the fusion reads the uploaded depth, whatever is filled
            fill_a, _ = capi.reffill_host(cfg, s.dep0, F5000, *view, guard, fr.GUARD_ABS, fr.GUARD_REL)
            _, _, fused_a, cnt = capi.reffuse_host(cfg, s.dep0, F5000, *view, GA, GR, 255)
            # fuse, then fill on the BASE plane
            _, _, fused_b, _ = capi.reffuse_host(cfg, s.dep0, F5000, *view, GA, GR, 255)
            base = ur.base(fused_b, s.dep0)
            fill_b, _ = capi.reffill_host(cfg, base, F5000, *view, guard, fr.GUARD_ABS, fr.GUARD_REL)
            assert np.array_equal(fill_a, fill_b), f"guard {guard}: {int((fill_a != fill_b).sum())} fills differ"
            assert np.array_equal(fused_a, fused_b)
            assert np.array_equal(ur.completed(fill_a, fused_a, s.dep0), ur.completed(fill_b, fused_b, s.dep0))
            assert fill_a.any() and int(cnt["n_changed"]) > 500
            moved += int((base != s.dep0).sum())
    assert moved > 0


# ---- what it is for -------------------------------------------------------------------------------------------------------------
def test_fusion_halves_the_depth_noise_of_a_plane(capi):
    """A fronto-parallel plane at the identity pose, 24 x 32, factor 2^-12, truth 8192 counts; the keyframe and eight target
    frames carry independent integer noise uniform in [-20, 20]; gate_abs 64.  The mean of nine independent samples has a
    third of one sample's deviation plus at most half a count of rounding: the RMS error of the completed depth must be below
    HALF the uploaded map's."""
    capi.load()
    rows, cols = 24, 32
    cfg = _cfg(capi)
    rng = np.random.default_rng(20261021)
    truth = 8192
    noisy = lambda: (truth + rng.integers(-20, 21, size=(rows, cols))).astype(np.uint16)
    dep0 = noisy()
    S = K = None
    for _ in range(8):
        S, K, fused, cnt = capi.reffuse_host(cfg, dep0, F12, EYE16, noisy(), F12, IDENTITY, 64, 0, 255, S, K)
        assert int(cnt["n_fused"]) == rows * cols and int(cnt["n_gated"]) == 0
    assert (K == 8).all() and (fused != 0).all()
    comp = ur.completed(np.zeros_like(dep0), fused, dep0).astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    before, after = rms(dep0.astype(np.float64)), rms(comp)
    print(f"RMS error against the truth: uploaded {before:.3f} counts, after eight fusions {after:.3f} counts")
    assert after < 0.5 * before
    assert (np.abs(fused.astype(np.int64) - dep0.astype(np.int64)) <= 64).all(), "a fused value left the gate of its uploaded sample"


def test_rule_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/reffuse_check.cpp: csrc/nid_reffuse_rule.h -- the refined count, the gate and the host's loop on top of the
    fill's part A -- in a program of its own (its own main, no preloaded runtime), built with -fsanitize=address,undefined as
    reffill_check.cpp is: random and degenerate inputs reach no undefined conversion or index and keep the invariants."""
    exe = str(tmp_path / "reffuse_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nid-pose-estimation_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "reffuse_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"reffuse: (\d+) planes \((\d+) with a special value\), (\d+) fused, (\d+) gated, (\d+) saturated, (\d+) changed, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 4000 and int(m.group(2)) >= 150 and int(m.group(3)) >= 50000 and int(m.group(4)) >= 5000 and \
        int(m.group(5)) >= 5000 and int(m.group(6)) >= 20000, r.stdout
