"""include/nid/nid_pyr_stream.h without a device: the export table, the argument rules (checked before any device is
touched) and the pose helpers against the 4x4-matrix route in numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = -1, -2
# per component, on poses of the size synth.make_pair uses: a few tens of ulps of O(1) quantities, the order two sin / cos
# implementations differ by (the written-out sin / cos against libm's)
TOL = 1e-14
EPS = np.finfo(np.float64).eps


def _declared():
    txt = open(os.path.join(ROOT, "include", "nid", "nid_pyr_stream.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nid_[A-Za-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported(capi):
    lib = capi.load()
    declared = _declared()
    assert len(declared) == 14 and sorted(capi.STREAM_SYMBOLS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nid_[A-Za-z0-9_]+)", nm))
    for name in declared:
        assert hasattr(lib, name) and name in exported, f"{name} declared in nid_pyr_stream.h but not exported"
    assert not set(declared) & set(capi.SYMBOLS) and not set(declared) & set(capi.PYR_SYMBOLS)
    assert not set(declared) & set(capi.MULTISTART_SYMBOLS) and not set(declared) & set(capi.MULTI_SYMBOLS)
    assert lib.nid_abi_version() == 4, "nid_pyr_stream.h is a header of its own: the C-ABI of nid_c.h has not changed"


def test_null_handles_and_pointers_are_refused(capi):
    lib = capi.load()
    p7, t6, T16 = np.array([0, 0, 0, 1, 0, 0, 0.0]), np.zeros(6), np.eye(4).reshape(16)
    o7, o16 = np.zeros(7), np.zeros(16)
    dp = lambda a: a.ctypes.data_as(capi.c_dp)
    im = np.zeros(4, dtype=np.uint8).ctypes.data_as(capi.c_u8p)
    dep = np.zeros(4, dtype=np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))
    res = capi.TrackResult()
    assert lib.nid_pyr_set_target_u8(None, im) == INVALID_ARG
    assert lib.nid_pyr_promote_target_u16(None, dep, 1.0, dp(T16)) == INVALID_ARG
    assert lib.nid_track_pose_inverse(None, dp(o7)) == INVALID_ARG and lib.nid_track_pose_inverse(dp(p7), None) == INVALID_ARG
    assert lib.nid_track_pose_compose(None, dp(p7), dp(o7)) == INVALID_ARG and lib.nid_track_pose_compose(dp(p7), None, dp(o7)) == INVALID_ARG
    assert lib.nid_track_pose_compose(dp(p7), dp(p7), None) == INVALID_ARG
    assert lib.nid_track_pose_perturb(None, dp(t6), dp(o7)) == INVALID_ARG and lib.nid_track_pose_perturb(dp(p7), None, dp(o7)) == INVALID_ARG
    assert lib.nid_track_pose_perturb(dp(p7), dp(t6), None) == INVALID_ARG
    assert lib.nid_track_pose_to_Twc16(None, dp(o16)) == INVALID_ARG and lib.nid_track_pose_to_Twc16(dp(p7), None) == INVALID_ARG
    assert lib.nid_track_pose_from_Twc16(None, dp(o7)) == INVALID_ARG and lib.nid_track_pose_from_Twc16(dp(T16), None) == INVALID_ARG
    assert lib.nid_track_destroy(None) == 0 and not lib.nid_track_pyramid(None)
    assert lib.nid_track_set_lm(None, 3, 1.0, None) == INVALID_ARG
    assert lib.nid_track_set_twists(None, dp(t6), 1) == INVALID_ARG
    assert lib.nid_track_set_pose(None, dp(p7)) == INVALID_ARG
    assert lib.nid_track_push_u16(None, dep, 1.0, im, None, C.byref(res)) == INVALID_ARG


def test_track_create_refuses_what_pyr_create_refuses_before_any_device(capi):
    lib = capi.load()
    h = C.c_void_p()
    good = capi.NidConfig(120, 160, 4, 8, 3, 0, 0, 0, 120.3, -120.0, 79.5, 59.5)
    odd_rows = capi.NidConfig(122, 160, 4, 8, 3, 0, 0, 0, 120.3, -120.0, 79.5, 59.5)
    odd_cols = capi.NidConfig(120, 162, 4, 8, 3, 0, 0, 0, 120.3, -120.0, 79.5, 59.5)
    shard = capi.NidConfig(120, 160, 4, 8, 3, 0, 0, 8, 120.3, -120.0, 79.5, 59.5)
    for cfg, levels in ((good, 4), (good, 0), (good, 9), (good, -1), (odd_rows, 3), (odd_cols, 3), (shard, 1), (shard, 3)):
        assert lib.nid_pyr_create(C.byref(cfg), levels, C.byref(h)) == INVALID_ARG
        assert lib.nid_track_create(C.byref(cfg), levels, C.byref(h)) == INVALID_ARG and not h
    assert lib.nid_track_create(None, 3, C.byref(h)) == INVALID_ARG
    assert lib.nid_track_create(C.byref(good), 3, None) == INVALID_ARG
    if lib.nid_device_count() > 0:
        # with a device the same call succeeds, and the argument rules of the setters can be seen
        assert lib.nid_track_create(C.byref(good), 3, C.byref(h)) == 0 and lib.nid_pyr_levels(lib.nid_track_pyramid(h)) == 3
        tw = np.zeros((capi.NID_MAX_BATCH, 6))
        assert lib.nid_track_set_twists(h, tw.ctypes.data_as(capi.c_dp), capi.NID_MAX_BATCH - 1) == INVALID_ARG
        assert lib.nid_track_set_twists(h, tw.ctypes.data_as(capi.c_dp), capi.NID_MAX_BATCH - 2) == 0
        assert lib.nid_track_set_twists(h, tw.ctypes.data_as(capi.c_dp), -1) == INVALID_ARG
        assert lib.nid_track_set_twists(h, None, 1) == INVALID_ARG and lib.nid_track_set_twists(h, None, 0) == 0
        assert lib.nid_track_set_lm(h, 0, 1.0, None) == INVALID_ARG
        for bad in ([2, 1, 5], [0, 1, 5]):
            assert lib.nid_track_set_lm(h, 3, 1.0, np.array(bad, dtype=np.int32).ctypes.data_as(capi.c_ip)) == INVALID_ARG
        assert lib.nid_track_set_lm(h, 3, 1.0, np.array([1, 2, 5], dtype=np.int32).ctypes.data_as(capi.c_ip)) == 0
        assert lib.nid_track_destroy(h) == 0
        return
    assert lib.nid_track_create(C.byref(good), 3, C.byref(h)) == NO_DEVICE and not h
    with pytest.raises(capi.NidError):
        capi.Tracker(120, 160, 4, 8, 120.3, -120.0, 79.5, 59.5, levels=3)


def _poses(synth, n, seed):
    """poses of the size synth.make_pair uses: its pose_init, perturbed as the tests' start clouds are, and such steps
    composed a few times"""
    rng = np.random.default_rng(seed)
    base = synth.make_pair("S").pose_init
    out = []
    for _ in range(n):
        p = base
        for _ in range(int(rng.integers(1, 4))):
            p = synth.perturb_pose7(p, rng.normal(0, 1e-2, 3), rng.normal(0, 5e-2, 3))
        out.append(p)
    return out


def _unit(q7, what):
    assert q7[3] >= 0, what
    assert abs(np.linalg.norm(q7[:4]) - 1.0) <= 4 * EPS, what


def _same_matrix(synth, pose7, M, what):
    d = np.abs(synth.pose7_to_matrix(pose7) - M).max()
    assert d <= TOL, f"{what}: {d:.3e}"


def test_pose_helpers_agree_with_the_matrix_route(capi, synth):
    capi.load()
    ps = _poses(synth, 40, 7)
    rng = np.random.default_rng(8)
    for k, (a, b) in enumerate(zip(ps[0::2], ps[1::2])):
        Ma, Mb = synth.pose7_to_matrix(a), synth.pose7_to_matrix(b)
        inv = capi.pose_inverse(a)
        _unit(inv, f"inverse {k}")
        _same_matrix(synth, inv, np.linalg.inv(Ma), f"inverse {k}")
        back = capi.pose_inverse(inv)
        assert np.abs(back - a).max() <= TOL, f"inverse(inverse(p)) {k}"
        ab = capi.pose_compose(a, b)
        _unit(ab, f"compose {k}")
        _same_matrix(synth, ab, Ma @ Mb, f"compose {k}")
        # the tracker's prediction (cur o inverse(prev)) o cur
        pred = capi.pose_compose(capi.pose_compose(a, capi.pose_inverse(b)), a)
        _same_matrix(synth, pred, Ma @ np.linalg.inv(Mb) @ Ma, f"prediction {k}")
        om, up = rng.normal(0, 1e-3, 3), rng.normal(0, 2e-3, 3)
        got = capi.pose_perturb(a, np.concatenate([om, up]))
        _unit(got, f"perturb {k}")
        want = synth.perturb_pose7(a, om, up)
        assert np.abs(got - want).max() <= TOL, f"perturb {k}: {np.abs(got - want).max():.3e}"
        T = capi.pose_to_Twc16(a)
        assert np.abs(T.reshape(4, 4).T - np.linalg.inv(Ma)).max() <= TOL, f"to_Twc16 {k}"
        assert T.reshape(4, 4).T[3].tolist() == [0, 0, 0, 1]
        assert np.abs(capi.pose_from_Twc16(T) - a).max() <= TOL, f"from_Twc16 {k}"
        assert np.abs(capi.pose_from_Twc16(synth.matrix_colmajor16(np.linalg.inv(Ma))) - a).max() <= TOL, f"from_Twc16 of numpy's inverse {k}"


def test_composition_with_a_negative_raw_w_is_renormalised(capi, synth):
    """two rotations of 0.6 x 2 pi about one axis: each quaternion has w = cos(0.6 pi) -> stored with w >= 0 (the
    convention), their raw product has w < 0; the result is unit, w >= 0, and the rotation the matrices give"""
    capi.load()
    ang = 0.6 * np.pi
    axis = np.array([1.0, 2.0, -2.0]) / 3.0
    q = np.concatenate([np.sin(ang) * axis, [np.cos(ang)]])
    a = np.concatenate([-q, [0.1, -0.2, 0.3]])  # w >= 0
    assert a[3] > 0
    b = synth.perturb_pose7(a, [0.01, 0.0, 0.02], [0.0, 0.1, 0.0])
    raw_w = a[3] * b[3] - a[:3] @ b[:3]
    assert raw_w < 0
    ab = capi.pose_compose(a, b)
    _unit(ab, "compose with a raw w < 0")
    _same_matrix(synth, ab, synth.pose7_to_matrix(a) @ synth.pose7_to_matrix(b), "compose with a raw w < 0")


def test_pose_helpers_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/track_pose_check.cpp: csrc/nid_track_pose.h alone in a program of its own, built with
    -fsanitize=address,undefined (runtimes linked statically: nothing of the environment is involved): the same identities
    over 4000 LCG poses, with twists on both sides of the exponential's small-angle switch."""
    exe = str(tmp_path / "track_pose_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nid-pose-estimation_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "track_pose_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"track pose: (\d+) cases \((\d+) twists below the small-angle switch, (\d+) above, (\d+) compositions with a raw w < 0\), 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) >= 200 and int(m.group(3)) >= 200 and int(m.group(4)) >= 20, r.stdout
