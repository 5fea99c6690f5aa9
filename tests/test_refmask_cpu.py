"""include/nid/nid_refmask.h without a device: the export table, the argument rules (checked before any device is touched),
known answers of nid_refmask_host, the host function against a numpy restatement of the header's rule on the scene the
GPU tests classify -- planes and counts compared for equality, and no decision of that scene within 1e-9 of a threshold --
and the rule alone in a program of its own under the host sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("refmask_restate", os.path.join(ROOT, "tests", "refmask_restate.py"))
rr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rr)

INVALID_ARG = -1
F5000 = rr.F5000
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0.0])
EYE16 = np.eye(4).reshape(16)


def _declared():
    txt = open(os.path.join(ROOT, "include", "nid", "nid_refmask.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nid_[A-Za-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported(capi):
    lib = capi.load()
    declared = _declared()
    assert len(declared) == 7 and sorted(capi.REFMASK_SYMBOLS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nid_[A-Za-z0-9_]+)", nm))
    for name in declared:
        assert hasattr(lib, name) and name in exported, f"{name} declared in nid_refmask.h but not exported"
    for other in (capi.SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PYR_SYMBOLS, capi.STREAM_SYMBOLS, capi.KEYFRAME_SYMBOLS, capi.MULTI_SYMBOLS):
        assert not set(declared) & set(other)
    assert lib.nid_abi_version() == 4, "nid_refmask.h is a header of its own: the C-ABI of nid_c.h has not changed"
    assert (capi.REFMASK_CALLER, capi.REFMASK_OCCLUDED, capi.REFMASK_THROUGH, capi.REFMASK_DILATED, capi.REFMASK_MAX_DILATE) == (1, 2, 4, 8, 8)


def _cfg(capi, rows=24, cols=32, fx=128.0, fy=-128.0, cx=15.5, cy=11.5):
    return capi.NidConfig(rows, cols, 4, 8, 3, 0, 0, 0, fx, fy, cx, cy)


def test_argument_rules_before_any_device(capi):
    lib = capi.load()
    cfg = _cfg(capi)
    N = 24 * 32
    d0, d1, m = np.full(N, 10000, dtype=np.uint16), np.full(N, 10000, dtype=np.uint16), np.zeros(N, dtype=np.uint8)
    cnt = np.zeros(1, dtype=capi.REFMASK_COUNTS_DTYPE)
    dp, u16p, u8p, vp = (lambda a: a.ctypes.data_as(capi.c_dp)), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))), \
        (lambda a: a.ctypes.data_as(capi.c_u8p)), (lambda a: a.ctypes.data_as(C.c_void_p))
    opt = lambda f, a: f(a) if a is not None else None

    def host(c=cfg, D0=d0, T=EYE16, D1=d1, Q=IDENTITY, ta=0.01, tr=0.02, classes=6, dilate=2, acc=0, Mk=m, Cn=cnt):
        return lib.nid_refmask_host(C.byref(c) if c is not None else None, opt(u16p, D0), F5000, opt(dp, T), opt(u16p, D1), F5000, opt(dp, Q), ta, tr,
                                    classes, dilate, acc, opt(u8p, Mk), opt(vp, Cn))

    assert host() == 0 and host(Cn=None) == 0 and host(classes=0, dilate=0) == 0 and host(dilate=8, acc=1) == 0
    for name in ("c", "D0", "T", "D1", "Q", "Mk"):
        assert host(**{name: None}) == INVALID_ARG, name
    for bad in (-1e-9, np.nan, np.inf, -np.inf):
        assert host(ta=bad) == INVALID_ARG and host(tr=bad) == INVALID_ARG
    for bad in (1, 3, 8, 7, -2, 16):
        assert host(classes=bad) == INVALID_ARG, bad
    for bad in (-1, 9, 1000):
        assert host(dilate=bad) == INVALID_ARG, bad
    assert host(c=_cfg(capi, rows=0)) == INVALID_ARG and host(c=_cfg(capi, cols=0)) == INVALID_ARG
    # the pyramid's and the tracker's entry points: a null handle or pointer, classes, dilate and the tolerances are refused first
    assert lib.nid_pyr_set_reference_mask_u8(None, u8p(m)) == INVALID_ARG
    assert lib.nid_pyr_mask_occluded(None, dp(IDENTITY), 0.01, 0.02, 6, 2, 0, vp(cnt)) == INVALID_ARG
    assert lib.nid_pyr_clear_reference_mask(None) == INVALID_ARG
    assert lib.nid_pyr_get_reference_mask_u8(None, u8p(m)) == INVALID_ARG
    assert lib.nid_track_set_masking(None, 6, 2) == INVALID_ARG
    assert lib.nid_track_last_mask(None, vp(cnt)) == INVALID_ARG


# ---- known answers ------------------------------------------------------------------------------------------------------
def _one(capi, cfg, d0, d1, dilate=0, classes=6, mask=None, accumulate=False, tol_abs=0.25, tol_rel=0.0):
    plane, cnt = capi.refmask_host(cfg, d0, 2.0 ** -12, EYE16, d1, 2.0 ** -12, IDENTITY, tol_abs, tol_rel, classes, dilate, accumulate, mask)
    want, wcnt, _ = rr.restate(cfg, d0, 2.0 ** -12, EYE16, d1, 2.0 ** -12, IDENTITY, tol_abs, tol_rel, classes, dilate, accumulate, mask)
    assert np.array_equal(plane, want) and rr.counts_dict(cnt) == wcnt
    return plane, rr.counts_dict(cnt)


def test_known_answers(capi):
    """identity pose and matrix, depth factor 2^-12: a pixel projects onto itself and every quantity is exact.  The
    keyframe is a plane at 2 m; a target sample at 1 m occludes the keyframe pixel under it, one at 4 m is seen through."""
    capi.load()
    rows, cols = 24, 32
    cfg = _cfg(capi)
    d0 = np.full((rows, cols), 8192, dtype=np.uint16)
    flat = d0.copy()
    plane, cnt = _one(capi, cfg, d0, flat, dilate=8)
    assert not plane.any() and cnt == dict(n_valid=rows * cols, n_caller=0, n_occluded=0, n_through=0, n_dilated=0, n_masked=0)

    # a single occluded pixel in the middle, dilate 2: a 5 x 5 block
    d1 = flat.copy()
    d1[10, 12] = 4096
    plane, cnt = _one(capi, cfg, d0, d1, dilate=2)
    want = np.zeros((rows, cols), dtype=np.uint8)
    want[8:13, 10:15] = 8
    want[10, 12] = 2
    assert np.array_equal(plane, want) and (cnt["n_occluded"], cnt["n_dilated"], cnt["n_masked"]) == (1, 24, 25)
    # ... at the corner and at an edge: the block is clipped at the border
    for (r, c), shape in (((0, 0), (3, 3)), ((rows - 1, cols - 2), (3, 4)), ((1, 15), (4, 5))):
        d1 = flat.copy()
        d1[r, c] = 4096
        plane, cnt = _one(capi, cfg, d0, d1, dilate=2)
        want = np.zeros((rows, cols), dtype=np.uint8)
        want[max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = 8
        want[r, c] = 2
        assert np.array_equal(plane, want) and cnt["n_dilated"] == shape[0] * shape[1] - 1, (r, c)
    # dilate 0 leaves the pixel alone; a class that is not selected leaves nothing
    d1 = flat.copy()
    d1[10, 12] = 4096
    d1[5, 5] = 16384
    plane, cnt = _one(capi, cfg, d0, d1)
    assert plane[10, 12] == 2 and plane[5, 5] == 4 and int(plane.astype(int).sum()) == 6
    plane, _ = _one(capi, cfg, d0, d1, classes=2, dilate=1)
    assert plane[10, 12] == 2 and plane[5, 5] == 0 and int((plane == 8).sum()) == 8
    plane, _ = _one(capi, cfg, d0, d1, classes=4)
    assert plane[10, 12] == 0 and plane[5, 5] == 4
    plane, _ = _one(capi, cfg, d0, d1, classes=0, dilate=8)
    assert not plane.any()

    # an invalid pristine depth gives no class bits -- but the dilation of a neighbour reaches it, and it is not counted as masked
    hole = d0.copy()
    hole[10, 12] = 0
    d1 = flat.copy()
    d1[10, 12] = 4096
    plane, cnt = _one(capi, cfg, hole, d1, dilate=2)
    assert not plane.any() and cnt["n_valid"] == rows * cols - 1
    d1[10, 13] = 4096
    plane, cnt = _one(capi, cfg, hole, d1, dilate=1)
    assert plane[10, 12] == 8 and plane[10, 13] == 2 and (cnt["n_dilated"], cnt["n_masked"]) == (8, 8)

    # the caller's bit stays, the derived bits go unless accumulated; a pixel of a class loses an accumulated bit 8
    before = np.zeros((rows, cols), dtype=np.uint8)
    before[2, 3] = 1 | 4
    before[20, 20] = 8
    before[10, 11] = 8
    before[10, 12] = 1 | 8
    d1 = flat.copy()
    d1[10, 12] = 4096
    plane, cnt = _one(capi, cfg, d0, d1, mask=before)
    assert (plane[2, 3], plane[20, 20], plane[10, 11], plane[10, 12]) == (1, 0, 0, 3) and cnt["n_caller"] == 2
    plane, cnt = _one(capi, cfg, d0, d1, mask=before, accumulate=True)
    assert (plane[2, 3], plane[20, 20], plane[10, 11], plane[10, 12]) == (5, 8, 8, 3)
    plane, cnt = _one(capi, cfg, d0, d1, mask=before, accumulate=True, dilate=1)
    assert plane[1, 2] == 8 and plane[2, 3] == 5 and int((plane & 8 != 0).sum()) == 8 + 8 + 1

    # the tolerance's edges (tol = 0.25, every quantity dyadic): |dz| == tol is consistent, one count of depth more is not
    d1 = flat.copy()
    d1[4, 4], d1[4, 6] = 7168, 7167    # zt = 1.75: dz = 0.25; zt = 1.75 - 2^-12
    d1[6, 4], d1[6, 6] = 9216, 9217    # zt = 2.25: dz = -0.25; zt = 2.25 + 2^-12
    plane, _ = _one(capi, cfg, d0, d1)
    assert (plane[4, 4], plane[4, 6], plane[6, 4], plane[6, 6]) == (0, 2, 0, 4)


# ---- the host function against the restatement on the GPU tests' scene ----------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(120, 168), (122, 174)])
def test_host_equals_the_restatement(capi, synth, rows, cols):
    capi.load()
    s = rr.Scene(synth, rows, cols, 4)
    cfg = s.cfg(capi)
    worst = np.inf
    seen = dict(n_occluded=0, n_through=0, n_dilated=0)
    for pose in (s.pose, s.pose_out):
        for classes in (2, 4, 6):
            for dilate in (0, 1, 8):
                args = (cfg, s.dep0, F5000, s.T0, s.dep1, F5000, pose, 0.01, 0.02, classes, dilate)
                plane, cnt = capi.refmask_host(*args, False, None)
                want, wcnt, margin = rr.restate(*args, False, None)
                assert np.array_equal(plane, want) and rr.counts_dict(cnt) == wcnt, (classes, dilate)
                worst = min(worst, margin)
                for k in seen:
                    seen[k] = max(seen[k], wcnt[k])
                # accumulate on top of another call's plane and a caller's bit
                prior = want.copy()
                prior[40:50, 100:120] |= 1
                args2 = (cfg, s.dep0, F5000, s.T0, s.dep0, F5000, s.pose0, 0.0, 0.001, 6, 1)  # the keyframe's own depth, tight tolerances
                for acc in (False, True):
                    plane2, cnt2 = capi.refmask_host(*args2, acc, prior)
                    want2, wcnt2, _ = rr.restate(*args2, acc, prior)
                    assert np.array_equal(plane2, want2) and rr.counts_dict(cnt2) == wcnt2, (classes, dilate, acc)
                assert wcnt2["n_caller"] == 200 and wcnt2["n_masked"] >= wcnt["n_masked"]
    print(f"{rows} x {cols}: smallest margin to a threshold {worst:.3e}, most bits seen {seen}")
    assert worst > 1e-9, "a decision of the scene hangs on a last bit: move the scene"
    assert seen["n_occluded"] > 500 and seen["n_through"] > 500 and seen["n_dilated"] > 100
    # the pose that moves part of the keyframe out of view classifies fewer pixels
    _, a = capi.refmask_host(cfg, s.dep0, F5000, s.T0, s.dep1, F5000, s.pose, 0.01, 0.02, 6, 0)
    _, b = capi.refmask_host(cfg, s.dep0, F5000, s.T0, np.full_like(s.dep1, 5000), F5000, s.pose_out, 0.01, 0.02, 6, 0)
    assert 0 < int(b["n_occluded"]) < int(b["n_valid"]) == int(a["n_valid"]) < rows * cols


def test_rule_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/refmask_check.cpp: csrc/nid_depth_check.h -- classify, the back-projection and the host's masking loop --
    in a program of its own (its own main, no preloaded runtime), built with -fsanitize=address,undefined as
    depth_check_check.cpp is: classify plus counting reproduces dc::sample's counts on random and degenerate samples; the
    masking loop over random and degenerate planes reaches no undefined conversion or index and keeps its invariants."""
    exe = str(tmp_path / "refmask_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nid-pose-estimation_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "refmask_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"refmask: (\d+) samples \((\d+) with a special value, (\d+) classified at step 5\), (\d+) planes \((\d+) bits set\), 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 200000 and int(m.group(2)) >= 50000 and int(m.group(3)) >= 5000 and int(m.group(4)) >= 100 and int(m.group(5)) >= 1000, r.stdout
