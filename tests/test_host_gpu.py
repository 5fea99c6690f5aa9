"""The C++ host stack on a GPU: the legacy operator signatures against the
oracle, and the recovered pose of the reference driver's 10-iteration LM against
the oracle's LM (pose tolerance 1e-6 per minimal-vector
component given an identical accept/reject sequence; the trace is compared too)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib():
    h = importlib.import_module("nid-pose-estimation_amd.hostlib")
    h.load()
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("strict", [False, True])
def test_legacy_operators(hostlib, oracle, synth, pair_S_edge, strict):
    import ctypes as C
    pair, nb = pair_S_edge, 10
    lib = hostlib.load()
    lib.nid_legacy_reset()
    lib.nid_legacy_set_math_mode(1 if strict else 0)   # the edge-case pair has saturated patches: both modes must hold
    N = pair.rows * pair.cols
    ncell = pair.cell ** 2
    dp = lambda a: a.ctypes.data_as(hostlib.c_dp)
    ip = lambda a: a.ctypes.data_as(hostlib.c_ip)
    depth = np.ascontiguousarray(pair.depth_m.reshape(-1))
    T = synth.matrix_colmajor16(pair.T_wc0)
    intr = pair.intr.copy()
    pts = np.zeros(3 * N)
    lib.nid_legacy_call_Calculate3Dpoint(dp(depth), dp(T), dp(pts), dp(intr), pair.rows, pair.cols)
    o = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix")
    m = ~np.isnan(o.points3d)
    assert np.array_equal(np.isnan(pts), ~m)
    assert np.array_equal(_bits(pts[m]), _bits(o.points3d[m]))

    im0 = pair.im0.reshape(-1).astype(np.float64)
    im1 = pair.im1.reshape(-1).astype(np.float64)
    M0 = oracle.se3_to_matrix16(pair.pose_init)
    bsv = np.zeros(4 * N); bsi = np.zeros(N, dtype=np.int32); cnt = np.zeros(ncell, dtype=np.int32)
    href = np.zeros(ncell)
    lib.nid_legacy_call_CudaComputeHref(dp(im0), dp(pts), dp(M0), dp(intr), nb, 3, pair.cell, pair.rows, pair.cols,
                                        dp(bsv), ip(bsi), ip(cnt), dp(href))
    cnt_o, href_o = o.compute_href(pair.pose_init)
    assert np.array_equal(cnt, cnt_o)
    act = cnt_o >= 300
    assert np.array_equal(np.isnan(href), ~act)
    np.testing.assert_allclose(href[act], href_o[act], rtol=0, atol=1e-11)
    # legacy NaN marker for pixels without a reference weight (CudaComputeHref.cu:126-130)
    d = o.dump_pixels() if False else None
    w = bsv.reshape(-1, 4)
    assert np.isnan(w[~m.reshape(-1, 3)[:, 0]]).all()

    up0 = lib.nid_legacy_upload_count()
    for pose in (pair.pose_init, pair.pose_true):
        M = oracle.se3_to_matrix16(pose)
        Ht = np.zeros(ncell); Hj = np.zeros(ncell); der = np.full(6 * ncell, 123.0)
        lib.nid_legacy_call_CudaComputeH(1, dp(im0), dp(im1), dp(pts), ip(cnt), dp(bsv), ip(bsi), dp(M), dp(intr),
                                         nb, 3, pair.cell, pair.rows, pair.cols, dp(href), dp(Ht), dp(Hj), dp(der))
        Hc_o, Hj_o, err_o, J_o = o.evaluate(pose, True)
        np.testing.assert_allclose(Ht[act], Hc_o[act], rtol=0, atol=1e-11)
        np.testing.assert_allclose(Hj[act], Hj_o[act], rtol=0, atol=1e-11)
        assert np.isnan(Ht[~act]).all() and np.isnan(der.reshape(-1, 6)[~act]).all()
        scale = np.abs(J_o[act]).max()
        np.testing.assert_allclose(der.reshape(-1, 6)[act], J_o[act], rtol=0, atol=1e-9 * scale)
        # cost-only call leaves `der` untouched (computeH.cu:480-481)
        der2 = np.full(6 * ncell, 7.0); Ht2 = np.zeros(ncell); Hj2 = np.zeros(ncell)
        lib.nid_legacy_call_CudaComputeH(0, dp(im0), dp(im1), dp(pts), ip(cnt), dp(bsv), ip(bsi), dp(M), dp(intr),
                                         nb, 3, pair.cell, pair.rows, pair.cols, dp(href), dp(Ht2), dp(Hj2), dp(der2))
        assert np.all(der2 == 7.0)
        assert np.array_equal(_bits(Ht2[act]), _bits(Ht[act]))
    # frame-pair state was uploaded once, not per call (the reference re-uploads 11 MB per call)
    assert lib.nid_legacy_upload_count() - up0 <= 2
    lib.nid_legacy_set_math_mode(0)
    lib.nid_legacy_reset()


def test_compiled_cpp_caller_of_the_legacy_operators(hostlib, oracle, synth, pair_S_edge, tmp_path):
    """The drop-in claim, checked by a compiler: tests/cpp/legacy_caller.cpp uses the operators the way the
    reference's main() does (NID_pose_estimation.cpp:229-276 -- cudaMallocManaged'ed images and points through the
    forwarding header include/nid/compat/cuda_runtime.h, caller-owned malloc'ed outputs, C++ linkage, the g2o
    namespace), is compiled here with g++ against include/nid/legacy_ops.h, linked to libnid_host.so and run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "nid-pose-estimation_amd")
    exe = tmp_path / "legacy_caller"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(root, "include", "nid", "compat"),
                           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "legacy_caller.cpp"),
                           "-o", str(exe), "-L", pkg, "-lnid_host", "-lnid_hip", f"-Wl,-rpath,{pkg}"])
    pair, nb = pair_S_edge, 10
    o = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix")
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pair.rows, pair.cols, pair.cell, nb], dtype=np.int32).tofile(f)
        for a in (pair.intr, synth.matrix_colmajor16(pair.T_wc0), oracle.se3_to_matrix16(pair.pose_init),
                  oracle.se3_to_matrix16(pair.pose_true), pair.depth_m, pair.im0.astype(np.float64), pair.im1.astype(np.float64)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ncell, N = pair.cell ** 2, pair.rows * pair.cols
    with open(tmp_path / "out.bin", "rb") as f:
        cnt = np.fromfile(f, dtype=np.int32, count=ncell)
        href, Ht, Hj = (np.fromfile(f, dtype=np.float64, count=ncell) for _ in range(3))
        der = np.fromfile(f, dtype=np.float64, count=6 * ncell).reshape(-1, 6)
        pts = np.fromfile(f, dtype=np.float64, count=3 * N)
    m = ~np.isnan(o.points3d)
    assert np.array_equal(np.isnan(pts), ~m) and np.array_equal(_bits(pts[m]), _bits(o.points3d[m]))
    cnt_o, href_o = o.compute_href(pair.pose_init)
    assert np.array_equal(cnt, cnt_o)
    act = cnt_o >= 300
    assert np.array_equal(np.isnan(href), ~act)
    np.testing.assert_allclose(href[act], href_o[act], rtol=0, atol=1e-11)
    Hc_o, Hj_o, _, J_o = o.evaluate(pair.pose_true, True)
    np.testing.assert_allclose(Ht[act], Hc_o[act], rtol=0, atol=1e-11)
    np.testing.assert_allclose(Hj[act], Hj_o[act], rtol=0, atol=1e-11)
    assert np.isnan(Ht[~act]).all() and np.isnan(der[~act]).all()
    scale = np.abs(J_o[act]).max(axis=1, keepdims=True)
    assert np.all(np.abs(der[act] - J_o[act]) <= 1e-9 * np.maximum(scale, 1e-6 * scale.max()))


def _write_lm_caller_input(path, pair, nb, poses16, change_at, change_px, pause_every, pose0_16, T16):
    with open(path, "wb") as f:
        np.array([pair.rows, pair.cols, pair.cell, nb, len(poses16), change_at, change_px, pause_every], dtype=np.int32).tofile(f)
        for a in (pair.intr, T16, pose0_16, np.concatenate(poses16), pair.depth_m, pair.im0.astype(np.float64), pair.im1.astype(np.float64)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def test_reference_call_pattern_then_free_at_once(hostlib, oracle, synth, pair_A, tmp_path):
    """VERDICT r05 item 1.  tests/cpp/legacy_lm_caller.cpp replays the reference's whole use of the operators at 640x480
    -- Calculate3Dpoint, CudaComputeHref, 64 CudaComputeH calls in the LM's pattern (der / cost / cost / verbose cost,
    changing poses, 3 ms of host work before every eighth), ONE undeclared in-place change of an im1 pixel that avoids
    the sampled indices, then the frees of NID_pose_estimation.cpp:388-395 at once (7.4 and 9.8 MB blocks: free() unmaps
    them) -- and calls nothing else: no nid_legacy_*.  In the DEFAULT mode, compiled at -O2, MALLOC_PERTURB_ set, 50
    processes: every one exits 0 with the same bytes; the change is followed within NID_LEGACY_SLICES calls and reported once; before
    it and after it the records equal what the operators give on freshly uploaded buffers, bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "nid-pose-estimation_amd")
    hdr = open(os.path.join(root, "include", "nid", "legacy_ops.h")).read()
    per_call = int(re.search(r"#define NID_LEGACY_SLICES_PER_CALL (\d+)", hdr).group(1))
    SLICES = -(-int(re.search(r"#define NID_LEGACY_SLICES (\d+)", hdr).group(1)) // (per_call - per_call // 4))   # calls until every slice was checked (cost-only calls check 3/4 of per_call)
    exe = tmp_path / "legacy_lm_caller"
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-I", os.path.join(root, "include", "nid", "compat"),
                           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "legacy_lm_caller.cpp"),
                           "-o", str(exe), "-L", pkg, "-lnid_host", "-lnid_hip", f"-Wl,-rpath,{pkg}"])
    pair, nb, ncalls, change_at, pause_every = pair_A, 8, 64, 13, 8
    N, ncell = pair.rows * pair.cols, pair.cell ** 2
    change_px = (pair.rows // 2 + 7) * pair.cols + pair.cols // 2 + 9      # mid-image: sampled under every pose of the walk
    assert change_px not in {int(k * (N - 1) // 63) for k in range(64)}
    M_init = oracle.se3_to_matrix16(pair.pose_init)
    poses7, poses16 = [], []
    for k in range(ncalls):   # an LM-like walk: from the initial pose towards the true one, a new pose per call
        w = k / (ncalls - 1.0)
        p7 = np.array(pair.pose_init if k % 3 else pair.pose_true, dtype=np.float64).copy()
        p7[4:7] = (1 - w) * pair.pose_init[4:7] + w * pair.pose_true[4:7]
        poses7.append(p7)
        poses16.append(oracle.se3_to_matrix16(p7))
    T16 = synth.matrix_colmajor16(pair.T_wc0)
    _write_lm_caller_input(tmp_path / "in.bin", pair, nb, poses16, change_at, change_px, pause_every, M_init, T16)
    env = dict(os.environ, MALLOC_PERTURB_="165")
    for drop in ("NID_LEGACY_TRUST_BUFFERS", "NID_LEGACY_VERIFY_EVERY_CALL", "NID_LEGACY_VERIFY_SLICES", "NID_LEGACY_ALWAYS_UPLOAD"):
        env.pop(drop, None)
    first = None
    for run in range(50):
        r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (run, r.returncode, r.stderr[-2000:])
        assert r.stderr.count("rewritten IN PLACE") == 1, (run, r.stderr[-2000:])
        out = open(tmp_path / "out.bin", "rb").read()
        if first is None:
            first = out
        assert out == first, f"run {run}: another result than run 0"
    cnt = np.frombuffer(first, dtype=np.int32, count=ncell)
    rec = np.frombuffer(first, dtype=np.float64, offset=4 * ncell).reshape(ncalls, 8, ncell)

    # what the operators give for each pose on freshly handed-over buffers, unchanged and changed target
    lib = hostlib.load()
    lib.nid_legacy_reset()
    lib.nid_legacy_set_verify_mode.argtypes = [hostlib.C.c_int]
    lib.nid_legacy_set_verify_mode(1)   # every slice on every call
    dp = lambda a: a.ctypes.data_as(hostlib.c_dp)
    ip = lambda a: a.ctypes.data_as(hostlib.c_ip)
    try:
        depth = np.ascontiguousarray(pair.depth_m.reshape(-1)); intr = pair.intr.copy(); pts = np.zeros(3 * N)
        im0 = pair.im0.reshape(-1).astype(np.float64); im1 = pair.im1.reshape(-1).astype(np.float64)
        bsv = np.zeros(4 * N); bsi = np.zeros(N, dtype=np.int32); cnt2 = np.zeros(ncell, dtype=np.int32); href = np.zeros(ncell)
        lib.nid_legacy_call_Calculate3Dpoint(dp(depth), dp(T16), dp(pts), dp(intr), pair.rows, pair.cols)
        lib.nid_legacy_call_CudaComputeHref(dp(im0), dp(pts), dp(M_init), dp(intr), nb, 3, pair.cell, pair.rows, pair.cols,
                                            dp(bsv), ip(bsi), ip(cnt2), dp(href))
        assert np.array_equal(cnt, cnt2)
        act = cnt >= 300

        def evaluate(k):
            Ht = np.zeros(ncell); Hj = np.zeros(ncell); der = np.zeros(6 * ncell)
            lib.nid_legacy_call_CudaComputeH(1, dp(im0), dp(im1), dp(pts), ip(cnt2), dp(bsv), ip(bsi), dp(poses16[k]), dp(intr),
                                             nb, 3, pair.cell, pair.rows, pair.cols, dp(href), dp(Ht), dp(Hj), dp(der))
            return Ht, Hj, der.reshape(ncell, 6)

        before = [evaluate(k) for k in range(ncalls)]
        im1[change_px] = 255.0 - im1[change_px]
        after = [evaluate(k) for k in range(ncalls)]
    finally:
        lib.nid_legacy_set_verify_mode(0)
        lib.nid_legacy_reset()
    followed_at = None
    for k in range(ncalls):
        Ht_b, Hj_b, der_b = before[k]
        Ht_a, Hj_a, der_a = after[k]
        assert not np.array_equal(_bits(Ht_a[act]), _bits(Ht_b[act])), "the changed pixel must matter to some cell"
        is_after = np.array_equal(_bits(rec[k, 0][act]), _bits(Ht_a[act]))
        is_before = np.array_equal(_bits(rec[k, 0][act]), _bits(Ht_b[act]))
        assert is_after or is_before, f"call {k}: neither the old nor the new target"
        if followed_at is None and is_after:
            followed_at = k
        want = (Ht_a, Hj_a, der_a) if is_after else (Ht_b, Hj_b, der_b)
        assert k >= change_at or is_before
        assert followed_at is None or is_after, f"call {k}: back on the old content"
        assert np.array_equal(_bits(rec[k, 1][act]), _bits(want[1][act]))
        if k % 4 == 0:
            assert np.array_equal(_bits(rec[k].reshape(-1)[2 * ncell:].reshape(ncell, 6)[act]), _bits(want[2][act]))
    assert followed_at is not None and change_at <= followed_at < change_at + SLICES, followed_at
    # ... and the oracle on the last call with a Jacobian (the changed target)
    k = ncalls - 4
    o = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix")
    o.compute_href(pair.pose_init)
    im1_changed = pair.im1.copy().reshape(-1); im1_changed[change_px] = 255 - im1_changed[change_px]
    o.set_target(im1_changed.reshape(pair.rows, pair.cols))
    Hc_o, Hj_o, _, J_o = o.evaluate(poses7[k], True)
    np.testing.assert_allclose(rec[k, 0][act], Hc_o[act], rtol=0, atol=1e-11)
    np.testing.assert_allclose(rec[k, 1][act], Hj_o[act], rtol=0, atol=1e-11)
    scale = np.abs(J_o[act]).max(axis=1, keepdims=True)
    assert np.all(np.abs(rec[k].reshape(-1)[2 * ncell:].reshape(ncell, 6)[act] - J_o[act]) <= 1e-9 * np.maximum(scale, 1e-6 * scale.max()))


def _compare_traces(recs, recs_o, pose, pose_o, synth):
    assert len(recs) == len(recs_o)
    for r, ro in zip(recs, recs_o):
        assert r["lm_trials"] == ro["lm_trials"], (r, ro)
        np.testing.assert_allclose(r["chi2"], ro["chi2"], rtol=1e-9)
        np.testing.assert_allclose(r["lambda_"], ro["lambda_"], rtol=1e-6)
    np.testing.assert_allclose(synth.pose7_minimal(pose), synth.pose7_minimal(pose_o), rtol=0, atol=1e-6)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("nb", [10, 8])
def test_lm_pose_parity_config_A(hostlib, oracle, synth, pair_A, nb, strict):
    pair = pair_A
    o = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix")
    o.compute_href(pair.pose_init)
    pose_o, recs_o = o.lm(pair.pose_init, 10)
    pose, recs, log = hostlib.run_lm(pair, nb, pair.pose_init, 10, strict=strict)
    assert "levenbergIter" in log
    _compare_traces(recs, recs_o, pose, pose_o, synth)
    # batch statistics (batch_stats.h): one timed entry per outer iteration
    assert all(0.0 < r["time_s"] < 1.0 for r in recs)
    # report how close the two really are (well inside the 1e-6 tolerance)
    d = np.abs(synth.pose7_minimal(pose) - synth.pose7_minimal(pose_o)).max()
    print(f"[{'STRICT' if strict else 'FAST'} nb={nb}] max |pose_gpu - pose_oracle| = {d:.3e}")
    assert d < 1e-8
    # and the optimisation did something: error vs ground truth went down
    e0 = np.linalg.norm(synth.pose7_minimal(pair.pose_true) - synth.pose7_minimal(pair.pose_init))
    e1 = np.linalg.norm(synth.pose7_minimal(pair.pose_true) - synth.pose7_minimal(pose))
    assert e1 < e0


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("nb", [8, 10])
def test_lm_pose_parity_flash_pair(hostlib, oracle, synth, nb, strict):
    """The data the path is meant for (BASELINE configs[0] is a FLASH pair): 640x480, a saturating hot spot over
    ~13 % of the second image, black / saturated patches, 5 % depth holes.  The reference driver's 10 LM
    iterations in FAST and STRICT math, per-edge flow and fused flow, against the oracle.

    Per-cell results agree like on any other data (entropies 1e-13, Jacobians 3e-10 of the cell's own scale:
    test_flash_pair_cells; the 6x6 system at the ORACLE's own LM poses to 1e-14: tools/diag_parity.py lmflash) --
    the saturation clamp is decided exactly like the reference decides it, in both modes.  What is different here is
    the reference's cost function itself: with thousands of samples sitting on the clamp, chi2(pose) is NOISY at the
    1e-8 level -- moving the pose by ONE ULP flips clamp decisions and changes the reference's own chi2 by up to
    9e-9 relative and its H, b by 1e-6 (tests/test_oracle_known_answers.py::test_reference_cost_is_noisy_on_saturated_data;
    nothing moves on the unsaturated pair).  Two faithful implementations whose 6x6 solves differ in the last bit
    therefore see different noise from the first trial pose on; the optimisation amplifies it by about a digit per
    iteration -- the reference does not even reproduce ITSELF: run with every cell's pixels in the opposite order
    (same arithmetic, other rounding of the sums) its 8-bin optimisation ends 4e-9 away and its 10-bin optimisation
    parts after six iterations and ends 6e-6 away (test_reference_lm_reproducibility_on_saturated_data).  What can
    be asked, and is: the same accept/reject trace up to a razor-edge decision, chi2 to 1e-5, and after
    every common iteration the pose within the stated 1e-6 or, where that is larger, within three times the
    reference's own forward / reversed deviation at that iteration (measured here, on the same pair).  The six GPU
    variants differ among themselves in the same way (tools/diag_lm_trace.py)."""
    pair = synth.make_pair("A", flash=True, edge_cases=True)
    o = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix")
    o.compute_href(pair.pose_init)
    pose_o, recs_o = o.lm(pair.pose_init, 10)
    # the reference's own reproducibility on this pair: the oracle with every cell's pixels visited in the opposite
    # order (tests/test_oracle_known_answers.py::test_reference_lm_reproducibility_on_saturated_data)
    o_rev = oracle.from_pair(pair, nb, jac_bound="cpu", xform="matrix", reversed_pixels=True)
    o_rev.compute_href(pair.pose_init)
    _, recs_rev = o_rev.lm(pair.pose_init, 10)

    def self_dev(i):   # how far the reference is from itself after iteration i (None once its two traces have parted)
        if i >= min(len(recs_o), len(recs_rev)) or any(recs_o[k]["lm_trials"] != recs_rev[k]["lm_trials"] for k in range(i + 1)):
            return None
        return float(np.abs(synth.pose7_minimal(recs_o[i]["pose7"]) - synth.pose7_minimal(recs_rev[i]["pose7"])).max())

    for fused in (0, 2):
        pose, recs, log = hostlib.run_lm(pair, nb, pair.pose_init, 10, strict=strict, fused=fused)
        # accept/reject decisions are occasionally taken on chi2 differences far below the agreement of
        # the two trajectories (here: iteration 0 amplifies the 1e-13 differences of H, b to ~1e-8 in chi2 -- lambda_0 is
        # tiny and seven trials are needed --, each iteration adds a digit, and from iteration 5 on lambda ~ 3e8 makes
        # every step improve chi2 by ~2e-6 relative only).  A trace that parts from the oracle's at such a razor-edge
        # decision is reported, not hidden, and everything is compared up to the last common iteration.  The six GPU
        # variants (FAST / STRICT x per-edge / fused / batched trials) differ among themselves in the same way
        # (tools/diag_lm_trace.py).
        common = 0
        while (common < min(len(recs), len(recs_o)) and recs[common]["lm_trials"] == recs_o[common]["lm_trials"]):
            common += 1
        if common < max(len(recs), len(recs_o)):
            i = min(common, len(recs_o) - 1)
            margin = abs(recs_o[i]["chi2"] - recs_o[i - 1]["chi2"]) / recs_o[i]["chi2"]
            print(f"[flash {'STRICT' if strict else 'FAST'} nb={nb} fused={fused}] traces part at iteration {common}: the oracle's "
                  f"decision there rests on a relative chi2 difference of {margin:.2e}")
            assert margin < 1e-5, "the traces part at a decision that is NOT a razor edge"
        assert common >= 5
        np.testing.assert_allclose([r["chi2"] for r in recs[:common]], [r["chi2"] for r in recs_o[:common]], rtol=1e-5)
        np.testing.assert_allclose([r["lambda_"] for r in recs[:common]], [r["lambda_"] for r in recs_o[:common]], rtol=1e-4)
        # pose: after every common iteration, within the stated 1e-6 -- or, where the reference does not reproduce ITSELF
        # to 1e-6 (its forward / reversed-order runs), within three times its own deviation
        worst = 0.0
        for i in range(common):
            sd = self_dev(i)
            if sd is None:         # the reference's own two runs have parted: nothing is defined beyond this iteration
                break
            d = float(np.abs(synth.pose7_minimal(recs[i]["pose7"]) - synth.pose7_minimal(recs_o[i]["pose7"])).max())
            assert d <= max(1e-6, 3.0 * sd), (i, d, sd)
            worst = max(worst, d)
        ends = float(np.abs(synth.pose7_minimal(recs_o[-1]["pose7"]) - synth.pose7_minimal(recs_rev[-1]["pose7"])).max())
        print(f"[flash {'STRICT' if strict else 'FAST'} nb={nb} fused={fused}] {common} common iterations, worst pose deviation "
              f"{worst:.3e}; the reference's own forward / reversed-order runs end {ends:.3e} apart")


def test_lm_fused_path_equals_per_edge_path(hostlib, synth, pair_A):
    pair, nb = pair_A, 10
    pose_a, recs_a, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=False)
    pose_b, recs_b, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=True)
    assert [r["lm_trials"] for r in recs_a] == [r["lm_trials"] for r in recs_b]
    np.testing.assert_allclose(synth.pose7_minimal(pose_a), synth.pose7_minimal(pose_b), rtol=0, atol=1e-8)
    # speculative batched trials: same decisions and, pose for pose, the same bits as the sequential fused path
    pose_c, recs_c, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=2)
    assert [r["lm_trials"] for r in recs_c] == [r["lm_trials"] for r in recs_b]
    assert [r["chi2"] for r in recs_c] == [r["chi2"] for r in recs_b]
    assert np.array_equal(pose_c, pose_b)
    # ... and with the first trials evaluated WITH their Jacobian (one launch per outer iteration): the accepted trial's
    # H, b and chi2 are the bits a fresh launch at that pose gives, so nothing changes
    pose_d, recs_d, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=3)
    assert [r["lm_trials"] for r in recs_d] == [r["lm_trials"] for r in recs_b]
    assert [r["chi2"] for r in recs_d] == [r["chi2"] for r in recs_b]
    assert np.array_equal(pose_d, pose_b)
    # fused 4: sequential trials, the first of every outer iteration with its Jacobian -- nothing but single-pose
    # evaluations; then the same, and the reference's per-edge flow, answered by the RESIDENT evaluator (a kernel that
    # stays on the device): the same bits again
    pose_e, recs_e, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=4)
    assert [r["chi2"] for r in recs_e] == [r["chi2"] for r in recs_b] and np.array_equal(pose_e, pose_b)
    hostlib.set_resident(True)
    try:
        pose_f, recs_f, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=4)
        assert [r["chi2"] for r in recs_f] == [r["chi2"] for r in recs_b] and np.array_equal(pose_f, pose_b)
        pose_g, recs_g, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=1)
        assert [r["chi2"] for r in recs_g] == [r["chi2"] for r in recs_b] and np.array_equal(pose_g, pose_b)
        pose_h, recs_h, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=False)
        assert [r["chi2"] for r in recs_h] == [r["chi2"] for r in recs_a] and np.array_equal(pose_h, pose_a)
        pose_i, recs_i, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=3)   # batched trials retire the kernel: still the same
        assert [r["chi2"] for r in recs_i] == [r["chi2"] for r in recs_b] and np.array_equal(pose_i, pose_b)
    finally:
        hostlib.set_resident(False)


@pytest.mark.parametrize("strict", [False, True])
def test_native_pair_setup_equals_the_legacy_operators_route(hostlib, synth, pair_A, pair_S_edge, strict):
    """the fused flows hand the frame pair over in the driver's own formats (u16 depth, u8 images;
    nid_legacy_set_pair_u16 -> nid_multi_set_pair_u16: back-projection, tiles, margins and the reference stage on the
    device, counts and Href back).  Same chi2 sequence and the same pose, BIT FOR BIT, as round 5's route through
    Calculate3Dpoint / CudaComputeHref (points and weights taken back to the host and uploaded again) -- plain pair, the
    edge-case pair (depth holes, saturated / black patches, an inactive cell), the pyramid, FAST and STRICT."""
    for pair, nb in ((pair_A, 8), (pair_S_edge, 10)):
        for fused in (1, 2, 4):
            pose_n, recs_n, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=fused, strict=strict)
            pose_l, recs_l, _ = hostlib.run_lm(pair, nb, pair.pose_init, 10, fused=fused, strict=strict, legacy_setup=True)
            assert [r["lm_trials"] for r in recs_n] == [r["lm_trials"] for r in recs_l]
            assert [r["chi2"] for r in recs_n] == [r["chi2"] for r in recs_l], (fused, nb)
            assert np.array_equal(_bits(pose_n), _bits(pose_l))
    # a legacy-route pair right behind a native one (and back): the operators' content keys were dropped, nothing stale
    pose_a, _, _ = hostlib.run_lm(pair_A, 8, pair_A.pose_init, 4, fused=0, strict=strict)
    pose_b, _, _ = hostlib.run_lm(pair_A, 8, pair_A.pose_init, 4, fused=2, strict=strict)
    pose_c, _, _ = hostlib.run_lm(pair_A, 8, pair_A.pose_init, 4, fused=0, strict=strict)
    assert np.array_equal(_bits(pose_a), _bits(pose_c))
    np.testing.assert_allclose(synth.pose7_minimal(pose_a), synth.pose7_minimal(pose_b), rtol=0, atol=1e-8)
    pose_p, per_p, _ = hostlib.run_pyramid_lm(pair_A, 8, pair_A.pose_init, levels=3, iterations=10, fused=2, strict=strict)
    pose_q, per_q, _ = hostlib.run_pyramid_lm(pair_A, 8, pair_A.pose_init, levels=3, iterations=10, fused=2, strict=strict, legacy_setup=True)
    assert [[r["chi2"] for r in lv] for lv in per_p] == [[r["chi2"] for r in lv] for lv in per_q]
    assert np.array_equal(_bits(pose_p), _bits(pose_q))


def test_pyramid_lm_pose_parity(hostlib, oracle, synth, pair_A):
    """Coarse-to-fine schedule (BASELINE configs[4]; own definition): 3 levels x 10 LM iterations on the
    C++ host stack + HIP kernels against the oracle's restatement of the same schedule: same accept/reject trace
    on every level, same pose to the 1e-6 tolerance of the north star."""
    pair, nb = pair_A, 8
    pose_o, per_o = oracle.pyramid_lm(pair, nb, pair.pose_init, levels=3, iterations=10)
    pose, per, log = hostlib.run_pyramid_lm(pair, nb, pair.pose_init, levels=3, iterations=10, fused=2)
    assert "pyramid level 2: 160x120, 4x4 cells" in log and "pyramid level 0: 640x480, 16x16 cells" in log
    assert [[r["lm_trials"] for r in lv] for lv in per] == [[r["lm_trials"] for r in lv] for lv in per_o]
    for lv, lv_o in zip(per, per_o):
        np.testing.assert_allclose([r["chi2"] for r in lv], [r["chi2"] for r in lv_o], rtol=1e-9)
    d = np.abs(synth.pose7_minimal(pose) - synth.pose7_minimal(pose_o)).max()
    print(f"pyramid: max |pose_gpu - pose_oracle| = {d:.3e}")
    assert d < 1e-8
    # the reference call schedule (per-edge walk) gives the same result as the fused path
    pose_r, per_r, _ = hostlib.run_pyramid_lm(pair, nb, pair.pose_init, levels=3, iterations=10, fused=0)
    np.testing.assert_allclose(synth.pose7_minimal(pose_r), synth.pose7_minimal(pose), rtol=0, atol=1e-8)
    # sizes that do not divide are refused
    with pytest.raises(RuntimeError):
        hostlib.run_pyramid_lm(pair, nb, pair.pose_init, levels=6, iterations=2)


def test_lm_cuda_bound_mode(hostlib, oracle, synth, pair_S):
    pair, nb = pair_S, 10
    o = oracle.from_pair(pair, nb, jac_bound="cuda", xform="matrix")
    o.compute_href(pair.pose_init)
    pose_o, recs_o = o.lm(pair.pose_init, 6)
    pose, recs, _ = hostlib.run_lm(pair, nb, pair.pose_init, 6, jac_bound_cuda=True)
    _compare_traces(recs, recs_o, pose, pose_o, synth)


def test_driver_end_to_end(hostlib, synth, pair_S, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["python", os.path.join(root, "tools", "make_dataset.py"), str(tmp_path), "S", "10"])
    exe = os.path.join(root, "nid-pose-estimation_amd", "nid_pose_estimation")
    r = subprocess.run([exe, str(tmp_path / "config.yaml")], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "the final error is" in r.stdout and "levenbergIter" in r.stderr
    row = open(tmp_path / "nid_error.csv").read().strip().split(",")
    err = np.array([float(x) for x in row[:6]])
    pose, recs, _ = hostlib.run_lm(pair_S, 10, pair_S.pose_init, 10)
    want = synth.pose7_minimal(pair_S.pose_true) - synth.pose7_minimal(pose)
    # the driver re-derives the start pose from groundtruth.txt (printed decimals), so only ~1e-9 agreement
    np.testing.assert_allclose(err, want, rtol=0, atol=1e-5)


def test_driver_on_shards(hostlib, synth, pair_S, tmp_path):
    """The driver's `devices:` key (cells sharded over a device list, here two shards on GPU 0) with the one-launch-
    per-iteration LM (`fused: 3`): the same nid_error.csv row as the single-context run to 1e-9."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "nid-pose-estimation_amd", "nid_pose_estimation")
    rows_out = []
    for extra in ("fused: 2\n", "fused: 3\ndevices: 0,0\n"):
        d = tmp_path / ("a" if not rows_out else "b")
        d.mkdir()
        subprocess.check_call(["python", os.path.join(root, "tools", "make_dataset.py"), str(d), "S", "10"])
        with open(d / "config.yaml", "a") as f:
            f.write(extra)
        r = subprocess.run([exe, str(d / "config.yaml")], capture_output=True, text=True, cwd=d, timeout=300)
        assert r.returncode == 0, r.stderr
        rows_out.append(np.array([float(x) for x in open(d / "nid_error.csv").read().strip().split(",")[:6]]))
    np.testing.assert_allclose(rows_out[0], rows_out[1], rtol=0, atol=1e-9)


def test_driver_reads_png_dataset(hostlib, synth, pair_S, tmp_path):
    """The driver on the ETH-CVG layout with PNG files (rgb/<id>.png, depth/<id>.png 16 bit): same result as
    with the PGM copies of the same pair."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "nid-pose-estimation_amd", "nid_pose_estimation")
    rows_out = []
    for fmt in ("png", "pgm"):
        d = tmp_path / fmt
        d.mkdir()
        subprocess.check_call(["python", os.path.join(root, "tools", "make_dataset.py"), str(d), "S", "10", fmt])
        assert (d / "rgb" / f"0000.{fmt}").exists() and not (d / "rgb" / ("0000.pgm" if fmt == "png" else "0000.png")).exists()
        r = subprocess.run([exe, str(d / "config.yaml")], capture_output=True, text=True, cwd=d, timeout=300)
        assert r.returncode == 0, r.stderr
        rows_out.append(open(d / "nid_error.csv").read().strip())
    assert rows_out[0] == rows_out[1]
    assert np.array_equal(hostlib.png_read_gray_u8(str(tmp_path / "png" / "rgb" / "0001.png")), pair_S.im1)
    assert np.array_equal(hostlib.png_read_u16(str(tmp_path / "png" / "depth" / "0000.png")), pair_S.depth_u16)


def test_driver_standard_property_mode(capi, synth, pair_S, tmp_path):
    """The reference's second program (NID_standard_property.cpp) as a driver mode: per-cell lines in its
    print format and "final nid is X" at the ground-truth relative pose."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["python", os.path.join(root, "tools", "make_dataset.py"), str(tmp_path), "S", "8"])
    with open(tmp_path / "config.yaml", "a") as f:
        f.write("mode: standard_property\n")
    exe = os.path.join(root, "nid-pose-estimation_amd", "nid_pose_estimation")
    r = subprocess.run([exe, str(tmp_path / "config.yaml")], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Href, current, joint from standard method is" in r.stdout
    final = float(re.search(r"final nid is ([0-9.eE+-]+)", r.stdout).group(1))
    ctx = capi.from_pair(pair_S, 8)
    want = ctx.plain_nid(pair_S.pose_true, 8)["total"]
    assert abs(final - want) < 1e-4 * max(1.0, want)   # %g print + pose re-derived from groundtruth.txt


def test_bench_plain_run_and_dumped_outputs(capi, synth, tmp_path):
    """bench.py without --full: one result line with the headline fields and none of the side measurements;
    --dump-outputs writes the timed region's result blocks (float64), the same bits from two processes, and the last
    step equals a synchronous evaluation of the last pose.  K <= 64 (the short-sequence form) dumps its K blocks too."""
    import json
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for name, steps, warmup in (("a", 300, 70), ("b", 300, 70), ("short", 20, 5)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                            str(warmup), "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(r.stdout.strip().splitlines()) == 1, r.stdout
        lines[name] = d = json.loads(r.stdout)
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "iterations/s" and d["dtype"] == "f64"
        assert abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-9 * 1e3
        assert not ({"roofline", "check", "cpu_baseline", "pose_error_vs_ref", "multi_gpu"} & set(d))
    sh = lines["short"]["short_sequence"]
    assert len(sh["us_per_shot"]) == 11 and "without_trailing_synchronisation_us_per_shot" not in sh
    names = ("reduced", "reduced_steps", "last_H", "last_b", "last_chi2", "last_n_active")
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype == np.float64 and np.array_equal(_bits(a), _bits(b)), n
    red = np.load(tmp_path / "a" / "reduced.npy")
    assert red.shape == (300, capi.NID_REDUCED_LEN) and np.array_equal(np.load(tmp_path / "a" / "reduced_steps.npy"), np.arange(300))
    assert np.load(tmp_path / "short" / "reduced.npy").shape == (20, capi.NID_REDUCED_LEN)
    pair = synth.make_pair("A")
    ctx = capi.from_pair(pair, 8)
    ctx.set_math_mode(capi.MATH_FAST)   # bench.py's default
    ctx.compute_href(pair.pose_init)
    last = bench.pose_trajectory(synth, pair, 256)[299 % 256]
    H, b, chi2, na = ctx.normal_equations(last, float(np.sqrt(0.95)))
    ctx.close()
    assert np.array_equal(np.load(tmp_path / "a" / "last_H.npy"), H) and np.array_equal(np.load(tmp_path / "a" / "last_b.npy"), b)
    assert np.load(tmp_path / "a" / "last_chi2.npy")[0] == chi2 and np.load(tmp_path / "a" / "last_n_active.npy")[0] == na
    Hp, bp, chi2p, nap = capi.unpack_reduced(red[-1])
    assert np.array_equal(Hp, H) and chi2p == chi2 and nap == na


def test_bench_multi_rank_code_path_on_one_gpu(tmp_path):
    """bench.py --gpus 2 / 4 through torch.distributed.run on ONE box: the ranks share GPU 0 (RCCL refuses two ranks
    per device), so the exchange goes through the library's exchange hook over gloo instead of ncclAllReduce --
    everything else is the multi-process path the driver runs on 8 GPUs: per-rank shard (nid_multi_create_rank),
    nid_multi_run_sequence, the pipelined == synchronous check inside bench.py; the sums must equal the 1-rank
    result.  --shards exercises the same C++ loop in one process with the host sum."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    bench = os.path.join(root, "bench.py")
    one = subprocess.run([sys.executable, bench, "--full", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--quick"],
                         capture_output=True, text=True, env=env, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    r1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert r1["scaling"] == "strong" and r1["n_gpus"] == 1
    sh = subprocess.run([sys.executable, bench, "--full", "--steps", "300", "--warmup", "70", "--no-cpu-baseline", "--shards", "3"],
                        capture_output=True, text=True, env=env, timeout=600)
    assert sh.returncode == 0, sh.stderr[-2000:]
    assert "3 shards" in json.loads(sh.stdout.strip().splitlines()[-1])["config"]["parallelism"]
    # the RCCL data path inside a process that has PyTorch (and its bundled ROCm libraries) loaded, as the driver's
    # multi-GPU runs have: communicator of one rank, ncclAllReduce from C++
    rc = subprocess.run([sys.executable, bench, "--full", "--steps", "300", "--warmup", "70", "--no-cpu-baseline", "--rccl-one-rank"],
                        capture_output=True, text=True, env=env, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert len(rc.stdout.strip().splitlines()) == 1, rc.stdout     # RCCL's own banner must not land on stdout
    rj = json.loads(rc.stdout.strip().splitlines()[-1])
    assert rj["rccl_ranks_seen"] == 1 and "RCCL" in rj["config"]["parallelism"]
    # RCCL that cannot be loaded (here: forced to a missing file): every rank notices, they agree -- and the job FAILS
    # with one error record instead of hanging in ncclCommInitRank or quietly measuring over gloo (round 4: a scaling
    # curve over the test transport must never read as the result; --backend gloo asks for it explicitly)
    nb_env = dict(env, NID_RCCL_LIBRARY="/nonexistent/librccl.so")
    fb = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                         "--master-addr", "127.0.0.1", "--master-port", "29516", bench, "--gpus", "2", "--no-cpu-baseline",
                         "--quick", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, env=nb_env, timeout=900)
    assert fb.returncode != 0, fb.stdout[-2000:]
    rf = json.loads([l for l in fb.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert rf["value"] is None and "RCCL" in rf["error"] and rf["n_gpus"] == 2 and rf["rccl_ranks_seen"] == 0
    # ... and a communicator RCCL refuses (two ranks on ONE device: ncclCommInitRank fails on both): same agreement.
    # Started the way the driver starts its N = 1 leg -- plain `python bench.py --gpus 2`, no launcher: bench.py starts
    # the two ranks itself (a child torch.distributed.run, before this process touches the GPU) and relays the record
    # and the exit code; it can no longer run one process and print n_gpus 1.
    env_plain = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dup = subprocess.run([sys.executable, bench, "--gpus", "2", "--no-cpu-baseline", "--quick", "--steps", "20", "--warmup", "5"],
                         capture_output=True, text=True, env=env_plain, timeout=900)
    assert dup.returncode != 0, dup.stdout[-2000:]
    assert len(dup.stdout.strip().splitlines()) == 1, dup.stdout
    rd = json.loads(dup.stdout.strip())
    assert rd["value"] is None and "ncclCommInitRank" in rd["error"] and rd["n_gpus"] == 2
    # the same plain invocation with the test transport asked for: a result line with n_gpus 2
    own = subprocess.run([sys.executable, bench, "--gpus", "2", "--full", "--no-cpu-baseline", "--quick", "--steps", "20", "--warmup", "5",
                          "--backend", "gloo"], capture_output=True, text=True, env=env_plain, timeout=900)
    assert own.returncode == 0, own.stderr[-3000:]
    assert len(own.stdout.strip().splitlines()) == 1, own.stdout
    ro = json.loads(own.stdout.strip())
    assert ro["n_gpus"] == 2 and ro["rccl_ranks_seen"] == 0 and "gloo" in ro["exchange"] and ro["value"] > 0
    assert "(interleaved)" in ro["config"]["parallelism"] and ro["multi_gpu"]["launches_per_exchange"] == 2   # the defaults
    # ... and the ranks it starts get EVERY flag as given (spawn_ranks forwards sys.argv[1:]): partition and group size
    fwd = subprocess.run([sys.executable, bench, "--gpus", "2", "--full", "--no-cpu-baseline", "--quick", "--steps", "300", "--warmup", "70",
                          "--backend", "gloo", "--partition", "contiguous", "--group", "3", "--batch", "16"],
                         capture_output=True, text=True, env=env_plain, timeout=900)
    assert fwd.returncode == 0, fwd.stderr[-3000:]
    rw = json.loads(fwd.stdout.strip())
    assert rw["n_gpus"] == 2 and "(contiguous)" in rw["config"]["parallelism"]
    assert rw["multi_gpu"]["launches_per_exchange"] == 3 and rw["multi_gpu"]["poses_per_launch"] == 16
    # a launcher that started another number of ranks than --gpus says is refused
    bad = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29515", bench, "--gpus", "4", "--no-cpu-baseline",
                          "--quick", "--steps", "20", "--warmup", "5", "--backend", "gloo"], capture_output=True, text=True, env=env, timeout=900)
    assert bad.returncode != 0
    for port, world, extra in ((29517, 2, ["--steps", "20", "--warmup", "5"]),
                               (29518, 2, ["--steps", "300", "--warmup", "70"]),
                               (29519, 2, ["--steps", "300", "--warmup", "70", "--group", "8", "--batch", "16"]),
                               (29520, 4, ["--steps", "700", "--warmup", "70"])):
        two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                              "--master-addr", "127.0.0.1", "--master-port", str(port), bench,
                              "--gpus", str(world), "--full", "--no-cpu-baseline", "--backend", "gloo"] + extra,
                             capture_output=True, text=True, env=env, timeout=900)
        assert two.returncode == 0, two.stderr[-3000:]
        line = [l for l in two.stdout.strip().splitlines() if l.startswith("{")][-1]
        r2 = json.loads(line)
        assert r2["n_gpus"] == world and r2["scaling"] == "strong"
        # what a flat scaling curve would be attributed with: every rank's kernel time, the exchange by itself
        mg = r2["multi_gpu"]
        assert len(mg["per_rank_kernel_ms"]) == world and all(t > 0 for t in mg["per_rank_kernel_ms"]) and mg["exchange_ms_per_group"] > 0
        assert r2["rccl_ranks_seen"] == 0   # (--backend gloo: the exchange does not go through RCCL)
        if extra[1] == "20":     # same last pose as the 1-rank run: the exchanged sums must agree
            assert r2["check"]["n_active"] == r1["check"]["n_active"]
            for k in ("chi2", "H00", "b0"):
                assert abs(r2["check"][k] - r1["check"][k]) <= 1e-12 * abs(r1["check"][k]), k
