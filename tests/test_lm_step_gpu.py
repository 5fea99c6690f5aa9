"""k_lm_step (the device compilation of lm::lm_step, csrc/nid_lm_step.h) against the host compilation on the corpus of
tests/lm_step_cases.py: every pair, every field of the state, the trace record, the pose record and the running word,
compared as bytes.  tests/test_lm_step_cpu.py asserts what the corpus reaches.

The one allowance: a double that is NaN on both sides passes whatever its sign and payload are -- IEEE fixes neither for
a NaN that arithmetic produced -- but only in the categories built to make NaNs (lm_step_cases.NAN_CATEGORIES); everywhere else the cap
on such fields is zero.  The count is printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_step_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cp(capi):
    return L.corpus(capi)


@pytest.fixture(scope="module")
def ctx(capi, pair_S):
    """a context with NO pair set: the seam needs none"""
    c = capi.Context(pair_S.rows, pair_S.cols, pair_S.cell, 8, pair_S.fx, pair_S.fy, pair_S.cx, pair_S.cy)
    yield c
    c.close()


NAN_EXAMPLES = {}  # field -> (category, device bits, host bits) of one field equal only as NaNs


def _compare(dev, ref, dtype, cats, nan_ok, what):
    """dev, ref: record arrays of one dtype.  Bytes equal, or a double NaN on both sides where nan_ok.  -> NaN-only fields"""
    nan_only = np.zeros(len(ref), dtype=np.int64)
    for name in dtype.names:
        d, r = dev[name].reshape(len(ref), -1), ref[name].reshape(len(ref), -1)
        if dtype[name].base == np.float64:
            same = d.view(np.uint64) == r.view(np.uint64)
            both_nan = ~same & np.isnan(d) & np.isnan(r)
            bad = ~same & ~both_nan
            nan_only += both_nan.sum(axis=1)
            if both_nan.any() and name not in NAN_EXAMPLES:
                i, j = np.argwhere(both_nan)[0]
                NAN_EXAMPLES[name] = (cats[i], hex(int(d.view(np.uint64)[i, j])), hex(int(r.view(np.uint64)[i, j])))
        else:
            bad = d != r
        if bad.any():
            k = int(np.flatnonzero(bad.any(axis=1))[0])
            by_cat = sorted({cats[i] for i in np.flatnonzero(bad.any(axis=1))})
            raise AssertionError(f"{what}.{name}: {int(bad.any(axis=1).sum())} pairs differ, categories {by_cat}; first pair {k} "
                                 f"({cats[k]}): device {d[k].tolist()} host {r[k].tolist()}")
    outside = np.flatnonzero((nan_only > 0) & ~nan_ok)
    assert len(outside) == 0, f"{what}: NaNs of different bits outside the NaN categories: pairs {outside[:8].tolist()} ({sorted({cats[i] for i in outside})})"
    return nan_only


REC_DTYPE = np.dtype([("q", "f8", 7), ("M", "f8", 12)])


def _launch_and_check(capi, ctx, cp, n):
    states = cp.states(n)
    rec19, mode = L.sentinel_records(n)
    word, trace = capi.lm_step_device(states, cp.blocks[:n], ctx, rec19, mode, trace=True)
    dev = np.frombuffer(bytes(memoryview(states)), dtype=L.STATE_DTYPE)
    ref = cp.after[:n]
    cats, nan_ok = cp.cats[:n], cp.nan_ok[:n]
    total = _compare(dev, ref, L.STATE_DTYPE, cats, nan_ok, "state")
    # frozen states: byte for byte what went in
    frozen = np.flatnonzero(cp.before["status"][:n] != 0)
    assert all(dev[k].tobytes() == cp.before[k].tobytes() for k in frozen), "a finished chain's state changed"
    # the trace record: lm_trace of the state behind the step (a finished chain repeats its state's)
    want = np.zeros(n, dtype=capi.MS_TRACE_DTYPE)
    for f, g in (("trial_chi2", "trial_chi2"), ("lambda_", "lambda_"), ("rho", "rho"), ("pose7", "pose7"), ("flags", "flags"), ("status", "status")):
        want[f] = ref[g]
    total += _compare(trace, want, capi.MS_TRACE_DTYPE, cats, nan_ok, "trace")
    # the pose record: a running chain's is rec_q / rec_M / rec_mode, any other keeps the sentinel it was handed
    want19, want_mode = L.expected_records(cp, n)
    total += _compare(rec19.view(REC_DTYPE).reshape(n), want19.view(REC_DTYPE).reshape(n), REC_DTYPE, cats, nan_ok, "record")
    assert (mode == want_mode).all(), f"record modes differ at {np.flatnonzero(mode != want_mode)[:8].tolist()}"
    s19, smode = L.sentinel_records(n)
    idle = ~cp.running[:n]
    assert rec19[idle].tobytes() == s19[idle].tobytes() and (mode[idle] == smode[idle]).all(), "a finished chain's record was written"
    assert word == int(cp.running[:n].sum()), f"running word {word}, host count {int(cp.running[:n].sum())}"
    return total


@pytest.mark.parametrize("n", [None, 1, 64, 65])
def test_device_step_equals_host_step_on_every_pair(capi, ctx, cp, n):
    n = cp.n if n is None else n
    nan_only = _launch_and_check(capi, ctx, cp, n)
    by_cat = {}
    for k in np.flatnonzero(nan_only):
        by_cat[cp.cats[k]] = by_cat.get(cp.cats[k], 0) + int(nan_only[k])
    print({k: v for k, v in sorted(NAN_EXAMPLES.items())})
    print(f"n = {n}: {int(nan_only.sum())} fields equal only as NaNs (of {int(cp.nan_ok[:n].sum())} pairs in the NaN categories): {by_cat}")
    if n == cp.n:
        assert int(cp.running.sum()) > 2000 and int((~cp.running).sum()) > 50


def test_the_seam_leaves_the_context_usable_and_refuses_bad_counts(capi, ctx, cp):
    """an error that is not a state error: n = 0 and n = 65537 raise, and the context still steps afterwards"""
    for n in (0, 65537):
        states = (capi.MsState * n)()
        rec19, mode = L.sentinel_records(max(n, 1))
        with pytest.raises(capi.NidError, match="invalid"):
            capi.lm_step_device(states, np.zeros((n, 32)), ctx, rec19[:n].copy(), mode[:n].copy())
    _launch_and_check(capi, ctx, cp, 3)
    # without a trace the rest is the same
    states = cp.states(65)
    rec19, mode = L.sentinel_records(65)
    word, trace = capi.lm_step_device(states, cp.blocks[:65], ctx, rec19, mode, trace=False)
    assert trace is None and word == int(cp.running[:65].sum())
    _compare(np.frombuffer(bytes(memoryview(states)), dtype=L.STATE_DTYPE), cp.after[:65], L.STATE_DTYPE, cp.cats[:65], cp.nan_ok[:65], "state")
