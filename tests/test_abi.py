"""The C-ABI library loads without a GPU and exports every symbol that
include/nid/nid_c.h declares; argument validation works without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "nid", "nid_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nid_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported(capi):
    lib = capi.load()
    declared = _declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nid_c.h but not exported"
    assert sorted(capi.SYMBOLS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nid_[a-z0-9_]+)", nm))
    assert set(declared) <= exported


def test_abi_version_and_strings(capi):
    lib = capi.load()
    assert lib.nid_abi_version() == 4
    assert lib.nid_status_string(0) == b"ok"
    assert b"invalid" in lib.nid_status_string(-1)


def test_create_rejects_bad_config_without_touching_a_gpu(capi):
    lib = capi.load()
    h = C.c_void_p()
    bad = capi.NidConfig(480, 640, 16, 10, 2, 0, 0, 0, 1.0, 1.0, 0.0, 0.0)      # degree != 3
    assert lib.nid_create(C.byref(bad), C.byref(h)) == -1
    bad = capi.NidConfig(480, 640, 16, 40, 3, 0, 0, 0, 1.0, 1.0, 0.0, 0.0)      # too many bins
    assert lib.nid_create(C.byref(bad), C.byref(h)) == -1
    bad = capi.NidConfig(480, 640, 16, 10, 3, 0, 200, 100, 1.0, 1.0, 0.0, 0.0)  # empty shard
    assert lib.nid_create(C.byref(bad), C.byref(h)) == -1
    assert lib.nid_create(None, C.byref(h)) == -1


def test_no_device_fails_loudly(capi):
    lib = capi.load()
    if lib.nid_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    ok = capi.NidConfig(480, 640, 16, 10, 3, 0, 0, 0, 481.2, -480.0, 319.5, 239.5)
    assert lib.nid_create(C.byref(ok), C.byref(h)) == -2   # NID_ERR_NO_DEVICE, no CPU fallback
    with pytest.raises(capi.NidError):
        capi.Context(480, 640, 16, 10, 481.2, -480.0, 319.5, 239.5)


def test_unpack_reduced_layout(capi):
    r = np.zeros(32)
    r[0] = 3.5
    r[1:7] = np.arange(1, 7)
    r[7:28] = np.arange(21) + 10
    r[28] = 17
    H, b, chi2, na = capi.unpack_reduced(r)
    assert chi2 == 3.5 and na == 17
    assert np.array_equal(b, np.arange(1, 7))
    assert np.array_equal(H, H.T)
    assert H[0, 0] == 10 and H[0, 5] == 15 and H[1, 1] == 16 and H[5, 5] == 30


def test_f64_image_conversion(capi):
    lib = capi.load()
    src = np.array([0.0, 1.0, 254.0, 255.0])
    out = np.zeros(4, dtype=np.uint8)
    assert lib.nid_set_reference_image_f64(src.ctypes.data_as(capi.c_dp), 4, out.ctypes.data_as(capi.c_u8p)) == 0
    assert list(out) == [0, 1, 254, 255]
    src = np.array([0.5])
    assert lib.nid_set_reference_image_f64(src.ctypes.data_as(capi.c_dp), 1, out.ctypes.data_as(capi.c_u8p)) == -4


def _declared_in(header):
    txt = open(os.path.join(ROOT, "include", "nid", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nid_[a-z0-9_]+)\s*\(", txt)))


def test_multi_header_symbols_are_exported(capi):
    """include/nid/nid_multi.h: the multi-GPU layer is part of the same library, every symbol exported; the RCCL
    library itself is NOT a load-time dependency (dlopen on first use: a single-GPU process never pays for it)."""
    lib = capi._load_multi()
    declared = _declared_in("nid_multi.h")
    assert len(declared) >= 30 and sorted(capi.MULTI_SYMBOLS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nid_[a-z0-9_]+)", nm))
    assert set(declared) <= exported
    needed = subprocess.run(["readelf", "-d", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "rccl" not in needed.lower()


def test_multi_cell_ranges_and_argument_checks(capi):
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import parallel_helpers as parallel   # tests/parallel_helpers.py: the numpy restatement of the cell ranges
    for ncell in (16, 64, 256, 1024, 250):
        for n in (1, 2, 3, 4, 8):
            rs = [capi.cell_range(k, n, ncell) for k in range(n)]
            assert rs == parallel.all_ranges(n, ncell)
    with pytest.raises(capi.NidError):
        capi.cell_range(0, 17, 16)          # more shards than cells
    lib = capi._load_multi()
    h = C.c_void_p()
    cfg = capi.NidConfig(480, 640, 16, 10, 3, 0, 0, 0, 481.2, -480.0, 319.5, 239.5)
    dv = np.zeros(2, dtype=np.int32)
    assert lib.nid_multi_create(C.byref(cfg), dv.ctypes.data_as(capi.c_ip), 0, C.byref(h)) == -1
    assert lib.nid_multi_create(C.byref(cfg), None, 2, C.byref(h)) == -1
    assert lib.nid_multi_create_rank(C.byref(cfg), 0, 3, 2, C.byref(h)) == -1   # rank >= world
    if lib.nid_device_count() == 0:
        assert lib.nid_multi_create(C.byref(cfg), dv.ctypes.data_as(capi.c_ip), 2, C.byref(h)) == -2   # no CPU fallback


def test_unit_flags_reach_only_the_throughput_unit():
    """csrc/UNIT_FLAGS (round 6): the machine scheduler's max-ilp strategy goes to the 128-thread cost + Jacobian unit and to no
    other -- the latency units measure slower with it (profiles/r06_sched_strategy_ab.txt).  That unit also builds the
    Jacobian kind's k_repair<256>, behind the 128- and the 256-thread launches (nid_eval_launch.h).  build() and the variant /
    register tools parse the file with the same function."""
    import importlib
    import os
    entry = importlib.import_module("__graft_entry__")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nid-pose-estimation_amd", "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert "nid_eval_nt128_jac.hip" in units and len(units) >= 10
    flagged = {u: entry._unit_flags(u) for u in units}
    assert flagged["nid_eval_nt128_jac.hip"] == ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
    assert all(not f for u, f in flagged.items() if u != "nid_eval_nt128_jac.hip"), flagged
    launch_h = open(os.path.join(csrc, "nid_eval_launch.h")).read()
    assert "constexpr int kRepairThreads = 256;" in launch_h
    assert "#if NID_TU_NT == 128\n" in open(os.path.join(csrc, "nid_eval_tu.inc")).read()  # the unit that builds k_repair<256>
    for tool in ("build_variant.py", "kernel_regs.py"):
        assert "from __graft_entry__ import _unit_flags" in open(os.path.join(os.path.dirname(csrc), "..", "tools", tool)).read()


def _code_object_kernels(lib_path, tmp_path):
    """the kernels of every gfx950 code object in the library's .hip_fatbin section: one list per offload bundle (one per
    translation unit with device code)"""
    import struct
    llvm = "/opt/rocm/llvm/bin"
    fat = tmp_path / "fatbin"
    subprocess.check_call([f"{llvm}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, str(fat)])
    data = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, start = [], data.find(magic)
    while start >= 0:
        (count,) = struct.unpack_from("<Q", data, start + len(magic))
        pos, end = start + len(magic) + 8, start + len(magic) + 8
        for _ in range(count):
            off, size, id_len = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24:pos + 24 + id_len].decode()
            pos += 24 + id_len
            end = max(end, start + off + size)
            if triple.endswith("gfx950"):
                co = tmp_path / f"co{len(out)}"
                co.write_bytes(data[start + off:start + off + size])
                syms = subprocess.run([f"{llvm}/llvm-readelf", "-sW", str(co)], capture_output=True, text=True, check=True).stdout
                out.append(sorted(set(re.findall(r"(\S+)\.kd$", syms, re.M))))
        start = data.find(magic, end)
    return out


def test_every_kernel_is_built_in_one_unit(capi, tmp_path):
    """Two code objects that define the same kernel register it twice, and the HIP runtime serves one copy to every launch --
    which one, the order of the modules decides.  The copies can differ (csrc/UNIT_FLAGS), so each kernel is compiled in
    exactly one translation unit."""
    units = _code_object_kernels(capi.LIB_PATH, tmp_path)
    assert len(units) >= 10 and all(units), [len(u) for u in units]
    seen = {}
    for i, kernels in enumerate(units):
        for k in kernels:
            seen.setdefault(k, []).append(i)
    twice = sorted(k for k, where in seen.items() if len(where) > 1)
    assert not twice, f"{len(twice)} kernels in two code objects: {twice[:4]}"
