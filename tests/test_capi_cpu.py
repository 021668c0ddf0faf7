"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports exactly the symbols that
include/orbslam3_hip.h declares (no compute calls without a GPU), the test-only host library links it rather than
copying it, and the C-ABI fails loudly without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from orb_slam3_study_kr_amd import capi

ROOT = Path(__file__).resolve().parent.parent


def _declared_symbols(header="orbslam3_hip.h"):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(osh_[a-z0-9_]+)\s*\(", text)))


def _readelf(*args):
    exe = shutil.which("readelf") or next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/llvm/bin/llvm-readelf")
                                           if os.access(p, os.X_OK)), None)
    assert exe, "neither readelf nor ROCm's llvm-readelf found"
    return subprocess.run([exe, "-W", *args], check=True, capture_output=True, text=True).stdout


def _defined_dynamic_symbols(lib_path):
    """Names of the defined non-local symbols of the dynamic symbol table."""
    names = set()
    for line in _readelf("--dyn-syms", str(lib_path)).splitlines():
        f = line.split()   # Num: Value Size Type Bind Vis Ndx Name
        if len(f) >= 8 and f[0].rstrip(":").isdigit() and f[4] != "LOCAL" and f[6] != "UND":
            names.add(f[7].split("@")[0])
    return names


def test_header_and_ctypes_mirror_agree():
    declared = _declared_symbols()
    assert declared, "no declarations parsed"
    assert sorted(capi.EXPORTED_SYMBOLS) == declared


def test_library_exports_every_declared_symbol():
    lib = capi.load_library()
    for name in _declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/orbslam3_hip.h but not exported"
    assert b"gfx950" in lib.osh_version()


def test_kernel_library_exports_exactly_the_c_abi():
    # no ORB_SLAM3:: C++ (the drop-in host sources belong to the integrator's library) and no osh_host_ test wrappers
    capi.load_library()
    assert sorted(_defined_dynamic_symbols(capi.LIB_PATH)) == _declared_symbols()


def test_host_library_defines_its_header_and_needs_the_kernel_library():
    capi.load_host_library()
    missing = set(_declared_symbols("orbslam3_hip_host.h")) - _defined_dynamic_symbols(capi.HOST_LIB_PATH)
    assert not missing, sorted(missing)
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", _readelf("-d", str(capi.HOST_LIB_PATH)))
    assert "liborbslam3_hip.so" in needed, needed


def test_both_loaders_share_one_kernel_library():
    # one copy of the kernel library in the process: one thread-local osh_last_error text for both handles
    def addr(lib):
        return C.cast(lib.osh_last_error, C.c_void_p).value
    assert addr(capi.load_host_library()) == addr(capi.load_library())


def test_kernel_library_override_serves_the_host_library(tmp_path):
    # ORBSLAM3_HIP_LIB loads a kernel library from elsewhere; its soname satisfies the host library's dependency
    alt = tmp_path / "liborbslam3_hip.so"
    shutil.copy(capi.LIB_PATH, alt)
    code = ("import ctypes as C\n"
            "from orb_slam3_study_kr_amd import capi\n"
            "a = C.cast(capi.load_library().osh_last_error, C.c_void_p).value\n"
            "b = C.cast(capi.load_host_library().osh_last_error, C.c_void_p).value\n"
            "maps = {l.split()[-1] for l in open('/proc/self/maps') if l.rstrip().endswith('liborbslam3_hip.so')}\n"
            "print(a == b, sorted(maps))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ORBSLAM3_HIP_LIB=str(alt)),
                         check=True, capture_output=True, text=True).stdout
    assert out.strip() == f"True {[str(alt)]}", out


def test_host_folder_is_the_integration_source_list():
    # csrc/host/ holds exactly the .cc files INTEGRATION.md section 2 tells an integrator to compile; test doubles live elsewhere
    snippet = re.search(r"```cmake\n(.*?)```", (ROOT / "INTEGRATION.md").read_text(), flags=re.S).group(1)
    listed = sorted(set(re.findall(r"csrc/host/(\w+\.cc)", snippet)))
    assert listed and listed == sorted(p.name for p in (ROOT / "orb_slam3_study_kr_amd" / "csrc" / "host").glob("*.cc"))


def test_struct_sizes_match_header_layout():
    # 4 ints + 8 pointers + 3 doubles + int (+pad) + 4 pointers (stop_flag, kb8, cam2, trl)
    assert C.sizeof(capi.LbaProblem) == 16 + 8 * 8 + 24 + 8 + 32
    assert C.sizeof(capi.LbaResult) == 4 * 8 + 16 + 128 * 8 * 2 + 128 * 4 + 8
    assert C.sizeof(capi.OrbBatch) == 16 + 6 * 8


def test_no_device_fails_loudly_not_silently():
    lib = capi.load_library()
    if lib.osh_device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the no-GPU container")
    ctx = C.c_void_p()
    rc = lib.osh_lba_create(0, C.byref(ctx))
    assert rc == capi.OSH_ERR_NO_DEVICE and not ctx
    assert "device" in capi.last_error(lib).lower()
    rc = lib.osh_orb_create(0, C.byref(ctx))
    assert rc == capi.OSH_ERR_NO_DEVICE


def test_product_package_never_imports_the_oracle():
    for py in (ROOT / "orb_slam3_study_kr_amd").rglob("*.py"):
        src = py.read_text()
        assert "import oracle" not in src and "from oracle" not in src, py
    for src in (ROOT / "orb_slam3_study_kr_amd" / "csrc").rglob("*"):
        if src.suffix in (".hip", ".cpp", ".cc", ".h"):
            assert "oracle" not in src.read_text().lower().replace("oracle/", "ORACLEDIR"), src
