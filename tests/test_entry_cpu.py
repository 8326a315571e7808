"""The error contract of the C boundary (include/mckpp_hip.h: 0 on success, <0 and a text on error; no C++ exception
leaves the library, every text begins with the function's name), held in one place: `entry` of
mckpp_f90_amd/csrc/mckpp_own.h.  Every entry point that takes a handle refuses a null one by its own name; the text of
that refusal is written once; and the guard itself - with for_columns and the owner of a half-built object - is run on
its own, in a host program built with the address and undefined-behaviour sanitizers (tests/entry_guard_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

from harness import api  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mckpp_f90_amd", "csrc")

# The functions of an int result and a handle that do not report through it: what they return for a null handle, and
# whether they leave a text.  (c_int32 is c_int: the two counts are in the sweep's reach and are named here.)
NOT_AN_ERROR_CODE = (
    ("mckpp_hip_finalize", 0),             # finalizing nothing is no error
    ("mckpp_hip_multi_finalize", 0),
    ("mckpp_hip_last_launch_count", 0),    # a count: int32_t in the header
    ("mckpp_hip_multi_ndev", -1),          # a count, -1 for no handle: int32_t in the header
)


def null_for(t):
    return 0.0 if t is C.c_double else 0 if t in (C.c_int, C.c_int32, C.c_int64, C.c_uint32) else None


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    lib = api._lib()
    swept = 0
    for name, (res, argtypes) in {**api._signatures(), **api._signatures_device()}.items():
        if res is not C.c_int or not argtypes or argtypes[0] is not api._H:
            continue
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        before = lib.mckpp_hip_last_error()
        rc = getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]])
        if name in dict(NOT_AN_ERROR_CODE):
            assert rc == dict(NOT_AN_ERROR_CODE)[name], name
            assert lib.mckpp_hip_last_error() == before, name
            continue
        assert rc == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept += 1
    assert swept >= 100, swept   # (the tables hold 52 such functions and their multi twins)
    assert {n for n, _ in NOT_AN_ERROR_CODE} <= set(api._signatures())


def test_the_null_handle_text_is_stated_once():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".cpp", ".hip")) or f == "Makefile":
            src = open(os.path.join(CSRC, f)).read()
            hits += [f] * src.count("null handle")
    assert hits == ["mckpp_own.h"], hits


def test_the_guard_on_its_own_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "entry_guard")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + CSRC, "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "entry_guard_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checks hold" in r.stdout, r.stdout + r.stderr
