"""Build and run one stand-alone ASan + UBSan program of the host tests (its own
main, no Python loading): one g++ per source in parallel, link, run, and scan
what it wrote.  Shared by the test_wire_*_host.py files; each keeps its own
source list and its own assertions on the program's output.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "cleisthenes_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-Wall"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build_and_run(tmp_path, name, cpp=(), csrc=(), headers=("hip/hip_runtime_api.h", "rccl/rccl.h")) -> str:
    """tests/cpp/<cpp...> and csrc/<csrc...> -> tmp_path/<name>, run under ENV; returns its stdout.
    Skips without g++ or the ROCm headers (types only: the programs link no ROCm library)."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    for h in headers:
        if not os.path.exists(os.path.join("/opt/rocm/include", h)):
            pytest.skip(f"/opt/rocm/include/{h} not available")
    exe = str(tmp_path / name)
    srcs = [os.path.join(CPP, f) for f in cpp] + [os.path.join(CSRC, f) for f in csrc]
    objs, procs = [], []
    for s in srcs:  # one compiler per file: capi.cpp alone takes most of the time
        objs.append(str(tmp_path / (os.path.basename(s) + ".o")))
        procs.append(subprocess.Popen(["g++", *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", s, "-o",
                                       objs[-1]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for s, p in zip(srcs, procs):
        out, _ = p.communicate()
        assert p.returncode == 0, f"{s}:\n{out}"
    r = subprocess.run(["g++", *SAN, "-o", exe, *objs, "-ldl", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for bad in ("AddressSanitizer", "runtime error", "FAIL"):
        assert bad not in r.stderr, r.stderr[-4000:]
    return r.stdout
