"""Host side of the parity-only shard commit, no GPU: two stand-alone programs
(their own main, no Python loading) built with ASan + UBSan.

* tests/cpp/split_rows_check.cpp -- from csrc/host_shared.h alone: the body of
  rbc_split_rows over k in {1, 2, 13, 44, 86}, every len in [1, 3k + 2] and a
  few large lengths, against a plain padded copy (klauspost Split): row
  pointers, tail bytes, tail_used, a tail of exactly rbc_split_tail_bytes is
  enough and one byte less is rejected.
* tests/cpp/parity_args_check.cpp -- csrc/capi.cpp linked with the unchanged
  host-memory HIP stand-in tests/cpp/hip_stub.cpp: the new entry points called
  with invalid arguments (NULL pointers, len == 0, pitch below Smax, too small a
  parity_cap, count == 0) return the documented status before any launcher.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SAN = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-Wall"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _build_and_run(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", *SAN, "-o", exe, os.path.join(CPP, name + ".cpp"), *extra],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for bad in ("AddressSanitizer", "runtime error", "FAIL"):
        assert bad not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout
    return r.stdout


def test_split_rows_matches_a_padded_copy_under_asan_ubsan(tmp_path):
    out = _build_and_run(tmp_path, "split_rows_check", [])
    # k in {1, 2, 13, 44, 86}: sum(3k + 2) + 6 large lengths each
    assert out.split()[1] == str(sum(3 * k + 2 + 6 for k in (1, 2, 13, 44, 86)))


def test_parity_entry_points_reject_invalid_arguments_before_any_launch(tmp_path):
    for h in ("hip/hip_runtime_api.h", "rccl/rccl.h"):  # capi.cpp's own includes (types only: hip_stub links)
        if not os.path.exists(os.path.join("/opt/rocm/include", h)):
            pytest.skip(f"/opt/rocm/include/{h} not available")
    _build_and_run(tmp_path, "parity_args_check",
                   ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(CPP, "hip_stub.cpp"),
                    os.path.join(ROOT, "cleisthenes_amd", "csrc", "capi.cpp"), "-ldl", "-lpthread"])


def test_header_announces_the_parity_only_commit_and_the_library_exports_it():
    from cleisthenes_amd import _lib
    assert "#define RBC_HAS_SHARD_COMMIT_PARITY 1" in open(_lib.HEADER_PATH).read()
    names = _lib.header_functions(_lib.HEADER_PATH)
    for fn in ("rbc_dev_shard_commit_parity", "rbc_shard_commit_parity", "rbc_shard_parity", "rbc_split_rows",
               "rbc_split_tail_bytes"):
        assert fn in names and hasattr(_lib.lib, fn), fn
    assert _lib.lib.rbc_abi_version() == 7  # additions are detected by symbol presence


def test_python_split_rows_aliases_the_value():
    """The binding's split_rows: whole rows are views of the value itself (a
    write through the value shows in the row), the padded rows hold the zero pad."""
    import numpy as np

    import cleisthenes_amd as ca
    for k, length in ((2, 1), (13, 14), (44, 44 * 600 + 7), (86, 86 * 3), (5, 11)):
        v = (np.arange(length, dtype=np.uint32) % 251 + 1).astype(np.uint8)
        S = (length + k - 1) // k
        padded = np.zeros(k * S, np.uint8)
        padded[:length] = v
        rows = ca.split_rows(k, v)
        assert len(rows) == k and all(len(r) == S for r in rows)
        assert all(np.array_equal(rows[j], padded[j * S:(j + 1) * S]) for j in range(k))
        for j in range(k):
            inside = (j + 1) * S <= length
            assert np.shares_memory(rows[j], v) == inside, (k, length, j)
    with pytest.raises(ca.RBCError) as e:
        ca.split_rows(3, b"")
    assert e.value.code == -6  # reedsolomon.ErrShortData
