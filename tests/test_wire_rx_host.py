"""Host side of the wire receive path, no GPU.

tests/cpp/wire_rx_fuzz.cpp is a stand-alone program (its own main, no Python
loading) built with ASan + UBSan from csrc/capi.cpp, batcher.cpp, rbc_node.cpp
and wire_rx.cpp, the unchanged host-memory HIP stand-in tests/cpp/hip_stub.cpp
and tests/cpp/wire_rx_stub.cpp, a scalar restatement of the unmarshal kernel
written from the format description.  It checks rbc_wire_validate's argument
checks (a rejected call enqueues nothing, a good call after it works), the
mutation corpus of tests/test_gpu_wire_rx.py against the host decoder, and that
buffers sized exactly to the contract are never overrun.
"""
import os

from san_program import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleisthenes_amd", "csrc")


def test_wire_rx_host_path_under_asan_ubsan(tmp_path):
    stdout = build_and_run(tmp_path, "wire_rx_fuzz", cpp=("wire_rx_fuzz.cpp", "wire_rx_stub.cpp", "hip_stub.cpp"),
                           csrc=("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_rx.cpp"))
    words = stdout.split()
    assert words[0] == "ok" and int(words[1]) > 3000, stdout  # the whole corpus ran


def test_header_announces_the_wire_receive_path_and_the_library_exports_it():
    from cleisthenes_amd import _lib
    header = os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")
    assert "#define RBC_HAS_WIRE_RX 1" in open(header).read()
    names = _lib.header_functions(header)
    for fn in ("rbc_dev_unmarshal_val", "rbc_wire_rx_create", "rbc_wire_rx_destroy", "rbc_wire_validate",
               "rbc_wire_wait", "rbc_wire_poll"):
        assert fn in names and hasattr(_lib.lib, fn) and fn in _lib._SIGS, fn
    assert _lib.lib.rbc_abi_version() == 7  # the addition is detected by symbol presence


def test_the_host_runtime_does_not_reference_the_new_launcher():
    """capi.cpp, batcher.cpp and rbc_node.cpp must keep linking with hip_stub.cpp alone."""
    for f in ("capi.cpp", "batcher.cpp", "rbc_node.cpp"):
        assert "unmarshal" not in open(os.path.join(CSRC, f)).read(), f
