"""Host side of the wire receiver (rbc_wire_receive), no GPU.

tests/cpp/wire_receive_fuzz.cpp is a stand-alone program (its own main, no
Python loading) built with ASan + UBSan from csrc/capi.cpp, batcher.cpp,
rbc_node.cpp (the host decoder) and wire_receive.cpp, the unchanged host-memory
HIP stand-in tests/cpp/hip_stub.cpp and tests/cpp/wire_receive_stub.cpp, a
scalar restatement of unmarshal_echo_kernel written from the format
description.  It checks rbc_wire_receive's argument checks (a rejected call
enqueues nothing, a good call after it works), random and boundary arguments
over buffers sized exactly to the contract, and the mutation corpus against the
host decoder status for status.
"""
import os

from san_program import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleisthenes_amd", "csrc")
NEW = ("rbc_dev_unmarshal_echo", "rbc_wire_receiver_create", "rbc_wire_receiver_destroy", "rbc_wire_receive",
       "rbc_wire_receive_wait", "rbc_wire_receive_poll")


def test_wire_receive_host_path_under_asan_ubsan(tmp_path):
    stdout = build_and_run(tmp_path, "wire_receive_fuzz",
                           cpp=("wire_receive_fuzz.cpp", "wire_receive_stub.cpp", "hip_stub.cpp"),
                           csrc=("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_receive.cpp"))
    words = stdout.split()
    assert words[0] == "ok" and int(words[1]) > 6000, stdout  # the whole corpus ran


def test_header_announces_the_wire_receiver_and_the_library_exports_it():
    from cleisthenes_amd import _lib
    header = os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")
    text = open(header).read()
    assert "#define RBC_HAS_WIRE_RECEIVE 1" in text
    assert "#define RBC_WIRE_OTHER_ROOT 2" in text and "#define RBC_WIRE_OTHER_LEN 3" in text
    names = _lib.header_functions(header)
    for fn in NEW:
        assert fn in names and hasattr(_lib.lib, fn) and fn in _lib._SIGS, fn
        assert getattr(_lib.lib, fn).argtypes == _lib._SIGS[fn][1], fn
    assert _lib.HAS_WIRE_RECEIVE
    _lib.require_wire_receive()
    assert (_lib.RBC_WIRE_OTHER_ROOT, _lib.RBC_WIRE_OTHER_LEN) == (2, 3)
    assert _lib.lib.rbc_abi_version() == 7  # the addition is detected by symbol presence


def test_signatures_have_the_arity_of_the_header():
    """Every new _SIGS entry takes as many arguments as its declaration."""
    import re

    from cleisthenes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")).read(), flags=re.S)
    for fn in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
        assert m, fn
        assert len(m.group(1).split(",")) == len(_lib._SIGS[fn][1]), fn


def test_the_python_binding_exports_the_receiver():
    import cleisthenes_amd as ca
    assert "WireReceiver" in ca.__all__
    for name in ("receive", "receive_submit", "close"):
        assert callable(getattr(ca.WireReceiver, name))
    assert callable(ca.Context.dev_unmarshal_echo)


def test_the_host_runtime_does_not_reference_the_new_launcher():
    """capi.cpp, batcher.cpp, rbc_node.cpp and wire_rx.cpp must keep linking with hip_stub.cpp and
    wire_rx_stub.cpp as they stand."""
    for f in ("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_rx.cpp"):
        assert "unmarshal_echo" not in open(os.path.join(CSRC, f)).read(), f
    assert "wire_receive.cpp" in open(os.path.join(CSRC, "Makefile")).read()
