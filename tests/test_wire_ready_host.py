"""Host side of the READY path (rbc_dev_unmarshal_ready, rbc_dev_quorum,
rbc_wire_quorum), no GPU.

tests/cpp/wire_ready_fuzz.cpp is a stand-alone program (its own main, no
Python loading) built with ASan + UBSan from csrc/capi.cpp, batcher.cpp,
rbc_node.cpp (the host decoder) and wire_ready.cpp, the unchanged host-memory
HIP stand-in tests/cpp/hip_stub.cpp and tests/cpp/wire_ready_stub.cpp, a scalar
restatement of unmarshal_ready_kernel and quorum_kernel written from the header
text.  It checks rbc_wire_quorum's argument checks (a rejected call enqueues
nothing, a good call after it works), buffers sized exactly to the contract,
every single-byte mutation of a canonical READY with its truncations and
extensions against the host decoder, the 31- and 33-byte roots, and the quorum
table over every (E, R, status, own bit) at (4, 1), (7, 2) and (4, 0).
"""
import json
import os
import re

from san_program import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleisthenes_amd", "csrc")
NEW = ("rbc_dev_unmarshal_ready", "rbc_dev_quorum", "rbc_wire_quorum_create", "rbc_wire_quorum_destroy",
       "rbc_wire_quorum", "rbc_wire_quorum_wait", "rbc_wire_quorum_poll")


def test_wire_ready_host_path_under_asan_ubsan(tmp_path):
    stdout = build_and_run(tmp_path, "wire_ready_fuzz",
                           cpp=("wire_ready_fuzz.cpp", "wire_ready_stub.cpp", "hip_stub.cpp"),
                           csrc=("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_ready.cpp"))
    words = stdout.split()
    # the whole corpus (65 bytes x 255 values and the rest) and the three quorum tables ran
    assert words[0] == "ok" and int(words[1]) > 16000 and int(words[3]) > 3000, stdout


def test_header_announces_the_ready_path_and_the_library_exports_it():
    from cleisthenes_amd import _lib
    header = os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")
    text = open(header).read()
    assert "#define RBC_HAS_WIRE_READY 1" in text
    for name, value in (("ECHO", 1), ("AMPLIFY", 2), ("SEND_READY", 4), ("DELIVER", 8)):
        assert f"#define RBC_QUORUM_{name} {value}" in text
        assert getattr(_lib, f"RBC_QUORUM_{name}") == value
    names = _lib.header_functions(header)
    for fn in NEW:
        assert fn in names and hasattr(_lib.lib, fn) and fn in _lib._SIGS, fn
        assert getattr(_lib.lib, fn).argtypes == _lib._SIGS[fn][1], fn
    assert _lib.HAS_WIRE_READY
    _lib.require_wire_ready()
    assert _lib.lib.rbc_abi_version() == 7  # the addition is detected by symbol presence


def test_signatures_have_the_arity_of_the_header():
    """Every new _SIGS entry takes as many arguments as its declaration."""
    from cleisthenes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")).read(), flags=re.S)
    for fn in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
        assert m, fn
        assert len(m.group(1).split(",")) == len(_lib._SIGS[fn][1]), fn


def test_the_python_binding_exports_the_quorum():
    import cleisthenes_amd as ca
    assert "WireQuorum" in ca.__all__
    for name in ("submit", "quorum", "close"):
        assert callable(getattr(ca.WireQuorum, name))
    assert callable(ca.Context.dev_unmarshal_ready) and callable(ca.Context.dev_quorum)


def test_the_host_runtime_does_not_reference_the_new_launchers():
    """capi.cpp, batcher.cpp, rbc_node.cpp, wire_rx.cpp and wire_receive.cpp must keep linking with
    hip_stub.cpp and the stubs of their own tests as they stand."""
    for f in ("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_rx.cpp", "wire_receive.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "unmarshal_ready" not in text and "launch_quorum" not in text, f
    assert "wire_ready.cpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_golden_ready_messages_still_encode_and_decode_the_same():
    """tests/golden/wire_ready_v1.json pins the format: the host encoder emits these bytes for these
    roots, the host decoder returns the roots, and every message has the one length."""
    from cleisthenes_amd import protocol
    with open(os.path.join(ROOT, "tests", "golden", "wire_ready_v1.json")) as fh:
        g = json.load(fh)
    assert g["messages"]
    for e in g["messages"]:
        root, msg = bytes.fromhex(e["root"]), bytes.fromhex(e["message"])
        assert protocol.pb_encode(protocol.READY, protocol.json_encode_ready(root)) == msg
        t, payload = protocol.pb_decode(msg)
        assert t == protocol.READY and payload == e["payload"].encode()
        assert protocol.json_decode_ready(payload) == root
        assert len(msg) == g["message_size"]
