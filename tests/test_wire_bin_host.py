"""Host side of the binary VAL / ECHO payload codec (RBC_HAS_WIRE_BINARY), no GPU.

* rbc_bin_encode_val / rbc_bin_decode_val / rbc_payload_decode_val and
  rbc_val_message_size_codec against tests/wire_bin.py, the Python restatement
  of the format table, and against tests/golden/wire_bin_v1.json, which freezes
  version 1.
* tests/cpp/wire_bin_fuzz.cpp: a stand-alone program (its own main, no Python
  loading) built with ASan + UBSan from csrc/capi.cpp, batcher.cpp,
  rbc_node.cpp, wire_rx.cpp and wire_receive.cpp, the unchanged host-memory HIP
  stand-in tests/cpp/hip_stub.cpp and tests/cpp/wire_bin_stub.cpp, a scalar
  restatement of the two binary receive kernels.
* The header, the exported symbols, the ctypes signatures and the Python API.
"""
import json
import os
import re

import numpy as np
import pytest

import wire_bin as wb
from san_program import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cleisthenes_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wire_bin_v1.json")
NEW = ("rbc_bin_encode_val", "rbc_bin_decode_val", "rbc_payload_decode_val", "rbc_val_message_size_codec",
       "rbc_ctx_set_wire_codec", "rbc_ctx_wire_codec", "rbc_node_set_wire_codec")


def _fields(rng, L, S):
    return tuple(rng.integers(0, 256, x, dtype=np.uint8).tobytes() for x in (32, 32 * L, S))


def test_bin_encode_val_equals_the_restatement_byte_for_byte():
    from cleisthenes_amd import protocol
    rng = np.random.default_rng(1)
    for S in (0, 1, 2, 15, 16, 17, 63, 64, 65, 1000):
        for L in (0, 1, 2, 7, 8):
            root, br, blk = _fields(rng, L, S)
            p = protocol.bin_encode_val(root, br, blk)
            assert p == wb.payload(root, br, blk), (S, L)
            assert len(p) == 40 + 32 * L + S and p[0] == 0xB1
            for decode in (protocol.bin_decode_val, protocol.payload_decode_val):
                got = decode(p)
                assert (got["RootHash"], got["Branch"], got["Block"][0]) == (root, br, blk), (S, L)
            for t in (wb.VAL, wb.ECHO):
                assert protocol.pb_encode(t, p) == wb.message(t, root, br, blk), (S, L, t)
            # each decoder rejects the other's payload
            with pytest.raises(protocol.RBCError):
                protocol.json_decode_val(p)
            if S:
                js = protocol.json_encode_val(root, br, blk)
                with pytest.raises(protocol.RBCError):
                    protocol.bin_decode_val(js)
                assert protocol.payload_decode_val(js) == protocol.json_decode_val(js)


def test_bin_codec_rejects_what_the_format_rules_out():
    from cleisthenes_amd import protocol
    rng = np.random.default_rng(2)
    root, br, blk = _fields(rng, 2, 50)
    good = wb.payload(root, br, blk)
    bad = [good[:39], good[:-1], good + b"\0", b"\xb0" + good[1:], good[:1] + b"\x02" + good[2:],
           good[:3] + b"\x01" + good[4:], good[:2] + b"\x03" + good[3:], good[:4] + b"\x33" + good[5:], b""]
    for p in bad:
        with pytest.raises(protocol.RBCError) as e:
            protocol.bin_decode_val(p)
        assert e.value.code == -20, p[:8]  # RBC_ERR_PROTOCOL
    for args in ((root[:31], br, blk), (root, br[:-1], blk), (root, bytes(32 * 256), blk)):
        with pytest.raises(protocol.RBCError):
            protocol.bin_encode_val(*args)


def test_the_golden_file_freezes_version_1():
    """A dozen whole messages, written once from the restatement: decode and
    re-encode must reproduce them, and so must the restatement as it is now."""
    from cleisthenes_amd import protocol
    cases = json.load(open(GOLDEN))["messages"]
    assert len(cases) >= 12
    for c in cases:
        msg = bytes.fromhex(c["hex"])
        root, br, blk = (bytes.fromhex(c[k]) for k in ("root", "branch", "shard"))
        assert wb.message(c["type"], root, br, blk) == msg, c["name"]
        t, pl = protocol.pb_decode(msg)
        got = protocol.bin_decode_val(pl)
        assert (t, got["RootHash"], got["Branch"], got["Block"][0]) == (c["type"], root, br, blk), c["name"]
        assert protocol.pb_encode(t, protocol.bin_encode_val(root, br, blk)) == msg, c["name"]
        assert len(msg) == c["bytes"]


def test_val_message_size_codec_is_the_length_of_the_restated_message():
    from cleisthenes_amd import _lib
    size = _lib.lib.rbc_val_message_size_codec
    for n in (4, 5, 7, 16, 256):
        grid = list(range(1, 201)) + [2 ** 21 - 104 + d for d in range(-3, 4)]
        if n == 4:  # varint(J) and varint(R) grow here
            grid += list(range(20, 26)) + list(range(16274, 16284))
        for idx in (0, n - 1):
            L = wb.flat_len(n, idx)
            for t in (wb.VAL, wb.ECHO):
                for S in grid:
                    want = len(wb.wrap(t, bytes(40 + 32 * L + S)))  # len() of the restated message
                    assert size(1, n, S, idx, t) == want, (n, idx, t, S)
                    assert size(0, n, S, idx, t) == _lib.lib.rbc_val_message_size(n, S, idx, t), (n, idx, t, S)
    assert size(2, 4, 10, 0, 0) == 0 and size(1, 0, 10, 0, 0) == 0
    # the issue's table: one C2 ECHO (S = 23,832, depth 7)
    assert size(1, 128, 23832, 0, 1) == 24106


def test_wire_bin_host_path_under_asan_ubsan(tmp_path):
    stdout = build_and_run(tmp_path, "wire_bin_fuzz", cpp=("wire_bin_fuzz.cpp", "wire_bin_stub.cpp", "hip_stub.cpp"),
                           csrc=("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_rx.cpp", "wire_receive.cpp"))
    words = stdout.split()
    assert words[0] == "ok" and int(words[1]) > 100000, stdout  # the whole corpus ran


def test_header_announces_the_binary_codec_and_the_library_exports_it():
    from cleisthenes_amd import _lib
    header = os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")
    text = open(header).read()
    assert "#define RBC_HAS_WIRE_BINARY 1" in text
    assert "#define RBC_WIRE_CODEC_JSON 0" in text and "#define RBC_WIRE_CODEC_BINARY 1" in text
    names = _lib.header_functions(header)
    for fn in NEW:
        assert fn in names and hasattr(_lib.lib, fn) and fn in _lib._SIGS, fn
        assert getattr(_lib.lib, fn).argtypes == _lib._SIGS[fn][1], fn
    assert _lib.HAS_WIRE_BINARY
    _lib.require_wire_binary()
    assert (_lib.RBC_WIRE_CODEC_JSON, _lib.RBC_WIRE_CODEC_BINARY) == (0, 1)
    assert _lib.lib.rbc_abi_version() == 7  # the addition is detected by symbol presence


def test_signatures_have_the_arity_of_the_header():
    from cleisthenes_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.INCLUDE_DIR, "rbc_protocol.h")).read(), flags=re.S)
    for fn in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % fn, text)
        assert m, fn
        assert len(m.group(1).split(",")) == len(_lib._SIGS[fn][1]), fn


def test_the_python_binding_exports_the_codec():
    import cleisthenes_amd as ca
    from cleisthenes_amd import protocol
    for name in ("bin_encode_val", "bin_decode_val", "payload_decode_val"):
        assert callable(getattr(protocol, name)), name
    assert callable(ca.Context.set_wire_codec) and isinstance(ca.Context.wire_codec, property)
    assert callable(protocol.Node.set_wire_codec)
    assert ca.Context.WIRE_CODECS == ("json", "binary")


def test_the_host_files_reference_no_new_launcher_and_the_kernels_live_in_wire_hip():
    """capi.cpp, wire_rx.cpp and wire_receive.cpp must keep linking with the
    stand-ins of the earlier sanitizer programs as they stand: they only set
    the codec field of the launchers' arguments."""
    launchers = set()
    for f in ("capi.cpp", "batcher.cpp", "rbc_node.cpp", "wire_rx.cpp", "wire_receive.cpp"):
        launchers |= set(re.findall(r"\brbc_launch_(?:un)?marshal_\w+", open(os.path.join(CSRC, f)).read()))
    assert launchers == {"rbc_launch_marshal_val", "rbc_launch_unmarshal_val", "rbc_launch_unmarshal_echo"}
    wire = open(os.path.join(CSRC, "wire.hip")).read()
    for k in ("marshal_val_bin_kernel", "unmarshal_val_bin_kernel", "unmarshal_echo_bin_kernel"):
        assert k in wire, k
    assert "wire.o" in open(os.path.join(ROOT, "tests", "mutants", "Makefile")).read()
