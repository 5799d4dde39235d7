"""The session the three wire handles share (csrc/wire_session.h), no GPU.

tests/cpp/wire_session_test.cpp is a stand-alone program (its own main, no
Python loading, tests/cpp/hip_stub.cpp not linked) built with ASan + UBSan.  It
includes the header, defines the HIP entry points the header uses, and makes the
completion event fail, report "not ready", or the k-th allocation fail: ticket 0
and tickets not issued yet, poll before and after readiness, a failed
completion (no copy-out, RBC_ERR_DEVICE from wait exactly once, the next
submission unharmed, two failures each against its own ticket), and a create
that fails half-way (nothing leaks).
"""
import os

from san_program import CSRC, build_and_run


def test_wire_session_under_asan_ubsan(tmp_path):
    stdout = build_and_run(tmp_path, "wire_session_test", cpp=("wire_session_test.cpp",),
                           headers=("hip/hip_runtime_api.h",))
    words = stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 59, stdout  # every check ran


def test_the_shared_code_exists_once():
    """wait, poll, the carving and the ring-slot check live in wire_session.h alone; the three
    handles include it and forward to it."""
    for f in ("wire_rx.cpp", "wire_receive.cpp", "wire_ready.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "wire_session.h"' in text, f
        for once in ("struct Carver", "round_up(size_t", "hipEventSynchronize", "hipEventQuery", "% 16"):
            assert once not in text, (f, once)
    header = open(os.path.join(CSRC, "wire_session.h")).read()
    for once in ("struct Carver", "round_up(size_t", "hipEventSynchronize", "hipEventQuery", "% 16"):
        assert header.count(once) == 1, once
    assert "wire_session.h" in open(os.path.join(CSRC, "Makefile")).read()
