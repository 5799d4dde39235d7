"""The launch rules of csrc/host_shared.h against their Python mirrors, no GPU.

tests/cpp/launch_rules_check.cpp (its own main, built from the header alone)
prints rbc_trees_per_block for a list of (width, count) and rbc_gf_pick_rc for
R = 0..255, and rbc_gf_regen_form for rows of 1..4200 bytes;
tests/launch_rules.py restates all three.  The GPU tests of the packed Merkle
kernels, of the gf_rows_kernel bodies and of the gf_regen_kernel pass bodies
choose their shapes by the mirrors, so the coverage they claim -- G in
{2, 4, .., 64}, every RC in 1..21, short last chunks, every (W, rows) pass of
gf_regen_kernel -- is asserted here against the C++ the launchers and
capi.cpp call."""
import os
import shutil
import subprocess

import pytest

import launch_rules as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

WIDTHS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
COUNTS = sorted({0, 1, 2, 5, 96, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2051, 4095, 4096, 4099, 8191, 8192,
                 8195, 16383, 16384, 16389, 32767, 32768, 32805, 65536, 1 << 20} |
                {c for _, c in lr.PACKED_CASES})


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("launch_rules") / "launch_rules_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", "-o", exe, os.path.join(CPP, "launch_rules_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [f"{w}:{c}" for w in WIDTHS for c in COUNTS]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""]
    out = dict(G={}, RC={}, RCMAX=None, KRC=None, REGEN={})
    for ln in lines[:-2]:
        t = ln.split()
        if t[0] == "G":
            out["G"][(int(t[1]), int(t[2]))] = int(t[3])
        elif t[0] == "RC":
            out["RC"][int(t[1])] = int(t[2])
        elif t[0] == "REGEN":
            out["REGEN"][(int(t[1]), int(t[2]))] = tuple(int(x) for x in t[3:])
        elif t[0] == "RCMAX":
            out["RCMAX"] = int(t[1])
        else:
            assert t[0] == "KRC", ln
            out["KRC"] = [int(x) for x in t[1:]]
    return out


def test_trees_per_block_mirror_equals_the_header(printed):
    assert len(printed["G"]) == len(WIDTHS) * len(COUNTS)
    for (w, c), g in printed["G"].items():
        assert g == lr.trees_per_block(w, c), (w, c)
        # what the kernels rely on: a power of two, at most 64 trees, 16 KiB of node LDS
        assert g >= 1 and g & (g - 1) == 0 and g <= 64 and g * w * 32 <= max(16384, w * 32), (w, c, g)


def test_gf_pick_rc_mirror_equals_the_header(printed):
    assert printed["RCMAX"] == lr.GF_RC_MAX and printed["KRC"] == lr.K_RC
    assert sorted(printed["RC"]) == list(range(256))
    for R, rc in printed["RC"].items():
        assert rc == lr.gf_pick_rc(R), R
        assert rc in lr.K_RC and rc <= lr.GF_RC_MAX, R  # an instantiated body, within the VGPR budget


def test_packed_cases_reach_every_g(printed):
    got = []
    for (n, count), want in zip(lr.PACKED_CASES, lr.PACKED_G):
        w = lr.tree_width(n)
        g = printed["G"][(w, count)]
        assert g == want == lr.packed_g(n, count), (n, count)
        blocks = (count + g - 1) // g
        assert blocks == 513 and 0 < count - 512 * g < g, (n, count)  # a partly filled last block
        assert printed["G"][(w, lr.UNPACKED_COUNT)] == 1
        got.append(g)
    assert set(got) == {2, 4, 8, 16, 32, 64}
    assert (199, 1025) in lr.PACKED_CASES  # W = 256, n > 128: the build's merkle_top_kernel path


def test_gf_cases_reach_every_row_chunk_body(printed):
    ctx = {f: printed["RC"][2 * f] for f in lr.GF_CONTEXT_F}
    enc = {p: printed["RC"][p] for p in lr.GF_ENCODER_P}
    assert all(ctx[f] == lr.context_rc(f) for f in ctx)
    assert set(ctx.values()) == set(range(2, 21, 2)) | set(range(11, 22))
    assert set(enc.values()) == {1, 3, 5, 7, 9}
    assert set(ctx.values()) | set(enc.values()) == set(range(1, lr.GF_RC_MAX + 1))
    short = [f for f in ctx if (2 * f) % ctx[f]]
    assert short == [22, 23], short  # R = 44 in chunks of 15, R = 46 in chunks of 16
    # several chunks (the chunk index enters the block -> rows mapping) and a single one
    assert any(2 * f > ctx[f] for f in ctx) and any(2 * f == ctx[f] for f in ctx)
    # KP = K rounded up to even: odd and even K in both lists
    assert {k % 2 for k in lr.GF_ENCODER_K} == {0, 1} and {(f + 1) % 2 for f in ctx} == {0, 1}


def test_gf_regen_form_mirror_equals_the_header(printed):
    got = printed["REGEN"]
    assert sorted(S for lens, S in got if lens == 0) == list(range(1, 4201))
    assert sorted(S for lens, S in got if lens == 1) == list(range(64, 4201, 64))
    for (lens, S), form in got.items():
        pitch = (S + 63) // 64 * 64
        assert form == lr.gf_regen_form(bool(lens), 0 if lens else S, pitch), (lens, S)
        W, rc, nt = form
        # what the launcher instantiates: <1, 40, JC, 3> and <2, 24, JC, 4>
        assert form == lr.REGEN_FORMS[W] and 256 * W * nt <= 2048 and rc <= 48, (lens, S)
    assert got[(0, 2048)][0] == 1 and got[(0, 2049)][0] == 2 and got[(1, 2048)][0] == 1 and got[(1, 2112)][0] == 2


def test_regen_cases_reach_every_pass_body(printed):
    """One straight-line pass body per exact row count: 1..40 at W = 1, 1..24
    at W = 2, 64 in all, each run at two geometries or more."""
    reached = {}
    for n, f, S, ms in lr.REGEN_BODY_CASES:
        k, p = n - 2 * f, 2 * f
        W, rc, nt = printed["REGEN"][(0, S)]
        assert (W, rc, nt) == lr.REGEN_FORMS[1 if S == lr.REGEN_S_SHORT else 2]
        assert len(set(ms)) == len(ms) and min(ms) == 1 and max(ms) <= min(k, p, rc), (n, S)
        # instance i misses m_i data rows and holds every parity row: at least k rows stay present
        assert all(n - m >= k for m in ms), (n, S)
        bodies = {(W, rows) for m in ms for r0 in range(0, m, rc) for rows in [min(rc, m - r0)]}
        assert bodies == lr.regen_case_bodies(n, f, S, ms) == {(W, m) for m in ms}
        for b in bodies:
            reached.setdefault(b, []).append(n)
        pitch = (S + 63) // 64 * 64
        tiles = (pitch + 256 * W - 1) // (256 * W)
        assert tiles % nt and pitch % (256 * W) == 64, (n, S)  # idle waves, a 64-byte last tile
    assert set(reached) == {(1, r) for r in range(1, 41)} | {(2, r) for r in range(1, 25)}
    assert len(reached) == 64 and all(len(v) >= 2 for v in reached.values())
    ks = {n - 2 * f for n, f, _, _ in lr.REGEN_BODY_CASES}
    assert {2, 6, 22, 44, 86} == ks  # K < JC, K % 4 != 0 (22, 86: zero-coefficient padding), K % 4 == 0
