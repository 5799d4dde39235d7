"""Python mirrors of the three launch rules in cleisthenes_amd/csrc/host_shared.h,
and the shapes the GPU tests pick by them.

* trees_per_block(width, count) == rbc_trees_per_block: the trees
  (merkle_kernel) or instances (merkle_recheck_kernel) packed into a one-wave
  block;
* gf_pick_rc(R, rcmax) == rbc_gf_pick_rc_impl, the body of rbc_gf_pick_rc:
  the gf_rows_kernel<RC> body that serves R output rows;
* gf_regen_form(per_instance_lens, uniform_len, row_pitch) == rbc_gf_regen_form:
  the (W, RC, NT) of the gf_regen_kernel that rbc_launch_gf_regen runs, whose
  passes are one straight-line body per exact row count 1 .. RC.

tests/test_launch_rules.py (no GPU) builds tests/cpp/launch_rules_check.cpp
from the header and compares its output with these mirrors, and asserts that
PACKED_CASES reach G = 2 .. 64, GF_CONTEXT_F / GF_ENCODER_P reach every
RC in 1 .. 21 and REGEN_BODY_CASES reach every (W, rows) pass body of
gf_regen_kernel: a changed launcher rule fails there instead of quietly moving
tests/test_gpu_packed_merkle.py, tests/test_gpu_gf_bodies.py and
tests/test_gpu_regen_bodies.py onto other launch shapes."""

GF_RC_MAX = 21  # kGfRcMax
K_RC = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 26, 28, 30, 32, 36,
        40, 42, 44, 48]
MIN_BLOCKS = 512


def tree_width(n):
    w = 1
    while w < n:
        w <<= 1
    return w


def trees_per_block(width, count):
    g = 1 if width >= 512 else min(512 // width, 64)
    while g > 1 and (count + g - 1) // g < MIN_BLOCKS:
        g >>= 1
    return g


def gf_pick_rc(R, rcmax=GF_RC_MAX):
    if R <= 0:
        return 1
    rcmax = min(max(rcmax, 1), 48)
    chunks = (R + rcmax - 1) // rcmax
    want = (R + chunks - 1) // chunks
    for rc in K_RC:
        if rc >= want:
            return rc
    return 48


# (n, count): 513 blocks of G trees each, the last one partly filled.  n = 7,
# 13, 31, 61 have padding leaves and an empty level-0 sibling; n = 199 takes
# the stop_m / merkle_top_kernel path of the build.
PACKED_CASES = [
    (4, 32768 + 37),   # W = 4,   G = 64
    (7, 32768 + 37),   # W = 8,   G = 64
    (7, 4096 + 3),     # W = 8,   G = 8 (halved from 64 by the 512-block rule)
    (13, 16384 + 5),   # W = 16,  G = 32
    (31, 8192 + 3),    # W = 32,  G = 16
    (61, 4096 + 3),    # W = 64,  G = 8
    (100, 2048 + 3),   # W = 128, G = 4
    (199, 1024 + 1),   # W = 256, G = 2
]
PACKED_G = [64, 64, 8, 32, 16, 8, 4, 2]
UNPACKED_COUNT = 96  # the batch size of the G = 1 comparison runs


def packed_g(n, count):
    return trees_per_block(tree_width(n), count)


# gf_rows_kernel bodies: a Context(3f + 1, f) runs R = 2f rows in encode and
# decode, an Encoder(k, p) runs R = p.
GF_CONTEXT_F = list(range(1, 25))
GF_ENCODER_P = [1, 3, 5, 7, 9]
GF_ENCODER_K = [1, 2, 7, 8]


def context_rc(f):
    return gf_pick_rc(2 * f)


# gf_regen_kernel: the interpolate of the FFT codec regenerates the m missing
# data rows of an instance in passes of RC rows, then one of m % RC.
REGEN_FORMS = {1: (1, 40, 3), 2: (2, 24, 4)}  # W -> (W, RC, NT)


def gf_regen_form(per_instance_lens, uniform_len, row_pitch):
    S = row_pitch if per_instance_lens else uniform_len
    return REGEN_FORMS[1 if S <= 2048 else 2]


def regen_pass_rows(m, rc):
    """The row counts of the passes that regenerate m rows: the bodies run."""
    return [min(rc, m - r0) for r0 in range(0, m, rc)]


# (n, f, S, the missing data rows m_i of instance i): S = 260 at pitch 320 is
# two 256-byte tiles for three waves, the second 64 bytes wide; S = 2049 at
# pitch 2112 is five 512-byte tiles in groups of four.  (64,21) has K = 22,
# KP = 24 (zero-coefficient padding), (16,5) K = 6 < JC, (256,85) K = 86, KP = 88.
REGEN_S_SHORT, REGEN_S_LONG = 260, 2049
REGEN_BODY_CASES = [
    (256, 85, REGEN_S_SHORT, list(range(1, 41))),
    (128, 42, REGEN_S_SHORT, list(range(1, 41))),
    (64, 21, REGEN_S_SHORT, list(range(1, 23))),
    (16, 5, REGEN_S_SHORT, list(range(1, 7))),
    (4, 1, REGEN_S_SHORT, [1, 2]),
    (128, 42, REGEN_S_LONG, list(range(1, 25))),
    (256, 85, REGEN_S_LONG, list(range(1, 25))),
    (64, 21, REGEN_S_LONG, list(range(1, 23))),
    (16, 5, REGEN_S_LONG, list(range(1, 7))),
]


def regen_case_bodies(n, f, S, ms):
    """The (W, rows) pass bodies one uniform-length batch of the case runs."""
    W, rc, _ = gf_regen_form(False, S, (S + 63) // 64 * 64)
    return {(W, rows) for m in ms for rows in regen_pass_rows(m, rc)}
