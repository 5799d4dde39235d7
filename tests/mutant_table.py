"""The value mutants of tests/mutants/Makefile (librbc_gpu_m_<name>.so) and the
test that must kill each: name, the product source its one sed substitution
changes, the number of lines it changes, and the killer's node id.
tests/test_mutant_table.py checks this table against the Makefile and the
built copies; tests/test_gpu_mutants.py runs every killer on its mutant."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_DIR = os.path.join(ROOT, "tests", "mutants")
SRC_DIR = os.path.join(ROOT, "cleisthenes_amd", "csrc")

WORDS = "tests/test_gpu_digest_words.py::"
TAILS = "tests/test_gpu_sha_tails.py::"

# (name, file, changed lines, killer)
MUTANTS = [
    ("recheck_root", "kernels.hip", 1, WORDS + "test_recheck_expect_root_word"),
    ("recheck_entry", "kernels.hip", 1, WORDS + "test_recheck_byzantine_node_word"),
    ("path_eq8", "kernels.hip", 1, WORDS + "test_shared_path_spec_entry_word"),
    ("wire_root", "wire.hip", 1, WORDS + "test_unmarshal_echo_root_word"),
    ("gf_rows_cmp", "kernels.hip", 1, WORDS + "test_gf_compare_byte"),
    ("fft_cmp_prefetch", "rs_fft.hip", 1, WORDS + "test_gf_compare_byte"),
    ("fft_cmp_flush", "rs_fft.hip", 1, WORDS + "test_gf_compare_byte"),
    ("merkle_check_root", "kernels.hip", 1, WORDS + "test_recheck_expect_root_word"),
    ("rx_walk_root", "kernels.hip", 1, WORDS + "test_walk_root_word"),
    ("sha_row2_tail", "device_common.h", 1, TAILS + "test_rows2_tail"),
    ("sha_row_tail", "device_common.h", 1, TAILS + "test_ragged_leaves"),
]


def library(name):
    return os.path.join(MUTANT_DIR, f"librbc_gpu_m_{name}.so")


def copy_of(name, file):
    return os.path.join(MUTANT_DIR, "gen", name, file)
