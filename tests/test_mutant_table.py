"""tests/mutant_table.py against tests/mutants/Makefile and what build() made of
it, and the references of test_gpu_digest_words.py against each other -- all
on the host, before any device time is spent on a mutant."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import digest_cases as dc
import mutant_table as mt
import rbc_ref


def _makefile():
    with open(os.path.join(mt.MUTANT_DIR, "Makefile")) as fh:
        return fh.read()


def test_table_and_makefile_name_the_same_mutants():
    r = subprocess.run(["make", "-s", "--no-print-directory", "-C", mt.MUTANT_DIR, "list"], capture_output=True,
                       text=True, check=True)
    assert r.stdout.split() == [m[0] for m in mt.MUTANTS]
    text = _makefile()
    for name, file, lines, killer in mt.MUTANTS:
        assert re.search(rf"^SRC_{name} = {re.escape(file)}$", text, re.M), name
        assert re.search(rf"^SED_{name} = \S", text, re.M), name
    assert re.search(r"^LINES = 1$", text, re.M) and all(m[2] == 1 for m in mt.MUTANTS)
    assert len(mt.MUTANTS) == 11 and len({m[0] for m in mt.MUTANTS}) == 11


@pytest.mark.parametrize("name,file,lines,killer", mt.MUTANTS, ids=[m[0] for m in mt.MUTANTS])
def test_built_copy_differs_in_the_declared_lines(name, file, lines, killer):
    assert os.path.exists(mt.library(name)), "build() makes tests/mutants"
    with open(os.path.join(mt.SRC_DIR, file)) as fh:
        product = fh.read().split("\n")
    with open(mt.copy_of(name, file)) as fh:
        copy = fh.read().split("\n")
    assert len(product) == len(copy)
    assert sum(a != b for a, b in zip(product, copy)) == lines
    # the mutant is no older than its copy: it was compiled from it
    assert os.path.getmtime(mt.library(name)) >= os.path.getmtime(mt.copy_of(name, file))


def test_every_killer_collects():
    killers = sorted({m[3] for m in mt.MUTANTS})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + killers,
                       cwd=mt.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in killers:
        assert any(ln.split("[")[0] == k for ln in r.stdout.splitlines()), k


@pytest.mark.parametrize("n,f", [(7, 2), (16, 5), (200, 66)])
def test_tree_builder_without_override_is_the_oracles_commitment(n, f):
    rows, root, br = dc.commit(n, f, 13, np.random.default_rng(n))
    levels, r2, b2 = dc.build_tree(n, dc.leaf_hashes(rows))
    assert r2 == root and np.array_equal(b2[:, : dc.depth_of(n)], br)
    assert [len(lv) for lv in levels] == [1 << (dc.depth_of(n) - l) for l in range(dc.depth_of(n) + 1)]
    # every leaf of the built tree verifies under the oracle's walk
    assert all(rbc_ref.verify(n, rows[j], j, b2[j, : dc.depth_of(n)], r2) for j in range(n))


def test_oracle_rejects_a_tree_with_one_wrong_node():
    """Recheck case (b): every ECHO sent verifies against R', interpolate reports a root mismatch."""
    case = dc.built("byz-trees", dc.ByzantineTrees)
    i = case.index(2, 5)
    l, v = case.node[i]
    assert l == 2 and not case.present[i, v << l: (v + 1) << l].any() and case.present[i].sum() == case.n - 4
    assert bytes(case.roots[i]) != bytes(case.honest_roots[i])
    assert np.array_equal(case.want_valid[i], case.present[i])
    assert case.want_status[i] == dc.ROOT_MISMATCH
    st, _, _ = rbc_ref.interpolate(case.n, case.f, case.rows[i], case.present[i], case.honest_roots[i].tobytes())
    assert st == 0  # the same rows against the honest tree's root deliver


def test_oracle_rejects_a_commitment_over_a_non_codeword():
    """A GF-lane case: all n rows prove, the re-encoding differs from the altered row alone."""
    n, f, _ = dc.GF_GEOMS["fft-16"]
    case = dc.built(("gf", n, f, n - 1), lambda: dc.NonCodewords(n, f, n - 1))
    b = 19
    assert (case.want_status == dc.ROOT_MISMATCH).all()
    diff = np.argwhere(case.rows[b] != case.want_rows[b])
    assert diff.tolist() == [[n - 1, b]]
    ok = [rbc_ref.verify(n, case.rows[b, j], j, case.branches[b, j], case.roots[b].tobytes()) for j in range(n)]
    assert all(ok)
