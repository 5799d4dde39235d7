"""Every value mutant of tests/mutants must be killed by the test
tests/mutant_table.py names for it: a fresh child process maps the mutant
(RBC_GPU_LIB) and runs that one test, which has to FAIL on an assertion -- exit
status 1 with the test among the failures.  Exit 0 is a survivor: the killer is
too weak.  Any other end of the child (a signal, an abort, a time-out) fails
the case and every case after it without another child being started: a mutant
changes a computed value or a verdict only, so nothing here is expected to do
more than fail an assertion.  The children run one at a time; none is retried."""
import os
import subprocess
import sys

import pytest

import mutant_table as mt

pytestmark = pytest.mark.gpu

# the child: say which library the package mapped, then run pytest on the killer
CHILD = ("import sys, pytest, cleisthenes_amd as ca\n"
         "print('rbc_library_path', ca.rbc.library_path(), flush=True)\n"
         "sys.exit(int(pytest.main(['-x', '-q', '-p', 'no:cacheprovider', sys.argv[1]])))\n")

_abnormal = []  # (mutant, what) of the first child that did not end as a test run ends


@pytest.mark.parametrize("name,file,lines,killer", mt.MUTANTS, ids=[m[0] for m in mt.MUTANTS])
def test_mutant_is_killed(gpu, name, file, lines, killer):
    assert not _abnormal, f"not run: the child of {_abnormal[0][0]} ended with {_abnormal[0][1]}"
    lib = mt.library(name)
    assert os.path.exists(lib), "build() makes tests/mutants"
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, killer], cwd=mt.ROOT, capture_output=True, text=True,
                           timeout=120, env=dict(os.environ, RBC_GPU_LIB=lib))
    except subprocess.TimeoutExpired:
        _abnormal.append((name, "a time-out"))
        raise
    tail = (r.stdout[-3000:], r.stderr[-2000:])
    if r.returncode not in (0, 1):
        _abnormal.append((name, f"status {r.returncode}"))
    assert r.returncode != 0, f"{name} survived {killer}"
    assert r.returncode == 1, (r.returncode, tail)
    mapped = [os.path.realpath(ln.split(" ", 1)[1]) for ln in r.stdout.splitlines() if ln.startswith("rbc_library_path ")]
    assert mapped == [os.path.realpath(lib)], mapped
    failed = [ln for ln in r.stdout.splitlines() if ln.startswith("FAILED ")]
    assert failed and all(ln.split()[1].split("[")[0] == killer for ln in failed), tail
    # by an assertion of the test, not by an error raised on the way
    errors = [ln[1:].strip() for ln in r.stdout.splitlines() if ln.startswith("E  ")]
    assert errors and errors[0].startswith(("AssertionError", "assert ")), tail
