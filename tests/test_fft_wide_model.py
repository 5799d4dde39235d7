"""CPU checks of the wide run-time-geometry additive-FFT codec's structure
(tests/fft_wide_model.py mirrors rs_fft_wide.hip: two 128-row halves, the
parked coefficients, the solve started at coset 128, both final transforms with
their skip rules).  Every output byte must equal klauspost v1.9.1's
encode-matrix product, at every n the kernel accepts."""
import numpy as np
import pytest

import fft_any_model as fam
import fft_model as fm
import fft_wide_model as fwm
import rbc_oracle as orc

# the geometries of tests/test_gpu_fft_wide.py
GPU_GEOMS = [(129, 42), (200, 66), (255, 84), (255, 127), (199, 36), (200, 36), (256, 64), (201, 36), (131, 1),
             (200, 20), (256, 32), (256, 1), (256, 0), (256, 85)]


def _check(n, f):
    k = n - 2 * f
    rng = np.random.default_rng(n * 31 + f)
    data = [rng.integers(0, 256, 8, dtype=np.uint8) for _ in range(k)]
    want = orc.gf_rows(orc.encode_matrix(k, n)[k:], data) if n > k else []
    got = fwm.encode(k, n, data)
    assert len(got) == n
    assert all(np.array_equal(g, d) for g, d in zip(got[:k], data))
    assert all(np.array_equal(g, w) for g, w in zip(got[k:], want)), (n, f)


def test_every_n_from_129_to_256_at_the_bft_maximum_f():
    for n in range(129, 257):
        _check(n, (n - 1) // 3)


@pytest.mark.parametrize("n,f", GPU_GEOMS, ids=[f"n{n}f{f}" for n, f in GPU_GEOMS])
def test_gpu_test_geometries(n, f):
    _check(n, f)


@pytest.mark.parametrize("k", [129, 130, 136, 137, 160, 191, 192, 193, 224, 255])
def test_upper_solve_at_every_level(k):
    """k > 128 at n = 256: tp = k - 128 walks the solve's cases at coset 128 (a
    lone row, the first compare group and one past it, a half, one either side
    of it, all but one row)."""
    data = [np.array([(7 * j + k) & 0xFF, (j * j + 1) & 0xFF], np.uint8) for j in range(k)]
    want = orc.gf_rows(orc.encode_matrix(k, 256)[k:], data)
    got = fwm.encode(k, 256, data)
    assert all(np.array_equal(g, w) for g, w in zip(got[k:], want))


def test_the_top_layer_is_free_at_coset_0():
    """W_7(0) = 0, and the table's W_7 is the only entry of its layer."""
    assert fm.twiddle(7, 0) == 0 and fam.tw(7, 0) == 0
    assert fam.tw_base(7) == 254


def test_solve_from_coset_0_is_the_narrow_solve():
    rng = np.random.default_rng(5)
    for k in (1, 45, 64, 87, 127, 128):
        rows = [rng.integers(0, 256, 4, dtype=np.uint8) if j < k else np.zeros(4, np.uint8) for j in range(128)]
        a, b = [r.copy() for r in rows], [r.copy() for r in rows]
        ca, cb = fam.Counter(), fwm.Counter()
        fam.solve_any(a, 7, k, ca)
        fwm.solve_from(b, 7, k, 0, cb)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert (ca.bfly, ca.mac, ca.copy) == (cb.bfly, cb.mac, cb.copy)


@pytest.mark.parametrize("n,f,bfly,mac", [(200, 66, 844, 4), (256, 85, 1025, 30)])
def test_butterfly_count_is_the_design_figure(n, f, bfly, mac):
    """butterflies (one constant multiply each) and unwinding
    multiplies per byte column of the wide transform."""
    k = n - 2 * f
    cnt = fwm.Counter()
    fwm.encode(k, n, [np.zeros(1, np.uint8)] * k, cnt)
    assert (cnt.bfly, cnt.mac) == (bfly, mac)
    assert cnt.mul < k * (n - k) // 10  # against the matrix product's MACs
