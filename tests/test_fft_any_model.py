"""CPU checks of the run-time-geometry additive-FFT codec's structure
(tests/fft_any_model.py mirrors rs_fft_any.hip: the solve levels unrolled with
the active block kept at row 0 by swapping halves, inner transforms with
constants looked up by (layer, lambda >> (j+1)), zero rows kept zero, the final
transform skipping groups outside [k, n)).  Every output byte must equal
klauspost v1.9.1's encode-matrix product, at every n the kernel accepts."""
import numpy as np
import pytest

import fft_any_model as fam
import fft_model as fm
import rbc_oracle as orc

# the geometries of tests/test_gpu_fft_any.py: every solve case at every level of every width
GPU_GEOMS = [(33, 10), (33, 16), (33, 0), (48, 8), (49, 8), (47, 8), (63, 20), (64, 20), (64, 1),
             (65, 21), (100, 33), (100, 18), (101, 18), (99, 18), (127, 42), (128, 30), (128, 0),
             (129, 42), (200, 66), (200, 36), (201, 36), (199, 36), (255, 84), (256, 64), (256, 1), (255, 127),
             (63, 31), (127, 63)]


def _check(n, f):
    k = n - 2 * f
    rng = np.random.default_rng(n * 31 + f)
    data = [rng.integers(0, 256, 8, dtype=np.uint8) for _ in range(k)]
    want = orc.gf_rows(orc.encode_matrix(k, n)[k:], data) if n > k else []
    got = fam.encode(k, n, data)
    assert len(got) == n
    assert all(np.array_equal(g, d) for g, d in zip(got[:k], data))
    assert all(np.array_equal(g, w) for g, w in zip(got[k:], want)), (n, f)


def test_n_from_33_to_256_at_the_bft_maximum_f():
    """Every third n, and every n within one of 64, 128 and 256: all 224 take
    eleven seconds in pure Python (most of it the oracle's matrix)."""
    ns = set(range(33, 257, 3)) | {63, 64, 65, 127, 128, 129, 255, 256}
    for n in sorted(ns):
        _check(n, (n - 1) // 3)


@pytest.mark.parametrize("n,f", GPU_GEOMS, ids=[f"n{n}f{f}" for n, f in GPU_GEOMS])
def test_gpu_test_geometries(n, f):
    _check(n, f)


def test_table_is_the_twiddle_by_layer_and_shifted_coset():
    assert len(fam.TW) == 255
    for j in range(8):
        for lam in range(0, 256, 1 << (j + 1)):  # a layer-j butterfly's coset has bits 0..j clear
            assert fam.tw(j, lam) == fm.twiddle(j, lam)
            # ... and W_j is constant on lam + V_j
            assert all(fm.twiddle(j, lam + x) == fam.tw(j, lam) for x in range(1 << j))


@pytest.mark.parametrize("n,f,bfly,mac", [(128, 42, 448, 16), (100, 33, 377, 2)])
def test_butterfly_count_is_the_design_figure(n, f, bfly, mac):
    """butterflies (one constant multiply each) and unwinding
    multiplies per byte column of the run-time-geometry transform."""
    k = n - 2 * f
    cnt = fam.Counter()
    fam.encode(k, n, [np.zeros(1, np.uint8)] * k, cnt)
    assert (cnt.bfly, cnt.mac) == (bfly, mac)
    assert cnt.mul < k * (n - k) // 5  # against the matrix product's MACs
