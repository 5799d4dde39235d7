"""Every reachable gf_rows_kernel<RC> body on the GPU.

The matrix codec serves every (N, k) outside the five additive-FFT geometries
and the whole reedsolomon.Encoder mirror.  gf_rows_kernel is compiled once per
row-chunk size RC; rbc_gf_pick_rc(R, 21) picks the body from the number of
output rows R (2f for a Context(3f + 1, f), p for an Encoder(k, p)).  Each body
unrolls its accumulator loop, lays out its LDS tables ([j][RC], K rounded up to
even) and breaks off a short last chunk in its own way.

* Context(3f + 1, f), f = 1..24, codec "matrix": RC = 2, 4, .., 20 (one
  chunk), 11..21 (two chunks) and 15, 16, 16 (three chunks; R = 44 and 46
  leave the last one short), encode and decode;
* Encoder(k, p), p in {1, 3, 5, 7, 9}: the odd bodies RC = p, with odd and
  even k.
tests/test_launch_rules.py asserts those RC against the launcher's own rule
without a GPU.  Shard lengths: under one 16-byte column, and two 4096-byte
column tiles with the second almost empty and S % 16 != 0.  Everything is
compared bit-exactly with the C oracle or rbc_oracle.Encoder.  The bodies
RC = 22..48 cannot be reached while kGfRcMax is 21 and are not run."""
import numpy as np
import pytest

import launch_rules as lr
import rbc_oracle as orc

pytestmark = pytest.mark.gpu

I = 5  # instances: one present set each


def rup(x, a):
    return (x + a - 1) // a * a


def _present_sets(rng, n, f, k):
    """exactly k random, parity-heavy (the last k rows), data-only, N - f random,
    N - f random with one corrupted ECHO -> present [I][n], corrupt [I]."""
    present = np.zeros((I, n), np.uint8)
    present[0, rng.permutation(n)[:k]] = 1
    present[1, n - k:] = 1
    present[2, :k] = 1
    present[3, rng.permutation(n)[: n - f]] = 1
    present[4, rng.permutation(n)[: n - f]] = 1
    corrupt = np.full(I, -1, np.int32)
    corrupt[4] = int(rng.choice(np.flatnonzero(present[4])))
    return present, corrupt


@pytest.mark.parametrize("S", [15, 4096 + 17])
@pytest.mark.parametrize("f", lr.GF_CONTEXT_F, ids=[f"f{f}-rc{lr.context_rc(f)}" for f in lr.GF_CONTEXT_F])
def test_matrix_codec_commit_and_receive_every_row_chunk_body(gpu, ref, f, S):
    n, k = 3 * f + 1, f + 1
    B = k * S - min(k - 1, 3)  # not a multiple of k: the last data row is zero-padded
    assert (B + k - 1) // k == S and B % k
    ctx = gpu.Context(n, f)
    ctx.set_codec("matrix")
    assert ctx.codec == "matrix" and ctx.k == k and ctx.p == 2 * f
    d = ctx.depth
    spitch, vpitch, opitch = rup(S, 64), rup(k * S + 32, 64), rup(k * S, 16)
    rng = np.random.default_rng(61000 + 97 * f + S)
    values = rng.integers(0, 256, (I, vpitch), dtype=np.uint8)
    present, corrupt = _present_sets(rng, n, f, k)
    mb = gpu.DeviceBuffer
    b = dict(values=mb(I * vpitch), shards=mb(I * n * spitch), leaves=mb(I * n * 32), roots=mb(I * 32),
             branches=mb(I * n * d * 32), present=mb(I * n), corrupt=mb(I * 4), valid=mb(I * n),
             leaves_r=mb(I * n * 32), out=mb(I * opitch), digests=mb(I * 32), status=mb(I * 4))
    b["values"].upload(values)
    b["present"].upload(present)
    b["corrupt"].upload(corrupt)
    b["shards"].upload(np.full(I * n * spitch, 0xA5, np.uint8))

    def shards():
        return b["shards"].download().reshape(I, n, spitch)

    # commit: encode (R = 2f parity rows from K = k data rows), leaves, tree
    ctx.dev_encode(None, I, b["values"], vpitch, None, B, b["shards"], spitch)
    ctx.dev_leaves(None, I, b["shards"], spitch, None, S, b["leaves"])
    ctx.dev_merkle_build(None, I, b["leaves"], b["roots"], b["branches"])
    gpu.rbc.lib.rbc_device_sync(0)
    sh = shards().copy()
    roots = b["roots"].download().reshape(I, 32).copy()
    brs = b["branches"].download().reshape(I, n, d, 32).copy()
    want = [ref.encode_commit(n, f, values[i, :B]) for i in range(I)]
    for i, (want_sh, want_root, want_br, _) in enumerate(want):
        assert np.array_equal(sh[i, :, :S], want_sh), (i, np.flatnonzero((sh[i, :, :S] != want_sh).any(axis=1)))
        assert not sh[i, :, S:].any(), "pad bytes past S must be zero"
        assert bytes(roots[i]) == want_root and np.array_equal(brs[i], want_br), i

    # one-shot receive: absent rows and the corrupted ECHO hold garbage, so only
    # the decode (R = 2f regenerated rows from the first k valid ones) restores them
    gpu.rbc.poison_rows(0, None, b["shards"], n * spitch, spitch, n, b["present"], b["corrupt"], I, 7 + f)
    ctx.dev_inject_faults(None, I, b["shards"], spitch, b["corrupt"])
    gpu.rbc.lib.rbc_device_sync(0)
    rx = shards().copy()
    gone = present == 0
    gone[4, corrupt[4]] = True
    assert np.array_equal(rx[~gone], sh[~gone]) and ((rx[gone][:, :S] != sh[gone][:, :S]).mean(axis=1) > 0.5).all()
    ctx.dev_verify(None, I, b["shards"], spitch, None, S, b["branches"], b["roots"], b["present"], b["valid"],
                   b["leaves_r"])
    ctx.dev_interpolate(None, I, b["shards"], spitch, None, S, b["valid"], b["leaves_r"], 1, b["roots"], b["out"],
                        opitch, b["digests"], b["status"])
    gpu.rbc.lib.rbc_device_sync(0)
    valid = b["valid"].download().reshape(I, n)
    status = np.frombuffer(b["status"].download().tobytes(), np.int32)
    out = b["out"].download().reshape(I, opitch)
    digests = b["digests"].download().reshape(I, 32)
    after = shards()
    for i in range(I):
        want_valid = np.array([present[i, j] and ref.verify(n, rx[i, j, :S], j, brs[i, j], bytes(roots[i]))
                               for j in range(n)], np.uint8)
        assert np.array_equal(valid[i], want_valid), i
        assert want_valid.sum() == present[i].sum() - (i == 4)
        rc, value, dig = ref.interpolate(n, f, rx[i, :, :S], want_valid, bytes(roots[i]))
        assert status[i] == rc == 0, (i, status[i], rc)
        assert np.array_equal(out[i, : k * S], value), i
        assert out[i, :B].tobytes() == values[i, :B].tobytes() and not out[i, B: k * S].any(), i
        assert bytes(digests[i]) == dig, i
        # every regenerated row, the parity rows that are no part of the value included
        assert np.array_equal(after[i, :, :S], want[i][0]), (i, np.flatnonzero((after[i, :, :S] != want[i][0]).any(axis=1)))


@pytest.mark.parametrize("k", lr.GF_ENCODER_K)
@pytest.mark.parametrize("p", lr.GF_ENCODER_P)
def test_encoder_odd_row_chunk_bodies(gpu, p, k):
    """Encoder(k, p) runs gf_rows_kernel<p> (one chunk of p rows) in Encode,
    Verify and Reconstruct; k = 1 and 7 pad the LDS coefficient tables to an
    even K."""
    assert lr.gf_pick_rc(p) == p
    enc, ref = gpu.Encoder(k, p), orc.Encoder(k, p)
    rng = np.random.default_rng(1000 * p + k)
    for S in (1, 4097):
        data = rng.integers(0, 256, k * S, dtype=np.uint8)
        want = ref.split(data)
        ref.encode(want)
        got = enc.split(data)
        assert all(np.array_equal(a, b_) for a, b_ in zip(got, ref.split(data)))
        enc.encode(got)
        assert all(np.array_equal(a, b_) for a, b_ in zip(got, want)), (S, "encode")
        assert enc.verify(got) and ref.verify(want)
        for row in (k, k + p - 1):  # a changed byte in the first / last parity row
            bad = [s.copy() for s in want]
            bad[row][S - 1] ^= 0x80
            assert not enc.verify(bad) and not ref.verify(bad), (S, row)
        keep = set(rng.permutation(k + p)[:k].tolist())
        part = [s.copy() if j in keep else None for j, s in enumerate(want)]
        want_part = [s.copy() if j in keep else None for j, s in enumerate(want)]
        enc.reconstruct(part)
        ref.reconstruct(want_part)
        assert all(np.array_equal(a, b_) for a, b_ in zip(part, want_part)), (S, sorted(keep))
        assert all(np.array_equal(a, b_) for a, b_ in zip(part, want)), (S, sorted(keep))
