"""Every SHA-256 tail in every row-hashing body, against hashlib.

A row of S bytes ends in a last block of S % 64 message bytes, the 0x80, zeros
and the bit length; with S % 64 > 55 the length moves to a block of its own.
sha256_row (sha_rows_kernel, sha_rx_kernel's two sides, the per-message form)
and sha256_row2 (sha_rows2_kernel) each write that tail themselves.

  ragged batches     one instance per length S = 1..192 at pitch 192, seeded
                     non-zero bytes in [S, pitch) of every row: rbc_dev_leaves
                     at (4,1) and (7,2), the cur side of rbc_dev_receive_step
                     (the received rows), its prev side (the regenerated rows)
                     and rbc_validate_packed (per-message lengths 1..192)
  walk form          (4,1), S in {2047, 2048, 2049, 2103, 2104}, 8 instances,
                     the last byte of one row flipped: leaves and valid[]
  sha_rows2_kernel   (2,0), 131,072 instances, present NULL, S in {1079, 1080}
                     (S % 64 = 55 and 56): every leaf, and valid[] with the
                     last byte of every 97th row flipped after the commit

Leaves are hashlib's over the S bytes the device holds; valid[] is the C
oracle's walk (rbc_ref.verify_many / rbc_ref.verify) over the same bytes."""
import hashlib

import numpy as np
import pytest

import rbc_ref

pytestmark = pytest.mark.gpu

PITCH = 192
LENS = np.arange(1, PITCH + 1, dtype=np.uint32)

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def sync(gpu):
    gpu.rbc.lib.rbc_device_sync(0)


def up(gpu, a):
    a = np.ascontiguousarray(a)
    b = gpu.DeviceBuffer(max(a.nbytes, 16))
    b.upload(a.view(np.uint8).reshape(-1))
    return b


def filled(gpu, nbytes, byte):
    b = gpu.DeviceBuffer(nbytes)
    b.upload(np.full(nbytes, byte, np.uint8))
    return b


def sha(b):
    return np.frombuffer(hashlib.sha256(bytes(b)).digest(), np.uint8)


class Ragged:
    """Instance i commits a value of shard length S = i + 1; every row's bytes
    [S, PITCH) hold non-zero garbage.  One row of each instance is absent."""

    def __init__(self, n, f, seed):
        rng = np.random.default_rng(seed)
        k, I = n - 2 * f, len(LENS)
        d = max((n - 1).bit_length(), 1)
        self.n, self.f, self.k, self.count, self.depth = n, f, k, I, d
        self.rows = rng.integers(1, 256, (I, n, PITCH), dtype=np.uint8)
        self.leaves = np.zeros((I, n, 32), np.uint8)
        self.roots = np.zeros((I, 32), np.uint8)
        self.branches = np.zeros((I, n, d, 32), np.uint8)
        self.present = np.ones((I, n), np.uint8)
        for i, S in enumerate(int(s) for s in LENS):
            value = rng.integers(0, 256, k * S - min(3, k - 1), dtype=np.uint8)
            shards, root, br, _ = rbc_ref.encode_commit(n, f, value)
            self.rows[i, :, :S] = shards
            self.roots[i] = np.frombuffer(root, np.uint8)
            self.branches[i] = br
            self.present[i, i % n] = 0
            for j in range(n):
                self.leaves[i, j] = sha(shards[j])
        self.rows.flags.writeable = False


def ragged(n, f):
    return once(("ragged", n, f), lambda: Ragged(n, f, 6100 + n))


def _wrong_lengths(got, want):
    """The shard lengths of the instances with a wrong leaf."""
    return [int(LENS[i]) for i in np.flatnonzero((got != want).any(axis=(1, 2)))]


@pytest.mark.parametrize("n,f", [(4, 1), (7, 2)])
def test_ragged_leaves(gpu, n, f):
    """rbc_dev_leaves: sha_rows_kernel<false>, one lane per row, per-instance lengths."""
    c = ragged(n, f)
    ctx = gpu.Context(n, f)
    leaves = filled(gpu, c.count * n * 32, 0xDD)
    ctx.dev_leaves(None, c.count, up(gpu, c.rows), PITCH, up(gpu, LENS), 0, leaves)
    sync(gpu)
    got = leaves.download().reshape(c.count, n, 32)
    assert not _wrong_lengths(got, c.leaves), _wrong_lengths(got, c.leaves)


def _receive_step(gpu):
    """(4,1): leaves and valid after the first call (cur's ECHO rows hashed),
    leaves, rows and status after the second (prev's regenerated rows hashed)."""
    c = ragged(4, 1)
    I, n = c.count, c.n
    ctx = gpu.Context(n, c.f)
    held = np.array(c.rows)
    garbage = np.random.default_rng(6200).integers(1, 256, held.shape, dtype=np.uint8)
    held[c.present == 0] = garbage[c.present == 0]  # absent rows: garbage, pads included
    vpitch = (c.k * PITCH + 15) // 16 * 16 + 16
    shards, leaves, valid = up(gpu, held), filled(gpu, I * n * 32, 0xDD), filled(gpu, I * n, 0xCC)
    status = gpu.DeviceBuffer(I * 4)
    status.zero()
    keep = (shards, leaves, valid, status, up(gpu, LENS), up(gpu, c.branches), up(gpu, c.roots), up(gpu, c.present),
            gpu.DeviceBuffer(I * vpitch), gpu.DeviceBuffer(I * 32))
    b = ctx.rx_batch(I, shards, PITCH, keep[4], 0, keep[5], keep[6], keep[7], valid, leaves, keep[8], vpitch, keep[9],
                     status)
    ctx.dev_receive_step(None, b, None)
    sync(gpu)
    first = dict(leaves=leaves.download().reshape(I, n, 32).copy(), valid=valid.download().reshape(I, n).copy())
    ctx.dev_receive_step(None, None, b)
    sync(gpu)
    second = dict(leaves=leaves.download().reshape(I, n, 32).copy(), status=status.download().view(np.int32).copy(),
                  rows=shards.download().reshape(I, n, PITCH).copy())
    return first, second


def test_ragged_receive_step_cur_side(gpu):
    """sha_rx_kernel's v side: the received rows of the batch being verified."""
    c = ragged(4, 1)
    first, _ = once("receive-step", lambda: _receive_step(gpu))
    pr = c.present == 1
    assert np.array_equal(first["valid"], c.present)
    bad = (first["leaves"] != c.leaves).any(axis=2) & pr
    assert not bad.any(), [int(LENS[i]) for i in np.flatnonzero(bad.any(axis=1))]


def test_ragged_receive_step_prev_side(gpu):
    """sha_rx_kernel's r side: the rows the decode regenerated, hashed by the next call."""
    c = ragged(4, 1)
    _, second = once("receive-step", lambda: _receive_step(gpu))
    assert not second["status"].any(), np.flatnonzero(second["status"])
    for i, S in enumerate(int(s) for s in LENS):
        assert np.array_equal(second["rows"][i, :, :S], c.rows[i, :, :S]), S  # the absent row is back
    assert not _wrong_lengths(second["leaves"], c.leaves), _wrong_lengths(second["leaves"], c.leaves)


def test_ragged_validate_packed(gpu):
    """rbc_validate_packed: sha_rows_kernel<true>'s per-message form, message
    m of 1 + m bytes at a 64-byte aligned offset of an arena of non-zero bytes."""
    c = ragged(4, 1)
    n, I = c.n, c.count
    rng = np.random.default_rng(6300)
    idx = (np.arange(I) % n).astype(np.uint8)
    offs, at = np.zeros(I, np.uint64), 0
    for m in range(I):
        offs[m] = at
        at += (int(LENS[m]) + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
    arena = rng.integers(1, 256, at, dtype=np.uint8)
    for m in range(I):
        arena[int(offs[m]): int(offs[m]) + int(LENS[m])] = c.rows[m, idx[m], : LENS[m]]
    br = np.stack([c.branches[m, idx[m]] for m in range(I)])
    want_ok = np.array([rbc_ref.verify(n, c.rows[m, idx[m], : LENS[m]], int(idx[m]), br[m], c.roots[m].tobytes())
                        for m in range(I)])
    assert want_ok.all()
    ok, leaves = gpu.Context(n, c.f).validate_packed(arena, offs, LENS, idx, br, c.roots, leaves=True)
    want = np.stack([c.leaves[m, idx[m]] for m in range(I)])
    wrong = [int(LENS[m]) for m in np.flatnonzero((leaves != want).any(axis=1))]
    assert not wrong, wrong
    assert np.array_equal(ok, want_ok)


# ---- walk form, uniform lengths ---------------------------------------------------------
WALK_LENS = (2047, 2048, 2049, 2103, 2104)


def _walk_case(S):
    n, f, I = 4, 1, 8
    rng = np.random.default_rng(6400 + S)
    pitch = (S + 63) // 64 * 64
    rows = np.zeros((I, n, pitch), np.uint8)
    roots, branches = np.zeros((I, 32), np.uint8), np.zeros((I, n, 2, 32), np.uint8)
    for i in range(I):
        shards, root, br, _ = rbc_ref.encode_commit(n, f, rng.integers(0, 256, 2 * S - 1, dtype=np.uint8))
        rows[i, :, :S], roots[i], branches[i] = shards, np.frombuffer(root, np.uint8), br
    rows[3, 2, S - 1] ^= 0x80  # after the commit: that row is invalid
    leaves = np.stack([[sha(rows[i, j, :S]) for j in range(n)] for i in range(I)])
    valid = np.array([[rbc_ref.verify(n, rows[i, j, :S], j, branches[i, j], roots[i].tobytes()) for j in range(n)]
                      for i in range(I)], np.uint8)
    assert valid.sum() == I * n - 1 and not valid[3, 2]
    return dict(n=n, f=f, I=I, S=S, pitch=pitch, rows=rows, roots=roots, branches=branches, leaves=leaves, valid=valid)


@pytest.mark.parametrize("S", WALK_LENS)
@pytest.mark.parametrize("via", ["verify", "step"])
def test_walk_form_tails(gpu, via, S):
    """sha_rows_kernel<true> (rbc_dev_verify, every row of every instance) and
    sha_rx_kernel with the walk (rbc_dev_receive_step) on both sides of the
    one-block / two-block padding boundary and of a whole last block."""
    c = once(("walk", S), lambda: _walk_case(S))
    n, I = c["n"], c["I"]
    ctx = gpu.Context(n, c["f"])
    assert ctx.verify_form(S) == "walk"
    shards, leaves, valid = up(gpu, c["rows"]), filled(gpu, I * n * 32, 0xDD), filled(gpu, I * n, 0xCC)
    branches, roots = up(gpu, c["branches"]), up(gpu, c["roots"])
    if via == "verify":
        ctx.dev_verify(None, I, shards, c["pitch"], None, S, branches, roots, None, valid, leaves)
        sync(gpu)
    else:
        vpitch = (2 * S + 15) // 16 * 16 + 16
        present, status = up(gpu, np.ones(I * n, np.uint8)), gpu.DeviceBuffer(I * 4)
        status.zero()
        values, digests = gpu.DeviceBuffer(I * vpitch), gpu.DeviceBuffer(I * 32)
        b = ctx.rx_batch(I, shards, c["pitch"], None, S, branches, roots, present, valid, leaves, values, vpitch,
                         digests, status)
        ctx.dev_receive_step(None, b, None)
        sync(gpu)
    got_leaves, got_valid = leaves.download().reshape(I, n, 32).copy(), valid.download().reshape(I, n).copy()
    if via == "step":  # the call that finishes the batch
        ctx.dev_receive_step(None, None, b)
        sync(gpu)
    assert np.array_equal(got_leaves, c["leaves"])
    assert np.array_equal(got_valid, c["valid"])


# ---- sha_rows2_kernel<true> ---------------------------------------------------------------
ROWS2_COUNT, ROWS2_PITCH = 131072, 1088


def _rows2_base():
    """[131072][2][1088] random bytes: the rows, and non-zero-ish garbage behind them."""
    rows = np.random.default_rng(6500).integers(0, 256, (ROWS2_COUNT, 2, ROWS2_PITCH), dtype=np.uint8)
    rows.flags.writeable = False
    return rows


@pytest.mark.parametrize("S", [1079, 1080])
def test_rows2_tail(gpu, S):
    """(2,0): k = n = 2, the rows are the value's halves, the root is
    H(leaf0 || leaf1) and each leaf's branch is the other leaf.  262,144 rows
    with no present mask is the smallest grid that takes sha_rows2_kernel; both
    lengths take the walk form.  S % 64 = 55 is the longest tail whose length
    shares the last block, 56 the shortest that needs a block of its own."""
    n, I, pitch = 2, ROWS2_COUNT, ROWS2_PITCH
    base = once("rows2", _rows2_base)
    ctx = gpu.Context(n, 0)
    assert ctx.verify_form(S) == "walk" and S % 64 in (55, 56)
    committed = np.ascontiguousarray(base[:, :, :S])
    leaves = np.frombuffer(b"".join(hashlib.sha256(r).digest() for r in committed.reshape(I * n, S)),
                           np.uint8).reshape(I, n, 32)
    roots = np.frombuffer(b"".join(hashlib.sha256(lv).digest() for lv in leaves.reshape(I, 64)), np.uint8).reshape(I, 32)
    branches = np.ascontiguousarray(leaves[:, ::-1, :]).reshape(I, n, 1, 32)
    held = np.array(base)
    flip = np.arange(0, I * n, 97)
    held.reshape(I * n, pitch)[flip, S - 1] ^= 0x01  # after the commit
    sent = np.ascontiguousarray(held[:, :, :S])
    _, ok = rbc_ref.verify_many(n, sent, branches, roots, np.repeat(np.arange(I, dtype=np.int32), n),
                                np.tile(np.arange(n, dtype=np.int32), I), 8)
    want_valid = ok.reshape(I * n)
    assert (want_valid[flip] == 0).all() and want_valid.sum() == I * n - len(flip)
    want_leaves = leaves.reshape(I * n, 32).copy()
    for r in flip:
        want_leaves[r] = sha(sent.reshape(I * n, S)[r])
    d_leaves, d_valid = filled(gpu, I * n * 32, 0xDD), filled(gpu, I * n, 0xCC)
    ctx.dev_verify(None, I, up(gpu, held), pitch, None, S, up(gpu, branches), up(gpu, roots), None, d_valid, d_leaves)
    sync(gpu)
    got_leaves, got_valid = d_leaves.download().reshape(I * n, 32), d_valid.download()
    assert np.array_equal(got_valid, want_valid), np.flatnonzero(got_valid != want_valid)[:8]
    assert np.array_equal(got_leaves, want_leaves), np.flatnonzero((got_leaves != want_leaves).any(axis=1))[:8]
