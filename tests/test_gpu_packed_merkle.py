"""Packed Merkle blocks on the GPU: more than one tree per one-wave block.

rbc_launch_merkle and rbc_launch_recheck pack G = rbc_trees_per_block(W, count)
trees (instances) into each block; G > 1 needs count >= 1024 and the largest G
needs count >= 512 * G, far above the batches of the other GPU tests (G = 1,
or 2 at the bench shapes).  The cases of tests/launch_rules.py PACKED_CASES
run G = 64, 64, 8, 32, 16, 8, 4 and 2 in 513 blocks, the last one partly
filled (tests/test_launch_rules.py asserts those G against the launcher's own
rule, without a GPU):

* merkle_kernel<false> (+ merkle_top_kernel at W = 256): rbc_dev_merkle_build
  on random leaves, every root and branch byte against the C oracle's
  rbcref_merkle_from_leaves, over poisoned output buffers, and against the
  same leaves built in batches of 96 (G = 1);
* merkle_kernel<true> and merkle_recheck_kernel: a device commit received
  through rbc_dev_verify + rbc_dev_interpolate and through
  rbc_dev_receive_step with the full and the node-reuse recheck, each instance
  in one of eight roles (honest, corrupted, Byzantine, too few shards) placed
  on every position of a block, with statuses, valid masks, values and digests
  from the C oracle for every instance.
All comparisons are bit-exact."""
import ctypes

import numpy as np
import pytest

import launch_rules as lr

pytestmark = pytest.mark.gpu

POISON = 0xA5
IDS = [f"n{n}-G{g}" for (n, _), g in zip(lr.PACKED_CASES, lr.PACKED_G)]


def rup(x, a):
    return (x + a - 1) // a * a


def _first_bad(a, b):
    """Index of the first instance (axis 0) where a and b differ, or None."""
    assert a.shape == b.shape
    if a.size == 0:
        return None
    bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
    return int(bad[0]) if len(bad) else None


def _oracle_trees(ref, n, leaves):
    """rbcref_merkle_from_leaves per instance -> roots [I][32], branches [I][n][d][32]."""
    I = len(leaves)
    d = ref.lib().rbcref_tree_depth(n)
    roots = np.zeros((I, 32), np.uint8)
    brs = np.zeros((I, n, max(d, 1), 32), np.uint8)
    fn = ref.lib().rbcref_merkle_from_leaves
    lv, rt, br = leaves.ctypes.data, roots.ctypes.data, brs.ctypes.data
    ls, bs = leaves.strides[0], brs.strides[0]
    for i in range(I):
        fn(n, ctypes.c_void_p(lv + i * ls), ctypes.c_void_p(rt + 32 * i), ctypes.c_void_p(br + i * bs))
    return roots, brs, d


def _build(gpu, ctx, leaves, chunk=None):
    """rbc_dev_merkle_build over poisoned root / branch buffers, in one batch or
    in batches of `chunk` instances -> roots, branches as the device left them."""
    I, n = leaves.shape[:2]
    d = ctx.depth
    b_lv, b_rt, b_br = gpu.DeviceBuffer(I * n * 32), gpu.DeviceBuffer(I * 32), gpu.DeviceBuffer(I * n * d * 32)
    b_lv.upload(leaves)
    b_rt.upload(np.full(I * 32, POISON, np.uint8))
    b_br.upload(np.full(I * n * d * 32, POISON, np.uint8))
    step = chunk or I
    for i0 in range(0, I, step):
        c = min(step, I - i0)
        ctx.dev_merkle_build(None, c, b_lv.value + i0 * n * 32, b_rt.value + i0 * 32, b_br.value + i0 * n * d * 32)
    gpu.rbc.lib.rbc_device_sync(0)
    return b_rt.download().reshape(I, 32), b_br.download().reshape(I, n, d, 32)


@pytest.mark.parametrize("n,count", lr.PACKED_CASES, ids=IDS)
def test_packed_merkle_build_every_root_and_branch(gpu, ref, n, count):
    G = lr.packed_g(n, count)
    assert G > 1 and count % G, "the case must pack trees and leave the last block partly filled"
    ctx = gpu.Context(n, (n - 1) // 3)
    rng = np.random.default_rng(77000 + 13 * n + count)
    leaves = rng.integers(0, 256, (count, n, 32), dtype=np.uint8)
    want_roots, want_brs, d = _oracle_trees(ref, n, leaves)
    assert d == ctx.depth
    roots, brs = _build(gpu, ctx, leaves)
    i = _first_bad(roots, want_roots)
    assert i is None, f"root of instance {i} (tree {i % G} of block {i // G}, G = {G})"
    i = _first_bad(brs, want_brs)
    assert i is None, f"branches of instance {i} (tree {i % G} of block {i // G}, G = {G})"


@pytest.mark.parametrize("n,count", [(7, 4096 + 3), (13, 16384 + 5), (199, 1024 + 1)], ids=["n7-G8", "n13-G32", "n199-G2"])
def test_packed_merkle_build_equals_unpacked_batches(gpu, n, count):
    """The same leaves as one batch (G trees per block) and as batches of 96
    (one tree per block): identical roots and branches, nothing left poisoned."""
    assert (n, count) in lr.PACKED_CASES and lr.packed_g(n, count) > 1 and lr.packed_g(n, lr.UNPACKED_COUNT) == 1
    ctx = gpu.Context(n, (n - 1) // 3)
    leaves = np.random.default_rng(88000 + n).integers(0, 256, (count, n, 32), dtype=np.uint8)
    r_packed, b_packed = _build(gpu, ctx, leaves)
    r_single, b_single = _build(gpu, ctx, leaves, chunk=lr.UNPACKED_COUNT)
    assert _first_bad(r_packed, r_single) is None and _first_bad(b_packed, b_single) is None
    assert not (r_single == POISON).all(axis=1).any()


# ------------------------------------------------------------ check / recheck

# an instance's role; the partly filled last block takes them in this order
BYZANTINE, ROOT_FLIPPED, TOO_FEW, BAD_SHARD, BAD_BRANCH, HONEST, EXACTLY_K, DATA_ONLY = range(8)
ROLE_NAMES = ["byzantine", "root-flipped", "k-1-present", "bad-shard", "bad-branch", "honest", "exactly-k",
              "data-only"]


def _roles(count, G):
    """Role of every instance: tree g of block b gets role (b + g) % 8, so each
    position of a block (first, interior, last) sees all eight roles over the
    513 blocks and neighbours differ; the trees of the partly filled last block
    take the roles in their order above (the failing ones first)."""
    i = np.arange(count)
    role = (i // G + i % G) % 8
    last = i // G == (count - 1) // G
    role[last] = (i[last] % G) % 8
    return role


class _Case:
    """One batch: committed on the device, then turned into what a receiver
    holds (per-role present sets and damage), with the C oracle's verdicts."""

    def __init__(self, gpu, ref, n, count, S):
        self.gpu, self.n, self.I, self.S = gpu, n, count, S
        self.f = f = (n - 1) // 3
        self.k = k = n - 2 * f
        self.G = lr.packed_g(n, count)
        self.B = B = k * S - min(k - 1, 3)  # not a multiple of k: the last data row is zero-padded
        self.spitch, self.vpitch, self.opitch = 64, rup(k * S + 32, 64), rup(k * S, 16)
        I = count
        rng = np.random.default_rng(99000 + 17 * n + count)
        self.role = role = _roles(count, self.G)
        self.values = rng.integers(0, 256, (I, self.vpitch), dtype=np.uint8)
        # present sets: N - f random rows, or the role's own
        order = np.argsort(rng.random((I, n)), axis=1)
        npres = np.full(I, n - f)
        npres[(role == EXACTLY_K) | (role == DATA_ONLY)] = k
        npres[role == TOO_FEW] = k - 1
        order[role == DATA_ONLY] = np.arange(n)
        present = np.zeros((I, n), np.uint8)
        np.put_along_axis(present, order, (np.arange(n)[None, :] < npres[:, None]).astype(np.uint8), axis=1)
        self.present = present
        # Byzantine proposer: the highest received row (a parity row, and past the
        # first k received: valid but unused by the decode) altered before the tree
        top = n - 1 - np.argmax(present[:, ::-1], axis=1)
        self.byz = np.where(role == BYZANTINE, top, -1).astype(np.int32)
        assert (self.byz[role == BYZANTINE] >= k).all()

        ctx = self.ctx = gpu.Context(n, f)
        d = self.d = ctx.depth
        mb = gpu.DeviceBuffer
        b = self.b = dict(values=mb(I * self.vpitch), shards=mb(I * n * 64), leaves=mb(I * n * 32), roots=mb(I * 32),
                          branches=mb(I * n * d * 32), present=mb(I * n), byz=mb(I * 4))
        b["values"].upload(self.values)
        b["present"].upload(present)
        b["byz"].upload(self.byz)
        ctx.dev_encode(None, I, b["values"], self.vpitch, None, B, b["shards"], 64)
        ctx.dev_inject_faults(None, I, b["shards"], 64, b["byz"])
        ctx.dev_leaves(None, I, b["shards"], 64, None, S, b["leaves"])
        ctx.dev_merkle_build(None, I, b["leaves"], b["roots"], b["branches"])
        gpu.rbc.lib.rbc_device_sync(0)
        sh = b["shards"].download().reshape(I, n, 64).copy()
        brs = b["branches"].download().reshape(I, n, d, 32).copy()
        self.roots = b["roots"].download().reshape(I, 32).copy()
        self.committed = sh[:, :, :S].copy()

        # what the receiver holds
        pick = np.argmax(present * rng.random((I, n)), axis=1)  # a random received row
        bs = np.flatnonzero(role == BAD_SHARD)
        sh[bs, pick[bs], rng.integers(0, S, len(bs))] ^= 0x10
        bb = np.flatnonzero(role == BAD_BRANCH)
        lvl = bb % d
        lvl[(lvl == 0) & ((pick[bb] ^ 1) >= n)] = 1 % d  # the empty level-0 sibling is never read
        brs[bb, pick[bb], lvl, rng.integers(0, 32, len(bb))] ^= 0x04
        garbage = rng.integers(0, 256, sh.shape, dtype=np.uint8)
        sh = np.where(present[:, :, None] != 0, sh, garbage)  # absent rows hold garbage
        self.rx_shards, self.rx_branches = sh, brs
        self.wrong_roots = self.roots.copy()
        self.wrong_roots[role == ROOT_FLIPPED, 3] ^= 0x01

        # the oracle: validateMessage of every received ECHO, then interpolate
        ii, jj = np.nonzero(present)
        _, ok = ref.verify_many(n, sh[:, :, :S], brs, self.roots, ii, jj, 4)
        self.want_valid = np.zeros((I, n), np.uint8)
        self.want_valid[ii, jj] = ok
        self.want_status = np.zeros(I, np.int32)
        self.want_out = np.zeros((I, k * S), np.uint8)
        self.want_digest = np.zeros((I, 32), np.uint8)
        rx = np.ascontiguousarray(sh[:, :, :S])
        for i in range(I):
            rc, value, dig = ref.interpolate(n, f, rx[i], self.want_valid[i], self.wrong_roots[i].tobytes())
            self.want_status[i] = rc
            if rc == 0:
                self.want_out[i] = value
                self.want_digest[i] = np.frombuffer(dig, np.uint8)

    def receive(self, mode):
        """-> status, valid, out, digests of one receive of the batch."""
        gpu, I, n, S = self.gpu, self.I, self.n, self.S
        mb = gpu.DeviceBuffer
        b = dict(shards=mb(I * n * 64), branches=mb(I * n * self.d * 32), roots=mb(I * 32), valid=mb(I * n),
                 leaves=mb(I * n * 32), out=mb(I * self.opitch), digests=mb(I * 32), status=mb(I * 4))
        b["shards"].upload(self.rx_shards)
        b["branches"].upload(self.rx_branches)
        b["roots"].upload(self.roots)
        for name in ("valid", "out", "digests", "status"):
            b[name].upload(np.full(b[name].nbytes, POISON, np.uint8))
        present = self.b["present"]
        if mode == "oneshot":
            c = self.ctx
            c.dev_verify(None, I, b["shards"], 64, None, S, b["branches"], b["roots"], present, b["valid"], b["leaves"])
            gpu.rbc.lib.rbc_device_sync(0)
            b["roots"].upload(self.wrong_roots)  # after the verify
            c.dev_interpolate(None, I, b["shards"], 64, None, S, b["valid"], b["leaves"], 1, b["roots"], b["out"],
                              self.opitch, b["digests"], b["status"])
        else:
            rx = gpu.Context(n, self.f)
            rx.set_recheck(mode)
            cur = rx.rx_batch(I, b["shards"], 64, None, S, b["branches"], b["roots"], present, b["valid"],
                              b["leaves"], b["out"], self.opitch, b["digests"], b["status"])
            rx.dev_receive_step(None, cur, None)
            gpu.rbc.lib.rbc_device_sync(0)
            b["roots"].upload(self.wrong_roots)  # after cur's verify, before its recheck in the next call
            rx.dev_receive_step(None, None, cur)
        gpu.rbc.lib.rbc_device_sync(0)
        return dict(status=np.frombuffer(b["status"].download().tobytes(), np.int32).copy(),
                    valid=b["valid"].download().reshape(I, n).copy(),
                    out=b["out"].download().reshape(I, self.opitch)[:, : self.k * S].copy(),
                    digests=b["digests"].download().reshape(I, 32).copy())


@pytest.mark.parametrize("case", range(len(lr.PACKED_CASES)), ids=IDS)
def test_packed_check_and_recheck_every_instance_vs_oracle(gpu, ref, case):
    """rbc_dev_verify + rbc_dev_interpolate, and rbc_dev_receive_step with
    RBC_RECHECK_FULL and RBC_RECHECK_REUSE, at G instances per block: every
    instance's status (0, -3, -8), valid mask, value and digest are the C
    oracle's, whatever its neighbours in the block are, and the three paths
    agree."""
    n, count = lr.PACKED_CASES[case]
    c = _Case(gpu, ref, n, count, S=16 + case)
    G, role, k, S, B = c.G, c.role, c.k, c.S, c.B
    assert G == lr.PACKED_G[case] and c.spitch == rup(S, 64)

    # the roles are what they are meant to be, by the oracle's verdicts
    ws = c.want_status
    assert (ws[role == TOO_FEW] == -3).all() and (ws[(role == BYZANTINE) | (role == ROOT_FLIPPED)] == -8).all()
    assert (ws[role >= BAD_SHARD] == 0).all()
    lost = c.present.sum(axis=1) - c.want_valid.sum(axis=1)
    assert (lost[(role == BAD_SHARD) | (role == BAD_BRANCH)] == 1).all() and not lost[role >= HONEST].any()
    # and every role sits on the first, the last and (G > 2) an interior tree of a block, and in the last block
    pos = np.arange(count) % G
    tail = np.arange(count) // G == (count - 1) // G
    for r in range(8):
        assert {0, G - 1} <= set(pos[(role == r) & ~tail]), ROLE_NAMES[r]
        assert G == 2 or ((pos > 0) & (pos < G - 1) & (role == r)).any(), ROLE_NAMES[r]
    assert set(role[tail]) == set(range(min(8, int(tail.sum()))))

    ok = ws == 0
    honest_value = np.ascontiguousarray(c.values[:, :B])
    res = {mode: c.receive(mode) for mode in ("oneshot", "full", "reuse")}
    for mode, r in res.items():
        def where(i):
            near = range(max(i - i % G, i - 2), min(i - i % G + G, i + 3, count))
            return (f"{mode}: instance {i} ({ROLE_NAMES[role[i]]}), tree {i % G} of block {i // G}, G = {G}; "
                    f"its neighbours in the block: {[(x - i, ROLE_NAMES[role[x]]) for x in near if x != i]}")
        i = _first_bad(r["status"], ws)
        assert i is None, f"status {r['status'][i]} != {ws[i]}: " + where(i)
        i = _first_bad(r["valid"], c.want_valid)
        assert i is None, "valid: " + where(i)
        i = _first_bad(r["out"][ok], c.want_out[ok])
        assert i is None, "value: " + where(np.flatnonzero(ok)[i])
        i = _first_bad(r["out"][ok][:, :B], honest_value[ok])
        assert i is None, "value != the proposer's input: " + where(np.flatnonzero(ok)[i])
        i = _first_bad(r["digests"][ok], c.want_digest[ok])
        assert i is None, "digest: " + where(np.flatnonzero(ok)[i])
    for mode in ("full", "reuse"):
        for key in ("status", "valid"):
            assert np.array_equal(res[mode][key], res["oneshot"][key]), (mode, key)
        for key in ("out", "digests"):
            assert np.array_equal(res[mode][key][ok], res["oneshot"][key][ok]), (mode, key)
