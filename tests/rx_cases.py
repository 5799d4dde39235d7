"""Receiver-side test cases built on the host from the C oracle, for the
device API (rbc_dev_verify, rbc_dev_interpolate, rbc_dev_receive_step): one
small batch of committed values, the ECHO rows a receiver holds, and what
interpolate must leave in every buffer.  Used by test_gpu_decode_n128.py and
test_gpu_receive_step_overlap.py."""
import numpy as np

import rbc_ref

PATTERNS = ("none", "worst", "parity", "corrupt_data", "corrupt_parity", "byzantine")


def round_up(x, a):
    return (x + a - 1) // a * a


class Case:
    """count instances of (n, f) with shard length S.

    pattern (every instance unless `byz` / `corrupt` name instances):
      none            every ECHO received: nothing is missing, nothing regenerated
      worst           all f absences on data rows
      parity          all f absences on parity rows
      corrupt_data    f absences anywhere, one received data row corrupted
      corrupt_parity  f absences on parity rows, one received parity row
                      (valid but unused, had it verified) corrupted
      byzantine       the proposer committed a non-codeword (the construction of
                      tests/test_gpu_verified.py): every ECHO verifies under the
                      root; even instances are random rows, odd ones a codeword
                      with one received, unused parity row altered.  Absences on
                      parity rows only, so the data rows decide the re-encoding.
    byz / corrupt: instance indices that get the byzantine / corrupt_data
    treatment on top of `pattern` (the receive-step test mixes them).
    """

    def __init__(self, n, f, S, count, pattern, seed, byz=None, corrupt=None):
        assert pattern in PATTERNS
        rng = np.random.default_rng(seed)
        k = n - 2 * f
        self.n, self.f, self.k, self.S, self.count = n, f, k, S, count
        self.B = k * S - min(3, k - 1)  # S = ceil(B / k), the last data row zero padded
        self.spitch = round_up(S, 64)
        self.vpitch = round_up(k * S, 16) + 16  # a tail to be zeroed
        self.depth = max(int(np.ceil(np.log2(n))), 0)
        byz = set(range(count) if pattern == "byzantine" else (byz or ()))
        corrupt = set(corrupt or ())
        d = max(self.depth, 1)
        self.rows_in = np.zeros((count, n, S), np.uint8)  # the committed rows (what honest ECHOs carry)
        self.want_rows = np.zeros((count, n, S), np.uint8)  # every row after interpolate
        self.roots = np.zeros((count, 32), np.uint8)
        self.branches = np.zeros((count, n, d, 32), np.uint8)
        self.present = np.ones((count, n), np.uint8)
        self.bad = np.full(count, -1)  # the corrupted received row
        self.want_status = np.zeros(count, np.int32)
        self.changed = [[] for _ in range(count)]  # valid rows the re-encoding replaces
        for i in range(count):
            value = rng.integers(0, 256, self.B, dtype=np.uint8)
            shards, root, br, _ = rbc_ref.encode_commit(n, f, value)
            pat = "byzantine" if i in byz else ("corrupt_data" if i in corrupt else pattern)
            data, par = np.arange(k), np.arange(k, n)
            if pat == "none":
                absent = []
            elif pat == "worst":
                absent = rng.permutation(data)[:f]
            elif pat == "parity":
                absent = rng.permutation(par)[:f]
            elif pat == "corrupt_data":
                absent = rng.permutation(n)[:f]
            elif pat == "corrupt_parity":
                absent = rng.permutation(par)[:f]
            else:
                absent = rng.permutation(par)[:f]
            self.present[i, absent] = 0
            rec = np.flatnonzero(self.present[i])
            if pat == "corrupt_data":
                self.bad[i] = int(rng.choice(rec[rec < k]))
            elif pat == "corrupt_parity":
                self.bad[i] = int(rng.choice(rec[rec >= k]))
            if pat == "byzantine":
                rows = shards.copy()
                if i % 2 == 0:
                    rows = rng.integers(0, 256, (n, S), dtype=np.uint8)
                else:
                    j = int(rng.choice(rec[rec >= k]))
                    rows[j, int(rng.integers(0, S))] ^= 0x21
                # the commitment is over the rows as they are; the re-encoding
                # of the (all received) data rows is what interpolate leaves
                _, root, br = commit_rows(n, rows)
                want, _, _, _ = rbc_ref.encode_commit(n, f, np.ascontiguousarray(rows[:k]).reshape(-1))
                self.changed[i] = [int(j) for j in rec if not np.array_equal(rows[j], want[j])]
                assert self.changed[i]
                self.want_status[i] = -8
                shards = rows
            else:
                want = shards
            self.rows_in[i], self.want_rows[i] = shards, want
            self.roots[i] = np.frombuffer(root, np.uint8)
            self.branches[i, :, : self.depth] = br
        self.want_valid = self.present.copy()
        for i in np.flatnonzero(self.bad >= 0):
            self.want_valid[i, self.bad[i]] = 0

    def receiver_rows(self, seed=5):
        """[count][n][spitch]: received rows in place, zero padded to the pitch
        (the corrupted one with a flipped byte); absent rows are garbage, their
        pads included."""
        buf = np.random.default_rng(seed).integers(0, 256, (self.count, self.n, self.spitch), dtype=np.uint8)
        buf[self.present == 1] = 0
        buf[:, :, : self.S] = np.where(self.present[:, :, None] == 1, self.rows_in, buf[:, :, : self.S])
        for i in np.flatnonzero(self.bad >= 0):
            buf[i, self.bad[i], self.S // 2] ^= 0x40
        return buf

    def want_leaves(self):
        out = np.zeros((self.count, self.n, 32), np.uint8)
        for i in range(self.count):
            for j in range(self.n):
                out[i, j] = np.frombuffer(rbc_ref.sha256(self.want_rows[i, j]), np.uint8)
        return out

    def want_value_digest(self, i):
        """The C oracle's interpolate over what the receiver holds (status 0 only)."""
        buf = self.receiver_rows()[i, :, : self.S]
        st, val, dig = rbc_ref.interpolate(self.n, self.f, buf, self.want_valid[i], self.roots[i].tobytes())
        return st, val, dig


def commit_rows(n, rows):
    """Merkle commitment over arbitrary rows: (leaves, root, branches [n][depth][32])."""
    import rbc_oracle as orc
    com = orc.rbc_commit([rows[j].tobytes() for j in range(n)])
    leaves = np.stack([np.frombuffer(x, np.uint8) for x in com["leaves"]])
    d = orc.tree_depth(n)
    br = np.zeros((n, d, 32), np.uint8)
    for j in range(n):
        flat = orc.flat_branch(com["branches"][j])
        br[j] = np.frombuffer(flat, np.uint8).reshape(d, 32)
    return leaves, com["root"], br


class DevCase:
    """A Case's buffers on the device, each its own allocation."""

    def __init__(self, gpu, case):
        c = self.case = case
        self.gpu = gpu
        mb = gpu.DeviceBuffer
        I, n = c.count, c.n
        self.shards = mb(I * n * c.spitch)
        self.branches = mb(c.branches.nbytes)
        self.roots = mb(I * 32)
        self.present = mb(I * n)
        self.valid = mb(I * n)
        self.leaves = mb(I * n * 32)
        self.values = mb(I * c.vpitch)
        self.digests = mb(I * 32)
        self.status = mb(I * 4)
        self.reset()

    def reset(self):
        c = self.case
        self.shards.upload(c.receiver_rows())
        self.branches.upload(c.branches)
        self.roots.upload(c.roots)
        self.present.upload(c.present)
        self.valid.upload(np.full(c.count * c.n, 0xCC, np.uint8))
        self.leaves.upload(np.full(c.count * c.n * 32, 0xDD, np.uint8))
        self.values.upload(np.full(c.count * c.vpitch, 0xA5, np.uint8))
        self.digests.upload(np.full(c.count * 32, 0x5A, np.uint8))
        self.status.zero()

    def serial(self, ctx, joined=True, stream=None):
        """rbc_dev_verify then rbc_dev_interpolate(leaves_verified = 1)."""
        c = self.case
        ctx.dev_verify(stream, c.count, self.shards, c.spitch, None, c.S, self.branches, self.roots, self.present,
                       self.valid, self.leaves)
        ctx.dev_interpolate(stream, c.count, self.shards, c.spitch, None, c.S, self.valid, self.leaves, 1, self.roots,
                            self.values if joined else None, c.vpitch if joined else 0, self.digests, self.status)

    def rx_batch(self, ctx, joined=True):
        c = self.case
        return ctx.rx_batch(c.count, self.shards, c.spitch, None, c.S, self.branches, self.roots, self.present,
                            self.valid, self.leaves, self.values if joined else None, c.vpitch if joined else 0,
                            self.digests, self.status)

    def read_status(self):
        return self.status.download().view(np.int32).copy()

    def read(self):
        c = self.case
        I, n = c.count, c.n
        return dict(rows=self.shards.download().reshape(I, n, c.spitch)[:, :, : c.S].copy(),
                    valid=self.valid.download().reshape(I, n).copy(),
                    leaves=self.leaves.download().reshape(I, n, 32).copy(),
                    values=self.values.download().reshape(I, c.vpitch).copy(),
                    digests=self.digests.download().reshape(I, 32).copy(),
                    status=self.read_status())


def check_against_oracle(case, got, joined=True):
    """Every row, valid byte, leaf, status, and for the delivered instances the
    digest, the joined value and its zero tail up to the pitch."""
    c = case
    assert np.array_equal(got["status"], c.want_status), (got["status"], c.want_status)
    assert np.array_equal(got["valid"], c.want_valid)
    assert np.array_equal(got["rows"], c.want_rows), np.argwhere((got["rows"] != c.want_rows).any(axis=2))[:8]
    assert np.array_equal(got["leaves"], c.want_leaves()), "leaves"
    for i in range(c.count):
        if c.want_status[i] != 0:
            continue
        st, val, dig = c.want_value_digest(i)
        assert st == 0
        assert bytes(got["digests"][i]) == dig, i
        assert np.array_equal(c.want_rows[i, : c.k].reshape(-1), val), i
        if joined:
            assert np.array_equal(got["values"][i, : c.k * c.S], val), i
            assert not got["values"][i, c.k * c.S:].any(), i  # the tail up to the pitch is zeroed
