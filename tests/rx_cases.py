"""Receiver-side test cases built on the host from the C oracle, for the
device API (rbc_dev_verify, rbc_dev_interpolate, rbc_dev_receive_step): one
small batch of committed values, the ECHO rows a receiver holds, and what
interpolate must leave in every buffer.  Used by test_gpu_decode_n128.py,
test_gpu_receive_step_overlap.py, test_gpu_receiver_contract.py,
test_gpu_dev_arena.py and test_gpu_regen_bodies.py (through dev_arena.py: the
same buffers as regions of one guarded allocation) and (the references against
each other, no device) test_rx_cases_host.py."""
import numpy as np

import rbc_ref

PATTERNS = ("none", "worst", "parity", "corrupt_data", "corrupt_parity", "byzantine")
# non-codewords with data rows absent: which k valid rows are used decides the re-encoding
GONE_PATTERNS = ("byzantine_data_gone", "kth_at")
# honest codewords with a chosen number of data rows absent (test_gpu_regen_bodies.py)
COUNT_PATTERNS = ("data_missing",)
VALUE_FILL, DIGEST_FILL = 0xA5, 0x5A  # DevCase's prefill of values / digests


def round_up(x, a):
    return (x + a - 1) // a * a


def reencode_from(n, k, rows, used):
    """The full re-encoding (klauspost Reconstruct) from the k rows `used` of
    rows [n][S] alone: every other row is handed over as absent."""
    import rbc_oracle as orc
    assert len(used) == k
    keep = set(int(j) for j in used)
    shards = [rows[j].copy() if j in keep else None for j in range(n)]
    orc.Encoder(k, n - k).reconstruct(shards)
    return np.stack(shards)


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
      byzantine_data_gone
                      random rows committed, every ECHO verifies; m data rows
                      (1 <= m <= f) and f - m parity rows absent.  The rows after
                      interpolate are the re-encoding of the first k valid rows
                      by index (another k-subset gives other rows); status -8.
      kth_at          as byzantine_data_gone, with the present set built so that
                      the k-th valid index is exactly `pos` (k-1 <= pos < n-1) and
                      at least one valid row lies above it: those are unused and
                      are replaced by the re-encoding.  `honest` names instances
                      that are pattern `worst` instead.
      data_missing    instance i misses exactly missing[i] data rows, at random
                      positions, and holds every parity row.
    byz / corrupt: instance indices that get the byzantine / corrupt_data
    treatment on top of `pattern` (the receive-step test mixes them).
    lens: per-instance shard lengths (S and count may then be None): the pitch
    comes from the longest, B_i = k*S_i - min(3, k-1) per instance.
    too_few: instances (honest codewords) that receive exactly k-1 ECHOs, all of
    which verify: status -3, only the received rows [0, S_i) are specified.
    dirty_pads: receiver_rows() leaves non-zero bytes in [S_i, spitch) of every
    received row too; every want_* is the same as without.
    """

    def __init__(self, n, f, S, count, pattern, seed, byz=None, corrupt=None, *, lens=None, too_few=None,
                 dirty_pads=False, pos=None, honest=None, missing=None):
        assert pattern in PATTERNS + GONE_PATTERNS + COUNT_PATTERNS
        rng = np.random.default_rng(seed)
        k = n - 2 * f
        self.ragged = lens is not None
        if self.ragged:
            assert S in (None, max(lens)) and count in (None, len(lens))
            S, count = max(lens), len(lens)
        self.lens = np.array(lens if self.ragged else [S] * count, np.uint32)
        self.n, self.f, self.k, self.S, self.count = n, f, k, S, count
        self.pattern, self.dirty_pads = pattern, dirty_pads
        self.B = k * S - min(3, k - 1)  # S = ceil(B / k), the last data row zero padded
        self.spitch = round_up(S, 64)
        self.vpitch = round_up(k * S, 16) + 16  # a tail to be zeroed
        self.depth = max(int(np.ceil(np.log2(n))), 0)
        byz = set(range(count) if pattern == "byzantine" else (byz or ()))
        corrupt = set(corrupt or ())
        self.too_few = set(too_few or ())
        honest = set(honest or ())
        assert self.too_few <= set(range(count)) and honest <= set(range(count))
        if pattern == "kth_at":
            assert pos is not None and k - 1 <= pos < n - 1
        if pattern == "data_missing":
            assert len(missing) == count and all(0 <= m <= min(k, n - k) for m in missing)
        if dirty_pads:  # room for the partial dword's pad bytes and one whole lane past S_i
            assert all(self.spitch - round_up(int(s), 4) >= 4 for s in self.lens)
        d = max(self.depth, 1)
        self.rows_in = np.zeros((count, n, S), np.uint8)  # the committed rows (what honest ECHOs carry)
        self.want_rows = np.zeros((count, n, S), np.uint8)  # every row after interpolate
        self.roots = np.zeros((count, 32), np.uint8)
        self.branches = np.zeros((count, n, d, 32), np.uint8)
        self.present = np.ones((count, n), np.uint8)
        self.bad = np.full(count, -1)  # the corrupted received row
        self.want_status = np.zeros(count, np.int32)
        self.changed = [[] for _ in range(count)]  # valid rows the re-encoding replaces
        self.gone = []  # the instances whose re-encoding depends on which k valid rows are used
        for i in range(count):
            Si = int(self.lens[i])
            value = rng.integers(0, 256, k * Si - min(3, k - 1), dtype=np.uint8)
            shards, root, br, _ = rbc_ref.encode_commit(n, f, value)
            pat = "byzantine" if i in byz else ("corrupt_data" if i in corrupt else pattern)
            if i in honest:
                pat = "worst"
            if i in self.too_few:
                pat = "too_few"
            data, par = np.arange(k), np.arange(k, n)
            if pat == "none":
                absent = []
            elif pat == "worst":
                absent = rng.permutation(data)[:f]
            elif pat == "parity":
                absent = rng.permutation(par)[:f]
            elif pat == "data_missing":
                absent = rng.permutation(data)[:missing[i]]
            elif pat == "corrupt_data":
                absent = rng.permutation(n)[:f]
            elif pat == "corrupt_parity":
                absent = rng.permutation(par)[:f]
            elif pat == "too_few":
                absent = rng.permutation(n)[k - 1:]
            elif pat == "byzantine_data_gone":
                m = int(rng.integers(1, f + 1))
                absent = np.concatenate([rng.permutation(data)[:m], rng.permutation(par)[:f - m]])
            elif pat == "kth_at":
                above = np.arange(pos + 1, n)
                held = above[rng.random(len(above)) < 0.5]
                if len(held) == 0:
                    held = above[-1:]
                here = np.concatenate([rng.permutation(pos)[:k - 1], [pos], held])
                absent = np.setdiff1d(np.arange(n), here)
            else:
                absent = rng.permutation(par)[:f]
            self.present[i, absent] = 0
            rec = np.flatnonzero(self.present[i])
            if pat == "corrupt_data":
                self.bad[i] = int(rng.choice(rec[rec < k]))
            elif pat == "corrupt_parity":
                self.bad[i] = int(rng.choice(rec[rec >= k]))
            if pat == "too_few":
                assert len(rec) == k - 1
                self.want_status[i] = -3
            if pat == "byzantine" or pat in GONE_PATTERNS:
                rows = shards.copy()
                if pat in GONE_PATTERNS or i % 2 == 0:
                    rows = rng.integers(0, 256, (n, Si), dtype=np.uint8)
                else:
                    j = int(rng.choice(rec[rec >= k]))
                    rows[j, int(rng.integers(0, Si))] ^= 0x21
                # the commitment is over the rows as they are
                _, root, br = commit_rows(n, rows)
                if pat == "byzantine":
                    # the re-encoding of the (all received) data rows is what interpolate leaves
                    want, _, _, _ = rbc_ref.encode_commit(n, f, np.ascontiguousarray(rows[:k]).reshape(-1))
                else:
                    want = reencode_from(n, k, rows, rec[:k])
                    self.gone.append(i)
                    if pat == "kth_at":
                        assert rec[k - 1] == pos and len(rec) > k
                self.changed[i] = [int(j) for j in rec if not np.array_equal(rows[j], want[j])]
                assert self.changed[i]
                if pat == "kth_at":  # the valid rows above pos are unused: replaced
                    assert any(j > pos for j in self.changed[i])
                self.want_status[i] = -8
                shards = rows
            else:
                want = shards
            self.rows_in[i, :, :Si], self.want_rows[i, :, :Si] = shards, want
            self.roots[i] = np.frombuffer(root, np.uint8)
            self.branches[i, :, : self.depth] = br
        self.want_valid = self.present.copy()
        for i in np.flatnonzero(self.bad >= 0):
            self.want_valid[i, self.bad[i]] = 0
        # the rows (and their leaves) that are specified after the call: all of
        # them, but for a too-few instance only the received ones
        self.specified = np.ones((count, n), bool)
        for i in self.too_few:
            self.specified[i] = self.present[i] == 1
        self._rows, self._leaves = {}, None

    def receiver_rows(self, seed=5):
        """[count][n][spitch]: received rows in place, zero padded to the pitch
        (seeded non-zero bytes there with dirty_pads; the corrupted one with a
        flipped byte); absent rows are garbage, their pads included.  The same
        read-only array on every call."""
        if seed in self._rows:
            return self._rows[seed]
        buf = np.random.default_rng(seed).integers(0, 256, (self.count, self.n, self.spitch), dtype=np.uint8)
        buf[self.present == 1] = 0
        if self.dirty_pads:  # every pad byte non-zero: the partial dword's and all whole lanes past S_i
            pad = np.random.default_rng(seed + 1).integers(1, 256, buf.shape, dtype=np.uint8)
            buf[self.present == 1] = pad[self.present == 1]
        for i in range(self.count):
            Si = int(self.lens[i])
            buf[i, :, :Si] = np.where(self.present[i, :, None] == 1, self.rows_in[i, :, :Si], buf[i, :, :Si])
            if self.bad[i] >= 0:
                buf[i, self.bad[i], Si // 2] ^= 0x40
        buf.flags.writeable = False
        self._rows[seed] = buf
        return buf

    def want_leaves(self):
        if self._leaves is None:
            out = np.zeros((self.count, self.n, 32), np.uint8)
            for i in range(self.count):
                for j in range(self.n):
                    out[i, j] = np.frombuffer(rbc_ref.sha256(self.want_rows[i, j, : self.lens[i]]), np.uint8)
            out.flags.writeable = False
            self._leaves = out
        return self._leaves

    def want_value_digest(self, i):
        """The C oracle's interpolate over what the receiver holds (status 0 only)."""
        buf = self.receiver_rows()[i, :, : self.lens[i]]
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
        for lvl, node in enumerate(com["branches"][j]):  # an empty level-0 sibling (n odd) stays zero
            if node:
                br[j, lvl] = np.frombuffer(node, np.uint8)
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
        # ragged: the device uint32 array passed as shard_lens, with uniform_shard_len = 0
        self.lens = mb(I * 4) if c.ragged else None
        self.ulen = 0 if c.ragged else c.S
        self.reset()

    def reset(self):
        c = self.case
        self.shards.upload(c.receiver_rows())
        self.branches.upload(c.branches)
        self.roots.upload(c.roots)
        self.present.upload(c.present)
        self.valid.upload(np.full(c.count * c.n, 0xCC, np.uint8))
        self.leaves.upload(np.full(c.count * c.n * 32, 0xDD, np.uint8))
        self.values.upload(np.full(c.count * c.vpitch, VALUE_FILL, np.uint8))
        self.digests.upload(np.full(c.count * 32, DIGEST_FILL, np.uint8))
        self.status.zero()
        if self.lens is not None:
            self.lens.upload(c.lens)

    def serial(self, ctx, joined=True, stream=None):
        """rbc_dev_verify then rbc_dev_interpolate(leaves_verified = 1)."""
        c = self.case
        ctx.dev_verify(stream, c.count, self.shards, c.spitch, self.lens, self.ulen, self.branches, self.roots,
                       self.present, self.valid, self.leaves)
        ctx.dev_interpolate(stream, c.count, self.shards, c.spitch, self.lens, self.ulen, self.valid, self.leaves, 1,
                            self.roots, self.values if joined else None, c.vpitch if joined else 0, self.digests,
                            self.status)

    def rx_batch(self, ctx, joined=True):
        c = self.case
        return ctx.rx_batch(c.count, self.shards, c.spitch, self.lens, self.ulen, self.branches, self.roots,
                            self.present, self.valid, self.leaves, self.values if joined else None,
                            c.vpitch if joined else 0, self.digests, self.status)

    def read_status(self):
        return self.status.download().view(np.int32).copy()

    def read(self):
        """rows: bytes [0, S) of every row; pitch_rows: the same rows to the pitch."""
        c = self.case
        I, n = c.count, c.n
        full = self.shards.download().reshape(I, n, c.spitch)
        return dict(rows=full[:, :, : c.S].copy(),
                    pitch_rows=full,
                    valid=self.valid.download().reshape(I, n).copy(),
                    leaves=self.leaves.download().reshape(I, n, 32).copy(),
                    values=self.values.download().reshape(I, c.vpitch).copy(),
                    digests=self.digests.download().reshape(I, 32).copy(),
                    status=self.read_status())


def check_against_oracle(case, got, joined=True, prefill=None):
    """Every specified row on [0, S_i), valid byte, leaf and status; the zero
    pad [S_i, spitch) of every regenerated row; for the delivered instances the
    digest, the joined value and (uniform length) its zero tail up to the pitch;
    for a too-few instance the untouched prefill of its value and digest
    (DevCase's constants, or the arrays prefill["values"] / prefill["digests"])."""
    c = case
    fill = prefill or dict(values=np.full_like(got["values"], VALUE_FILL),
                           digests=np.full_like(got["digests"], DIGEST_FILL))
    assert np.array_equal(got["status"], c.want_status), (got["status"], c.want_status)
    assert np.array_equal(got["valid"], c.want_valid)
    want_leaves = c.want_leaves()
    for i in range(c.count):
        Si, spec = int(c.lens[i]), c.specified[i]
        same = (got["rows"][i, :, :Si] == c.want_rows[i, :, :Si]).all(axis=1)
        assert same[spec].all(), (i, np.flatnonzero(spec & ~same)[:8])
        assert np.array_equal(got["leaves"][i, spec], want_leaves[i, spec]), ("leaves", i)
        if c.want_status[i] == -3:  # skipped by every kernel after the prepare
            assert np.array_equal(got["values"][i], fill["values"][i]), i
            assert np.array_equal(got["digests"][i], fill["digests"][i]), i
            continue
        regen = c.want_valid[i] == 0  # absent, or the corrupted ECHO
        assert not got["pitch_rows"][i, regen, Si:].any(), ("pad of a regenerated row", i)
        if c.want_status[i] != 0:
            continue
        st, val, dig = c.want_value_digest(i)
        assert st == 0
        assert bytes(got["digests"][i]) == dig, i
        assert np.array_equal(c.want_rows[i, : c.k, :Si].reshape(-1), val), i
        if joined:
            assert np.array_equal(got["values"][i, : c.k * Si], val), i
            if not c.ragged:  # ragged: bytes past k*S_i are unspecified
                assert not got["values"][i, c.k * c.S:].any(), i  # the tail up to the pitch is zeroed


def specified(case, got, joined=True):
    """What of `got` the API specifies, everything else zeroed: two runs of one
    case (another form, another codec, dirty pads) must agree on all of it."""
    c = case
    out = {key: got[key].copy() for key in ("rows", "valid", "leaves", "status", "digests")}
    out["values"] = got["values"].copy() if joined else np.zeros_like(got["values"])
    for i in range(c.count):
        Si = int(c.lens[i])
        out["rows"][i, :, Si:] = 0
        out["rows"][i, ~c.specified[i]] = 0
        out["leaves"][i, ~c.specified[i]] = 0
        if got["status"][i] != 0:
            out["digests"][i] = 0
            out["values"][i] = 0
        out["values"][i, c.k * Si:] = 0
    return out


# ---- the cases of test_gpu_receiver_contract.py ------------------------------
# One table, so that test_rx_cases_host.py checks on the host exactly the cases
# the device tests run.  id -> (positional arguments, keyword arguments).
RAGGED_128 = (4, 5, 63, 64, 65, 252, 256, 260, 763, 2049, 2052)
RAGGED_SMALL = (1, 4, 5, 63, 64, 65, 257)
FEW_A, FEW_B = (0, 5, 10), (1, 5, 9)  # first / middle / last, then another set
DIRTY_GEOMS = [(128, 42, 5), (128, 42, 252), (128, 42, 257), (128, 42, 763), (256, 85, 257), (16, 5, 257),
               (37, 12, 257)]
DIRTY_PATTERNS = PATTERNS + ("byzantine_data_gone",)
KTH_POS = {(128, 42): (43, 62, 63, 64, 65, 126), (256, 85): (85, 127, 128, 129, 191, 192, 193, 254),
           (64, 21): (21, 62)}
CONTRACT = {}


def _add(cid, *args, **kw):
    assert cid not in CONTRACT
    CONTRACT[cid] = (args, kw)


for _p in ("worst", "corrupt_data", "byzantine"):
    _add(f"ragged-128-{_p}", 128, 42, None, None, _p, 7100 + len(CONTRACT), lens=RAGGED_128)
for _n, _f in [(4, 1), (16, 5), (64, 21), (256, 85)]:
    _add(f"ragged-{_n}", _n, _f, None, None, "corrupt_data", 7200 + _n, lens=RAGGED_SMALL)
for _n, _f in [(128, 42), (64, 21)]:
    for _p in ("worst", "byzantine"):
        for _b, _few in (("a", FEW_A), ("b", FEW_B)):
            _add(f"few-{_n}-{_p}-uniform-{_b}", _n, _f, 260, 11, _p, 7300 + len(CONTRACT), too_few=_few)
            _add(f"few-{_n}-{_p}-ragged-{_b}", _n, _f, None, None, _p, 7300 + len(CONTRACT), lens=RAGGED_128,
                 too_few=_few)
for _g, (_n, _f, _S) in enumerate(DIRTY_GEOMS):
    for _q, _p in enumerate(DIRTY_PATTERNS):
        for _dirty in (False, True):  # one seed: the same case but for the pads
            _add(f"pads-{_n}-{_S}-{_p}-{'dirty' if _dirty else 'clean'}", _n, _f, _S, 4, _p, 7400 + 100 * _g + _q,
                 dirty_pads=_dirty)
for (_n, _f), _poss in KTH_POS.items():
    for _pos in _poss:
        _add(f"kth-{_n}-{_pos}", _n, _f, 13, 8, "kth_at", 8200 + _n + _pos, pos=_pos, honest=(0,))

_built = {}


def contract_case(cid):
    """The Case of id `cid`, built once per process; treat it as read-only."""
    if cid not in _built:
        args, kw = CONTRACT[cid]
        _built[cid] = Case(*args, **kw)
    return _built[cid]
