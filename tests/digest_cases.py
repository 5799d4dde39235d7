"""Cases with exactly one wrong bit in one 32-bit word of one compared digest
(or one wrong byte of one compared row), built on the host for
test_gpu_digest_words.py, and the Merkle builder they share.  Every expected
verdict comes from the C oracle (rbc_ref.verify_many, rbc_ref.interpolate),
never from the device; test_mutant_table.py checks the builder and the
references against each other without a device."""
import hashlib

import numpy as np

import rbc_ref

ROOT_MISMATCH = -8


def depth_of(n):
    d = 0
    while (1 << d) < n:
        d += 1
    return d


def round_up(x, a):
    return (x + a - 1) // a * a


def flip_word(digest, w, rng):
    """One bit of 32-bit word w of the 32-byte array `digest` flipped, in place."""
    digest[4 * w + int(rng.integers(0, 4))] ^= np.uint8(1 << int(rng.integers(0, 8)))


def flipped(digest, w, rng):
    out = np.frombuffer(bytes(digest), np.uint8).copy()
    flip_word(out, w, rng)
    return out.tobytes()


def build_tree(n, leaves, override=None):
    """The project's Merkle tree over n leaf hashes: a node is H(L || R) and an
    empty padding leaf contributes no bytes.  override: {(level, index): fn},
    the node's value replaced by fn(value) before its ancestors are hashed
    (level 0: a leaf hash).  -> (levels, root, branches [n][max(d,1)][32]);
    levels[l][v] is node v of level l (None: an empty leaf); branch entry
    (j, l) is node (j >> l) ^ 1 of level l, zero for an empty leaf."""
    d = depth_of(n)
    W = 1 << d
    override = override or {}
    levels = []
    for l in range(d + 1):
        if l == 0:
            lvl = [bytes(leaves[j]) if j < n else None for j in range(W)]
        else:
            prev = levels[-1]
            lvl = [hashlib.sha256((prev[2 * i] or b"") + (prev[2 * i + 1] or b"")).digest() for i in range(W >> l)]
        for (ol, ov), fn in override.items():
            if ol == l:
                lvl[ov] = fn(lvl[ov])
        levels.append(lvl)
    br = np.zeros((n, max(d, 1), 32), np.uint8)
    for j in range(n):
        for l in range(d):
            node = levels[l][(j >> l) ^ 1]
            if node is not None:
                br[j, l] = np.frombuffer(node, np.uint8)
    return levels, levels[d][0], br


def device_rows(case, seed=3):
    """[count][n][pitch] as a receiver holds them: present rows zero padded to
    the 64-byte pitch, absent rows garbage, their pads included."""
    buf = np.random.default_rng(seed).integers(0, 256, (case.count, case.n, round_up(case.S, 64)), dtype=np.uint8)
    buf[case.present == 1] = 0
    buf[:, :, : case.S] = np.where(case.present[:, :, None] == 1, case.rows, buf[:, :, : case.S])
    return buf


def leaf_hashes(rows):
    return [hashlib.sha256(bytes(r)).digest() for r in rows]


def commit(n, f, S, rng):
    """An honest commitment: rows [n][S], root, branches [n][d][32]."""
    k = n - 2 * f
    value = rng.integers(0, 256, k * S - min(3, k - 1), dtype=np.uint8)
    rows, root, br, _ = rbc_ref.encode_commit(n, f, value)
    return rows, root, br


# ---- ECHO verify: one wrong word in a root or in a branch entry -----------------
# kinds: root     the instance's root differs in word w: every row invalid
#        sib      one leaf's level-l entry differs: that leaf alone invalid
#        nonrep   the same, the leaf not being the first participant of its group
#        rep      the same, the leaf being the first participant of its group
#        all      every participant under one level-l node holds the same wrong entry
# A group is the leaves under a level-l node v with v even (under v's parent at
# l = 0, where a node is one leaf), so its first participant is the first one
# under v's parent too: the representative in both of merkle_path_kernel's forms.
class VerifyBatch:
    def __init__(self, n, f, S, cases, seed, masked_half=False):
        rng = np.random.default_rng(seed)
        self.n, self.f, self.S, self.cases = n, f, S, list(cases)
        d = self.depth = depth_of(n)
        I = self.count = len(self.cases)
        self.spitch = round_up(S, 64)
        self.rows = np.zeros((I, n, S), np.uint8)
        self.roots = np.zeros((I, 32), np.uint8)
        self.branches = np.zeros((I, n, max(d, 1), 32), np.uint8)
        self.present = np.ones((I, n), np.uint8)
        self.touched = [None] * I  # the leaves whose entry was altered
        for i, (kind, l, w) in enumerate(self.cases):
            rows, root, br = commit(n, f, S, rng)
            self.rows[i], self.branches[i, :, :d] = rows, br
            self.roots[i] = np.frombuffer(root, np.uint8)
            if masked_half and i % 2:
                self.present[i] = 0
                self.present[i, rng.permutation(n)[: n - f]] = 1
            pr = self.present[i]
            if kind == "root":
                flip_word(self.roots[i], w, rng)
                continue
            if kind == "sib":
                js = [int(rng.choice([j for j in np.flatnonzero(pr) if not (l == 0 and (j ^ 1) >= n)]))]
            else:
                span = 1 << max(l, 1)  # the group's leaves: [v << l, (v << l) + span)
                cands = []
                for v in range(0, (n + (1 << l) - 1) >> l, 2):
                    under = [j for j in range(v << l, min(n, (v << l) + span)) if pr[j]]
                    if len(under) >= 2 and (l > 0 or (pr[v] and v + 1 < n)):
                        cands.append(under)
                under = cands[int(rng.integers(0, len(cands)))]
                if kind == "rep":
                    js = under[:1]
                elif kind == "nonrep":
                    js = [int(rng.choice(under[1:]))]
                else:  # all: the participants under v itself
                    js = under if l > 0 else under[:1]
            honest = self.branches[i, js[0], l].copy()
            wrong = honest.copy()
            flip_word(wrong, w, rng)
            for j in js:
                assert np.array_equal(self.branches[i, j, l], honest)
                self.branches[i, j, l] = wrong
            self.touched[i] = js
        self.want_valid = self._oracle()
        for i, (kind, l, w) in enumerate(self.cases):  # the construction and the oracle agree
            want = np.zeros(n, np.uint8) if kind == "root" else self.present[i].copy()
            if kind != "root":
                want[self.touched[i]] = 0
            assert np.array_equal(self.want_valid[i], want), (i, kind, l, w)

    def _oracle(self):
        """The oracle's per-leaf walk over every (instance, leaf), and the present mask."""
        I, n = self.count, self.n
        inst = np.repeat(np.arange(I, dtype=np.int32), n)
        j = np.tile(np.arange(n, dtype=np.int32), I)
        _, ok = rbc_ref.verify_many(n, self.rows, self.branches[:, :, : self.depth], self.roots, inst, j, 1)
        return (ok.reshape(I, n) != 0).astype(np.uint8) & self.present

    def index(self, kind, l, w):
        return self.cases.index((kind, l, w))


def verify_cases(kinds, levels):
    out = [("root", -1, w) for w in range(8)]
    for kind in kinds:
        out += [(kind, l, w) for l in levels for w in range(8)]
    return out


WALK = dict(n=4, f=1, S=2048, cases=verify_cases(("sib",), range(2)), seed=5101)
PATH_KINDS = ("nonrep", "rep", "all")
EXACT = dict(n=16, f=5, S=13, cases=verify_cases(PATH_KINDS, range(4)), seed=5102)
SPEC = {n: dict(n=n, f=f, S=13, cases=verify_cases(PATH_KINDS, range(2, 8)), seed=5103 + n, masked_half=True)
        for n, f in ((256, 85), (200, 66))}

_built = {}


def built(key, make):
    """One build per process of a host-side batch; treat it as read-only."""
    if key not in _built:
        _built[key] = make()
    return _built[key]


# ---- the receive step's recheck ---------------------------------------------------
class RecheckRoots:
    """Honest instances at (n, f); instance w's expect_roots differs in word w
    once the ECHOs are verified (wrong_roots), the last instance's does not."""

    def __init__(self, n=16, f=5, S=13, seed=5201):
        rng = np.random.default_rng(seed)
        self.n, self.f, self.S, self.count = n, f, S, 9
        d = depth_of(n)
        I = self.count
        self.rows = np.zeros((I, n, S), np.uint8)
        self.roots = np.zeros((I, 32), np.uint8)
        self.branches = np.zeros((I, n, d, 32), np.uint8)
        self.present = np.zeros((I, n), np.uint8)
        for i in range(I):
            self.rows[i], root, self.branches[i] = commit(n, f, S, rng)
            self.roots[i] = np.frombuffer(root, np.uint8)
            self.present[i, rng.permutation(n)[: n - f]] = 1
        self.wrong_roots = self.roots.copy()
        for w in range(8):
            flip_word(self.wrong_roots[w], w, rng)
        # the oracle: interpolate against the root the caller expects now
        self.want_status = np.array([rbc_ref.interpolate(n, f, self.rows[i], self.present[i],
                                                         self.wrong_roots[i].tobytes())[0] for i in range(I)], np.int32)
        assert (self.want_status[:8] == ROOT_MISMATCH).all() and self.want_status[8] == 0


class ByzantineTrees:
    """Recheck case (b): for each level l and word w one instance whose tree
    holds, at one node (l, v), the honest value with one bit of word w flipped,
    its ancestors hashed over that; the ECHOs of every leaf outside v's subtree
    carry their branches in that tree, so all of them verify against its root
    R', the decode regenerates the subtree's rows, and the re-encoding's tree
    (the honest one) has another root: RBC_ERR_ROOT_MISMATCH."""

    def __init__(self, n=16, f=5, S=13, levels=range(4), seed=5301):
        rng = np.random.default_rng(seed)
        k = n - 2 * f
        d = depth_of(n)
        self.n, self.f, self.S = n, f, S
        self.cases = [(l, w) for l in levels for w in range(8)]
        I = self.count = len(self.cases)
        self.rows = np.zeros((I, n, S), np.uint8)
        self.roots = np.zeros((I, 32), np.uint8)
        self.honest_roots = np.zeros((I, 32), np.uint8)
        self.branches = np.zeros((I, n, d, 32), np.uint8)
        self.present = np.ones((I, n), np.uint8)
        self.node = [None] * I
        for i, (l, w) in enumerate(self.cases):
            rows, root, _ = commit(n, f, S, rng)
            v = int(rng.integers(0, (n + (1 << l) - 1) >> l))
            _, r2, br = build_tree(n, leaf_hashes(rows), {(l, v): lambda x, w=w: flipped(x, w, rng)})
            assert r2 != root
            self.rows[i], self.branches[i] = rows, br
            self.roots[i] = np.frombuffer(r2, np.uint8)
            self.honest_roots[i] = np.frombuffer(root, np.uint8)
            self.present[i, v << l: (v + 1) << l] = 0
            assert self.present[i].sum() >= k
            self.node[i] = (l, v)
        inst = np.repeat(np.arange(I, dtype=np.int32), n)
        j = np.tile(np.arange(n, dtype=np.int32), I)
        _, ok = rbc_ref.verify_many(n, self.rows, self.branches, self.roots, inst, j, 1)
        self.want_valid = (ok.reshape(I, n) != 0).astype(np.uint8) & self.present
        assert np.array_equal(self.want_valid, self.present)  # every ECHO sent verifies against R'
        self.want_status = np.array([rbc_ref.interpolate(n, f, self.rows[i], self.present[i],
                                                         self.roots[i].tobytes())[0] for i in range(I)], np.int32)

    def index(self, l, w):
        return self.cases.index((l, w))



# ---- GF compare lanes ---------------------------------------------------------------
class NonCodewords:
    """One instance per byte b of [0, S): parity row `pos` of an honest
    encoding altered at byte b before the Merkle build, so every ECHO proves;
    all n rows are present, so the altered row is valid but unused.  The
    oracle's interpolate gives the status (a root mismatch); interpolate leaves
    the re-encoding (want_rows) in every row."""

    def __init__(self, n, f, pos, S=23, seed=5401):
        rng = np.random.default_rng(seed + 1000 * n + pos)
        self.n, self.f, self.S, self.pos = n, f, S, pos
        d = depth_of(n)
        I = self.count = S
        self.rows = np.zeros((I, n, S), np.uint8)
        self.want_rows = np.zeros((I, n, S), np.uint8)
        self.roots = np.zeros((I, 32), np.uint8)
        self.branches = np.zeros((I, n, d, 32), np.uint8)
        self.present = np.ones((I, n), np.uint8)
        assert n - 2 * f <= pos < n
        for b in range(S):
            rows, _, _ = commit(n, f, S, rng)
            self.want_rows[b] = rows
            rows = rows.copy()
            rows[pos, b] ^= np.uint8(rng.integers(1, 256))
            _, root, br = build_tree(n, leaf_hashes(rows))
            self.rows[b], self.branches[b] = rows, br
            self.roots[b] = np.frombuffer(root, np.uint8)
        self.want_status = np.array([rbc_ref.interpolate(n, f, self.rows[i], self.present[i],
                                                         self.roots[i].tobytes())[0] for i in range(I)], np.int32)



# geometry id -> (n, f, codec): the FFT decode's pipelined compare, its prefetch
# compare (N = 128), and gf_rows_kernel's compare mode under the matrix codec
GF_GEOMS = {"fft-16": (16, 5, "fft"), "fft-128": (128, 42, "fft"), "matrix-7": (7, 2, "matrix"),
            "matrix-16": (16, 5, "matrix")}
