"""Every 32-bit word of every digest compare on the receive side, and every
byte lane of the decode's row compares.

The kernels compare 32-byte digests component by component (two uint4, or
eight words in a loop) and rows dword by dword or 16 bytes at a time.  In each
case here ONE bit is flipped in word w of ONE compared operand, for every w in
0..7 (for the row compares: one byte b, for every b of the row), in an instance
of its own, and the verdict -- valid[] or status -- must be the C oracle's
(tests/digest_cases.py builds the cases and asks the oracle; nothing expected
comes from the device).  A compare that skipped one word would pass every
other test of the suite with good odds; tests/test_gpu_mutants.py shows that it
fails here.

  walk form          sha_rows_kernel<true> (rbc_dev_verify) and sha_rx_kernel
                     (rbc_dev_receive_step) at (4,1), S = 2048: root words,
                     sibling words at each level
  shared-path form   merkle_path_kernel's exact levels at (16,5) and its
                     speculative top levels at (256,85) and (200,66), S = 13:
                     a non-representative leaf's entry, the representative's,
                     an entry all leaves under a node agree on, the root
  recheck            expect_roots wronged after the verify (node-reuse and
                     full), and a tree with one wrong node that every ECHO
                     proves against (merkle_recheck_kernel's entry compare)
  ECHO unmarshal     the instance's root against the message's, both codecs
  GF compare lanes   a non-codeword commitment whose altered parity row is
                     valid but unused, at every byte, on the FFT decode's
                     pipelined and prefetch compares and gf_rows_kernel's
"""
import numpy as np
import pytest

import digest_cases as dc
import wire_bin as wb
from test_gpu_wire_bin import CANARY, canaried, checked, dev, flat, pack

pytestmark = pytest.mark.gpu

WORDS = range(8)
OTHER_ROOT = 2


class Dev:
    """A case's receiver buffers on the device, each its own allocation."""

    def __init__(self, gpu, case):
        c = self.case = case
        I, n = c.count, c.n
        self.gpu, self.k = gpu, n - 2 * c.f
        self.spitch = dc.round_up(c.S, 64)
        self.vpitch = dc.round_up(self.k * c.S, 16) + 16
        mb = gpu.DeviceBuffer
        self.shards, self.branches, self.roots = mb(I * n * self.spitch), mb(c.branches.nbytes), mb(I * 32)
        self.present, self.valid, self.leaves = mb(I * n), mb(I * n), mb(I * n * 32)
        self.values, self.digests, self.status = mb(I * self.vpitch), mb(I * 32), mb(I * 4)
        self.shards.upload(dc.device_rows(c))
        self.branches.upload(c.branches)
        self.roots.upload(c.roots)
        self.present.upload(c.present)
        self.valid.upload(np.full(I * n, 0xCC, np.uint8))
        self.leaves.upload(np.full(I * n * 32, 0xDD, np.uint8))
        self.values.upload(np.full(I * self.vpitch, 0xA5, np.uint8))
        self.digests.upload(np.full(I * 32, 0x5A, np.uint8))
        self.status.zero()

    def sync(self):
        self.gpu.rbc.lib.rbc_device_sync(0)

    def verify(self, ctx, masked=True):
        c = self.case
        ctx.dev_verify(None, c.count, self.shards, self.spitch, None, c.S, self.branches, self.roots,
                       self.present if masked else None, self.valid, self.leaves)

    def interpolate(self, ctx):
        c = self.case
        ctx.dev_interpolate(None, c.count, self.shards, self.spitch, None, c.S, self.valid, self.leaves, 1, self.roots,
                            self.values, self.vpitch, self.digests, self.status)

    def batch(self, ctx):
        c = self.case
        return ctx.rx_batch(c.count, self.shards, self.spitch, None, c.S, self.branches, self.roots, self.present,
                            self.valid, self.leaves, self.values, self.vpitch, self.digests, self.status)

    def run(self, ctx, mode, roots_after_verify=None):
        """ECHO verify, then the decode and its recheck: "oneshot"
        (rbc_dev_verify + rbc_dev_interpolate) or the receive step with the
        "reuse" / "full" recheck.  roots_after_verify: what the caller's roots
        hold once the ECHOs are verified (expect_roots of the recheck)."""
        if mode == "oneshot":
            self.verify(ctx)
            self.sync()
            if roots_after_verify is not None:
                self.roots.upload(roots_after_verify)
            self.interpolate(ctx)
        else:
            ctx.set_recheck(mode)
            b = self.batch(ctx)
            ctx.dev_receive_step(None, b, None)
            self.sync()
            if roots_after_verify is not None:
                self.roots.upload(roots_after_verify)
            ctx.dev_receive_step(None, None, b)
        self.sync()
        return self.read()

    def read_valid(self):
        return self.valid.download().reshape(self.case.count, self.case.n).copy()

    def read(self):
        c = self.case
        return dict(valid=self.read_valid(), status=self.status.download().view(np.int32).copy(),
                    rows=self.shards.download().reshape(c.count, c.n, self.spitch)[:, :, : c.S].copy())


_results = {}


def once(key, make):
    """One device run per process and key: the cases of a batch share it."""
    if key not in _results:
        _results[key] = make()
    return _results[key]


def _same_valid(case, got, i):
    assert np.array_equal(got[i], case.want_valid[i]), (case.cases[i], got[i], case.want_valid[i])


# ---- walk form ------------------------------------------------------------------------
def _walk(gpu, via):
    case = dc.built("walk", lambda: dc.VerifyBatch(**dc.WALK))

    def run():
        ctx = gpu.Context(case.n, case.f)
        assert ctx.verify_form(case.S) == "walk"
        d = Dev(gpu, case)
        if via == "verify":  # every row of every instance: no work list
            d.verify(ctx, masked=False)
            d.sync()
            return d.read_valid()
        b = d.batch(ctx)
        ctx.dev_receive_step(None, b, None)
        d.sync()
        got = d.read_valid()
        ctx.dev_receive_step(None, None, b)
        d.sync()
        return got
    return case, once(("walk", via), run)


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("via", ["verify", "step"])
def test_walk_root_word(gpu, via, w):
    case, got = _walk(gpu, via)
    i = case.index("root", -1, w)
    assert not case.want_valid[i].any()
    _same_valid(case, got, i)


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("l", range(2))
@pytest.mark.parametrize("via", ["verify", "step"])
def test_walk_sibling_word(gpu, via, l, w):
    case, got = _walk(gpu, via)
    i = case.index("sib", l, w)
    assert case.want_valid[i].sum() == case.n - 1
    _same_valid(case, got, i)


# ---- shared-path form -----------------------------------------------------------------
def _path(gpu, key, spec):
    case = dc.built(key, lambda: dc.VerifyBatch(**spec))

    def run():
        ctx = gpu.Context(case.n, case.f)
        assert ctx.verify_form(case.S) == "shared_path"
        d = Dev(gpu, case)
        d.verify(ctx)
        d.sync()
        return d.read_valid()
    return case, once(key, run)


@pytest.mark.parametrize("w", WORDS)
def test_shared_path_exact_root_word(gpu, w):
    case, got = _path(gpu, "exact", dc.EXACT)
    _same_valid(case, got, case.index("root", -1, w))


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("kind", dc.PATH_KINDS)
def test_shared_path_exact_entry_word(gpu, kind, w):
    case, got = _path(gpu, "exact", dc.EXACT)
    for l in range(4):
        _same_valid(case, got, case.index(kind, l, w))


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("n", sorted(dc.SPEC))
def test_shared_path_spec_root_word(gpu, n, w):
    case, got = _path(gpu, ("spec", n), dc.SPEC[n])
    _same_valid(case, got, case.index("root", -1, w))


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("kind", dc.PATH_KINDS)
@pytest.mark.parametrize("n", sorted(dc.SPEC))
def test_shared_path_spec_entry_word(gpu, n, kind, w):
    case, got = _path(gpu, ("spec", n), dc.SPEC[n])
    assert case.present[1::2].sum() == (case.count // 2) * (case.n - case.f)  # half the instances masked
    for l in range(2, 8):
        _same_valid(case, got, case.index(kind, l, w))


# ---- the recheck ----------------------------------------------------------------------
@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("mode", ["reuse", "full"])
def test_recheck_expect_root_word(gpu, mode, w):
    """expect_roots word w wronged after the verify: merkle_recheck_kernel's
    root_same (reuse) and merkle_kernel<true>'s root compare (full)."""
    case = dc.built("recheck-roots", dc.RecheckRoots)
    got = once(("recheck-roots", mode),
               lambda: Dev(gpu, case).run(gpu.Context(case.n, case.f), mode, roots_after_verify=case.wrong_roots))
    assert np.array_equal(got["valid"], case.present)
    assert got["status"][8] == case.want_status[8] == 0  # the instance whose root was left alone
    assert got["status"][w] == case.want_status[w] == dc.ROOT_MISMATCH, (w, got["status"])


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("l", range(4))
@pytest.mark.parametrize("mode", ["reuse", "full", "oneshot"])
def test_recheck_byzantine_node_word(gpu, mode, l, w):
    """A tree whose node (l, v) differs from the hash of its children in word
    w; the ECHOs of every leaf outside v's subtree prove against its root."""
    case = dc.built("byz-trees", dc.ByzantineTrees)
    got = once(("byz-trees", mode), lambda: Dev(gpu, case).run(gpu.Context(case.n, case.f), mode))
    i = case.index(l, w)
    assert np.array_equal(got["valid"][i], case.want_valid[i]) and case.want_valid[i].sum() == case.n - (1 << l)
    assert np.array_equal(got["rows"][i], case.rows[i])  # the subtree's rows are regenerated
    assert got["status"][i] == case.want_status[i] == dc.ROOT_MISMATCH, (l, w, case.node[i], got["status"])


# ---- ECHO unmarshal -------------------------------------------------------------------
def _echo(gpu, codec):
    n, f, S, pitch = 7, 2, 13, 64
    rng = np.random.default_rng(5501)
    from cleisthenes_amd import protocol
    ctx = gpu.Context(n, f)
    ctx.set_wire_codec(codec)
    d = ctx.depth
    count = 9  # instance w expects a root that differs in word w; the last one the message's
    msgs, roots, want = [], np.zeros((count, 32), np.uint8), []
    idx = np.array([(3 * i) % n for i in range(count)], np.uint8)  # leaf 6 (no level-0 sibling) among them
    for i in range(count):
        rows, root, br = dc.commit(n, f, S, rng)
        j = int(idx[i])
        fb = flat(n, j, br[j])
        msgs.append(wb.message(wb.ECHO, root, fb, rows[j].tobytes()) if codec == "binary" else
                    protocol.pb_encode(protocol.ECHO, protocol.json_encode_val(root, fb, rows[j].tobytes())))
        roots[i] = np.frombuffer(root, np.uint8)
        if i < 8:
            dc.flip_word(roots[i], i, rng)
        want.append((rows[j], br[j], root))
    ring, offs, lens = pack(gpu, msgs)
    sizes = {"shards": count * n * pitch, "branches": count * n * d * 32, "present": count * n, "status": count * 4}
    out = {name: canaried(gpu, size) for name, size in sizes.items()}
    ctx.dev_unmarshal_echo(None, count, count, dev(gpu, ring), dev(gpu, offs), dev(gpu, lens),
                           dev(gpu, np.arange(count, dtype=np.uint32)), dev(gpu, idx), dev(gpu, roots), None, S,
                           out["shards"], pitch, out["branches"], out["present"], out["status"])
    gpu.rbc.lib.rbc_device_sync(0)
    got = {name: checked(out[name], size, name) for name, size in sizes.items()}
    ctx.close()
    return dict(status=got["status"].view(np.int32), shards=got["shards"].reshape(count, n, pitch),
                branches=got["branches"].reshape(count, n, d * 32), present=got["present"].reshape(count, n),
                idx=idx, want=want, roots=roots, S=S)


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("codec", ["json", "binary"])
def test_unmarshal_echo_root_word(gpu, codec, w):
    """root_diff: a message whose root differs from its instance's in word w
    alone is WIRE_OTHER_ROOT and leaves its slot as it was."""
    r = once(("echo", codec), lambda: _echo(gpu, codec))
    assert bytes(r["roots"][w]) != r["want"][w][2]  # the host's compare of the 32 bytes
    assert r["status"][w] == OTHER_ROOT
    assert (r["shards"][w] == CANARY).all() and (r["branches"][w] == CANARY).all() and (r["present"][w] == CANARY).all()
    # the message whose root is its instance's is decoded into its slot
    row, br, root = r["want"][8]
    j = int(r["idx"][8])
    assert bytes(r["roots"][8]) == root and r["status"][8] == 0 and r["present"][8, j] == 1
    assert np.array_equal(r["shards"][8, j, : r["S"]], row) and np.array_equal(r["branches"][8, j], br.reshape(-1))


# ---- GF compare lanes -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["k", "last"])
@pytest.mark.parametrize("mode", ["reuse", "full", "oneshot"])
@pytest.mark.parametrize("geom", sorted(dc.GF_GEOMS))
def test_gf_compare_byte(gpu, geom, mode, which):
    """A commitment over a non-codeword: parity row k (or n-1) altered at byte
    b, every ECHO valid, every row present.  For every b the status is the
    oracle's (a root mismatch) and the altered row is overwritten with the
    re-encoding of the data rows."""
    n, f, codec = dc.GF_GEOMS[geom]
    pos = n - 2 * f if which == "k" else n - 1
    case = dc.built(("gf", n, f, pos), lambda: dc.NonCodewords(n, f, pos))
    assert case.count == case.S == 23 and (case.want_status == dc.ROOT_MISMATCH).all()
    ctx = gpu.Context(n, f)
    ctx.set_codec(codec)
    assert ctx.codec == codec
    got = Dev(gpu, case).run(ctx, mode)
    ctx.close()
    assert (got["valid"] == 1).all()
    for b in range(case.S):
        assert got["status"][b] == case.want_status[b], (b, got["status"])
        assert np.array_equal(got["rows"][b], case.want_rows[b]), (b, np.argwhere(got["rows"][b] != case.want_rows[b])[:4])
