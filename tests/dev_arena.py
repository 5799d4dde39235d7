"""A guarded device arena: every buffer of a device-API call carved out of one
allocation, with guard bytes around each, so that a store outside an output --
one lane, one 16-byte chunk, one column tile or one row past its end, or into
a const input -- is seen.  Separate allocations hide such a store in the
allocator's slack.

    arena = Arena(gpu, arena_bytes(sizes, guard), seed, guard=guard_for(row_pitch))
    shards = arena.carve("shards", count * n * pitch, "inout")   # an int device address
    arena.put("shards", rows)
    ... the call under test, then a device sync ...
    out = arena.check()     # guards and "in" regions untouched; -> the "out" / "inout" regions

The arena is filled with seeded random bytes (a constant fill would hide a
stray store of that constant).  Every region starts 256-byte aligned, as
separate allocations always have, and has exactly the size asked for.  A guard
of at least `guard` bytes lies before the first region, between every two and
after the last: `guard` is a multiple of 256, at least 4096, and by guard_for()
at least twice the largest row pitch of the case, so that an overrun of one
row, tile or record stays inside the arena's own allocation.

Arena(None, ..., buffer=HostBuffer) keeps the bytes in a numpy array instead:
tests/test_dev_arena_host.py checks the bookkeeping that way without a GPU.
"""
import numpy as np

ALIGN = 256
MIN_GUARD = 4096
KINDS = ("out", "in", "inout")


def round_up(x, a):
    return (x + a - 1) // a * a


def guard_for(row_pitch=0):
    """The guard size for a case whose largest row pitch (or record size) is row_pitch."""
    return max(MIN_GUARD, round_up(2 * int(row_pitch), ALIGN))


def arena_bytes(sizes, guard):
    """Bytes of an arena that holds regions of `sizes`, carved in that order."""
    at = guard
    for s in sizes:
        at = round_up(round_up(at, ALIGN) + int(s) + guard, ALIGN)
    return at


class HostBuffer:
    """A numpy-backed stand-in for DeviceBuffer: upload / download by offset,
    and a made-up 256-byte aligned base address."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.mem = np.zeros(self.nbytes, np.uint8)
        self.value = 0x7F0000000000

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert offset + a.nbytes <= self.nbytes
        self.mem[offset: offset + a.nbytes] = a

    def download(self, nbytes=None, offset=0):
        n = self.nbytes - offset if nbytes is None else nbytes
        return self.mem[offset: offset + n].copy()

    def poke(self, address, value):
        """What a device store of one byte at `address` would do."""
        self.mem[address - self.value] = value


class Arena:
    def __init__(self, gpu, nbytes, seed, guard=MIN_GUARD, buffer=None):
        assert guard % ALIGN == 0 and guard >= MIN_GUARD, guard
        self.nbytes, self.guard = int(nbytes), guard
        assert self.nbytes >= 2 * guard
        self.buf = (buffer or gpu.DeviceBuffer)(self.nbytes)
        self.base = self.buf.value
        assert self.base % ALIGN == 0
        # what every byte held before the call: the fill, then what put() uploaded
        self.before = np.random.default_rng(seed).integers(0, 256, self.nbytes, dtype=np.uint8)
        self.buf.upload(self.before)
        self.regions = {}  # name -> (start, end, kind), in carve (= address) order
        self._at = guard

    def carve(self, name, nbytes, kind):
        assert kind in KINDS and name not in self.regions and nbytes > 0
        start = round_up(self._at, ALIGN)
        end = start + int(nbytes)
        assert end + self.guard <= self.nbytes, f"arena too small for region {name!r}"
        self.regions[name] = (start, end, kind)
        self._at = end + self.guard
        return self.base + start

    def address(self, name):
        return self.base + self.regions[name][0]

    def size(self, name):
        start, end, _ = self.regions[name]
        return end - start

    def put(self, name, array):
        a = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        start, end, _ = self.regions[name]
        assert a.nbytes == end - start, (name, a.nbytes, end - start)
        self.before[start:end] = a
        self.buf.upload(a, start)

    def fill(self, name, value):
        self.put(name, np.full(self.size(name), value, np.uint8))

    def get(self, name):
        start, end, _ = self.regions[name]
        return self.buf.download(end - start, start)

    def prefill(self, name):
        """What region `name` held before the call (the random fill, or the last put)."""
        start, end, _ = self.regions[name]
        return self.before[start:end].copy()

    def _describe(self, off):
        """Where byte `off` of the arena lies, for the failure message."""
        prev = nxt = None
        for name, (start, end, kind) in self.regions.items():
            if start <= off < end:
                return f"'{kind}' region {name!r} changed at byte offset {off - start}"
            if end <= off:
                prev = (name, off - end + 1)
            elif nxt is None:
                nxt = (name, start - off)
        parts = []
        if prev:
            parts.append(f"{prev[1]} byte(s) past the end of region {prev[0]!r}")
        if nxt:
            parts.append(f"{nxt[1]} byte(s) before the start of region {nxt[0]!r}")
        return "guard byte changed " + ", ".join(parts)

    def check(self):
        """One download of the whole arena.  Every guard byte and every "in"
        region must hold what was put there; -> {name: bytes} of the "out" and
        "inout" regions."""
        got = self.buf.download()
        diff = got != self.before
        out = {}
        for name, (start, end, kind) in self.regions.items():
            if kind != "in":
                diff[start:end] = False
                out[name] = got[start:end].copy()
        if diff.any():
            bad = np.flatnonzero(diff)
            off = int(bad[0])
            raise AssertionError(f"{self._describe(off)} (arena offset {off}: {int(self.before[off]):#04x} -> "
                                 f"{int(got[off]):#04x}; {len(bad)} stray byte(s) in all, the last at arena "
                                 f"offset {int(bad[-1])}: {self._describe(int(bad[-1]))})")
        return out


def make(gpu, specs, seed, row_pitch=0, buffer=None):
    """An arena sized for specs = [(name, nbytes, kind), ...], carved in that
    order -> (arena, {name: device address})."""
    guard = guard_for(row_pitch)
    arena = Arena(gpu, arena_bytes([s[1] for s in specs], guard), seed, guard=guard, buffer=buffer)
    return arena, {name: arena.carve(name, nbytes, kind) for name, nbytes, kind in specs}


# ---- the buffers of a receiver case (rx_cases.Case) as arena regions ------------
RX_OUT = ("valid", "leaves", "values", "digests", "status")


def rx_specs(case, tag="", vpitch=None, kinds=None):
    """rx_cases.DevCase's buffers as (name, nbytes, kind), every name prefixed
    with `tag`: the rows, then the const inputs (branches, roots, present, the
    ragged lens), then each output.  kinds: {name: kind} where a stage takes a
    buffer otherwise (rbc_dev_verify: shards "in"; rbc_dev_interpolate alone:
    valid "in", leaves "inout")."""
    c = case
    I, n = c.count, c.n
    vpitch = c.vpitch if vpitch is None else vpitch
    specs = [("shards", I * n * c.spitch, "inout"), ("branches", c.branches.nbytes, "in"), ("roots", I * 32, "in"),
             ("present", I * n, "in")]
    if c.ragged:
        specs.append(("lens", I * 4, "in"))
    specs += [("valid", I * n, "out"), ("leaves", I * n * 32, "out"), ("values", I * vpitch, "out"),
              ("digests", I * 32, "out"), ("status", I * 4, "out")]
    return [(tag + name, nbytes, (kinds or {}).get(name, kind)) for name, nbytes, kind in specs]


def interleave(*spec_lists):
    """[a0, b0, a1, b1, ...]: two batches' buffers side by side in the arena."""
    assert len({len(s) for s in spec_lists}) == 1
    return [spec for group in zip(*spec_lists) for spec in group]


class RxRegions:
    """A Case's buffers in an arena that was carved from rx_specs(case, tag,
    ...): rx_cases.DevCase with integer device addresses.  The outputs keep
    the arena's random fill as their prefill."""

    def __init__(self, arena, case, tag="", vpitch=None):
        self.arena, self.case, self.tag = arena, case, tag
        self.vpitch = case.vpitch if vpitch is None else vpitch
        for name in ("shards", "branches", "roots", "present", "lens") + RX_OUT:
            setattr(self, name, arena.address(tag + name) if tag + name in arena.regions else None)
        self.ulen = 0 if case.ragged else case.S
        c = case
        arena.put(tag + "shards", c.receiver_rows())
        arena.put(tag + "branches", c.branches)
        arena.put(tag + "roots", c.roots)
        arena.put(tag + "present", c.present)
        if c.ragged:
            arena.put(tag + "lens", c.lens)

    def verify(self, ctx, stream=None):
        c = self.case
        ctx.dev_verify(stream, c.count, self.shards, c.spitch, self.lens, self.ulen, self.branches, self.roots,
                       self.present, self.valid, self.leaves)

    def interpolate(self, ctx, joined=True, leaves_verified=1, stream=None):
        c = self.case
        ctx.dev_interpolate(stream, c.count, self.shards, c.spitch, self.lens, self.ulen, self.valid, self.leaves,
                            leaves_verified, self.roots, self.values if joined else None,
                            self.vpitch if joined else 0, self.digests, self.status)

    def rx_batch(self, ctx, joined=True):
        c = self.case
        return ctx.rx_batch(c.count, self.shards, c.spitch, self.lens, self.ulen, self.branches, self.roots,
                            self.present, self.valid, self.leaves, self.values if joined else None,
                            self.vpitch if joined else 0, self.digests, self.status)

    def prefill(self):
        c = self.case
        return dict(values=self.arena.prefill(self.tag + "values").reshape(c.count, self.vpitch),
                    digests=self.arena.prefill(self.tag + "digests").reshape(c.count, 32))

    def read(self, out):
        """rx_cases.DevCase.read() from what arena.check() returned."""
        c, t = self.case, self.tag
        I, n = c.count, c.n
        full = out[t + "shards"].reshape(I, n, c.spitch)
        return dict(rows=full[:, :, : c.S].copy(), pitch_rows=full, valid=out[t + "valid"].reshape(I, n),
                    leaves=out[t + "leaves"].reshape(I, n, 32), values=out[t + "values"].reshape(I, self.vpitch),
                    digests=out[t + "digests"].reshape(I, 32), status=out[t + "status"].view(np.int32).copy())
