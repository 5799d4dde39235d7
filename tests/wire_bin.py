"""The binary VAL / ECHO payload codec (include/rbc_protocol.h, version 1),
restated in Python from the format table for the tests: expected bytes come
from here, never from the code under test.

    pb.Message:  0x1a varint(R) 0x0a varint(J) <payload, J bytes> [0x10 type]
                 R = 1 + varint_len(J) + J + (type ? 2 : 0); type absent for VAL
    payload:     0xB1 0x01 L 0x00 | S as u32 LE | root[32] | branch[32*L] | shard[S]
"""
import struct

MAGIC, VERSION = 0xB1, 0x01
VAL, ECHO = 0, 1
OK, FALLBACK, OTHER_ROOT, OTHER_LEN = 0, 1, 2, 3


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def payload(root: bytes, branch: bytes, shard: bytes) -> bytes:
    assert len(root) == 32 and len(branch) % 32 == 0 and len(branch) // 32 <= 255
    return bytes([MAGIC, VERSION, len(branch) // 32, 0]) + struct.pack("<I", len(shard)) + root + branch + shard


def wrap(msg_type: int, body: bytes) -> bytes:
    """pb.Message{rbc: pb.RBC{payload, type}} for a non-empty payload."""
    inner = b"\x0a" + varint(len(body)) + body + (b"\x10" + varint(msg_type) if msg_type else b"")
    return b"\x1a" + varint(len(inner)) + inner


def message(msg_type: int, root: bytes, branch: bytes, shard: bytes) -> bytes:
    return wrap(msg_type, payload(root, branch, shard))


def depth_of(n: int) -> int:
    d = 0
    while (1 << d) < n:
        d += 1
    return d


def flat_len(n: int, index: int) -> int:
    """Branch entries of leaf `index` in the Go flat form: the depth, less the
    empty level-0 sibling of an odd last leaf."""
    d = depth_of(n)
    return d - (1 if d > 0 and (index ^ 1) >= n else 0)


def message_size(n: int, shard_len: int, index: int, msg_type: int) -> int:
    J = 40 + 32 * flat_len(n, index) + shard_len
    R = 1 + len(varint(J)) + J + (2 if msg_type else 0)
    return 1 + len(varint(R)) + R


def header_len(msg: bytes) -> int:
    """Bytes in front of the payload: 0x1a varint(R) 0x0a varint(J)."""
    p = 1
    while msg[p] & 0x80:
        p += 1
    p += 2
    while msg[p] & 0x80:
        p += 1
    return p + 1


def parse_payload(p: bytes):
    """(root, branch, shard) of a well-formed payload, else None."""
    if len(p) < 40 or p[0] != MAGIC or p[1] != VERSION or p[3] != 0:
        return None
    L, S = p[2], struct.unpack("<I", p[4:8])[0]
    if len(p) != 40 + 32 * L + S:
        return None
    return p[8:40], p[40:40 + 32 * L], p[40 + 32 * L:]


def _read_varint(b: bytes, p: int):
    v = sh = 0
    while p < len(b) and sh < 35:
        v |= (b[p] & 0x7F) << sh
        p += 1
        if not b[p - 1] & 0x80:
            return v, p
        sh += 7
    return None, p


def canonical(msg: bytes, n: int, index: int, pitch: int):
    """(type, root, branch, shard) when msg is what message() writes for leaf
    `index` of an n-leaf tree with 1 <= S <= pitch, else None: the device
    decoders' OK.  Read front to back, then compared with its re-encoding."""
    if len(msg) < 4 or msg[0] != 0x1A:
        return None
    R, p = _read_varint(msg, 1)
    if R is None or p >= len(msg) or msg[p] != 0x0A:
        return None
    J, p = _read_varint(msg, p + 1)
    if J is None or p + J > len(msg):
        return None
    rest = msg[p + J:]
    if rest not in (b"", b"\x10\x01"):
        return None
    t = ECHO if rest else VAL
    f = parse_payload(msg[p:p + J])
    if not f or not 1 <= len(f[2]) <= pitch or len(f[1]) != 32 * flat_len(n, index) or message(t, *f) != msg:
        return None
    return (t,) + f


def device_branch(n: int, index: int, flat: bytes) -> bytes:
    """The device form [max(depth,1)][32]: a zero slot for an empty level-0
    sibling or a depth-0 tree."""
    d = depth_of(n)
    if d == 0:
        return bytes(32)
    return (bytes(32) if flat_len(n, index) < d else b"") + flat


def unreachable_totals(n: int, index: int, lo: int, hi: int):
    """Totals in [lo, hi) that no (S >= 1, type) yields for this leaf."""
    reach = set()
    for t in (VAL, ECHO):
        for s in range(1, hi):
            z = message_size(n, s, index, t)
            if z >= hi:
                break
            reach.add(z)
    return [z for z in range(max(lo, message_size(n, 1, index, VAL)), hi) if z not in reach]
