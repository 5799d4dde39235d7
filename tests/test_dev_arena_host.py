"""The bookkeeping of tests/dev_arena.py on its numpy backend, no GPU: check()
must name the region and the offset of a stray byte next to a region, in a
const input and deep inside a guard, and must let a write inside an output
pass.  The GPU tests that carve their buffers from an arena rely on it."""
import re

import numpy as np
import pytest

import dev_arena as da

SPECS = [("rows", 5 * 320, "inout"), ("present", 37, "in"), ("valid", 37, "out"), ("digests", 5 * 32, "out")]


def _arena(row_pitch=320):
    arena, at = da.make(None, SPECS, seed=11, row_pitch=row_pitch, buffer=da.HostBuffer)
    arena.put("rows", np.arange(5 * 320, dtype=np.uint32).astype(np.uint8))
    arena.put("present", np.ones(37, np.uint8))
    return arena, at


def _flip(arena, address):
    """A one-byte device store at `address` that changes the byte there."""
    arena.buf.poke(address, int(arena.buf.mem[address - arena.base]) ^ 0x5A)


def test_layout_alignment_exact_sizes_and_guards():
    arena, at = _arena(row_pitch=3000)
    assert arena.guard == 6144 == da.guard_for(3000) and da.guard_for(0) == da.guard_for(2048) == 4096
    assert da.guard_for(2049) == 4352 and da.guard_for(2112) % 256 == 0 and da.guard_for(2112) >= 2 * 2112
    ends = []
    for name, nbytes, kind in SPECS:
        start, end, k = arena.regions[name]
        assert at[name] == arena.address(name) == arena.base + start and at[name] % 256 == 0
        assert end - start == nbytes == arena.size(name) and k == kind  # no slack added
        assert start - (ends[-1] if ends else 0) >= arena.guard  # a guard before every region
        ends.append(end)
    assert arena.nbytes - ends[-1] >= arena.guard  # and one after the last
    assert arena.nbytes == da.arena_bytes([s[1] for s in SPECS], arena.guard)
    fill = arena.buf.mem[: arena.guard]
    assert len(np.unique(fill)) > 200  # seeded random bytes, not a constant
    other, _ = da.make(None, SPECS, seed=12, buffer=da.HostBuffer)
    assert not np.array_equal(other.buf.mem[:4096], fill[:4096])
    with pytest.raises(AssertionError):
        da.Arena(None, 1 << 16, 1, guard=4000, buffer=da.HostBuffer)  # not a multiple of 256
    with pytest.raises(AssertionError):
        da.Arena(None, 1 << 16, 1, guard=2048, buffer=da.HostBuffer)  # under 4096
    with pytest.raises(AssertionError, match="too small"):
        arena.carve("more", 1 << 20, "out")


def test_put_get_and_untouched_arena_passes():
    arena, _ = _arena()
    assert np.array_equal(arena.get("present"), np.ones(37, np.uint8))
    assert np.array_equal(arena.get("rows"), np.arange(5 * 320, dtype=np.uint32).astype(np.uint8))
    out = arena.check()
    assert sorted(out) == ["digests", "rows", "valid"]  # the "out" and "inout" regions
    assert np.array_equal(out["valid"], arena.prefill("valid")) and len(out["digests"]) == 160


def test_a_write_inside_an_output_passes():
    arena, at = _arena()
    for name in ("valid", "rows", "digests"):
        _flip(arena, at[name])
        _flip(arena, at[name] + arena.size(name) - 1)
    out = arena.check()
    assert out["valid"][0] == arena.prefill("valid")[0] ^ 0x5A
    assert out["rows"][-1] == arena.prefill("rows")[-1] ^ 0x5A


@pytest.mark.parametrize("name", [s[0] for s in SPECS])
def test_a_byte_one_past_a_regions_end_is_named(name):
    arena, at = _arena()
    _flip(arena, at[name] + arena.size(name))
    with pytest.raises(AssertionError, match=re.escape(f"1 byte(s) past the end of region {name!r}")):
        arena.check()


@pytest.mark.parametrize("name", [s[0] for s in SPECS])
def test_a_byte_one_before_a_regions_start_is_named(name):
    arena, at = _arena()
    _flip(arena, at[name] - 1)
    with pytest.raises(AssertionError, match=re.escape(f"1 byte(s) before the start of region {name!r}")):
        arena.check()


@pytest.mark.parametrize("off", [0, 17, 36])
def test_a_changed_input_byte_is_named(off):
    arena, at = _arena()
    _flip(arena, at["present"] + off)
    with pytest.raises(AssertionError, match=re.escape(f"'in' region 'present' changed at byte offset {off}")):
        arena.check()


def test_a_byte_deep_inside_a_guard_is_named():
    arena, at = _arena()
    _flip(arena, at["rows"] + arena.size("rows") + 2000)  # one 320-byte row and more past the rows
    with pytest.raises(AssertionError) as e:
        arena.check()
    start_present = arena.regions["present"][0]
    gap = start_present - arena.regions["rows"][1]
    assert f"2001 byte(s) past the end of region 'rows'" in str(e.value)
    assert f"{gap - 2000} byte(s) before the start of region 'present'" in str(e.value)
    # the guards before the first region and after the last
    arena, at = _arena()
    _flip(arena, arena.base + 5)
    with pytest.raises(AssertionError, match=re.escape(f"{arena.regions['rows'][0] - 5} byte(s) before the start "
                                                       "of region 'rows'")):
        arena.check()
    arena, at = _arena()
    _flip(arena, arena.base + arena.nbytes - 1)
    tail = arena.nbytes - arena.regions["digests"][1]
    with pytest.raises(AssertionError, match=re.escape(f"{tail} byte(s) past the end of region 'digests'")):
        arena.check()


def test_every_stray_byte_is_counted_and_the_last_one_named():
    arena, at = _arena()
    _flip(arena, at["valid"] - 1)
    _flip(arena, at["digests"] + arena.size("digests") + 15)
    with pytest.raises(AssertionError) as e:
        arena.check()
    msg = str(e.value)
    assert "1 byte(s) before the start of region 'valid'" in msg and "2 stray byte(s) in all" in msg
    assert "16 byte(s) past the end of region 'digests'" in msg
