"""Streamed SHA-1 columns on every kernel form, bit-exact against hashlib.

tv_verify_host, tv_stream_* and tv_stream_file_table hash a shard one column of C bytes of every piece at a time: each
launch carries blk_begin > 0, a clipped blk_end and finalize = 0, start_state() loads every piece's chaining value from
d_state and finish() writes it back.  Here the six kernel forms of tests/v1_columns.py VARIANTS (the lane kernel's
3-deep and pair rings, the split kernel at 1 and 2 pairs, the twin kernel's 2- and 4-wave workgroups) are forced and
run over columns of 1 .. 8 and 13 blocks on the shapes of tests/v1_columns.py (tests/test_v1_columns_shapes.py holds
them to their classes): a short last piece that ended in an earlier column (fast_end < fast_begin), columns wholly past
it (end < fast_begin), a padding block that falls into the next column, a last piece that ends exactly with a column,
1, 33, 65 and 130 pieces.  Every payload is verified twice: against the digests of the intact bytes (only the
corrupted pieces' bits clear) and against the digests of the corrupted bytes (every bit set: the corrupted pieces were
hashed, and hashed right).

Then windows x columns (two windows of columns, the final window down to the short last piece alone: n_main = 0),
unreadable and masked pieces through the tv_stream_* calls, stale 0xFF bytes past every row of a reused chunk buffer
(the helpers' spare block and the lane rings' clamped loads read there), and shards."""
import random

import pytest

from tests import v1_columns as vc
from tests.v1_columns import CS, PS, VARIANTS, Case, bits, bitfield, shapes

pytestmark = pytest.mark.gpu

# payloads and digests are built once per (L, last, P) and shared by the variants: the tests run width by width, and
# the cache holds one width's cases
_CACHE = {"group": None, "cases": {}}


def _case(group, L, last, P, bad=None):
    if _CACHE["group"] != group:
        _CACHE["group"], _CACHE["cases"] = group, {}
    key = (L, last, P)
    if key not in _CACHE["cases"]:
        _CACHE["cases"][key] = Case(L, last, P, bad)
    return _CACHE["cases"][key]


def _context(native, variant, chunk=0, budget=0):
    kernel, pairs, lane_pairs = VARIANTS[variant]
    ctx = native.Context(0)
    ctx.set_option(native.TV_OPT_RESIDENT, 0)
    ctx.set_option(native.TV_OPT_STREAM_CHUNK, chunk)
    ctx.set_option(native.TV_OPT_RESIDENT_BUDGET, budget)
    ctx.set_option(native.TV_OPT_KERNEL, kernel)
    ctx.set_option(native.TV_OPT_SPLIT_PAIRS, pairs)
    ctx.set_option(native.TV_OPT_LANE_PAIRS, lane_pairs)
    return ctx


def _verify_both(native, ctx, variant, case, units, window=None):
    """Call A: the intact bytes' digests over the corrupted payload; call B: the corrupted bytes' digests over it.  After
    each: the kernel and the launch count, and the final launch's grid (over the final window's pieces)."""
    what = (case.L, case.last, case.P)
    kernel = VARIANTS[variant][0]
    final = case.P if window is None else (case.P - 1) % window + 1
    grid = vc.workgroups(variant, final, case.last < case.L)
    ctx.set_layout(case.total, case.L, case.P)
    ctx.set_digests(case.good)
    got = ctx.verify_host(case.flipped)
    assert len(got) == (case.P + 7) // 8 and bits(got, case.P) == case.bits(case.bad), what
    assert ctx.last_kernel() == (kernel, units), what
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == grid, what
    ctx.set_digests(case.good_flipped)
    got = ctx.verify_host(case.flipped)
    assert got == bitfield(case.bits()), what
    assert ctx.last_kernel() == (kernel, units), what
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == grid, what


@pytest.mark.parametrize("c,variant", [(c, v) for c in CS for v in VARIANTS])
def test_column_sweep(native, variant, c):
    C = 64 * c
    kernel = VARIANTS[variant][0]
    pairs = shapes(c)
    biggest = max(L for L, _ in pairs) * max(PS)
    with _context(native, variant, chunk=C) as ctx, native.PinnedBuffer(biggest) as pinned:
        for k, (L, last) in enumerate(pairs):
            units = -(-L // C)
            assert units == vc.host_units(L, max(PS), C, 0)
            for P in PS:
                _verify_both(native, ctx, variant, _case(("sweep", c), L, last, P), units)
            # a page-locked source: the rows are DMA'd straight from it, 2D copies of source pitch L
            case = _case(("sweep", c), L, last, PS[k % len(PS)])
            pinned.mv[:case.total] = case.flipped
            ctx.set_layout(case.total, L, case.P)
            ctx.set_digests(case.good)
            got = ctx.verify_host(pinned.mv[:case.total])
            assert bits(got, case.P) == case.bits(case.bad), ("pinned", L, last, case.P)
            assert ctx.last_kernel() == (kernel, units)


@pytest.mark.parametrize("c,variant", [(c, v) for c in (1, 3, 6) for v in VARIANTS])
def test_windows_of_columns(native, variant, c):
    """Two windows of 2,048 pieces, each hashed in columns of C bytes (tv_plan.h stream_geometry under a budget of two
    chunk buffers of 2,048 rows of C + 256 bytes); the final window holds the short last piece alone, one full piece
    and it, or 64 pieces and it."""
    C = 64 * c
    budget = vc.column_budget(C)
    with _context(native, variant, budget=budget) as ctx:
        for P in (2049, 2050, 2048 + 65):
            for L in (3 * C, 3 * C + 56):
                assert vc.stream_geometry(L, P, budget) == (C, 2048)
                for last in (1, C, L - 1):
                    case = _case(("windows", c), L, last, P, bad=(0, 63, 64, 2047, 2048, P - 1))
                    _verify_both(native, ctx, variant, case, 2 * -(-L // C), window=vc.MIN_WIN)


def _stream(ctx, case, count, avail, unreadable, rng=None):
    """One stream driven by hand: rows written into the lent slot (row_bytes bytes each, the rest of the slot left as it
    is) or, by turns drawn from rng, committed from the payload.  -> the shard's bits."""
    L = case.L
    ctx.stream_begin(avail)
    while True:
        req = ctx.stream_next()
        if not req.rows:
            break
        for i in unreadable:
            if req.piece <= i < req.piece + req.rows:
                ctx.stream_unreadable(i)
        base = req.piece * L + req.offset
        if rng is None or rng.random() < 0.5:
            slot = ctx.stream_slot(req)
            for q in range(req.rows):
                n = ctx.row_bytes(req, q)
                slot[q * req.width:q * req.width + n] = case.flipped[base + q * L:base + q * L + n]
            slot.release()
            ctx.stream_commit(req)
        else:
            ctx.stream_commit_from(req, case.flipped, L, base)
    return bits(ctx.stream_end(), count)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_unreadable_and_masked_pieces(native, variant):
    """tv_stream_begin .. tv_stream_end by hand at columns of two blocks: the first, a middle and the last piece
    reported unreadable and random availability bits; expected = hashlib AND the mask AND readable, against the intact
    bytes' digests and (every other shape) the corrupted bytes' own, which every readable piece must match."""
    c = 2
    C = 64 * c
    kernel = VARIANTS[variant][0]
    rng = random.Random(20)
    with _context(native, variant, chunk=C) as ctx:
        for k, (L, last) in enumerate(shapes(c)):
            for P in (PS[k % len(PS)], 130):
                case = _case(("masked", c), L, last, P)
                unreadable = {0, P // 2, P - 1}
                mask = [rng.randrange(4) != 0 for _ in range(P)]
                ctx.set_layout(case.total, L, P)
                bad = case.bad if k % 2 == 0 else ()
                ctx.set_digests(case.good if k % 2 == 0 else case.good_flipped)
                got = _stream(ctx, case, P, bitfield(mask), unreadable, rng)
                want = [int(mask[i] and i not in unreadable and i not in bad) for i in range(P)]
                assert got == want, (L, last, P)
                assert ctx.last_kernel() == (kernel, -(-L // C))


@pytest.mark.parametrize("c,variant", [(c, v) for c in (1, 4) for v in VARIANTS])
def test_stale_bytes_past_a_row(native, variant, c):
    """A stream of 0xFF bytes in columns 8 x wider fills both chunk buffers; the narrow stream after it needs fewer
    bytes, so the buffers are kept (no allocation) and whatever a kernel reads past a row's bytes -- the helpers' spare
    block, the clamped ring loads, the blocks after a short row -- is 0xFF, not zeros.  The rows go through the lent
    slot, row_bytes bytes each."""
    C = 64 * c
    kernel = VARIANTS[variant][0]
    P = 65
    wide = Case(16 * C, 16 * C, P, bad=(), payload=b"\xff" * (16 * C * P))
    rng = random.Random(c)
    with _context(native, variant) as ctx:
        for L in vc.lengths(C):
            for last in (C - 8, C, C + 1):
                if last > L:
                    continue
                ctx.set_option(native.TV_OPT_STREAM_CHUNK, 8 * C)
                ctx.set_layout(wide.total, wide.L, P)
                ctx.set_digests(wide.good)
                assert _stream(ctx, wide, P, None, (), rng) == [1] * P
                assert ctx.last_kernel() == (kernel, 2)                    # two columns: one in each chunk buffer
                allocs = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
                case = _case(("stale", c), L, last, P)
                ctx.set_option(native.TV_OPT_STREAM_CHUNK, C)
                ctx.set_layout(case.total, L, P)
                ctx.set_digests(case.good)
                got = _stream(ctx, case, P, None, ())          # (every row through the slot)
                assert got == case.bits(case.bad), (L, last)
                assert ctx.last_kernel() == (kernel, -(-L // C))
                assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs   # the chunk buffers were reused


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_shards_of_columns(native, variant):
    """130 pieces in columns of three blocks as the shards (0, 64), (64, 66) and (8, 120), each on a layout of its own:
    the shard's bits equal its slice of the whole torrent's."""
    c, P = 3, 130
    C = 64 * c
    kernel = VARIANTS[variant][0]
    with _context(native, variant, chunk=C) as ctx:
        for L, last in shapes(c):
            case = _case(("shards", c), L, last, P)
            want = case.bits(case.bad)
            for first, count in ((0, 64), (64, 66), (8, 120)):
                if first == 0 and last != L:
                    continue                                # (a shard without the last piece: once per piece length)
                ctx.set_layout(case.total, L, P, first, count)
                ctx.set_digests(case.good)
                got = ctx.verify_host(case.flipped[first * L:min(case.total, (first + count) * L)])
                assert bits(got, count) == want[first:first + count], (L, last, first, count)
                assert ctx.last_kernel() == (kernel, -(-L // C))
            whole = []
            for first, count in ((0, 64), (64, 66)):
                ctx.set_layout(case.total, L, P, first, count)
                ctx.set_digests(case.good_flipped)
                whole += bits(ctx.verify_host(case.flipped[first * L:min(case.total, (first + count) * L)]), count)
            assert whole == [1] * P, (L, last)
