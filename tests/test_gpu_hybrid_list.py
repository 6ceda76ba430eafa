"""tv_hybrid_verify_list on the GPU: completed pieces of a hybrid torrent checked against both descriptions from one
staging, on a slot pool and on a resident shard, bit-exact against hashlib SHA-1 over the padded linear bytes and the
merkle reference (tests/hybrid_util.py Layout.verdicts; no code shared with the library).  Every slot is staged as 0xFF
over its whole row before the file bytes, so a pad range the call failed to zero shows as a v1 mismatch, and the rows are
read back to see exactly which bytes it stored.  The shapes are the smallest at which the call takes another path."""
import ctypes
import random

import numpy as np
import pytest

from tests import hybrid_list_util as hl
from tests import hybrid_util as hu
from tests import synth, v2_ref

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384
L0 = 64 * K
LENGTHS0 = [2 * L0 + 20000, L0, 1, 3 * L0 - 17, 5]          # pieces: L, L, 20000 | L | 1 | L, L, L - 17 | 5


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def layouts():
    """The fixture layout with and without a trailing pad, computed once and left unchanged."""
    files = [rnd(30 + k, n) for k, n in enumerate(LENGTHS0)]
    return {t: hu.Layout(files, L0, trailing=t) for t in (False, True)}


def _raises(native, code, fn, *a, **kw):
    with pytest.raises(native.NativeError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def _scrambled(P, seed=3):
    order = list(range(P))
    random.Random(seed).shuffle(order)
    assert order != sorted(order)
    return order


# ---- the fixture layout on a slot pool ------------------------------------------------------------------------------------

@pytest.mark.parametrize("trailing", [False, True])
def test_fixture_layout_on_a_slot_pool(ctx, native, layouts, trailing):
    lay = layouts[trailing]
    P = lay.P
    assert lay.pb == [L0, L0, 20000, L0, 1, L0, L0, L0 - 17, 5] and lay.tails == [2, 4, 7] + ([8] if trailing else [])
    ok1, ok2, _, _ = lay.verdicts(lay.files)
    assert all(ok1) and all(ok2)
    never = 5
    hl.set_pool(ctx, native, lay, P)
    hl.stage_pieces(ctx, lay, [i for i in _scrambled(P) if i != never])
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == P - 1
    want = [i != never for i in range(P)]
    lists = [[2], list(range(P)), list(reversed(range(P))), [8, 2, 2, 0, 8, 4, never, 7, 4], [never]]
    for listed in lists:
        ok, v1, v2 = hl.run_list(ctx, lay, listed, release=False)
        assert v1 == [want[i] for i in listed], listed
        assert v2 == [want[i] for i in listed], listed
        assert ok == [want[i] for i in listed], listed
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == P - 1
    assert hl.run_list(ctx, lay, list(range(P)))[0] == want
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == 0
    assert hl.run_list(ctx, lay, [0, 2]) == ([False] * 2,) * 3          # their slots were freed


def test_independent_verdicts(ctx, native, layouts):
    lay = layouts[True]
    P = lay.P
    staged = [bytearray(f) for f in lay.files]
    staged[0][2 * L0 + 19999] ^= 0x01                       # piece 2: the last byte before its pad range
    staged[3][0] ^= 0x80                                    # piece 5: its first byte
    staged = [bytes(s) for s in staged]
    pieces = hu.xor_at(lay.pieces, 20 * 0 + 7, 0x10)        # piece 0: its v1 digest only
    hashes = list(lay.hashes)
    hashes[3] = hu.xor_at(hashes[3], 31, 0x01)              # piece 3: its v2 hash only
    leaves = list(lay.tl)
    assert leaves[4] == 1
    leaves[4] = 2                                           # piece 4 (one byte, a tree of one leaf): the wrong width
    ok1, ok2, _, _ = lay.verdicts(staged, pieces, hashes)
    assert v2_ref.piece_root(hl.piece_data(lay, 4), 2) != lay.hashes[4]      # (another root under the other width)
    ok2[4] = False
    assert ok1 == [i not in (0, 2, 5) for i in range(P)] and ok2 == [i not in (2, 3, 4, 5) for i in range(P)]
    hl.set_pool(ctx, native, lay, P, pieces=pieces)
    hl.stage_pieces(ctx, lay, _scrambled(P, 4), staged)
    ok, v1, v2 = hl.run_list(ctx, lay, list(range(P)), hashes=hashes, leaves=leaves)
    assert v1 == ok1 and v2 == ok2 and ok == [a and b for a, b in zip(ok1, ok2)]
    assert (ok[0], v1[0], v2[0]) == (False, False, True)
    assert (ok[3], v1[3], v2[3]) == (False, True, False)
    assert (ok[4], v1[4], v2[4]) == (False, True, False)
    # NULL v1 / v2 outputs: the AND alone
    hl.stage_pieces(ctx, lay, _scrambled(P, 5), staged)
    lib = native.lib()
    pc = np.arange(P, dtype=np.uint64)
    pb, tl = np.array(lay.pb, np.uint32), np.array(leaves, np.uint32)
    out = ctypes.create_string_buffer(P)
    assert lib.tv_hybrid_verify_list(ctx._h, P, pc.ctypes.data, pb.ctypes.data, tl.ctypes.data, b"".join(hashes), None,
                                     None, out, 1) == native.TV_OK
    assert [bool(x) for x in out.raw[:P]] == ok


def test_read_back_and_release(ctx, native, layouts):
    lay = layouts[True]
    P = lay.P
    hl.set_pool(ctx, native, lay, P)
    hl.stage_pieces(ctx, lay, _scrambled(P, 6))
    listed = [8, 2, 0, 7, 2]
    assert hl.run_list(ctx, lay, listed, release=False)[0] == [True] * len(listed)
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == P
    for i in range(P):
        row, data, v1 = hl.read_row(ctx, lay, i), hl.piece_data(lay, i), lay.v1_len[i]
        assert row[:lay.pb[i]] == data, i                   # the staged bytes
        pad = row[lay.pb[i]:]
        assert len(pad) == v1 - lay.pb[i]
        assert pad == (bytes(len(pad)) if i in listed else b"\xff" * len(pad)), i   # zeros exactly in [piece_bytes, v1_len)
    # a pad left as 0xFF fails v1 only where there is one; the call zeroes it, so every piece passes; release frees
    assert hl.run_list(ctx, lay, list(range(P)), release=True)[0] == [True] * P
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == 0


@pytest.mark.parametrize("kernel", [0, 1, 2, 4])
def test_every_sha1_kernel_form(ctx, native, layouts, kernel):
    lay = layouts[False]
    P = lay.P
    staged = [bytearray(f) for f in lay.files]
    staged[3][L0 + 5] ^= 0x04                               # piece 6
    staged = [bytes(s) for s in staged]
    ok1, ok2, _, _ = lay.verdicts(staged)
    assert ok1 == ok2 == [i != 6 for i in range(P)]
    listed = _scrambled(P, 8) + [6, 8, 0]                   # (the short last piece among full ones: list_plan's own waves)
    ctx.set_option(native.TV_OPT_KERNEL, kernel)
    try:
        hl.set_pool(ctx, native, lay, P)
        hl.stage_pieces(ctx, lay, _scrambled(P, 7), staged)
        ok, v1, v2 = hl.run_list(ctx, lay, listed)
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
    assert v1 == [ok1[i] for i in listed] and v2 == [ok2[i] for i in listed] and ok == v1
    assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 3)


# ---- piece lengths ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [16 * K, 64 * K, 256 * K, 8192 * K])
def test_piece_lengths(ctx, native, L):
    """A 100-byte tail, a 1-byte tail (256 KiB: four pad chunks) and, below 8 MiB, an L - 1 one; at 8 MiB W = 512 (two
    tiles of the v2 list kernel) and three pieces."""
    lengths = [L + 100, 1] + ([L - 1] if L < 8192 * K else [])
    files = [rnd(L // K + k, n) for k, n in enumerate(lengths)]
    lay = hu.Layout(files, L, trailing=True)
    P = lay.P
    assert P == len(lengths) + 1 and lay.tails == list(range(1, P))
    staged = [bytearray(f) for f in files]
    staged[0][L + 99] ^= 0x20                               # piece 1: the last byte before its pad range
    staged = [bytes(s) for s in staged]
    ok1, ok2, _, _ = lay.verdicts(staged)
    assert ok1 == ok2 == [i != 1 for i in range(P)]
    hl.set_pool(ctx, native, lay, P)
    hl.stage_pieces(ctx, lay, list(reversed(range(P))), staged)
    ok, v1, v2 = hl.run_list(ctx, lay, list(range(P)), release=False)
    assert (ok, v1, v2) == ([a and b for a, b in zip(ok1, ok2)], ok1, ok2)
    assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 3)
    k, total = ctx.last_timing()
    assert 0 < k <= total
    row = hl.read_row(ctx, lay, 2)                          # the 1-byte piece: its byte, then zeros out to L
    assert row[:1] == staged[1] and row[1:] == bytes(L - 1)
    hl.run_list(ctx, lay, list(range(P)))


# ---- a resident shard, a shard that starts at piece 8 ------------------------------------------------------------------------

def test_whole_shard_resident_layout(ctx, native, layouts):
    lay = layouts[True]
    P = lay.P
    staged = [bytearray(f) for f in lay.files]
    staged[4][4] ^= 0x01                                    # piece 8: the last byte before the trailing pad
    staged = [bytes(s) for s in staged]
    ok1, ok2, _, _ = lay.verdicts(staged)
    hl.set_pool(ctx, native, lay, 0)
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == 0
    hu.load(ctx, lay, staged=staged, relayout=False)        # the whole shard as 0xFF, then the files
    listed = _scrambled(P, 9) + [8, 4]
    ok, v1, v2 = hl.run_list(ctx, lay, listed)
    assert v1 == [ok1[i] for i in listed] and v2 == [ok2[i] for i in listed]
    assert ok == [i != 8 for i in listed]
    assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 3)
    assert hu.read_shard(ctx, lay) == hu.padded_linear(staged, L0, True)
    # a resident row stays: listed again, the same answers
    assert hl.run_list(ctx, lay, listed)[0] == ok


def test_a_shard_that_starts_at_piece_8(ctx, native, layouts):
    files = layouts[False].files * 2                        # 18 pieces; the shard: pieces 8 .. 17
    lay = hu.Layout(files, L0, trailing=False)
    assert lay.P == 18
    first, count = 8, 10
    staged = [bytearray(f) for f in files]
    staged[5][0] ^= 0x02                                    # piece 9
    staged = [bytes(s) for s in staged]
    ok1, ok2, _, _ = lay.verdicts(staged)
    hl.set_pool(ctx, native, lay, count, first, count)
    order = [first + j for j in _scrambled(count, 10)]
    hl.stage_pieces(ctx, lay, order, staged)
    _raises(native, native.TV_ERR_ARG, hl.run_list, ctx, lay, [8, 7])
    listed = list(reversed(order)) + [17, 8]
    ok, v1, v2 = hl.run_list(ctx, lay, listed)
    assert v1 == [ok1[i] for i in listed] and v2 == [ok2[i] for i in listed]
    assert ok == [i != 9 for i in listed]
    assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == 0


# ---- reporting ------------------------------------------------------------------------------------------------------------------

def test_reporting_and_flat_device_memory(ctx, native, layouts):
    lay = layouts[True]
    P = lay.P
    hl.set_pool(ctx, native, lay, P)
    assert hl.run_list(ctx, lay, [0, 2])[0] == [False, False]           # nothing holds a slot
    assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 0)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 0
    held = None
    for rep in range(3):
        hl.stage_pieces(ctx, lay, _scrambled(P, 11 + rep))
        assert hl.run_list(ctx, lay, [0, 1, 3, 5, 6], release=False)[0] == [True] * 5      # whole pieces: no pad range
        assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 2)
        assert hl.run_list(ctx, lay, list(range(P)))[0] == [True] * P
        assert ctx.last_kernel() == (native.KERNEL_HYBRID_LIST, 3)
        k, total = ctx.last_timing()
        assert 0 < k <= total
        # the v2 list launch's grid: 64 entries of 4 leaves per workgroup
        assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 1
        now = (ctx.counter(native.TV_COUNTER_DEVICE_BYTES), ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS))
        held = held or now
        assert now == held
    # beyond the two list calls' buffers: at most 16 bytes per listed entry, for at least 1,024 entries
    with native.Context(0) as c:
        hl.set_pool(c, native, lay, P)
        hl.stage_pieces(c, lay, range(P))
        c.verify_list(list(range(P)))
        hl.stage_pieces(c, lay, range(P))
        c.v2_verify_list(list(range(P)), lay.pb, lay.tl, b"".join(lay.hashes))
        before = c.counter(native.TV_COUNTER_DEVICE_BYTES)
        hl.stage_pieces(c, lay, range(P))
        hl.run_list(c, lay, list(range(P)))
        assert 0 < c.counter(native.TV_COUNTER_DEVICE_BYTES) - before <= 16 * 1024


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals(native, layouts):
    ARG, STATE = native.TV_ERR_ARG, native.TV_ERR_STATE
    lay = layouts[True]
    P, L = lay.P, L0
    h = bytes(32)
    lib = native.lib()
    with native.Context(0) as c:
        call = c.hybrid_verify_list
        assert "tv_set_layout" in _raises(native, STATE, call, [0], [L], [4], h)          # before tv_set_layout
        c.set_layout(lay.total, L, P)
        assert "tv_set_digests" in _raises(native, STATE, call, [0], [L], [4], h)         # before tv_set_digests
        # a windowed layout; no resident payload; a stream
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 4 * (L + 256) + 256)
        c.set_layout(16 * L, L, 16)
        c.set_digests(bytes(20 * 16))
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) > 0
        assert "windowed" in _raises(native, STATE, call, [0], [L], [4], h)
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
        c.set_option(native.TV_OPT_RESIDENT, 0)
        c.set_layout(16 * L, L, 16)
        c.set_digests(bytes(20 * 16))
        assert "TV_OPT_RESIDENT" in _raises(native, STATE, call, [0], [L], [4], h)
        c.set_option(native.TV_OPT_RESIDENT, 1)
        c.set_layout(2 * L, L, 2)
        c.set_digests(bytes(40))
        c.stream_begin()
        assert "stream" in _raises(native, STATE, call, [0], [L], [4], h)
        c.stream_abort()
        assert call([], [], [], b"") == (b"", b"", b"")                                   # n == 0
        # piece lengths: not a power of two, below 16 KiB, above 1 GiB
        for bad_L in (3 * LEAF, 8192):
            c.set_layout(2 * bad_L, bad_L, 2)
            c.set_digests(bytes(40))
            _raises(native, ARG, call, [0], [1], [1], h)
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(2 << 30, 2 << 30, 1)
        c.set_digests(bytes(20))
        _raises(native, ARG, call, [0], [LEAF], [1], h)
        # the rest on a slot pool holding every piece over a 0xFF fill: a refused call changes nothing
        hl.set_pool(c, native, lay, P)
        hl.stage_pieces(c, lay, _scrambled(P, 12))
        rows = [hl.read_row(c, lay, i) for i in range(P)]
        pc, pb, tl = np.array([2], np.uint64), np.array([20000], np.uint32), np.array([4], np.uint32)
        outs = [ctypes.create_string_buffer(1) for _ in range(3)]
        args = [pc.ctypes.data, pb.ctypes.data, tl.ctypes.data, lay.hashes[2]]
        for k in range(4):                                                                # each input NULL with n > 0
            assert lib.tv_hybrid_verify_list(c._h, 1, *[None if q == k else a for q, a in enumerate(args)], *outs, 1) == ARG
        assert lib.tv_hybrid_verify_list(c._h, 1, *args, outs[0], outs[1], None, 1) == ARG    # ok_out
        for piece in (P, 1 << 40):                                                        # outside the shard
            _raises(native, ARG, call, [2, piece], [20000, L], [4, 4], h * 2)
        for b, w in ((0, 4), (L + 1, 4), (L, 3), (L, 0), (LEAF + 1, 1), (L, 8)):          # tv_v2_set_pieces' ranges
            msg = _raises(native, ARG, call, [2, 3], [20000, b], [4, w], h * 2)
            assert ("piece_bytes[1]" in msg) or ("tree_leaves[1]" in msg)
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == P
        assert [hl.read_row(c, lay, i) for i in range(P)] == rows                         # no zero was stored
        # piece_bytes > v1_len: the short last piece of the layout WITHOUT the trailing pad
        short = layouts[False]
        hl.set_pool(c, native, short, P)
        hl.stage_pieces(c, short, _scrambled(P, 13))
        rows = [hl.read_row(c, short, i) for i in range(P)]
        msg = _raises(native, ARG, call, [2, 8], [20000, 6], [4, 1], h * 2)
        assert "exceeds the piece's v1 length 5" in msg and "not the v1 space" in msg
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == P
        assert [hl.read_row(c, short, i) for i in range(P)] == rows
        # afterwards the two separate list calls on the same ctx give their own answers: v1 hashes the 0xFF pads
        want1 = [short.pb[i] == short.v1_len[i] for i in range(P)]
        assert want1 == [i not in (2, 4, 7) for i in range(P)]
        assert [bool(x) for x in c.verify_list(list(range(P)))] == want1
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
        hl.stage_pieces(c, short, _scrambled(P, 14))
        assert list(c.v2_verify_list(list(range(P)), short.pb, short.tl, b"".join(short.hashes))) == [1] * P
        hl.stage_pieces(c, short, _scrambled(P, 15))
        assert hl.run_list(c, short, list(range(P)))[0] == [True] * P
