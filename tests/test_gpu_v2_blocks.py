"""tv_v2_leaf_hashes and tv_v2_check_blocks on the GPU (one lane per 16 KiB block, one launch per call), bit-exact
against tests/v2_ref.py (hashlib) and the golden layouts.  The shapes are the smallest at which the kernel can go
wrong: one block per piece, a piece that is one wave and one that is one workgroup, a list of mixed lengths whose
items straddle wave boundaries, last blocks around the SHA-256 padding edges, sparse want bits, stale slot bytes."""
import ctypes
import random

import numpy as np
import pytest

from tests import synth, v2_fuzz, v2_ref
from tests.v2_util import golden, golden_files

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384
ZERO = bytes(32)


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def flipped(data: bytes, pos: int, bit: int = 0x10) -> bytes:
    b = bytearray(data)
    b[pos] ^= bit
    return bytes(b)


def layer(data, W: int) -> bytes:
    """The reference leaf layer of one piece, out to W positions."""
    hs = v2_ref.leaf_hashes(data)
    return b"".join(hs + [ZERO] * (W - len(hs)))


def row_of(blocks, W: int) -> bytes:
    r = bytearray((W + 7) // 8)
    for i in blocks:
        r[i >> 3] |= 0x80 >> (i & 7)
    return bytes(r)


def held(nbytes: int) -> range:
    return range(-(-nbytes // LEAF))


def _raises(native, code, fn, *a, **kw):
    with pytest.raises(native.NativeError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


# ---- every width: leaves out, one flipped byte, one flipped expected hash -------------------------------------------------

@pytest.mark.parametrize("L", [16 * K, 64 * K, 1024 * K, 4096 * K])
def test_leaf_layers_and_single_flips(ctx, native, L):
    W, P = L // LEAF, 3
    nbytes = [L, L, L - 5]                                 # the last piece's last block is short
    data = rnd(L // K + 2, 2 * L + nbytes[2])
    pieces = [data[i * L:i * L + nbytes[i]] for i in range(P)]
    want = b"".join(layer(p, W) for p in pieces)
    m = sum(len(held(b)) for b in nbytes)
    ctx.set_layout(len(data), L, P)
    ctx.stage(0, data)
    idx = list(range(P))
    assert ctx.v2_leaf_hashes(idx, nbytes, [W] * P) == want
    assert ctx.last_kernel() == (native.KERNEL_V2_BLOCKS, 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-m // 256)
    k, total = ctx.last_timing()
    assert 0 < k <= total
    every = b"".join(row_of(held(b), W) for b in nbytes)
    assert ctx.v2_check_blocks(idx, nbytes, [W] * P, want) == every
    assert ctx.last_kernel() == (native.KERNEL_V2_BLOCKS, 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-m // 256)
    # one flipped byte in block k clears exactly bit k: a first byte, a middle block, the last valid byte of a short block
    flips = [(0, 0, 0), (1, W // 2, (W // 2) * LEAF + 777), (2, W - 1, nbytes[2] - 1)]
    staged = bytearray(data)
    for i, _, pos in flips:
        staged[i * L + pos] ^= 0x04
    ctx.stage(0, bytes(staged))
    expect = b"".join(row_of([q for q in held(b) if (i, q) not in {(a, c) for a, c, _ in flips}], W)
                      for i, b in enumerate(nbytes))
    assert ctx.v2_check_blocks(idx, nbytes, [W] * P, want) == expect != every
    # one flipped byte in the expected hash of block k clears exactly bit k
    ctx.stage(0, data)
    bad = bytearray(want)
    for i, q, _ in flips:
        bad[32 * (i * W + q) + (q % 32)] ^= 0x80
    assert ctx.v2_check_blocks(idx, nbytes, [W] * P, bytes(bad)) == expect
    assert ctx.v2_check_blocks(idx, nbytes, [W] * P, want) == every


def test_mixed_lengths_straddle_wave_boundaries(ctx, native):
    L, W = 1024 * K, 64
    nbytes = [1, LEAF, LEAF + 1, L - 1, L]                 # 1 + 1 + 2 + 64 + 64 = 132 items
    P = len(nbytes)
    pieces = [rnd(900 + i, b) for i, b in enumerate(nbytes)]
    ctx.set_layout(P * L, L, P)
    ctx.stage(0, rnd(8, P * L))                            # the rows hold other bytes past every piece's own
    for i, d in enumerate(pieces):
        ctx.stage(i * L, d)
    idx = list(range(P))
    widths = [1, 1, 2, W, W]                               # the narrowest trees: the width changes no leaf
    want = b"".join(layer(d, W) for d in pieces)
    for tl in (widths, [W] * P):
        assert ctx.v2_leaf_hashes(idx, nbytes, tl) == want
        assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 1
    every = b"".join(row_of(held(b), W) for b in nbytes)
    assert ctx.v2_check_blocks(idx, nbytes, widths, want) == every
    # the last valid byte of every piece: the last item of each run, on both sides of the wave boundaries
    for i, d in enumerate(pieces):
        ctx.stage(i * L, flipped(d, len(d) - 1))
    expect = b"".join(row_of(list(held(b))[:-1], W) for b in nbytes)
    assert ctx.v2_check_blocks(idx, nbytes, widths, want) == expect


def test_last_block_lengths_around_the_padding_edges(ctx):
    L, W = 64 * K, 4
    tails = [1, 55, 56, 63, 64, 65, 16383]
    nbytes = tails + [LEAF + t for t in tails]             # the short block alone, and after a whole one
    P = len(nbytes)
    pieces = [rnd(400 + i, b) for i, b in enumerate(nbytes)]
    ctx.set_layout(P * L, L, P)
    ctx.stage(0, rnd(6, P * L))
    for i, d in enumerate(pieces):
        ctx.stage(i * L, d)
    idx = list(range(P))
    widths = [v2_ref.next_pow2(len(held(b))) for b in nbytes]
    want = b"".join(layer(d, W) for d in pieces)
    assert ctx.v2_leaf_hashes(idx, nbytes, widths) == want
    for i, d in enumerate(pieces):                         # the last valid byte, and the byte after it stays unread
        ctx.stage(i * L, flipped(d, len(d) - 1) + b"\xa5")
    expect = b"".join(row_of(list(held(b))[:-1], W) for b in nbytes)
    assert ctx.v2_check_blocks(idx, nbytes, widths, want) == expect
    for i, d in enumerate(pieces):
        ctx.stage(i * L, d + b"\x5a")
    assert ctx.v2_check_blocks(idx, nbytes, widths, want) == b"".join(row_of(held(b), W) for b in nbytes)


# ---- want bits ------------------------------------------------------------------------------------------------------------

def test_sparse_want_bits(ctx, native):
    L, W = 1024 * K, 64
    nbytes = [L, 5 * LEAF + 77]
    pieces = [rnd(30, nbytes[0]), rnd(31, nbytes[1])]
    ctx.set_layout(2 * L, L, 2)
    ctx.stage(0, flipped(pieces[0], 8 * LEAF + 3))         # block 8 of piece 0 is bad
    ctx.stage(L, flipped(pieces[1], 2 * LEAF))             # block 2 of piece 1 is bad
    want = layer(pieces[0], W) + layer(pieces[1], W)
    bad = {(0, 8), (1, 2)}
    cases = [([7], []),                                    # a single block
             ([8], [2]),                                   # ... the bad ones alone
             (list(range(0, W, 2)), list(range(1, W, 2))),  # alternate blocks (piece 1: most hold no byte)
             ([], [5]),                                    # only the short last block
             ([], []),
             (list(range(W)), list(range(W)))]
    for w0, w1 in cases:
        bits = ctx.v2_check_blocks([0, 1], nbytes, [W, 8], want, row_of(w0, W) + row_of(w1, W))
        ok0 = [q for q in w0 if (0, q) not in bad]
        ok1 = [q for q in w1 if q in held(nbytes[1]) and (1, q) not in bad]
        assert bits == row_of(ok0, W) + row_of(ok1, W), (w0[:4], w1[:4])
        m = len(w0) + len([q for q in w1 if q in held(nbytes[1])])
        assert ctx.last_kernel() == (native.KERNEL_V2_BLOCKS, 1 if m else 0)
        assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-m // 256)
    # only wanted positions of leaf_hashes are read: garbage everywhere else changes nothing
    noise = bytearray(rnd(32, len(want)))
    noise[32 * 7:32 * 8] = want[32 * 7:32 * 8]
    noise[32 * (W + 5):32 * (W + 6)] = want[32 * (W + 5):32 * (W + 6)]
    assert ctx.v2_check_blocks([0, 1], nbytes, [W, 8], bytes(noise), row_of([7], W) + row_of([5], W)) == \
        row_of([7], W) + row_of([5], W)


def test_stale_slot_bytes_around_a_staged_block(native):
    L, W = 64 * K, 4
    b_piece = rnd(51, L)
    hashes = bytearray(rnd(52, 32 * W))                    # only position 3 is the piece's
    hashes[96:128] = v2_ref.sha256(b_piece[3 * LEAF:])
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(3 * L, L, 3)
        results = []
        for a_seed in (60, 61):                            # whatever piece A left in the slot
            a_piece = rnd(a_seed, L)
            c.stage(0, a_piece)
            assert c.v2_leaf_hashes([0], [L], [W], release=True) == layer(a_piece, W)
            assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
            c.stage(2 * L + 3 * LEAF, b_piece[3 * LEAF:])  # only block 3 of piece B: the same slot
            results.append(c.v2_check_blocks([2], [L], [W], bytes(hashes), row_of([3], W), release=True))
            assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
        assert results == [row_of([3], W)] * 2
        c.stage(2 * L + 3 * LEAF, flipped(b_piece[3 * LEAF:], LEAF - 1))
        assert c.v2_check_blocks([2], [L], [W], bytes(hashes), row_of([3], W), release=True) == bytes(1)


# ---- slot pools, shards, duplicates ------------------------------------------------------------------------------------------

def test_release_and_pieces_without_a_slot(native):
    L, W = 32 * K, 2
    datas = {i: rnd(70 + i, L if i != 9 else LEAF + 3) for i in (2, 5, 9)}
    nb = {i: len(d) for i, d in datas.items()}
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 4)
        c.set_layout(9 * L + nb[9], L, 10)
        for i, d in datas.items():
            c.stage(i * L, d)
        used = lambda: c.counter(native.TV_COUNTER_SLOTS_USED)  # noqa: E731
        assert used() == 3
        order = [5, 2, 5, 9]                               # a duplicate
        args = (order, [nb[i] for i in order], [W] * 4)
        want = b"".join(layer(datas[i], W) for i in order)
        assert c.v2_leaf_hashes(*args) == want and used() == 3                     # release = 0 keeps the slots
        assert c.v2_check_blocks(*args, want) == b"\xc0\xc0\xc0\xc0" and used() == 3
        assert c.v2_check_blocks([5], [L], [W], layer(datas[5], W), release=True) == b"\xc0" and used() == 2
        assert c.v2_leaf_hashes([9], [nb[9]], [W], release=True) == layer(datas[9], W) and used() == 1
        # a piece without a slot: 0 bits from the check, TV_ERR_STATE naming it from the leaf call; nothing is freed
        assert c.v2_check_blocks([5, 2, 7], [L] * 3, [W] * 3, layer(datas[5], W) + layer(datas[2], W) * 2) == \
            b"\x00\xc0\x00"
        assert used() == 1
        assert c.v2_check_blocks([7], [L], [W], bytes(64), release=True) == b"\x00"
        assert c.last_kernel() == (native.KERNEL_V2_BLOCKS, 0) and c.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 0
        msg = _raises(native, native.TV_ERR_STATE, c.v2_leaf_hashes, [2, 7], [L, L], [W, W], release=True)
        assert "piece 7" in msg and used() == 1
        assert c.v2_leaf_hashes([2], [L], [W], release=True) == layer(datas[2], W) and used() == 0


def test_a_shard_with_first_above_zero_and_unreadable_pieces(ctx, native, tmp_path):
    L, W = 64 * K, 4
    nbytes = {8: L, 9: L, 10: LEAF + 1}
    datas = {i: rnd(80 + i, b) for i, b in nbytes.items()}
    ctx.set_layout(24 * L, L, 24, 8, 3)                    # the shard: pieces 8, 9, 10
    for i, d in datas.items():
        ctx.stage(i * L, d)
    order = [9, 8, 9, 10, 10]
    args = (order, [nbytes[i] for i in order], [W, W, W, W, 2])
    want = b"".join(layer(datas[i], W) for i in order)
    assert ctx.v2_leaf_hashes(*args) == want
    assert ctx.v2_check_blocks(*args, want) == b"\xf0\xf0\xf0\xc0\xc0"
    # piece 9 from a file that is not there: unreadable until it is staged again
    p8 = tmp_path / "p8.bin"
    p8.write_bytes(datas[8])
    st = ctx.stage_files([str(p8), str(tmp_path / "missing.bin")], [0, 0], [8 * L, 9 * L], [L, L])
    assert [s == native.TV_OK for s in st] == [True, False]
    assert ctx.v2_check_blocks(*args, want) == b"\x00\xf0\x00\xc0\xc0"
    assert "piece 9" in _raises(native, native.TV_ERR_STATE, ctx.v2_leaf_hashes, *args)
    assert ctx.v2_leaf_hashes([8, 10], [L, LEAF + 1], [W, 2]) == layer(datas[8], W) + layer(datas[10], W)
    ctx.stage(9 * L, datas[9])
    assert ctx.v2_check_blocks(*args, want) == b"\xf0\xf0\xf0\xc0\xc0"


# ---- errors ------------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors(native):
    ARG, STATE = native.TV_ERR_ARG, native.TV_ERR_STATE
    L, W = 64 * K, 4
    h = bytes(32 * W)
    lib = native.lib()

    def both(c, code, pieces, nbytes, widths):
        _raises(native, code, c.v2_leaf_hashes, pieces, nbytes, widths)
        _raises(native, code, c.v2_check_blocks, pieces, nbytes, widths, h * len(pieces))

    with native.Context(0) as c:
        c.piece_length = L                                 # (the binding sizes its buffers by the layout's piece length)
        both(c, STATE, [0], [L], [W])                      # before tv_set_layout
        for bad_L in (3 * LEAF, 8192, 16383):              # not a power of two / below 16 KiB
            c.set_layout(2 * bad_L, bad_L, 2)
            c.piece_length = LEAF
            _raises(native, ARG, c.v2_leaf_hashes, [0], [1], [1])
            _raises(native, ARG, c.v2_check_blocks, [0], [1], [1], bytes(32))
            assert c.v2_leaf_hashes([], [], []) == b"" and c.v2_check_blocks([], [], [], b"") == b""
        c.set_layout(24 * L, L, 24, 8, 3)                  # the shard: pieces 8, 9, 10
        assert c.v2_leaf_hashes([], [], []) == b"" and c.v2_check_blocks([], [], [], b"") == b""       # n == 0
        pc, pb, tl = np.array([8], np.uint64), np.array([L], np.uint32), np.array([W], np.uint32)
        out = ctypes.create_string_buffer(32 * W)
        args = [pc.ctypes.data, pb.ctypes.data, tl.ctypes.data, out]
        assert lib.tv_v2_leaf_hashes(c._h, 1, *args, 0) == native.TV_OK
        for k in range(4):                                 # each pointer NULL with n > 0
            assert lib.tv_v2_leaf_hashes(c._h, 1, *[None if q == k else a for q, a in enumerate(args)], 0) == ARG
        args = [pc.ctypes.data, pb.ctypes.data, tl.ctypes.data, h, None, out]
        assert lib.tv_v2_check_blocks(c._h, 1, *args, 0) == native.TV_OK             # want_bits may be NULL
        for k in (0, 1, 2, 3, 5):
            assert lib.tv_v2_check_blocks(c._h, 1, *[None if q == k else a for q, a in enumerate(args)], 0) == ARG
        assert lib.tv_v2_leaf_hashes(None, 0, None, None, None, None, 0) == ARG
        assert lib.tv_v2_check_blocks(None, 0, None, None, None, None, None, None, 0) == ARG
        for piece in (0, 7, 11, 24, 1 << 40):              # outside the shard
            both(c, ARG, [8, piece], [L, L], [W, W])
        for b, w in ((0, 4), (L + 1, 4), (L, 3), (L, 0), (LEAF + 1, 1), (L, 8)):
            both(c, ARG, [8, 9], [L, b], [W, w])
        # a stream is active
        c.set_layout(2 * L, L, 2)
        c.set_digests(bytes(40))
        c.stream_begin()
        both(c, STATE, [0], [L], [W])
        c.stream_abort()
        assert c.v2_check_blocks([0], [L], [W], h) == b"\x00"
        # a windowed layout; no resident payload
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 4 * (L + 256) + 256)
        c.set_layout(16 * L, L, 16)
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) > 0
        both(c, STATE, [0], [L], [W])
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
        c.set_option(native.TV_OPT_RESIDENT, 0)
        c.set_layout(16 * L, L, 16)
        both(c, STATE, [0], [L], [W])
        c.set_option(native.TV_OPT_RESIDENT, 1)
        # a refused call frees no slot, whatever `release` says
        c.set_option(native.TV_OPT_LIST_SLOTS, 2)
        c.set_layout(16 * L, L, 16)
        d5, d9 = rnd(1, L), rnd(2, L)
        c.stage(5 * L, d5)
        c.stage(9 * L, d9)
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 2
        _raises(native, ARG, c.v2_leaf_hashes, [5, 9, 16], [L] * 3, [W] * 3, release=True)
        _raises(native, ARG, c.v2_check_blocks, [5, 9], [L, L], [W, 2], h * 2, release=True)
        _raises(native, STATE, c.v2_leaf_hashes, [5, 9, 3], [L] * 3, [W] * 3, release=True)     # 3 holds no slot
        assert lib.tv_v2_check_blocks(c._h, 1, None, pb.ctypes.data, tl.ctypes.data, h, None, out, 1) == ARG
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 2
        assert c.v2_check_blocks([5, 9], [L, L], [W, W], layer(d5, W) + layer(d9, W), release=True) == b"\xf0\xf0"
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0


def test_item_cap_and_piece_lengths_past_the_list_limit(native):
    """More than TV_V2_BLOCKS_MAX blocks are refused before anything is read; a 2 GiB piece length (W = 131,072), which
    tv_v2_verify_list refuses, is taken: there is no tree in on-chip memory.  Only six blocks of the piece hold bytes,
    so it is staged and referenced in milliseconds; a slot pool of one slot holds it."""
    ARG = native.TV_ERR_ARG
    lib = native.lib()
    L, W = 4096 * K, 256
    n = native.TV_V2_BLOCKS_MAX // W + 1                   # 16,385 entries (duplicates of piece 0) of 256 blocks
    pc, pb, tl = np.zeros(n, np.uint64), np.full(n, L, np.uint32), np.full(n, W, np.uint32)
    dummy = ctypes.create_string_buffer(64)                # (a refused call neither reads nor writes its buffers)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(L, L, 1)
        c.stage(0, rnd(3, LEAF))
        a = (pc.ctypes.data, pb.ctypes.data, tl.ctypes.data)
        assert lib.tv_v2_leaf_hashes(c._h, n, *a, dummy, 1) == ARG
        assert lib.tv_v2_check_blocks(c._h, n, *a, dummy, None, dummy, 1) == ARG
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 1
        # the cap counts the blocks to hash, not the entries: with no block wanted the same list is no item at all
        want = np.zeros((n, W // 8), np.uint8)
        bits = np.full((n, W // 8), 0xEE, np.uint8)
        assert lib.tv_v2_check_blocks(c._h, n, *a, dummy, want.ctypes.data, bits.ctypes.data, 0) == native.TV_OK
        assert not bits.any() and c.last_kernel() == (native.KERNEL_V2_BLOCKS, 0)
        L2 = 2 << 30
        W2 = L2 // LEAF
        data = rnd(78, 5 * LEAF + 9)
        c.set_layout(L2, L2, 1)
        c.stage(0, data)
        got = c.v2_leaf_hashes([0], [len(data)], [W2])
        assert len(got) == 32 * W2 and got[:192] == layer(data, 6) and got[192:] == bytes(32 * (W2 - 6))
        c.stage(5 * LEAF, flipped(data[5 * LEAF:], 8))
        bits = c.v2_check_blocks([0], [len(data)], [8], got, release=True)
        assert bits == row_of([0, 1, 2, 3, 4], W2)


# ---- reporting and memory ----------------------------------------------------------------------------------------------------

def test_reporting_and_no_reallocation(native):
    L, W, P = 1024 * K, 64, 20                             # 1,280 items: above the 1,024-item floor
    data = rnd(90, P * L)
    want = b"".join(layer(data[i * L:(i + 1) * L], W) for i in range(P))
    with native.Context(0) as c:
        c.set_layout(P * L, L, P)
        c.stage(0, data)
        extra0 = c.counter(native.TV_COUNTER_DEVICE_BYTES)
        allocs = None
        for rep in range(4):
            n = P if rep != 2 else 5                       # the same n, then a smaller one
            idx = list(range(n))
            if rep % 2:
                assert c.v2_leaf_hashes(idx, [L] * n, [W] * n) == want[:32 * W * n]
            else:
                assert c.v2_check_blocks(idx, [L] * n, [W] * n, want[:32 * W * n]) == b"\xff" * (8 * n)
            assert c.last_kernel() == (native.KERNEL_V2_BLOCKS, 1)
            assert c.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-n * W // 256)
            if rep == 0:
                allocs = c.counter(native.TV_COUNTER_DEVICE_ALLOCS)
                assert 0 < c.counter(native.TV_COUNTER_DEVICE_BYTES) - extra0 <= 48 * P * W
        assert c.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs
        assert c.counter(native.TV_COUNTER_DEVICE_BYTES) - extra0 <= 48 * P * W


# ---- the golden layouts and the seeded sweep -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(golden()))
def test_golden_leaf_layers_reduce_to_the_piece_hashes(ctx, name):
    g = golden()[name]
    files = golden_files(name)
    L = g["piece_length"]
    W = L // LEAF
    table = v2_ref.piece_table(g["lengths"], L)
    P = len(table)
    ctx.set_layout(P * L, L, P)
    for i, (f, o, b, w) in enumerate(table):
        ctx.stage(i * L, files[f][o:o + b])
    got = ctx.v2_leaf_hashes(list(range(P)), [r[2] for r in table], [r[3] for r in table])
    for i, (f, o, b, w) in enumerate(table):
        row = [got[32 * (i * W + q):32 * (i * W + q + 1)] for q in range(W)]
        assert row == [layer(files[f][o:o + b], W)[32 * q:32 * q + 32] for q in range(W)], (name, i)
        assert v2_ref.reduce_row(row[:w]).hex() == g["piece_hashes"][i], (name, i)


@pytest.mark.parametrize("seed", range(16))
def test_seeded_sweep(ctx, seed):
    d = v2_fuzz.draw(seed)
    L, W = d.L, d.L // LEAF
    table = d.table
    P = len(table)
    rng = random.Random(7100 + seed)
    ctx.set_layout(P * L, L, P)
    ctx.stage(0, rng.randbytes(P * L))                     # the rows hold other bytes past every piece's own
    for i, (f, o, b, w) in enumerate(table):
        ctx.stage(i * L, d.staged[f][o:o + b])
    clean = [layer(d.files[f][o:o + b], W) for f, o, b, w in table]
    dirty = [layer(d.staged[f][o:o + b], W) for f, o, b, w in table]
    assert clean != dirty                                  # the draw corrupts at least one block
    order = list(range(P)) + rng.sample(range(P), min(P, 3))
    rng.shuffle(order)
    nb, tl = [table[i][2] for i in order], [table[i][3] for i in order]
    # every piece's leaf layer (of the bytes staged: the corrupted ones)
    assert ctx.v2_leaf_hashes(order, nb, tl) == b"".join(dirty[i] for i in order)
    # random want bits over the corrupted blocks, against the uncorrupted layers
    pitch = (W + 7) // 8
    want = rng.randbytes(pitch * len(order))
    expect = bytearray(len(want))
    for k, i in enumerate(order):
        for q in held(table[i][2]):
            wanted = want[k * pitch + (q >> 3)] & (0x80 >> (q & 7))
            if wanted and clean[i][32 * q:32 * q + 32] == dirty[i][32 * q:32 * q + 32]:
                expect[k * pitch + (q >> 3)] |= 0x80 >> (q & 7)
    assert ctx.v2_check_blocks(order, nb, tl, b"".join(clean[i] for i in order), want) == bytes(expect)
    every = ctx.v2_check_blocks(order, nb, tl, b"".join(clean[i] for i in order))
    bad = {(i, pos // LEAF) for (i, pos) in d.corrupt}
    for k, i in enumerate(order):
        row = every[k * pitch:(k + 1) * pitch]
        assert row == row_of([q for q in held(table[i][2]) if (i, q) not in bad], W), (seed, i)
