"""The call-time device buffers, one context through every call kind: the list buffers of tv_verify_list, the piece
table and node buffers of tv_v2_set_pieces, the entry tables of tv_v2_verify_list and of the block calls, the tail
table and the two bit-word halves of a hybrid verify, the chunk buffers, table and nodes of a v2 stream.  After each
call the growth of TV_COUNTER_DEVICE_BYTES and TV_COUNTER_DEVICE_ALLOCS is held to the sizes the library documents
(restated below), a repeat of the call moves neither counter, and a layout of 0 pieces keeps only what tv_set_layout's
rules keep.  The results of the calls are checked against hashlib on the way.

Shape: L = 64 KiB (W = 4 leaves), 12 pieces in two files, so that piece 5 has a pad tail (a hybrid torrent's v1 space)
and piece 11 is short."""
import hashlib

import pytest

from tests import hybrid_util, synth

pytestmark = pytest.mark.gpu

K = 1 << 10
L, LEAF, W, P = 64 * K, 16 * K, 4, 12
LIST_MIN = 1024                       # entries a list / item / tail buffer is allocated for at least


def node_words(count, width):
    """tv_v2.hip v2_node_words: level buffers A [8][count x width] and B [8][count x max(width / 2, 1)]."""
    return 8 * count * (width + (width // 2 if width > 1 else 1))


def leaf_layer(data: bytes) -> bytes:
    """32 x W bytes: SHA-256 of every 16 KiB block that holds bytes, zero hashes out to W."""
    out = b"".join(hashlib.sha256(data[o:o + LEAF]).digest() for o in range(0, len(data), LEAF))
    return out + bytes(32 * W - len(out))


def run_v2_stream(ctx, lay):
    """One v2 stream over the shard, every request filled from the layout's bytes -> the bitfield."""
    ctx.v2_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes))
    while True:
        req = ctx.stream_next()
        if req.rows == 0:
            return ctx.stream_end()
        assert req.width == LEAF                                   # one-leaf columns
        slot = ctx.stream_slot(req)
        for q in range(req.rows):
            n = ctx.row_bytes(req, q)
            at = (req.piece + q) * L + req.offset
            slot[q * req.width:q * req.width + n] = lay.linear[at:at + n]
        slot.release()
        ctx.stream_commit(req)


def test_call_buffers_grow_once_by_their_documented_sizes(native):
    N = native
    lay = hybrid_util.Layout([bytes(synth.fill(31, 0, 5 * L + 100)), bytes(synth.fill(32, 0, 5 * L + 1000))], L)
    assert (lay.P, lay.tails, lay.pb[-1]) == (P, [5], 1000)
    hashes = b"".join(lay.hashes)
    piece = lambda i: lay.linear[i * L:i * L + lay.pb[i]]           # noqa: E731
    with N.Context(0) as ctx:
        counters = lambda: (ctx.counter(N.TV_COUNTER_DEVICE_BYTES), ctx.counter(N.TV_COUNTER_DEVICE_ALLOCS))  # noqa: E731

        def step(what, call, want, grow_bytes, grow_allocs):
            """The call grows both counters by exactly this much, gives `want`, and a repeat moves neither."""
            b0, a0 = counters()
            assert call() == want, what
            b1, a1 = counters()
            print(f"{what}: +{b1 - b0} bytes, +{a1 - a0} allocations")
            assert (b1 - b0, a1 - a0) == (grow_bytes, grow_allocs), what
            assert call() == want, what
            assert counters() == (b1, a1), what

        ctx.set_layout(0, L, 0)
        assert counters() == (0, 0)
        ctx.set_layout(lay.total, L, P)
        ctx.set_digests(lay.pieces)
        hybrid_util.load(ctx, lay, fill=0, relayout=False)
        bit_words = 4                                               # 64-bit words, whole 256-piece groups
        payload = ctx.counter(N.TV_COUNTER_PAYLOAD_BYTES)
        per_layout = P * 3 * 5 * 4 + bit_words * 8 * 3              # digests / state / hash rows, three bit-word buffers
        assert counters() == (payload + per_layout, 1 + 3 + 3)

        some = [0, 5, 11]
        pb, tl = [lay.pb[i] for i in some], [lay.tl[i] for i in some]
        step("tv_verify_list", lambda: ctx.verify_list(some), b"\1\1\1", 9 * LIST_MIN, 2)
        step("tv_v2_set_pieces", lambda: ctx.v2_set_pieces(lay.pb, lay.tl, hashes), None,
             18 * P * 4 + node_words(P, W) * 4, 2)
        step("tv_v2_verify_list", lambda: ctx.v2_verify_list(some, pb, tl, b"".join(lay.hashes[i] for i in some)),
             b"\1\1\1", 48 * LIST_MIN, 1)
        two = [1, 11]
        step("tv_v2_check_blocks",
             lambda: ctx.v2_check_blocks(two, [lay.pb[i] for i in two], [lay.tl[i] for i in two],
                                         b"".join(leaf_layer(piece(i)) for i in two)),
             b"\xf0\x80", 48 * LIST_MIN, 1)
        step("tv_v2_leaf_hashes", lambda: ctx.v2_leaf_hashes([5], [lay.pb[5]], [lay.tl[5]]), leaf_layer(piece(5)),
             0, 0)                                                  # (the block calls share one buffer)

        # a hybrid layout of the same size: everything above is reused
        before = counters()
        hybrid_util.load(ctx, lay, fill=0)
        assert counters() == before
        ones = hybrid_util.bits(P)
        step("tv_hybrid_verify", ctx.hybrid_verify, (ones, ones, ones),
             16 * max(len(lay.tails), LIST_MIN) + 2 * bit_words * 8, 2)

        ctx.set_option(N.TV_OPT_STREAM_CHUNK, LEAF)
        chunk = (LEAF + 256) * P + 256                              # rows of C + 256 bytes and the slack after them
        step("tv_v2_stream_begin", lambda: run_v2_stream(ctx, lay), ones,
             2 * chunk + 11 * P * 4 + node_words(P, L // LEAF) * 4, 4)

        # an empty layout: no payload, no v2 piece table, no stream table; the buffers tv_set_layout's rules keep for a
        # shard of any size stay (per-piece rows and bit words, the list / item / tail buffers at their minimum, the
        # chunk buffers)
        allocs = counters()[1]
        ctx.set_layout(0, L, 0)
        assert ctx.counter(N.TV_COUNTER_PAYLOAD_BYTES) == 0
        assert counters() == (per_layout + 9 * LIST_MIN + 2 * 48 * LIST_MIN + 16 * LIST_MIN + 2 * bit_words * 8 +
                              2 * chunk, allocs)
