"""SHA-1 pieces of 2^29 bytes and more on every kernel form and path, bit-exact against hashlib.

2^29 bytes is the shortest message whose 64-bit bit length has a non-zero high word (tv_block.h build_tail_block:
w[14] = bits >> 32), and every other piece of the suite is shorter: a form that wrote the low word only, or lost w[14]
in the helper's byte swap or the twin schedule, would pass everything else.  The same pieces take the per-piece block
counters past 2^23 (wave_geom's uni() truncations) and, streamed, give a ninth 64 MiB column: blk_begin = 2^23,
data_off = 2^29.  Shapes, payload and expected digests: tests/long_pieces.py (tests/test_long_pieces_ref.py checks
them and the C oracle on the CPU).

A piece is hashed by one lane or one lane pair, so a pass over 2^29 bytes takes seconds however few pieces there are,
and all pieces of a launch hash side by side.  Every test therefore makes exactly ONE SHA-1 pass (one launch; a stream:
one launch per column) over a payload with piece 1's last byte flipped, and expects 0b101: a set bit shows that the
length words and every block of that piece were right, the cleared bit that the byte past 2^29 - 2 was really read.
The device fills the payload itself (tv_fill_synthetic, tv_stream_fill_synthetic); only the hybrid test stages half a
gibibyte from the host.  Measured durations: profiles/long_pieces/README.md."""
import pytest

from tests import hybrid_util as hu
from tests import long_pieces as lp
from tests import synth
from tests import v1_columns as vc
from tests.long_pieces import BOTH, EDGE, RES

pytestmark = pytest.mark.gpu
FAMILIES = {"lane": vc.LANE, "split": vc.SPLIT, "twin": vc.TWIN}


def _context(native, kernel=0, pairs=0, lane_pairs=0, resident=1):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    ctx = native.Context(0)
    ctx.set_option(native.TV_OPT_RESIDENT, resident)
    ctx.set_option(native.TV_OPT_KERNEL, kernel)
    ctx.set_option(native.TV_OPT_SPLIT_PAIRS, pairs)
    ctx.set_option(native.TV_OPT_LANE_PAIRS, lane_pairs)
    return ctx


def _resident(ctx, shape, digests=None):
    """The shape's layout, the payload filled on the device, then piece 1's last byte flipped."""
    ctx.set_layout(lp.total(shape), shape.L, shape.P)
    if digests is not None:
        ctx.set_digests(digests)
    ctx.fill_synthetic(lp.SEED)
    ctx.stage(lp.bad_offset(shape), lp.bad_byte(shape))


# ---- A. resident verify, every form ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", list(vc.VARIANTS))
def test_resident_verify(native, variant):
    """RES: the full pieces' bit length is 2^32 exactly (high word 1, low word 0), the short last piece's 0xFFFFFFF8 in
    the same launch.  (Companion workgroups off: the grid is the form's own, which the counter then shows.)"""
    kernel, pairs, lane_pairs = vc.VARIANTS[variant]
    with _context(native, kernel, pairs, lane_pairs) as ctx:
        ctx.set_option(native.TV_OPT_TWIN_FILL, 0)
        _resident(ctx, RES, lp.digests(RES))
        assert ctx.verify() == lp.WANT
        assert ctx.last_kernel() == (kernel, 1)
        assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == vc.workgroups(variant, RES.P, short=True)


# ---- B. creation mode -----------------------------------------------------------------------------------------------------

def test_hash(native):
    """tv_hash with the library's own kernel choice: the three digests, piece 1's that of the flipped bytes."""
    good, flipped = lp.expected(RES)
    with _context(native) as ctx:
        _resident(ctx, RES)
        got = ctx.hash()
        assert [got[20 * i:20 * i + 20].hex() for i in range(RES.P)] == [good[0].hex(), flipped.hex(), good[2].hex()]
        assert flipped != good[lp.BAD]
        assert ctx.last_kernel()[1] == 1


# ---- C. incremental list --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", list(FAMILIES))
def test_verify_list(native, family):
    """BOTH (both length words non-zero, L no multiple of 64) through tv_verify_list: the short last piece first, in
    waves of its own (tv_plan.h list_plan)."""
    kernel = FAMILIES[family]
    with _context(native, kernel) as ctx:
        _resident(ctx, BOTH, lp.digests(BOTH))
        assert list(ctx.verify_list([2, 0, 1])) == [1, 1, 0]
        assert ctx.last_kernel() == (kernel, 1)


# ---- D. streamed columns, a piece longer than a ring slot --------------------------------------------------------------------

@pytest.mark.parametrize("family", list(FAMILIES))
def test_stream_nine_columns(native, family):
    """BOTH through tv_stream_begin .. tv_stream_end with no chunk option: columns of one 64 MiB ring slot, one row per
    request.  The ninth column holds 65 bytes of pieces 0 and 1 and only the padding block of piece 2; its launch has
    blk_begin = 2^23 and reads the chaining values the eighth wrote."""
    kernel = FAMILIES[family]
    L, P, _ = BOTH
    C, ncol, nreq = lp.columns(BOTH)
    assert (C, ncol, nreq) == (vc.SLOT, 9, 27)
    bad_col, bad_at = (L - 1) // C, (L - 1) % C
    assert (bad_col, bad_at) == (8, 64)
    with _context(native, kernel, resident=0) as ctx:
        ctx.set_option(native.TV_OPT_STREAM_CHUNK, 0)
        ctx.set_layout(lp.total(BOTH), L, P)
        ctx.set_digests(lp.digests(BOTH))
        ctx.stream_begin()
        seq = 0
        for col in range(ncol):
            for piece in range(P):
                seq += 1
                req = ctx.stream_next()
                # (the ninth column is as wide as what is left of a piece)
                assert (req.piece, req.rows, req.offset, req.width, req.seq) == (piece, 1, col * C, min(C, L - col * C),
                                                                                 seq)
                assert ctx.row_bytes(req, 0) == max(0, min(req.width, lp.piece_len(BOTH, piece) - req.offset))
                ctx.stream_fill_synthetic(req, lp.SEED)
                if (piece, col) == (lp.BAD, bad_col):
                    slot = ctx.stream_slot(req)
                    slot[bad_at] ^= lp.FLIP
                    assert bytes([slot[bad_at]]) == lp.bad_byte(BOTH)
                    slot.release()
                ctx.stream_commit(req)
        assert seq == nreq and ctx.stream_next().rows == 0
        assert ctx.stream_end() == lp.WANT
        assert ctx.last_kernel() == (kernel, 9)


# ---- E. hybrid, resident -----------------------------------------------------------------------------------------------------

def test_hybrid_pad_of_half_a_gibibyte(native):
    """One file of 2^29 + 16 KiB + 1 bytes under L = 2^29 with a trailing pad: piece 0 is a full 2^29-byte SHA-1
    message, piece 1 is 16,385 bytes and a pad range of 2^29 - 16,385 bytes, which tv_hybrid_pad_kernel zeroes in 8,192
    chunks of one row (stale 0xFF bytes staged first).  All three bitfields against tests/hybrid_util.Layout.verdicts;
    then the last file byte flipped, which clears piece 1 in all three."""
    n = EDGE + 16384 + 1
    lay = hu.Layout([synth.fill(lp.SEED + 1, 0, n)], EDGE, trailing=True)
    assert (lay.P, lay.pb, lay.tl, lay.total, lay.tails) == (2, [EDGE, 16385], [EDGE // 16384] * 2, 2 * EDGE, [1])
    assert -(-(EDGE - 16384) // 65536) == 8192              # the pad chunks (tv_plan.h hybrid_tails)

    def want(staged):
        ok1, ok2, _, _ = lay.verdicts(staged)
        return hu.pack([a and b for a, b in zip(ok1, ok2)]), hu.pack(ok1), hu.pack(ok2)

    with _context(native) as ctx:
        hu.load(ctx, lay, fill=0xFF)
        assert ctx.hybrid_verify() == (hu.pack([1, 1]),) * 3
        assert ctx.last_kernel() == (native.KERNEL_HYBRID, lay.launches())
        # the pad range reads as zeros at its ends and at a chunk edge; the bytes before it are the file's
        for off, k in ((16385, 63), (16384 + 65536 - 32, 64), (EDGE - 64, 64)):
            out = bytearray(k)
            ctx.read(EDGE + off, out)
            assert out == bytes(k), off
        out = bytearray(1)
        ctx.read(EDGE + 16384, out)
        assert out == lay.files[0][-1:]
        # (Layout.verdicts of the layout's own files compares its hashes with themselves: all ones, as asserted above)
        # second pass: the last file byte flipped
        bad = [hu.xor_at(lay.files[0], n - 1, 0x01)]
        ctx.stage(n - 1, bad[0][-1:])
        assert ctx.hybrid_verify() == want(bad) == (hu.pack([1, 0]),) * 3
