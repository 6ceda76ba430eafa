"""Differential sweep of the hybrid calls (tv_hybrid_verify, tv_hybrid_hash, tv_hybrid_pad_kernel) against hashlib SHA-1
over the padded linear bytes (tests/hybrid_util.py) and tests/v2_ref.py, bit-exact:

a. tails that start around every chunk boundary of the pad kernel (64 KiB) at L = 128 KiB, 256 KiB and 1 MiB, a full
   row on each side, every row read back in full;
b. every SHA-1 kernel (lane with single and with pair loads, split, twin, auto) after the pad kernel at L = 16 KiB,
   piece counts beside a twin workgroup, a split pair and a lane workgroup, corrupted bytes and flipped hashes;
c. shards that start and end off a byte of the bitfield, on one context (spare bits, the reused second bitfield);
d. the cached tail table zeroes again, and a new table on the same layout replaces it;
e. more tail entries than the first allocation of the tail table holds, then a small layout, then the large one again;
f. the caller's availability bits and pieces file staging could not read, together.

Before the files the whole shard is staged as 0xFF, so a pad byte the kernel does not zero cannot pass by luck.  A wrong
digest must not pass for a detected corruption: every corrupted staging is also hashed (tv_hybrid_hash) and compared
with the references of the corrupted bytes."""
import functools
import random

import pytest

from tests import hybrid_util as hu

gpu = pytest.mark.gpu                                        # (not the module: the chunk-class test below needs no GPU)
K = 1024
LEAF = 16384
C = 65536                                                    # kHybridChunk (torrent_amd/csrc/tv_plan.h)


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def _files(seed: int, lengths) -> list:
    blob = memoryview(random.Random(seed).randbytes(sum(lengths)))
    out, o = [], 0
    for n in lengths:
        out.append(bytes(blob[o:o + n]))
        o += n
    return out


def _check_clean(ctx, native, lay, first=0, count=None):
    """A staged, uncorrupted shard: both hash sets, the three bitfields, the launch count, every row's bytes."""
    count = lay.P - first if count is None else count
    d, r = ctx.hybrid_hash()
    assert d == lay.pieces[20 * first:20 * (first + count)]
    assert r == b"".join(lay.hashes[first:first + count])
    assert ctx.last_kernel() == (native.KERNEL_HYBRID, lay.launches(first, count))
    assert ctx.hybrid_verify() == (hu.pack([True] * count),) * 3
    assert ctx.last_kernel() == (native.KERNEL_HYBRID, lay.launches(first, count))
    got = hu.read_shard(ctx, lay, first, count)
    want = lay.linear[first * lay.L:(first + count) * lay.L]
    at = hu.first_difference(got, want)
    assert at is None, ("row", at // lay.L, "byte", at % lay.L, "piece_bytes", lay.pb[first + at // lay.L])


# ---- a. tail positions across chunk boundaries -----------------------------------------------------------------------

A_LENGTHS = [128 * K, 256 * K, 1024 * K]


def tail_starts(L: int) -> list:
    raw = [1, 15, 16, 17, C - 17, C - 16, C - 15, C - 1, C, C + 1, C + 16, L - C - 1, L - C, L - C + 1, L - C + 15,
           L - C + 16, L - C + 17, L - 17, L - 16, L - 15, L - 1]
    return sorted({b for b in raw if 0 < b < L})


def chunks_of(b: int, end: int) -> list:
    """The byte count of every chunk of a tail [b, end): tv_plan.h's rule restated (chunk k is the bytes of [b, end)
    inside [a0 + k C, a0 + (k + 1) C), a0 = b rounded down to 16)."""
    a0 = b // 16 * 16
    n = -(-(end - a0) // C)
    return [min(end, a0 + (k + 1) * C) - max(b, a0 + k * C) for k in range(n)]


def test_tail_starts_reach_every_chunk_class():
    """(no GPU work) What the starts of (a) give.  Of the counts 1, 2, 3, 4, 15, 16 and 17, 17 cannot occur: a tail of
    a 1 MiB row has at most ceil(L / C) = 16 chunks, since its first chunk starts at or after the row's byte 0."""
    counts, lasts, firsts, phases = set(), set(), set(), set()
    for L in A_LENGTHS:
        starts = tail_starts(L)
        assert len(starts) == (17 if L == 2 * C else 21) and all(0 < b < L for b in starts)
        per = {b: chunks_of(b, L) for b in starts}
        for b, cs in per.items():
            assert sum(cs) == L - b and all(0 < c <= C for c in cs) and all(c == C for c in cs[1:-1])
            counts.add(len(cs))
            lasts.add(cs[-1])
            firsts.add(cs[0])
            phases.add(b % 16)
        assert {len(cs) for cs in per.values()} == {2 * C: {1, 2}, 4 * C: {1, 2, 3, 4}, 16 * C: {1, 2, 15, 16}}[L]
        # a last chunk of exactly 16 bytes for every start in C - 16 .. C - 1, and multi-chunk tails that end a chunk
        assert all(per[b][-1] == 16 and len(per[b]) > 1 for b in (C - 16, C - 15, C - 1))
        assert per[C - 17][-1] == 32 and per[C][-1] == C and per[L - C] == [C]
        assert len(per[C]) == L // C - 1 and len(per[1]) == L // C and per[1][0] == C - 1
    assert counts == {1, 2, 3, 4, 15, 16}
    assert {16, 32, C} <= lasts and {1, 15, 16, 17, C - 1, C} <= firsts
    assert phases == {0, 1, 15}


@functools.lru_cache(maxsize=None)
def tail_layout(L: int, trailing: bool) -> hu.Layout:
    """A whole piece, then for every start b a file of b bytes and a whole piece; a last file of 12,345 bytes: a short
    last piece, or with `trailing` one more tail."""
    lengths = [L]
    for b in tail_starts(L):
        lengths += [b, L]
    lengths.append(12345)
    lay = hu.Layout(_files(6100 + L // K, lengths), L, trailing)
    assert lay.P == len(lengths) and lay.tails == list(range(1, lay.P - 1, 2)) + ([lay.P - 1] if trailing else [])
    assert all(lay.pb[i] == L for i in range(0, lay.P - 1, 2))
    return lay


@gpu
@pytest.mark.parametrize("trailing", [False, True])
@pytest.mark.parametrize("L", A_LENGTHS)
def test_tails_across_chunk_boundaries(ctx, native, L, trailing):
    lay = tail_layout(L, trailing)
    hu.load(ctx, lay)
    _check_clean(ctx, native, lay)
    # stale bytes in the pad ranges again (not 0xFF), the cached table: the same answers and the same rows
    hu.load(ctx, lay, fill=0x5A, relayout=False)
    _check_clean(ctx, native, lay)


# ---- b. every SHA-1 kernel after the pad kernel ----------------------------------------------------------------------

SMALL = [1, 55, 56, 63, 64, 65, 16383, 16384]
B_PIECES = [31, 33, 65, 129, 257, 300]
# (name, TV_OPT_KERNEL, TV_OPT_LANE_PAIRS)
PATHS = [("lane-single", 1, 2), ("lane-pairs", 1, 1), ("split", 2, 0), ("twin", 4, 0), ("auto", 0, 0)]


@functools.lru_cache(maxsize=None)
def small_layout(P: int, trailing: bool) -> hu.Layout:
    """P pieces of 16 KiB (every piece one leaf): mostly one-piece files of the SMALL lengths, a few of two and three
    pieces; the last file is shorter than a piece.  Both endings hold the same files."""
    L = 16 * K
    rng = random.Random(7300 + P)
    lengths = SMALL + [L + 55, 2 * L + 63]                  # (every length and both longer kinds at any P)
    pieces = sum(-(-n // L) for n in lengths)
    while pieces < P - 1:
        room, r = P - 1 - pieces, rng.random()
        if r < 0.06 and room >= 3:
            n = 2 * L + rng.choice(SMALL)
        elif r < 0.16 and room >= 2:
            n = L + rng.choice(SMALL)
        else:
            n = rng.choice(SMALL)
        n = min(n, room * L)
        lengths.append(n)
        pieces += -(-n // L)
    lengths.append(rng.choice(SMALL[:-1]))
    lay = hu.Layout(_files(7400 + P, lengths), L, trailing)
    assert lay.P == P and set(lay.tl) == {1} and lay.launches() == 4
    assert (P - 1 in lay.tails) == trailing and len(lay.tails) > P // 2
    assert any(n > 2 * L for n in lengths) and any(L < n <= 2 * L for n in lengths) and set(SMALL) <= set(lengths)
    return lay


def _corrupted(lay: hu.Layout):
    """The files with three bytes flipped: the last file byte before a tail, a byte inside a full piece, the last
    piece's first byte.  -> (staged files, the three pieces)."""
    inner = [i for i in lay.tails if i != lay.P - 1]
    full = [i for i in range(lay.P) if lay.pb[i] == lay.L]
    t, f, last = inner[len(inner) // 2], full[len(full) // 3], lay.P - 1
    staged = list(lay.files)
    for i, pos in ((t, lay.pb[t] - 1), (f, lay.L // 2 + 5), (last, 0)):
        k, o, _, _ = lay.table[i]
        staged[k] = hu.xor_at(staged[k], o + pos, 0x10)
    return staged, {t, f, last}


def _flip_pieces(P: int) -> list:
    return [0, P // 2, P - 1] + ([64 + 5, 128 + 17, 192 + 40, 256 + 3] if P == 300 else [])


@gpu
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("trailing", [False, True], ids=["short-last", "trailing-pad"])
@pytest.mark.parametrize("P", B_PIECES)
def test_every_sha1_kernel_after_the_pad_kernel(ctx, native, P, trailing, path):
    from torrent_amd.hybrid import HybridResult
    lay = small_layout(P, trailing)
    _, kernel, pairs = path
    allset = hu.pack([True] * P)
    ctx.set_option(native.TV_OPT_KERNEL, kernel)
    ctx.set_option(native.TV_OPT_LANE_PAIRS, pairs)
    try:
        hu.load(ctx, lay)
        _check_clean(ctx, native, lay)
        # the v1 and the v2 call on the same staging keep their own answers
        assert ctx.verify() == allset and ctx.last_kernel() == (kernel or native.KERNEL_TWIN, 1)
        assert ctx.v2_verify() == allset and ctx.last_kernel()[0] == native.KERNEL_V2
        # three corrupted pieces: exactly their bits clear in all three fields, and the hashes are the corrupted bytes'
        staged, bad = _corrupted(lay)
        ok1, ok2, d, r = lay.verdicts(staged)
        assert [i for i in range(P) if not ok1[i]] == sorted(bad) == [i for i in range(P) if not ok2[i]]
        hu.load(ctx, lay, staged=staged)
        want = hu.pack([i not in bad for i in range(P)])
        assert ctx.hybrid_verify() == (want,) * 3
        assert ctx.hybrid_hash() == (d, b"".join(r))
        assert ctx.verify() == want and ctx.v2_verify() == want
        # one bit of one v1 digest, of one v2 hash: only that field disagrees, and `both` is the AND
        hu.load(ctx, lay, relayout=False)
        for i in _flip_pieces(P):
            less = hu.pack([j != i for j in range(P)])
            ctx.set_digests(hu.xor_at(lay.pieces, 20 * i + i % 20, 1 << (i % 8)))
            both, v1, v2 = ctx.hybrid_verify()
            assert (both, v1, v2) == (less, less, allset), i
            assert HybridResult(bytearray(both), bytearray(v1), bytearray(v2)).disagree == [i]
            assert ctx.verify() == less and ctx.v2_verify() == allset
            ctx.set_digests(lay.pieces)
            hs = list(lay.hashes)
            hs[i] = hu.xor_at(hs[i], i % 32, 0x80 >> (i % 8))
            ctx.v2_set_pieces(lay.pb, lay.tl, b"".join(hs))
            both, v1, v2 = ctx.hybrid_verify()
            assert (both, v1, v2) == (less, allset, less), i
            assert HybridResult(bytearray(both), bytearray(v1), bytearray(v2)).disagree == [i]
            ctx.v2_set_pieces(lay.pb, lay.tl, b"".join(lay.hashes))
        assert ctx.hybrid_verify() == (allset,) * 3
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, 0)


# ---- c. spare bits and shards ----------------------------------------------------------------------------------------

SHARDS = [(0, 300), (0, 67), (67, 61), (128, 172), (5, 70)]


@gpu
def test_shards_off_the_byte_boundaries(ctx, native):
    """The shards run in this order on one context: the second bitfield and the v2 table are reused at a smaller and
    then at a larger size.  (67, 61) and (5, 70) cannot be set as they stand -- shard_first is a multiple of 8 --: the
    refusal is asserted, and they run as (64, 61) and (0, 70)."""
    P = 300
    lay = small_layout(P, False)
    staged, bad = _corrupted(lay)
    pieces, hashes = lay.pieces, list(lay.hashes)
    flip1, flip2 = [3, 66, 67, 130, 299], [5, 74, 127, 128, 290]
    assert not (set(flip1) | set(flip2)) & (bad - {P - 1})
    for i in flip1:
        pieces = hu.xor_at(pieces, 20 * i + 19, 0x01)
    for i in flip2:
        hashes[i] = hu.xor_at(hashes[i], 0, 0x80)
    ok1, ok2, d, r = lay.verdicts(staged, pieces, hashes)
    assert [i for i in range(P) if not ok1[i]] == sorted(bad | set(flip1))
    assert [i for i in range(P) if not ok2[i]] == sorted(bad | set(flip2))
    for first, count in SHARDS:
        if first % 8:
            # a shard starts a byte of the bitfield (tv_set_layout's contract: the shards' bitfields are joined as
            # bytes); such a case keeps its piece count and ends off a byte, from the byte its first piece lies in
            with pytest.raises(native.NativeError) as ei:
                ctx.set_layout(lay.total, lay.L, P, first, count)
            assert ei.value.code == native.TV_ERR_ARG
            first -= first % 8
        hu.load(ctx, lay, first, count, pieces=pieces, hashes=hashes, staged=staged)
        s1, s2 = ok1[first:first + count], ok2[first:first + count]
        want = (hu.pack([a and b for a, b in zip(s1, s2)]), hu.pack(s1), hu.pack(s2))
        got = ctx.hybrid_verify()
        assert got == want, (first, count)
        assert ctx.last_kernel() == (native.KERNEL_HYBRID, lay.launches(first, count))
        if count % 8:
            assert all(f[-1] & (0xFF >> (count % 8)) == 0 for f in got), (first, count)
        held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
        assert ctx.hybrid_verify() == want
        assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == held
        sl = slice(first, first + count)
        assert ctx.hybrid_hash() == (d[20 * first:20 * (first + count)], b"".join(r[sl])), (first, count)
        assert ctx.verify() == want[1] and ctx.v2_verify() == want[2]


# ---- d. the cached table really zeroes, and a new table replaces it --------------------------------------------------

@gpu
def test_cached_table_zeroes_again_and_a_new_table_replaces_it(ctx, native):
    L = 128 * K
    starts = [1, C - 16, C, C + 17, L - 15, 4000]
    a_len, b_len = [], []
    for k, b in enumerate(starts):
        a_len += [b, L]                                     # A: even rows hold a tail, odd rows are full
        b_len += [L, starts[(k + 1) % len(starts)]]          # B: the reverse
    A = hu.Layout(_files(6500, a_len), L, True)
    B = hu.Layout(_files(6600, b_len), L, True)
    P = A.P
    assert P == B.P == 12 and A.total == B.total == P * L
    assert A.tails == list(range(0, P, 2)) and B.tails == list(range(1, P, 2))
    hu.load(ctx, A)
    _check_clean(ctx, native, A)
    held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    # 0xFF over everything and the files again, the table cached on the device: every pad range is zeroed again
    hu.load(ctx, A, relayout=False)
    assert hu.read_shard(ctx, A) != A.linear
    _check_clean(ctx, native, A)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == held
    # another file set on the same layout: tails become full rows and full rows tails
    ctx.v2_set_pieces(B.pb, B.tl, b"".join(B.hashes))
    ctx.set_digests(B.pieces)
    hu.load(ctx, B, relayout=False)
    _check_clean(ctx, native, B)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == held
    # and back, without staging the fill: B's full rows keep their bytes where A has a pad range until the call
    ctx.v2_set_pieces(A.pb, A.tl, b"".join(A.hashes))
    ctx.set_digests(A.pieces)
    hu.load(ctx, A, relayout=False, fill=None)
    _check_clean(ctx, native, A)


# ---- e. tail-table growth --------------------------------------------------------------------------------------------

CYCLE = [1, 15, 16, 17, 55, 56, 63, 64, 65, 1000, 4095, 4096, 4097, 8191, 8192, 16367, 16368, 16369, 16383, 16384, 9999,
         12345, 333]


@functools.lru_cache(maxsize=None)
def many_tails() -> hu.Layout:
    lengths = [CYCLE[k % len(CYCLE)] for k in range(1100)]
    lay = hu.Layout(_files(6700, lengths), 16 * K, False)
    assert lay.P == 1100 and 1024 < len(lay.tails) < 1100
    return lay


@gpu
def test_tail_table_grows_is_released_and_grows_again(ctx, native):
    big, small = many_tails(), small_layout(31, True)
    hu.load(ctx, small)                                      # (the tail table, if any, is the first allocation's size)
    _check_clean(ctx, native, small)
    hu.load(ctx, big)
    held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    _check_clean(ctx, native, big)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) - held <= 2 + 1     # tail table and second bitfield, one regrow
    # a small layout after it: the grown table is far larger than it needs and is released
    hu.load(ctx, small)
    held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    _check_clean(ctx, native, small)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) - held == 1        # (a table of the first size again)
    hu.load(ctx, big)
    held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    _check_clean(ctx, native, big)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) - held <= 2 + 1
    staged, bad = _corrupted(big)
    hu.load(ctx, big, staged=staged)
    assert ctx.hybrid_verify() == (hu.pack([i not in bad for i in range(big.P)]),) * 3


# ---- f. availability -------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("trailing", [False, True], ids=["short-last", "trailing-pad"])
def test_caller_bits_and_unreadable_files_together(ctx, native, tmp_path, trailing):
    P = 129
    lay = small_layout(P, trailing)
    staged, bad = _corrupted(lay)
    ok = [i not in bad for i in range(P)]
    hu.load(ctx, lay, staged=staged)
    # two files that do not exist, in different words of the output: the one holding piece 20, the one holding 100
    unread = set()
    for i in (20, 100):
        k = lay.table[i][0]
        p0, n = lay.first_piece(k), -(-lay.lengths[k] // lay.L)
        assert p0 // 64 == i // 64 and not set(range(p0, p0 + n)) & bad
        assert ctx.stage_file(str(tmp_path / ("missing%d.bin" % i)), 0, lay.offs[k], lay.lengths[k]) is False
        unread |= set(range(p0, p0 + n))
    mask = random.Random(6800).randbytes((P + 7) // 8)
    m = [bool((mask[i >> 3] >> (7 - (i & 7))) & 1) for i in range(P)]
    assert 30 < sum(m) < 100 and any(m[i] for i in bad) and any(m[i] for i in unread)
    want = hu.pack([ok[i] and m[i] and i not in unread for i in range(P)])
    assert ctx.hybrid_verify(mask) == (want,) * 3
    # without a mask only the unreadable (and the corrupted) pieces are clear
    want = hu.pack([ok[i] and i not in unread for i in range(P)])
    assert ctx.hybrid_verify() == (want,) * 3
    assert ctx.hybrid_verify(bytes([0xFF]) * len(mask)) == (want,) * 3
    assert ctx.verify() == want and ctx.v2_verify() == want
