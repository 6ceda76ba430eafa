"""The twin kernel's rounds loop on small shapes where its block-count handling can go wrong.

The rounds wave's loop consumes the blocks every lane of a workgroup has in common; whatever the loop is
unrolled by (its K+W ring has three buffers, and a loop trip may cover more than one block), the blocks
before, inside and after it must be exactly the piece's blocks, in order, for every block count and
parity, and the padded tail blocks must follow on the right ring buffer.  Here the twin kernel is forced
(TV_OPT_KERNEL = 4) and compared with hashlib for

  * piece lengths of 1 to 7 blocks (counting the padding block), in every padding class: 64 k - 9 (the
    padding fits the last data block), 64 k - 8 (the length field no longer fits: one more block), 64 k
    (a padding block of its own) and 64 k + 1;
  * a short last piece whose block count has the other parity than the full pieces';
  * 1, 31, 32, 33, 64 and 96 pieces: a lone partial workgroup, exactly one, one and a bit, two, three,
    with companion workgroups (TV_OPT_TWIN_FILL) on and off;
  * creation mode (tv_hash), tv_verify with one digest in seven corrupted, and the twin list kernel
    (tv_verify_list) over the same pieces in shuffled order.

The split kernel runs the same helper-wave and rounds-wave bodies as the twin kernel (tv_kernels.hip helper_wave /
rounds_wave), so the same lengths, counts, short last pieces and checks also run with the 2-pair twin workgroup
(TV_OPT_SPLIT_PAIRS = 2) and with the split kernel forced (TV_OPT_KERNEL = 2) at 1 and 2 pairs per workgroup.  A
split workgroup covers 64 pieces per pair, so its rows add 65, 128 and 129 pieces: one 1-pair workgroup and a bit,
exactly two, two and a bit.

The lane kernel (TV_OPT_KERNEL = 1) runs the same matrix with its 3-deep register ring and with its ring of two pairs
(TV_OPT_LANE_PAIRS = 2 / 1): its workgroup is four waves of 64 pieces, so its rows add 63, 65, 255, 256 and 257
pieces.  With the lane kernel forced the list call runs tv_list_kernel, whose two-deep A/B ring with clamped prologue
loads so sees every length and every short last piece here.
"""
import hashlib
import random

import pytest

TWIN = 4
SPLIT = 2
LANE = 1
# the other kernels on the shared wave bodies, and the lane kernel's two rings:
# name -> (TV_OPT_KERNEL, TV_OPT_SPLIT_PAIRS, TV_OPT_LANE_PAIRS)
VARIANTS = {"twin2": (TWIN, 2, 0), "split1": (SPLIT, 1, 0), "split2": (SPLIT, 2, 0),
            "lane3": (LANE, 0, 2), "lanepairs": (LANE, 0, 1)}
COUNTS = [1, 31, 32, 33, 64, 96]
SPLIT_COUNTS = [65, 128, 129]
LANE_COUNTS = [63, 65, 255, 256, 257]
EXTRA_COUNTS = {SPLIT: SPLIT_COUNTS, LANE: LANE_COUNTS}
# 64 k - 9, 64 k - 8, 64 k, 64 k + 1 for k = 1 .. 6 (k, k + 1, k + 1, k + 1 blocks), and the one-byte piece
LENGTHS = [1] + [64 * k + d for k in range(1, 7) for d in (-9, -8, 0, 1)]


def _nblocks(n):
    return (n + 8) // 64 + 1


def _digests(payload, L, P, last):
    return b"".join(hashlib.sha1(payload[i * L:i * L + (last if i == P - 1 else L)]).digest() for i in range(P))


def _bits(bf, P):
    return [(bf[i >> 3] >> (7 - (i & 7))) & 1 for i in range(P)]


def _check(native, ctx, L, P, last, seed, kernel=TWIN):
    total = L * (P - 1) + last
    rng = random.Random(seed)
    payload = rng.randbytes(total)
    good = _digests(payload, L, P, last)
    ctx.set_layout(total, L, P)
    ctx.stage(0, payload)
    assert ctx.hash() == good, (L, P, last)
    assert ctx.last_kernel()[0] == kernel
    bad = set(range(P // 2 % 7, P, 7))          # one digest in seven
    pieces = bytearray(good)
    for i in bad:
        pieces[20 * i + i % 20] ^= 1 << (i % 8)
    ctx.set_digests(bytes(pieces))
    want = [0 if i in bad else 1 for i in range(P)]
    bf = ctx.verify()
    assert len(bf) == (P + 7) // 8 and _bits(bf, P) == want, (L, P, last)
    assert ctx.last_kernel()[0] == kernel
    order = list(range(P))
    rng.shuffle(order)
    assert list(ctx.verify_list(order)) == [want[i] for i in order], (L, P, last)
    assert ctx.last_kernel()[0] == kernel              # (forced: the list call runs that kernel's list form)


def test_lengths_cover_every_block_count_and_padding_class():
    """(CPU) The shapes above are what the docstring says: block counts 1 .. 6 (and 7), each padding class."""
    by_class = {d: sorted(_nblocks(64 * k + d) for k in range(1, 7)) for d in (-9, -8, 0, 1)}
    assert by_class[-9] == [1, 2, 3, 4, 5, 6]
    assert by_class[-8] == by_class[0] == by_class[1] == [2, 3, 4, 5, 6, 7]
    assert _nblocks(1) == 1 and _nblocks(55) == 1 and _nblocks(56) == 2


def _block_counts(native, ctx, P, kernel):
    for L in LENGTHS:
        _check(native, ctx, L, P, L, seed=L * 131 + P, kernel=kernel)


def _short_last_piece(native, ctx, P, kernel):
    for L in [l for l in LENGTHS if _nblocks(l) >= 2]:
        lasts = {L - 64 if L > 64 else L - 9, 1}
        assert any(_nblocks(x) % 2 != _nblocks(L) % 2 for x in lasts)
        for last in sorted(lasts):
            _check(native, ctx, L, P, last, seed=L * 977 + P * 7 + last, kernel=kernel)
    assert _nblocks(16384) == 257 and _nblocks(8192) == 129
    _check(native, ctx, 16384, P, 8192 - 64, seed=P, kernel=kernel)          # 257 blocks, last piece 128
    _check(native, ctx, 16384 - 64, P, 8192, seed=P + 1, kernel=kernel)      # 256 blocks, last piece 129


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [1, 0])
@pytest.mark.parametrize("P", COUNTS)
def test_twin_block_counts(native, P, fill):
    """Every length of LENGTHS at P equal pieces (no short last piece)."""
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_KERNEL, TWIN)
        ctx.set_option(native.TV_OPT_TWIN_FILL, fill)
        _block_counts(native, ctx, P, TWIN)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [1, 0])
@pytest.mark.parametrize("P", [2, 33, 65, 97])
def test_twin_short_last_piece_of_other_parity(native, P, fill):
    """Full pieces of 2 .. 7 blocks with a short last piece of one block fewer (the other parity) and of a
    single block; also long full pieces (16 KiB: 257 blocks, and 256: many trips of the loop) with a last
    piece of 128 and of 129 blocks."""
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_KERNEL, TWIN)
        ctx.set_option(native.TV_OPT_TWIN_FILL, fill)
        _short_last_piece(native, ctx, P, TWIN)


def _variant_cases(counts):
    """(variant, P): the twin counts for every variant, and for the split and lane rows their own counts too."""
    return [(v, P) for v, (kernel, _, _) in VARIANTS.items()
            for P in counts + [c for c in EXTRA_COUNTS.get(kernel, []) if c not in counts]]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,P", _variant_cases(COUNTS))
def test_variant_block_counts(native, variant, P):
    """As test_twin_block_counts, for the 2-pair twin workgroup, the split kernel at 1 and 2 pairs and the lane kernel's
    two rings."""
    kernel, pairs, lane_pairs = VARIANTS[variant]
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_KERNEL, kernel)
        ctx.set_option(native.TV_OPT_SPLIT_PAIRS, pairs)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, lane_pairs)
        _block_counts(native, ctx, P, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,P", _variant_cases([2, 33, 65, 97]))
def test_variant_short_last_piece_of_other_parity(native, variant, P):
    """As test_twin_short_last_piece_of_other_parity, for the 2-pair twin workgroup and the split kernel at 1 and
    2 pairs (the short last piece's own workgroup follows 1, 32, 64, 96 and, split, 127 and 128 full pieces) and the
    lane kernel's two rings (its own wave follows 62, 64, 254, 255 and 256 full pieces too)."""
    kernel, pairs, lane_pairs = VARIANTS[variant]
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_KERNEL, kernel)
        ctx.set_option(native.TV_OPT_SPLIT_PAIRS, pairs)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, lane_pairs)
        _short_last_piece(native, ctx, P, kernel)
