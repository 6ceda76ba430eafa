"""The twin kernel's role-split rounds wave on the GPU: lane mapping, role masks, block entry, tail conversion.

In a twin rounds wave lanes 16r + k and 16r + 8 + k (k < 8) are the two roles of the wave's piece 8r + k; role b
reads helper lane 2(8r + k) + b's K+W words, role 0 writes the piece's outputs, and the verify bits of a wave are the
low byte of each 16 lanes of its ballot.  A wrong mapping, mask, odd/even block entry or tail conversion gives a wrong
digest, or the right bit at the wrong piece, at these sizes.  The twin kernel is forced (TV_OPT_KERNEL = 4) in its
2-wave and 4-wave workgroup (TV_OPT_SPLIT_PAIRS = 1 / 2), and everything is compared with hashlib:

  * pieces of 64, 128, 192, 448 and 16,384 bytes and of 55, 56, 63, 65, 119 and 120 bytes past 128 (1, 2, 3, 7 and 256
    full blocks: odd and even loop entries, one and two padded tail blocks), at 1 .. 65 pieces across the 8-, 16- and
    32-piece boundaries of the lane mapping, each also with a short last piece of the other length class: tv_hash;
  * tv_verify with exactly one digest corrupted, for each piece 0 .. 16 in turn, at 17 and 33 pieces;
  * the twin list kernel over a scrambled list with a duplicate;
  * a streamed column pass three launches wide, the chaining value going through the state buffer between them.
"""
import functools
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

TWIN = 4
SHAPES = {"2wave": 1, "4wave": 2}          # TV_OPT_SPLIT_PAIRS
LENGTHS = [64, 128, 192, 448, 16384] + [128 + d for d in (55, 56, 63, 65, 119, 120)]
COUNTS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 65]
_POOL = random.Random(20260).randbytes(16384 * 65 + 4096)


def _short(L):
    """A short last piece with a different block count than L's."""
    return L // 2 + 1


@functools.lru_cache(maxsize=None)
def _case(L, P, last, skew=0):
    """-> (payload, hashlib digests), one per shape of the shard, shared by the tests and workgroup shapes."""
    total = L * (P - 1) + last
    off = (L * 7 + P * 13 + last + skew) % 4096
    payload = _POOL[off:off + total]
    digests = b"".join(hashlib.sha1(payload[i * L:i * L + (last if i == P - 1 else L)]).digest() for i in range(P))
    return payload, digests


def _context(native, shape, **options):
    ctx = native.Context(0)
    ctx.set_option(native.TV_OPT_KERNEL, TWIN)
    ctx.set_option(native.TV_OPT_SPLIT_PAIRS, SHAPES[shape])
    for key, value in options.items():
        ctx.set_option(getattr(native, key), value)
    return ctx


def _bits(bf, P):
    return [(bf[i >> 3] >> (7 - (i & 7))) & 1 for i in range(P)]


def _corrupt(digests, pieces):
    out = bytearray(digests)
    for i in pieces:
        out[20 * i + (7 * i) % 20] ^= 1 << (i % 8)
    return bytes(out)


def _expected_bits(good, given, P):
    return [int(good[20 * i:20 * i + 20] == given[20 * i:20 * i + 20]) for i in range(P)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_hash_every_count(native, shape, L):
    with _context(native, shape) as ctx:
        for P in COUNTS:
            for last in (L, _short(L)):
                payload, good = _case(L, P, last)
                ctx.set_layout(len(payload), L, P)
                ctx.stage(0, payload)
                assert ctx.hash() == good, (L, P, last)
                assert ctx.last_kernel()[0] == TWIN


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("P", [17, 33])
def test_verify_one_corrupt_digest_at_each_index(native, shape, P):
    """The bit that clears is the corrupted piece's own: a transposed piece index cannot cancel out."""
    L = 192
    with _context(native, shape) as ctx:
        for last in (L, _short(L)):
            payload, good = _case(L, P, last)
            ctx.set_layout(len(payload), L, P)
            ctx.stage(0, payload)
            for i in range(17):
                given = _corrupt(good, [i])
                want = _expected_bits(good, given, P)
                assert want.count(0) == 1 and want[i] == 0
                ctx.set_digests(given)
                bf = ctx.verify()
                assert len(bf) == (P + 7) // 8 and _bits(bf, P) == want, (P, last, i)
                assert ctx.last_kernel()[0] == TWIN


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("L,P", [(183, 33), (448, 65)])
def test_list_kernel_scrambled_with_a_duplicate(native, shape, L, P):
    with _context(native, shape) as ctx:
        for last in (L, _short(L)):
            payload, good = _case(L, P, last)
            given = _corrupt(good, [0, 8, 9, 16, P - 1])
            want = _expected_bits(good, given, P)
            order = list(range(P))
            random.Random(P + last).shuffle(order)
            order = order[:P - 3] + [order[1], order[0], P - 1]       # duplicates, and the last piece again
            ctx.set_layout(len(payload), L, P)
            ctx.stage(0, payload)
            ctx.set_digests(given)
            assert list(ctx.verify_list(order)) == [want[i] for i in order], (L, P, last)
            assert ctx.last_kernel()[0] == TWIN


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C,L", [(128, 384), (128, 375), (192, 448)])
def test_streamed_columns_in_three_launches(native, shape, C, L):
    """Columns of C bytes split each piece into three launches (two, one and one or two blocks wide): the role-0 lane
    stores the chaining value and both roles load it in the next launch."""
    assert -(-L // C) == 3
    with _context(native, shape, TV_OPT_RESIDENT=0, TV_OPT_STREAM_CHUNK=C) as ctx:
        for P in (17, 33, 65):
            for last in (L, _short(L), 1):
                payload, good = _case(L, P, last, skew=C)
                given = _corrupt(good, [0, 8, P - 1])
                ctx.set_layout(len(payload), L, P)
                ctx.set_digests(given)
                bf = ctx.verify_host(payload)
                assert _bits(bf, P) == _expected_bits(good, given, P), (C, L, P, last)
                assert ctx.last_kernel() == (TWIN, 3)
