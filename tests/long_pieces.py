"""Shapes and expected values of the long-piece tests (tests/test_long_pieces_ref.py, tests/test_gpu_long_pieces.py):
SHA-1 pieces of 2^29 bytes and more, the smallest whose 64-bit bit length has a non-zero high word.  It imports nothing
from torrent_amd.

A SHA-1 message ends with its length in bits as two big-endian words.  Every shorter piece of the suite has a zero
high word, so a kernel that wrote the low word only would pass it.  Here:

  RES  = 3 pieces of L = 2^29, the last of 2^29 - 1 bytes.  The full pieces have bits = 2^32 exactly (high word 1, low
         word 0); the short last piece has bits = 0xFFFFFFF8, the control just below the edge, in the same launch.
  BOTH = 3 pieces of L = 2^29 + 65, the last of 2^29 bytes.  L is no multiple of 64 and both length words are non-zero
         (1 and 0x208); the last piece ends on a block boundary and on a 64 MiB column boundary, so its only padded
         block holds no data.  Streamed, a piece is nine columns of one ring slot: the ninth holds 65 bytes of pieces 0
         and 1 and the padding block of piece 2, and starts at block 2^23.

The payload is tests/synth.fill's generator at SEED: the device fills the same bytes itself (tv_fill_synthetic,
tv_stream_fill_synthetic), so no gibibyte buffer crosses PCIe.  The expected digests are hashlib's, computed once per
shape, three pieces at a time.  The BAD piece is piece 1 with its LAST byte XOR 0x01, at piece offset L - 1 >= 2^29 - 1:
a verify that reports it good has not read that byte."""
from __future__ import annotations

import functools
import hashlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

from tests import synth
from tests.v1_columns import SLOT, nblocks, stream_column  # noqa: F401  (restated geometry, re-exported)

EDGE = 1 << 29
SEED = 0x10C9_91EC
BAD = 1                    # the corrupted piece
FLIP = 0x01                # XOR of its last byte

Shape = namedtuple("Shape", "L P last")
RES = Shape(EDGE, 3, EDGE - 1)
BOTH = Shape(EDGE + 65, 3, EDGE)


def total(s: Shape) -> int:
    return s.L * (s.P - 1) + s.last


def piece_len(s: Shape, i: int) -> int:
    return s.last if i == s.P - 1 else s.L


def length_words(n: int) -> tuple:
    """(high, low) word of the bit length that ends a SHA-1 message of n bytes."""
    bits = 8 * n
    return bits >> 32, bits & 0xFFFFFFFF


def bad_offset(s: Shape) -> int:
    """Linear offset of the corrupted byte: the last byte of piece BAD."""
    return BAD * s.L + s.L - 1


def bad_byte(s: Shape) -> bytes:
    """The corrupted byte's value (the generator's byte XOR FLIP), as tv_stage takes it."""
    return bytes([synth.fill(SEED, bad_offset(s), 1)[0] ^ FLIP])


def columns(s: Shape, count: int = 0) -> tuple:
    """(column bytes, columns per piece, requests) of a stream over `count` pieces (default: all) with no chunk option:
    a piece longer than a ring slot gives one row per request."""
    count = count or s.P
    C = stream_column(s.L, count, 0)
    ncol = -(-s.L // C)
    return C, ncol, ncol * -(-count // max(1, SLOT // C))


@functools.lru_cache(maxsize=None)
def expected(s: Shape) -> tuple:
    """(hashlib SHA-1 of every piece of the intact payload, that of piece BAD with its last byte flipped)."""
    def one(i):
        n = piece_len(s, i)
        buf = synth.fill(SEED, i * s.L, n, threads=1)
        h = hashlib.sha1(memoryview(buf)[:n - 1])
        g = h.copy()
        h.update(bytes([buf[n - 1]]))
        g.update(bytes([buf[n - 1] ^ FLIP]))
        return h.digest(), g.digest()

    with ThreadPoolExecutor(3) as ex:             # (numpy and hashlib release the GIL; one piece per thread)
        both = list(ex.map(one, range(s.P)))
    return tuple(d for d, _ in both), both[BAD][1]


def digests(s: Shape) -> bytes:
    """The v1 `pieces` string of the intact payload."""
    return b"".join(expected(s)[0])


def digests_flipped(s: Shape) -> bytes:
    """The `pieces` string of the payload with the corrupted byte."""
    good, bad = expected(s)
    return b"".join(bad if i == BAD else d for i, d in enumerate(good))


def pack(bits) -> bytes:
    """MSB-first bitfield."""
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


WANT = pack([1, 0, 1])     # what every verify over the corrupted payload must report: 0b101
