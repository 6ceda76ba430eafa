"""BitTorrent v2 (BEP 52) piece hashing restated with hashlib alone: the expected values of the v2 tests.  It shares no
code with torrent_amd.

Rules: a leaf is SHA-256 of a 16 KiB block of ONE file at its real length (the last block 1 .. 16,384 bytes, not
padded); an interior node is SHA-256(left || right); a leaf position past the file's end is 32 zero bytes.  Every file
starts a new piece.  A file longer than the piece length L has a piece layer of ceil(len / L) hashes, each the root of
the L / 16 KiB-leaf subtree of that piece (missing leaves zero); its pieces root pads the layer to a power of two with
the root of an all-zero-leaf piece subtree and reduces it.  A file of 1 .. L bytes is one piece whose hash is the pieces
root itself, over a tree only next_pow2(ceil(len / 16 KiB)) leaves wide.  A zero-length file has no piece.
"""
from __future__ import annotations

import hashlib

LEAF = 16384
ZERO = bytes(32)


def sha256(b) -> bytes:
    return hashlib.sha256(b).digest()


def next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


def reduce_row(row: list) -> bytes:
    """Root of a power-of-two row of 32-byte nodes."""
    assert row and len(row) & (len(row) - 1) == 0
    while len(row) > 1:
        row = [sha256(row[i] + row[i + 1]) for i in range(0, len(row), 2)]
    return row[0]


def leaf_hashes(data) -> list:
    mv = memoryview(data)
    return [sha256(mv[o:o + LEAF]) for o in range(0, len(mv), LEAF)]


def piece_root(data, width: int) -> bytes:
    """Root of the `width`-leaf tree over the bytes of one piece (1 .. width * 16 KiB bytes)."""
    leaves = leaf_hashes(data)
    assert 1 <= len(leaves) <= width
    return reduce_row(leaves + [ZERO] * (width - len(leaves)))


def zero_piece_root(L: int) -> bytes:
    return reduce_row([ZERO] * (L // LEAF))


def file_hashes(data, L: int):
    """(pieces root or None, piece layer bytes or b"", [expected hash of each piece]) of one file."""
    n = len(data)
    if n == 0:
        return None, b"", []
    if n <= L:
        root = piece_root(data, next_pow2(-(-n // LEAF)))
        return root, b"", [root]
    mv = memoryview(data)
    layer = [piece_root(mv[o:o + L], L // LEAF) for o in range(0, n, L)]
    root = reduce_row(layer + [zero_piece_root(L)] * (next_pow2(len(layer)) - len(layer)))
    return root, b"".join(layer), layer


def piece_table(lengths, L: int) -> list:
    """[(file index, offset in the file, bytes, tree leaves)] of every piece, in file order."""
    out = []
    for f, n in enumerate(lengths):
        for o in range(0, n, L):
            b = min(L, n - o)
            out.append((f, o, b, L // LEAF if n > L else next_pow2(-(-n // LEAF))))
    return out


def expected_bitfield(files, L: int, expected: list, have=None) -> bytes:
    """MSB-first have-bits of `files` (one bytes-like per file; None or a short buffer = the pieces it cannot supply
    are unreadable) against the expected piece hashes, for the declared `have` lengths (default: len of each)."""
    lengths = have if have is not None else [len(f) for f in files]
    table = piece_table(lengths, L)
    bits = bytearray((len(table) + 7) // 8)
    for i, (f, o, b, w) in enumerate(table):
        data = files[f]
        if data is None or len(data) < o + b:
            continue
        if piece_root(memoryview(data)[o:o + b], w) == expected[i]:
            bits[i >> 3] |= 0x80 >> (i & 7)
    return bytes(bits)
