"""Shared by the hybrid tests: hybrid .torrent fixtures with real BEP 47 pad entries, written with the tests' own
bencoder (tests/v2_util.py), and the expected values from hashlib (SHA-1 over the padded linear bytes) and tests/v2_ref.py
(the merkle side).  It shares no code with torrent_amd."""
from __future__ import annotations

import hashlib

from tests import v2_ref, v2_util


def pad_len(n: int, L: int) -> int:
    return -n % L


def padded_linear(files, L: int, trailing_pad: bool = False) -> bytes:
    """The v1 linear space of a hybrid torrent: every file followed by zeros up to the next piece boundary, except the
    last file that holds bytes (unless trailing_pad)."""
    last = max((k for k, d in enumerate(files) if len(d)), default=-1)
    out = bytearray()
    for k, d in enumerate(files):
        out += d
        if len(d) and (k != last or trailing_pad):
            out += bytes(pad_len(len(d), L))
    return bytes(out)


def v1_pieces(files, L: int, trailing_pad: bool = False) -> bytes:
    lin = padded_linear(files, L, trailing_pad)
    return b"".join(hashlib.sha1(lin[o:o + L]).digest() for o in range(0, len(lin), L))


def v2_expected(files, L: int) -> list:
    """The expected hash of every piece, in piece order."""
    out = []
    for d in files:
        out += v2_ref.file_hashes(d, L)[2]
    return out


def v1_file_list(files, paths, L: int, trailing_pad: bool = False) -> list:
    """The v1 `files` list with a pad entry after every file that does not end a piece and is followed by a file that
    holds bytes (and after the last one with trailing_pad)."""
    last = max((k for k, d in enumerate(files) if len(d)), default=-1)
    out = []
    for k, (comps, d) in enumerate(zip(paths, files)):
        out.append({"length": len(d), "path": list(comps)})
        n = pad_len(len(d), L)
        if n and len(d) and (k != last or trailing_pad):
            out.append({"attr": "p", "length": n, "path": [".pad", str(n)]})
    return out


def torrent_hybrid(files, L: int, name: str = "t", paths=None, trailing_pad: bool = False, pieces: bytes | None = None,
                   v1_files=None, single: bool = False, mutate=None) -> bytes:
    """A hybrid .torrent for `files` (bytes per file, file-tree order = list order).  pieces: the v1 `pieces` string
    (default: hashlib over the padded linear bytes).  v1_files: the v1 `files` list (default: v1_file_list).  single:
    one file described by `length` and `name`.  mutate(top) may edit the dictionary before it is encoded."""
    paths = [[name]] if single else (paths or v2_util.file_names(len(files)))

    def add_v1(top):
        info = top["info"]
        if single:
            info["length"] = len(files[0])
        else:
            info["files"] = v1_file_list(files, paths, L, trailing_pad) if v1_files is None else v1_files
        info["pieces"] = v1_pieces(files, L, trailing_pad) if pieces is None else pieces
        if mutate:
            mutate(top)

    return v2_util.torrent_v2(files, L, name=name, paths=paths, mutate=add_v1)


def bits(n: int, clear=()) -> bytes:
    return v2_util.set_bits(n, clear)


# ---- shared by the sweep and the fuzz (tests/test_gpu_hybrid_sweep.py, tests/test_gpu_hybrid_fuzz.py) ----------------

def pack(oks) -> bytes:
    """MSB-first bitfield of a list of truth values; the spare bits of the last byte are 0."""
    bf = bytearray((len(oks) + 7) // 8)
    for i, ok in enumerate(oks):
        if ok:
            bf[i >> 3] |= 0x80 >> (i & 7)
    return bytes(bf)


def unpack(bf, n: int) -> list:
    """The first n bits of an MSB-first bitfield of exactly ceil(n / 8) bytes whose spare bits are 0."""
    assert len(bf) == (n + 7) // 8 and pack([(bf[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]) == bytes(bf)
    return [bool((bf[i >> 3] >> (7 - (i & 7))) & 1) for i in range(n)]


def xor_at(data, pos: int, mask: int) -> bytes:
    b = bytearray(data)
    b[pos] ^= mask
    return bytes(b)


class Layout:
    """Files under piece length L as a hybrid torrent lays them out: the piece table (tests/v2_ref.py), the v1 length
    with or without a pad after the last file, the rows that hold a pad range, both expected hash sets, and the number
    of launches of one hybrid call (pad if any row has a tail, SHA-1, v2 leaves, one per tree level, v2 finish)."""

    def __init__(self, files, L: int, trailing: bool = False):
        self.L, self.trailing = L, trailing
        self.files = [bytes(f) for f in files]
        self.lengths = [len(f) for f in self.files]
        self.table = v2_ref.piece_table(self.lengths, L)          # (file, offset, bytes, leaves) per piece
        self.P = len(self.table)
        self.pb = [r[2] for r in self.table]
        self.tl = [r[3] for r in self.table]
        self.offs, p = [], 0
        for n in self.lengths:
            self.offs.append(p * L)
            p += -(-n // L)
        self.total = self.P * L if trailing else (self.P - 1) * L + self.pb[-1]
        self.v1_len = [min(L, self.total - i * L) for i in range(self.P)]
        self.tails = [i for i in range(self.P) if self.pb[i] < self.v1_len[i]]
        self.linear = padded_linear(self.files, L, trailing)
        assert len(self.linear) == self.total
        self.pieces = v1_pieces(self.files, L, trailing)
        self.hashes = v2_expected(self.files, L)

    def launches(self, first: int = 0, count=None) -> int:
        count = self.P - first if count is None else count
        tail = any(first <= i < first + count for i in self.tails)
        return (1 if tail else 0) + 1 + 2 + max(self.tl[first:first + count]).bit_length() - 1

    def first_piece(self, k: int) -> int:
        return self.offs[k] // self.L

    def verdicts(self, staged, pieces=None, hashes=None):
        """(v1 ok, v2 ok) per piece of `staged` (one buffer per file, the files' lengths) against the v1 `pieces`
        string and the v2 hash list given (default: this layout's own), and both hash sets of the staged bytes."""
        pieces = self.pieces if pieces is None else pieces
        hashes = self.hashes if hashes is None else hashes
        got1, got2 = v1_pieces(staged, self.L, self.trailing), v2_expected(staged, self.L)
        assert len(got1) == 20 * self.P and len(got2) == self.P
        ok1 = [got1[20 * i:20 * i + 20] == pieces[20 * i:20 * i + 20] for i in range(self.P)]
        ok2 = [got2[i] == hashes[i] for i in range(self.P)]
        return ok1, ok2, got1, got2


def load(ctx, lay: Layout, first: int = 0, count=None, pieces=None, hashes=None, staged=None, fill=0xFF,
         relayout: bool = True) -> None:
    """Layout (the v1 space), piece table and digests (skipped with relayout=False: the context keeps its own); the
    whole shard staged as `fill`, then the bytes of `staged` (default: the files) that meet the shard."""
    L = lay.L
    count = lay.P - first if count is None else count
    if relayout:
        ctx.set_layout(lay.total, L, lay.P, first, count)
        ctx.v2_set_pieces(lay.pb, lay.tl, b"".join(lay.hashes if hashes is None else hashes))
        ctx.set_digests(lay.pieces if pieces is None else pieces)
    lo, hi = first * L, min((first + count) * L, lay.total)
    if fill is not None and hi > lo:
        ctx.stage(lo, bytes([fill]) * (hi - lo))
    ctx.stage_many([(off, data) for off, data in zip(lay.offs, lay.files if staged is None else staged)
                    if len(data) and off < hi and off + len(data) > lo])


def read_shard(ctx, lay: Layout, first: int = 0, count=None) -> bytes:
    """Every byte of the shard's rows inside the v1 space, read back from the device."""
    count = lay.P - first if count is None else count
    lo, hi = first * lay.L, min((first + count) * lay.L, lay.total)
    out = bytearray(hi - lo)
    ctx.read(lo, out)
    return bytes(out)


def first_difference(a: bytes, b: bytes):
    """None, or the first position where two equally long byte strings differ."""
    assert len(a) == len(b)
    if a == b:
        return None
    return next(i for i in range(len(a)) if a[i] != b[i])
