"""Seeded random BitTorrent v2 layouts: the draw of tests/test_gpu_v2_fuzz.py, and the features a layout shows
(tests/test_v2_fuzz_draw.py holds the seed list to them on the CPU, so the fuzz cannot quietly go shallow).

draw(seed) gives a piece length, 1 .. 40 files (zero-length, tiny, whole leaves, whole pieces, piece multiples plus the
SHA-256 padding edges, uniform), their bytes, the same bytes with some pieces corrupted (always including the last
valid byte of a short leaf), and the on-disk state: some files missing, some truncated.  A layout's aligned size stays
near 8 MiB, except the seeds with seed % 8 == 7, which are built to hold >= 64 pieces of >= 4 leaves (the smallest
layout on which the piece-major lane mapping runs)."""
from __future__ import annotations

import random
from dataclasses import dataclass, field

from tests import v2_ref

K = 1024
LEAF = v2_ref.LEAF
PIECE_LENGTHS = [16 * K, 32 * K, 64 * K, 128 * K, 256 * K, 1024 * K]
TAILS = (1, 55, 56, 64, 16383, 16384, 16385)
SEEDS = list(range(24))
FEATURES = ("zero_file", "narrow_one_piece", "short_last_full_width", "whole_leaves_short_piece", "tail_1_55",
            "tail_56_63", "W1", "W64", "piece_major", "missing", "cut_inside_piece")


@dataclass
class Draw:
    seed: int
    L: int
    lengths: list                      # declared length of every file, file-tree order
    files: list                        # the files' bytes as the torrent describes them
    staged: list                       # the same with the corrupted positions flipped
    corrupt: dict                      # {(piece, position in the piece): xor mask}
    missing: set = field(default_factory=set)      # files absent on disk
    short: dict = field(default_factory=dict)      # {file: bytes kept on disk}

    @property
    def table(self) -> list:
        return v2_ref.piece_table(self.lengths, self.L)

    def disk(self) -> list:
        """One buffer per file as the disk holds it: None for a missing file, a short buffer for a truncated one."""
        return [None if k in self.missing else s[:self.short.get(k, len(s))] for k, s in enumerate(self.staged)]

    def expected(self) -> list:
        """The expected hash of every piece (of the uncorrupted files)."""
        out = []
        for f in self.files:
            out += v2_ref.file_hashes(f, self.L)[2]
        return out

    def staged_roots(self) -> list:
        """The root of every piece of the corrupted bytes."""
        out = []
        for f in self.staged:
            out += v2_ref.file_hashes(f, self.L)[2]
        return out

    def file_offsets(self) -> list:
        """Aligned linear offset of every file (a zero-length file: where the next one starts)."""
        offs, p = [], 0
        for n in self.lengths:
            offs.append(p * self.L)
            p += -(-n // self.L)
        return offs


def _clamp(n: int, L: int, room: int) -> int:
    while -(-n // L) > room:
        n -= L
    return n


def draw(seed: int) -> Draw:
    rng = random.Random(52000 + seed)
    big = seed % 8 == 7
    if big:                                                # >= 64 pieces of >= 4 leaves
        L = rng.choice([64 * K, 128 * K])
        cap, n_files = rng.randrange(66, 81), 39
    else:
        L = PIECE_LENGTHS[seed % len(PIECE_LENGTHS)]
        cap, n_files = max(4, min(24, (8 << 20) // L)), rng.choice([1, 2, 5, 17, 40])
    W = L // LEAF
    lengths, pieces = [], 0
    while len(lengths) < n_files and pieces < cap:
        room = cap - pieces
        kind = rng.random()
        if kind < 0.12:
            n = 0
        elif kind < 0.27:
            n = rng.randrange(1, 200)
        elif kind < 0.42:                                  # a whole number of leaves, at most one piece
            n = rng.randrange(1, W + 1) * LEAF
        elif kind < 0.55:                                  # whole pieces
            n = rng.randrange(1, 4) * L
        elif kind < 0.80:                                  # the padding edges after 0 .. 3 whole pieces
            n = rng.randrange(0, 4) * L + rng.choice(TAILS)
        else:
            n = rng.randrange(1, 4 * L)
        n = _clamp(n, L, room)
        lengths.append(n)
        pieces += -(-n // L)
    if big and pieces < 64:                                # one long file with a short last piece makes up the rest
        lengths.append((64 - pieces) * L + rng.choice(TAILS))
    if sum(lengths) == 0:
        lengths.append(_clamp(L + 3, L, cap))
    if all(b % LEAF == 0 for _, _, b, _ in v2_ref.piece_table(lengths, L)):
        k = max(k for k, n in enumerate(lengths) if n)     # no short leaf anywhere: the last file loses a byte
        lengths[k] -= 1
    files = [rng.randbytes(n) for n in lengths]
    table = v2_ref.piece_table(lengths, L)
    P = len(table)
    corrupt = {}
    for i in rng.sample(range(P), max(1, P // 8)):
        corrupt[(i, rng.randrange(table[i][2]))] = 1 << rng.randrange(8)
    i = rng.choice([i for i, r in enumerate(table) if r[2] % LEAF])
    corrupt[(i, table[i][2] - 1)] = 1 << rng.randrange(8)  # the last valid byte of a short leaf
    staged = [bytearray(f) for f in files]
    for (i, pos), mask in corrupt.items():
        f, o, b, w = table[i]
        staged[f][o + pos] ^= mask
    d = Draw(seed, L, lengths, files, [bytes(s) for s in staged], corrupt)
    for k, n in enumerate(lengths):
        r = rng.random()
        if r < 0.08:
            d.missing.add(k)
        elif r < 0.20 and n:
            d.short[k] = rng.randrange(n)
    return d


def features(d: Draw) -> set:
    L, W = d.L, d.L // LEAF
    table = d.table
    out = set()
    if 0 in d.lengths:
        out.add("zero_file")
    if any(0 < n <= L and v2_ref.next_pow2(-(-n // LEAF)) < W for n in d.lengths):
        out.add("narrow_one_piece")
    if any(n > L and n % L for n in d.lengths):
        out.add("short_last_full_width")
    if any(b < L and b % LEAF == 0 for _, _, b, _ in table):
        out.add("whole_leaves_short_piece")
    last_leaf = [b - (-(-b // LEAF) - 1) * LEAF for _, _, b, _ in table]
    if any(1 <= n % 64 <= 55 for n in last_leaf):
        out.add("tail_1_55")
    if any(56 <= n % 64 <= 63 for n in last_leaf):
        out.add("tail_56_63")
    if W == 1:
        out.add("W1")
    if W == 64:
        out.add("W64")
    if len(table) >= 64 and W >= 4:
        out.add("piece_major")
    if any(d.lengths[k] for k in d.missing):
        out.add("missing")
    if any(keep % L for keep in d.short.values()):
        out.add("cut_inside_piece")
    return out
