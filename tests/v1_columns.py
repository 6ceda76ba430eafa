"""Shapes of the streamed SHA-1 column sweep (tests/test_gpu_v1_columns.py), and the stream geometry restated.

A streamed verify (tv_verify_host, tv_stream_*, tv_stream_file_table) launches one kernel per column of C bytes of every
piece: blocks [blk_begin, blk_end) with the chaining values carried in d_state between launches.  The shapes here put
the short last piece's end, its padding blocks and the columns past it at every place the kernels' group geometry
(tv_kernels.hip wave_geom / main_geom / resolve_group) tells apart, for column widths of 1 .. 8 and 13 blocks; classes()
names what a shape reaches, and tests/test_v1_columns_shapes.py holds the list to every class at every width on the
CPU, so the sweep cannot quietly go shallow.

stream_column (tv_stream.hip) and stream_geometry (tv_plan.h) are restated in Python: the GPU tests derive the launch
count they expect (tv_last_kernel) from them, and the CPU test compares stream_geometry with the library's own
(tests/c/plan_stream_main.cpp)."""
from __future__ import annotations

import hashlib
import random

LANE, SPLIT, TWIN = 1, 2, 4
# name -> (TV_OPT_KERNEL, TV_OPT_SPLIT_PAIRS, TV_OPT_LANE_PAIRS); lane pairs 2 = the 3-deep ring, 1 = the pair ring
VARIANTS = {
    "lane3": (LANE, 0, 2),
    "lanepairs": (LANE, 0, 1),
    "split1": (SPLIT, 1, 0),
    "split2": (SPLIT, 2, 0),
    "twin1": (TWIN, 0, 0),
    "twin2": (TWIN, 2, 0),
}
# column widths in 64-byte blocks: 1 .. 6 reach every exit of the helpers' six-block loop, 7 its back edge, 8 and 13 its
# second lap; 1 .. 8 every residue of the lane kernel's rings of 3 and 4 blocks; both parities for the twin rounds loop
CS = [1, 2, 3, 4, 5, 6, 7, 8, 13]
PS = (1, 33, 65, 130)      # the last group alone; + one twin workgroup; + one wave / split pair; + two pairs and a piece
CLASSES = ("pad_in_col", "spill", "exact", "dead", "dead2", "in_last_col", "one_block", "parity")

MiB = 1 << 20
SLOT = 64 * MiB            # one ring slot (kRingSlotBytes)
SLACK = 256                # bytes after a chunk buffer's last row (kSlack)
CHUNK_MAX = 256 * MiB      # tv_plan.h kStreamChunkMax
MIN_WIN = 2048             # pieces per window of tv_verify_host and a warm tv_stream_file_table


def nblocks(n: int) -> int:
    return (n + 8) // 64 + 1


def lengths(C: int) -> list:
    """Piece lengths for columns of C bytes: one to four columns, the final one of full width, of one partial block, or
    (c >= 2) of one raw block and two padded ones."""
    out = [C, 2 * C, 3 * C, 3 * C + 1, 3 * C + 55, 3 * C + 56, 3 * C + 63]
    if C >= 128:
        out.append(2 * C + 64 + 56)
    return out


def lasts(C: int, L: int) -> list:
    """Lengths of the last piece: the padding edges and the column edges below L, and L itself (no short piece)."""
    xs = {1, 55, 56, C - 9, C - 8, C, C + 1, 2 * C - 8, 2 * C, L - 64, L - 1}
    return sorted({x for x in xs if 1 <= x < L} | {L})


def shapes(c: int) -> list:
    """Every (L, last) of the sweep at columns of c blocks."""
    C = 64 * c
    return [(L, last) for L in lengths(C) for last in lasts(C, L)]


def classes(C: int, L: int, last: int) -> set:
    """What the SHORT last piece of a shape reaches in columns of C bytes (empty for last == L).  Column k hashes blocks
    [k c, (k + 1) c), the final column every block from its first on."""
    if last >= L:
        return set()
    c, ncol, nb = C // 64, -(-L // C), nblocks(last)

    def col(b):
        return min(b // c, ncol - 1)

    data_col = col((last - 1) // 64)                      # the column of the last block that holds data
    pad_cols = {col(b) for b in range(last // 64, nb)}    # the padded blocks: the 0x80 byte and the bit length
    dead = sum(1 for k in range(ncol) if k * c >= nb)     # columns that start at or after the piece's last block's end
    out = set()
    if pad_cols == {data_col}:
        out.add("pad_in_col")
    if max(pad_cols) > data_col:
        out.add("spill")
    if last % C == 0 and last // C <= ncol - 1:
        out.add("exact")
    if dead == 1:
        out.add("dead")
    if dead >= 2:
        out.add("dead2")
    if col(nb - 1) == ncol - 1:
        out.add("in_last_col")
    if last < 56 and ncol >= 2:
        out.add("one_block")
    if nb % 2 != nblocks(L) % 2:
        out.add("parity")
    return out


# ---- the library's geometry, restated ---------------------------------------------------------------------------------------

def stream_column(L: int, count: int, chunk: int) -> int:
    """tv_stream.hip stream_column: TV_OPT_STREAM_CHUNK, or the widest power of two from 64 KiB up to L whose column of
    every piece stays <= 512 MiB; a multiple of 64, at most the padded piece and one ring slot."""
    C = chunk
    if not C:
        C = 64 << 10
        while C * 2 <= L and C * 2 * count <= 512 * MiB:
            C *= 2
    C = min(C // 64 * 64, -(-L // 64) * 64)
    return max(64, min(C, SLOT))


def stream_geometry(L: int, count: int, budget: int, min_win: int = MIN_WIN, slot: int = SLOT,
                    slack: int = SLACK) -> tuple:
    """tv_plan.h stream_geometry: (column bytes, pieces per window) of a stream under a device budget."""
    half = min(budget // 2, CHUNK_MAX)
    lpad = min(-(-L // 64) * 64, slot)
    w = min(count, min_win)
    per = (half - slack) // w if half > slack and w else 0
    wid = per - 256 if per > 256 else 64
    C = max(64, min(wid // 4096 * 4096 if wid >= 4096 else wid // 64 * 64, lpad))
    if C == lpad and w < count and half > slack:
        w = min(count, max(w, (half - slack) // (C + 256) // 64 * 64))
    return C, w


def column_budget(C: int, win: int = MIN_WIN) -> int:
    """A TV_OPT_RESIDENT_BUDGET under which stream_geometry gives columns of C bytes (C < 4096) and windows of `win`."""
    return 2 * (win * (C + 256) + SLACK)


def host_units(L: int, count: int, chunk: int, budget: int) -> int:
    """Kernel launches of one tv_verify_host call (tv_last_kernel's count): columns across the shard with
    TV_OPT_STREAM_CHUNK, else windows x columns within the budget (1 GiB when none is set)."""
    if chunk:
        C, win = stream_column(L, count, chunk), count
    else:
        C, win = stream_geometry(L, count, budget or (1 << 30))
        win = min(win, count)
    return -(-count // win) * -(-L // C)


def workgroups(variant: str, n: int, short: bool) -> int:
    """The grid of one launch over n pieces, the last of them short (tv_kernels.hip tv_launch_verify): main groups of
    64 pieces per split pair, 32 per twin pair, four lane waves of 64 to a workgroup; the short last piece's group after
    them.  TV_COUNTER_LAST_WORKGROUPS reports it, which tells the 1- and 2-pair forms apart."""
    kernel, pairs, _ = VARIANTS[variant]
    n_main, extra = n - int(short), int(short)
    if kernel == SPLIT:
        return -(-n_main // (64 * (2 if pairs == 2 else 1))) + extra
    if kernel == TWIN:
        return -(-n_main // (32 * (2 if pairs == 2 else 1))) + extra
    return -(-(-(-n_main // 64) + extra) // 4)


# ---- payloads ---------------------------------------------------------------------------------------------------------------

def piece_len(L: int, P: int, last: int, i: int) -> int:
    return last if i == P - 1 else L


def digests(payload, L: int, P: int, last: int) -> bytes:
    return b"".join(hashlib.sha1(payload[i * L:i * L + piece_len(L, P, last, i)]).digest() for i in range(P))


def corrupted(P: int) -> list:
    """One piece of every 32, at a position that moves through the group, and always the last piece."""
    return sorted({g * 32 + (7 * g + 3) % 32 for g in range(-(-P // 32)) if g * 32 + (7 * g + 3) % 32 < P} | {P - 1})


class Case:
    """A torrent of P pieces of L bytes (the last of `last`): its bytes, the same with the LAST VALID BYTE of the pieces
    `bad` flipped, and the digests of both."""

    def __init__(self, L: int, last: int, P: int, bad=None, payload=None):
        self.L, self.last, self.P = L, last, P
        self.total = L * (P - 1) + last
        rng = random.Random((L * 1009 + last) * 1009 + P)
        self.payload = rng.randbytes(self.total) if payload is None else payload
        assert len(self.payload) == self.total
        self.bad = corrupted(P) if bad is None else sorted(set(bad))
        flipped = bytearray(self.payload)
        for i in self.bad:
            flipped[i * L + piece_len(L, P, last, i) - 1] ^= 1 << (i % 8)
        self.flipped = bytes(flipped)
        self.good = digests(self.payload, L, P, last)
        self.good_flipped = digests(self.flipped, L, P, last)
        assert all(self.good[20 * i:20 * i + 20] != self.good_flipped[20 * i:20 * i + 20] for i in self.bad)

    def bits(self, clear=()) -> list:
        return [0 if i in clear else 1 for i in range(self.P)]


def bits(bf, n: int) -> list:
    return [(bf[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def bitfield(bs) -> bytes:
    out = bytearray((len(bs) + 7) // 8)
    for i, b in enumerate(bs):
        if b:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)
