"""Designed batches for tv_batch_verify's mixed-length groups (tests/test_gpu_batch_groups.py runs them on every kernel
form; tests/test_batch_groups_shapes.py holds them to their promises on the CPU through batch_fuzz.ref_plan).

batch_plan sorts a batch's pieces by SHA-1 block count and packs what comes next into a group until nb_max - nfull_min
would exceed cut = max(8, nb_max / 8), so here, and nowhere else, the masked tail of the rounds wave and of the lane
form and the helper's padded-block region [fast_end, end] are up to cut blocks long.  The seeded draw of
batch_fuzz.py takes piece lengths far apart, which sort into groups of their own; these batches are built the other way:

ladder(span, nb_max, T)  one full group of one-piece torrents with every block count nb_max - T .. nb_max in it
staircase()              several hundred one-piece torrents in an arithmetic progression of lengths: nearly every group
                         is cut early, padded with origin -1 copies and has every lane different
crowd()                  more than 16,384 short pieces: the lane form by auto, more workgroups than CUs when forced
"""
from __future__ import annotations

import random

from tests.batch_fuzz import CUT_BLOCKS, CUT_SHARE, flip_byte, flip_digest, make, nblocks

REMAINDERS = (0, 1, 55, 56, 63)        # len % 64 by lane: paddings of one block (<= 55) and of two side by side
LADDER_TAILS_LONG = (0, 1, 2, 3, 16, 29, 30, 31)


def cut_of(nb_max: int) -> int:
    return max(CUT_BLOCKS, nb_max // CUT_SHARE)


def ladder_grid() -> list:
    """(nb_max, T) of every ladder: each tail the cut allows at small block counts, and at 257 / 258 blocks tails that
    take the K+W ring's indices past 30 into the masked region."""
    grid = [(nb, T) for nb in (2, 3, 9, 10, 41, 64) for T in range(min(cut_of(nb) - 1, nb - 1) + 1)]
    return grid + [(nb, T) for nb in (257, 258) for T in LADDER_TAILS_LONG]


def ladder_lens(span: int, nb_max: int, T: int) -> list:
    """Lane l has nb_max - l * (T + 1) // span blocks and len % 64 = REMAINDERS[l % 5].  Two exceptions: a piece of one
    block has 1 .. 55 bytes (never 0), and at T = cut - 1, the longest tail the plan ever hands a kernel, the shortest
    members pad inside their last data block (len % 64 <= 55: otherwise the plan closes the group one entry early)."""
    assert 0 <= T <= min(cut_of(nb_max) - 1, nb_max - 1) and T < span
    out = []
    for l in range(span):
        nb, r = nb_max - l * (T + 1) // span, REMAINDERS[l % 5]
        if nb == 1:
            r = {0: 2, 56: 54, 63: 7}.get(r, r)
        elif nb == nb_max - T and T == cut_of(nb_max) - 1:
            r = {56: 54, 63: 2}.get(r, r)
        out.append((nb - 1) * 64 + r if r <= 55 else (nb - 2) * 64 + r)
        assert out[-1] > 0 and nblocks(out[-1]) == nb and out[-1] % 64 == r
    return out


def ladder_geom(span: int, nb_max: int, T: int) -> tuple:
    """(fast_end, end, nb_min) the ladder is built for: its shortest members have nb_max - T blocks, and the raw blocks
    end one block below that, two where one of the shortest carries a two-block padding (a member a block longer that
    carries one ends its raw blocks where a shortest one with a one-block padding does)."""
    nb_min = nb_max - T
    two = any(n % 64 > 55 for n in ladder_lens(span, nb_max, T) if nblocks(n) == nb_min)
    return max(0, nb_min - (2 if two else 1)), nb_max, nb_min


def ladder(span: int, nb_max: int, T: int) -> list:
    """`span` one-piece torrents (L = total = len, n = 1) that the plan packs into exactly one full group with
    end == nb_max and end - nb_min == T, the extreme block counts at its first and last positions.  Corrupted: the last
    byte of the longest member (position 0) and of the shortest (the last position), a digest bit of the one in the
    middle."""
    rng = random.Random(f"ladder {span} {nb_max} {T}")
    ts = [make(n, n, rng) for n in ladder_lens(span, nb_max, T)]
    flip_byte(ts[0], 0, -1)
    flip_byte(ts[-1], 0, -1)
    flip_digest(ts[span // 2], 0)
    return ts


STAIR_STEP, STAIR_COUNT = 37, 600       # lengths 37, 74, .. 22,200: an odd step, no multiple of 64
STAIR_MAX_BYTES = 8 << 20
STAIR_MULTI = ((100, (100, 7 * 100 + 33)), (300, (1000, 5 * 1000 + 999)), (500, (4096, 3 * 4096 + 1)))


def staircase() -> list:
    """One-piece torrents of STAIR_STEP * i bytes, i = 1 .. STAIR_COUNT, in ascending order, with three multi-piece
    torrents (a short last piece each) put among them at STAIR_MULTI's positions; a seeded eighth of the pieces has a
    flipped first or last byte or a flipped digest bit."""
    rng = random.Random(600037)
    ts = [make(STAIR_STEP * i, STAIR_STEP * i, rng) for i in range(1, STAIR_COUNT + 1)]
    for at, (L, total) in STAIR_MULTI:
        ts.insert(at, make(L, total, rng))
    entries = [(k, i) for k, t in enumerate(ts) for i in range(t.n)]
    for q, (k, i) in enumerate(rng.sample(entries, len(entries) // 8)):
        if q % 3 == 2:
            flip_digest(ts[k], i, rng.randrange(160))
        else:
            flip_byte(ts[k], i, 0 if q % 3 else -1)
    return ts


def shuffled(ts: list, seed: int = 91) -> tuple:
    """-> (perm, [ts[p] for p in perm]): the same torrents in a seeded shuffled order."""
    perm = list(range(len(ts)))
    random.Random(seed).shuffle(perm)
    return perm, [ts[p] for p in perm]


def index_bits(n_entries: int) -> int:
    return max(1, (n_entries - 1).bit_length())


def index_bit_digests(ts: list, k: int) -> list:
    """Every torrent's digest string with a bit flipped (another one than flip_digest's default) in exactly the entries
    whose index in the batch's (torrent, piece) order has bit k set.  Any two entries differ in some bit k below
    index_bits(N), so over those k a result delivered to the wrong entry shows in at least one launch."""
    out, e = [], 0
    for t in ts:
        d = bytearray(t.digests)
        for i in range(t.n):
            if (e >> k) & 1:
                d[20 * i + 19] ^= 0x40
            e += 1
        out.append(bytes(d))
    return out


CROWD_TORRENTS, CROWD_PIECES, CROWD_MAX_L = 200, 82, 640
CROWD_MAX_BYTES = 12 << 20
CROWD_LONGER = tuple(641 + 53 * i for i in range(24))      # 11 .. 30 blocks


def crowd() -> list:
    """CROWD_TORRENTS torrents of CROWD_PIECES pieces, the piece length drawn per torrent from 2 .. 640 bytes (1 .. 11
    blocks; below 64 bytes no raw block at all), each with a short last piece; a seeded tenth of the pieces has a
    flipped byte or digest bit.  Pieces this close never close a group early, so in the middle of the batch stand 24
    one-piece torrents of CROWD_LONGER's lengths: the launch's first groups are cut early and padded, and the launch
    has another length under a span of 32 than under one of 64."""
    rng = random.Random(16400)
    ts = []
    for _ in range(CROWD_TORRENTS):
        L = rng.randrange(2, CROWD_MAX_L + 1)
        ts.append(make(L, (CROWD_PIECES - 1) * L + rng.randrange(1, L), rng))
    ts[CROWD_TORRENTS // 2:CROWD_TORRENTS // 2] = [make(n, n, rng) for n in CROWD_LONGER]
    entries = [(k, i) for k, t in enumerate(ts) for i in range(t.n)]
    for q, (k, i) in enumerate(rng.sample(entries, len(entries) // 10)):
        if q % 2:
            flip_digest(ts[k], i, rng.randrange(160))
        else:
            flip_byte(ts[k], i, rng.choice([0, -1]))
    return ts


def all_lens(ts: list) -> list:
    return [x for t in ts for x in t.lens()]
