"""Seeded random hybrid torrents: the draw of tests/test_gpu_hybrid_fuzz.py, and the features a draw shows
(tests/test_hybrid_fuzz_draw.py holds the seed list to them on the CPU, so the fuzz cannot quietly go shallow).

draw(seed) gives what tests/v2_fuzz.py's draw gives (a piece length, files, their bytes, the same bytes with some
pieces corrupted -- always including the last file byte before a pad range --, files missing or truncated on disk) and:
whether a pad follows the last file (`trailing`), pieces whose v1 digest and pieces whose v2 hash the torrent states
wrongly, a split of the pieces into two or three shards (at multiples of 8 pieces, as tv_set_layout takes them), one
more shard that ends inside a byte of the bitfield, and for some seeds a forced SHA-1 kernel.  A draw's aligned size
stays near 8 MiB; the draws with more than 64 pieces use L <= 32 KiB.  Seeds 11 and 23 hold only files that are whole
pieces (and a short last piece): no row has a pad range, and the pad kernel is not launched."""
from __future__ import annotations

import random
from dataclasses import dataclass, field

from tests import hybrid_util as hu
from tests import v2_ref
from tests.v2_fuzz import LEAF, PIECE_LENGTHS, TAILS, Draw, _clamp

K = 1024
CHUNK = 64 * K                                             # kHybridChunk (torrent_amd/csrc/tv_plan.h)
SEEDS = list(range(24))
FEATURES = ("multi_chunk_tail", "tail_starts_unaligned", "tail_starts_aligned", "no_tail", "trailing", "short_last",
            "zero_file", "count_mod8", "multiword", "L16K", "L_ge_256K", "v1_only_mismatch", "v2_only_mismatch",
            "missing", "cut_inside_piece", "forced_lane", "forced_split")
KERNEL_AUTO, KERNEL_LANE, KERNEL_SPLIT = 0, 1, 2


@dataclass
class HybridDraw(Draw):
    trailing: bool = False                                 # a pad file follows the last file
    v1_flips: dict = field(default_factory=dict)           # {piece: (byte of its digest, xor mask)}
    v2_flips: dict = field(default_factory=dict)           # {piece: (byte of its hash, xor mask)}
    shards: list = field(default_factory=list)             # [(first, count)], in order, covering every piece
    odd: tuple = (0, 1)                                    # one more shard: count % 8 != 0, without the last piece
    kernel: int = KERNEL_AUTO                              # TV_OPT_KERNEL of the ABI route
    lane_pairs: int = 0                                    # TV_OPT_LANE_PAIRS of the ABI route

    def layout(self) -> hu.Layout:
        return hu.Layout(self.files, self.L, self.trailing)

    def stated(self, lay: hu.Layout) -> tuple:
        """The v1 `pieces` string and the v2 hash list as the torrent states them (the flips applied)."""
        pieces, hashes = lay.pieces, list(lay.hashes)
        for i, (q, mask) in self.v1_flips.items():
            pieces = hu.xor_at(pieces, 20 * i + q, mask)
        for i, (q, mask) in self.v2_flips.items():
            hashes[i] = hu.xor_at(hashes[i], q, mask)
        return pieces, hashes

    def readable(self) -> list:
        """Per piece: the disk (missing and truncated files) supplies all of its bytes."""
        return [f not in self.missing and self.short.get(f, self.lengths[f]) >= o + b for f, o, b, w in self.table]


def _tails(d: HybridDraw, first: int = 0, count=None) -> list:
    """(row begin, row end) of every pad range of pieces [first, first + count)."""
    table = d.table
    P = len(table)
    count = P - first if count is None else count
    total = P * d.L if d.trailing else (P - 1) * d.L + table[-1][2]
    out = []
    for i in range(first, first + count):
        end = min(d.L, total - i * d.L)
        if table[i][2] < end:
            out.append((table[i][2], end))
    return out


def draw(seed: int) -> HybridDraw:
    rng = random.Random(71000 + seed)
    L = PIECE_LENGTHS[seed % len(PIECE_LENGTHS)]
    whole_only = seed % 12 == 11
    many = L <= 32 * K and seed % 4 < 2                    # more than 64 pieces (L <= 32 KiB only)
    if many:
        cap, n_files = rng.randrange(70, min(300, (8 << 20) // L)), 400
    else:
        cap, n_files = max(10, min(24, (8 << 20) // L)), rng.choice([3, 5, 17, 40])
    W = L // LEAF
    floor = 66 if many else 17 if L <= 256 * K else 9      # enough pieces for two shards and one that ends inside a byte
    lengths, pieces = [], 0
    while (len(lengths) < n_files or pieces < floor) and pieces < cap:
        room = cap - pieces
        kind = rng.random()
        if kind < 0.10:
            n = 0
        elif whole_only:
            n = rng.randrange(1, 3) * L
        elif kind < 0.25:
            n = rng.randrange(1, 200)
        elif kind < 0.38:                                  # a whole number of leaves, at most one piece
            n = rng.randrange(1, W + 1) * LEAF
        elif kind < 0.48:                                  # whole pieces
            n = rng.randrange(1, 4) * L
        elif kind < 0.66:                                  # the padding edges after 0 .. 3 whole pieces
            n = rng.randrange(0, 4) * L + rng.choice(TAILS)
        elif kind < 0.80:                                  # a pad range that begins beside a 64 KiB chunk boundary
            b = rng.randrange(1, L)
            if L > CHUNK:
                b = L - rng.randrange(1, L // CHUNK) * CHUNK + rng.choice((-17, -1, 0, 1, 16))
            n = rng.randrange(0, 2) * L + b
        else:
            n = rng.randrange(1, 4 * L)
        n = _clamp(n, L, room)
        lengths.append(n)
        pieces += -(-n // L)
    k = max(k for k, n in enumerate(lengths) if n)
    if whole_only:                                         # a short last piece, and no pad after it
        lengths[k] += 1 + rng.randrange(L - 1)
    elif all(n % L == 0 for n in lengths):
        lengths[k] -= 1
    files = [rng.randbytes(n) for n in lengths]
    table = v2_ref.piece_table(lengths, L)
    P = len(table)
    d = HybridDraw(seed, L, lengths, files, [], {})
    d.trailing = not whole_only and rng.random() < 0.5
    # corrupted bytes: some pieces anywhere, and the last file byte before a pad range (or of a short last piece)
    for i in rng.sample(range(P), max(1, P // 8)):
        d.corrupt[(i, rng.randrange(table[i][2]))] = 1 << rng.randrange(8)
    i = rng.choice([i for i, r in enumerate(table) if r[2] < L])
    d.corrupt[(i, table[i][2] - 1)] = 1 << rng.randrange(8)
    staged = [bytearray(f) for f in files]
    for (i, pos), mask in d.corrupt.items():
        f, o, b, w = table[i]
        staged[f][o + pos] ^= mask
    d.staged = [bytes(s) for s in staged]
    # hashes the torrent states wrongly: the two sets are disjoint, and some of each lie on an uncorrupted piece
    n_flip = max(1, P // 10)
    clean = [i for i in range(P) if i not in {i for i, _ in d.corrupt}]
    picks = rng.sample(clean, min(len(clean), 2))
    rest = [i for i in range(P) if i not in picks]
    picks += rng.sample(rest, min(len(rest), 2 * (n_flip - 1)))
    for n, i in enumerate(picks):
        if n % 2 == 0:
            d.v1_flips[i] = (rng.randrange(20), 1 << rng.randrange(8))
        else:
            d.v2_flips[i] = (rng.randrange(32), 1 << rng.randrange(8))
    # two or three shards: a shard starts a byte of the bitfield (tv_set_layout's contract), so the cuts are arbitrary
    # multiples of 8; and one more shard that ends inside a byte and before the last piece
    eights = list(range(8, P, 8))
    cuts = sorted(rng.sample(eights, min(len(eights), rng.choice([1, 2]))))
    if many:                                               # the first shard has more than one word of output
        c = rng.choice([e for e in eights if e > 64])
        cuts = [c] + ([rng.choice([e for e in eights if e > c])] if eights[-1] > c and rng.random() < 0.5 else [])
    first = rng.choice([0] + eights[:-1])
    count = rng.randrange(1, P - first)
    d.odd = (first, count - 1 if count % 8 == 0 else count)
    edges = [0] + cuts + [P]
    d.shards = [(a, b - a) for a, b in zip(edges, edges[1:])]
    if seed % 4 == 1:
        d.kernel, d.lane_pairs = KERNEL_LANE, 1 + (seed // 4) % 2
    elif seed % 4 == 3:
        d.kernel = KERNEL_SPLIT
    for k, n in enumerate(lengths):
        r = rng.random()
        if r < 0.08:
            d.missing.add(k)
        elif r < 0.20 and n:
            d.short[k] = rng.randrange(n)
    return d


def features(d: HybridDraw) -> set:
    L = d.L
    table = d.table
    P = len(table)
    bad = {i for i, _ in d.corrupt}
    out = set()
    tails = _tails(d)
    if any(-(-(e - b // 16 * 16) // CHUNK) > 1 for b, e in tails):
        out.add("multi_chunk_tail")
    if any(b % 16 for b, e in tails):
        out.add("tail_starts_unaligned")
    if any(b % 16 == 0 for b, e in tails):
        out.add("tail_starts_aligned")
    if any(not _tails(d, first, count) for first, count in d.shards):
        out.add("no_tail")                                 # a shard whose call launches no pad kernel
    if table[-1][2] < L:
        out.add("trailing" if d.trailing else "short_last")
    if 0 in d.lengths:
        out.add("zero_file")
    if any(count % 8 for first, count in d.shards + [d.odd]):
        out.add("count_mod8")
    if any(count > 64 for first, count in d.shards):
        out.add("multiword")
    if L == 16 * K:
        out.add("L16K")
    if L >= 256 * K:
        out.add("L_ge_256K")
    if any(i not in bad and i not in d.v2_flips for i in d.v1_flips):
        out.add("v1_only_mismatch")
    if any(i not in bad and i not in d.v1_flips for i in d.v2_flips):
        out.add("v2_only_mismatch")
    if any(d.lengths[k] for k in d.missing):
        out.add("missing")
    if any(keep % L for keep in d.short.values()):
        out.add("cut_inside_piece")
    if d.kernel == KERNEL_LANE:
        out.add("forced_lane")
    if d.kernel == KERNEL_SPLIT:
        out.add("forced_split")
    return out


def torrent(d: HybridDraw, lay: hu.Layout, paths) -> bytes:
    """The hybrid .torrent of the draw with its wrongly stated hashes: a v1 `pieces` string with the flipped digests; a
    flipped v2 hash in the `pieces root` of a one-piece file, or in the piece layer of a longer one under the pieces
    root of that layer (so the layer still is the one its root commits to)."""
    pieces, hashes = d.stated(lay)

    def wrong_v2(top):
        tree, layers = top["info"]["file tree"], top["piece layers"]
        for k, n in enumerate(d.lengths):
            p0, cnt = lay.first_piece(k), -(-n // d.L)
            if not any(p0 <= i < p0 + cnt for i in d.v2_flips):
                continue
            node = tree
            for c in paths[k]:
                node = node[c]
            old = node[""]["pieces root"]
            row = hashes[p0:p0 + cnt]
            if cnt == 1:
                node[""]["pieces root"] = row[0]
                continue
            root = v2_ref.reduce_row(row + [v2_ref.zero_piece_root(d.L)] * (v2_ref.next_pow2(cnt) - cnt))
            del layers[old]
            layers[root] = b"".join(row)
            node[""]["pieces root"] = root

    return hu.torrent_hybrid(d.files, d.L, name="fz", paths=paths, trailing_pad=d.trailing, pieces=pieces,
                             mutate=wrong_v2)
