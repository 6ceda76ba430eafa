"""Seeded random BitTorrent v1 cases across the SHA-1 kernel forms and the paths that launch them: the draw of
tests/test_gpu_v1_kernel_fuzz.py, and the features a draw shows (tests/test_v1_kernel_fuzz_draw.py holds the seed list
to them on the CPU, so the fuzz cannot quietly go shallow).

draw(seed) gives a piece length, a piece count and a last piece's length (half the time from the padding and column
edges of tests/v1_columns.py), one kernel form of VARIANTS or the library's own choice, a route, a shard, an
availability mask, the payload with some bytes flipped and the digest string with some digests flipped and sometimes cut
ragged.  The route and the kernel form go round the seeds so that every pair of them that matters comes up; everything
else is drawn.

Expected (tests/test_gpu_fuzz.py _expected's rule on a linear payload): bit i = piece i available, its 20-byte slice of
the digest string complete, and hashlib.sha1 of its staged bytes equal to that slice."""
from __future__ import annotations

import hashlib
import random
from dataclasses import dataclass

from tests import v1_columns as vc

SEEDS = list(range(32))
ROUTES = ("resident", "windowed", "columns", "win_columns", "list", "list_slots")
KERNELS = tuple(vc.VARIANTS) + ("auto",)
PIECE_LENGTHS = (64, 100, 448, 1000, 4096, 16384 + 7, 65536)
MAX_BYTES = 4 << 20
WINDOW = 3                 # pieces per window of the windowed route
FEATURES = tuple("route_" + r for r in ROUTES) + tuple("kernel_" + k for k in KERNELS) + (
    "short_last", "spill", "exact", "dead", "n_main_zero_window", "odd_L", "multiword", "ragged", "masked", "shard")


@dataclass
class Draw:
    seed: int
    L: int
    P: int
    last: int
    kernel: str            # a name of tests/v1_columns.py VARIANTS, or "auto"
    route: str
    c: int                 # blocks per column (the streamed routes)
    first: int             # the shard: pieces [first, first + count)
    count: int
    avail: bytes | None    # the shard's availability bits, or None
    payload: bytes         # the torrent's bytes as its digests describe them
    staged: bytes          # the same with some bytes flipped
    digests: bytes         # 20 bytes per piece, some flipped; ragged: the last slice cut short
    order: list            # the list routes: global pieces in call order, with duplicates
    slots: int             # list_slots: the pool's size

    @property
    def total(self) -> int:
        return self.L * (self.P - 1) + self.last

    def piece(self, i: int, data=None) -> bytes:
        data = self.staged if data is None else data
        return data[i * self.L:i * self.L + (self.last if i == self.P - 1 else self.L)]

    def shard_bytes(self) -> bytes:
        return self.staged[self.first * self.L:min(self.total, (self.first + self.count) * self.L)]

    def matches(self, i: int) -> int:
        """Piece i's digest slice is complete and equals hashlib's digest of the staged bytes."""
        d = self.digests[20 * i:20 * i + 20]
        return int(len(d) == 20 and hashlib.sha1(self.piece(i)).digest() == d)

    def available(self, i: int) -> int:
        j = i - self.first
        return 1 if self.avail is None else (self.avail[j >> 3] >> (7 - (j & 7))) & 1

    def expected(self) -> list:
        """The shard's have-bits."""
        return [self.matches(i) & self.available(i) for i in range(self.first, self.first + self.count)]

    def staged_digests(self) -> bytes:
        """tv_hash's answer for the shard: the digests of the staged bytes."""
        return b"".join(hashlib.sha1(self.piece(i)).digest() for i in range(self.first, self.first + self.count))

    def stride(self) -> int:
        return -(-self.L // 64) * 64 + 256

    def window_budget(self, bufs: int) -> int:
        """The windowed route's TV_OPT_RESIDENT_BUDGET: `bufs` window buffers of WINDOW pieces."""
        return bufs * (WINDOW * self.stride() + 256)

    def windowed(self, bufs: int) -> bool:
        """tv_plan.h plan_payload: the shard does not fit that budget, so it is hashed in windows of WINDOW pieces."""
        return self.count * self.stride() + 256 > self.window_budget(bufs)


def _edges(C: int, L: int) -> list:
    return [x for x in (1, 55, 56, C - 9, C - 8, C, C + 1, 2 * C - 8, 2 * C, L - 64, L - 9, L - 8, L - 1) if 1 <= x < L]


def draw(seed: int) -> Draw:
    rng = random.Random(61000 + seed)
    route = ROUTES[seed % len(ROUTES)]
    kernel = KERNELS[(seed // len(ROUTES) + 3 * (seed % len(ROUTES))) % len(KERNELS)]   # (six kernels per route)
    streamed = route in ("columns", "win_columns")
    if route == "win_columns":                             # two windows of 2,048 pieces: small pieces, narrow columns
        L = rng.choice([100, 448, 448])
        P = rng.randrange(2049, 2200)
    else:
        L = rng.choice(PIECE_LENGTHS)
        P = rng.randrange(1, min(600, MAX_BYTES // L) + 1)
    c = rng.randrange(1, 14)
    if streamed and L > 64:                                # two columns or more
        c = rng.randrange(1, min(13, -(-L // 64) - 1) + 1)
    C = 64 * c
    ncol = -(-L // C)
    if streamed and ncol >= 2 and rng.random() < 0.75:
        # the streamed routes go round the column edges: the padding block in the next column, a last piece that ends
        # with a column, columns wholly past it
        k = rng.randrange(1, ncol)
        last = (k * C - 8, k * C, rng.choice([1, 55, 56]))[seed // len(ROUTES) % 3]
    elif rng.random() < 0.5 and _edges(C, L):
        last = rng.choice(_edges(C, L))
    else:
        last = rng.randrange(1, L + 1)
    # the shard: whole bytes of the bitfield before it; the streamed-window seeds keep more than one window
    first = 0
    if route == "win_columns":
        first = 8 * rng.randrange(0, (P - 2049) // 8 + 1)
    elif P > 8 and rng.random() < 0.5:
        first = 8 * rng.randrange(0, (P - 1) // 8 + 1)
    count = P - first
    if not streamed and count > 1 and rng.random() < 0.3:
        count = rng.randrange(1, count + 1)
    # a final window that holds only the short last piece: 3 k + 1 pieces in windows of 3, 2,049 in windows of 2,048
    if route == "windowed" and seed % 8 == 1:
        first, P = 0, WINDOW * rng.randrange(4, min(40, MAX_BYTES // L // WINDOW)) + 1
        count, last = P, rng.randrange(1, L)
    if route == "win_columns" and seed % 12 == 3:
        P = first + 2049
        count, last = 2049, last if last < L else rng.choice(_edges(C, L))
    total = L * (P - 1) + last
    assert total <= MAX_BYTES
    payload = rng.randbytes(total)
    digests = bytearray(vc.digests(payload, L, P, last))
    staged = bytearray(payload)
    for i in rng.sample(range(P), max(1, P // 10)):        # flipped bytes, the last piece's last byte among them
        n = last if i == P - 1 else L
        staged[i * L + rng.randrange(n)] ^= 1 << rng.randrange(8)
    if rng.random() < 0.5:
        staged[total - 1] ^= 0x80
    for i in rng.sample(range(P), P // 12):                # flipped digests
        digests[20 * i + rng.randrange(20)] ^= 1 << rng.randrange(8)
    if rng.random() < 0.2:                                 # ragged: the last slice is short, never equal
        digests = digests[:len(digests) - rng.randrange(1, 20)]
    avail = None
    if rng.random() < 0.6:
        avail = vc.bitfield([rng.random() < 0.85 for _ in range(count)])
    order, slots = [], 0
    if route in ("list", "list_slots"):
        order = list(range(first, first + count))
        rng.shuffle(order)
        order += rng.sample(order, min(len(order), 1 + len(order) // 5))      # duplicates
        slots = rng.randrange(1, 9)
    return Draw(seed, L, P, last, kernel, route, c, first, count, avail, payload, bytes(staged), bytes(digests), order,
                slots)


def features(d: Draw) -> set:
    out = {"route_" + d.route, "kernel_" + d.kernel}
    has_last = d.first + d.count == d.P
    short = has_last and d.last < d.L
    if short:
        out.add("short_last")
    if d.route in ("columns", "win_columns") and short:
        got = vc.classes(vc.stream_column(d.L, d.count, 64 * d.c), d.L, d.last)
        out |= got & {"spill", "exact"}
        if got & {"dead", "dead2"}:
            out.add("dead")
    # the pieces of the launches that hold the last piece: the shard, a window of WINDOW pieces, one of 2,048
    group = {"windowed": WINDOW if d.windowed(3) else d.count, "win_columns": vc.MIN_WIN}.get(d.route, d.count)
    if short and d.route not in ("list", "list_slots") and (d.count - 1) % group == 0:
        out.add("n_main_zero_window")
    if d.L % 64:
        out.add("odd_L")
    if d.count > 64:
        out.add("multiword")
    if len(d.digests) % 20:
        out.add("ragged")
    if d.avail is not None and any(not d.available(i) for i in range(d.first, d.first + d.count)):
        out.add("masked")
    if d.count < d.P:
        out.add("shard")
    return out
