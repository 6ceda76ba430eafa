"""What the batch tests share: the plan of a batch launch restated in plain Python (ref_plan: tv_plan.h batch_plan's
rules), a torrent as the batch tests build it (Torrent: its bytes, the bytes staged, its digest string, the have-bits
hashlib expects) and the seeded draw of tests/test_gpu_batch_fuzz.py (tests/test_batch_fuzz_draw.py holds it to its
promises on the CPU).

Expected bits (tv_verify's rule): piece i is 1 iff it is available, its 20-byte slice of the digest string is complete,
its bytes lie inside the torrent (i * L + len_i <= total, len_i per piece.ts:16-19 with the digest count as the piece
count) and hashlib.sha1 of the staged bytes equals the slice."""
from __future__ import annotations

import hashlib
import random
from dataclasses import dataclass, field
from typing import Optional

CUT_BLOCKS, CUT_SHARE = 8, 8          # tv_plan.h kBatchCutBlocks, kBatchCutShare
SPANS = {"twin": 32, "split": 64, "lane": 64}
KERNEL_IDS = {"auto": 0, "lane": 1, "split": 2, "twin": 4}


def nblocks(length: int) -> int:
    return (length + 8) // 64 + 1


def ref_plan(lens, span: int):
    """-> (launch, origin, groups): the entries in launch order (padding: a copy of the group's last entry, origin
    -1), and (fast_end, end, nb_min) per group of `span` launch positions."""
    order = sorted(range(len(lens)), key=lambda k: -nblocks(lens[k]))       # (stable)
    launch, origin, groups = [], [], []
    i = 0
    while i < len(order):
        nb_max = nblocks(lens[order[i]])
        cut = max(CUT_BLOCKS, nb_max // CUT_SHARE)
        members = []
        while len(members) < span and i < len(order):
            cand = members + [order[i]]
            if nb_max - min(lens[k] // 64 for k in cand) > cut:
                break
            members = cand
            i += 1
        pad = span - len(members) if i < len(order) else 0
        launch += members + [members[-1]] * pad
        origin += members + [-1] * pad
        groups.append((min(lens[k] // 64 for k in members), nb_max, min(nblocks(lens[k]) for k in members)))
    return launch, origin, groups


def auto_kernel(n: int, cus: int = 256) -> str:
    return "twin" if n <= 64 * cus else ("split" if n <= 16384 else "lane")


def bitfield(bits) -> bytes:
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


@dataclass
class Torrent:
    L: int
    n: int                 # digests (the piece count of the layout); may exceed ceil(total / L)
    total: int
    payload: bytes         # the torrent's bytes as its digests describe them
    staged: bytes = b""    # the same with some bytes flipped
    digests: bytes = b""   # 20 bytes per piece, some flipped; ragged: the last slice cut short
    avail: Optional[list] = None
    flipped: set = field(default_factory=set)   # pieces with a flipped byte or digest

    def piece_len(self, i: int) -> int:
        return self.total % self.L if i == self.n - 1 and self.total % self.L else self.L

    def lens(self) -> list:
        return [self.piece_len(i) for i in range(self.n)]

    def expected(self, avail=None) -> list:
        avail = self.avail if avail is None else avail
        out = []
        for i in range(self.n):
            n, d = self.piece_len(i), self.digests[20 * i:20 * i + 20]
            ok = len(d) == 20 and i * self.L + n <= self.total
            ok = ok and hashlib.sha1(self.staged[i * self.L:i * self.L + n]).digest() == d
            out.append(int(bool(ok and (avail is None or avail[i]))))
        return out


def make(L: int, total: int, rng: random.Random, n: Optional[int] = None) -> Torrent:
    """A clean torrent of `total` random bytes: n digests (default ceil(total / L)), the surplus ones zero."""
    whole = -(-total // L)
    n = whole if n is None else n
    payload = rng.randbytes(total)
    t = Torrent(L, n, total, payload)
    d = bytearray()
    for i in range(n):
        ln = t.piece_len(i)
        d += hashlib.sha1(payload[i * L:i * L + ln]).digest() if i * L + ln <= total else bytes(20)
    t.staged, t.digests = payload, bytes(d)
    return t


def flip_byte(t: Torrent, i: int, at: int) -> None:
    """Flip a bit of byte `at` (negative: from its end) of piece i's staged bytes."""
    s = bytearray(t.staged)
    s[i * t.L + (at if at >= 0 else t.piece_len(i) + at)] ^= 0x10
    t.staged = bytes(s)
    t.flipped.add(i)


def flip_digest(t: Torrent, i: int, bit: int = 3) -> None:
    d = bytearray(t.digests)
    d[20 * i + bit // 8] ^= 1 << (bit % 8)
    t.digests = bytes(d)
    t.flipped.add(i)


def avail_bytes(ts) -> Optional[bytes]:
    """The batch's availability bitfields back to back (None when no torrent has a mask)."""
    if all(t.avail is None for t in ts):
        return None
    return b"".join(bitfield(t.avail if t.avail is not None else [1] * t.n) for t in ts)


def run_batch(ctx, ts, kernel: str = "auto", stage=None) -> list:
    """Set the batch of torrents `ts` on `ctx`, give every torrent its digests and staged bytes (stage(ctx, k, t)
    instead, when given) and verify: the have-bits of every torrent as lists."""
    ctx.set_option(1, KERNEL_IDS[kernel])                   # TV_OPT_KERNEL
    ctx.set_batch_layout([t.total for t in ts], [t.L for t in ts], [t.n for t in ts])
    for k, t in enumerate(ts):
        ctx.batch_select(k)
        ctx.set_digests(t.digests)
        if stage is not None:
            stage(ctx, k, t)
        elif t.staged:
            ctx.stage(0, t.staged)
    return [bits_list(b, t.n) for b, t in zip(ctx.batch_verify(avail_bytes(ts)), ts)]


def bits_list(field_, n: int) -> list:
    assert len(field_) == (n + 7) // 8
    assert n % 8 == 0 or field_[-1] & (0xFF >> (n % 8)) == 0             # the spare bits are 0
    return [(field_[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def run_alone(ctx, t: Torrent, kernel: str = "auto") -> list:
    """The same torrent alone through tv_set_layout + tv_verify."""
    ctx.set_option(1, KERNEL_IDS[kernel])
    ctx.set_layout(t.total, t.L, t.n)
    ctx.set_digests(t.digests)
    if t.staged:
        ctx.stage(0, t.staged)
    return bits_list(ctx.verify(bitfield(t.avail) if t.avail is not None else None), t.n)


# ---- the seeded draw of tests/test_gpu_batch_fuzz.py ---------------------------------------------------------------------

SEEDS = list(range(24))
PIECE_LENGTHS = (64, 100, 4096, 16384, 16400, 65536)
MAX_BYTES = 8 << 20
MAX_TORRENTS, MAX_PIECES = 40, 90


def draw(seed: int) -> list:
    """1 .. 40 torrents of 0 .. 90 pieces each, at most 8 MiB in all, with flipped bytes and digests, ragged digest
    strings, surplus digests and availability masks."""
    rng = random.Random(73000 + seed)
    out, left = [], MAX_BYTES
    small = seed % 4 == 3                                    # every fourth draw: a batch shorter than one group
    for _ in range(rng.randrange(1, (3 if small else MAX_TORRENTS) + 1)):
        L = rng.choice(PIECE_LENGTHS)
        pieces = min(rng.randrange(0, (9 if small else MAX_PIECES) + 1), left // L)
        if pieces == 0:
            t = make(L, 0, rng, 0)
        else:
            last = rng.choice([1, 55, 56, 63, 64, L - 9, L - 8, L - 1, L, rng.randrange(1, L + 1)])
            last = max(1, min(L, last))
            total = (pieces - 1) * L + last
            t = make(L, total, rng, pieces + (rng.randrange(1, 4) if rng.random() < 0.1 else 0))
        left -= t.total
        whole = -(-t.total // t.L)
        for i in rng.sample(range(whole), whole // 8 + (1 if whole and rng.random() < 0.5 else 0)):
            ln = min(t.L, t.total - i * t.L)
            s = bytearray(t.staged)
            s[i * t.L + rng.choice([0, ln - 1, rng.randrange(ln)])] ^= 1 << rng.randrange(8)
            t.staged = bytes(s)
            t.flipped.add(i)
        for i in rng.sample(range(t.n), t.n // 12):
            flip_digest(t, i, rng.randrange(160))
        if t.n and rng.random() < 0.2:                      # ragged: the last slice is short, never equal
            t.digests = t.digests[:len(t.digests) - rng.randrange(1, 20)]
        if t.n and rng.random() < 0.5:
            t.avail = [int(rng.random() < 0.85) for _ in range(t.n)]
        out.append(t)
    return out
