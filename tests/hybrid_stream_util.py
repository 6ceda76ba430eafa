"""Shared by the hybrid stream tests (tests/test_plan_hybrid_stream.py, tests/test_gpu_hybrid_stream.py,
tests/test_hybrid_stream_host.py): tv_plan.h's hybrid_stream_geometry and hybrid_col_range restated in plain Python, and
the launch count of a hybrid stream.  It shares no code with torrent_amd."""
from __future__ import annotations

K, M, G = 1 << 10, 1 << 20, 1 << 30
LEAF = 16 * K
SLOT = 64 * M                     # one ring slot: the widest column
CHUNK_MAX = 256 * M               # kStreamChunkMax: a chunk buffer, at most
WIN_FLOOR = 2048                  # kHybridStreamWin
PAD_CHUNK = 64 * K                # kHybridChunk
SLACK = 256


def geometry(L: int, count: int, budget: int, chunk: int) -> tuple:
    """(column bytes, pieces per window); budget 0 = the default 1 GiB."""
    cmax = min(L, SLOT)
    if chunk:
        C = LEAF
        while C * 2 <= min(max(chunk, LEAF), cmax):
            C *= 2
        return C, count
    half = min((budget or G) // 2, CHUNK_MAX)
    w0 = min(count, WIN_FLOOR)

    def fits(C, rows):
        return half >= SLACK and rows <= (half - SLACK) // (C + 256)

    C = cmax
    while C > LEAF and not fits(C, w0):
        C //= 2
    wn = (half - SLACK) // (C + 256) // 64 * 64 if half > SLACK else 0
    return C, min(max(64, wn), count)


def window_budget(C: int, rows: int = 64) -> int:
    """The smallest budget whose chunk buffers hold `rows` rows of C bytes."""
    return 2 * (rows * (C + 256) + SLACK)


def col_range(pb: int, v1: int, offset: int, C: int) -> tuple:
    """The column-relative bytes of a row that must read as zeros; empty when b >= e."""
    return min(max(pb - offset, 0), C), min(max(v1 - offset, 0), C)


def col_chunks(b: int, e: int) -> int:
    return -(-(e - b // 16 * 16) // PAD_CHUNK) if b < e else 0


def launches(pb, v1_len, L: int, first: int, count: int, C: int, wn: int) -> int:
    """Per unit 2 (+ 1 where a row has a pad range inside the column), per window log2(L / C) + 1."""
    ncol, n = L // C, 0
    for j0 in range(0, count, wn):
        rows = range(first + j0, first + min(j0 + wn, count))
        for col in range(ncol):
            pad = any(b < e for b, e in (col_range(pb[i], v1_len[i], col * C, C) for i in rows))
            n += 2 + (1 if pad else 0)
        n += ncol.bit_length() - 1 + 1
    return n
