"""The three sources of a stream request on every kind of stream (v1, v2, hybrid): rows written into the lent ring slot
(tv_stream_commit), rows copied from pageable memory and rows DMA'd from a page-locked buffer (tv_stream_commit_from).
One commit path serves all nine combinations (tv_stream.hip stream_commit_locked over tv_plan.h for_row_copies); each
kind's three bitfields must be equal to each other and to hashlib's.

The source is piece-major with a pitch above the row width (piece i at i * (L + 192), 0xFF after its valid bytes, as
in the slot), so a wrong pitch, a row copied past its bytes into the next row's or a run that swallows a short row
shows as a wrong bit.  Shapes, the smallest that reach every branch of the copy plan:

* v2 and hybrid: 70 pieces of 64 KiB in four 16 KiB columns, one request per column (more than one 64-row word); files
  end pieces at 1 byte, 16 KiB - 1, 16 KiB + 1 and 64 KiB, so a column's request holds full, short and empty rows and
  its runs of full rows are broken mid-request; a flipped byte in a full row, in a short row and just before a
  piece's end;
* v1: 70 pieces of 40,000 bytes (odd) in columns of 4,096, a last piece of 1 byte: a short row in column 0, an empty
  one in every later column; a flipped byte in the last piece and mid-shard."""
import contextlib
import ctypes
import hashlib

import pytest

from tests import hybrid_util as hu
from tests import synth
from tests.hybrid_stream_util import launches as hybrid_launches

pytestmark = pytest.mark.gpu
K = 1 << 10
SOURCES = ("slot", "pageable", "pinned")
GAP = 192                                                  # source pitch - L


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def piece_major(L, rows) -> bytearray:
    """rows: every piece's valid bytes -> piece i at i * (L + GAP), every other byte 0xFF."""
    src = bytearray(b"\xff" * (len(rows) * (L + GAP)))
    for i, data in enumerate(rows):
        src[i * (L + GAP):i * (L + GAP) + len(data)] = data
    return src


@contextlib.contextmanager
def source_memory(ctx, native, src, source):
    """What the requests are committed from: None (the lent slot), `src` itself (pageable) or a page-locked copy."""
    if source != "pinned":
        yield None if source == "slot" else src
        return
    with native.PinnedBuffer(len(src)) as pinned:
        pinned.mv[:] = src
        try:
            yield pinned.mv
        finally:
            ctx.stream_abort()                             # (nothing after stream_end; a failed test's DMAs drain here)


def drive(ctx, L, src, mem):
    """The request loop of the begun stream, every request's rows taken from the piece-major `src`: written into the
    slot (mem is None) or committed from `mem`.  -> the widths, row counts and row lengths seen."""
    pitch = L + GAP
    seen = []
    while True:
        req = ctx.stream_next()
        if not req.rows:
            return seen
        base = req.piece * pitch + req.offset
        seen.append((req.width, req.rows, [ctx.row_bytes(req, q) for q in range(req.rows)]))
        if mem is not None:
            ctx.stream_commit_from(req, mem, pitch, base)
            continue
        ctypes.memset(req.slot, 0xFF, req.rows * req.width)
        slot = ctx.stream_slot(req)
        for q, n in enumerate(seen[-1][2]):
            slot[q * req.width:q * req.width + n] = src[base + q * pitch:base + q * pitch + n]
        slot.release()
        ctx.stream_commit(req)


def stream_layout(ctx, N, total, L, P, chunk):
    ctx.set_option(N.TV_OPT_RESIDENT, 0)                   # (no resident payload: the stream's buffers only)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    ctx.set_option(N.TV_OPT_STREAM_CHUNK, chunk)
    ctx.set_layout(total, L, P)


# ---- v2 and hybrid ---------------------------------------------------------------------------------------------------

L2, C2 = 64 * K, 16 * K


@pytest.fixture(scope="module")
def hybrid_case():
    """(layout, staged files with three flipped bytes, the flipped pieces)."""
    sizes = [20 * L2 + 1, 10 * L2 + C2 - 1, 15 * L2 + C2 + 1, 22 * L2]      # pieces 0-20, 21-31, 32-47, 48-69
    lay = hu.Layout([rnd(300 + k, n) for k, n in enumerate(sizes)], L2)
    assert lay.P == 70 and [lay.pb[i] for i in (20, 31, 47, 69)] == [1, C2 - 1, C2 + 1, L2]
    staged = list(lay.files)
    staged[3] = hu.xor_at(staged[3], 5 * L2 + C2 + 4000, 0x20)              # piece 53, column 1: a full row
    staged[1] = hu.xor_at(staged[1], 10 * L2 + 100, 0x20)                   # piece 31, column 0: a short row
    staged[2] = hu.xor_at(staged[2], 15 * L2 + C2, 0x20)                    # piece 47: the byte before its end
    return lay, staged, {31, 47, 53}


def v2_rows(lay, staged):
    return [staged[f][o:o + b] for f, o, b, _ in lay.table]


def check_requests(seen, pb):
    """One request per column; column 0 has full and short rows, the later ones empty rows too, runs broken."""
    assert [(w, rows) for w, rows, _ in seen] == [(C2, 70)] * 4
    for col, (_, _, rows) in enumerate(seen):
        assert rows == [max(0, min(C2, b - col * C2)) for b in pb]
    assert {1, C2 - 1, C2} == set(seen[0][2]) and {0, 1, C2} == set(seen[1][2]) and {0, C2} == set(seen[2][2])


def test_v2_stream_from_every_source(ctx, native, hybrid_case):
    lay, staged, bad = hybrid_case
    ok2 = lay.verdicts(staged)[1]
    assert {i for i, ok in enumerate(ok2) if not ok} == bad
    src = piece_major(L2, v2_rows(lay, staged))
    got = {}
    for source in SOURCES:
        stream_layout(ctx, native, lay.total, L2, lay.P, C2)
        with source_memory(ctx, native, src, source) as mem:
            ctx.v2_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes))
            check_requests(drive(ctx, L2, src, mem), lay.pb)
            got[source] = ctx.stream_end()
        assert ctx.last_kernel() == (native.KERNEL_V2_STREAM, 4 + 2 + 1)   # the columns, two levels, the finish
    assert got["slot"] == got["pageable"] == got["pinned"] == hu.pack(ok2)


def test_hybrid_stream_from_every_source(ctx, native, hybrid_case):
    lay, staged, bad = hybrid_case
    ok1, ok2, _, _ = lay.verdicts(staged)                  # hashlib SHA-1 over the padded linear bytes; tests/v2_ref.py
    assert {i for i, ok in enumerate(ok1) if not ok} == bad == {i for i, ok in enumerate(ok2) if not ok}
    want = (hu.pack([a and b for a, b in zip(ok1, ok2)]), hu.pack(ok1), hu.pack(ok2))
    src = piece_major(L2, v2_rows(lay, staged))
    got = {}
    for source in SOURCES:
        stream_layout(ctx, native, lay.total, L2, lay.P, C2)
        ctx.set_digests(lay.pieces)
        with source_memory(ctx, native, src, source) as mem:
            ctx.hybrid_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes))
            check_requests(drive(ctx, L2, src, mem), lay.pb)
            got[source] = ctx.hybrid_stream_end()
        assert ctx.last_kernel() == (native.KERNEL_HYBRID_STREAM,
                                     hybrid_launches(lay.pb, lay.v1_len, L2, 0, lay.P, C2, lay.P))
    assert got["slot"] == got["pageable"] == got["pinned"] == want


# ---- v1 --------------------------------------------------------------------------------------------------------------

def test_v1_stream_from_every_source(ctx, native):
    L, P, C = 40000, 70, 4096
    total = (P - 1) * L + 1
    payload = bytearray(rnd(77, total))
    pieces = b"".join(hashlib.sha1(payload[o:o + L]).digest() for o in range(0, total, L))
    payload[total - 1] ^= 0x20                             # the last piece's only byte
    payload[33 * L + 20000] ^= 0x20                        # mid-shard: piece 33, column 4
    ok = [hashlib.sha1(payload[i * L:i * L + L]).digest() == pieces[20 * i:20 * i + 20] for i in range(P)]
    assert [i for i in range(P) if not ok[i]] == [33, P - 1]
    src = piece_major(L, [bytes(payload[o:o + L]) for o in range(0, total, L)])
    ncol = -(-L // C)
    got, kernels = {}, set()
    for source in SOURCES:
        stream_layout(ctx, native, total, L, P, C)
        ctx.set_digests(pieces)
        with source_memory(ctx, native, src, source) as mem:
            ctx.stream_begin()
            seen = drive(ctx, L, src, mem)
            got[source] = ctx.stream_end()
        assert [(w, rows) for w, rows, _ in seen] == [(min(C, L - col * C), P) for col in range(ncol)]
        assert seen[0][2] == [C] * (P - 1) + [1]           # the last piece: a short row in column 0 ...
        assert all(rows == [w] * (P - 1) + [0] for w, _, rows in seen[1:])    # ... an empty one in the later columns
        kernel, n = ctx.last_kernel()
        assert n == ncol == 10                             # one launch per unit
        kernels.add(kernel)
    assert got["slot"] == got["pageable"] == got["pinned"] == hu.pack(ok)
    assert len(kernels) == 1 and kernels.pop() not in (native.KERNEL_V2_STREAM, native.KERNEL_HYBRID_STREAM)
