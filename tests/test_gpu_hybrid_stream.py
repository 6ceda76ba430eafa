"""Streamed hybrid verify (tv_hybrid_stream_begin / _end / _file_table and the stream hosts of torrent_amd/hybrid.py):
every ABI case is driven request by request from Python, the requests held to the geometry rule of tv_plan.h
hybrid_stream_geometry (restated in tests/hybrid_stream_util.py), the slot bytes past each row's valid length filled
with 0xFF, and all three bitfields compared bit for bit with tests/hybrid_util.Layout.verdicts (hashlib SHA-1 over the
padded linear bytes, tests/v2_ref.py for the merkle side) -- where the shard also fits resident, with tv_hybrid_verify on
the same bytes too.  Before each real stream a stream of all-0xFF full-length pieces runs on the same ctx with the same
geometry, so the chunk buffers hold stale non-zero bytes exactly where the pad ranges must read as zeros.

The shapes are the smallest that reach each path: L = 16 KiB (one column, c = 1); L = 64 KiB in four 16 KiB columns
(pad ranges that start before, inside and at the edge of a column, and columns wholly in the pad: SHA-1 hashes C zeros,
v2 takes the zero subtree); L = 1 MiB in 256 KiB columns (multi-chunk pad ranges); two windows (64 + 2 pieces);
mid-shard starts; a short last v1 piece and a trailing pad."""
import ctypes
import functools
import os
import random

import pytest

from tests import hybrid_util as hu
from tests import synth
from tests.hybrid_fuzz import draw
from tests.hybrid_stream_util import K, M, SLOT, geometry, launches, window_budget
from tests.v2_util import file_names, set_bits

pytestmark = pytest.mark.gpu
KERNEL_LANE, KERNEL_SPLIT, KERNEL_TWIN = 1, 2, 4


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def sizes(L):
    return [1, 15, 16, 17, 16383, 16384, 16385, L - 1, L, L + 1, 2 * L + 5]


@functools.lru_cache(maxsize=None)
def layout(L: int, trailing: bool, short_last: bool = False) -> hu.Layout:
    """Files of every edge size and one zero-length file; short_last: the last file ends in a short piece (with
    trailing: a pad follows it, else the last v1 piece is short)."""
    ns = sizes(L)
    ns.insert(4, 0)
    if not short_last:
        ns.append(L)                                          # the last file ends a piece: no tail at the end
    return hu.Layout([rnd(100 + k, n) for k, n in enumerate(ns)], L, trailing)


def want(lay, staged=None, first=0, count=None, pieces=None, hashes=None, clear=()):
    """(bitfield, v1, v2) of the shard from hashlib / v2_ref."""
    count = lay.P - first if count is None else count
    ok1, ok2, _, _ = lay.verdicts(lay.files if staged is None else staged, pieces, hashes)
    ok1 = [ok and i not in clear for i, ok in enumerate(ok1)][first:first + count]
    ok2 = [ok and i not in clear for i, ok in enumerate(ok2)][first:first + count]
    return hu.pack([a and b for a, b in zip(ok1, ok2)]), hu.pack(ok1), hu.pack(ok2)


def stream_layout(ctx, N, lay, first, count, chunk, budget, pieces=None, total=None):
    ctx.set_option(N.TV_OPT_RESIDENT, 0)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
    ctx.set_option(N.TV_OPT_STREAM_CHUNK, chunk)
    ctx.set_layout(lay.total if total is None else total, lay.L, lay.P, first, count)
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    if pieces is not False:
        ctx.set_digests(lay.pieces if pieces is None else pieces)


def drive(ctx, lay, staged, first, count, chunk=0, budget=0, unreadable=(), from_src=False, stop_after=None):
    """The request loop of an active hybrid stream: every request held to the geometry rule, the slot filled with 0xFF
    and then row q's valid bytes of `staged`.  -> geometry info."""
    L = lay.L
    C, wn = geometry(L, count, budget, chunk)
    ncol, per = L // C, max(1, SLOT // C)
    expect = []
    for j0 in range(0, count, wn):
        wc = min(wn, count - j0)
        for col in range(ncol):
            for r0 in range(0, wc, per):
                expect.append((first + j0 + r0, min(per, wc - r0), col * C))
    for seq, (piece, rows, offset) in enumerate(expect, 1):
        if stop_after is not None and seq > stop_after:
            return None
        req = ctx.stream_next()
        assert (req.piece, req.rows, req.offset, req.width, req.seq) == (piece, rows, offset, C, seq)
        ctypes.memset(req.slot, 0xFF, rows * C)
        slot = ctx.stream_slot(req)
        src = bytearray(b"\xff" * (rows * C)) if from_src else None
        for q in range(rows):
            f, o, b, w = lay.table[piece + q]
            n = max(0, min(C, b - offset))
            assert ctx.row_bytes(req, q) == n
            if n:
                (src if from_src else slot)[q * C:q * C + n] = staged[f][o + offset:o + offset + n]
        slot.release()
        for i in unreadable:
            if piece <= i < piece + rows and offset == 0:
                ctx.stream_unreadable(i)
        if from_src:
            ctx.stream_commit_from(req, src, C)
        else:
            ctx.stream_commit(req)
    assert ctx.stream_next().rows == 0
    return {"C": C, "wn": wn, "ncol": ncol, "nwin": -(-count // wn)}


def dirty(ctx, N, L, P, chunk, budget):
    """A first stream of P full-length all-0xFF pieces under the same geometry: the chunk buffers keep its bytes."""
    full = hu.Layout.__new__(hu.Layout)
    full.L, full.P, full.total = L, P, P * L
    full.table = [(0, i * L, L, L // (16 * K)) for i in range(P)]
    full.pieces = bytes(20 * P)
    stream_layout(ctx, N, full, 0, P, chunk, budget)
    ctx.hybrid_stream_begin([L] * P, [L // (16 * K)] * P, bytes(32 * P))
    ones = b"\xff" * (P * L)
    drive(ctx, full, [ones], 0, P, chunk, budget)
    assert ctx.hybrid_stream_end() == (bytes((P + 7) // 8),) * 3


def run_stream(ctx, N, lay, staged=None, first=0, count=None, chunk=0, budget=0, avail=None, pieces=None, hashes=None,
               end="hybrid", pre=True, **kw):
    staged = lay.files if staged is None else staged
    count = lay.P - first if count is None else count
    if pre:
        dirty(ctx, N, lay.L, lay.P, chunk, budget)
    stream_layout(ctx, N, lay, first, count, chunk, budget, pieces)
    ctx.hybrid_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes if hashes is None else hashes), avail)
    info = drive(ctx, lay, staged, first, count, chunk, budget, **kw)
    got = ctx.hybrid_stream_end() if end == "hybrid" else ctx.stream_end()
    kernel, n = ctx.last_kernel()
    assert kernel == N.KERNEL_HYBRID_STREAM == 256
    assert n == launches(lay.pb, lay.v1_len, lay.L, first, count, info["C"], info["wn"])
    k_ms, total_ms = ctx.last_timing()
    assert 0 < k_ms <= total_ms
    return got, info


def run_resident(ctx, N, lay, staged=None, pieces=None, hashes=None, avail=None):
    """tv_hybrid_verify on the same bytes (the shard resident)."""
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    hu.load(ctx, lay, pieces=pieces, hashes=hashes, staged=staged)
    return ctx.hybrid_verify(avail)


def flipped(data: bytes, pos: int) -> bytes:
    return hu.xor_at(data, pos, 0x20)


# ---- shapes ----------------------------------------------------------------------------------------------------------

SHAPES = [(16 * K, 0), (64 * K, 16 * K), (1 * M, 256 * K)]


@pytest.mark.parametrize("trailing,short_last", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("L,chunk", SHAPES)
def test_clean_and_corrupted_bytes(ctx, native, L, chunk, trailing, short_last):
    lay = layout(L, trailing, short_last)
    got, info = run_stream(ctx, native, lay, chunk=chunk)
    assert info["C"] == (chunk or L) and info["nwin"] == 1
    assert got == (set_bits(lay.P),) * 3 == want(lay)
    # a flipped file byte in the first and in the last column of a piece (the last byte before a pad range), and the
    # last byte of the torrent: both bits of those pieces only
    staged = list(lay.files)
    staged[0] = flipped(staged[0], 0)                          # the 1-byte file: piece 0
    k = len(staged) - (1 if short_last else 2)                 # the 2L + 5 file: its first and its last piece
    staged[k] = flipped(flipped(staged[k], L - 1), 2 * L + 4)
    p0 = lay.first_piece(k)
    got, _ = run_stream(ctx, native, lay, staged, chunk=chunk, pre=False)
    assert got == (set_bits(lay.P, clear={0, p0, p0 + 2}),) * 3 == want(lay, staged)
    assert got == run_resident(ctx, native, lay, staged)


def test_a_torrent_without_a_tail_launches_no_pad_kernel(ctx, native):
    L = 64 * K
    lay = hu.Layout([rnd(7, 5 * L)], L)
    assert lay.tails == []
    got, info = run_stream(ctx, native, lay, chunk=16 * K)
    assert got == (set_bits(5),) * 3
    assert ctx.last_kernel() == (256, 4 * 2 + 2 + 1)          # per column SHA-1 + v2; two levels and the finish
    lay = hu.Layout([rnd(7, 4 * L + 100)], L, trailing=True)   # ... and a tail in the last piece only: one pad launch per column
    got, info = run_stream(ctx, native, lay, chunk=16 * K)
    assert got == (set_bits(5),) * 3 == want(lay)
    assert ctx.last_kernel() == (256, 4 * 3 + 2 + 1)


# ---- windows ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_66():
    L = 16 * K
    # pieces 0-3, 4, 5-46, 47-48, 49-64, 65: the last window holds piece 64 (a file's 16,383-byte tail) and piece 65
    ns = [3 * L + 5, 17, 42 * L, 2 * L - 1, 15 * L + 16383, 5]
    return hu.Layout([rnd(200 + k, n) for k, n in enumerate(ns)], L, trailing=True)


def test_two_windows_and_mid_shard_starts(ctx, native):
    lay = layout_66()
    assert lay.P == 66
    budget = window_budget(16 * K)
    staged = list(lay.files)
    staged[4] = flipped(staged[4], 15 * lay.L - 1)            # piece 63 (the first window's last): its last byte
    staged[5] = flipped(staged[5], 4)                         # piece 65 (the last window's last)
    got, info = run_stream(ctx, native, lay, staged, budget=budget)
    assert (info["C"], info["wn"], info["nwin"]) == (16 * K, 64, 2)
    assert got == (set_bits(66, clear={63, 65}),) * 3 == want(lay, staged)
    assert got == run_resident(ctx, native, lay, staged)
    # a mid-shard first: 8, and 48 = one past a file boundary (file 3 starts at piece 47; piece 48 is its tail)
    for first, count in ((8, 58), (48, 18), (48, 11)):
        got, _ = run_stream(ctx, native, lay, staged, first=first, count=count, budget=budget, pre=False)
        assert got == want(lay, staged, first, count)


# ---- the SHA-1 kernel forms, and both commit calls ---------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [KERNEL_LANE, KERNEL_SPLIT, KERNEL_TWIN])
def test_v1_kernel_forms(ctx, native, kernel):
    lay = layout(64 * K, True, True)
    staged = list(lay.files)
    staged[5] = flipped(staged[5], 16382)                      # the 16,383-byte file
    ctx.set_option(native.TV_OPT_KERNEL, kernel)
    try:
        got, _ = run_stream(ctx, native, lay, staged, chunk=16 * K)
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
    assert got == want(lay, staged) and got[0] == set_bits(lay.P, clear={lay.first_piece(5)})


def test_commit_from_pageable_memory(ctx, native):
    lay = layout(64 * K, False, True)
    got, _ = run_stream(ctx, native, lay, chunk=16 * K, from_src=True)
    assert got == (set_bits(lay.P),) * 3


# ---- verdicts ------------------------------------------------------------------------------------------------------------

def test_descriptions_that_disagree(ctx, native):
    from torrent_amd.hybrid import HybridResult
    lay = layout(64 * K, True, True)
    pieces = hu.xor_at(lay.pieces, 20 * 3 + 7, 1)
    hashes = list(lay.hashes)
    hashes[6] = hu.xor_at(hashes[6], 31, 0x80)
    got, _ = run_stream(ctx, native, lay, chunk=16 * K, pieces=pieces, hashes=hashes)
    assert got == (set_bits(lay.P, clear={3, 6}), set_bits(lay.P, clear={3}), set_bits(lay.P, clear={6}))
    assert got == want(lay, pieces=pieces, hashes=hashes) == run_resident(ctx, native, lay, pieces=pieces, hashes=hashes)
    assert HybridResult(*map(bytearray, got)).disagree == [3, 6]
    # tv_stream_end on a hybrid stream: v1 AND v2
    both, _ = run_stream(ctx, native, lay, chunk=16 * K, pieces=pieces, hashes=hashes, end="plain", pre=False)
    assert both == got[0]
    # a ragged `pieces` string (the last slice short): v1 0 for that piece, v2 unchanged
    got, _ = run_stream(ctx, native, lay, chunk=16 * K, pieces=lay.pieces[:-5], pre=False)
    assert got == (set_bits(lay.P, clear={lay.P - 1}),) * 2 + (set_bits(lay.P),)


def test_unreadable_and_unavailable_pieces_clear_all_three(ctx, native):
    lay = layout(64 * K, False, True)
    avail = bytearray(set_bits(lay.P, clear={2, 9}))
    got, _ = run_stream(ctx, native, lay, chunk=16 * K, avail=bytes(avail), unreadable=(5, lay.P - 1))
    assert got == (set_bits(lay.P, clear={2, 5, 9, lay.P - 1}),) * 3


# ---- calls ---------------------------------------------------------------------------------------------------------------

def _code(N, fn, *a):
    with pytest.raises(N.NativeError) as ei:
        fn(*a)
    return ei.value.code


def test_call_rules(native):
    N = native
    lay = layout(64 * K, False, True)
    hashes = b"".join(lay.hashes)
    with N.Context(0) as c:
        assert _code(N, c.hybrid_stream_begin, lay.pb, lay.tl, hashes) == N.TV_ERR_STATE      # before tv_set_layout
        stream_layout(c, N, lay, 0, lay.P, 16 * K, 0, pieces=False)
        assert _code(N, c.hybrid_stream_begin, lay.pb, lay.tl, hashes) == N.TV_ERR_STATE      # without digests
        assert "tv_set_digests" in c._err()
        assert _code(N, c.stream_next) == N.TV_ERR_STATE
        # a piece_bytes[i] > v1_len(i): the layout's total_length ends inside the last piece's bytes; no stream is left
        stream_layout(c, N, lay, 0, lay.P, 16 * K, 0, total=lay.total - 1)
        assert _code(N, c.hybrid_stream_begin, lay.pb, lay.tl, hashes) == N.TV_ERR_ARG and "v1 length" in c._err()
        assert _code(N, c.stream_next) == N.TV_ERR_STATE
        # tv_hybrid_stream_end on a stream that is not hybrid: refused, and the stream stays active
        stream_layout(c, N, lay, 0, lay.P, 16 * K, 0)
        c.v2_stream_begin(lay.pb, lay.tl, hashes)
        assert _code(N, c.hybrid_stream_end) == N.TV_ERR_STATE
        assert c.stream_next().rows > 0
        c.stream_abort()
        # two streams: the second allocates no device memory
        first, _ = run_stream(c, N, lay, chunk=16 * K, pre=False)
        allocs = c.counter(N.TV_COUNTER_DEVICE_ALLOCS)
        held = c.counter(N.TV_COUNTER_DEVICE_BYTES)
        again, _ = run_stream(c, N, lay, chunk=16 * K, pre=False)
        assert first == again == (set_bits(lay.P),) * 3
        assert c.counter(N.TV_COUNTER_DEVICE_ALLOCS) == allocs and c.counter(N.TV_COUNTER_DEVICE_BYTES) == held
        assert c.counter(N.TV_COUNTER_LAST_WORKGROUPS) > 0
        # abort mid-stream, then a resident tv_hybrid_verify on the same ctx
        stream_layout(c, N, lay, 0, lay.P, 16 * K, 0)
        c.hybrid_stream_begin(lay.pb, lay.tl, hashes)
        assert drive(c, lay, lay.files, 0, lay.P, 16 * K, 0, stop_after=2) is None
        c.stream_abort()
        assert run_resident(c, N, lay) == (set_bits(lay.P),) * 3
        # an empty shard
        stream_layout(c, N, lay, lay.P, 0, 16 * K, 0)
        c.hybrid_stream_begin(lay.pb, lay.tl, hashes)
        assert c.stream_next().rows == 0
        assert c.hybrid_stream_end() == (b"", b"", b"")


# ---- files and hosts -------------------------------------------------------------------------------------------------------

def _write(root, files, skip=()):
    paths = file_names(len(files))
    for k, (comps, d) in enumerate(zip(paths, files)):
        p = os.path.join(root, *comps)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if k not in skip:
            with open(p, "wb") as f:
                f.write(d)
    return paths


@pytest.mark.parametrize("trailing", [False, True])
def test_file_table_and_hosts(ctx, native, tmp_path, trailing):
    from torrent_amd import (parse_metainfo_hybrid, verify_files_hybrid, verify_payload_hybrid, verify_stream_hybrid)
    N = native
    L = 64 * K
    lay = layout(L, trailing, True)
    root = str(tmp_path)
    on_disk = list(lay.files)
    on_disk[7] = on_disk[7][:-1]                              # a short file (16,385 bytes declared)
    on_disk[9] = flipped(on_disk[9], L - 1)                   # a flipped byte
    paths = _write(root, on_disk, skip={2})                   # a missing file
    ro = os.path.join(root, *paths[10])                       # an unwritable file: read under TV_OPT_OPEN_RW = 0
    os.chmod(ro, 0o444)
    pieces = hu.xor_at(lay.pieces, 20 * 1 + 3, 2)             # the torrent states piece 1's digest wrongly
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(lay.files, L, paths=paths, trailing_pad=trailing, pieces=pieces))
    assert meta is not None and meta.total_length == lay.total
    resident = verify_files_hybrid(meta, root)
    gone = {lay.first_piece(2), lay.first_piece(7)}
    v1 = set_bits(lay.P, clear=gone | {1, lay.first_piece(9)})
    v2 = set_bits(lay.P, clear=gone | {lay.first_piece(9)})
    assert (bytes(resident.bitfield), bytes(resident.v1), bytes(resident.v2)) == (v1, v1, v2)
    # the ABI call, on the module's ctx (its chunk buffers hold the bytes of earlier streams)
    stream_layout(ctx, N, lay, 0, lay.P, 16 * K, 0, pieces)
    ctx.set_option(N.TV_OPT_OPEN_RW, 0)
    try:
        full = [os.path.join(root, *comps) for comps in paths]
        bits, status = ctx.hybrid_stream_file_table(lay.pb, lay.tl, b"".join(lay.hashes), lay.lengths, full)
    finally:
        ctx.set_option(N.TV_OPT_OPEN_RW, 1)
    assert bits == (v1, v1, v2)
    assert [k for k, s in enumerate(status) if s != N.TV_OK] == [2, 7]
    assert ctx.last_kernel()[0] == 256
    # the hosts: equal to their resident forms, on one device and on two shards; never raising for size
    for devices in (None, [0, 0]):
        r = verify_files_hybrid(meta, root, devices=devices, stream=True)
        assert (r.bitfield, r.v1, r.v2) == (resident.bitfield, resident.v1, resident.v2) and r.disagree == [1]
    bufs = list(on_disk)
    bufs[2] = None
    for devices in (None, [0, 0]):
        r = verify_payload_hybrid(meta, bufs, devices=devices, stream=True)
        assert (r.bitfield, r.v1, r.v2) == (resident.bitfield, resident.v1, resident.v2)
        assert verify_payload_hybrid(meta, bufs, devices=devices).v1 == r.v1
    small = 6 * L
    with pytest.raises(MemoryError):
        verify_payload_hybrid(meta, bufs, budget=small)
    with pytest.raises(MemoryError):
        verify_files_hybrid(meta, root, budget=small)
    assert verify_payload_hybrid(meta, bufs, budget=small, stream=True).v1 == resident.v1
    r = verify_files_hybrid(meta, root, budget=small, stream=True)
    assert (r.bitfield, r.v1, r.v2) == (resident.bitfield, resident.v1, resident.v2)
    avail = set_bits(lay.P, clear={4})
    r = verify_stream_hybrid(meta, lambda k, o, n: None if bufs[k] is None or len(bufs[k]) < o + n else bufs[k][o:o + n],
                             avail=avail, chunk=16 * K, threads=2)
    assert bytes(r.v2) == set_bits(lay.P, clear=gone | {4, lay.first_piece(9)}) and r.disagree == [1]


# ---- a small seeded fuzz: tests/hybrid_fuzz.py's draw, a drawn chunk or budget per case -------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 3, 6, 10, 11, 17, 20])
def test_fuzz(ctx, native, seed):
    d = draw(seed)
    lay = d.layout()
    pieces, hashes = d.stated(lay)
    rng = random.Random(9100 + seed)
    L = lay.L
    if rng.random() < 0.5:
        chunk, budget = rng.choice([c for c in (16 * K, 32 * K, 64 * K, 256 * K, L) if c <= L]), 0
    else:
        chunk, budget = 0, window_budget(rng.choice([c for c in (16 * K, 64 * K, L) if c <= L]), rng.choice([64, 128]))
    ctx.set_option(native.TV_OPT_KERNEL, d.kernel)
    try:
        whole, _ = run_stream(ctx, native, lay, d.staged, chunk=chunk, budget=budget, pieces=pieces, hashes=hashes)
        first, count = d.shards[-1]
        part, _ = run_stream(ctx, native, lay, d.staged, first=first, count=count, chunk=chunk, budget=budget,
                             pieces=pieces, hashes=hashes, pre=False)
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
    assert whole == want(lay, d.staged, pieces=pieces, hashes=hashes)
    assert part == want(lay, d.staged, first, count, pieces=pieces, hashes=hashes)
    assert whole == run_resident(ctx, native, lay, d.staged, pieces=pieces, hashes=hashes)
