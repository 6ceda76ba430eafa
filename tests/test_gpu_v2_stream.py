"""Streamed BitTorrent v2 verify (tv_v2_stream_begin, tv_v2_stream_file_table and the stream=True hosts of
torrent_amd/v2.py): every case is driven request by request from Python, the requests' offset / width / rows are held
to the geometry rule of tv_plan.h v2_stream_geometry (restated here), and every bitfield is compared bit for bit with
tests/v2_ref.py (hashlib) -- where the shard also fits resident, with tv_v2_verify on the same bytes too.

The shapes are the smallest that take each path of the column kernel: c = 1 (the leaf is the node), c < 256 (several
rows per workgroup), c = 256, c = 512 (two tiles) and c = 4,096 (16 tiles, a 128 MiB piece in two 64 MiB columns);
trees narrower than a column, short last pieces that end at and inside a column, a column wholly past a piece's bytes
(the all-zero subtree); one window and several, with a last window of two pieces; chunk buffers reused by a window of
shorter rows."""
import ctypes
import functools
import os

import pytest

from tests import synth, v2_ref
from tests.v2_fuzz import SEEDS, draw
from tests.v2_util import file_names, golden, golden_files, set_bits, torrent_v2

pytestmark = pytest.mark.gpu
K, M, G = 1 << 10, 1 << 20, 1 << 30
LEAF = 16 * K
SLOT = 64 * M


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def flipped(data: bytes, positions) -> bytes:
    b = bytearray(data)
    for pos in positions:
        b[pos] ^= 0x20
    return bytes(b)


def _and(a: bytes, b: bytes) -> bytes:
    assert len(a) == len(b)
    return bytes(x & y for x, y in zip(a, b))


class Case:
    """Files as the torrent describes them: the piece table and the expected piece hashes (computed once)."""

    def __init__(self, L, files):
        self.L, self.files = L, list(files)
        self.lengths = [len(f) for f in files]
        self.table = v2_ref.piece_table(self.lengths, L)
        self.P = len(self.table)
        self.expected = []
        for f in files:
            self.expected += v2_ref.file_hashes(f, L)[2]
        self.hashes = b"".join(self.expected)
        self.bytes = [r[2] for r in self.table]
        self.leaves = [r[3] for r in self.table]
        self.total = (self.P - 1) * L + self.table[-1][2]

    def want(self, staged, clear=()):
        bf = bytearray(v2_ref.expected_bitfield(staged, self.L, self.expected, have=self.lengths))
        for i in clear:
            bf[i >> 3] &= ~(0x80 >> (i & 7)) & 0xFF
        return bytes(bf)


def geometry(L, count, budget, chunk):
    """tv_plan.h v2_stream_geometry restated: (column bytes, pieces per window)."""
    cmax = min(L, SLOT)
    if chunk:
        C = LEAF
        while C * 2 <= min(max(chunk, LEAF), cmax):
            C *= 2
        return C, count
    half = (budget or G) // 2

    def fits(C, rows):
        return half >= 256 and rows <= (half - 256) // (C + 256)

    C = cmax
    while C > LEAF and not fits(C, 64):
        C //= 2
    wn = max(64, (half - 256) // (C + 256) // 64 * 64 if half > 256 else 0)
    return C, min(wn, count)


def window_budget(C, rows=64):
    """The smallest budget whose chunk buffers hold `rows` rows of C bytes."""
    return 2 * (rows * (C + 256) + 256)


def stream_layout(ctx, N, case, first=0, count=None, chunk=0, budget=0):
    count = case.P - first if count is None else count
    ctx.set_option(N.TV_OPT_RESIDENT, 0)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
    ctx.set_option(N.TV_OPT_STREAM_CHUNK, chunk)
    ctx.set_layout(case.total, case.L, case.P, first, count)
    return count


def drive(ctx, case, staged, first, count, chunk=0, budget=0, unreadable=(), filler=None, from_src=False):
    """The request loop of an active v2 stream: every request held to the geometry rule, row q filled with the bytes
    of `staged` (filler: the byte written past each row's valid bytes).  -> (bitfield, info)."""
    L = case.L
    C, wn = geometry(L, count, budget, chunk)
    ncol, per = L // C, max(1, SLOT // C)
    expect = []
    for j0 in range(0, count, wn):
        wc = min(wn, count - j0)
        for col in range(ncol):
            for r0 in range(0, wc, per):
                expect.append((first + j0 + r0, min(per, wc - r0), col * C))
    seq = 0
    for piece, rows, offset in expect:
        req = ctx.stream_next()
        seq += 1
        assert (req.piece, req.rows, req.offset, req.width, req.seq) == (piece, rows, offset, C, seq)
        slot = ctx.stream_slot(req)
        if filler is not None:
            ctypes.memset(req.slot, filler, rows * C)
        src = bytearray(rows * C) if from_src else None
        for q in range(rows):
            f, o, b, w = case.table[piece + q]
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
    bits = ctx.stream_end()
    nwin = -(-count // wn)
    return bits, {"C": C, "wn": wn, "ncol": ncol, "nwin": nwin, "requests": len(expect)}


def run_stream(ctx, N, case, staged=None, first=0, count=None, chunk=0, budget=0, avail=None, **kw):
    staged = case.files if staged is None else staged
    count = stream_layout(ctx, N, case, first, count, chunk, budget)
    ctx.v2_stream_begin(case.bytes, case.leaves, case.hashes, avail)
    bits, info = drive(ctx, case, staged, first, count, chunk, budget, **kw)
    kernel, launches = ctx.last_kernel()
    assert kernel == N.KERNEL_V2_STREAM == 32
    logn = info["ncol"].bit_length() - 1
    assert launches <= info["nwin"] * (info["ncol"] + logn + 1)
    assert launches == info["nwin"] * (info["ncol"] + logn + 1)     # (this engine's count: no launch is skipped)
    k_ms, total_ms = ctx.last_timing()
    assert 0 < k_ms <= total_ms
    return bits, info


def run_resident(ctx, N, case, staged, avail=None):
    """tv_v2_verify on the same bytes (the shard resident)."""
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    ctx.set_layout(case.total, case.L, case.P, 0, case.P)
    ctx.v2_set_pieces(case.bytes, case.leaves, case.hashes)
    offs, p = [], 0
    for n in case.lengths:
        offs.append(p * case.L)
        p += -(-n // case.L)
    ctx.stage_many([(o, d) for o, d in zip(offs, staged) if len(d)])
    return ctx.v2_verify(avail)


# ---- L = 16 KiB: the leaf is the root ---------------------------------------------------------------------------------

def test_one_leaf_pieces(ctx, native):
    case = Case(16 * K, [rnd(1, 5 * 16 * K + 100), rnd(2, 1), rnd(3, 16 * K)])
    assert case.leaves == [1] * 8
    bits, info = run_stream(ctx, native, case)
    assert (info["C"], info["ncol"], info["nwin"]) == (16 * K, 1, 1)
    assert bits == set_bits(8) == case.want(case.files)
    assert ctx.last_kernel() == (32, 2)                     # the column launch and the finish launch, no level
    staged = [flipped(case.files[0], [3 * 16 * K + 7, 5 * 16 * K + 99]), case.files[1], flipped(case.files[2], [16383])]
    bits, _ = run_stream(ctx, native, case, staged)
    assert bits == set_bits(8, clear={3, 5, 7}) == case.want(staged)


# ---- L = 64 KiB, 130 pieces: c = 1 in four columns, and three windows of whole pieces ----------------------------------

@functools.lru_cache(maxsize=None)
def case_130():
    L = 64 * K
    case = Case(L, [rnd(10, 129 * L + 777)])
    bad = [(0, 0), (63, 1), (64, 2), (127, 3), (128, 1), (129, 0)]     # (piece, column of 16 KiB): one in each column
    staged = [flipped(case.files[0], [i * L + col * LEAF + 123 + i for i, col in bad])]
    return case, staged, {i for i, _ in bad}


@pytest.mark.parametrize("mode", ["chunk16k", "windows64"])
def test_130_pieces(ctx, native, mode):
    case, staged, bad = case_130()
    L = case.L
    kw = {"chunk": 16 * K} if mode == "chunk16k" else {"budget": window_budget(L)}
    avail = bytearray(set_bits(130, clear={5}))           # a cleared bit on a good piece; the bad ones keep theirs
    bits, info = run_stream(ctx, native, case, staged, avail=bytes(avail), unreadable=[70], **kw)
    if mode == "chunk16k":
        assert (info["C"], info["ncol"], info["wn"], info["nwin"]) == (16 * K, 4, 130, 1)
        assert ctx.last_kernel() == (32, 4 + 2 + 1)
    else:
        assert (info["C"], info["ncol"], info["wn"], info["nwin"]) == (L, 1, 64, 3)      # the last window: 2 pieces
        assert ctx.last_kernel() == (32, 3 * 2)
    assert bits == set_bits(130, clear=bad | {5, 70}) == case.want(staged, clear={5, 70})
    assert run_resident(ctx, native, case, staged, bytes(set_bits(130, clear={5, 70}))) == bits
    clean, _ = run_stream(ctx, native, case, **kw)
    assert clean == set_bits(130)


# ---- L = 8 MiB: the tiled path (two tiles), c = 256 untiled, c = 4 in 128 columns ---------------------------------------

@functools.lru_cache(maxsize=None)
def case_8m():
    L = 8 * M
    case = Case(L, [rnd(20, 3 * L - 5)])
    staged = [flipped(case.files[0], [2 * L - 9, 3 * L - 6])]   # the last leaf of piece 1, the last valid byte of piece 2
    return case, staged


@pytest.mark.parametrize("chunk", [0, 4 * M, 64 * K])
def test_8m_pieces(ctx, native, chunk):
    case, staged = case_8m()
    L = case.L
    assert case.bytes == [L, L, L - 5] and case.leaves == [512] * 3
    kw = {"chunk": chunk} if chunk else {"budget": window_budget(L)}
    bits, info = run_stream(ctx, native, case, **kw)
    assert (info["C"], info["ncol"], info["nwin"]) == (chunk or L, L // (chunk or L), 1)
    assert bits == set_bits(3)
    wg = ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS)
    assert wg == (3 if info["C"] >= 4 * M else -(-3 // (256 // (info["C"] // LEAF))))
    bits, _ = run_stream(ctx, native, case, staged, **kw)
    assert bits == set_bits(3, clear={1, 2}) == case.want(staged)


# ---- L = 128 MiB: a piece longer than a ring slot: two columns of 4,096 leaves (16 tiles), an all-zero column ----------

def test_128m_piece(ctx, native):
    L = 128 * M
    case = Case(L, [rnd(30, L + LEAF + 1)])
    assert case.bytes == [L, LEAF + 1] and case.leaves == [8192, 8192]
    bits, info = run_stream(ctx, native, case, chunk=L)        # (capped at the ring slot)
    assert (info["C"], info["ncol"], info["nwin"], info["requests"]) == (64 * M, 2, 1, 4)
    assert bits == set_bits(2)              # piece 1's second column is the all-zero subtree of 4,096 leaves
    staged = [flipped(case.files[0], [L - 1, L + LEAF])]       # piece 0's last byte (column 1), piece 1's last byte
    bits, _ = run_stream(ctx, native, case, staged, chunk=L)
    assert bits == set_bits(2, clear={0, 1})


# ---- L = 1 MiB in columns of 256 KiB: trees narrower than a column, pieces ending at and inside a column ------------------

@functools.lru_cache(maxsize=None)
def case_narrow():
    L = M
    sizes = [1, 16384, 16385, 262144, 262145, 1048575,           # one-piece files: tree widths 1, 1, 2, 16, 32, 64
             L + 512 * K, L + 256 * K, 2 * L + 768 * K,          # the last piece ends exactly at a column boundary
             L + 300000, L + 1, 2 * L + 540000 + LEAF // 2]      # ... or in the middle of a leaf
    case = Case(L, [rnd(40 + k, n) for k, n in enumerate(sizes)])
    return case


def test_narrow_trees_and_edges(ctx, native):
    case = case_narrow()
    assert case.leaves[:6] == [1, 1, 2, 16, 32, 64] and set(case.leaves[6:]) == {64}
    for kw in ({"chunk": 256 * K}, {"chunk": 64 * K}, {"budget": window_budget(M)}):
        bits, info = run_stream(ctx, native, case, **kw)
        assert bits == set_bits(case.P), kw
    # the last valid byte of every piece flipped: every piece drops; the first byte of each file: its first piece
    staged = [flipped(f, {min(len(f), (q + 1) * case.L) - 1 for q in range(-(-len(f) // case.L))}) for f in case.files]
    bits, _ = run_stream(ctx, native, case, staged, chunk=256 * K)
    assert bits == bytes(len(bits)) == case.want(staged)
    staged = [flipped(f, [0]) for f in case.files]
    bits, _ = run_stream(ctx, native, case, staged, chunk=256 * K, from_src=True)
    assert bits == case.want(staged) and bits != bytes(len(bits))
    assert run_resident(ctx, native, case, staged) == bits


# ---- stale bytes: a window of full pieces, then windows of short pieces in the same chunk buffers -----------------------

def test_stale_bytes_are_never_hashed(ctx, native):
    L = 64 * K
    sizes = [64 * L] + [1 + (7919 * k) % (L - 1) for k in range(126)] + [LEAF, LEAF + 1]
    case = Case(L, [rnd(60 + k, n) for k, n in enumerate(sizes)])
    assert case.P == 64 + 128
    got = []
    for filler in (0x00, 0xFF):
        bits, info = run_stream(ctx, native, case, budget=window_budget(L), filler=filler)
        assert (info["wn"], info["nwin"], info["ncol"]) == (64, 3, 1)
        got.append(bits)
    assert got[0] == got[1] == set_bits(case.P)
    for filler in (0x00, 0xFF):     # and in columns: the short rows of later columns are not copied at all
        bits, _ = run_stream(ctx, native, case, budget=window_budget(LEAF), filler=filler)
        assert bits == set_bits(case.P)


# ---- shards: the global table on every shard ----------------------------------------------------------------------------

def test_shards(ctx, native):
    case, staged, bad = case_130()
    whole, _ = run_stream(ctx, native, case, staged, chunk=32 * K)
    parts = b""
    for first, count in ((0, 48), (48, 40), (88, 42)):
        bits, info = run_stream(ctx, native, case, staged, first=first, count=count, chunk=32 * K)
        assert info["wn"] == count
        parts += bits
    assert parts == whole == set_bits(130, clear=bad)


# ---- the golden layouts and the seeded fuzz, through the hosts ------------------------------------------------------------

def _write(root, paths, buffers):
    for comps, data in zip(paths, buffers):
        if data is None:
            continue
        p = root.joinpath(*comps)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)


def _hosts(tmp_path, L, files, disk, lengths, expected):
    """Every streamed host under a budget of 64 rows of a quarter piece (columns, and two windows where the layout
    has more than 64 pieces), verify_stream_v2 under 32 KiB columns, and the resident call."""
    from torrent_amd import parse_metainfo_v2, verify_files_v2, verify_payload_v2, verify_stream_v2
    paths = file_names(len(files))
    meta = parse_metainfo_v2(torrent_v2(files, L, name="st", paths=paths))
    assert meta is not None and meta.layout.hashes == b"".join(expected)
    want = v2_ref.expected_bitfield(disk, L, expected, have=lengths)
    budget = window_budget(max(LEAF, L // 4))
    assert geometry(L, meta.n_pieces, budget, 0) == (max(LEAF, L // 4), min(64, meta.n_pieces))

    def read(k, offset, n):
        return None if disk[k] is None else disk[k][offset:offset + n]

    assert bytes(verify_payload_v2(meta, disk)) == want                                   # resident
    assert bytes(verify_payload_v2(meta, disk, budget=budget, stream=True)) == want
    assert bytes(verify_stream_v2(meta, read, budget=budget, threads=2)) == want
    assert bytes(verify_stream_v2(meta, read, chunk=32 * K)) == want
    assert bytes(verify_stream_v2(meta, read, devices=[0, 0, 0], budget=budget)) == want
    root = tmp_path / "dl"
    root.mkdir(parents=True)
    _write(root, paths, disk)
    before = sorted(str(p) for p in root.rglob("*"))
    assert bytes(verify_files_v2(meta, str(root), budget=budget, stream=True, threads=3)) == want
    assert bytes(verify_files_v2(meta, str(root), devices=[0, 0, 0], budget=budget, stream=True)) == want
    assert sorted(str(p) for p in root.rglob("*")) == before             # nothing was created
    with pytest.raises(MemoryError, match="resident"):                   # the default still refuses, and says how
        verify_payload_v2(meta, disk, budget=LEAF // 2)
    return want


@pytest.mark.parametrize("name", sorted(golden()))
def test_golden_layouts_through_the_hosts(native, tmp_path, name):
    g = golden()[name]
    files = list(golden_files(name))
    L = g["piece_length"]
    expected = [bytes.fromhex(h) for h in g["piece_hashes"]]
    assert _hosts(tmp_path, L, files, files, g["lengths"], expected) == bytes.fromhex(g["bitfield"])
    cut = g["truncated"]
    disk = [f[:cut["keep"]] if k == cut["file"] else f for k, f in enumerate(files)]
    assert _hosts(tmp_path / "cut", L, files, disk, g["lengths"], expected) == bytes.fromhex(cut["bitfield"])


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_layouts_through_the_hosts(native, tmp_path, seed):
    d = draw(seed)
    want = _hosts(tmp_path, d.L, d.files, d.disk(), d.lengths, d.expected())
    assert len(want) == (len(d.table) + 7) // 8
    if len(d.table) > 64:
        assert geometry(d.L, len(d.table), window_budget(max(LEAF, d.L // 4)), 0)[1] == 64     # two windows


# ---- files: tv_v2_stream_file_table's readability rule ---------------------------------------------------------------------

def test_files_missing_short_and_unopenable(ctx, native, tmp_path):
    L = 64 * K
    sizes = [3 * L + 100, 2 * L, L, LEAF, 2 * L + L // 2, 0, 5]
    case = Case(L, [rnd(80 + k, n) for k, n in enumerate(sizes)])
    paths = [str(tmp_path / ("f%d.bin" % k)) for k in range(len(sizes))]
    for k, f in enumerate(case.files):
        if k == 1:
            continue                                   # file 1: missing
        if k == 3:
            os.mkdir(paths[k])                         # file 3: a directory in its place
            continue
        keep = len(f) - 1 if k == 2 else len(f) - L if k == 4 else len(f)     # 2: short by a byte; 4: by a piece
        with open(paths[k], "wb") as fh:
            fh.write(f[:keep])
    before = sorted(os.listdir(tmp_path))
    first_piece = [0, 4, 6, 7, 8, 11, 11]
    assert [r[0] for r in case.table] == [0] * 4 + [1] * 2 + [2] + [3] + [4] * 3 + [6]
    clear = {4, 5, 6, 7, 9, 10}        # file 4 keeps its first piece (8); its second is cut at the end, the third gone
    for kw in ({"chunk": 16 * K}, {"budget": window_budget(L)}):
        stream_layout(ctx, native, case, **kw)
        ctx.set_option(native.TV_OPT_OPEN_RW, 0)
        try:
            bits, status = ctx.v2_stream_file_table(case.bytes, case.leaves, case.hashes, case.lengths, paths)
        finally:
            ctx.set_option(native.TV_OPT_OPEN_RW, 1)
        assert bits == set_bits(case.P, clear=clear), kw
        assert status == [0, native.TV_ERR_IO, native.TV_ERR_IO, native.TV_ERR_IO, native.TV_ERR_IO, 0, 0], kw
        assert ctx.last_kernel()[0] == native.KERNEL_V2_STREAM
    assert sorted(os.listdir(tmp_path)) == before and first_piece[4] == 8
    # the files' piece count must be the table's
    stream_layout(ctx, native, case, chunk=16 * K)
    with pytest.raises(native.NativeError) as ei:
        ctx.v2_stream_file_table(case.bytes, case.leaves, case.hashes, case.lengths[:-1], paths[:-1])
    assert ei.value.code == native.TV_ERR_ARG and "pieces" in str(ei.value)


# ---- state and arguments ------------------------------------------------------------------------------------------------------

def test_state_and_arguments(native):
    import hashlib
    L = 64 * K
    case = Case(L, [rnd(90, 2 * L + 300), rnd(91, LEAF + 1)])
    P = case.P
    with native.Context(0) as c:
        def begin(pb=None, tl=None, hs=case.hashes):
            c.v2_stream_begin(case.bytes if pb is None else pb, case.leaves if tl is None else tl, hs)

        def code(fn, *a, **k):
            with pytest.raises(native.NativeError) as ei:
                fn(*a, **k)
            return ei.value.code

        assert code(begin) == native.TV_ERR_STATE                                     # before a layout
        stream_layout(c, native, case, chunk=32 * K)
        # each bad-table case of tv_v2_set_pieces, and a table of another length
        assert code(begin, pb=[0] + case.bytes[1:]) == native.TV_ERR_ARG
        assert code(begin, pb=[L + 1] + case.bytes[1:]) == native.TV_ERR_ARG
        assert code(begin, tl=[3] + case.leaves[1:]) == native.TV_ERR_ARG
        assert code(begin, tl=[2] + case.leaves[1:]) == native.TV_ERR_ARG             # narrower than the piece's leaves
        assert code(begin, tl=[8] + case.leaves[1:]) == native.TV_ERR_ARG             # wider than a piece
        assert code(begin, tl=[0] + case.leaves[1:]) == native.TV_ERR_ARG
        assert code(begin, pb=case.bytes[:-1], tl=case.leaves[:-1], hs=case.hashes[:-32]) == native.TV_ERR_ARG
        lib = native.lib()
        assert lib.tv_v2_stream_begin(c._h, P, None, None, None, None) == native.TV_ERR_ARG
        import numpy as np
        pb, tl = np.asarray(case.bytes, dtype=np.uint32), np.asarray(case.leaves, dtype=np.uint32)
        assert lib.tv_v2_stream_begin(c._h, P, pb.ctypes.data, tl.ctypes.data, None, None) == native.TV_ERR_ARG
        c.set_layout(3 * 48 * K, 48 * K, 3, 0, 3)                                     # not a power of two
        assert code(c.v2_stream_begin, [48 * K] * 3, [2] * 3, bytes(96)) == native.TV_ERR_ARG
        c.set_layout(3 * 8 * K, 8 * K, 3, 0, 3)                                       # below a leaf
        assert code(c.v2_stream_begin, [8 * K] * 3, [1] * 3, bytes(96)) == native.TV_ERR_ARG
        # during a stream: a second begin (v2 or v1) and the resident v2 calls are refused
        stream_layout(c, native, case, chunk=32 * K)
        begin()
        assert code(begin) == native.TV_ERR_STATE
        assert code(c.stream_begin) == native.TV_ERR_STATE
        assert code(c.v2_set_pieces, case.bytes, case.leaves, case.hashes) == native.TV_ERR_STATE
        # tv_stream_end before the last request: aborted, and the ctx is usable again
        req = c.stream_next()
        c.stream_commit(req)
        assert code(c.stream_end) == native.TV_ERR_STATE
        assert code(c.stream_next) == native.TV_ERR_STATE
        begin()
        bits, _ = drive(c, case, case.files, 0, P, chunk=32 * K)
        assert bits == set_bits(P)
        # v2, then v1, then v2 on one ctx without a resident payload, each exact
        v1_payload = rnd(92, 5 * L + 17)
        digests = b"".join(hashlib.sha1(v1_payload[o:o + L]).digest() for o in range(0, len(v1_payload), L))
        c.set_option(native.TV_OPT_STREAM_CHUNK, 0)
        c.set_layout(len(v1_payload), L, 6, 0, 6)
        c.set_digests(digests)
        bad = bytearray(v1_payload)
        bad[2 * L + 5] ^= 1
        c.stream_begin()
        while True:
            req = c.stream_next()
            if not req.rows:
                break
            slot = c.stream_slot(req)
            for q in range(req.rows):
                n = c.row_bytes(req, q)
                o = (req.piece + q) * L + req.offset
                slot[q * req.width:q * req.width + n] = bad[o:o + n]
            slot.release()
            c.stream_commit(req)
        assert c.stream_end() == set_bits(6, clear={2})
        assert c.last_kernel()[0] in (native.KERNEL_LANE, native.KERNEL_SPLIT, native.KERNEL_TWIN)
        staged = [flipped(case.files[0], [L + 1]), case.files[1]]
        stream_layout(c, native, case, budget=window_budget(L))
        begin()
        bits, _ = drive(c, case, staged, 0, P, budget=window_budget(L))
        assert bits == set_bits(P, clear={1})
        assert code(c.v2_set_pieces, case.bytes, case.leaves, case.hashes) == native.TV_ERR_STATE   # no resident payload
        assert code(c.v2_verify) == native.TV_ERR_STATE
        # a resident table set before a v2 stream still verifies after it (and after an aborted one)
        assert run_resident(c, native, case, case.files) == set_bits(P)
        c.set_option(native.TV_OPT_STREAM_CHUNK, 16 * K)
        begin()
        bits, _ = drive(c, case, staged, 0, P, chunk=16 * K)
        assert bits == set_bits(P, clear={1})
        assert c.v2_verify() == set_bits(P)
        begin()
        c.stream_next()
        c.stream_abort()
        assert c.v2_verify() == set_bits(P)
        c.set_option(native.TV_OPT_STREAM_CHUNK, 0)


# ---- resources --------------------------------------------------------------------------------------------------------------

def test_device_memory_is_bounded_and_reused(native):
    """DEVICE_BYTES - 2 x chunk buffer <= 64 B x count + 64 B x wn x ncol + 4 KiB, in columns of one leaf and in
    windows of whole pieces -- tv_set_layout's own per-piece rows (60 B per piece, there on every layout) included; what
    the stream itself adds is 44 B per shard piece of table and at most 48 B per node of a window.  A second stream of
    the same geometry allocates nothing."""
    case, staged, bad = case_130()
    L, count = case.L, case.P
    for kw in ({"chunk": 16 * K}, {"budget": window_budget(L)}):
        with native.Context(0) as c:
            stream_layout(c, native, case, **kw)
            base = c.counter(native.TV_COUNTER_DEVICE_BYTES)      # what the layout itself holds (no payload, no chunks)
            c.v2_stream_begin(case.bytes, case.leaves, case.hashes)
            bits, info = drive(c, case, staged, 0, count, **kw)
            assert bits == set_bits(count, clear=bad)
            chunk_buffer = (info["C"] + 256) * info["wn"] + 256
            held = c.counter(native.TV_COUNTER_DEVICE_BYTES)
            bound = 64 * count + 64 * info["wn"] * info["ncol"] + 4 * K
            print("device bytes", kw, held, "chunk buffers", 2 * chunk_buffer, "layout", base, "bound", bound)
            assert held - base - 2 * chunk_buffer <= 44 * count + 48 * info["wn"] * info["ncol"]    # the stream's own
            assert held - 2 * chunk_buffer <= bound
            allocs = c.counter(native.TV_COUNTER_DEVICE_ALLOCS)
            c.v2_stream_begin(case.bytes, case.leaves, case.hashes)
            bits, _ = drive(c, case, case.files, 0, count, **kw)
            assert bits == set_bits(count)
            assert c.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs
            assert c.counter(native.TV_COUNTER_DEVICE_BYTES) == held
