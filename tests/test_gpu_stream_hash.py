"""Streamed creation on the GPU (tv_stream_hash_begin, tv_v2_stream_hash_begin, tv_hybrid_stream_hash_begin,
tv_stream_hash_end, the three *_hash_file_table calls and the stream=True creation hosts).

Every expected value comes from the CPU -- the oracle's SHA-1 (oracle.hash_pieces), hashlib merkle roots through
tests/v2_ref.py and tests/hybrid_util.py -- and wherever the shard also fits resident the output must be byte-equal to
tv_hash / tv_v2_hash / tv_hybrid_hash over the same bytes.  The creation launches are forms the verify tests never run:
the HASH instantiations of the SHA-1 kernels with blk_begin > 0 (the chaining value read from d_state), finalize in a
window of a larger shard (digests stored at d_hash + j0), the short last piece's own group in column form, and
tv_v2_finish_kernel<true> over a window's column nodes.  The shapes are the smallest that reach each: pieces of one
block, of 16 KiB + 3 blocks and of 48 KiB in columns of one block, 4 KiB and the whole piece; 1, 33, 65 and 257 pieces;
a last piece of 1, 55, 56, 64, L - 1 and L bytes (1 .. 64: it ends in the first column, every later launch only carries
its state)."""
import ctypes
import functools
import hashlib
import json
import os
import random

import pytest

from tests import hybrid_util as hu
from tests import synth
from tests import v1_columns as vc
from tests.hybrid_stream_util import K, window_budget
from tests.hybrid_stream_util import geometry as hybrid_geometry
from tests.v1_columns import VARIANTS
from tests.v2_util import file_names, set_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MARK = 0xA5


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def force(ctx, N, variant=None):
    kernel, pairs, lane_pairs = VARIANTS[variant] if variant else (0, 0, 0)
    ctx.set_option(N.TV_OPT_KERNEL, kernel)
    ctx.set_option(N.TV_OPT_SPLIT_PAIRS, pairs)
    ctx.set_option(N.TV_OPT_LANE_PAIRS, lane_pairs)


def stream_layout(ctx, N, total, L, P, first=0, count=None, chunk=0, budget=0, rows=0):
    ctx.set_option(N.TV_OPT_RESIDENT, 0)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
    ctx.set_option(N.TV_OPT_STREAM_CHUNK, chunk)
    ctx.set_option(N.TV_OPT_STREAM_ROWS, rows)
    try:
        ctx.set_layout(total, L, P, first, P - first if count is None else count)
    finally:
        ctx.set_option(N.TV_OPT_RESIDENT, 1)


# ---- v1 -------------------------------------------------------------------------------------------------------------------

V1_LENGTHS = [64, 16 * K + 64 * 3, 48 * K]
V1_PIECES = [1, 33, 65, 257]


@functools.lru_cache(maxsize=None)
def v1_payload(L: int):
    """257 pieces of L bytes and every full piece's digest (the oracle's); a torrent of P pieces is a prefix."""
    from oracle import oracle as O
    P = max(V1_PIECES)
    data = rnd(L, P * L)
    return data, O.hash_pieces(data, P * L, L, P, threads=4)


def v1_want(L: int, P: int, last: int) -> bytes:
    from oracle import oracle as O
    data, full = v1_payload(L)
    return full[:20 * (P - 1)] + O.sha1(data[(P - 1) * L:(P - 1) * L + last])


def v1_lasts(L: int) -> list:
    return sorted({n for n in (1, 55, 56, 64, L - 1, L) if 1 <= n <= L})


def v1_stream(ctx, data, L, from_src, fill=None):
    """The request loop of an active v1 creation stream -> its requests.  from_src: rows committed from the payload;
    else written into the lent slot, which is first filled with `fill` (bytes past a row's length are then not zeros)."""
    n = 0
    while True:
        req = ctx.stream_next()
        if not req.rows:
            return n
        n += 1
        base = req.piece * L + req.offset
        if from_src:
            ctx.stream_commit_from(req, data, L, base)
            continue
        if fill is not None:
            ctypes.memset(req.slot, fill, req.rows * req.width)
        slot = ctx.stream_slot(req)
        for q in range(req.rows):
            nb = ctx.row_bytes(req, q)
            slot[q * req.width:q * req.width + nb] = data[base + q * L:base + q * L + nb]
        slot.release()
        ctx.stream_commit(req)


def resident_v1(ctx, N, data, total, L, P) -> bytes:
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    ctx.set_layout(total, L, P)
    ctx.stage(0, data[:total])
    return ctx.hash()


@pytest.mark.parametrize("L", V1_LENGTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_v1_every_kernel_form_in_columns(ctx, native, variant, L):
    data, _ = v1_payload(L)
    kernel = VARIANTS[variant][0]
    chunks = sorted({64, min(4 * K, -(-L // 64) * 64), -(-L // 64) * 64})      # many columns, a few, one
    try:
        force(ctx, native, variant)
        for C in chunks:
            units = -(-L // C)
            for P in V1_PIECES:
                for k, last in enumerate(v1_lasts(L)):
                    total = (P - 1) * L + last
                    stream_layout(ctx, native, total, L, P, chunk=C)
                    ctx.stream_hash_begin()
                    # (by turns from the payload and through the lent slot; 257 pieces in one-block columns: the payload)
                    from_src = (k + P) % 2 == 0 or (P > 65 and units > 64)
                    assert v1_stream(ctx, data, L, from_src=from_src, fill=0xFF) == units
                    got = ctx.stream_hash_end()
                    what = (variant, L, C, P, last)
                    assert got == v1_want(L, P, last), what
                    assert ctx.last_kernel() == (kernel, units), what
                    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == vc.workgroups(variant, P, last < L), what
                    assert ctx.counter(native.TV_COUNTER_LAST_STREAM_REQUESTS) == units, what
                    k_ms, total_ms = ctx.last_timing()
                    assert 0 < k_ms <= total_ms
        # byte-equal to tv_hash over the same bytes (the same forced kernel form, one resident launch)
        for P, last in ((65, L), (257, 55 if L > 55 else 1)):
            total = (P - 1) * L + last
            assert resident_v1(ctx, native, data, total, L, P) == v1_want(L, P, last)
    finally:
        force(ctx, native)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_v1_whole_piece_rows_in_windows(ctx, native, variant):
    """TV_OPT_STREAM_ROWS = 1: every row a whole piece.  Under a budget of two buffers of 64 rows a 130-piece shard runs
    in windows of 64, 64 and 2 pieces: each window's launch finalizes, into its own rows of the shard's digests."""
    L = 16 * K + 64 * 3
    data, _ = v1_payload(L)
    kernel = VARIANTS[variant][0]
    pitch = -(-L // 64) * 64 + 256
    try:
        force(ctx, native, variant)
        for budget, windows in ((0, 1), (2 * 64 * pitch, 3)):
            for last in (1, 56, L - 1, L):
                P = 130
                total = (P - 1) * L + last
                stream_layout(ctx, native, total, L, P, rows=1, budget=budget)
                ctx.stream_hash_begin()
                v1_stream(ctx, data, L, from_src=last % 2 == 0, fill=0xFF)
                assert ctx.stream_hash_end() == v1_want(L, P, last), (variant, budget, last)
                assert ctx.last_kernel() == (kernel, windows)
        # a shard in the middle of the torrent, and one holding the short last piece alone
        last = 55
        for P, first, count in ((130, 8, 72), (130, 64, 66), (129, 128, 1)):
            total = (P - 1) * L + last
            stream_layout(ctx, native, total, L, P, first, count, rows=1, budget=2 * 64 * pitch)
            ctx.stream_hash_begin()
            v1_stream(ctx, data, L, from_src=False, fill=0xFF)
            assert ctx.stream_hash_end() == v1_want(L, P, last)[20 * first:20 * (first + count)]
    finally:
        force(ctx, native)
        ctx.set_option(native.TV_OPT_STREAM_ROWS, 0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_v1_windows_of_columns_from_a_file(ctx, native, variant, tmp_path):
    """tv_stream_hash_file_table under a budget of two buffers of 2,048 rows of three blocks: two windows (2,048 and 65
    pieces) of columns, the second one's launches at d_hash + 2,048 with the short last piece's group."""
    C, L = 192, 3 * 192 + 56
    P, last = 2048 + 65, 57
    total = (P - 1) * L + last
    data = rnd(9, total)
    from oracle import oracle as O
    want = O.hash_pieces(data, total, L, P, threads=4)
    path = tmp_path / "one"
    path.write_bytes(data)
    budget = vc.column_budget(C)
    assert vc.stream_geometry(L, P, budget) == (C, 2048)
    try:
        force(ctx, native, variant)
        stream_layout(ctx, native, total, L, P, budget=budget)
        got, status = ctx.stream_hash_file_table([total], [str(path)])
        assert status == [0] and got == want
        assert ctx.last_kernel() == (VARIANTS[variant][0], 2 * -(-L // C))
    finally:
        force(ctx, native)


# ---- v2 and hybrid ----------------------------------------------------------------------------------------------------------

def table_sizes(L: int) -> list:
    return [1, 16384, 0, 16385, L, L + 1, 3 * L - 5]


@functools.lru_cache(maxsize=None)
def table_layout(L: int) -> hu.Layout:
    """Files of 1, 16,384 and 16,385 bytes, L, L + 1 and 3 L - 5 bytes and a zero-length one: one-piece trees narrower
    than a piece, and short last pieces of longer files."""
    return hu.Layout([rnd(300 + k, n) for k, n in enumerate(table_sizes(L))], L)


@functools.lru_cache(maxsize=None)
def layout_two_windows() -> hu.Layout:
    """70 pieces of 64 KiB: under a budget of 64 rows of 16 KiB a stream runs two windows (64 and 6 pieces) of four
    columns, so each window's top tree has two levels over column nodes."""
    L = 64 * K
    ns = [3 * L + 5, 17, 40 * L, 2 * L - 1, 16 * L + 16383, 5, 4 * L + 1]
    lay = hu.Layout([rnd(400 + k, n) for k, n in enumerate(ns)], L)
    assert lay.P == 70
    return lay


def table_stream(ctx, lay, first=0, fill=0xFF, staged=None):
    """The request loop of an active v2 or hybrid creation stream: the slot filled with `fill`, then row q's valid bytes."""
    staged = lay.files if staged is None else staged
    while True:
        req = ctx.stream_next()
        if not req.rows:
            return
        ctypes.memset(req.slot, fill, req.rows * req.width)
        slot = ctx.stream_slot(req)
        for q in range(req.rows):
            f, o, b, w = lay.table[req.piece + q]
            n = ctx.row_bytes(req, q)
            assert n == max(0, min(req.width, b - req.offset))
            if n:
                slot[q * req.width:q * req.width + n] = staged[f][o + req.offset:o + req.offset + n]
        slot.release()
        ctx.stream_commit(req)


def v2_launches(L, count, C, wn) -> int:
    """Per unit the column launch; per window log2(L / C) levels and the finish."""
    ncol = L // C
    return -(-count // wn) * (ncol + ncol.bit_length() - 1 + 1)


def run_v2(ctx, N, lay, first=0, count=None, chunk=0, budget=0, staged=None):
    count = lay.P - first if count is None else count
    stream_layout(ctx, N, lay.total, lay.L, lay.P, first, count, chunk=chunk, budget=budget)
    ctx.v2_stream_hash_begin(lay.pb, lay.tl)
    table_stream(ctx, lay, first, staged=staged)
    return ctx.stream_hash_end()


def resident_v2(ctx, N, lay) -> bytes:
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    ctx.set_layout(lay.total, lay.L, lay.P)
    ctx.v2_set_pieces(lay.pb, lay.tl, None)
    ctx.stage(0, b"\xff" * lay.total)
    ctx.stage_many([(off, d) for off, d in zip(lay.offs, lay.files) if len(d)])
    return ctx.v2_hash()


@pytest.mark.parametrize("L", [16 * K, 64 * K, 256 * K])
def test_v2_file_table_edges(ctx, native, L):
    lay = table_layout(L)
    want = b"".join(lay.hashes)
    for C in sorted({16 * K, max(16 * K, L // 2), L}):
        got = run_v2(ctx, native, lay, chunk=C)
        assert got == want, (L, C)
        assert ctx.last_kernel() == (native.KERNEL_V2_STREAM, v2_launches(L, lay.P, C, lay.P))
    assert resident_v2(ctx, native, lay) == want


def test_v2_two_windows_and_shards(ctx, native):
    lay = layout_two_windows()
    want = b"".join(lay.hashes)
    budget = window_budget(16 * K)
    got = run_v2(ctx, native, lay, budget=budget)
    assert got == want
    assert ctx.last_kernel() == (native.KERNEL_V2_STREAM, v2_launches(lay.L, lay.P, 16 * K, 64))
    for first, count in ((8, 62), (64, 6), (16, 54)):
        assert run_v2(ctx, native, lay, first, count, budget=budget) == want[32 * first:32 * (first + count)]
    assert resident_v2(ctx, native, lay) == want


def dirty_hybrid(ctx, N, L, P, chunk, budget):
    """A creation stream of P full-length all-0xFF pieces under the same geometry: the chunk buffers keep its bytes, so a
    pad range the pad launch missed would hash 0xFF.  Its own outputs are checked too."""
    full = hu.Layout.__new__(hu.Layout)
    full.L, full.P, full.total = L, P, P * L
    full.table = [(0, i * L, L, L // (16 * K)) for i in range(P)]
    full.files = [b"\xff" * (P * L)]
    stream_layout(ctx, N, P * L, L, P, chunk=chunk, budget=budget)
    ctx.hybrid_stream_hash_begin([L] * P, [L // (16 * K)] * P)
    table_stream(ctx, full)
    d, r = ctx.stream_hash_end()
    from tests import v2_ref
    assert d == hashlib.sha1(b"\xff" * L).digest() * P and r == v2_ref.piece_root(b"\xff" * L, L // (16 * K)) * P


def run_hybrid(ctx, N, lay, first=0, count=None, chunk=0, budget=0, pre=True, staged=None):
    count = lay.P - first if count is None else count
    if pre:
        dirty_hybrid(ctx, N, lay.L, lay.P, chunk, budget)
    stream_layout(ctx, N, lay.total, lay.L, lay.P, first, count, chunk=chunk, budget=budget)
    ctx.hybrid_stream_hash_begin(lay.pb, lay.tl)
    table_stream(ctx, lay, first, staged=staged)
    out = ctx.stream_hash_end()
    assert ctx.last_kernel()[0] == N.KERNEL_HYBRID_STREAM
    return out


@pytest.mark.parametrize("L", [16 * K, 64 * K, 256 * K])
def test_hybrid_file_table_edges(ctx, native, L):
    lay = table_layout(L)
    assert lay.tails and lay.pieces == hu.v1_pieces(lay.files, L)          # pads between the files, none after the last
    want = (lay.pieces, b"".join(lay.hashes))
    for C in sorted({16 * K, max(16 * K, L // 2), L}):
        assert run_hybrid(ctx, native, lay, chunk=C) == want, (L, C)
    hu.load(ctx, lay)
    assert ctx.hybrid_hash() == want


@pytest.mark.parametrize("variant", ["lane3", "split1", "twin1"])
def test_hybrid_two_windows_and_the_sha1_forms(ctx, native, variant):
    lay = layout_two_windows()
    want = (lay.pieces, b"".join(lay.hashes))
    budget = window_budget(16 * K, 64)
    assert hybrid_geometry(lay.L, lay.P, budget, 0) == (16 * K, 64)
    try:
        force(ctx, native, variant)
        assert run_hybrid(ctx, native, lay, budget=budget) == want
        first, count = 64, 6
        got = run_hybrid(ctx, native, lay, first, count, budget=budget, pre=False)
        assert got == (want[0][20 * first:20 * (first + count)], want[1][32 * first:32 * (first + count)])
    finally:
        force(ctx, native)


# ---- the file-table calls and the stream=True hosts ----------------------------------------------------------------------

def tree_sizes(L: int) -> list:
    rng = random.Random(41)
    ns = [1, 0, L, L + 1, 3 * L - 5, 16384, 16385, 5 * L + 77, 24 * L + 3, 17 * L]
    ns += [rng.choice([rng.randrange(1, 300), rng.randrange(1, 3 * L)]) for _ in range(30)]
    return ns


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """40 files, about 5 MiB, pieces of 64 KiB: (directory, [(path components, length)], the files' bytes)."""
    L = 64 * K
    root = tmp_path_factory.mktemp("creation_tree") / "payload"
    ns = tree_sizes(L)
    assert len(ns) == 40 and sum(ns) < 8 << 20
    names = sorted(file_names(len(ns)), key=lambda comps: [os.fsencode(c) for c in comps])   # file-tree order
    files = [rnd(500 + k, n) for k, n in enumerate(ns)]
    for comps, data in zip(names, files):
        p = root.joinpath(*comps)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)
    return str(root), [(list(c), n) for c, n in zip(names, ns)], files


def test_stream_true_hosts_equal_the_resident_hosts(native, tree):
    from torrent_amd import (FileInfo, hash_files, hash_files_hybrid, hash_files_v2, hash_pieces, hash_stream,
                             hash_stream_hybrid, hash_stream_v2, make_info)
    root, listed, files = tree
    L = 64 * K
    lay = hu.Layout(files, L)
    small = window_budget(16 * K)                                           # 64 rows of 16 KiB: far below the payload
    assert small < sum(n for _, n in listed) // 2
    with pytest.raises(MemoryError):                                        # (resident creation does not fit it)
        hash_files_v2(root, L, files=listed, budget=small)
    # v1: the files back to back
    lin = b"".join(files)
    info = make_info(L, bytes(20 * -(-len(lin) // L)), "payload", files=[FileInfo(length=n, path=c) for c, n in listed])
    from oracle import oracle as O
    want1 = O.hash_pieces(lin, len(lin), L, -(-len(lin) // L), threads=4)
    assert hash_files(info, root) == want1
    assert hash_files(info, root, stream=True) == want1
    assert hash_files(info, root, stream=True, budget=1 << 20, devices=[0, 0, 0]) == want1
    assert hash_pieces(lin, L, stream=True) == want1 == hash_pieces(lin, L)
    assert hash_pieces(lin, L, stream=True, budget=1 << 20, devices=[0, 0]) == want1
    assert hash_stream(len(lin), L, lambda off, n: lin[off:off + n], threads=2) == want1
    assert hash_stream(len(lin), L, lambda off, n: lin[off:off + n], chunk=4096, devices=[0, 0]) == want1
    # v2 and hybrid: the resident hosts at the default budget, the streamed ones under the small one
    res2 = hash_files_v2(root, L, files=listed)
    str2 = hash_files_v2(root, L, files=listed, stream=True, budget=small)
    assert [(f.path, f.length, f.pieces_root, f.layer) for f in res2] == \
           [(f.path, f.length, f.pieces_root, f.layer) for f in str2]
    read = lambda k, off, n: files[k][off:off + n]                         # noqa: E731
    assert hash_stream_v2([n for _, n in listed], L, read, budget=small, devices=[0, 0]) == b"".join(lay.hashes)
    p_res, f_res = hash_files_hybrid(root, L, files=listed)
    p_str, f_str = hash_files_hybrid(root, L, files=listed, stream=True, budget=small, devices=[0, 0])
    assert p_res == p_str == lay.pieces
    assert [(f.pieces_root, f.layer) for f in f_res] == [(f.pieces_root, f.layer) for f in f_str]
    assert hash_stream_hybrid([n for _, n in listed], L, read, budget=small, threads=2) == (lay.pieces, b"".join(lay.hashes))


def test_make_torrent_stream_true_is_byte_identical(native, tree):
    from torrent_amd import make_torrent, make_torrent_hybrid, make_torrent_v2
    root, listed, files = tree
    L = 64 * K
    small = window_budget(16 * K)
    kw = {"comment": "c", "creation_date": 1700000000, "piece_length": L}
    assert make_torrent(root, "http://t/a", **kw) == make_torrent(root, "http://t/a", stream=True, budget=small, **kw)
    assert make_torrent_v2(root, "http://t/a", **kw) == make_torrent_v2(root, "http://t/a", stream=True, budget=small, **kw)
    assert make_torrent_hybrid(root, "http://t/a", **kw) == \
        make_torrent_hybrid(root, "http://t/a", stream=True, budget=small, **kw)
    one = os.path.join(root, *listed[-1][0])                                # a single file
    for make in (make_torrent, make_torrent_v2, make_torrent_hybrid):
        assert make(one, "http://t/a", **kw) == make(one, "http://t/a", stream=True, budget=small, **kw)


@pytest.mark.parametrize("name", ["singlefile", "multifile"])
def test_make_torrent_stream_reproduces_the_reference_fixtures(native, tmp_path, name):
    """make_torrent(stream=True) on the reconstructed payloads of the reference's own test_data: its .torrent files byte
    for byte (every digest through the creation stream, under a budget a tenth of the payload)."""
    from torrent_amd import make_torrent, parse_metainfo
    ref = open(os.path.join(GOLDEN, f"{name}.torrent"), "rb").read()
    meta = parse_metainfo(ref)
    rd = json.load(open(os.path.join(GOLDEN, "refdata.json")))[name]
    p = tmp_path / (rd["files"][0]["path"] if name == "singlefile" else "multifile")
    for f in rd["files"]:
        q = p if name == "singlefile" else p.joinpath(*f["path"].split("/"))
        q.parent.mkdir(parents=True, exist_ok=True)
        q.write_bytes(f["pattern"].encode() * (f["length"] // len(f["pattern"])))
    out = make_torrent(str(p), meta.announce, comment=meta.comment, creation_date=meta.creation_date,
                       files=None if name == "singlefile" else meta.info.files, stream=True, budget=48 << 20)
    assert out == ref


def file_table_calls(ctx, N, lay, listed_paths, budget):
    """The three *_hash_file_table calls over the same files -> (v1 digests over the files back to back, v2 roots,
    (hybrid digests, hybrid roots)), each with its statuses."""
    lengths = lay.lengths
    lin = sum(lengths)
    stream_layout(ctx, N, lin, lay.L, -(-lin // lay.L), budget=budget)
    a = ctx.stream_hash_file_table(lengths, listed_paths)
    stream_layout(ctx, N, lay.total, lay.L, lay.P, budget=budget)
    b = ctx.v2_stream_hash_file_table(lay.pb, lay.tl, lengths, listed_paths)
    c = ctx.hybrid_stream_hash_file_table(lay.pb, lay.tl, lengths, listed_paths)
    return a, b, c


def test_file_table_calls(ctx, native, tree):
    root, listed, files = tree
    L = 64 * K
    lay = hu.Layout(files, L)
    paths = [os.path.join(root, *c) for c, _ in listed]
    lin = b"".join(files)
    from oracle import oracle as O
    want1 = O.hash_pieces(lin, len(lin), L, -(-len(lin) // L), threads=4)
    ctx.set_option(native.TV_OPT_OPEN_RW, 1)                                # creation opens read-only whatever this says
    for p in paths:
        os.chmod(p, 0o444)
    try:
        for budget in (0, window_budget(16 * K)):
            a, b, c = file_table_calls(ctx, native, lay, paths, budget)
            assert a == (want1, [0] * 40)
            assert b == (b"".join(lay.hashes), [0] * 40)
            assert c == ((lay.pieces, b"".join(lay.hashes)), [0] * 40)
    finally:
        for p in paths:
            os.chmod(p, 0o644)


def test_a_truncated_file_is_an_io_error_and_writes_nothing(ctx, native, tree, tmp_path):
    import shutil
    root, listed, files = tree
    L = 64 * K
    lay = hu.Layout(files, L)
    copy = tmp_path / "copy"
    shutil.copytree(root, copy)
    paths = [str(copy.joinpath(*c)) for c, _ in listed]
    k = 4                                                                   # the 3 L - 5 file, one byte short on disk
    assert lay.lengths[k] == 3 * L - 5
    with open(paths[k], "r+b") as f:
        f.truncate(lay.lengths[k] - 1)
    lib = native.lib()
    n, ln, blob, st = native._file_table("t", lay.lengths, paths)
    pb, tl = native._v2_arrays("t", lay.pb, lay.tl)
    lin = sum(lay.lengths)
    d = ctypes.create_string_buffer(bytes([MARK]) * (20 * lay.P), 20 * lay.P)
    r = ctypes.create_string_buffer(bytes([MARK]) * (32 * lay.P), 32 * lay.P)
    untouched = lambda buf: buf.raw == bytes([MARK]) * len(buf)             # noqa: E731
    want_status = [native.TV_ERR_IO if q == k else 0 for q in range(n)]
    for kind in ("v1", "v2", "hybrid"):
        st[:] = 7
        if kind == "v1":
            stream_layout(ctx, native, lin, L, -(-lin // L))
            rc = lib.tv_stream_hash_file_table(ctx._h, n, ln.ctypes.data, blob, len(blob), d, st.ctypes.data)
        elif kind == "v2":
            stream_layout(ctx, native, lay.total, L, lay.P)
            rc = lib.tv_v2_stream_hash_file_table(ctx._h, len(pb), pb.ctypes.data, tl.ctypes.data, n, ln.ctypes.data, blob,
                                                  len(blob), r, st.ctypes.data)
        else:
            stream_layout(ctx, native, lay.total, L, lay.P)
            rc = lib.tv_hybrid_stream_hash_file_table(ctx._h, len(pb), pb.ctypes.data, tl.ctypes.data, n, ln.ctypes.data,
                                                      blob, len(blob), d, r, st.ctypes.data)
        assert rc == native.TV_ERR_IO, kind
        assert st.tolist() == want_status, kind
        assert untouched(d) and untouched(r), kind
        # the stream was aborted and the ctx starts a new one
        ctx.v2_stream_hash_begin(lay.pb, lay.tl) if kind != "v1" else ctx.stream_hash_begin()
        ctx.stream_abort()
    # the hosts raise, with hash_files' message
    from torrent_amd import FileInfo, hash_files, hash_files_hybrid, hash_files_v2, make_info
    info = make_info(L, bytes(20 * -(-lin // L)), "copy", files=[FileInfo(length=n_, path=c) for c, n_ in listed])
    with pytest.raises(FileNotFoundError, match="hash_files: a file is missing or shorter than its declared length"):
        hash_files(info, str(copy), stream=True)
    with pytest.raises(FileNotFoundError, match="hash_files_v2: a file is missing or shorter"):
        hash_files_v2(str(copy), L, files=listed, stream=True)
    os.remove(paths[k])
    with pytest.raises(FileNotFoundError, match="hash_files_hybrid: a file is missing or shorter"):
        hash_files_hybrid(str(copy), L, files=listed, stream=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def verify_stream_bits(ctx, N, lay, kind):
    """A verify stream of `kind` over the layout's bytes on the same ctx -> the bitfield(s) it returns."""
    if kind == "v1":
        lin = b"".join(lay.files)
        P = -(-len(lin) // lay.L)
        stream_layout(ctx, N, len(lin), lay.L, P, chunk=4096)
        ctx.set_digests(b"".join(hashlib.sha1(lin[o:o + lay.L]).digest() for o in range(0, len(lin), lay.L)))
        ctx.stream_begin()
        v1_stream(ctx, lin, lay.L, from_src=True)
        return ctx.stream_end(), set_bits(P)
    stream_layout(ctx, N, lay.total, lay.L, lay.P, chunk=16 * K)
    if kind == "v2":
        ctx.v2_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes))
        table_stream(ctx, lay)
        return ctx.stream_end(), set_bits(lay.P)
    ctx.set_digests(lay.pieces)
    ctx.hybrid_stream_begin(lay.pb, lay.tl, b"".join(lay.hashes))
    table_stream(ctx, lay)
    return ctx.hybrid_stream_end(), (set_bits(lay.P),) * 3


def begin(ctx, N, lay, kind, hash_mode=True):
    if kind == "v1":
        lin = sum(lay.lengths)
        stream_layout(ctx, N, lin, lay.L, -(-lin // lay.L), chunk=4096)
        if hash_mode:
            return ctx.stream_hash_begin()
        ctx.set_digests(bytes(20 * -(-lin // lay.L)))
        return ctx.stream_begin()
    stream_layout(ctx, N, lay.total, lay.L, lay.P, chunk=16 * K)
    if hash_mode:
        return ctx.v2_stream_hash_begin(lay.pb, lay.tl) if kind == "v2" else ctx.hybrid_stream_hash_begin(lay.pb, lay.tl)
    if kind == "hybrid":
        ctx.set_digests(lay.pieces)
    fn = ctx.v2_stream_begin if kind == "v2" else ctx.hybrid_stream_begin
    return fn(lay.pb, lay.tl, b"".join(lay.hashes))


def feed(ctx, lay, kind):
    if kind == "v1":
        v1_stream(ctx, b"".join(lay.files), lay.L, from_src=True)
    else:
        table_stream(ctx, lay)


@pytest.mark.parametrize("kind", ["v1", "v2", "hybrid"])
def test_refusals(ctx, native, kind):
    lay = table_layout(64 * K)
    lib = native.lib()
    N = native
    nd, nr = 20 * (lay.P + 8), 32 * lay.P
    d = ctypes.create_string_buffer(bytes([MARK]) * nd, nd)
    r = ctypes.create_string_buffer(bytes([MARK]) * nr, nr)
    bits = ctypes.create_string_buffer(bytes([MARK]) * 16, 16)
    clean = lambda: d.raw == bytes([MARK]) * nd and r.raw == bytes([MARK]) * nr and bits.raw == bytes([MARK]) * 16  # noqa: E731

    def refused(rc, code, active_after):
        assert rc == code and clean()
        # what the ctx says about a stream now: tv_stream_abort always succeeds, tv_stream_next tells
        req = N.StreamReq()
        rc2 = lib.tv_stream_next(ctx._h, ctypes.byref(req))
        assert (rc2 != N.TV_ERR_STATE) == active_after
        ctx.stream_abort()
        got, want = verify_stream_bits(ctx, N, lay, kind)
        assert got == want

    # tv_stream_unreadable on a creation stream: refused, the stream stays active
    begin(ctx, N, lay, kind)
    refused(lib.tv_stream_unreadable(ctx._h, 0), N.TV_ERR_STATE, True)
    # tv_stream_end / tv_hybrid_stream_end on a creation stream: refused and aborted
    begin(ctx, N, lay, kind)
    feed(ctx, lay, kind)
    refused(lib.tv_stream_end(ctx._h, bits), N.TV_ERR_STATE, False)
    begin(ctx, N, lay, kind)
    feed(ctx, lay, kind)
    refused(lib.tv_hybrid_stream_end(ctx._h, bits, bits, bits), N.TV_ERR_STATE, False)
    # tv_stream_hash_end on a verify stream: refused and aborted
    begin(ctx, N, lay, kind, hash_mode=False)
    feed(ctx, lay, kind)
    refused(lib.tv_stream_hash_end(ctx._h, d, r), N.TV_ERR_STATE, False)
    # ... and with no stream at all
    refused(lib.tv_stream_hash_end(ctx._h, d, r), N.TV_ERR_STATE, False)
    # ending before the last column
    begin(ctx, N, lay, kind)
    refused(lib.tv_stream_hash_end(ctx._h, d, r), N.TV_ERR_STATE, False)
    # a required pointer that is NULL
    for dd, rr in {"v1": [(None, r)], "v2": [(d, None)], "hybrid": [(None, r), (d, None)]}[kind]:
        begin(ctx, N, lay, kind)
        feed(ctx, lay, kind)
        refused(lib.tv_stream_hash_end(ctx._h, dd, rr), N.TV_ERR_ARG, False)
    # the pointer a kind does not write may be NULL
    begin(ctx, N, lay, kind)
    feed(ctx, lay, kind)
    assert lib.tv_stream_hash_end(ctx._h, d if kind != "v2" else None, r if kind != "v1" else None) == 0
    # a creation stream needs no digests: a fresh context, nothing set but the layout
    with N.Context(0) as fresh:
        begin(fresh, N, lay, kind)
        feed(fresh, lay, kind)
        out = fresh.stream_hash_end()
        lin = b"".join(lay.files)
        want1 = b"".join(hashlib.sha1(lin[o:o + lay.L]).digest() for o in range(0, len(lin), lay.L))
        assert out == {"v1": want1, "v2": b"".join(lay.hashes), "hybrid": (lay.pieces, b"".join(lay.hashes))}[kind]


# ---- round trip ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["v1", "v2", "hybrid"])
def test_round_trip_through_the_verify_streams(ctx, native, kind):
    """The hashes a creation stream produced, fed to the verify stream of its kind over the same bytes: all ones; after
    one flipped byte: exactly one zero bit."""
    N = native
    lay = table_layout(64 * K)
    begin(ctx, N, lay, kind)
    feed(ctx, lay, kind)
    made = ctx.stream_hash_end()
    k, pos = 6, 2 * lay.L + 9                                               # the 3 L - 5 file's third piece
    staged = list(lay.files)
    staged[k] = hu.xor_at(staged[k], pos, 0x10)
    for files, clear in ((lay.files, ()), (staged, None)):
        if kind == "v1":
            lin = b"".join(files)
            P = -(-len(lin) // lay.L)
            stream_layout(ctx, N, len(lin), lay.L, P, chunk=4096)
            ctx.set_digests(made)
            ctx.stream_begin()
            v1_stream(ctx, lin, lay.L, from_src=False, fill=0xFF)
            bad = (sum(lay.lengths[:k]) + pos) // lay.L
            assert ctx.stream_end() == set_bits(P, clear=() if clear == () else {bad})
            continue
        bad = lay.first_piece(k) + 2
        want = set_bits(lay.P, clear=() if clear == () else {bad})
        stream_layout(ctx, N, lay.total, lay.L, lay.P, chunk=16 * K)
        if kind == "v2":
            ctx.v2_stream_begin(lay.pb, lay.tl, made)
            table_stream(ctx, lay, staged=files)
            assert ctx.stream_end() == want
        else:
            ctx.set_digests(made[0])
            ctx.hybrid_stream_begin(lay.pb, lay.tl, made[1])
            table_stream(ctx, lay, staged=files)
            assert ctx.hybrid_stream_end() == (want,) * 3
