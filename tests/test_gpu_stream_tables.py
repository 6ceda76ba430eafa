"""The host side of the stream engine (torrent_amd/csrc/tv_stream.hip) on the layouts of tests/stream_tables.py, every
bitfield and per-file status compared with references only (Storage(fs_storage).get + hashlib; tests/v2_ref.py;
tests/hybrid_util.Layout.verdicts plus the header's readability rule):

  - file tables of more than 256 files (FdCache keeps the first 256 descriptors; every later file is opened and closed
    around each read), v1, v2 and hybrid, with a missing, a short, a directory-shadowed and an unwritable file and
    flipped bytes on both sides of position 256; the process's descriptor count and the directory tree are the same
    before and after every call;
  - units of more than one request on v2 and hybrid streams (4,096 + 70 rows: the second request lands at row 4096 of
    the chunk buffer), driven request by request over chunk buffers a stream of 0xFF pieces dirtied first, and through
    the file tables; TV_COUNTER_LAST_STREAM_REQUESTS holds the number of requests to the restated geometry;
  - TV_OPT_STREAM_COLD_REQ on evicted files (tools/fsutil.py), v1, v2 and hybrid, with O_DIRECT on and refused, held to
    the request counter (off: no shard is judged cold, the requests stay one slot long); TV_OPT_STREAM_COLD_READERS is
    set there too, but it has no observable effect to assert;
  - the stream=True hosts over the same trees, on one shard and on two.

Not covered: FdCache's EMFILE / ENFILE rule (out of descriptors is not the file's failure).  Reaching it means
lowering RLIMIT_NOFILE in a process that holds the GPU, which these tests do not do.  And the unwritable file is
refused under TV_OPT_OPEN_RW = 1 only where this process may not write it (stream_tables.blocked_here): run as root,
both values of the option expect the same bits and statuses and that branch is not reached (the CPU pins model it by
treating the file as missing).

A 104-piece v1 shard is one window under any budget (tv_plan.h stream_geometry: windows of at least 2,048 pieces), so
its two windows come from whole-piece rows (TV_OPT_STREAM_ROWS) under a budget of 64 rows."""
import contextlib
import errno
import functools
import os
import sys

import pytest

from tests import hybrid_stream_util as hsu
from tests import hybrid_util as hu
from tests import stream_tables as T
from tests.test_gpu_hybrid_stream import dirty
from tests.test_gpu_hybrid_stream import drive as hybrid_drive
from tests.test_gpu_hybrid_stream import stream_layout as hybrid_layout
from tests.test_gpu_v2_stream import drive as v2_drive
from tests.test_gpu_v2_stream import geometry as v2_geometry
from tests.test_gpu_v2_stream import stream_layout as v2_layout
from tests.test_gpu_v2_stream import window_budget as v2_window_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
K, M = T.K, T.M


def fds() -> int:
    return len(os.listdir("/proc/self/fd"))


@contextlib.contextmanager
def unchanged(root: str):
    """The process's open descriptors and the directory tree are the same after the block as before it."""
    tree, n = T.tree_listing(root), fds()
    yield
    assert fds() == n
    assert T.tree_listing(root) == tree


def requests(ctx, N) -> int:
    return ctx.counter(N.TV_COUNTER_LAST_STREAM_REQUESTS)


def hashes(lay) -> bytes:
    return b"".join(lay.hashes)


# ---- the trees, written once ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def v1_tree(tmp_path_factory):
    """C1 on disk, and its expected bits from Storage(fs_storage).get + hashlib over a copy: with the unwritable files
    still writable (what read-only opens see, TV_OPT_OPEN_RW = 0) and after their chmod (read + write opens)."""
    v = T.v1_table()
    base = tmp_path_factory.mktemp("many_v1")
    root, ref = str(base / "dl"), str(base / "ref")
    full = T.write_tree(root, v.paths, v.files, v.faults)
    ref_full = T.write_tree(ref, v.paths, v.files, v.faults, chmod=False)
    want_ro = v.expected_from_tree(ref)
    T.make_readonly(ref_full, v.faults)
    want_rw = v.expected_from_tree(ref)
    blocked = T.blocked_here(full, v.faults)
    assert want_ro == v.expected_model(False) and want_rw == v.expected_model(blocked)
    return {"v": v, "root": root, "full": full, "want": {0: want_ro, 1: want_rw}, "blocked": blocked}


def _aligned_tree(tmp_path_factory, name, a):
    root = str(tmp_path_factory.mktemp(name) / "dl")
    full = T.write_tree(root, a.paths, a.files, a.faults)
    return {"a": a, "root": root, "full": full, "blocked": T.blocked_here(full, a.faults)}


@pytest.fixture(scope="module")
def many_tree(tmp_path_factory):
    return _aligned_tree(tmp_path_factory, "many", T.many())


@pytest.fixture(scope="module")
def tall_tree(tmp_path_factory):
    return _aligned_tree(tmp_path_factory, "tall", T.tall())


@pytest.fixture(scope="module")
def cold_tree(tmp_path_factory):
    """C6 on disk; the v1 bits of the same files back to back from Storage(fs_storage).get + hashlib over a copy."""
    tree = _aligned_tree(tmp_path_factory, "cold", T.cold())
    v = T.cold_v1()
    ref = str(tmp_path_factory.mktemp("cold_ref") / "ref")
    T.write_tree(ref, v.paths, v.files, v.faults)
    tree["want_v1"] = v.expected_from_tree(ref)
    assert tree["want_v1"] == v.expected_model(False)
    return tree


@functools.lru_cache(maxsize=None)
def many_want(kind: str, trailing: bool, blocked: bool):
    a = T.many()
    return a.expected_v2(blocked) if kind == "v2" else a.expected_hybrid(blocked, trailing)


@functools.lru_cache(maxsize=None)
def tall_want(kind: str):
    t = T.tall()
    return t.expected_v2(False) if kind == "v2" else t.expected_hybrid(False, True)


# ---- C1 / C3: many files, v1 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("open_rw", [1, 0])
@pytest.mark.parametrize("threads", [1, 8])
def test_many_files_v1(native, v1_tree, threads, open_rw):
    N, v = native, v1_tree["v"]
    want = v1_tree["want"][open_rw]
    status = T.expected_status(v.lengths, v.faults, bool(open_rw) and v1_tree["blocked"])
    col_budget = 2 * (v.P * (8192 + 256) + 256)
    # (chunk, budget, whole-piece rows) -> windows x columns
    geoms = [((4096, 0, 0), 1 * 4),
             ((0, col_budget, 0), 1 * (v.L // T.v1_budget_geometry(v.L, v.P, col_budget)[0])),
             ((0, T.v1_rows_budget(v.L), 1), -(-v.P // T.v1_row_window(v.L, v.P, T.v1_rows_budget(v.L))) * 1)]
    assert [n for _, n in geoms] == [4, 2, 2]
    with N.Context(0) as ctx:
        ctx.set_option(N.TV_OPT_FILE_THREADS, threads)
        ctx.set_option(N.TV_OPT_OPEN_RW, open_rw)
        for k, ((chunk, budget, rows), launches) in enumerate(geoms):
            ctx.set_option(N.TV_OPT_RESIDENT, 0)
            ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
            ctx.set_option(N.TV_OPT_STREAM_CHUNK, chunk)
            ctx.set_option(N.TV_OPT_STREAM_ROWS, rows)
            ctx.set_layout(v.total, v.L, v.P)
            ctx.set_digests(v.digests)
            if k == 0:
                ctx.stream_file_table(v.lengths, v1_tree["full"])        # (the runtime may open descriptors lazily)
            with unchanged(v1_tree["root"]):
                bits, st = ctx.stream_file_table(v.lengths, v1_tree["full"])
            assert bits == want, (chunk, budget, rows)
            assert st == status, (chunk, budget, rows)
            assert ctx.last_kernel()[1] == launches                      # windows x columns
            assert requests(ctx, N) == launches                          # (one request per unit: the rows fit a slot)


# ---- C2 / C3: many files, v2 and hybrid ----------------------------------------------------------------------------------------

KINDS = [("v2", False), ("hybrid", False), ("hybrid", True)]


def aligned_call(ctx, N, kind, lay, lengths, full, chunk, budget, pieces=None):
    """Layout, then the kind's file-table call -> (call, kernel id, launches, requests) under the restated geometry."""
    P, L = lay.P, lay.L
    if kind == "v2":
        C, wn = v2_geometry(L, P, budget, chunk)
        v2_layout(ctx, N, lay, chunk=chunk, budget=budget)
        call = lambda: ctx.v2_stream_file_table(lay.pb, lay.tl, hashes(lay), lengths, full)       # noqa: E731
        kernel, launches = N.KERNEL_V2_STREAM, T.v2_launches(P, C, wn, L)
    else:
        C, wn = hsu.geometry(L, P, budget, chunk)
        hybrid_layout(ctx, N, lay, 0, P, chunk, budget, pieces)
        call = lambda: ctx.hybrid_stream_file_table(lay.pb, lay.tl, hashes(lay), lengths, full)   # noqa: E731
        kernel, launches = N.KERNEL_HYBRID_STREAM, hsu.launches(lay.pb, lay.v1_len, L, 0, P, C, wn)
    return call, kernel, launches, len(T.request_plan(0, P, C, wn, L))


def resident_bits(ctx, N, kind, lay, staged, avail):
    """tv_v2_verify / tv_hybrid_verify on the same bytes, the unreadable pieces given as availability."""
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    hu.load(ctx, lay, staged=staged)
    return ctx.v2_verify(avail) if kind == "v2" else ctx.hybrid_verify(avail)


@pytest.mark.parametrize("open_rw", [1, 0])
@pytest.mark.parametrize("kind,trailing", KINDS)
def test_many_files_aligned(native, many_tree, kind, trailing, open_rw):
    N, a = native, many_tree["a"]
    lay = a.lay(trailing)
    blocked = bool(open_rw) and many_tree["blocked"]
    want = many_want(kind, trailing, blocked)
    status = T.expected_status(a.lengths, a.faults, blocked)
    budget = v2_window_budget(16 * K) if kind == "v2" else hsu.window_budget(16 * K, a.P)      # seven / two windows
    with N.Context(0) as ctx:
        ctx.set_option(N.TV_OPT_OPEN_RW, open_rw)
        for k, (chunk, bud) in enumerate(((16 * K, 0), (0, budget))):
            call, kernel, launches, reqs = aligned_call(ctx, N, kind, lay, a.lengths, many_tree["full"], chunk, bud)
            if k == 0:
                call()
            with unchanged(many_tree["root"]):
                got, st = call()
            assert got == want, (chunk, bud)
            assert st == status, (chunk, bud)
            assert ctx.last_kernel() == (kernel, launches)
            assert requests(ctx, N) == reqs
        assert resident_bits(ctx, N, kind, lay, a.staged(), a.readable_bits(blocked)) == want


# ---- C4: the hosts ----------------------------------------------------------------------------------------------------------------

def test_hosts_v1(native, v1_tree):
    from torrent_amd import verify_files
    v, root = v1_tree["v"], v1_tree["root"]
    info, want = v.info(), v1_tree["want"][1]                 # (verify_files opens as fsStorage.get does: read + write)
    tree = T.tree_listing(root)
    assert bytes(verify_files(info, root, stream=False)) == want
    assert bytes(verify_files(info, root, stream=True)) == want
    assert bytes(verify_files(info, root, devices=[0, 0], stream=True, threads=3)) == want
    assert bytes(verify_files(info, root, budget=2 * (v.P * (4096 + 256) + 256), stream=True)) == want
    assert T.tree_listing(root) == tree


def test_hosts_v2(native, many_tree):
    from torrent_amd import parse_metainfo_v2, verify_files_v2
    from tests.v2_util import torrent_v2
    a, root = many_tree["a"], many_tree["root"]
    meta = parse_metainfo_v2(torrent_v2(a.files, a.L, name="many", paths=a.paths))
    assert meta is not None and meta.layout.hashes == hashes(a.lay())
    want = many_want("v2", False, False)                      # (the v2 hosts open read-only)
    tree = T.tree_listing(root)
    assert bytes(verify_files_v2(meta, root)) == want
    assert bytes(verify_files_v2(meta, root, budget=v2_window_budget(16 * K), stream=True)) == want
    assert bytes(verify_files_v2(meta, root, devices=[0, 0], stream=True, threads=3)) == want
    assert T.tree_listing(root) == tree


@pytest.mark.parametrize("trailing", [False, True])
def test_hosts_hybrid(native, many_tree, trailing):
    from torrent_amd import parse_metainfo_hybrid, verify_files_hybrid
    a, root = many_tree["a"], many_tree["root"]
    lay = a.lay(trailing)
    pieces = hu.xor_at(lay.pieces, 20 * 5 + 3, 2)             # the torrent states piece 5's v1 digest wrongly
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(a.files, a.L, name="many", paths=a.paths, trailing_pad=trailing,
                                                   pieces=pieces))
    assert meta is not None and meta.total_length == lay.total
    want = a.expected_hybrid(False, trailing, pieces=pieces)
    tree = T.tree_listing(root)
    r = verify_files_hybrid(meta, root)
    assert (bytes(r.bitfield), bytes(r.v1), bytes(r.v2)) == want and r.disagree == [5]
    for kw in ({"budget": hsu.window_budget(16 * K, a.P)}, {"devices": [0, 0], "threads": 3}):
        r = verify_files_hybrid(meta, root, stream=True, **kw)
        assert (bytes(r.bitfield), bytes(r.v1), bytes(r.v2)) == want, kw
        assert r.disagree == [5]
    assert T.tree_listing(root) == tree


# ---- C5: tall units ------------------------------------------------------------------------------------------------------------------

def tall_geometry(shape: str) -> tuple:
    """(chunk, budget): 16 KiB columns across the shard, or windows of 2,112 whole pieces (the last one 2,054)."""
    return (16 * K, 0) if shape == "columns" else (0, v2_window_budget(T.TALL_L, T.TALL_WINDOW))


@pytest.mark.parametrize("shape", ["columns", "windows"])
@pytest.mark.parametrize("kind", ["v2", "hybrid"])
def test_tall_units_driven(native, kind, shape):
    """Every unit is two requests; the second one's rows start at row 4096 (columns) / 2048 (windows) of the chunk
    buffer, which a stream of 0xFF pieces has filled before."""
    N, t = native, T.tall()
    lay = t.lay(kind == "hybrid")
    L, P = lay.L, lay.P
    chunk, budget = tall_geometry(shape)
    C, wn = (v2_geometry if kind == "v2" else hsu.geometry)(L, P, budget, chunk)
    plan = T.request_plan(0, P, C, wn, L)
    assert len(plan) == 4 and set(T.requests_per_unit(P, C, wn)) == {2}
    staged, want = t.staged(), tall_want(kind)
    with N.Context(0) as ctx:
        assert requests(ctx, N) == 0                                       # before any stream
        dirty(ctx, N, L, P, chunk, budget)
        assert requests(ctx, N) == 4
        if kind == "v2":
            v2_layout(ctx, N, lay, chunk=chunk, budget=budget)
            ctx.v2_stream_begin(lay.pb, lay.tl, hashes(lay))
            got, info = v2_drive(ctx, lay, staged, 0, P, chunk, budget, filler=0xFF)
            assert ctx.last_kernel() == (N.KERNEL_V2_STREAM, T.v2_launches(P, C, wn, L))
        else:
            hybrid_layout(ctx, N, lay, 0, P, chunk, budget)
            ctx.hybrid_stream_begin(lay.pb, lay.tl, hashes(lay))
            info = hybrid_drive(ctx, lay, staged, 0, P, chunk, budget)
            got = ctx.hybrid_stream_end()
            assert ctx.last_kernel() == (N.KERNEL_HYBRID_STREAM, hsu.launches(lay.pb, lay.v1_len, L, 0, P, C, wn))
        assert (info["C"], info["wn"]) == (C, wn)
        assert got == want
        assert requests(ctx, N) == len(plan)
        # a stream that is aborted, and one ended early (aborted by the library), leave the counter alone
        begin = ctx.v2_stream_begin if kind == "v2" else ctx.hybrid_stream_begin
        begin(lay.pb, lay.tl, hashes(lay))
        ctx.stream_next()
        ctx.stream_abort()
        assert requests(ctx, N) == len(plan)
        begin(lay.pb, lay.tl, hashes(lay))
        ctx.stream_commit(ctx.stream_next())
        with pytest.raises(N.NativeError):
            ctx.stream_end()
        assert requests(ctx, N) == len(plan)


@pytest.mark.parametrize("shape", ["columns", "windows"])
@pytest.mark.parametrize("kind", ["v2", "hybrid"])
def test_tall_units_file_table(native, tall_tree, kind, shape):
    N, t = native, tall_tree["a"]
    lay = t.lay(kind == "hybrid")
    chunk, budget = tall_geometry(shape)
    with N.Context(0) as ctx:
        call, kernel, launches, reqs = aligned_call(ctx, N, kind, lay, t.lengths, tall_tree["full"], chunk, budget)
        assert reqs == 4
        got, st = call()
        assert got == tall_want(kind)
        assert st == [N.TV_OK] * t.n
        assert ctx.last_kernel() == (kernel, launches)
        assert requests(ctx, N) == reqs


# ---- C6: cold shards, small requests ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odirect", [1, 0, 2])
@pytest.mark.parametrize("kind", ["v1", "v2", "hybrid"])
def test_cold_small_requests(native, cold_tree, kind, odirect):
    """A shard whose files are mostly not in the page cache is read in requests of TV_OPT_STREAM_COLD_REQ bytes (1 MiB:
    four rows of 256 KiB) by TV_OPT_STREAM_COLD_READERS readers; the files of 5 MiB go O_DIRECT (every file's last row
    through the aligned scratch), the one under 1 MiB never does; a refused O_DIRECT read falls back per file.  With
    TV_OPT_FILE_ODIRECT = 0 no shard is judged cold (shard_is_cold), so its requests stay one slot long: those three
    cases exercise neither cold option.  TV_OPT_STREAM_COLD_READERS = 3 is run under, not asserted: the reader count
    shows in no counter, so nothing here tells whether it was obeyed."""
    import fsutil
    N, c = native, cold_tree["a"]
    full, L, C = cold_tree["full"], T.COLD_L, T.COLD_C
    if kind == "v1":
        v = T.cold_v1()
        P, want = v.P, cold_tree["want_v1"]
        budget = 2 * (P * (C + 256) + 256)
    else:
        lay = c.lay(kind == "hybrid")
        P = lay.P
        want = c.expected_v2(False) if kind == "v2" else c.expected_hybrid(False, True)
        budget = v2_window_budget(C) if kind == "v2" else hsu.window_budget(C, P)
    status = T.expected_status(c.lengths, c.faults, False)
    small, one_slot = c.lengths[1], len(T.request_plan(0, P, C, P, L))
    four_rows = len(T.request_plan(0, P, C, P, L, T.COLD_REQ)) if odirect else one_slot
    assert (one_slot, four_rows) == (4, {"v1": 16}.get(kind, 20) if odirect else 4)
    with N.Context(0) as ctx:
        if kind == "v1":
            ctx.set_option(N.TV_OPT_RESIDENT, 0)
            ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
            ctx.set_option(N.TV_OPT_STREAM_CHUNK, 0)
            ctx.set_layout(v.total, L, P)
            ctx.set_digests(v.digests)
            call, launches = (lambda: ctx.stream_file_table(c.lengths, full)), 4
        else:
            call, _, launches, reqs = aligned_call(ctx, N, kind, lay, c.lengths, full, 0, budget)
            assert reqs == one_slot

        def run(cold_pass: bool, req: int):
            ctx.set_option(N.TV_OPT_STREAM_COLD_REQ, req)
            if cold_pass:
                assert fsutil.drop_cache(full) <= 0.01
            else:
                for p in full:
                    with open(p, "rb") as f:
                        f.read()
                assert fsutil.resident(full) > 0.99
            ctx._reset_file_clock()
            got, st = call()
            clock = ctx._file_clock()
            print(kind, odirect, "cold" if cold_pass else "warm", req, requests(ctx, N), clock)
            assert got == want, (cold_pass, req)
            assert st == status and ctx.last_kernel()[1] == launches
            return clock

        keys = (N.TV_OPT_STREAM_COLD_REQ, N.TV_OPT_STREAM_COLD_READERS, N.TV_OPT_FILE_ODIRECT, N.TV_OPT_FILE_THREADS)
        before = [ctx.get_option(k) for k in keys]
        try:
            ctx.set_option(N.TV_OPT_FILE_THREADS, 4)
            ctx.set_option(N.TV_OPT_FILE_ODIRECT, odirect)
            ctx.set_option(N.TV_OPT_STREAM_COLD_READERS, 3)
            clock = run(False, T.COLD_REQ)                     # warm: never cold, never O_DIRECT
            assert requests(ctx, N) == one_slot
            assert clock["bytes_odirect"] == 0 and clock["odirect_fallbacks"] == 0, clock
            clock = run(True, T.COLD_REQ)
            assert requests(ctx, N) == four_rows
            if odirect == 1:
                assert 0 < clock["bytes_odirect"] <= clock["bytes_read"] - small, clock
                assert clock["odirect_fallbacks"] == 0 and clock["odirect_errno"] == 0, clock
            else:
                assert clock["bytes_odirect"] == 0, clock
                if odirect == 2:
                    assert clock["odirect_fallbacks"] > 0 and clock["odirect_errno"] == errno.EINVAL, clock
                else:
                    assert clock["odirect_fallbacks"] == 0, clock
            run(True, 0)                                       # cold, the default request size: one slot
            assert requests(ctx, N) == one_slot
        finally:
            for k, value in zip(keys, before):
                ctx.set_option(k, value)
