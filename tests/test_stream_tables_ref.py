"""CPU: what makes the layouts of tests/stream_tables.py reach the stream engine's host paths, pinned so that
tests/test_gpu_stream_tables.py cannot quietly go shallow -- the file counts and what lies past FdCache's 256 kept
descriptors, a v1 piece spanning 20 files and more, the requests per unit under the restated geometry, expected
bitfields that are neither all ones nor all zeros -- and the references held to each other: Storage(fs_storage).get +
hashlib on a written tree against the byte model, tests/v2_ref.py against hybrid_util.Layout.verdicts."""
import os

import pytest

from tests import hybrid_stream_util as hsu
from tests import hybrid_util as hu
from tests import stream_tables as T
from tests.test_gpu_v2_stream import geometry as v2_geometry
from tests.test_gpu_v2_stream import window_budget as v2_window_budget

K, M = T.K, T.M


def mixed(bits: bytes, n: int) -> bool:
    oks = hu.unpack(bits, n)
    return any(oks) and not all(oks)


# ---- C1 ---------------------------------------------------------------------------------------------------------------

def test_v1_table_shape():
    v = T.v1_table()
    assert (v.L, v.n, v.P) == (16 * K, 336, 104) and v.total % v.L == 5575          # >= 320 files, a short last piece
    assert sum(1 for k in range(v.n) if k >= T.CACHED_FDS) == 80                    # >= 40 files past the kept descriptors
    assert T.both_sides(v.faults, v.n)
    v.check()
    spans = [len(v.files_in_piece(i)) for i in range(v.P)]
    assert max(spans) == 42 and sum(1 for s in spans if s >= 20) >= 7               # pieces spanning >= 20 files
    assert any(len(v.pieces_of(k)) >= 11 for k in range(v.n))                       # files of several pieces
    zeros = [k for k, n in enumerate(v.lengths) if n == 0]
    assert zeros[0] == 0 and v.lengths[-2] == 0 and len(zeros) == 24                # before, between and after
    assert any(k > T.CACHED_FDS for k in zeros)
    # the piece spanning the most files lies past position 256 too (its files are opened per read)
    assert any(min(v.files_in_piece(i)) >= T.CACHED_FDS and s >= 20 for i, s in enumerate(spans))


def test_v1_geometries():
    v = T.v1_table()
    assert T.v1_column(v.L, 4096) == 4096                                           # four columns, one window
    budget = 2 * (v.P * (8192 + 256) + 256)
    assert T.v1_budget_geometry(v.L, v.P, budget) == (8192, v.P)                    # two columns; below 2,048 pieces: one window
    assert T.v1_row_window(v.L, v.P, T.v1_rows_budget(v.L)) == 64                   # whole-piece rows: two windows
    # what each geometry opens past the 256 kept descriptors (a row's walk ends at its first failing file), as root
    # and as a user whom the unwritable files refuse, opened read-only and read + write
    for blocked, open_rw in ((False, False), (False, True), (True, True)):
        own = [len(v.opened(C, blocked, open_rw)) - T.CACHED_FDS for C in (4096, 8192, v.L)]
        assert min(own) >= 40, (blocked, open_rw, own)


@pytest.mark.parametrize("blocked", [False, True])
def test_v1_reference_on_a_written_tree(tmp_path, blocked):
    """Storage(fs_storage).get + hashlib over the written tree equals the byte model (a read-only file blocks a
    read + write open only where this process may not write it: `blocked` is simulated by leaving it out)."""
    v = T.v1_table()
    faults = v.faults
    if blocked:
        faults = T.Faults(faults.missing + faults.readonly, faults.short, faults.directory, (), faults.flips)
    root = str(tmp_path / "ref")
    T.write_tree(root, v.paths, v.files, faults, chmod=False)
    want = v.expected_from_tree(root)
    assert want == v.expected_model(blocked) and mixed(want, v.P)
    assert want == v.expected_from_tree(root)                                        # (the files it created change nothing)
    bad = [i for i, ok in enumerate(hu.unpack(want, v.P)) if not ok]
    assert len(bad) == (23 if blocked else 9)
    status = T.expected_status(v.lengths, v.faults, blocked)
    assert [k for k, s in enumerate(status) if s] == sorted(v.faults.failing(blocked))


# ---- C2 ---------------------------------------------------------------------------------------------------------------

def test_many_files_shape_and_references():
    a = T.many()
    assert (a.L, a.n, a.P) == (32 * K, 341, 403) and a.n - T.CACHED_FDS >= 40
    assert min(len(a.opened(b, rw)) for b, rw in ((False, False), (False, True), (True, True))) - T.CACHED_FDS >= 40
    assert T.both_sides(a.faults, a.n)
    a.check()
    for blocked in (False, True):
        v2 = a.expected_v2(blocked)
        assert mixed(v2, a.P)
        for trailing in (False, True):
            both, v1, v2h = a.expected_hybrid(blocked, trailing)
            assert v2h == v2 and both == v1 == v2                 # two references agree; every fault shows in both sets
        assert hu.pack([i not in a.unreadable(blocked) for i in range(a.P)]) == a.readable_bits(blocked)
    assert len(a.unreadable(True)) - len(a.unreadable(False)) == 2                   # the read-only files' pieces
    # one wrongly stated v1 digest: the two sets disagree on that piece alone
    lay = a.lay(True)
    both, v1, v2 = a.expected_hybrid(False, True, pieces=hu.xor_at(lay.pieces, 20 * 5 + 3, 2))
    assert [i for i in range(a.P) if hu.unpack(v1, a.P)[i] != hu.unpack(v2, a.P)[i]] == [5]


def test_many_files_geometries():
    a = T.many()
    L, P = a.L, a.P
    assert v2_geometry(L, P, 0, 16 * K) == hsu.geometry(L, P, 0, 16 * K) == (16 * K, P)           # 16 KiB columns
    assert v2_geometry(L, P, v2_window_budget(16 * K), 0) == (16 * K, 64)                        # seven windows
    assert hsu.geometry(L, P, hsu.window_budget(16 * K, P), 0) == (16 * K, 384)                  # two windows
    assert T.requests_per_unit(P, 16 * K, 64) == [1] * 7 and T.requests_per_unit(P, 16 * K, 384) == [1, 1]


# ---- C5 ---------------------------------------------------------------------------------------------------------------

def test_tall_units_shape_and_geometries():
    L, P = T.TALL_L, T.TALL_P
    sizes = T.tall_sizes()
    table = T.v2_ref.piece_table(sizes, L)
    assert len(table) == P == 4166
    pb = [r[2] for r in table]
    # short and empty rows on both sides of row 4096, in both columns of 16 KiB
    assert pb[4090:4099] == [100, 1, 16384, 16385, L, L, L - 5, 20000, 55] and pb[4159] == 16383 and pb[-1] == 1
    for col in (0, 16 * K):
        rows = [max(0, min(16 * K, b - col)) for b in pb]
        for side in (rows[:4096], rows[4096:]):
            assert any(0 < r < 16 * K for r in side) and (col == 0 or any(r == 0 for r in side))
    # shape 1: 16 KiB columns across the shard: every unit is two requests (4096 + 70 rows), four in all (three slots)
    assert v2_geometry(L, P, 0, 16 * K) == hsu.geometry(L, P, 0, 16 * K) == (16 * K, P)
    plan = T.request_plan(0, P, 16 * K, P, L)
    assert [(p, r, o) for p, r, o in plan] == [(0, 4096, 0), (4096, 70, 0), (0, 4096, 16 * K), (4096, 70, 16 * K)]
    # shape 2: windows of 2,112 whole pieces: two requests per unit, and a shorter last window (2,054 = 2,048 + 6)
    W = T.TALL_WINDOW
    assert v2_geometry(L, P, v2_window_budget(L, W), 0) == hsu.geometry(L, P, hsu.window_budget(L, W), 0) == (L, W)
    assert T.requests_per_unit(P, L, W) == [2, 2]
    assert T.request_plan(0, P, L, W, L) == [(0, 2048, 0), (2048, 64, 0), (2112, 2048, 0), (4160, 6, 0)]


@pytest.mark.slow
def test_tall_units_reference():
    t = T.tall()
    both, v1, v2 = t.expected_hybrid(False, True)
    assert both == v1 == v2 == t.expected_v2(False) == hu.pack([i not in T.TALL_FLIPPED for i in range(t.P)])
    lay = t.lay(True)
    assert {4090, 4096, 4159, 4165} <= set(lay.tails)            # pad ranges on both sides of row 4096, and in the last row


# ---- C6 ---------------------------------------------------------------------------------------------------------------

def test_cold_shape_and_geometries():
    c, v = T.cold(), T.cold_v1()
    L, C = T.COLD_L, T.COLD_C
    assert (c.P, v.P) == (19, 16) and min(c.lengths) < M and sorted(c.lengths)[1] >= 5 * M
    assert all(n % 4096 for n in c.lengths)                                           # every file's last row is short
    # 256 KiB columns under each kind's budget, warm or cold (a cold v1 shard's windows: at least 512 pieces)
    b1 = 2 * (v.P * (C + 256) + 256)
    assert T.v1_budget_geometry(L, v.P, b1) == T.v1_budget_geometry(L, v.P, b1, 512) == (C, v.P)
    assert v2_geometry(L, c.P, v2_window_budget(C), 0) == (C, c.P)
    assert hsu.geometry(L, c.P, hsu.window_budget(C, c.P), 0) == (C, c.P)
    # four rows per request under TV_OPT_STREAM_COLD_REQ = 1 MiB, one request per unit otherwise
    assert len(T.request_plan(0, v.P, C, v.P, L, T.COLD_REQ)) == 16 and len(T.request_plan(0, v.P, C, v.P, L)) == 4
    assert len(T.request_plan(0, c.P, C, c.P, L, T.COLD_REQ)) == 20 and len(T.request_plan(0, c.P, C, c.P, L)) == 4
    assert T.requests_per_unit(c.P, C, c.P, T.COLD_REQ) == [5]
    # the short file's tail pieces are unreadable, and nothing else
    assert sorted(c.unreadable(False)) == [16, 17, 18]
    want = c.expected_v2(False)
    assert mixed(want, c.P) and c.expected_hybrid(False, True)[0] == want == c.expected_hybrid(False, False)[2]
    assert [i for i, ok in enumerate(hu.unpack(want, c.P)) if not ok] == [3, 6, 12, 16, 17, 18]
    assert [i for i, ok in enumerate(hu.unpack(v.expected_model(False), v.P)) if not ok] == [3, 5, 10, 13, 14, 15]


def test_cold_v1_reference_on_a_written_tree(tmp_path):
    v = T.cold_v1()
    root = str(tmp_path / "ref")
    full = T.write_tree(root, v.paths, v.files, v.faults)
    assert os.path.getsize(full[3]) == v.lengths[3] - T.COLD_CUT
    assert v.expected_from_tree(root) == v.expected_model(False)
