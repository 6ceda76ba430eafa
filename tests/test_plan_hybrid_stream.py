"""CPU unit tests of the hybrid stream planning in torrent_amd/csrc/tv_plan.h (hybrid_stream_geometry, hybrid_col_range and
the chunk helpers tv_hybrid_col_pad_kernel shares with them), run through tests/c/plan_hybrid_stream_main.cpp (an
ordinary executable: it also builds with -fsanitize=address,undefined): the geometry against a plain-Python
restatement (tests/hybrid_stream_util.py) and its invariants; which bytes of a column's rows read as zeros; and --
replaying the column pad launch workgroup by workgroup on a host buffer -- that exactly those bytes are stored, each
once, vector stores aligned, nothing in a row outside the unit, for every alignment of the row bases."""
import os
import shutil
import subprocess

import pytest

from tests.hybrid_stream_util import G, K, LEAF, M, SLOT, col_chunks, col_range, geometry, window_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "plan_hybrid_stream_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _runner(exe):
    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_hybrid_stream") / "plan_hybrid_stream_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    return _runner(exe)


LENGTHS = [16 * K, 64 * K, 1 * M, 128 * M]
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 51200]
MIN_BUDGET = window_budget(LEAF)                            # 64 rows of 16 KiB
BUDGETS = [MIN_BUDGET, MIN_BUDGET + 1, window_budget(64 * K), 64 * M, G // 4, G // 2, G, 2 * G, 4 * G]


def test_geometry_matches_the_restatement_and_keeps_its_invariants(plan):
    cases = [(L, n, b, ch) for L in LENGTHS for n in COUNTS for b in BUDGETS
             for ch in (0, 1, 16 * K, 48 * K, L, 2 * L)]
    out = plan(["g %d %d %d %d" % c for c in cases])
    for (L, n, budget, chunk), line in zip(cases, out):
        C, wn = map(int, line.split())
        assert (C, wn) == geometry(L, n, budget, chunk), (L, n, budget, chunk)
        assert C & (C - 1) == 0 and LEAF <= C <= min(L, SLOT)           # a power of two within bounds
        assert wn == n or wn % 64 == 0
        assert 1 <= wn <= n
        if chunk:
            assert wn == n and C <= max(chunk, LEAF)                   # one window across the shard
        else:
            assert 2 * (wn * (C + 256) + 256) <= budget                # (every budget here holds 64 rows of 16 KiB)
            assert wn * (C + 256) + 256 <= 256 * M                     # kStreamChunkMax per buffer
            # the floor: fewer than min(count, 2,048) pieces (in whole 64s) per window only at the narrowest column
            assert wn >= min(n, 2048) // 64 * 64 or C == LEAF


def test_documented_geometry(plan):
    # cfg2 (16,384 x 1 MiB) under the default budget and under 0.25 GiB: 2,048 rows of pitch 128 KiB + 256 do not fit
    # 256 MiB (2,044 do), so the columns are 64 KiB / 32 KiB and a window holds 4,032 pieces
    out = plan(["g %d 16384 %d 0" % (M, G), "g %d 16384 %d 0" % (M, G // 4), "g %d 100 %d 0" % (M, G),
                "g %d 16384 %d %d" % (M, G, 48 * K)])
    assert out[0].split() == [str(64 * K), str(4032)]
    assert out[1].split() == [str(32 * K), str(4032)]
    assert out[2].split() == [str(M), "100"]                            # a small shard: whole pieces, one window
    assert out[3].split() == [str(32 * K), "16384"]


SIZES = lambda L: sorted({s for s in (1, 15, 16, 17, 16383, 16384, 16385, L - 1, L) if 1 <= s <= L})   # noqa: E731


@pytest.mark.parametrize("L,C", [(16 * K, 16 * K), (64 * K, 16 * K), (1 * M, 256 * K), (1 * M, 1 * M)])
def test_column_ranges(plan, L, C):
    cases = []
    for pb in SIZES(L):
        for v1 in (L, pb):                                  # a pad out to the piece's end; a short last piece (no pad)
            for offset in range(0, L, C):                   # the column before, inside, at and past the piece's end
                cases.append((pb, v1, offset, C))
    out = plan(["r %d %d %d %d" % c for c in cases])
    for (pb, v1, offset, C_), line in zip(cases, out):
        b, e, chunks = map(int, line.split())
        assert (b, e) == col_range(pb, v1, offset, C_), (pb, v1, offset)
        assert chunks == col_chunks(b, e)
        assert 0 <= b <= C_ and 0 <= e <= C_
        if v1 == pb:
            assert b >= e                                   # no pad range: nothing to zero
        elif offset + C_ <= pb:
            assert b >= e                                   # the column lies before the piece's end
        elif offset >= pb:
            assert (b, e) == (0, C_)                        # ... wholly in the pad: the whole column
        else:
            assert (b, e) == (pb - offset, C_)              # ... holds the piece's end


def _table(L, trailing):
    """Rows of every size, then a last piece that is short (trailing: followed by a pad out to L)."""
    pb = SIZES(L) + [L, 777]
    total = len(pb) * L if trailing else (len(pb) - 1) * L + pb[-1]
    return total, pb


@pytest.mark.parametrize("L,C", [(16 * K, 16 * K), (64 * K, 16 * K), (1 * M, 256 * K)])
def test_replayed_column_launch_stores_exactly_the_ranges(plan, L, C):
    lines, cases = [], []
    for trailing in (False, True):
        total, pb = _table(L, trailing)
        for offset in range(0, L, C):
            for align in (0, 1, 8, 15):
                for first, rows in ((0, pb), (3, pb[3:])):      # (a unit that starts mid-shard: v1_len by GLOBAL piece)
                    lines.append("p %d %d %d %d %d %d %d %s" % (total, L, first, len(rows), offset, C, align,
                                                                " ".join(map(str, rows))))
                    cases.append((total, first, rows, offset))
    for (total, first, rows, offset), line in zip(cases, plan(lines)):
        head, _, body = line.partition("|")
        want, chunks = [], 0
        for r, pb in enumerate(rows):
            v1 = max(0, min(L, total - (first + r) * L))
            b, e = col_range(pb, v1, offset, C)
            want.append("%d:%d" % (b, e) if b < e else "-")
            chunks = max(chunks, col_chunks(b, e))
        assert int(head) == chunks
        assert body.split() == want, (total, first, offset)


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "plan_hybrid_stream_asan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L, C = 64 * K, 16 * K
    total, pb = _table(L, True)
    out = _runner(exe)(["g %d 2049 %d 0" % (L, MIN_BUDGET), "g %d 51200 %d 0" % (128 * M, 4 * G),
                        "r 17 %d 0 %d" % (L, C)] +
                       ["p %d %d 0 %d %d %d 15 %s" % (total, L, len(pb), off, C, " ".join(map(str, pb)))
                        for off in range(0, L, C)])
    assert out[0].split() == ["%d" % LEAF, "64"] and out[2].split() == ["17", str(C), "1"]
    assert tuple(map(int, out[1].split())) == geometry(128 * M, 51200, 4 * G, 0)
    assert all("guard" not in line and " x" not in line for line in out[3:])
