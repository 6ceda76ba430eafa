"""CPU unit tests of the v2 stream planning in torrent_amd/csrc/tv_plan.h, run through tests/c/plan_v2_main.cpp:
v2_stream_geometry (a streamed v2 verify's column width and window under a device budget or an explicit chunk) over a
grid, and v2_file_starts (where each file sits in the aligned linear space) against make_layout's file_offset."""
import os
import shutil
import subprocess

import pytest

from tests.v2_util import golden
from torrent_amd.metainfo_v2 import make_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, G = 1 << 10, 1 << 20, 1 << 30
LEAF = 16 * K
SLACK = 256          # bytes after a chunk buffer's last row (what the library passes)
COL_MAX = 64 * M     # one ring slot

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_v2") / "plan_v2_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_v2_main.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines)
        return out

    return run


def two_buffers(C, rows):
    return 2 * (rows * (C + 256) + SLACK)


def pow2(x):
    return x > 0 and x & (x - 1) == 0


def test_geometry_grid(plan):
    Ls = [16 * K, 32 * K, 64 * K, 1 * M, 8 * M, 64 * M, 128 * M, 1 * G]
    counts = [1, 2, 63, 64, 65, 130, 1000, 16384, 200000]
    budgets = [0, 1 * M, 2 * M + 100 * K, 3 * M, 16 * M, 256 * M, 300 * M + 12345, 1 * G, 2 * G, 64 * G]
    chunks = [0, 1, 16 * K, 16 * K + 1, 24 * K, 32 * K, 100 * K, 4 * M, 48 * M, 64 * M, 100 * M, 1 * G, 5 * G]
    cases = [(L, n, B, 0) for L in Ls for n in counts for B in budgets]
    cases += [(L, n, B, X) for L in Ls for n in (1, 130, 16384) for B in (0, 1 * G) for X in chunks[1:]]
    out = plan(["g %d %d %d %d" % c for c in cases])
    for (L, count, B, X), line in zip(cases, out):
        C, wn = map(int, line.split())
        cmax = min(L, COL_MAX)
        what = (L, count, B, X, C, wn)
        assert pow2(C) and LEAF <= C <= cmax, what
        assert wn == count or (wn % 64 == 0 and 64 <= wn < count), what
        if X:
            # the largest power of two <= min(max(X, 16 KiB), Cmax), one window across the shard
            lim = min(max(X, LEAF), cmax)
            assert C <= lim < 2 * C and wn == count, what
            continue
        if two_buffers(LEAF, 64) <= B:      # 64 rows of one leaf fit: so does what was chosen
            assert two_buffers(C, wn) <= B, what
            if wn < count:
                assert B < two_buffers(C, wn + 64), what     # the largest such window
        if two_buffers(cmax, 64) <= B:      # 64 whole pieces (or slot-wide columns) fit: no narrower column
            assert C == cmax, what
        elif C > LEAF:                      # halved only as far as needed
            assert two_buffers(C, 64) <= B < two_buffers(2 * C, 64), what
        else:
            assert B < two_buffers(2 * LEAF, 64), what


def test_geometry_documented_shapes(plan):
    out = plan(["g %d %d %d %d" % c for c in [
        (1 * M, 16384, 1 * G, 0),        # cfg2 under the default budget: whole pieces, 448 per window
        (1 * M, 16384, 256 * M, 0),      # a quarter GiB: still whole pieces
        (64 * K, 130, 2 * 64 * (64 * K + 256) + 512, 0),   # exactly 64 whole pieces per buffer
        (128 * M, 2, 1 * G, 0),          # a piece longer than a ring slot: 64 rows of a column must fit, so 4 MiB
        (128 * M, 2, 16 * G, 0),         # ... and with room for them the column is the slot's 64 MiB
        (128 * M, 2, 0, 128 * M),        # an explicit chunk is capped at the slot too
        (8 * M, 3, 0, 4 * M),
        (8 * M, 3, 0, 64 * K)]])
    assert [tuple(map(int, ln.split())) for ln in out] == [
        (1 * M, 448), (1 * M, 64), (64 * K, 64), (4 * M, 2), (64 * M, 2), (64 * M, 2), (4 * M, 3),
        (64 * K, 3)]


def _layout_cases():
    cases = [(g["piece_length"], list(g["lengths"])) for g in golden().values()]
    for L in (16 * K, 64 * K):   # zero-length files (first, between, last) and files of exactly L and L + 1 bytes
        cases += [(L, [0, L, 0, 0, L + 1, 1, 0]), (L, [L]), (L, [L + 1]), (L, [0]), (L, []), (L, [0, 0, 3 * L, L - 1, 0])]
    return cases


def test_aligned_file_starts_equal_make_layout(plan):
    cases = _layout_cases()
    assert len(cases) >= 12
    out = plan(["s %d %d %s" % (L, len(ln), " ".join(map(str, ln))) for L, ln in cases])
    for (L, lengths), line in zip(cases, out):
        start = list(map(int, line.split()))
        lay = make_layout(lengths, L)
        assert len(start) == len(lengths) + 1
        assert start[:-1] == list(lay.file_offset), (L, lengths)
        assert start[-1] == lay.n_pieces * L, (L, lengths)
        for k, n in enumerate(lengths):
            assert start[k] % L == 0 and start[k + 1] - start[k] == -(-n // L) * L


def test_file_starts_overflow(plan):
    big = (1 << 64) - 1
    assert plan(["s %d 2 %d %d" % (16 * K, big - 5, 1), "s %d 2 %d %d" % (16 * K, 16 * K, big)]) == \
        ["overflow 0", "overflow 1"]
