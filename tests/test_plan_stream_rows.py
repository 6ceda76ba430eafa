"""CPU unit tests of the stream engine's two pure rules in torrent_amd/csrc/tv_plan.h, run through
tests/c/plan_stream_rows_main.cpp (an ordinary executable: it also builds with -fsanitize=address,undefined):

* for_row_copies, the copy plan of a request (one 2D copy per maximal run of full-width rows, one copy per short row,
  none for an empty row): against a plain-Python restatement, its invariants, the shape of a v1 request, and -- each
  emit replayed on host buffers -- that the destination is the row-by-row copy of every row's valid bytes and nothing
  else changed;
* walk_row_files, a row's linear range over the file table: against a brute-force byte-to-file map, over back-to-back
  and aligned (v2_file_starts) tables with zero-length files, gaps and the table's end."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "plan_stream_rows_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

WALKED, GAP, SHORT = 0, 1, 2


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
    exe = str(tmp_path_factory.mktemp("plan_stream_rows") / "plan_stream_rows_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    return _runner(exe)


# ---- the copy plan ----------------------------------------------------------------------------------------------------

def copy_plan(rows, width):
    """The restatement: [(first_row, rows, bytes_per_row)]."""
    out, q = [], 0
    while q < len(rows):
        e = q + 1
        if rows[q] == width:
            while e < len(rows) and rows[e] == width:
                e += 1
        if rows[q]:
            out.append((q, e - q, rows[q]))
        q = e
    return out


def _copy_query(rows, width, pitch, stop=-1):
    return "c %d %d %d %d %s" % (width, pitch, stop, len(rows), " ".join(map(str, rows)))


def _parse_copy(line):
    ret, emits, status = (f.strip() for f in line.split("|"))
    return int(ret), [] if emits == "-" else [tuple(map(int, e.split(":"))) for e in emits.split()], status


def _check_plan(rows, width, emits):
    assert emits == copy_plan(rows, width), rows
    covered, prev = [], None
    for first, n, nb in emits:
        assert n >= 1 and 0 < nb <= width
        assert n == 1 or nb == width                                  # only full rows run together
        assert prev is None or first >= prev[0] + prev[1]             # in row order, disjoint
        if prev is not None and nb == width and prev[2] == width:
            assert first > prev[0] + prev[1]                          # maximal: no two adjacent full runs
        assert all(rows[q] == nb for q in range(first, first + n))
        covered += range(first, first + n)
        prev = (first, n, nb)
    assert covered == [q for q, nb in enumerate(rows) if nb]          # exactly the non-empty rows


@pytest.mark.parametrize("width,pitch", [(64, 64), (64, 100), (4096, 4096 + 192)])
def test_copy_plan_exhaustive_small(plan, width, pitch):
    cases = [list(rows) for n in range(0, 7) for rows in itertools.product((0, 1, width - 1, width), repeat=n)]
    out = plan([_copy_query(rows, width, pitch) for rows in cases])
    for rows, line in zip(cases, out):
        ret, emits, status = _parse_copy(line)
        assert ret == 0 and status == "ok", (rows, line)
        _check_plan(rows, width, emits)


def test_copy_plan_seeded_random(plan):
    rng = random.Random(20260411)
    cases = []
    for _ in range(300):
        width = rng.choice((1, 2, 64, 1000, 16384))
        n = rng.randint(1, 300)
        weights = rng.choice(((1, 1, 1, 1), (1, 1, 1, 12), (6, 1, 1, 2), (0, 1, 1, 1)))
        rows = rng.choices((0, 1, width - 1, width), weights=weights, k=n)
        cases.append((rows, width, width + rng.choice((0, 1, 64, 333))))
    out = plan([_copy_query(*c) for c in cases])
    for (rows, width, _), line in zip(cases, out):
        ret, emits, status = _parse_copy(line)
        assert ret == 0 and status == "ok", (rows, width)
        _check_plan(rows, width, emits)


def test_copy_plan_of_a_v1_request(plan):
    """All rows full but possibly the last (the torrent's short last piece: short in its column, empty in the later
    ones): the full run, then the tail -- the copies the v1 commit path queued before it shared this plan."""
    width = 4096
    cases = [[width] * full + tail for full in (0, 1, 2, 69) for tail in ([], [0], [1], [width - 1])]
    out = plan([_copy_query(rows, width, width + 64) for rows in cases])
    for rows, line in zip(cases, out):
        ret, emits, status = _parse_copy(line)
        assert ret == 0 and status == "ok"
        full = sum(1 for nb in rows if nb == width)
        tail = rows[-1] if rows and 0 < rows[-1] < width else 0
        assert emits == ([(0, full, width)] if full else []) + ([(full, 1, tail)] if tail else [])
        assert len(emits) <= 2


def test_copy_plan_stops_at_a_nonzero_emit(plan):
    rows, width = [64, 64, 3, 0, 64, 63, 64], 64
    full = copy_plan(rows, width)
    out = plan([_copy_query(rows, width, 80, stop) for stop in range(len(full))])
    for stop, line in enumerate(out):
        ret, emits, status = _parse_copy(line)
        assert ret == 7 and emits == full[:stop + 1] and status == "ok"     # (the rows before the stop were copied)


# ---- the row walk -----------------------------------------------------------------------------------------------------

def file_starts(lengths, L):
    start = [0]
    for n in lengths:
        end = start[-1] + n
        start.append((end + L - 1) // L * L if L else end)
    return start


def brute_walk(lengths, L, a, b, stop=-1):
    """Byte by byte: (result, [(file, file_offset, dst_offset, len)])."""
    start = file_starts(lengths, L)
    owner = {}
    for k, n in enumerate(lengths):
        for o in range(n):
            owner[start[k] + o] = (k, o)
    segs, pos = [], a
    while pos < b:
        if pos not in owner:
            # before a later file's start (a zero-length one too): the gap after a file; else the table has ended
            return (GAP if lengths and start[len(lengths) - 1] > pos else WALKED), segs
        k, o = owner[pos]
        n = 1
        while pos + n < b and owner.get(pos + n) == (k, o + n):
            n += 1
        segs.append((k, o, pos - a, n))
        if len(segs) - 1 == stop:
            return SHORT, segs
        pos += n
    return WALKED, segs


def _walk_query(lengths, L, a, b, stop=-1):
    return "w %d %d %d %d %d %s" % (L, a, b, stop, len(lengths), " ".join(map(str, lengths)))


def _parse_walk(line):
    res, segs = (f.strip() for f in line.split("|"))
    return int(res), [] if segs == "-" else [tuple(map(int, s.split(":"))) for s in segs.split()]


TABLES = [
    ([5, 7, 3], 0),
    ([0, 0, 5, 0, 0, 7, 0], 0),              # zero-length files at the start, in the middle and at the end
    ([0], 0), ([], 0), ([9], 0),
    ([16, 5, 33, 1], 16),                    # aligned: gaps after files 1, 2 and 3
    ([0, 5, 0, 0, 32, 0, 17, 0], 16),        # ... with zero-length files at the start, in the middle and at the end
    ([20], 16), ([16, 16], 16),
]


@pytest.mark.parametrize("lengths,L", TABLES)
def test_row_walk_matches_the_byte_map(plan, lengths, L):
    end = file_starts(lengths, L)[-1]
    cases = [(a, b) for a in range(0, end + 4) for b in range(a, end + 6)]
    out = plan([_walk_query(lengths, L, a, b) for a, b in cases])
    for (a, b), line in zip(cases, out):
        res, segs = _parse_walk(line)
        assert (res, segs) == brute_walk(lengths, L, a, b), (a, b)
        assert res in (WALKED, GAP)
        at = 0
        for k, fo, dst, n in segs:                     # contiguous in the destination, inside their files, in order
            assert dst == at and n > 0 and fo + n <= lengths[k]
            at += n
        assert at <= b - a
        assert [s[0] for s in segs] == sorted({s[0] for s in segs})
        if res == WALKED and b <= sum(lengths) and not L:
            assert at == b - a                         # back to back, inside the table: every byte is covered


def test_row_walk_named_cases(plan):
    L = 16
    aligned = [40, 0, 16, 3]                           # starts 0, 48, 48, 64; the table ends at 80 (file 3 at 67)
    assert file_starts(aligned, L) == [0, 48, 48, 64, 80]
    queries = [
        (aligned, L, 32, 40),                          # a row ending with its file, inside the file's last piece
        (aligned, L, 32, 48),                          # ... reaching into the gap after it
        (aligned, L, 40, 44),                          # ... starting in the gap
        (aligned, L, 48, 64),                          # past a zero-length file that shares its start
        (aligned, L, 64, 80),                          # the last file's piece: the table ends before the row does
        (aligned, L, 80, 96), (aligned, L, 200, 216),  # at and past the table's end
        ([5, 7], 0, 3, 30),                            # runs out of table mid-way
        ([5, 7], 0, 12, 20), ([5, 7], 0, 12, 12),
    ]
    out = [_parse_walk(line) for line in plan([_walk_query(*q) for q in queries])]
    assert out == [(WALKED, [(0, 32, 0, 8)]), (GAP, [(0, 32, 0, 8)]), (GAP, []), (WALKED, [(2, 0, 0, 16)]),
                   (WALKED, [(3, 0, 0, 3)]), (WALKED, []), (WALKED, []), (WALKED, [(0, 3, 0, 2), (1, 0, 2, 7)]),
                   (WALKED, []), (WALKED, [])]
    assert out == [brute_walk(*q) for q in queries]


def test_row_walk_stops_at_a_short_segment(plan):
    lengths = [4, 0, 6, 5, 0, 9]
    whole = brute_walk(lengths, 0, 1, 23)[1]
    assert len(whole) == 4
    out = plan([_walk_query(lengths, 0, 1, 23, stop) for stop in range(len(whole))])
    for stop, line in enumerate(out):
        assert _parse_walk(line) == (SHORT, whole[:stop + 1]) == brute_walk(lengths, 0, 1, 23, stop)


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "plan_stream_rows_asan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    width = 64
    rows = [list(r) for n in range(0, 5) for r in itertools.product((0, 1, width - 1, width), repeat=n)]
    rows += [[width] * 69 + [1], [width] * 70, [0] * 5]
    lines = [_copy_query(r, width, 100) for r in rows]
    walks = [(lengths, L, a, b) for lengths, L in TABLES
             for a in range(0, file_starts(lengths, L)[-1] + 3, 3) for b in (a, a + 1, a + 16, a + 100)]
    lines += [_walk_query(*w) for w in walks]
    out = _runner(exe)(lines)
    for r, line in zip(rows, out):
        assert _parse_copy(line) == (0, copy_plan(r, width), "ok")
    for w, line in zip(walks, out[len(rows):]):
        assert _parse_walk(line) == brute_walk(*w)
