"""CPU unit tests of the hybrid tail planning in torrent_amd/csrc/tv_plan.h (hybrid_tails and the chunk helpers the pad
kernel shares with it), run through tests/c/plan_hybrid_main.cpp (an ordinary executable: it also builds with
-fsanitize=address,undefined): which rows of a shard get a pad range, which bytes, and -- replaying the launch workgroup
by workgroup on a host buffer -- that exactly those bytes are stored, each once, vector stores aligned, for every
alignment of the row bases.  The expected values are restated here in plain Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 64 << 10
SRC = os.path.join(ROOT, "tests", "c", "plan_hybrid_main.cpp")

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
    exe = str(tmp_path_factory.mktemp("plan_hybrid") / "plan_hybrid_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    return _runner(exe)


def v1_len(total, L, i):
    return max(0, min(L, total - i * L))


def ref_tails(total, L, first, pb):
    """[(row, begin, end, chunk0)], or ("bad", j)."""
    out, chunks = [], 0
    for j, b in enumerate(pb):
        v1 = v1_len(total, L, first + j)
        if b > v1:
            return ("bad", j), 0
        if b < v1:
            out.append((j, b, v1, chunks))
            chunks += -(-(v1 - b // 16 * 16) // CHUNK)
    return out, chunks


def files_table(lengths, L, trailing_pad=False):
    """(total, piece_bytes) of files at aligned offsets: the v1 length ends at the last file's bytes, or at its pad."""
    pb = []
    for n in lengths:
        pb += [min(L, n - q * L) for q in range(-(-n // L))]
    total = (len(pb) - 1) * L + (L if trailing_pad else pb[-1]) if pb else 0
    return total, pb


def parse(line):
    tok = line.split()
    return [tuple(map(int, t.split(":"))) for t in tok[2:]], int(tok[1])


SIZES = lambda L: [1, 15, 16, 17, 16383, 16384, 16385, L - 1, L]   # noqa: E731


@pytest.mark.parametrize("L", [16 << 10, 64 << 10, 1 << 20])
def test_tail_table(plan, L):
    cases = []
    sizes = [s for s in SIZES(L) if s <= L]
    # every size as a one-piece file between full files; as the tail of a longer file; as the last file, with and
    # without a trailing pad; shards that start mid-file
    for s in sizes:
        for lengths in ([L, s, 2 * L], [2 * L + s, s], [L, L + s], [s]):
            for trailing in (False, True):
                total, pb = files_table(lengths, L, trailing)
                for first in (0, 8) if len(pb) > 8 else (0,):
                    cases.append((total, L, first, pb[first:]))
    total, pb = files_table([3 * L + s for s in sizes] + [5 * L + 7], L)      # first = 8, 16: mid-file starts
    for first in (0, 8, 16, 24):
        cases.append((total, L, first, pb[first:first + 11]))
    out = plan(["t %d %d %d %d %s" % (t, L_, f, len(p), " ".join(map(str, p))) for t, L_, f, p in cases])
    for (t, L_, f, p), line in zip(cases, out):
        want, chunks = ref_tails(t, L_, f, p)
        assert parse(line) == (want, chunks), (t, L_, f, p)
        for row, b, e, _ in want:
            assert 0 < b < e <= L_ and p[row] == b


def test_documented_shapes(plan):
    L = 64 << 10
    # a short last piece gives no entry; a trailing pad gives one out to L
    out = plan(["t %d %d 0 3 %d %d 100" % (2 * L + 100, L, L, L), "t %d %d 0 3 %d %d 100" % (3 * L, L, L, L),
                # one entry per file that does not end a piece, chunk0 = the chunks before it
                "t %d %d 0 4 1 %d 17 %d" % (4 * L, L, L, L - 1),
                # piece_bytes past the v1 length: refused, naming the piece; a layout shorter than the table too
                "t %d %d 0 2 %d 101" % (L + 100, L, L), "t %d %d 0 2 %d 5" % (L, L, L),
                "t 100 %d 0 1 50" % (1 << 32)])
    assert parse(out[0]) == ([], 0)
    assert parse(out[1]) == ([(2, 100, L, 0)], 1)
    assert parse(out[2]) == ([(0, 1, L, 0), (2, 17, L, 1), (3, L - 1, L, 2)], 3)
    assert out[3] == "bad 1" and out[4] == "bad 1" and out[5] == "bad L"
    L = 4 << 20            # a 4 MiB tail is 64 chunks: not one workgroup's work
    assert parse(plan(["t %d %d 0 2 1 %d" % (2 * L, L, L)])[0]) == ([(0, 1, L, 0)], 64)
    assert parse(plan(["t %d %d 0 2 17 %d" % (2 * L, L, L)])[0]) == ([(0, 17, L, 0)], 64)
    assert parse(plan(["t %d %d 0 2 %d %d" % (2 * L, L, CHUNK + 16, L)])[0]) == ([(0, CHUNK + 16, L, 0)], 63)


@pytest.mark.parametrize("L", [16 << 10, 64 << 10, 1 << 20])
def test_replayed_launch_stores_exactly_the_pad_ranges(plan, L):
    """Every row base alignment a stride could give (the library's are multiples of 64; the kernel aligns by address)."""
    sizes = [s for s in SIZES(L) if s <= L]
    total, pb = files_table(sizes + [L + 3], L, trailing_pad=True)
    lines, cases = [], []
    for stride, align in ((L + 256, 0), (L + 64, 0), (L + 1, 1), (L + 7, 15), (L + 24, 8), (L, 0)):
        for first in (0, 8):
            p = pb[first:]
            lines.append("p %d %d %d %d %d %d %s" % (total, L, first, len(p), stride, align, " ".join(map(str, p))))
            cases.append((first, p, stride))
    for (first, p, stride), line in zip(cases, plan(lines)):
        head, _, rows = line.partition("|")
        want, chunks = ref_tails(total, L, first, p)
        assert head.split() == [str(len(want)), str(chunks)]
        ranges = {row: "%d:%d" % (b, e) for row, b, e, _ in want}
        assert rows.split() == [ranges.get(j, "-") for j in range(len(p))], (first, stride)


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "plan_hybrid_asan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = 64 << 10
    total, pb = files_table([1, 15, 16, 17, 16383, 16385, L - 1, L, 2 * L + 5], L, trailing_pad=True)
    p = " ".join(map(str, pb))
    out = _runner(exe)(["t %d %d 0 %d %s" % (total, L, len(pb), p),
                        "p %d %d 0 %d %d 15 %s" % (total, L, len(pb), L + 7, p),
                        "t %d %d 0 %d %s" % (total - L, L, len(pb), p)])
    want, chunks = ref_tails(total, L, 0, pb)
    assert parse(out[0]) == (want, chunks) and out[2].startswith("bad ")
