"""CPU unit test of the index rules a creation stream adds to torrent_amd/csrc/tv_plan.h (v2s_tab_words, v2s_hash_words,
v2s_hash_base, v2s_hash_word, v2s_nodes_b_base), run through tests/c/plan_stream_hash_main.cpp (an ordinary executable:
it also builds with -fsanitize=address,undefined).  A v2 stream's device table holds three rows of `count` words and then
eight hash words per piece, SoA [8][wcount] window after window: a verify stream's expected roots, a creation stream's
computed ones, which tv_stream_hash_end reads back through v2s_hash_word.  The rule is checked against a brute-force
restatement that lays the windows' tables out one after another, word by word."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "plan_stream_hash_main.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

COUNTS = [1, 63, 64, 65, 130]
WINDOWS = [64, 128]
COLUMNS = [1, 2, 16]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_stream_hash") / "plan_stream_hash_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, SRC, "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines)
        return out
    return run


def brute(count: int, wn: int, ncol: int):
    """The table written out word by word: rows of piece bytes, tree leaves and top-tree widths, then every window's
    [8][wcount] hash rows in window order.  -> (words, hash words, [(window base, B base)], {(j, q): hash-region word})."""
    words = []                                     # what each word of the table holds
    for row in ("bytes", "leaves", "widths"):
        words += [(row, j) for j in range(count)]
    hash0 = len(words)
    windows = []
    for j0 in range(0, count, wn):
        wcount = min(wn, count - j0)
        base = len(words)
        for q in range(8):
            words += [("hash", j0 + r, q) for r in range(wcount)]
        # level buffer A of the window's top tree holds 8 words for each of its wcount x ncol column nodes; B follows it
        windows.append((base, sum(8 for _ in range(wcount * ncol))))
    where = {(w[1], w[2]): k - hash0 for k, w in enumerate(words) if w[0] == "hash"}
    return len(words), len(words) - hash0, windows, where


def test_the_hash_rows_of_a_stream_table(plan):
    cases = [(n, wn, ncol) for n in COUNTS for wn in WINDOWS for ncol in COLUMNS]
    out = plan(["r %d %d %d" % c for c in cases])
    for (count, wn, ncol), line in zip(cases, out):
        tok = line.split()
        words, hash_words, windows, where = brute(count, wn, ncol)
        assert (int(tok[0]), int(tok[1])) == (words, hash_words) == (11 * count, 8 * count)
        at = 2
        got_windows = []
        while tok[at] == "w":
            got_windows.append((int(tok[at + 1]), int(tok[at + 2])))
            at += 3
        assert got_windows == windows, (count, wn, ncol)
        assert tok[at] == "i"
        idx = [int(x) for x in tok[at + 1:]]
        assert len(idx) == 8 * count
        for j in range(count):
            for q in range(8):
                assert idx[8 * j + q] == where[(j, q)], (count, wn, ncol, j, q)
        # every word of the region belongs to exactly one (piece, word): the windows' tables tile it
        assert sorted(idx) == list(range(8 * count))
        # a window's base is where its own [8][wcount] table starts: word q of its piece r is base + q * wcount + r
        for k, (base, _) in enumerate(windows):
            j0, wcount = k * wn, min(wn, count - k * wn)
            for q in (0, 7):
                for r in (0, wcount - 1):
                    assert base - 3 * count + q * wcount + r == where[(j0 + r, q)]
