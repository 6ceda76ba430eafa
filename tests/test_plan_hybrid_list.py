"""CPU unit tests of the pad launch of a hybrid list call (tv_hybrid_verify_list): torrent_amd/csrc/tv_plan.h
hybrid_list_chunks / hybrid_list_chunk, which tv_hybrid_list_pad_kernel shares with tests/c/plan_hybrid_list_main.cpp (an
ordinary executable: it also builds with -fsanitize=address,undefined).  The launch is replayed workgroup by workgroup
on a host buffer of slot rows: exactly [piece_bytes, v1_len) of each listed row is stored, each byte once per listing,
vector stores 16-byte aligned, nothing else -- for every edge size, three piece lengths, three row strides, a last piece
with and without a trailing pad, a duplicate entry, and rows in an order that differs from piece order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "plan_hybrid_list_main.cpp")
K = 1024
CHUNK = 64 * K                                              # kHybridChunk

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
    exe = str(tmp_path_factory.mktemp("plan_hybrid_list") / "plan_hybrid_list_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe])
    return _runner(exe)


def sizes(L):
    return [1, 15, 16, 17, L // 2, L - 1, L]


def chunks_of(pb, v1):
    """The chunks of the range [pb, v1): 64 KiB each, counted from pb rounded down to 16."""
    return -(-(v1 - pb // 16 * 16) // CHUNK) if pb < v1 else 0


def case(L, stride, trailing):
    """Pieces of every edge size, then a short last piece (trailing: followed by a pad out to L); every piece but one
    held in a scrambled row of a pool with three rows more than pieces; listed in reverse piece order with a piece listed
    twice (and the last piece twice).  -> (query line, the most chunks, the expected text of every row)."""
    pbs = sizes(L) + [777]
    P = len(pbs)
    total = P * L if trailing else (P - 1) * L + pbs[-1]
    nrows = P + 3                                           # 11 rows: 3 is coprime, so the map below is a permutation
    row_of = {i: (3 * i + 1) % nrows for i in range(P)}
    unlisted = 4
    listed = [i for i in reversed(range(P)) if i != unlisted] + [1, P - 1]
    want = ["-"] * nrows
    chunks = 0
    for i in set(listed):
        v1 = min(L, total - i * L)
        n = listed.count(i)
        if pbs[i] < v1:
            want[row_of[i]] = "%d:%d:%d:%d" % (pbs[i], v1, n, n)
        chunks = max(chunks, chunks_of(pbs[i], v1))
    line = "p %d %d %d %d %d %s" % (total, L, stride, nrows, len(listed),
                                    " ".join("%d %d %d" % (row_of[i], i, pbs[i]) for i in listed))
    return line, chunks, want


LENGTHS = [16 * K, 64 * K, 256 * K]


@pytest.mark.parametrize("L", LENGTHS)
def test_replayed_list_launch_stores_exactly_the_listed_ranges(plan, L):
    cases = [case(L, (L + 63) // 64 * 64 + extra, trailing) for extra in (0, 64, 256) for trailing in (False, True)]
    for (line, chunks, want), got in zip(cases, plan([c[0] for c in cases])):
        head, _, body = got.partition("|")
        assert int(head) == chunks
        assert body.split() == want, line[:60]
    # the 1-byte piece of 256 KiB pieces has four chunks (the first begins at byte 1); a full piece has none
    assert max(c[1] for c in cases) == (4 if L == 256 * K else 1)


def test_chunk_counts(plan):
    L = 256 * K
    total = 3 * L + 100                                     # piece 3 is a short last piece: no pad after it
    cases = [(1, 0, 4), (16, 0, 4), (17, 0, 4), (L - CHUNK, 1, 1), (L - CHUNK - 1, 1, 2), (L, 2, 0), (100, 3, 0),
             (50, 3, 1), (1, 4, 0)]                         # (piece 4 lies past the torrent's end: no v1 bytes)
    out = plan(["c %d %d %d %d" % (pb, total, L, piece) for pb, piece, _ in cases])
    assert [int(x) for x in out] == [want for _, _, want in cases]
    for pb, piece, want in cases:
        assert want == chunks_of(pb, max(0, min(L, total - piece * L)))


def test_a_row_outside_the_payload_is_skipped(plan):
    L = 16 * K
    out = plan(["p %d %d %d 2 2 0 0 100 7 1 100" % (2 * L, L, L)])   # entry 1 names row 7 of a 2-row payload
    assert out[0].split() == ["1", "|", "100:%d:1:1" % L, "-"]


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "plan_hybrid_list_asan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [case(L, L + extra, trailing) for L in (16 * K, 256 * K) for extra in (0, 64) for trailing in (False, True)]
    for (line, chunks, want), got in zip(cases, _runner(exe)([c[0] for c in cases])):
        head, _, body = got.partition("|")
        assert int(head) == chunks and body.split() == want
