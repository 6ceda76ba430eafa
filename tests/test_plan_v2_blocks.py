"""CPU unit tests of the v2 block item planning in torrent_amd/csrc/tv_plan.h (v2_block_items, v2_block_scatter), run
through tests/c/plan_v2_blocks_main.cpp (an ordinary executable: it also builds with -fsanitize=address,undefined):
which blocks of which entries a tv_v2_leaf_hashes / tv_v2_check_blocks launch hashes, and how its per-item results
come back as per-entry bit rows.  The expected values are restated here in plain Python."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 16384

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_v2_blocks") / "plan_v2_blocks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_v2_blocks_main.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = r.stdout.strip().split("\n")
        assert len(out) == len(lines)
        return out

    return run


def bit(row: bytes, i: int) -> bool:
    return bool(row[i >> 3] & (0x80 >> (i & 7)))


def ref_items(W, nbytes, want, skip):
    """[(entry, leaf, len)] in entry order, leaves ascending: wanted positions that hold at least one byte."""
    out = []
    for k, b in enumerate(nbytes):
        if skip and skip[k]:
            continue
        for i in range(W):
            if i * LEAF < b and (want is None or bit(want[k], i)):
                out.append((k, i, min(LEAF, b - i * LEAF)))
    return out


def ref_scatter(W, n, items, results):
    rows = [bytearray((W + 7) // 8) for _ in range(n)]
    for (k, i, _), r in zip(items, results):
        if r:
            rows[k][i >> 3] |= 0x80 >> (i & 7)
    return [bytes(r) for r in rows]


def query(W, cap, nbytes, want, skip, results):
    words = [0] * ((len(results) + 63) // 64)
    for t, r in enumerate(results):
        if r:
            words[t >> 6] |= 1 << (t & 63)
    tok = ["b", W, cap, len(nbytes), int(want is not None), int(skip is not None)] + list(nbytes)
    if want is not None:
        tok += [w.hex() for w in want]
    if skip is not None:
        tok += [int(s) for s in skip]
    tok += [len(words)] + ["%x" % w for w in words]
    return " ".join(map(str, tok))


def parse(line):
    head, _, rows = line.partition("|")
    tok = head.split()
    items = [tuple(map(int, t.split(":"))) for t in tok[1:]]
    assert int(tok[0]) == len(items)
    return items, [bytes.fromhex(r) for r in rows.split()]


def want_rows(kind, W, n, rng):
    pitch = (W + 7) // 8
    if kind == "null":
        return None
    if kind == "zeros":
        return [bytes(pitch)] * n
    if kind == "ones":           # the spare bits of the last byte included: they name no block
        return [b"\xff" * pitch] * n
    return [rng.randbytes(pitch) for _ in range(n)]


def test_items_and_scatter_over_a_grid(plan):
    rng = random.Random(5)
    cases = []
    for W in (1, 2, 4, 8, 16, 64, 256, 1024):
        L = W * LEAF
        sizes = sorted({1, 55, LEAF - 1, LEAF, min(L, LEAF + 1), L // 2 + 1 if W > 1 else 1, L - 1, L})
        for kind in ("null", "zeros", "ones", "random"):
            for n in (0, 1, 3, len(sizes)):
                nbytes = [sizes[(k * 3 + n) % len(sizes)] for k in range(n)] if n != len(sizes) else list(sizes)
                for skipped in (False, True):
                    want = want_rows(kind, W, n, rng)
                    skip = [rng.random() < 0.4 for _ in range(n)] if skipped else None
                    items = ref_items(W, nbytes, want, skip)
                    for res in ("all", "none", "random"):
                        results = [res == "all" or (res == "random" and rng.random() < 0.5) for _ in items]
                        cases.append((W, nbytes, want, skip, items, results))
    assert len(cases) > 500
    out = plan([query(W, 1 << 22, nb, want, skip, results) for W, nb, want, skip, items, results in cases])
    for (W, nbytes, want, skip, items, results), line in zip(cases, out):
        got_items, got_rows = parse(line)
        what = (W, nbytes, None if want is None else [w.hex() for w in want], skip)
        assert got_items == items, what
        assert got_rows == ref_scatter(W, len(nbytes), items, results), what
        for k, row in enumerate(got_rows):                 # never a bit that was not wanted or holds no byte
            for i in range(8 * len(row)):
                if bit(row, i):
                    assert i < W and i * LEAF < nbytes[k] and (want is None or bit(want[k], i))


def test_documented_shapes(plan):
    W, L = 64, 64 * LEAF
    nbytes = [1, LEAF, LEAF + 1, L - 1, L]                 # 1 + 1 + 2 + 64 + 64 items
    items = ref_items(W, nbytes, None, None)
    assert len(items) == 132
    got, rows = parse(plan([query(W, 132, nbytes, None, None, [True] * 132)])[0])
    assert got == items
    assert got[0] == (0, 0, 1) and got[3] == (2, 1, 1) and got[67] == (3, 63, LEAF - 1)
    assert [r.hex() for r in rows] == ["80" + "00" * 7, "80" + "00" * 7, "c0" + "00" * 7, "ff" * 8, "ff" * 8]
    # W = 1: one byte per row, one item per entry
    got, rows = parse(plan([query(1, 10, [1, LEAF, 77], None, None, [True, False, True])])[0])
    assert got == [(0, 0, 1), (1, 0, LEAF), (2, 0, 77)] and [r.hex() for r in rows] == ["80", "00", "80"]
    # a wanted position past the piece's bytes gives no item, and its bit stays 0
    got, rows = parse(plan([query(8, 10, [LEAF + 5], [b"\x0f"], None, [])])[0])
    assert got == [] and rows == [b"\x00"]
    got, rows = parse(plan([query(8, 10, [LEAF + 5], [b"\x4f"], None, [True])])[0])
    assert got == [(0, 1, 5)] and rows == [b"\x40"]


def test_item_cap(plan):
    W = 256
    nbytes = [W * LEAF] * 4                                # 1,024 items
    out = plan([query(W, 1024, nbytes, None, None, [True] * 1024),
                query(W, 1023, nbytes, None, None, [True] * 1024),
                query(W, 0, nbytes, None, None, []),
                query(W, 0, nbytes, [bytes(W // 8)] * 4, None, []),          # nothing wanted: no item, within any cap
                query(W, 256, nbytes, None, [1, 1, 0, 1], [True] * 256)])    # skipped entries do not count
    assert parse(out[0])[0] == ref_items(W, nbytes, None, None)
    assert out[1] == "over" and out[2] == "over"
    assert parse(out[3]) == ([], [bytes(W // 8)] * 4)
    items, rows = parse(out[4])
    assert len(items) == 256 and {k for k, _, _ in items} == {2}
    assert rows == [bytes(32), bytes(32), b"\xff" * 32, bytes(32)]
