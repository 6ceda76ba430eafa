"""CPU unit tests of the launch order of a v1 list in torrent_amd/csrc/tv_plan.h (list_plan, what tv_verify_list
launches), run through tests/c/plan_list_main.cpp (an ordinary executable: it also builds with
-fsanitize=address,undefined).  The rules, restated in plain Python below: entries without a slot are not launched; when
the launched entries hold the torrent's short last piece AND other pieces, the others come first in the caller's order,
then copies of the first launched piece up to a multiple of 64, then the last-piece entries in the caller's order;
otherwise the caller's order with no padding."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, LAST = 200, 199            # the shard's pieces; its last one is the torrent's short last piece (or no piece is)
SIZES = [0, 1, 63, 64, 65, 130]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_list") / "plan_list_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_list_main.cpp"), "-o", exe])

    def run(cases):
        """cases: (pieces, held or None, last or None) -> [(launch, origin)]."""
        lines = []
        for pieces, held, last in cases:
            tok = ["l", len(pieces), -1 if last is None else last, int(held is not None)] + list(pieces)
            lines.append(" ".join(map(str, tok + ([int(h) for h in held] if held is not None else []))))
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        out = r.stdout.strip().split("\n")
        assert len(out) == len(cases)
        got = []
        for line in out:
            tok = line.split()
            pairs = [tuple(map(int, t.split(":"))) for t in tok[1:]]
            assert int(tok[0]) == len(pairs)
            got.append(([p for p, _ in pairs], [o for _, o in pairs]))
        return got

    return run


def ref_plan(pieces, held, last):
    sel = [k for k in range(len(pieces)) if held is None or held[k]]
    tail = [k for k in sel if last is not None and pieces[k] == last]
    if not 0 < len(tail) < len(sel):
        return [pieces[k] for k in sel], sel, False
    origin = [k for k in sel if pieces[k] != last]
    origin += [-1] * (-len(origin) % 64)
    launch = [pieces[k] if k >= 0 else pieces[origin[0]] for k in origin]
    return launch + [last] * len(tail), origin + tail, True


def check(case, got):
    pieces, held, last = case
    launch, origin, split = ref_plan(pieces, held, last)
    assert got == (launch, origin), case
    # every launched entry exactly once, none that holds no slot
    assert sorted(o for o in got[1] if o >= 0) == [k for k in range(len(pieces)) if held is None or held[k]]
    assert all(got[0][t] == pieces[o] for t, o in enumerate(got[1]) if o >= 0)
    pad = [t for t, o in enumerate(got[1]) if o < 0]
    if not split:
        assert not pad
        return
    first = sum(1 for o in got[1] if o >= 0 and pieces[o] != last)        # the full pieces, then the padding
    assert pad == list(range(first, first + len(pad))) and (first + len(pad)) % 64 == 0 and len(pad) < 64
    assert all(got[0][t] == got[0][0] for t in pad)
    assert all(got[0][t] != last for t in range(first + len(pad))) and all(p == last for p in got[0][first + len(pad):])


def lists(n, rng):
    """(what, pieces, last) for a list of n entries."""
    full = rng.sample(range(LAST), n)                                     # distinct full pieces, any order
    out = [("no last piece", full, None), ("a full last piece", rng.sample(range(COUNT), n), None),
           ("only last-piece entries", [LAST] * n, LAST), ("the last piece is not listed", full, LAST)]
    if n:
        for what, at in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            out.append((f"the last piece {what}", full[:at] + [LAST] + full[at + 1:], LAST))
        dup = [full[k % max(1, n // 3)] for k in range(n)]                 # duplicates of full pieces
        out.append(("duplicates", dup, LAST))
        out.append(("duplicates and the last piece twice", [LAST] + dup[1:-1] + [LAST] if n > 1 else [LAST], LAST))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_launch_order(plan, n):
    rng = random.Random(n)
    cases = []
    for what, pieces, last in lists(n, rng):
        masks = [None, [0] * n, [1] * n, [rng.random() < 0.6 for _ in range(n)]]
        if last is not None and LAST in pieces:                           # the last piece holds no slot, the others do
            masks.append([p != LAST for p in pieces])
            masks.append([p == LAST for p in pieces])                     # ... and the other way round
        cases += [(pieces, m, last) for m in masks]
    got = plan(cases)
    for case, g in zip(cases, got):
        check(case, g)
    assert n == 0 or any(ref_plan(*c)[2] for c in cases) == (n > 1)       # the split form is among them


def test_documented_shapes(plan):
    got = plan([([LAST], None, LAST),                                      # the last piece alone: as listed
                ([3, LAST, 5], None, LAST),                                # split: 3, 5, 62 copies of 3, the last piece
                ([3, LAST, 5], None, None),                                # no short last piece: as listed
                ([3, LAST, 5], [1, 0, 1], LAST),                           # it holds no slot: the others as listed
                ([LAST, 3], [1, 0], LAST),
                (list(range(64)) + [LAST], None, LAST)])                   # 64 full pieces: no padding needed
    assert got[0] == ([LAST], [0])
    assert got[1] == ([3, 5] + [3] * 62 + [LAST], [0, 2] + [-1] * 62 + [1])
    assert got[2] == ([3, LAST, 5], [0, 1, 2])
    assert got[3] == ([3, 5], [0, 2])
    assert got[4] == ([LAST], [0])
    assert got[5] == (list(range(64)) + [LAST], list(range(65)))
