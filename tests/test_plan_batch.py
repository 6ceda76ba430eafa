"""CPU unit tests of the launch order and group geometry of a batch in torrent_amd/csrc/tv_plan.h (batch_plan, what
tv_batch_verify launches), run through tests/c/plan_batch_main.cpp (an ordinary executable: it also builds with
-fsanitize=address,undefined).  The rules are restated in plain Python in tests/batch_fuzz.py ref_plan: entries sorted
by SHA-1 block count, longest first, stably; groups of `span` launch positions; a group closed early -- and padded with
copies of its own last entry -- when the next entry would make nb_max - nfull_min exceed max(8, nb_max / 8); per group
{fast_end, end, nb_min} = {min len / 64, max blocks, min blocks}."""
import os
import random
import shutil
import subprocess

import pytest

from tests.batch_fuzz import CUT_BLOCKS, CUT_SHARE, nblocks, ref_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_batch") / "plan_batch_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_batch_main.cpp"), "-o", exe])

    def run(cases):
        """cases: (span, lens) -> [(launch, origin, groups)]."""
        lines = [" ".join(map(str, ["b", span, len(lens)] + list(lens))) for span, lens in cases]
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        out = r.stdout.strip().split("\n")
        assert len(out) == len(cases)
        got = []
        for line in out:
            tok = line.split()
            m, g = int(tok[0]), int(tok[1])
            assert len(tok) == 2 + m + g
            pos = [tuple(map(int, t.split(":"))) for t in tok[2:2 + m]]
            got.append(([e for e, _ in pos], [o for _, o in pos], [tuple(map(int, t.split(":"))) for t in tok[2 + m:]]))
        return got

    return run


def check(case, got):
    span, lens = case
    launch, origin, groups = got
    assert got == ref_plan(lens, span), case
    n = len(lens)
    # launch minus padding is a permutation of the input, and every answered position hashes the entry it answers
    assert sorted(o for o in origin if o >= 0) == list(range(n))
    assert all(launch[t] == o for t, o in enumerate(origin) if o >= 0)
    # block counts do not ascend; equal counts keep the input's order (the sort is stable)
    real = [o for o in origin if o >= 0]
    assert all(nblocks(lens[a]) >= nblocks(lens[b]) for a, b in zip(real, real[1:]))
    assert all(a < b for a, b in zip(real, real[1:]) if nblocks(lens[a]) == nblocks(lens[b]))
    # groups are span positions; only the last may be short, and it is not padded
    assert len(groups) == -(-len(launch) // span)
    assert n == 0 or len(launch) % span == 0 or origin[len(launch) // span * span:].count(-1) == 0
    for g, (fast_end, end, nb_min) in enumerate(groups):
        members = launch[g * span:(g + 1) * span]
        assert members
        ml = [lens[e] for e in members]
        assert (fast_end, end, nb_min) == (min(x // 64 for x in ml), max(map(nblocks, ml)), min(map(nblocks, ml)))
        assert all(fast_end * 64 <= x for x in ml)                       # no raw-block load leaves a member's bytes
        assert end - fast_end <= max(CUT_BLOCKS, end // CUT_SHARE)        # the cut rule
        # padding: copies of a member of the group (its last real entry), after the real entries
        o = origin[g * span:(g + 1) * span]
        k = len([x for x in o if x >= 0])
        assert k >= 1 and all(x >= 0 for x in o[:k]) and all(x < 0 for x in o[k:])
        assert all(e == members[k - 1] for e in members[k:])
        if k < len(o) or (len(members) < span and g + 1 < len(groups)):   # closed early: the next entry would break the rule
            nxt = launch[(g + 1) * span]
            assert end - min(fast_end, lens[nxt] // 64) > max(CUT_BLOCKS, end // CUT_SHARE)


@pytest.mark.parametrize("span", [32, 64])
def test_shapes(plan, span):
    rng = random.Random(span)
    cases = []
    for n in (0, 1, span - 1, span, span + 1, 3 * span + 5):
        cases.append((span, [4096] * n))                                   # all lengths equal
        # two classes far apart (257 against 2 blocks): no group mixes them
        cases.append((span, [16384 if k % 3 else 100 for k in range(n)]))
        # lengths differing by one block inside a group
        cases.append((span, [4096 + 64 * (k % 2) for k in range(n)]))
        cases.append((span, [rng.choice([55, 56, 119, 120, 4096]) for _ in range(n)]))
    cases.append((span, list(range(131))))                                 # every length of 0 .. 130 bytes
    cases.append((span, list(range(130, -1, -1))))
    got = plan(cases)
    for case, g in zip(cases, got):
        check(case, g)
    for (sp, lens), (launch, origin, groups) in zip(cases, got):
        if lens and set(lens) == {16384, 100}:
            for g in range(len(groups)):
                assert len({lens[e] for e in launch[g * sp:(g + 1) * sp]}) == 1
        if lens and set(lens) == {4096, 4160} and len(lens) <= span:
            assert len(groups) == 1 and -1 not in origin                   # one block apart: one group, no padding
    # a zero-length piece still has one block
    assert plan([(span, [0])])[0] == ([0], [0], [(0, 1, 1)])


def test_documented_shapes(plan):
    got = plan([(32, [100, 16384, 100]),           # the long piece first, padded to a group of its own, then the short
                (64, [64] * 64 + [55])])          # a full group, then the rest
    assert got[0] == ([1] * 32 + [0, 2], [1] + [-1] * 31 + [0, 2], [(256, 257, 257), (1, 2, 2)])
    assert got[1] == (list(range(65)), list(range(65)), [(1, 2, 2), (0, 1, 1)])


def test_random_draws_keep_the_invariants(plan):
    rng = random.Random(20240)
    cases = []
    for _ in range(200):
        span = rng.choice([32, 64])
        classes = rng.sample([1, 55, 56, 64, 100, 119, 120, 4096, 16384, 16400, 65536, 262144], rng.randrange(1, 6))
        lens = []
        for _ in range(rng.randrange(0, 4 * span)):
            L = rng.choice(classes)
            lens.append(L if rng.random() < 0.8 else rng.randrange(0, L + 1))
        cases.append((span, lens))
    for case, g in zip(cases, plan(cases)):
        check(case, g)
    assert any(-1 in g[1] for g in plan(cases))                            # early cuts are among them
