"""(CPU) The shape list of the streamed SHA-1 column sweep (tests/v1_columns.py) is as deep as it claims: every class of
classes() at every column width and every piece count, the loop and ring residues the widths are chosen for, and the
restated stream geometry equal to the library's (tv_plan.h stream_geometry through tests/c/plan_stream_main.cpp)."""
import os
import random
import shutil
import subprocess

import pytest

from tests import v1_columns as vc
from tests.v1_columns import CLASSES, CS, PS, VARIANTS, classes, lasts, lengths, nblocks, shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variants_are_the_six_kernel_forms():
    assert VARIANTS == {"lane3": (1, 0, 2), "lanepairs": (1, 0, 1), "split1": (2, 1, 0), "split2": (2, 2, 0),
                        "twin1": (4, 0, 0), "twin2": (4, 2, 0)}


def test_widths_reach_every_loop_and_ring_residue():
    assert CS == [1, 2, 3, 4, 5, 6, 7, 8, 13]
    assert {(c - 1) % 6 for c in CS} == set(range(6))       # every exit of the helpers' six-block loop
    assert any(c > 6 for c in CS) and any(c > 12 for c in CS)   # its back edge, and a second lap
    assert {c % 3 for c in CS} == {0, 1, 2}                 # the lane kernel's 3-deep ring
    assert {c % 4 for c in CS} == {0, 1, 2, 3}              # ... and its ring of two pairs
    assert {c % 2 for c in CS} == {0, 1}                    # the twin rounds loop: two blocks per trip


@pytest.mark.parametrize("c", CS)
def test_every_class_at_every_width(c):
    C = 64 * c
    assert lengths(C)[:7] == [C, 2 * C, 3 * C, 3 * C + 1, 3 * C + 55, 3 * C + 56, 3 * C + 63]
    assert lengths(C)[7:] == ([2 * C + 64 + 56] if c >= 2 else [])
    pairs = shapes(c)
    short = [(L, last) for L, last in pairs if last < L]
    assert len(short) <= 83 and len(pairs) == len(short) + len(lengths(C))
    assert all((L, L) in pairs for L in lengths(C))         # every length also without a short piece
    assert {-(-L // C) for L, _ in pairs} == {1, 2, 3, 4}   # one to four columns
    for L in lengths(C):
        assert lasts(C, L) == sorted(set(lasts(C, L))) and all(1 <= x <= L for x in lasts(C, L))
    seen = {name: 0 for name in CLASSES}
    for L, last in short:
        got = classes(C, L, last)
        assert got <= set(CLASSES) and got
        assert ("pad_in_col" in got) != ("spill" in got)    # the padding either stays in the data's column or not
        assert not ({"dead", "dead2"} <= got)
        assert ("in_last_col" in got) != bool(got & {"dead", "dead2"})
        for name in got:
            seen[name] += 1
    assert all(n >= 1 for n in seen.values()), seen
    # the sweep crosses every shape with every piece count, so each count sees each class
    assert PS == (1, 33, 65, 130)
    assert all(classes(C, L, L) == set() for L in lengths(C))


def test_classes_on_worked_examples():
    C = 128                                                  # columns of two blocks
    # 120 bytes: the data ends in column 0's second block, the length field no longer fits: block 2 is in column 1
    assert nblocks(120) == 3 and {"spill", "dead"} <= classes(C, 3 * C, 120)
    # 119 bytes: both blocks in column 0, columns 1 and 2 have nothing to do
    assert nblocks(119) == 2 and {"pad_in_col", "dead2"} <= classes(C, 3 * C, 119)
    # a last piece that ends with column 0: its padding block opens column 1
    assert {"exact", "spill", "dead"} <= classes(C, 3 * C, C)
    assert {"exact", "spill", "in_last_col"} <= classes(C, 3 * C + 1, 3 * C)   # ... or the final (fourth) column
    assert "exact" not in classes(C, 3 * C, C + 1) and "exact" not in classes(C, 3 * C, C - 8)
    assert {"one_block", "dead2", "pad_in_col"} <= classes(C, 3 * C, 1)
    assert "one_block" not in classes(C, C, 1)               # a single column
    assert "in_last_col" in classes(C, 3 * C, 3 * C - 1) and "parity" in classes(C, 3 * C, 3 * C - 64)
    assert "parity" not in classes(C, 3 * C, 3 * C - 1)


def test_corrupted_pieces_move_through_the_groups():
    for P in PS + (2049, 2113):
        bad = vc.corrupted(P)
        assert P - 1 in bad and all(0 <= i < P for i in bad)
        assert {i // 32 for i in bad} >= set(range(P // 32))              # every whole group of 32 has one
    assert len({i % 32 for i in vc.corrupted(130)}) == len(vc.corrupted(130))
    case = vc.Case(192, 65, 33)
    diff = [k for k in range(case.total) if case.payload[k] != case.flipped[k]]
    assert diff == [i * 192 + (65 if i == 32 else 192) - 1 for i in case.bad]
    assert vc.bits(vc.bitfield(case.bits(case.bad)), 33) == case.bits(case.bad)
    # the windowed cases' list: pieces around the word and window edges (2048 is also the last of 2,049 pieces)
    assert vc.Case(64, 1, 2049, bad=(0, 63, 64, 2047, 2048, 2048)).bad == [0, 63, 64, 2047, 2048]


def test_window_budget_gives_the_columns_the_sweep_asks_for():
    for c in CS:
        C = 64 * c
        for L in (3 * C, 3 * C + 56):
            for P in (2049, 2050, 2048 + 65):
                assert vc.stream_geometry(L, P, vc.column_budget(C)) == (C, 2048)
                assert vc.host_units(L, P, 0, vc.column_budget(C)) == 2 * -(-L // C)
                assert vc.host_units(L, P, C, 0) == -(-L // C)
    assert vc.stream_column(65539, 97, 0) == 65536 and vc.stream_column(100, 5, 4096) == 128
    assert vc.stream_column(1000, 5, 1) == 64


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_restated_stream_geometry_equals_the_library(tmp_path):
    exe = str(tmp_path / "plan_stream_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_stream_main.cpp"), "-o", exe])
    K, M, G = 1 << 10, 1 << 20, 1 << 30
    cases = [(M, 16384, G // 2, 2048), (M, 16384, 2 * G, 2048), (M, 16384, G // 4, 2048), (M, 16384, G, 512),
             (4096, 5000, G, 2048), (4096, 5000, 1, 2048), (G, 3, G, 2048), (M, 160, 2 * (160 * (256 * K + 256) + 256), 64)]
    cases += [(L, P, vc.column_budget(64 * c), 2048) for c in CS for L in lengths(64 * c)
              for P in (1, 130, 2048, 2049, 2113, 5000)]
    rng = random.Random(7)
    for _ in range(4000):
        cases.append((rng.randrange(1, 96 * M), rng.randrange(1, 70000), rng.randrange(8 * G), rng.choice([512, 2048])))
        cases.append((rng.randrange(1, 5000), rng.randrange(1, 5000), rng.randrange(16 * M), rng.choice([64, 2048])))
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % q for q in cases), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    out = [tuple(map(int, ln.split())) for ln in r.stdout.split("\n") if ln]
    assert len(out) == len(cases)
    for (L, count, budget, min_win), got in zip(cases, out):
        assert vc.stream_geometry(L, count, budget, min_win) == got, (L, count, budget, min_win)
    assert out[0] == (124 * K, 2048) and out[4] == (4096, 5000) and out[5] == (64, 2048)   # tests/c/plan_test.cpp's


def test_workgroup_counts_tell_the_forms_apart():
    """tv_launch_verify's grids restated: 130 pieces with a short last piece, and a final window of the short piece."""
    got = {v: vc.workgroups(v, 130, True) for v in VARIANTS}
    assert got == {"lane3": 1, "lanepairs": 1, "split1": 4, "split2": 3, "twin1": 6, "twin2": 4}
    assert {v: vc.workgroups(v, 1, True) for v in VARIANTS} == dict.fromkeys(VARIANTS, 1)
    assert vc.workgroups("twin1", 65, False) == 3 and vc.workgroups("split2", 65, False) == 1
    assert vc.workgroups("lane3", 258, True) == 2 and vc.workgroups("lane3", 256, False) == 1
