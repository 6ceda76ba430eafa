"""(CPU, slow) The long-piece shapes of tests/long_pieces.py are what they claim, the C oracle hashes them as hashlib
does, and the restated stream geometry equals the library's.

The GPU parity tests, smoke() and bench.py trust oracle/sha1_oracle.c, and before this file it had never hashed a piece
of 2^29 bytes either: a wrong high length word in the oracle would have agreed with no kernel, or with a kernel that was
wrong in the same way."""
import os
import shutil
import subprocess

import pytest

from tests import long_pieces as lp
from tests import synth
from tests import v1_columns as vc
from tests.long_pieces import BOTH, EDGE, RES

pytestmark = pytest.mark.slow
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def test_shape_facts():
    assert EDGE == 1 << 29 and RES == (EDGE, 3, EDGE - 1) and BOTH == (EDGE + 65, 3, EDGE)
    # the bit length that ends each message: (high word, low word)
    assert lp.length_words(RES.L) == (1, 0)                          # exactly 2^32 bits
    assert lp.length_words(RES.last) == (0, 0xFFFFFFF8)              # the control just below the edge
    assert lp.length_words(EDGE - 1)[0] == 0 and lp.length_words(EDGE)[0] == 1   # no shorter piece has a high word
    assert lp.length_words(BOTH.L) == (1, 8 * 65) and BOTH.L % 64 == 1
    assert lp.length_words(BOTH.last) == (1, 0)
    # blocks: a full 2^29-byte piece ends with a data-free padding block; the piece one byte shorter has as many (63
    # bytes and the 0x80 fill its last data block, the length needs one more), two of them padded
    assert vc.nblocks(RES.L) == vc.nblocks(RES.last) == (1 << 23) + 1 and RES.last // 64 == (1 << 23) - 1
    assert vc.nblocks(BOTH.L) == (1 << 23) + 2 and vc.nblocks(BOTH.last) == (1 << 23) + 1
    assert vc.nblocks(EDGE) > 1 << 23                                # a per-piece block counter past 2^23
    # the corrupted byte: the last of piece 1, past 2^29 - 2 in its piece
    for s in (RES, BOTH):
        assert lp.total(s) == 2 * s.L + s.last and lp.piece_len(s, 2) == s.last < s.L
        assert lp.bad_offset(s) == 2 * s.L - 1 and lp.bad_offset(s) % s.L >= EDGE - 1
    assert lp.WANT == bytes([0b10100000])
    # BOTH streamed with no chunk option: columns of one ring slot, nine of them, one row per request
    assert lp.stream_column is vc.stream_column
    assert lp.columns(BOTH) == (64 * MiB, 9, 27) and vc.SLOT == 64 * MiB
    assert BOTH.last == 8 * vc.SLOT                                  # the last piece ends with the eighth column
    C = vc.SLOT
    assert {"exact", "spill", "in_last_col"} <= vc.classes(C, BOTH.L, BOTH.last)
    assert 8 * C // 64 == 1 << 23                                    # blk_begin of the ninth column's launch
    assert BOTH.L - 8 * C == 65                                      # ... which holds 65 bytes of pieces 0 and 1
    assert vc.host_units(BOTH.L, BOTH.P, 0, 0) == 9                  # (tv_verify_host's launches, the same columns)


@pytest.mark.parametrize("shape", [RES, BOTH], ids=["res", "both"])
def test_oracle_equals_hashlib(oracle, shape):
    L, P, last = shape
    total = lp.total(shape)
    good, flipped = lp.expected(shape)
    payload = synth.fill(lp.SEED, 0, total)
    assert bytes(payload[:64]) == bytes(oracle.synth_fill(lp.SEED, 0, 64))
    assert bytes(payload[-64:]) == bytes(oracle.synth_fill(lp.SEED, total - 64, 64))
    pieces = lp.digests(shape)
    assert oracle.hash_pieces(payload, total, L, P, threads=3) == pieces
    assert oracle.synth_piece_digests(lp.SEED, total, L, P, threads=3) == pieces
    assert oracle.verify_linear(payload, total, L, pieces) == lp.pack([1, 1, 1])
    payload[lp.bad_offset(shape)] ^= lp.FLIP
    assert bytes([payload[lp.bad_offset(shape)]]) == lp.bad_byte(shape)
    assert oracle.verify_linear(payload, total, L, pieces) == lp.WANT
    assert oracle.hash_pieces(payload, total, L, P, first=lp.BAD, count=1) == flipped != good[lp.BAD]
    assert oracle.verify_linear(payload, total, L, lp.digests_flipped(shape)) == lp.pack([1, 1, 1])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_library_geometry_equals_the_restated(tmp_path):
    """tv_plan.h stream_geometry (tv_verify_host's columns) through tests/c/plan_stream_main.cpp, as
    tests/test_v1_columns_shapes.py drives it: a piece longer than a ring slot gets columns of one slot."""
    exe = str(tmp_path / "plan_stream_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_stream_main.cpp"), "-o", exe])
    G = 1 << 30
    cases = [(s.L, n, budget, 2048) for s in (RES, BOTH) for n in (1, 3) for budget in (G, 8 * G, G // 8)]
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % q for q in cases), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    out = [tuple(map(int, ln.split())) for ln in r.stdout.split("\n") if ln]
    assert len(out) == len(cases)
    for (L, count, budget, min_win), got in zip(cases, out):
        assert vc.stream_geometry(L, count, budget, min_win) == got, (L, count, budget)
    assert out[cases.index((BOTH.L, 3, G, 2048))] == (64 * MiB, 3) == (lp.columns(BOTH)[0], BOTH.P)
    assert out[cases.index((RES.L, 3, G, 2048))] == (64 * MiB, 3)
