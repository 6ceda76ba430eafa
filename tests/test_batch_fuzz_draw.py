"""The seeded batch draw (tests/batch_fuzz.py) on the CPU: the draws are deterministic and within the sizes the GPU fuzz
(tests/test_gpu_batch_fuzz.py) promises, the edges it is meant to reach occur, and the expectation is hashlib's."""
import hashlib

import pytest

from tests import batch_fuzz as bf


@pytest.fixture(scope="module")
def draws():
    return [bf.draw(s) for s in bf.SEEDS]


def test_draws_are_what_the_fuzz_promises(draws):
    assert bf.SEEDS == list(range(24))
    for ts in draws:
        assert 1 <= len(ts) <= bf.MAX_TORRENTS
        assert sum(t.total for t in ts) <= bf.MAX_BYTES
        for t in ts:
            whole = -(-t.total // t.L)
            assert t.L in bf.PIECE_LENGTHS and 0 <= whole <= bf.MAX_PIECES and whole <= t.n <= whole + 3
            assert len(t.payload) == len(t.staged) == t.total
            assert 20 * (t.n - 1) < len(t.digests) <= 20 * t.n or t.n == 0
            assert t.avail is None or len(t.avail) == t.n
            want = t.expected()
            assert len(want) == t.n
            for i in range(t.n):
                n = t.piece_len(i)
                d = t.digests[20 * i:20 * i + 20]
                ok = (len(d) == 20 and i * t.L + n <= t.total
                      and hashlib.sha1(t.staged[i * t.L:i * t.L + n]).digest() == d)
                assert want[i] == int(ok and (t.avail is None or bool(t.avail[i]))), i
            assert not any(want[i] for i in t.flipped)                    # a flipped piece never matches


def test_the_edges_occur(draws):
    every = [t for ts in draws for t in ts]
    assert {t.L for t in every} == set(bf.PIECE_LENGTHS)
    assert sum(1 for t in every if t.n == 0) >= 2                          # torrents without pieces
    assert sum(1 for t in every if len(t.digests) % 20) >= 2               # ragged digest strings
    assert sum(1 for t in every if t.n > -(-t.total // t.L)) >= 2          # more digests than pieces
    assert sum(1 for t in every if t.total % t.L) >= 10                    # short last pieces
    assert sum(1 for t in every if t.avail and not all(t.avail)) >= 10
    assert sum(1 for t in every if t.flipped) >= 10
    assert sum(1 for ts in draws if len({t.L for t in ts}) >= 3) >= 10     # mixed piece lengths in one batch
    assert any(sum(t.n for t in ts) > 64 for ts in draws) and any(sum(t.n for t in ts) < 32 for ts in draws)
    # the plan of some draw cuts a group early (padding) under both spans
    for span in (32, 64):
        assert any(-1 in bf.ref_plan([x for t in ts for x in t.lens()], span)[1] for ts in draws)


def test_draw_is_deterministic():
    for seed in (0, 3, 17):
        a, b = bf.draw(seed), bf.draw(seed)
        assert a == b
    assert bf.draw(4) != bf.draw(5)
