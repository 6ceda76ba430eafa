"""The seeded v1 kernel draw (tests/v1_kernel_fuzz.py) on the CPU: every route, every kernel form and every edge the GPU
fuzz is meant to reach occurs in at least two seeds, every seed shows several, the draws are deterministic and within
the sizes the fuzz promises, and the expectation is hashlib's."""
import hashlib

import pytest

from tests import v1_columns as vc
from tests import v1_kernel_fuzz as vf
from tests.v1_kernel_fuzz import FEATURES, KERNELS, ROUTES, SEEDS, draw, features


@pytest.fixture(scope="module")
def draws():
    return [draw(s) for s in SEEDS]


def test_every_feature_occurs_in_at_least_two_seeds(draws):
    assert SEEDS == list(range(32))
    assert {"route_" + r for r in ROUTES} | {"kernel_" + k for k in KERNELS} | {
        "short_last", "spill", "exact", "dead", "n_main_zero_window", "odd_L", "multiword"} <= set(FEATURES)
    assert set(KERNELS) == set(vc.VARIANTS) | {"auto"}
    count = {name: 0 for name in FEATURES}
    for d in draws:
        got = features(d)
        assert got <= set(FEATURES)
        assert len(got) >= 3, (d.seed, got)
        for name in got:
            count[name] += 1
    assert all(n >= 2 for n in count.values()), count
    # the streamed windows (more than 2,048 pieces, pieces of at most 448 bytes) come up in at least three seeds
    wide = [d for d in draws if d.route == "win_columns"]
    assert len(wide) >= 3 and all(d.count > vc.MIN_WIN and d.L <= 448 for d in wide)
    # every route runs under at least four kernel forms
    for r in ROUTES:
        assert len({d.kernel for d in draws if d.route == r}) >= 4, r


def test_draws_are_what_the_fuzz_promises(draws):
    for d in draws:
        assert d.L in vf.PIECE_LENGTHS and 1 <= d.last <= d.L and d.total <= vf.MAX_BYTES
        assert 1 <= d.P <= 600 or d.route == "win_columns"
        assert d.first % 8 == 0 and d.count >= 1 and d.first + d.count <= d.P
        assert 1 <= d.c <= 13
        assert len(d.payload) == len(d.staged) == d.total
        assert d.avail is None or len(d.avail) == (d.count + 7) // 8
        assert len(d.digests) == 20 * d.P or 20 * (d.P - 1) < len(d.digests) < 20 * d.P
        # flipped bytes and flipped digests both occur, and a flipped piece never matches
        flipped = [i for i in range(d.P) if d.piece(i) != d.piece(i, d.payload)]
        assert flipped and not any(d.matches(i) for i in flipped)
        want = d.expected()
        assert len(want) == d.count
        for j, i in enumerate(range(d.first, d.first + d.count)):
            slice_ = d.digests[20 * i:20 * i + 20]
            ok = len(slice_) == 20 and hashlib.sha1(d.piece(i)).digest() == slice_
            assert want[j] == int(ok and d.available(i)), (d.seed, i)
        assert d.staged_digests() == vc.digests(d.staged, d.L, d.P, d.last)[20 * d.first:20 * (d.first + d.count)]
        if d.route in ("list", "list_slots"):
            assert set(d.order) == set(range(d.first, d.first + d.count)) and len(d.order) > d.count
            assert 1 <= d.slots <= 8
        if d.route == "windowed" and d.windowed(3):
            assert d.count * d.stride() + 256 > d.window_budget(3) >= 3 * (vf.WINDOW * d.stride() + 256)


def test_draw_is_deterministic():
    for seed in (0, 3, 17):
        a, b = draw(seed), draw(seed)
        assert a == b
    assert draw(4) != draw(5)
