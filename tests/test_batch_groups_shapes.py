"""The designed batches (tests/batch_groups.py) on the CPU: through batch_fuzz.ref_plan every ladder is the one group it
was built for, the ladder grid, the staircase and the crowd reach the group shapes tests/test_gpu_batch_groups.py is
meant to run, and the expectation is hashlib's.  Conditions on the shapes, not measurements."""
import hashlib

import pytest

from tests import batch_fuzz as bf
from tests import batch_groups as bg

SPANS = (32, 64)


def _groups(ts, span):
    """-> (launch, origin, groups, members): members[g] = the entries of group g without its padding."""
    lens = bg.all_lens(ts)
    launch, origin, groups = bf.ref_plan(lens, span)
    members = [[k for k in origin[g * span:(g + 1) * span] if k >= 0] for g in range(len(groups))]
    return lens, launch, origin, groups, members


@pytest.fixture(scope="module")
def ladder_plans():
    """{(span, nb_max, T): (lens, groups)} over the grid, from the lengths alone."""
    out = {}
    for span in SPANS:
        for nb_max, T in bg.ladder_grid():
            lens = bg.ladder_lens(span, nb_max, T)
            launch, origin, groups = bf.ref_plan(lens, span)
            assert launch == origin == list(range(span))          # one full group, in the ladder's own order
            out[span, nb_max, T] = (lens, groups)
    return out


@pytest.fixture(scope="module")
def stair():
    return bg.staircase()


@pytest.fixture(scope="module")
def crowd():
    return bg.crowd()


def test_the_ladder_grid_is_the_issue_s():
    grid = bg.ladder_grid()
    assert len(grid) == len(set(grid)) == 53
    for nb_max in (2, 3, 9, 10, 41, 64):
        assert bg.cut_of(nb_max) == 8
        assert [T for nb, T in grid if nb == nb_max] == list(range(min(7, nb_max - 1) + 1))
    for nb_max in (257, 258):
        assert bg.cut_of(nb_max) == 32
        assert [T for nb, T in grid if nb == nb_max] == [0, 1, 2, 3, 16, 29, 30, 31]
    assert max(sum(bg.ladder_lens(64, nb, T)) for nb, T in grid) <= 64 * 16512        # 64 x 16 KiB and a block: ~1 MiB


def test_every_ladder_is_one_group_of_its_geometry(ladder_plans):
    for (span, nb_max, T), (lens, groups) in ladder_plans.items():
        assert len(lens) == span and min(lens) > 0
        assert groups == [bg.ladder_geom(span, nb_max, T)], (span, nb_max, T)
        fast_end, end, nb_min = groups[0]
        assert (end, end - nb_min) == (nb_max, T)
        nbs = [bf.nblocks(n) for n in lens]
        assert sorted(set(nbs)) == list(range(nb_max - T, nb_max + 1))                # exactly T + 1 block counts
        assert (nbs[0], nbs[-1]) == (nb_max, nb_max - T)                              # the extremes at the group's ends
        assert all(fast_end * 64 <= n for n in lens)
        rems = {n % 64 for n in lens}
        assert any(r <= 55 for r in rems) and any(r > 55 for r in rems)               # paddings of one block and of two
        if nb_max > 2 + T:
            assert [n % 64 for n in lens[:5]] == list(bg.REMAINDERS)
        if T == bg.cut_of(nb_max) - 1:                                                # the longest tail the plan allows:
            assert end - fast_end == bg.cut_of(nb_max)
            two = lens[:-1] + [(nb_min - 2) * 64 + 56]                                # a two-block padding on the shortest
            assert bf.nblocks(two[-1]) == nb_min and len(bf.ref_plan(two, span)[2]) == 2      # closes the group early


def test_the_ladder_grid_reaches_the_tails(ladder_plans):
    for span in SPANS:
        groups = [g[0] for (s, _, _), (_, g) in ladder_plans.items() if s == span]
        for T in range(8):
            with_T = [(f, e, m) for f, e, m in groups if e - m == T]
            assert {m % 2 for _, _, m in with_T} == {0, 1}, (span, T)                 # both parities of nb_min
            assert {e % 2 for _, e, _ in with_T} == {0, 1}, (span, T)                 # ... and of end
        assert {e - m for _, e, m in groups} == {0, 1, 2, 3, 4, 5, 6, 7, 16, 29, 30, 31}
        assert any(f == 0 and e >= 3 for f, e, _ in groups)                           # no raw block, three padded ones
    # the helper's padded-block region carries raw data: fast_end at least 4 blocks below a member's whole blocks
    for span in SPANS:
        assert any(max(n // 64 for n in lens) - g[0][0] >= 4
                   for (s, _, _), (lens, g) in ladder_plans.items() if s == span)
        assert any(max(n // 64 for n in lens) - g[0][0] >= 30
                   for (s, _, _), (lens, g) in ladder_plans.items() if s == span)     # ring indices past 30


def test_ladder_torrents():
    for span in SPANS:
        for nb_max, T in ((2, 1), (10, 7), (257, 31)):
            ts = bg.ladder(span, nb_max, T)
            assert [t.total for t in ts] == bg.ladder_lens(span, nb_max, T)
            assert all((t.L, t.n) == (t.total, 1) and t.lens() == [t.total] for t in ts)
            bad = {0, span // 2, span - 1}
            assert [k for k, t in enumerate(ts) if t.flipped] == sorted(bad)
            assert [t.expected() for t in ts] == [[int(k not in bad)] for k in range(span)]
            assert ts[0].staged[:-1] == ts[0].payload[:-1] and ts[0].staged[-1] != ts[0].payload[-1]
            assert ts[-1].staged[:-1] == ts[-1].payload[:-1] and ts[-1].staged[-1] != ts[-1].payload[-1]
            assert ts[span // 2].staged == ts[span // 2].payload


STAIR_TAILS = {32: [6, 7, 8, 9, 11, 12, 14, 17, 18],
               64: [6, 7, 8, 9, 11, 12, 14, 16, 19, 21, 25, 29, 32, 36, 37]}


def test_the_staircase_cuts_its_groups_early(stair):
    assert len(stair) == bg.STAIR_COUNT + len(bg.STAIR_MULTI)
    assert sum(t.total for t in stair) <= bg.STAIR_MAX_BYTES
    assert sum(1 for t in stair if t.n == 1) == bg.STAIR_COUNT and sum(1 for t in stair if t.n > 1) == 3
    assert all(t.total % t.L for t in stair if t.n > 1)                               # short last pieces
    for span in SPANS:
        lens, launch, origin, groups, members = _groups(stair, span)
        assert min(lens) > 0                                                          # no zero-length piece
        assert sum(1 for g in range(len(groups)) if -1 in origin[g * span:(g + 1) * span]) >= 10
        assert max(len({bf.nblocks(lens[k]) for k in m}) for m in members) >= 16
        assert sorted({e - m for _, e, m in groups}) == STAIR_TAILS[span]
        assert {m % 2 for _, _, m in groups} == {0, 1}
        assert sorted(k for m in members for k in m) == list(range(len(lens)))        # every entry answered once
    assert [len(_groups(stair, span)[3]) for span in SPANS] == [26, 22]


def test_the_crowd_is_a_large_launch(crowd):
    n = sum(t.n for t in crowd)
    assert n > 16384 and n == bg.CROWD_TORRENTS * bg.CROWD_PIECES + len(bg.CROWD_LONGER)
    assert sum(t.total for t in crowd) <= bg.CROWD_MAX_BYTES
    assert bf.auto_kernel(n, 256) == "lane"                    # 64 x 256 CUs < n: auto takes the lane form
    many = [t for t in crowd if t.n > 1]
    assert len(many) == bg.CROWD_TORRENTS and all(t.n == bg.CROWD_PIECES for t in many)
    assert all(t.total % t.L and 2 <= t.L <= bg.CROWD_MAX_L for t in many)            # a short last piece each
    assert [t.total for t in crowd if t.n == 1] == list(bg.CROWD_LONGER)
    lens = bg.all_lens(crowd)
    assert {bf.nblocks(x) for x in lens} >= set(range(1, 12)) and min(lens) > 0
    plans = [bf.ref_plan(lens, span) for span in SPANS]
    groups32, groups64 = plans[0][2], plans[1][2]
    assert len(groups32) > 512                                 # a forced twin launch: more workgroups than 2 x 256 CUs
    assert len(groups64) % 4                                   # the lane grid's last workgroup has waves without a group
    for groups in (groups32, groups64):
        assert any(f == 0 for f, _, _ in groups) and any(e - m >= 4 for _, e, m in groups)
    # the two spans pad differently: a launch of one form on the tables another form's launch sized
    assert len(plans[0][0]) != len(plans[1][0]) and -1 in plans[0][1] and -1 in plans[1][1]


def _corrupted(t):
    """The pieces whose staged bytes or digest differ from the clean torrent's."""
    out = set()
    for i in range(t.n):
        a, n = i * t.L, t.piece_len(i)
        if t.staged[a:a + n] != t.payload[a:a + n]:
            out.add(i)
        if t.digests[20 * i:20 * i + 20] != hashlib.sha1(t.payload[a:a + n]).digest():
            out.add(i)
    return out


def test_expected_is_zero_exactly_at_the_corrupted_pieces(stair, crowd):
    for ts, share in ((stair, 8), (crowd, 10)):
        n = sum(t.n for t in ts)
        assert sum(len(t.flipped) for t in ts) == n // share
        for t in ts:
            assert len(t.payload) == len(t.staged) == t.total and len(t.digests) == 20 * t.n and t.avail is None
            assert _corrupted(t) == t.flipped
            assert t.expected() == [int(i not in t.flipped) for i in range(t.n)]
    for t in bg.ladder(32, 41, 5) + bg.ladder(64, 3, 2):
        assert _corrupted(t) == t.flipped
        assert t.expected() == [int(not t.flipped)]


def test_index_bits_tell_any_two_entries_apart(stair):
    n = sum(t.n for t in stair)
    bits = bg.index_bits(n)
    assert 2 ** (bits - 1) < n <= 2 ** bits and bg.index_bits(1024) == 10 and bg.index_bits(1025) == 11
    marks = [0] * n
    for k in range(bits):
        ds = bg.index_bit_digests(stair, k)
        assert [len(d) for d in ds] == [len(t.digests) for t in stair]
        e = 0
        for t, d in zip(stair, ds):
            for i in range(t.n):
                changed = d[20 * i:20 * i + 20] != t.digests[20 * i:20 * i + 20]
                assert changed == bool((e >> k) & 1)
                # never back to the clean digest: a piece whose digest the staircase flipped stays wrong
                assert not changed or d[20 * i:20 * i + 20] != hashlib.sha1(
                    t.payload[i * t.L:i * t.L + t.piece_len(i)]).digest()
                marks[e] |= int(changed) << k
                e += 1
    assert marks == list(range(n))


def test_the_designed_batches_are_deterministic():
    assert bg.staircase() == bg.staircase()
    assert bg.crowd() == bg.crowd()
    for args in ((32, 9, 7), (64, 258, 31)):
        assert bg.ladder(*args) == bg.ladder(*args)
    assert bg.ladder(32, 9, 7) != bg.ladder(32, 9, 6)
    perm, ts = bg.shuffled(bg.ladder(32, 2, 0))
    assert sorted(perm) == list(range(32)) and perm != sorted(perm) and bg.shuffled(ts)[0] == perm
