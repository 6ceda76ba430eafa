"""The seeded hybrid draw (tests/hybrid_fuzz.py) on the CPU: every feature the GPU fuzz is meant to reach occurs in at
least two seeds and every seed shows at least three, every draw is within the sizes the fuzz promises, the .torrent made
of a draw parses as the hybrid torrent it describes (wrongly stated hashes included), and the feature `no_tail` means
what the library's own planner says (torrent_amd.metainfo_v2.make_layout gives the same table)."""
import pytest

from tests import hybrid_fuzz, v2_ref
from tests.hybrid_fuzz import FEATURES, SEEDS, draw, features
from tests.v2_util import file_names


@pytest.fixture(scope="module")
def draws():
    return [draw(s) for s in SEEDS]


def test_every_feature_occurs_in_at_least_two_seeds_and_every_seed_shows_three(draws):
    assert len(SEEDS) >= 24 and len(FEATURES) == 17
    count = {name: 0 for name in FEATURES}
    for d in draws:
        got = features(d)
        assert got <= set(FEATURES)
        assert len(got) >= 3, (d.seed, got)
        for name in got:
            count[name] += 1
    assert all(n >= 2 for n in count.values()), count


def test_draws_are_what_the_module_promises(draws):
    for d in draws:
        table = d.table
        P, L = len(table), d.L
        assert L in hybrid_fuzz.PIECE_LENGTHS and 1 <= len(d.lengths) <= 400 and P >= 9
        assert P * L <= (8 << 20) + 4 * L, (d.seed, P)
        assert P <= 64 or L <= 32 * 1024, (d.seed, P)
        assert [len(f) for f in d.files] == d.lengths == [len(f) for f in d.staged]
        # the shards cover the pieces in order
        assert 2 <= len(d.shards) <= 3 and d.shards[0][0] == 0 and all(c > 0 for _, c in d.shards)
        assert [a + c for a, c in d.shards] == [a for a, _ in d.shards[1:]] + [P]
        assert all(a % 8 == 0 for a, _ in d.shards + [d.odd])               # (tv_set_layout takes no other start)
        assert d.odd[1] % 8 and d.odd[0] + d.odd[1] < P
        # the staged bytes differ from the files' in exactly the corrupted positions, one of them the last file byte
        # before a pad range or of a short last piece
        assert d.corrupt and any(pos == table[i][2] - 1 and table[i][2] < L for i, pos in d.corrupt)
        diff = set()
        for i, (f, o, b, w) in enumerate(table):
            a, s = d.files[f][o:o + b], d.staged[f][o:o + b]
            if a != s:
                diff |= {(i, q) for q in range(b) if a[q] != s[q]}
        assert diff == set(d.corrupt)
        # wrongly stated hashes: disjoint sets, every entry changes its hash
        assert d.v1_flips and d.v2_flips and not set(d.v1_flips) & set(d.v2_flips)
        lay = d.layout()
        pieces, hashes = d.stated(lay)
        assert [i for i in range(P) if pieces[20 * i:20 * i + 20] != lay.pieces[20 * i:20 * i + 20]] == \
            sorted(d.v1_flips)
        assert [i for i in range(P) if hashes[i] != lay.hashes[i]] == sorted(d.v2_flips)
        assert d.kernel in (0, 1, 2) and (d.lane_pairs in (1, 2)) == (d.kernel == 1)


def test_draw_is_deterministic():
    def key(d):
        return (d.L, d.lengths, d.files, d.staged, d.corrupt, d.missing, d.short, d.trailing, d.v1_flips, d.v2_flips,
                d.shards, d.odd, d.kernel, d.lane_pairs)
    assert key(draw(5)) == key(draw(5))


def test_the_torrent_of_a_draw_parses_as_the_hybrid_it_describes(draws):
    from torrent_amd import parse_metainfo_hybrid
    for d in draws:
        lay = d.layout()
        pieces, hashes = d.stated(lay)
        meta = parse_metainfo_hybrid(hybrid_fuzz.torrent(d, lay, file_names(len(d.lengths))))
        assert meta is not None, d.seed
        assert meta.total_length == lay.total and meta.n_pieces == lay.P, d.seed
        assert meta.pieces == pieces and meta.layout.hashes == b"".join(hashes), d.seed
        assert meta.layout.piece_bytes == lay.pb and meta.layout.tree_leaves == lay.tl, d.seed
        assert meta.layout.file_offset == lay.offs == d.file_offsets(), d.seed
        assert lay.table == v2_ref.piece_table(d.lengths, d.L)
