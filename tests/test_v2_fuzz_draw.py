"""The seeded v2 draw (tests/v2_fuzz.py) on the CPU: every feature the GPU fuzz is meant to reach occurs in at least two
seeds, every layout is within the sizes the fuzz promises, and the hashlib reference's piece table equals the
product's (metainfo_v2.make_layout) on every seed."""
import pytest

from tests import v2_fuzz, v2_ref
from tests.v2_fuzz import FEATURES, LEAF, SEEDS, draw, features


@pytest.fixture(scope="module")
def draws():
    return [draw(s) for s in SEEDS]


def test_every_feature_occurs_in_at_least_two_seeds(draws):
    assert len(SEEDS) >= 24
    count = {name: 0 for name in FEATURES}
    for d in draws:
        got = features(d)
        assert got <= set(FEATURES)
        for name in got:
            count[name] += 1
    assert all(n >= 2 for n in count.values()), count


def test_layouts_are_what_the_draw_promises(draws):
    for d in draws:
        table = d.table
        P = len(table)
        assert d.L in v2_fuzz.PIECE_LENGTHS and 1 <= len(d.lengths) <= 40 and P >= 1
        assert P * d.L <= (8 << 20) if d.seed % 8 != 7 else 64 <= P <= 84, (d.seed, P)
        assert [len(f) for f in d.files] == d.lengths == [len(f) for f in d.staged]
        # the corrupted positions: at least one piece, one of them the last valid byte of a short leaf, and the
        # staged bytes differ from the files' in exactly those
        assert d.corrupt and any(pos == table[i][2] - 1 and table[i][2] % LEAF for i, pos in d.corrupt)
        diff = set()
        for i, (f, o, b, w) in enumerate(table):
            a, s = d.files[f][o:o + b], d.staged[f][o:o + b]
            if a != s:
                diff |= {(i, q) for q in range(b) if a[q] != s[q]}
        assert diff == set(d.corrupt)
        # corrupted pieces fail, the others pass, and a piece the disk cannot supply is 0
        want, roots = d.expected(), d.staged_roots()
        bad = {i for i, _ in d.corrupt}
        assert [a == b for a, b in zip(want, roots)] == [i not in bad for i in range(P)]
        bits = v2_ref.expected_bitfield(d.disk(), d.L, want, have=d.lengths)
        for i, (f, o, b, w) in enumerate(table):
            readable = f not in d.missing and d.short.get(f, d.lengths[f]) >= o + b
            assert bool(bits[i >> 3] & (0x80 >> (i & 7))) == (readable and i not in bad), (d.seed, i)


def test_draw_is_deterministic():
    a, b = draw(3), draw(3)
    assert (a.L, a.lengths, a.files, a.staged, a.corrupt, a.missing, a.short) == \
           (b.L, b.lengths, b.files, b.staged, b.corrupt, b.missing, b.short)


def test_reference_piece_table_equals_make_layout(draws):
    from torrent_amd.metainfo_v2 import make_layout
    for d in draws:
        table = d.table
        lay = make_layout(d.lengths, d.L)
        assert lay.piece_bytes == [r[2] for r in table], d.seed
        assert lay.tree_leaves == [r[3] for r in table], d.seed
        assert lay.file_offset == d.file_offsets(), d.seed
        assert lay.piece_file == [r[0] for r in table] and lay.piece_offset == [r[1] for r in table], d.seed
        assert lay.total_length == (len(table) - 1) * d.L + table[-1][2]
