"""Hybrid torrents on the CPU: parse_metainfo_hybrid's consistency rules over fixtures with real pad entries
(tests/hybrid_util.py), and the structure make_torrent_hybrid writes, with the library context replaced by a stand-in
that hashes with hashlib and tests/v2_ref.py (as tests/test_flush_policy.py replaces it).  The GPU side is
tests/test_gpu_hybrid.py."""
import hashlib
import os

import pytest

from tests import hybrid_util as hu
from tests import synth, v2_ref, v2_util
from torrent_amd import hybrid, parse_metainfo, parse_metainfo_hybrid, parse_metainfo_v2, verify

L = 32 << 10
LEAF = 16384


def make_files(lengths, seed=40):
    return [bytes(synth.fill(seed + k, 0, n)) for k, n in enumerate(lengths)]


LENGTHS = [1, L, 17, 0, 2 * L + 5, LEAF + 1, 3 * L]
FILES = make_files(LENGTHS)
PATHS = v2_util.file_names(len(FILES))


def check_accepts(tor, files, trailing_pad=False):
    m = parse_metainfo_hybrid(tor)
    assert m is not None
    lin = hu.padded_linear(files, L, trailing_pad)
    assert m.total_length == len(lin)
    assert m.pieces == hu.v1_pieces(files, L, trailing_pad) and len(m.pieces) == 20 * m.n_pieces
    assert [f.length for f in m.files] == [len(d) for d in files]
    assert m.layout.hashes == b"".join(hu.v2_expected(files, L))
    assert m.v2.hybrid and m.info_hash_v2 == parse_metainfo_v2(tor).info_hash_v2
    assert m.info_hash == parse_metainfo(tor).info_hash and len(m.info_hash) == 20
    assert m.name == "t" and m.piece_length == L
    return m


def test_accepts_a_padded_multi_file_hybrid():
    tor = hu.torrent_hybrid(FILES, L, paths=PATHS)
    m = check_accepts(tor, FILES)
    assert m.total_length % L == 0           # (the last file is whole pieces)
    v1 = parse_metainfo(tor)                 # the v1 parser sees the pad entries as files: its length is the padded one
    assert v1.info.length == m.total_length and len(v1.info.files) > len(FILES)


def test_accepts_a_single_file_hybrid():
    for n in (5, L, 2 * L + 9):
        files = make_files([n])
        m = check_accepts(hu.torrent_hybrid(files, L, single=True), files)
        assert m.total_length == n and [f.path for f in m.files] == [["t"]]


def test_accepts_a_trailing_pad_and_a_short_last_piece():
    files = make_files([L + 3, 2 * L + 100])
    short = check_accepts(hu.torrent_hybrid(files, L), files)
    assert short.total_length == 2 * L + 2 * L + 100
    full = check_accepts(hu.torrent_hybrid(files, L, trailing_pad=True), files, trailing_pad=True)
    assert full.total_length == 5 * L and full.n_pieces == short.n_pieces == 5
    assert full.pieces[:80] == short.pieces[:80] and full.pieces[80:] != short.pieces[80:]


def test_accepts_a_zero_length_file_between_files():
    files = make_files([7, 0, L + 1, 0])
    m = check_accepts(hu.torrent_hybrid(files, L), files)
    assert m.n_pieces == 3 and m.total_length == L + L + 1
    # the pad may stand on either side of the empty file: it takes no bytes
    paths = v2_util.file_names(4)
    swapped = [{"length": 7, "path": paths[0]}, {"length": 0, "path": paths[1]},
               {"attr": "p", "length": L - 7, "path": [".pad", str(L - 7)]}, {"length": L + 1, "path": paths[2]},
               {"length": 0, "path": paths[3]}]
    check_accepts(hu.torrent_hybrid(files, L, v1_files=swapped), files)


def _with_files(edit):
    v1 = hu.v1_file_list(FILES, PATHS, L)
    edit(v1)
    return hu.torrent_hybrid(FILES, L, paths=PATHS, v1_files=v1)


def _pad_positions(v1):
    return [k for k, e in enumerate(v1) if "attr" in e]


def test_rejects_a_wrong_pad_length():
    def edit(v1):
        v1[_pad_positions(v1)[0]]["length"] += 1
    assert parse_metainfo_hybrid(_with_files(edit)) is None


def test_rejects_a_missing_pad():
    def edit(v1):
        del v1[_pad_positions(v1)[1]]
    assert parse_metainfo_hybrid(_with_files(edit)) is None


def test_rejects_a_pad_where_none_is_needed():
    def edit(v1):      # after the file of exactly L bytes
        k = next(k for k, e in enumerate(v1) if "attr" not in e and e["length"] == L)
        v1.insert(k + 1, {"attr": "p", "length": L, "path": [".pad", str(L)]})
    assert parse_metainfo_hybrid(_with_files(edit)) is None

    def twice(v1):     # a second pad after a pad
        k = _pad_positions(v1)[0]
        v1.insert(k + 1, dict(v1[k]))
    assert parse_metainfo_hybrid(_with_files(twice)) is None

    def first(v1):     # a pad before the first file
        v1.insert(0, {"attr": "p", "length": L, "path": [".pad", str(L)]})
    assert parse_metainfo_hybrid(_with_files(first)) is None


def test_rejects_files_reordered_between_the_descriptions():
    order = [1, 0] + list(range(2, len(FILES)))
    v1 = hu.v1_file_list([FILES[k] for k in order], [PATHS[k] for k in order], L)
    assert parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS, v1_files=v1)) is None


def test_rejects_a_length_mismatch():
    def edit(v1):      # one byte moved from the file into its pad: the v1 space is the same size, the file is not
        k = next(k for k, e in enumerate(v1) if e["length"] == 17)
        v1[k]["length"], v1[k + 1]["length"] = 16, v1[k + 1]["length"] + 1
    assert parse_metainfo_hybrid(_with_files(edit)) is None
    single = hu.torrent_hybrid(make_files([L + 9]), L, single=True, mutate=lambda top: top["info"].update(length=L + 8))
    assert parse_metainfo_hybrid(single) is None
    renamed = hu.torrent_hybrid(make_files([L + 9]), L, single=True, mutate=lambda top: top["info"].update(name="u"))
    assert parse_metainfo_hybrid(renamed) is None and parse_metainfo_v2(renamed) is not None


def test_rejects_a_different_piece_length():
    # the v1 side (pads and pieces) made for L / 2 pieces, the v2 side and `piece length` for L
    v1 = hu.v1_file_list(FILES, PATHS, L // 2)
    tor = hu.torrent_hybrid(FILES, L, paths=PATHS, v1_files=v1, pieces=hu.v1_pieces(FILES, L // 2))
    assert parse_metainfo_v2(tor) is not None and parse_metainfo_hybrid(tor) is None
    # and for 2 L, where only some pads differ
    v1 = hu.v1_file_list(FILES, PATHS, 2 * L)
    tor = hu.torrent_hybrid(FILES, L, paths=PATHS, v1_files=v1, pieces=hu.v1_pieces(FILES, 2 * L))
    assert parse_metainfo_hybrid(tor) is None


def test_rejects_a_pieces_string_one_digest_short():
    good = hu.v1_pieces(FILES, L)
    assert parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS, pieces=good[:-20])) is None
    assert parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS, pieces=good + bytes(20))) is None
    assert parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS, pieces=good[:-1])) is None


def test_rejects_v2_only_and_v1_only():
    v2_only = v2_util.torrent_v2(FILES, L, paths=PATHS)
    assert parse_metainfo_v2(v2_only) is not None and parse_metainfo_hybrid(v2_only) is None

    def strip(top):
        del top["info"]["file tree"], top["info"]["meta version"], top["piece layers"]
    v1_only = hu.torrent_hybrid(FILES, L, paths=PATHS, mutate=strip)
    assert parse_metainfo(v1_only) is not None and parse_metainfo_hybrid(v1_only) is None
    assert parse_metainfo_hybrid(b"not a torrent") is None


def test_disagree_lists_the_pieces_where_the_bitfields_differ():
    r = hybrid.HybridResult(bytearray(b"\xa0\x80"), bytearray(b"\xe0\x80"), bytearray(b"\xa0\xc0"))
    assert r.disagree == [1, 9]


class _HashCtx:
    """tv_ctx stand-in for creation mode: stage_files() reads the files into the aligned space, hybrid_hash() hashes it
    with hashlib (the pad ranges as zeros) and tests/v2_ref.py."""

    thread_budget = 1

    def set_option(self, key, value):
        pass

    def counter(self, key):
        return 0

    def set_layout(self, total, L_, P, first, count):
        self.total, self.L, self.P, self.first, self.count = total, L_, P, first, count
        self.space = bytearray(b"\xff" * (P * L_))       # stale bytes: the pads must not come from here

    def v2_set_pieces(self, piece_bytes, tree_leaves, hashes=None):
        assert hashes is None
        self.pb, self.tl = list(piece_bytes), list(tree_leaves)

    def stage_files(self, paths, file_offsets, linear_offsets, lens):
        for p, fo, lo, n in zip(paths, file_offsets, linear_offsets, lens):
            with open(p, "rb") as f:
                f.seek(fo)
                self.space[lo:lo + n] = f.read(n)
        return [0] * len(paths)

    def hybrid_hash(self):
        d, r = b"", b""
        for i in range(self.first, self.first + self.count):
            row = self.space[i * self.L:i * self.L + self.pb[i]]
            v1_len = min(self.L, self.total - i * self.L)
            d += hashlib.sha1(bytes(row) + bytes(v1_len - self.pb[i])).digest()
            r += v2_ref.piece_root(row, self.tl[i])
        return d, r


@pytest.fixture
def fake(monkeypatch):
    def run_shards(devs, n_pieces, fn):
        ranges = [(0, 8), (8, n_pieces - 8)] if n_pieces > 8 else [(0, n_pieces)]    # two shards where there are pieces for two
        return ranges, [fn(_HashCtx(), first, count) for first, count in ranges]
    monkeypatch.setattr(verify, "_run_shards", run_shards)      # (where the shared shard runners look it up)


def _write_tree(root, lengths, seed=70):
    names = [os.path.join("a", "x.bin"), os.path.join("a", "y.bin"), "b.bin", os.path.join("c", "d", "e.bin"),
             "f.bin", "g.bin", "h.bin"][:len(lengths)]
    files = make_files(lengths, seed)
    for name, d in zip(names, files):
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        with open(os.path.join(root, name), "wb") as f:
            f.write(d)
    return [n.split(os.sep) for n in names], files


@pytest.mark.parametrize("lengths", [[1, L, 17, 0, 2 * L + 5, LEAF + 1, 3 * L], [L + 3, 0, 2 * L + 100], [5, 0, 0],
                                     [4 * L, 6 * L + 1]])
def test_make_torrent_hybrid_round_trips(tmp_path, fake, lengths):
    root = str(tmp_path / "t")
    os.makedirs(root)
    paths, files = _write_tree(root, lengths)
    tor = hybrid.make_torrent_hybrid(root, "http://example.com/announce", creation_date=1, piece_length=L)
    m = parse_metainfo_hybrid(tor)
    assert m is not None and [f.path for f in m.files] == paths and [f.length for f in m.files] == lengths
    assert m.pieces == hu.v1_pieces(files, L) and m.total_length == len(hu.padded_linear(files, L))
    assert m.layout.hashes == b"".join(hu.v2_expected(files, L))
    v1, v2 = parse_metainfo(tor), parse_metainfo_v2(tor)
    assert v1 is not None and v2 is not None and v2.hybrid
    assert v1.info.length == m.total_length and v1.info.pieces_raw == m.pieces and v1.info_hash == m.info_hash
    # the pad entries: `attr` p, path [".pad", "<length>"], after every file that does not end a piece and is followed
    # by one that holds bytes; none after the last
    from torrent_amd import bdecode
    entries = bdecode(tor)["info"]["files"]
    got = [(bytes(e["attr"]) if "attr" in e else None, e["length"], [bytes(c).decode() for c in e["path"]]) for e in entries]
    want = [(b"p" if "attr" in e else None, e["length"], e["path"]) for e in hu.v1_file_list(files, paths, L)]
    assert got == want
    assert tor == hu.v2_util.benc(_decoded(tor))        # canonical: keys sorted at every level


def _decoded(tor):
    from torrent_amd import bdecode_raw

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, list):
            return [plain(x) for x in v]
        return bytes(v) if isinstance(v, memoryview) else v
    return plain(bdecode_raw(tor))


def test_make_torrent_hybrid_single_file(tmp_path, fake):
    d = make_files([2 * L + 77], 90)[0]
    p = tmp_path / "one.bin"
    p.write_bytes(d)
    tor = hybrid.make_torrent_hybrid(str(p), "http://example.com/announce", creation_date=1, piece_length=L)
    m = parse_metainfo_hybrid(tor)
    assert m is not None and m.name == "one.bin" and m.total_length == len(d)
    assert m.pieces == hu.v1_pieces([d], L) and m.layout.hashes == b"".join(hu.v2_expected([d], L))
    v1 = parse_metainfo(tor)
    assert v1.info.files is None and v1.info.length == len(d)
