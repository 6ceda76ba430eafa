"""BitTorrent v2 host side, no GPU: the hashlib reference's known answers (they follow from the BEP 52 rules as
DESIGN / INTEGRATION restate them), the v2 metainfo parser, the raw-key bencode decoder, and V2Layout against the
golden piece tables."""
import hashlib
import os

import pytest

from tests import v2_ref
from tests.v2_util import benc, golden, golden_files, torrent_v2

K = 1024


def H(b):
    return hashlib.sha256(b).digest()


# ---- the reference itself: answers that follow from the spec text ---------------------------------------------

def test_ref_one_leaf_file_is_plain_sha256():
    data = os.urandom(16384)
    root, layer, hashes = v2_ref.file_hashes(data, 16 * K)
    assert root == H(data) and layer == b"" and hashes == [root]
    assert v2_ref.file_hashes(data, 1024 * K)[0] == H(data)        # whatever the piece length: one leaf, width 1
    assert v2_ref.file_hashes(data[:1], 64 * K)[0] == H(data[:1])  # a short leaf is hashed at its real length


def test_ref_two_leaves():
    data = os.urandom(32 * K)
    assert v2_ref.file_hashes(data, 64 * K)[0] == H(H(data[:16384]) + H(data[16384:]))


def test_ref_three_leaves_at_width_four():
    data = os.urandom(2 * 16384 + 777)
    h0, h1, h2 = H(data[:16384]), H(data[16384:32768]), H(data[32768:])
    want = H(H(h0 + h1) + H(h2 + bytes(32)))
    assert v2_ref.file_hashes(data, 128 * K)[0] == want
    assert v2_ref.piece_root(data, 4) == want


def test_ref_layer_is_padded_with_the_zero_piece_subtree_root():
    L = 32 * K                                  # 2 leaves per piece
    data = os.urandom(3 * L)                    # 3 pieces -> a layer padded to 4
    root, layer, hashes = v2_ref.file_hashes(data, L)
    p = [H(H(data[i * L:i * L + 16384]) + H(data[i * L + 16384:(i + 1) * L])) for i in range(3)]
    assert layer == b"".join(p) and hashes == p
    zero_piece = H(bytes(64))                   # the root of a piece whose two leaves are zero hashes
    assert root == H(H(p[0] + p[1]) + H(p[2] + zero_piece))
    assert root != H(H(p[0] + p[1]) + H(p[2] + bytes(32)))


def test_ref_short_last_piece_keeps_the_full_width():
    L = 64 * K                                  # 4 leaves per piece
    data = os.urandom(L + 16384 + 5)            # the last piece holds 2 leaves (one short) of 4
    _, layer, _ = v2_ref.file_hashes(data, L)
    t = data[L:]
    assert layer[32:] == H(H(H(t[:16384]) + H(t[16384:])) + H(bytes(64)))


def test_ref_piece_table():
    L = 64 * K
    assert v2_ref.piece_table([L + 1, 0, 1, 3 * 16384], L) == [(0, 0, L, 4), (0, L, 1, 4), (2, 0, 1, 1), (3, 0, 49152, 4)]


# ---- bencode: raw keys and spans ---------------------------------------------------------------------------------

def test_bdecode_raw_keeps_byte_keys_and_gives_spans():
    from torrent_amd import bdecode, bdecode_raw
    key = bytes(range(224, 256))                # not UTF-8
    raw_info = benc({"x": 1})
    data = b"d4:info" + raw_info + b"12:piece layersd32:" + key + b"3:abcee"
    val, spans = bdecode_raw(data, spans=True)
    assert list(val) == [b"info", b"piece layers"]
    assert bytes(val[b"piece layers"][key]) == b"abc"
    a, b = spans[b"info"]
    assert data[a:b] == raw_info
    assert key.decode("utf-8", "replace") in bdecode(data)["piece layers"]      # bdecode itself is unchanged
    assert bdecode_raw(data) == val
    with pytest.raises(ValueError):
        bdecode_raw(b"d3:abc")


# ---- the parser ---------------------------------------------------------------------------------------------------

def _files():
    return [os.urandom(n) for n in (3 * 64 * K + 5, 0, 1, 64 * K, 64 * K + 1)]


def test_parse_v2_only():
    from torrent_amd import parse_metainfo, parse_metainfo_v2
    files = _files()
    L = 64 * K
    raw = torrent_v2(files, L, name="demo")
    m = parse_metainfo_v2(raw)
    assert m is not None and not m.hybrid and m.name == "demo" and m.piece_length == L
    assert [f.length for f in m.files] == [len(f) for f in files]
    assert [f.path for f in m.files] == [["d00", "f000.bin"], ["d00", "f001.bin"], ["d00", "f002.bin"],
                                         ["d01", "f003.bin"], ["d01", "f004.bin"]]
    want = [v2_ref.file_hashes(f, L) for f in files]
    assert [f.pieces_root for f in m.files] == [w[0] for w in want]
    assert m.files[1].pieces_root is None
    # the layer keys are 32 raw bytes (almost never UTF-8): they survive
    assert m.piece_layers == {w[0]: w[1] for w in want if w[1]}
    assert len(m.piece_layers) == 2
    i = raw.index(b"4:info") + 6
    j = raw.index(b"12:piece layers")
    assert m.info_hash_v2 == hashlib.sha256(raw[i:j]).digest()
    assert m.layout.hashes == b"".join(b"".join(w[2]) for w in want)
    assert parse_metainfo(raw) is None                  # the v1 parser still has nothing to say about it


def test_parse_hybrid_with_both_parsers():
    from torrent_amd import parse_metainfo, parse_metainfo_v2
    L = 32 * K
    data = os.urandom(5 * L)
    pieces = b"".join(hashlib.sha1(data[i:i + L]).digest() for i in range(0, len(data), L))
    raw = torrent_v2([data], L, name="one.bin", paths=[["one.bin"]], hybrid_pieces=pieces)
    m1, m2 = parse_metainfo(raw), parse_metainfo_v2(raw)
    assert m1 is not None and m2 is not None and m2.hybrid
    assert m1.info.pieces_raw == pieces and m1.info.length == len(data) == m2.files[0].length
    assert m2.layout.n_pieces == m1.info.n_pieces == 5


@pytest.mark.parametrize("what", ["L_not_pow2", "L_small", "no_layer", "short_layer", "long_layer", "wrong_layer",
                                  "zero_with_root", "no_root", "v1", "no_tree", "short_root"])
def test_parse_rejects(what):
    from torrent_amd import parse_metainfo_v2
    files = _files()
    L = 64 * K
    big_root = v2_ref.file_hashes(files[0], L)[0]

    def mutate(top):
        info, tree = top["info"], top["info"]["file tree"]
        if what == "L_not_pow2":
            info["piece length"] = 3 * 16384
        elif what == "L_small":
            info["piece length"] = 8192
        elif what == "no_layer":
            del top["piece layers"][big_root]
        elif what == "short_layer":
            top["piece layers"][big_root] = top["piece layers"][big_root][:-32]
        elif what == "long_layer":
            top["piece layers"][big_root] += bytes(32)
        elif what == "wrong_layer":
            top["piece layers"][big_root] = bytes(32) + top["piece layers"][big_root][32:]
        elif what == "zero_with_root":
            tree["d00"]["f001.bin"][""]["pieces root"] = bytes(32)
        elif what == "no_root":
            del tree["d00"]["f002.bin"][""]["pieces root"]
        elif what == "v1":
            info["meta version"] = 1
        elif what == "no_tree":
            del info["file tree"]
        elif what == "short_root":
            tree["d00"]["f002.bin"][""]["pieces root"] = bytes(31)

    assert parse_metainfo_v2(torrent_v2(files, L)) is not None
    assert parse_metainfo_v2(torrent_v2(files, L, mutate=mutate)) is None
    assert parse_metainfo_v2(b"not bencode") is None


# ---- V2Layout against the golden tables ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["multi64k", "small128k", "leaf16k"])
def test_layout_equals_golden(name):
    from torrent_amd import parse_metainfo_v2
    g = golden()[name]
    files = golden_files(name)
    L = g["piece_length"]
    m = parse_metainfo_v2(torrent_v2(files, L))
    lay = m.layout
    table = [tuple(r) for r in g["piece_table"]]
    assert list(zip(lay.piece_file, lay.piece_offset, lay.piece_bytes, lay.tree_leaves)) == table
    assert lay.hashes.hex() == "".join(g["piece_hashes"])
    assert [None if f.pieces_root is None else f.pieces_root.hex() for f in m.files] == g["pieces_roots"]
    assert {k.hex(): v.hex() for k, v in m.piece_layers.items()} == g["piece_layers"]
    # every file starts a new piece: its aligned offset is its first piece x L
    for k, n in enumerate(g["lengths"]):
        assert lay.file_offset[k] == lay.file_first_piece[k] * L
        if n:
            assert table[lay.file_first_piece[k]][:2] == (k, 0)
    assert lay.total_length == (len(table) - 1) * L + table[-1][2]


def test_golden_file_is_current(tmp_path):
    """tests/golden/v2_layouts.json is what make_golden_v2.py writes (hashlib + tests/synth.py)."""
    import importlib.util
    import json
    from tests.v2_util import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_v2", os.path.join(ROOT, "tests", "golden", "make_golden_v2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert [mod.build(s) for s in mod.LAYOUTS] == json.load(open(os.path.join(ROOT, "tests", "golden", "v2_layouts.json")))


def test_native_binding_has_the_v2_calls(native):
    assert native.TV_V2_LEAF_BYTES == 16384 and native.KERNEL_V2 == 8
    lib = native.lib()
    assert lib.tv_v2_set_pieces(None, 0, None, None, None) == native.TV_ERR_ARG
    assert lib.tv_v2_verify(None, None, None) == native.TV_ERR_ARG
    assert lib.tv_v2_hash(None, None) == native.TV_ERR_ARG
    for name in ("v2_set_pieces", "v2_verify", "v2_hash"):
        assert callable(getattr(native.Context, name))
