"""CPU tests of torrent_amd/merkle_v2.py: proof_v2 / check_proof_v2 against a restatement of a file's merkle tree
written here on hashlib alone (every layer of the tree over the file's leaf hashes, zero-padded to a power of two), and
BlockRepairVerifierV2 with a faked Context (as tests/test_flush_policy.py fakes it) whose answers come from hashlib."""
import hashlib

import pytest

from tests import synth, v2_ref
from tests.v2_util import torrent_v2
from torrent_amd import incremental, merkle_v2, parse_metainfo_v2
from torrent_amd.piece import BLOCK_SIZE, PieceMsg

K = 1024
LEAF = 16384
L = 64 * K                                                 # W = 4
# one leaf; three leaves (one piece, a 4-leaf tree); 2, 3 and 5 pieces (trees of 8, 16 and 32 leaves)
LENGTHS = [100, 2 * LEAF + 5, L + 1, 2 * L + LEAF + 7, 4 * L + 3 * LEAF]


def sha(b):
    return hashlib.sha256(b).digest()


def full_tree(data) -> list:
    """Every layer of the file's tree, bottom-up: layer 0 = SHA-256 of each 16 KiB block at its real length, then 32
    zero bytes per position out to the next power of two; layer b + 1 = SHA-256 of the pairs of layer b."""
    row = [sha(data[o:o + LEAF]) for o in range(0, len(data), LEAF)]
    width = 1
    while width < len(row):
        width *= 2
    row += [bytes(32)] * (width - len(row))
    layers = [row]
    while len(row) > 1:
        row = [sha(row[i] + row[i + 1]) for i in range(0, len(row), 2)]
        layers.append(row)
    return layers


@pytest.fixture(scope="module")
def torrent():
    files = [bytes(synth.fill(300 + k, 0, n)) for k, n in enumerate(LENGTHS)]
    meta = parse_metainfo_v2(torrent_v2(files, L))
    assert meta is not None
    lay = meta.layout
    leaves = {}
    for i in range(lay.n_pieces):
        d = files[lay.piece_file[i]][lay.piece_offset[i]:lay.piece_offset[i] + lay.piece_bytes[i]]
        hs = v2_ref.leaf_hashes(d)
        leaves[i] = b"".join(hs + [bytes(32)] * (lay.tree_leaves[i] - len(hs)))
    trees = [full_tree(f) for f in files]
    for f, t in zip(meta.files, trees):
        assert t[-1][0] == f.pieces_root                   # the restatement agrees with tests/v2_ref.py
    return meta, files, leaves, trees


def ranges(tree):
    H = len(tree) - 1
    for base in range(H + 1):
        n = len(tree[base])
        length = 1
        while length <= n:
            for index in range(0, n, length):
                yield base, index, length
            length *= 2


def expected_uncles(tree, base, index, length):
    layer, i = base + length.bit_length() - 1, index // length
    out = []
    while layer < len(tree) - 1:
        out.append(tree[layer][i ^ 1])
        layer, i = layer + 1, i >> 1
    return out


def test_every_layer_and_aligned_range(torrent):
    meta, files, leaves, trees = torrent
    assert [len(t) - 1 for t in trees] == [0, 2, 3, 4, 5]
    seen = 0
    for f, tree in enumerate(trees):
        H = len(tree) - 1
        for base, index, length in ranges(tree):
            hashes, uncles = merkle_v2.proof_v2(meta, f, base, index, length, leaves)
            what = (f, base, index, length)
            assert hashes == tree[base][index:index + length], what
            assert uncles == expected_uncles(tree, base, index, length), what
            assert len(uncles) == H - base - (length.bit_length() - 1), what
            assert merkle_v2.check_proof_v2(meta, f, base, index, hashes, uncles), what
            assert merkle_v2.check_proof_v2(meta, f, base, index, b"".join(hashes), b"".join(uncles)), what
            seen += 1
    assert seen > 150
    # ranges in the zero padding: the last leaves of the 5-piece file's 32-leaf tree, and its all-zero pieces 5 .. 7
    tree = trees[4]
    assert tree[0][19:] == [bytes(32)] * 13
    hashes, uncles = merkle_v2.proof_v2(meta, 4, 0, 24, 8, leaves)
    assert hashes == [bytes(32)] * 8 and merkle_v2.check_proof_v2(meta, 4, 0, 24, hashes, uncles)
    hashes, uncles = merkle_v2.proof_v2(meta, 4, 2, 5, 1, leaves)
    assert hashes == [v2_ref.zero_piece_root(L)] and merkle_v2.check_proof_v2(meta, 4, 2, 5, hashes, uncles)


def test_piece_layer_and_above_need_no_leaves(torrent):
    meta, files, leaves, trees = torrent
    for f, hp in ((2, 2), (3, 2), (4, 2), (0, 0), (1, 2)):     # the piece layer (a one-piece file's: its root)
        tree = trees[f]
        for base in range(hp, len(tree)):
            for index in range(len(tree[base])):
                hashes, uncles = merkle_v2.proof_v2(meta, f, base, index, 1)
                assert hashes == [tree[base][index]] and uncles == expected_uncles(tree, base, index, 1)
    # a proof inside piece 1 of the 3-piece file needs that piece's leaves and no other's
    first = meta.layout.file_first_piece[3]
    hashes, uncles = merkle_v2.proof_v2(meta, 3, 0, 4, 2, {first + 1: leaves[first + 1]})
    assert merkle_v2.check_proof_v2(meta, 3, 0, 4, hashes, uncles)


def test_refusals(torrent):
    meta, files, leaves, trees = torrent
    f, tree = 3, trees[3]                                  # 3 pieces, 16 leaves, H = 4
    hashes, uncles = merkle_v2.proof_v2(meta, f, 0, 4, 2, leaves)
    assert len(uncles) == 3 and merkle_v2.check_proof_v2(meta, f, 0, 4, hashes, uncles)

    def flip(h):
        return bytes([h[0] ^ 1]) + h[1:]

    for k in range(len(hashes)):                           # a tampered hash
        bad = list(hashes)
        bad[k] = flip(bad[k])
        assert not merkle_v2.check_proof_v2(meta, f, 0, 4, bad, uncles)
    for k in range(len(uncles)):                           # a tampered uncle
        bad = list(uncles)
        bad[k] = flip(bad[k])
        assert not merkle_v2.check_proof_v2(meta, f, 0, 4, hashes, bad)
    for index in (0, 2, 6, 8, 14, 16, 5, -2):              # a wrong index (aligned or not, inside the tree or not)
        assert not merkle_v2.check_proof_v2(meta, f, 0, index, hashes, uncles)
    assert not merkle_v2.check_proof_v2(meta, 4, 0, 4, hashes, uncles)      # another file
    assert not merkle_v2.check_proof_v2(meta, len(files), 0, 4, hashes, uncles)
    # one level off: the nodes of layer 1 passed as leaves.  Their own uncles are one fewer than a base-0 proof has, and
    # they do fold to the right root -- only the exact count refuses them
    h1, u1 = merkle_v2.proof_v2(meta, f, 1, 2, 2, leaves)
    assert merkle_v2.check_proof_v2(meta, f, 1, 2, h1, u1) and len(u1) == 2
    node, i = sha(h1[0] + h1[1]), 1
    for u in u1:
        node = sha(u + node) if i & 1 else sha(node + u)
        i >>= 1
    assert node == meta.files[f].pieces_root
    assert not merkle_v2.check_proof_v2(meta, f, 0, 2, h1, u1)
    assert not merkle_v2.check_proof_v2(meta, f, 0, 2, h1, u1 + [bytes(32)])
    assert not merkle_v2.check_proof_v2(meta, f, 0, 4, hashes, uncles[:-1])
    assert not merkle_v2.check_proof_v2(meta, f, 0, 4, hashes, uncles + [uncles[-1]])
    # a length that is no power of two, malformed values
    for length in (0, 3, 5, 6):
        with pytest.raises(ValueError):
            merkle_v2.proof_v2(meta, f, 0, 0, length, leaves)
    with pytest.raises(ValueError):
        merkle_v2.proof_v2(meta, f, 0, 2, 4, leaves)       # not a multiple of the length
    with pytest.raises(ValueError):
        merkle_v2.proof_v2(meta, f, 0, 16, 1, leaves)      # past the tree
    with pytest.raises(ValueError):
        merkle_v2.proof_v2(meta, f, 5, 0, 1, leaves)       # above the root
    assert not merkle_v2.check_proof_v2(meta, f, 0, 0, tree[0][:3], expected_uncles(tree, 0, 0, 4))
    assert not merkle_v2.check_proof_v2(meta, f, 0, 0, [], [])
    assert not merkle_v2.check_proof_v2(meta, f, 0, 4, [h[:31] for h in hashes], uncles)
    assert not merkle_v2.check_proof_v2(meta, f, 0, 4, b"".join(hashes)[:-1], uncles)
    # missing leaves: below the piece layer the touched pieces' leaf layers are needed
    first = meta.layout.file_first_piece[f]
    with pytest.raises(KeyError):
        merkle_v2.proof_v2(meta, f, 0, 4, 2)
    with pytest.raises(KeyError):
        merkle_v2.proof_v2(meta, f, 0, 4, 2, {first: leaves[first]})        # piece 0's, where piece 1's is needed
    with pytest.raises(KeyError):
        merkle_v2.proof_v2(meta, 1, 0, 0, 1)                                 # a one-piece file, below its root


# ---- BlockRepairVerifierV2 with a faked Context ---------------------------------------------------------------------------

class _FakeCtx:
    """The calls BlockRepairVerifierV2 makes, answered with hashlib: a slot pool that holds what was staged."""

    def __init__(self, device=0):
        self.staged = {}
        self.list_calls, self.check_calls = [], []

    def set_option(self, key, value):
        pass

    def set_layout(self, total, piece_length, n_pieces, first=0, count=None):
        self.L = piece_length

    def stage(self, offset, buf):
        assert offset % self.L == 0 and len(self.staged) < 3
        self.staged[offset // self.L] = bytes(buf)

    def v2_verify_list(self, pieces, piece_bytes, tree_leaves, hashes):
        self.list_calls.append(list(pieces))
        out = bytes(v2_ref.piece_root(self.staged[i][:b], w) == hashes[32 * k:32 * k + 32]
                    for k, (i, b, w) in enumerate(zip(pieces, piece_bytes, tree_leaves)))
        for i in pieces:
            self.staged.pop(i, None)
        return out

    def v2_check_blocks(self, pieces, piece_bytes, tree_leaves, leaf_hashes, want_bits=None, release=False):
        assert want_bits is None
        self.check_calls.append((list(pieces), release))
        W = self.L // LEAF
        assert len(leaf_hashes) == 32 * W * len(pieces)
        out = bytearray(len(pieces) * ((W + 7) // 8))
        for k, (i, b) in enumerate(zip(pieces, piece_bytes)):
            for q in range(-(-b // LEAF)):
                if sha(self.staged[i][q * LEAF:min(b, (q + 1) * LEAF)]) == leaf_hashes[32 * (k * W + q):][:32]:
                    out[k * ((W + 7) // 8) + (q >> 3)] |= 0x80 >> (q & 7)
        if release:
            for i in pieces:
                self.staged.pop(i, None)
        return bytes(out)

    def close(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    made = []

    def ctx(device=0):
        c = _FakeCtx(device)
        made.append(c)
        return c

    monkeypatch.setattr(incremental._native, "Context", ctx)
    return made


def _layout(n_bytes):
    data = bytes(synth.fill(77, 0, n_bytes))
    meta = parse_metainfo_v2(torrent_v2([data], L, name="one"))
    lay = meta.layout
    layers = {}
    for i in range(lay.n_pieces):
        hs = v2_ref.leaf_hashes(data[i * L:i * L + lay.piece_bytes[i]])
        layers[i] = b"".join(hs + [bytes(32)] * (lay.tree_leaves[i] - len(hs)))
    return data, lay, layers


def _msgs(data, lay, i):
    d = data[i * L:i * L + lay.piece_bytes[i]]
    return [PieceMsg(i, o, d[o:o + BLOCK_SIZE]) for o in range(0, len(d), BLOCK_SIZE)]


def test_block_repair_names_the_bad_block_and_completes_on_it(fake):
    data, lay, layers = _layout(2 * L + LEAF + 9)          # three pieces, the last short (2 blocks of its 4-leaf tree)
    bad = []
    v = merkle_v2.BlockRepairVerifierV2(lay, flush_pieces=None, flush_age_ms=None, slots=3, leaf_source=layers.get,
                                        on_bad_blocks=lambda i, blocks: bad.append((i, blocks)))
    ctx = fake[0]
    for i in range(3):
        for m in _msgs(data, lay, i):
            if (i, m.offset) == (1, 2 * BLOCK_SIZE):
                m = PieceMsg(1, m.offset, bytes([m.block[0] ^ 1]) + m.block[1:])
            v.on_block(m)
    assert sorted(v._kept) == [0, 1, 2]                    # the pending pieces' host bytes, until the flush returns
    assert v.flush() == [(0, True), (1, False), (2, True)]
    assert bad == [(1, [2])] and v._kept == {}
    assert ctx.list_calls == [[0, 1, 2]] and ctx.check_calls == [([1], True)] and ctx.staged == {}
    good = _msgs(data, lay, 1)
    assert v.on_block(good[0]) is False                    # a block it has: the piece is still one block short
    assert v.on_block(good[2]) is True                     # the bad block alone completes the piece
    assert v.flush() == [(1, True)]
    assert bytes(v.bitfield) == b"\xe0" and len(ctx.check_calls) == 1


def test_block_repair_checks_every_failed_piece_in_one_call(fake):
    data, lay, layers = _layout(2 * L + LEAF + 9)
    bad = {}
    known = {0: layers[0], 2: layers[2]}                   # piece 1's leaf layer is not known: forgotten, as before
    v = merkle_v2.BlockRepairVerifierV2(lay, flush_pieces=None, flush_age_ms=None, slots=3, leaf_source=known.get,
                                        on_bad_blocks=bad.__setitem__)
    ctx = fake[0]
    for i in range(3):
        for m in _msgs(data, lay, i):
            if (i, m.offset) in ((0, 0), (0, 3 * BLOCK_SIZE), (1, BLOCK_SIZE), (2, BLOCK_SIZE)):
                m = PieceMsg(i, m.offset, m.block[:-1] + bytes([m.block[-1] ^ 0x80]))   # (2, 1): its last valid byte
            v.on_block(m)
    assert v.flush() == [(0, False), (1, False), (2, False)]
    assert bad == {0: [0, 3], 2: [1]} and ctx.check_calls == [([0, 2], True)]
    assert 1 not in v._bufs and v._have_blocks[0] == {1, 2} and v._have_blocks[2] == {0}
    for i, o in ((0, 0), (2, 1), (0, 3)):
        assert v.on_block(_msgs(data, lay, i)[o]) is (o != 0)
    assert v.flush() == [(2, True), (0, True)]
    for m in _msgs(data, lay, 1):                          # the forgotten piece arrives whole again
        v.on_block(m)
    assert v.flush() == [(1, True)] and bytes(v.bitfield) == b"\xe0"


def test_a_layer_that_contradicts_the_root_makes_every_block_bad(fake):
    data, lay, layers = _layout(2 * L)
    corrupt = bytearray(data)
    corrupt[L + 5] ^= 2
    wrong = b"".join(v2_ref.leaf_hashes(bytes(corrupt[L:2 * L])))            # the layer of the corrupted bytes
    bad = []
    v = merkle_v2.BlockRepairVerifierV2(lay, flush_pieces=None, flush_age_ms=None, slots=2,
                                        leaf_source={1: wrong}.get, on_bad_blocks=lambda i, b: bad.append((i, b)))
    for m in _msgs(bytes(corrupt), lay, 1):
        v.on_block(m)
    assert v.flush() == [(1, False)]
    assert bad == [(1, [0, 1, 2, 3])] and 1 not in v._bufs and 1 not in v._have_blocks
    with pytest.raises(ValueError):                        # a leaf layer of the wrong size is the caller's error
        v.leaf_source = {1: wrong[:-32]}.get
        for m in _msgs(bytes(corrupt), lay, 1):
            v.on_block(m)
        v.flush()
