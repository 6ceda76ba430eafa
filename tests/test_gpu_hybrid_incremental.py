"""IncrementalVerifierHybrid and verify_piece_hybrid on the GPU, over a hybrid .torrent written by the tests' own bencoder
(tests/hybrid_util.py torrent_hybrid) and parsed by parse_metainfo_hybrid: blocks fed in random order with re-sends, two
slots (so flushes are forced), corrupted pieces, one piece with a flipped v1 digest and one with a flipped v2 hash.  The
expected have-bits are v1 AND v2 of hashlib SHA-1 over the padded linear bytes and the merkle reference."""
import random

import pytest

from tests import hybrid_util as hu
from tests import synth

pytestmark = pytest.mark.gpu
K = 1024
L = 64 * K
LENGTHS = [2 * L + 20000, L, 1, 3 * L - 17, 5]


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


@pytest.fixture(scope="module")
def fixture():
    """The files, the layout's expected values and the torrent's stated hashes: piece 1's v1 digest and piece 6's v2
    hash are stated wrongly."""
    files = [rnd(80 + k, n) for k, n in enumerate(LENGTHS)]
    lay = hu.Layout(files, L, trailing=True)
    pieces = hu.xor_at(lay.pieces, 20 * 1 + 3, 0x40)
    bad_v2 = 6
    return files, lay, pieces, bad_v2


def _torrent(files, lay, pieces, bad_v2):
    """The hybrid .torrent with the flipped v1 digest, and the flipped v2 hash in its file's piece layer (under the
    pieces root that layer reduces to, so the layer still is the one its root commits to)."""
    from tests import hybrid_fuzz
    from tests.v2_util import file_names
    d = hybrid_fuzz.HybridDraw(0, L, [len(f) for f in files], files, [], {}, trailing=True,
                               v1_flips={1: (3, 0x40)}, v2_flips={bad_v2: (9, 0x02)})
    stated_pieces, hashes = d.stated(lay)
    assert stated_pieces == pieces and hashes[bad_v2] == hu.xor_at(lay.hashes[bad_v2], 9, 0x02)
    return hybrid_fuzz.torrent(d, lay, file_names(len(files))), hashes


def _have(bitfield, i):
    return bool(bitfield[i >> 3] & (0x80 >> (i & 7)))


def _blocks(lay, staged, i):
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    f, o, b, _ = lay.table[i]
    d = staged[f][o:o + b]
    return [PieceMsg(i, q, bytes(d[q:q + BLOCK_SIZE])) for q in range(0, b, BLOCK_SIZE)]


def test_incremental_verifier_hybrid(native, fixture):
    from torrent_amd import IncrementalVerifierHybrid, parse_metainfo_hybrid
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    files, lay, pieces, bad_v2 = fixture
    data, hashes = _torrent(files, lay, pieces, bad_v2)
    meta = parse_metainfo_hybrid(data)
    assert meta is not None and meta.total_length == lay.total and meta.pieces == pieces
    assert meta.layout.hashes == b"".join(hashes) and meta.layout.piece_bytes == lay.pb
    P = lay.P
    rng = random.Random(21)
    staged = [bytearray(f) for f in files]
    staged[0][2 * L + 19999] ^= 0x08                        # piece 2: the last byte before its pad range
    staged[3][L + 77] ^= 0x01                               # piece 6 (its v2 hash is stated wrongly too)
    staged = [bytes(s) for s in staged]
    ok1, ok2, _, _ = lay.verdicts(staged, pieces, hashes)
    assert ok1 == [i not in (1, 2, 6) for i in range(P)] and ok2 == [i not in (2, 6) for i in range(P)]
    want = [a and b for a, b in zip(ok1, ok2)]
    msgs = [m for i in range(P) for m in _blocks(lay, staged, i)]
    rng.shuffle(msgs)
    msgs += rng.sample(msgs, 6)                             # re-sends
    seen = {}
    v = IncrementalVerifierHybrid(meta, flush_pieces=None, flush_age_ms=None, slots=2,
                                  on_verified=lambda i, ok: seen.setdefault(i, []).append(ok))
    try:
        stride = L + 256
        assert v.device_payload_bytes() == 2 * stride + 256
        for m in msgs:
            v.on_block(m)
        for i, ok in v.flush():
            seen.setdefault(i, []).append(ok)
        assert v.forced_flushes >= 2
        assert v.device_payload_bytes() == 2 * stride + 256
        assert v.ctx.last_kernel()[0] == native.KERNEL_HYBRID_LIST
        for i in range(P):
            assert seen[i][0] == want[i], i
            assert _have(v.bitfield, i) == want[i], i
        assert bytes(v.bitfield) == hu.pack(want)
        assert sorted(v.disagree) == [1]                    # exactly one description accepted piece 1's bytes
        # a failed piece can be received again and then passes: piece 2 with its own bytes
        for m in _blocks(lay, files, 2):
            v.on_block(m)
        assert v.flush() == [(2, True)] and _have(v.bitfield, 2)
        # ... and piece 6's good bytes still fail v2 alone: its hash is stated wrongly, so the descriptions disagree
        for m in _blocks(lay, files, 6):
            v.on_block(m)
        assert v.flush() == [(6, False)] and sorted(v.disagree) == [1, 6]
        with pytest.raises(ValueError):
            v.on_block(PieceMsg(2, 2 * BLOCK_SIZE, bytes(BLOCK_SIZE)))                   # a block inside the pad
    finally:
        v.close()


def test_verify_piece_hybrid(native, fixture):
    from torrent_amd import parse_metainfo_hybrid, verify_piece_hybrid
    files, lay, _, _ = fixture
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(files, L, trailing_pad=False))
    assert meta is not None and meta.total_length == lay.total - (L - 5)

    def piece(i):
        f, o, b, _ = lay.table[i]
        return files[f][o:o + b]

    assert verify_piece_hybrid(meta, 0, piece(0)) == (True, True, True)                   # a good piece
    assert verify_piece_hybrid(meta, 2, piece(2)) == (True, True, True)                   # a tail piece: 20,000 bytes + pad
    assert verify_piece_hybrid(meta, 4, piece(4)) == (True, True, True)                   # one byte + pad
    assert verify_piece_hybrid(meta, 8, piece(8)) == (True, True, True)                   # the short last piece: no pad
    assert verify_piece_hybrid(meta, 2, hu.xor_at(piece(2), 19999, 0x01)) == (False, False, False)   # a bad piece
    assert verify_piece_hybrid(meta, 3, hu.xor_at(piece(3), 0, 0x80)) == (False, False, False)
    assert verify_piece_hybrid(meta, 2, piece(2) + b"\0") == (False, False, False)        # the wrong length
    with pytest.raises(ValueError):
        verify_piece_hybrid(meta, 9, piece(0))
