"""The hosts of the v2 block calls on the GPU (torrent_amd/merkle_v2.py): leaf_hashes_v2 / check_blocks_v2 on one piece,
leaf_layers_files_v2 from disk feeding proof_v2 / check_proof_v2, and BlockRepairVerifierV2 end to end.  Expected
values come from tests/v2_ref.py (hashlib) and the golden layouts."""
import os

import pytest

from tests import synth, v2_ref
from tests.v2_util import file_names, golden, golden_files, torrent_v2

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384


def ref_layer(data, width: int) -> bytes:
    hs = v2_ref.leaf_hashes(data)
    return b"".join(hs + [bytes(32)] * (width - len(hs)))


@pytest.fixture(scope="module")
def gold(native):
    from torrent_amd import parse_metainfo_v2
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    files = list(golden_files("multi64k"))
    meta = parse_metainfo_v2(torrent_v2(files, golden()["multi64k"]["piece_length"], name="gold"))
    lay = meta.layout
    pieces = [files[lay.piece_file[i]][lay.piece_offset[i]:lay.piece_offset[i] + lay.piece_bytes[i]]
              for i in range(lay.n_pieces)]
    layers = [ref_layer(d, lay.tree_leaves[i]) for i, d in enumerate(pieces)]
    return meta, files, pieces, layers


def test_one_piece_calls(gold):
    from torrent_amd import check_blocks_v2, leaf_hashes_v2
    meta, files, pieces, layers = gold
    lay = meta.layout
    g = golden()["multi64k"]
    for i, d in enumerate(pieces):
        got = leaf_hashes_v2(meta, i, d)
        assert got == layers[i], i
        row = [got[q:q + 32] for q in range(0, len(got), 32)]
        assert len(row) == lay.tree_leaves[i] and v2_ref.reduce_row(row).hex() == g["piece_hashes"][i]
        assert check_blocks_v2(meta, i, d, layers[i]) == []
    i = max(range(lay.n_pieces), key=lambda p: lay.piece_bytes[p])          # a piece of several blocks
    d, nblocks = pieces[i], -(-lay.piece_bytes[i] // LEAF)
    assert nblocks >= 3
    bad = bytearray(d)
    bad[LEAF + 1] ^= 1
    bad[len(d) - 1] ^= 0x80
    assert check_blocks_v2(meta, i, bytes(bad), layers[i]) == [1, nblocks - 1]
    assert check_blocks_v2(meta, i, bytes(bad), layers[i], blocks=[0, 1]) == [1]
    assert check_blocks_v2(meta, i, bytes(bad), layers[i], blocks=[0]) == []
    assert check_blocks_v2(meta, i, bytes(bad), layers[i], blocks=[]) == []
    wrong = bytearray(layers[i])
    wrong[0] ^= 1
    assert check_blocks_v2(meta, i, d, bytes(wrong)) == [0]
    for call in (lambda: leaf_hashes_v2(meta, i, d[:-1]), lambda: check_blocks_v2(meta, i, d, layers[i][:-32]),
                 lambda: check_blocks_v2(meta, i, d, layers[i], blocks=[nblocks]),
                 lambda: leaf_hashes_v2(meta, lay.n_pieces, d)):
        with pytest.raises(ValueError):
            call()


def test_leaf_layers_from_disk_feed_proofs(gold, tmp_path):
    from torrent_amd import check_proof_v2, leaf_layers_files_v2, proof_v2
    meta, files, pieces, layers = gold
    lay = meta.layout
    L, P = lay.piece_length, lay.n_pieces
    W = L // LEAF
    for comps, data in zip(file_names(len(files)), files):
        p = tmp_path.joinpath(*comps)
        p.parent.mkdir(exist_ok=True)
        p.write_bytes(data)
    got = leaf_layers_files_v2(meta, str(tmp_path), range(P))
    assert got == dict(enumerate(layers))
    some = [P - 1, 0, 0, 3]
    assert leaf_layers_files_v2(meta, str(tmp_path), some) == {i: layers[i] for i in some}
    assert leaf_layers_files_v2(meta, str(tmp_path), []) == {}
    # a file of several pieces: a base-0 range across the boundary of its pieces 0 and 1, and a single block of each
    f = max(range(len(files)), key=lambda k: len(files[k]))
    assert len(files[f]) > 2 * L
    first = lay.file_first_piece[f]
    leaves = {first: got[first], first + 1: got[first + 1]}
    hashes, uncles = proof_v2(meta, f, 0, 0, 2 * W, leaves)
    assert b"".join(hashes) == layers[first] + layers[first + 1]
    assert check_proof_v2(meta, f, 0, 0, hashes, uncles)
    hashes, uncles = proof_v2(meta, f, 0, W - 2, 2, leaves)                 # the last two blocks of piece 0
    assert check_proof_v2(meta, f, 0, W - 2, hashes, uncles) and not check_proof_v2(meta, f, 0, W, hashes, uncles)
    hashes, uncles = proof_v2(meta, f, 0, W, 1, leaves)                     # the first block of piece 1
    assert hashes == [v2_ref.sha256(files[f][L:L + LEAF])] and check_proof_v2(meta, f, 0, W, hashes, uncles)
    with pytest.raises(KeyError):
        proof_v2(meta, f, 0, 2 * W, 1, leaves)                              # piece 2's layer was not supplied
    # a missing file
    os.remove(tmp_path.joinpath(*file_names(len(files))[f]))
    with pytest.raises(FileNotFoundError):
        leaf_layers_files_v2(meta, str(tmp_path), [first])
    other = next(i for i in range(P) if lay.piece_file[i] != f)
    assert leaf_layers_files_v2(meta, str(tmp_path), [other]) == {other: layers[other]}


def test_block_repair_verifier_end_to_end():
    from torrent_amd import BlockRepairVerifierV2, _native, parse_metainfo_v2
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    L = 64 * K
    data = bytes(synth.fill(55, 0, 3 * L))
    lay = parse_metainfo_v2(torrent_v2([data], L, name="one")).layout
    assert lay.n_pieces == 3
    layers = {i: ref_layer(data[i * L:(i + 1) * L], 4) for i in range(3)}
    msgs = [PieceMsg(i, o, data[i * L + o:i * L + o + BLOCK_SIZE]) for i in range(3) for o in range(0, L, BLOCK_SIZE)]
    bad = []
    v = BlockRepairVerifierV2(lay, flush_pieces=None, flush_age_ms=None, slots=3, leaf_source=layers.get,
                              on_bad_blocks=lambda i, blocks: bad.append((i, blocks)))
    try:
        for m in msgs:
            if (m.index, m.offset) == (1, 2 * BLOCK_SIZE):
                m = PieceMsg(1, m.offset, bytes([m.block[0] ^ 0x40]) + m.block[1:])
            v.on_block(m)
        assert v.flush() == [(0, True), (1, False), (2, True)]
        assert bad == [(1, [2])]
        assert v.ctx.counter(_native.TV_COUNTER_SLOTS_USED) == 0           # the check released the re-staged piece
        assert v.on_block(msgs[4 + 2]) is True             # block 2 of piece 1 alone completes the piece
        assert v.flush() == [(1, True)]
        assert bytes(v.bitfield) == b"\xe0" and bad == [(1, [2])]
    finally:
        v.close()
