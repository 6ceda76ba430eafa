"""Incremental hybrid verify, the host side without a GPU: tv_hybrid_verify_list in the three bindings, and
IncrementalVerifierHybrid over a recording stand-in for the context: the layout and digests it sets, its block validation
(the v2 side's: a short piece in the MIDDLE of the torrent; pads are never received), its flush cost model (the sum of
the v1 and the v2 model), and how it turns one hybrid_verify_list answer into have-bits and `disagree`."""
import ctypes
import os
import random
import re

import pytest

from tests import hybrid_util as hu
from torrent_amd import _native, incremental
from torrent_amd.hybrid import parse_metainfo_hybrid
from torrent_amd.incremental import (IncrementalVerifierHybrid, flush_cost_ms, flush_cost_ms_hybrid, flush_cost_ms_v2)
from torrent_amd.piece import BLOCK_SIZE, PieceMsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 65536
# file 0: three pieces, the last 20,000 bytes (a short piece in the middle, followed by a pad); file 1: one whole piece;
# file 2: 1 byte; file 3: three pieces, the last 17 bytes short; file 4: the torrent's last piece, 5 bytes
LENGTHS = [2 * L + 20000, L, 1, 3 * L - 17, 5]
PIECE_BYTES = [L, L, 20000, L, 1, L, L, L - 17, 5]


def _meta(trailing=False):
    rng = random.Random(5)
    files = [rng.randbytes(n) for n in LENGTHS]
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(files, L, trailing_pad=trailing))
    assert meta is not None and meta.layout.piece_bytes == PIECE_BYTES
    return meta, files


class FakeContext:
    """Records what the verifier hands the library; hybrid_verify_list answers from `verdicts` ({piece: (v1, v2)})."""

    def __init__(self, device=0):
        self.options, self.layout, self.digests, self.staged, self.lists = {}, None, None, [], []
        self.verdicts = {}

    def set_option(self, key, value):
        self.options[key] = value

    def set_layout(self, *args):
        self.layout = args

    def set_digests(self, pieces):
        self.digests = bytes(pieces)

    def stage(self, offset, buf):
        self.staged.append((offset, bytes(buf)))

    def hybrid_verify_list(self, pieces, piece_bytes, tree_leaves, hashes, release=True):
        self.lists.append((list(pieces), list(piece_bytes), list(tree_leaves), bytes(hashes), release))
        v1 = bytes(self.verdicts.get(i, (1, 1))[0] for i in pieces)
        v2 = bytes(self.verdicts.get(i, (1, 1))[1] for i in pieces)
        return bytes(a & b for a, b in zip(v1, v2)), v1, v2

    def close(self):
        pass


@pytest.fixture
def verifier(monkeypatch):
    monkeypatch.setattr(_native, "Context", FakeContext)

    def make(trailing=False, **kw):
        meta, files = _meta(trailing)
        kw.setdefault("flush_pieces", None)
        kw.setdefault("flush_age_ms", None)
        return IncrementalVerifierHybrid(meta, **kw), meta, files
    return make


def test_null_ctx_is_an_argument_error():
    lib = _native.lib()
    assert lib.tv_hybrid_verify_list(None, 0, None, None, None, None, None, None, None, 0) == _native.TV_ERR_ARG
    assert _native.KERNEL_HYBRID_LIST == 512


def test_ctypes_argtypes():
    at = _native.lib().tv_hybrid_verify_list.argtypes
    assert len(at) == 10
    assert at[1] is ctypes.c_uint64 and at[9] is ctypes.c_int
    assert all(a is ctypes.c_void_p for k, a in enumerate(at) if k not in (1, 9))
    assert _native.lib().tv_hybrid_verify_list.restype is ctypes.c_int


def test_the_ts_symbol_table_names_the_call():
    ts = open(os.path.join(ROOT, "ts", "verify.ts"), encoding="utf-8").read()
    m = re.search(r"tv_hybrid_verify_list:\s*\{(.*?)\}", ts, re.S)
    assert m, "ts/verify.ts does not name tv_hybrid_verify_list"
    assert "nonblocking: true" in m.group(1)
    params = re.findall(r'"(\w+)"', m.group(1).split("result")[0])
    assert params == ["pointer", "u64"] + ["pointer"] * 7 + ["i32"]


def test_the_package_exports_both_names():
    import torrent_amd
    assert torrent_amd.IncrementalVerifierHybrid is IncrementalVerifierHybrid
    assert callable(torrent_amd.verify_piece_hybrid)
    assert {"IncrementalVerifierHybrid", "verify_piece_hybrid"} <= set(torrent_amd.__all__)


@pytest.mark.parametrize("trailing", [False, True])
def test_the_context_is_a_slot_pool_over_the_v1_space(verifier, trailing):
    v, meta, files = verifier(trailing, slots=3)
    P = len(PIECE_BYTES)
    assert meta.total_length == (P * L if trailing else (P - 1) * L + 5)
    assert v.ctx.options[_native.TV_OPT_LIST_SLOTS] == 3
    assert v.ctx.layout == (meta.total_length, L, P, 0, P)
    assert v.ctx.digests == meta.pieces and len(meta.pieces) == 20 * P
    assert isinstance(v, incremental._Incremental)


@pytest.mark.parametrize("index,offset,n", [
    (0, 0, BLOCK_SIZE), (1, L - BLOCK_SIZE, BLOCK_SIZE),
    (2, 0, BLOCK_SIZE), (2, BLOCK_SIZE, 20000 - BLOCK_SIZE),      # the middle file's short last piece
    (4, 0, 1), (7, 3 * BLOCK_SIZE, BLOCK_SIZE - 17), (8, 0, 5),
])
def test_valid_blocks_pass(verifier, index, offset, n):
    v, _, _ = verifier()
    assert v.on_block(PieceMsg(index, offset, bytes(n))) in (False, True)


@pytest.mark.parametrize("index,offset,n,what", [
    (9, 0, BLOCK_SIZE, "piece index"),
    (0, 1, BLOCK_SIZE, "block offset"), (0, L, BLOCK_SIZE, "block offset"),
    (2, 2 * BLOCK_SIZE, BLOCK_SIZE, "block offset"),              # inside the pad that follows the 20,000 bytes
    (4, BLOCK_SIZE, BLOCK_SIZE, "block offset"),                  # ... and the one that follows the 1-byte file
    (2, BLOCK_SIZE, BLOCK_SIZE, "block length"),                  # the short piece's last block sent padded to a block
    (2, BLOCK_SIZE, 20000 - BLOCK_SIZE - 1, "block length"),
    (4, 0, BLOCK_SIZE, "block length"), (7, 3 * BLOCK_SIZE, BLOCK_SIZE, "block length"),
    (8, 0, BLOCK_SIZE, "block length"),
])
def test_invalid_blocks_raise(verifier, index, offset, n, what):
    v, _, _ = verifier(trailing=True)                             # (a trailing pad changes nothing: pads are never received)
    with pytest.raises(ValueError, match=what):
        v.on_block(PieceMsg(index, offset, bytes(n)))
    assert v.ctx.staged == []


def test_the_cost_model_is_the_sum_of_the_two_models(verifier):
    for k in range(17):
        n = 16384 << k
        assert flush_cost_ms_hybrid(n) == flush_cost_ms(n) + flush_cost_ms_v2(n)
    monkey_v, _, _ = verifier(flush_age_ms=incremental._AUTO)
    assert monkey_v.flush_age_ms == max(5.0, 10 * (flush_cost_ms(L) + flush_cost_ms_v2(L)))


def test_a_flush_is_one_call_and_the_have_bit_is_v1_and_v2(verifier):
    v, meta, files = verifier()
    lay = meta.layout
    order = [7, 2, 4, 0, 8]
    for i in order:
        f, o, n = lay.piece_file[i], lay.piece_offset[i], lay.piece_bytes[i]
        data = files[f][o:o + n]
        blocks = [(b, data[b:b + BLOCK_SIZE]) for b in range(0, n, BLOCK_SIZE)]
        done = [v.on_block(PieceMsg(i, b, blk)) for b, blk in blocks]
        assert done == [False] * (len(blocks) - 1) + [True]
    # staged at the piece's ALIGNED offset, file bytes only (no pad)
    assert v.ctx.staged == [(i * L, files[lay.piece_file[i]][lay.piece_offset[i]:][:lay.piece_bytes[i]]) for i in order]
    v.ctx.verdicts = {2: (1, 0), 4: (0, 1), 0: (0, 0)}
    res = v.flush()
    assert res == [(7, True), (2, False), (4, False), (0, False), (8, True)]
    assert len(v.ctx.lists) == 1
    pieces, pb, tl, hashes, release = v.ctx.lists[0]
    assert pieces == order and pb == [lay.piece_bytes[i] for i in order] and tl == [lay.tree_leaves[i] for i in order]
    assert hashes == b"".join(lay.hashes[32 * i:32 * i + 32] for i in order) and release
    assert v.disagree == [2, 4]                                   # exactly one description accepted them
    assert bytes(v.bitfield) == hu.pack([i in (7, 8) for i in range(len(PIECE_BYTES))])
    assert v.flush() == [] and len(v.ctx.lists) == 1
