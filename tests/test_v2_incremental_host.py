"""Incremental BitTorrent v2 verify, the host side without a GPU: block validation against a V2Layout (every file's
last piece can be short), the flush cost model, and the new call's presence in the three bindings."""
import ctypes
import math
import os
import re

import pytest

from torrent_amd import _native
from torrent_amd.incremental import flush_cost_ms_v2, validate_received_block_v2
from torrent_amd.metainfo_v2 import make_layout
from torrent_amd.piece import BLOCK_SIZE, PieceMsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 65536
# file 0: three pieces, the last 20,000 bytes (a short last piece in the MIDDLE of the torrent); file 1: empty;
# file 2: one 16 KiB-multiple piece; file 3: the torrent's last piece, 1 byte
LAYOUT = make_layout([2 * L + 20000, 0, 32768, 1], L)


def msg(index, offset, n):
    return PieceMsg(index, offset, bytes(n))


def test_layout_of_the_fixture():
    assert LAYOUT.piece_bytes == [L, L, 20000, 32768, 1]


@pytest.mark.parametrize("index,offset,n", [
    (0, 0, BLOCK_SIZE), (0, L - BLOCK_SIZE, BLOCK_SIZE), (1, 32768, BLOCK_SIZE),
    (2, 0, BLOCK_SIZE), (2, BLOCK_SIZE, 20000 - BLOCK_SIZE),      # the middle file's short last piece
    (3, 0, BLOCK_SIZE), (3, BLOCK_SIZE, BLOCK_SIZE),              # a last block that is a whole block
    (4, 0, 1),
])
def test_valid_blocks_pass(index, offset, n):
    validate_received_block_v2(LAYOUT, msg(index, offset, n))


@pytest.mark.parametrize("index,offset,n,what", [
    (5, 0, BLOCK_SIZE, "piece index"), (99, 0, BLOCK_SIZE, "piece index"),
    (0, 1, BLOCK_SIZE, "block offset"), (0, BLOCK_SIZE + 64, BLOCK_SIZE, "block offset"),
    (0, L, BLOCK_SIZE, "block offset"),                           # at the piece's end
    (2, 2 * BLOCK_SIZE, BLOCK_SIZE, "block offset"),              # a whole block past the short piece's 20,000 bytes
    (4, BLOCK_SIZE, 1, "block offset"),
    (0, 0, BLOCK_SIZE - 1, "block length"), (0, 0, BLOCK_SIZE + 1, "block length"), (0, 0, 0, "block length"),
    (2, BLOCK_SIZE, BLOCK_SIZE, "block length"),                  # the short piece's last block sent whole
    (2, BLOCK_SIZE, 20000 - BLOCK_SIZE - 1, "block length"),
    (2, 0, 20000, "block length"),
    (3, BLOCK_SIZE, BLOCK_SIZE - 1, "block length"),
    (4, 0, BLOCK_SIZE, "block length"), (4, 0, 2, "block length"),
])
def test_invalid_blocks_raise(index, offset, n, what):
    with pytest.raises(ValueError, match=what):
        validate_received_block_v2(LAYOUT, msg(index, offset, n))


def test_null_ctx_is_an_argument_error():
    lib = _native.lib()
    assert lib.tv_v2_verify_list(None, 0, None, None, None, None, None) == _native.TV_ERR_ARG
    assert _native.KERNEL_V2_LIST == 16
    assert lib.tv_v2_verify_list.argtypes[1] is ctypes.c_uint64


def test_the_ts_symbol_table_names_the_call():
    ts = open(os.path.join(ROOT, "ts", "verify.ts"), encoding="utf-8").read()
    m = re.search(r"tv_v2_verify_list:\s*\{(.*?)\}", ts, re.S)
    assert m, "ts/verify.ts does not name tv_v2_verify_list"
    assert "nonblocking: true" in m.group(1)
    assert m.group(1).count('"pointer"') == 6 and '"u64"' in m.group(1)


def test_flush_cost_is_flat_in_the_piece_length_up_to_the_tree_levels():
    """One leaf plus log2 W levels: every doubling of the piece length adds the same two compressions, so the cost
    of a 1 GiB piece's flush is within 2 x 16 / 257 of a 16 KiB piece's (SHA-1's grows 65,536-fold)."""
    cost = [flush_cost_ms_v2(16384 << k) for k in range(17)]
    steps = [b - a for a, b in zip(cost, cost[1:])]
    assert all(s > 0 for s in steps)
    assert all(math.isclose(s, steps[0], rel_tol=1e-9) for s in steps)
    leaf = cost[0]
    assert steps[0] < leaf * 2 / 257 + 1e-12                # a level is two of the leaf's 257 compressions
    assert cost[16] < leaf * (1 + 32 / 257) + 1e-12
    assert flush_cost_ms_v2(4 << 20) / flush_cost_ms_v2(256 << 10) < 1.04
