"""BitTorrent v2 (BEP 52) below the piece: leaf layers, single blocks against them, and merkle proofs.

A v2 piece hash is the root of a SHA-256 tree over the piece's 16 KiB blocks so that a block can be checked on its
own.  The GPU's part is the leaves (tv_v2_leaf_hashes, tv_v2_check_blocks: one lane per block, one launch per call);
the tree above them is a few hundred small hashes, host work on hashlib like a file's `pieces root`.

    leaf_hashes_v2(meta, index, data) -> bytes                       the leaf layer of one piece
    check_blocks_v2(meta, index, data, leaf_layer, blocks=None) -> [bad block numbers]
    leaf_layers_files_v2(meta, dir_path, pieces, device=0) -> {piece: leaf layer}     a seeder's source, from disk
    proof_v2(meta, file_index, base, index, length, leaves=None) -> (hashes, uncles)
    check_proof_v2(meta, file_index, base, index, hashes, uncles) -> bool
    BlockRepairVerifierV2(layout, leaf_source=..., on_bad_blocks=...)    IncrementalVerifierV2 that names bad blocks

A piece's LEAF LAYER here is 32 x tree_leaves[piece] bytes: SHA-256 of each 16 KiB block that holds bytes (the last
one at its real length), then 32 zero bytes per padding leaf out to the width of the piece's tree.

A file's tree is next_pow2(ceil(length / 16 KiB)) leaves wide, H levels high; layer 0 is the leaves, layer H the
`pieces root`.  A file of at most `piece length` bytes is its one piece.  A longer file's piece layer (layer
log2(piece length / 16 KiB)) is its `piece layers` entry padded to a power of two with the root of an all-zero piece
subtree, as metainfo_v2.layer_root pads it; below the piece layer an all-zero subtree of height h is Z_h, with
Z_0 = 32 zero bytes and Z_(h+1) = SHA-256(Z_h || Z_h).

The wire protocol is out of scope here, as everywhere in this package: how many of the uncle hashes a `hashes` message
carries for a given `proof layers` field (a peer may omit the layers the receiver already has) is the wire layer's
business.  proof_v2 always returns, and check_proof_v2 always expects, every uncle up to the `pieces root`.
"""
from __future__ import annotations

import hashlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from . import _native
from .incremental import _AUTO, IncrementalVerifierV2
from .metainfo_v2 import LEAF_BYTES, MetainfoV2, next_pow2
from .piece import BLOCK_SIZE
from .verify import _PIECE_SLOT, _context

ZERO = bytes(32)


def _h2(a: bytes, b: bytes) -> bytes:
    return hashlib.sha256(a + b).digest()


def _log2(n: int) -> int:
    return n.bit_length() - 1


def _pow2(n) -> bool:
    return isinstance(n, int) and n > 0 and n & (n - 1) == 0


def _zero_root(h: int) -> bytes:
    z = ZERO
    for _ in range(h):
        z = _h2(z, z)
    return z


def _levels(row: List[bytes]) -> List[List[bytes]]:
    """Every level of the tree over a power-of-two row, bottom-up; the last holds the root."""
    out = [row]
    while len(row) > 1:
        row = [_h2(row[i], row[i + 1]) for i in range(0, len(row), 2)]
        out.append(row)
    return out


def _split(layer) -> List[bytes]:
    b = bytes(layer)
    if len(b) % 32:
        raise ValueError("a hash layer is a multiple of 32 bytes")
    return [b[i:i + 32] for i in range(0, len(b), 32)]


def _pad_layer(lay, index: int, leaf_layer) -> bytes:
    """A piece's leaf layer (32 x tree_leaves bytes) in the library's shape: out to W with zero hashes."""
    n = memoryview(leaf_layer).nbytes
    if n != 32 * lay.tree_leaves[index]:
        raise ValueError(f"the leaf layer of piece {index} is {32 * lay.tree_leaves[index]} bytes, not {n}")
    return bytes(leaf_layer) + bytes(32 * (lay.piece_length // LEAF_BYTES) - n)


# ---- one piece on the small context (as verify_piece_v2) --------------------------------------------------------------

def _one_piece(meta: MetainfoV2, index: int, data, what: str):
    lay = meta.layout
    if index < 0 or index >= lay.n_pieces:
        raise ValueError(f"{what}: invalid piece index {index}")
    n = memoryview(data).nbytes
    if n != lay.piece_bytes[index]:
        raise ValueError(f"{what}: piece {index} has {lay.piece_bytes[index]} bytes, not {n}")
    return lay, n


def leaf_hashes_v2(meta: MetainfoV2, index: int, data) -> bytes:
    """The leaf layer of one piece from its bytes: 32 x tree_leaves[index] bytes (tv_v2_leaf_hashes)."""
    lay, n = _one_piece(meta, index, data, "leaf_hashes_v2")
    with _context(0, _PIECE_SLOT) as ctx:      # its own context: never evicts a bulk call's payload
        ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, 0)
        ctx.set_layout(n, lay.piece_length, 1, 0, 1)
        ctx.stage(0, data)
        return ctx.v2_leaf_hashes([0], [n], [lay.tree_leaves[index]])[:32 * lay.tree_leaves[index]]


def check_blocks_v2(meta: MetainfoV2, index: int, data, leaf_layer, blocks: Optional[Sequence[int]] = None) -> List[int]:
    """The numbers of the 16 KiB blocks of one piece that do not match its leaf layer (tv_v2_check_blocks), ascending.
    blocks: the block numbers to check (default: every block of the piece); the others are neither read nor hashed."""
    lay, n = _one_piece(meta, index, data, "check_blocks_v2")
    W, nblocks = lay.piece_length // LEAF_BYTES, -(-n // LEAF_BYTES)
    want = sorted(set(range(nblocks) if blocks is None else blocks))
    if want and not 0 <= want[0] <= want[-1] < nblocks:
        raise ValueError(f"check_blocks_v2: piece {index} has blocks 0 .. {nblocks - 1}")
    bits = bytearray((W + 7) // 8)
    for i in want:
        bits[i >> 3] |= 0x80 >> (i & 7)
    with _context(0, _PIECE_SLOT) as ctx:
        ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, 0)
        ctx.set_layout(n, lay.piece_length, 1, 0, 1)
        ctx.stage(0, data)
        ok = ctx.v2_check_blocks([0], [n], [lay.tree_leaves[index]], _pad_layer(lay, index, leaf_layer), bytes(bits))
    return [i for i in want if not ok[i >> 3] & (0x80 >> (i & 7))]


# ---- a seeder's source: leaf layers of pieces on disk --------------------------------------------------------------------

_BATCH_BYTES = 1 << 30      # slot-pool bytes of one leaf_layers_files_v2 batch, at most (and at least one piece)


def leaf_layers_files_v2(meta: MetainfoV2, dir_path: str, pieces: Sequence[int], device: int = 0) -> Dict[int, bytes]:
    """{piece: its leaf layer} of the listed pieces of the files under dir_path: what a seeder answers a hash request
    from (proof_v2's `leaves`).  The pieces are staged from disk (read-only) into a slot pool and hashed by ONE
    tv_v2_leaf_hashes call; a list of more than TV_V2_BLOCKS_MAX leaf positions, or of more than 1 GiB of pieces, takes
    one call per such batch.  Raises FileNotFoundError when a file is missing or too short for a listed piece."""
    from .v2 import _file_paths
    lay = meta.layout
    L, W = lay.piece_length, lay.piece_length // LEAF_BYTES
    want = sorted(set(int(i) for i in pieces))
    if want and not 0 <= want[0] <= want[-1] < lay.n_pieces:
        raise ValueError("leaf_layers_files_v2: a piece index is out of range")
    paths = _file_paths(meta.name, meta.files, dir_path)
    batch = max(1, min(_native.TV_V2_BLOCKS_MAX // W, _BATCH_BYTES // L))
    out: Dict[int, bytes] = {}
    if not want:
        return out
    with _context(device) as ctx:
        ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, 0)
        ctx.set_option(_native.TV_OPT_LIST_SLOTS, min(batch, len(want)))
        ctx.set_option(_native.TV_OPT_OPEN_RW, 0)          # nothing is written: read-only
        try:
            ctx.set_layout(lay.total_length, L, lay.n_pieces)
            for a in range(0, len(want), batch):
                part = want[a:a + batch]
                try:
                    status = ctx.stage_files([paths[lay.piece_file[i]] for i in part],
                                             [lay.piece_offset[i] for i in part], [i * L for i in part],
                                             [lay.piece_bytes[i] for i in part])
                    if any(st != _native.TV_OK for st in status):
                        raise FileNotFoundError("leaf_layers_files_v2: a file is missing or shorter than its declared "
                                                "length")
                    got = ctx.v2_leaf_hashes(part, [lay.piece_bytes[i] for i in part],
                                             [lay.tree_leaves[i] for i in part], release=True)
                except BaseException:
                    ctx.set_layout(lay.total_length, L, lay.n_pieces)      # (drops the slots the batch took)
                    raise
                for k, i in enumerate(part):
                    out[i] = got[32 * W * k:32 * W * k + 32 * lay.tree_leaves[i]]
        finally:
            ctx.set_option(_native.TV_OPT_LIST_SLOTS, 0)
            ctx.set_option(_native.TV_OPT_OPEN_RW, 1)
    return out


# ---- proofs (host, hashlib) ------------------------------------------------------------------------------------------------

class _FileTree:
    """The nodes of one file's merkle tree: layers at or above the piece layer from the metainfo, layers below it from
    the leaf layers the caller supplies ({global piece index: leaf layer})."""

    def __init__(self, meta: MetainfoV2, file_index: int, leaves):
        if not 0 <= file_index < len(meta.files):
            raise ValueError(f"invalid file index {file_index}")
        f = meta.files[file_index]
        if f.length == 0:
            raise ValueError(f"file {file_index} is empty: it has no pieces root")
        lay = meta.layout
        L = meta.piece_length
        self.root = f.pieces_root
        self.width = next_pow2(-(-f.length // LEAF_BYTES))
        self.H = _log2(self.width)
        self.first = lay.file_first_piece[file_index]
        self.leaves = leaves if leaves is not None else {}
        self._piece_levels: Dict[int, List[List[bytes]]] = {}
        self._top: Optional[List[List[bytes]]] = None
        if f.length <= L:                       # the file is its one piece: the piece layer is the root
            self.hp, self.pieces, self._layer = self.H, 1, self.root
        else:
            self.hp, self.pieces = _log2(L // LEAF_BYTES), -(-f.length // L)
            self._layer = meta.piece_layers[f.pieces_root]

    def node(self, layer: int, j: int) -> bytes:
        if layer >= self.hp:
            if self._top is None:               # the piece layer, padded with all-zero piece subtrees, and up
                row = _split(self._layer)
                self._top = _levels(row + [_zero_root(self.hp)] * (next_pow2(len(row)) - len(row)))
            return self._top[layer - self.hp][j]
        q, local = j >> (self.hp - layer), j & ((1 << (self.hp - layer)) - 1)
        if q >= self.pieces:                    # inside the piece layer's padding: an all-zero subtree
            return _zero_root(layer)
        lv = self._piece_levels.get(q)
        if lv is None:
            row = _split(self.leaves[self.first + q])          # KeyError: the caller did not supply this piece
            if len(row) != 1 << self.hp:
                raise ValueError(f"the leaf layer of piece {self.first + q} is {32 << self.hp} bytes, not {32 * len(row)}")
            lv = self._piece_levels[q] = _levels(row)
        return lv[layer][local]


def _range_ok(t: _FileTree, base, index, length) -> bool:
    return (isinstance(base, int) and isinstance(index, int) and _pow2(length) and 0 <= base <= t.H and
            index >= 0 and index % length == 0 and index + length <= t.width >> base)


def proof_v2(meta: MetainfoV2, file_index: int, base: int, index: int, length: int,
             leaves: Optional[Dict[int, bytes]] = None) -> Tuple[List[bytes], List[bytes]]:
    """What answers a hash request for file `file_index`: (hashes, uncles).  hashes: the `length` nodes of layer `base`
    starting at node `index` (layer 0 = the leaves; length a power of two, index a multiple of it).  uncles: every
    uncle hash from that subtree's root up to the file's `pieces root`, bottom-up.  Layers at or above the piece layer
    come from the metainfo's `piece layers`; layers below it need leaves[piece] (leaf_layers_files_v2, leaf_hashes_v2)
    for every piece the range or its uncles touch inside one piece -- a missing one raises KeyError.  ValueError for a
    range the file's tree does not hold."""
    t = _FileTree(meta, file_index, leaves)
    if not _range_ok(t, base, index, length):
        raise ValueError(f"proof_v2: no aligned range of {length} nodes at {index} in layer {base} of a tree of "
                         f"{t.width} leaves")
    hashes = [t.node(base, index + k) for k in range(length)]
    layer, i = base + _log2(length), index // length
    uncles = []
    while layer < t.H:
        uncles.append(t.node(layer, i ^ 1))
        layer, i = layer + 1, i >> 1
    return hashes, uncles


def check_proof_v2(meta: MetainfoV2, file_index: int, base: int, index: int, hashes, uncles) -> bool:
    """Do `hashes` (nodes index .. of layer `base`, a list of 32-byte values or their concatenation) and `uncles`
    prove themselves against the file's `pieces root`?  The hashes are reduced to their subtree's root, the uncles are
    folded in by the bits of index, and the result is compared with the root.  The number of uncles must be EXACTLY
    H - base - log2(len(hashes)): were it not checked, the nodes of layer 1 passed as leaves with one uncle fewer
    would fold to the right root.  Malformed input (a peer's) is False, not an exception."""
    try:
        t = _FileTree(meta, file_index, None)
        row = _split(hashes) if isinstance(hashes, (bytes, bytearray, memoryview)) else [bytes(h) for h in hashes]
        unc = _split(uncles) if isinstance(uncles, (bytes, bytearray, memoryview)) else [bytes(u) for u in uncles]
    except (ValueError, TypeError, KeyError):
        return False
    if not _range_ok(t, base, index, len(row)) or any(len(h) != 32 for h in row + unc):
        return False
    if len(unc) != t.H - base - _log2(len(row)):
        return False
    node, i = _levels(row)[-1][0], index // len(row)
    for u in unc:
        node = _h2(u, node) if i & 1 else _h2(node, u)
        i >>= 1
    return node == t.root


# ---- incremental verify that names the bad blocks ------------------------------------------------------------------------

class BlockRepairVerifierV2(IncrementalVerifierV2):
    """IncrementalVerifierV2 that does not throw a failed piece away whole.  After a flush, every failed piece whose
    leaf layer is known -- leaf_source(index) -> 32 x tree_leaves[index] bytes, checked by the caller against the
    piece's hash (check_proof_v2), or None -- is staged again and its blocks are checked against that layer in ONE
    tv_v2_check_blocks launch.  The piece goes back to the assembling state with its good blocks present, and
    on_bad_blocks(index, [block numbers]) names the others: the piece completes again when only those arrive.  When no
    block is bad the layer contradicts the piece's hash, so every block counts as bad.  A failed piece with no leaf
    layer is forgotten, as in IncrementalVerifierV2.

    Cost: the host bytes of each pending piece are kept until its flush returns (the base class frees them once
    staged), i.e. up to pending x piece_length bytes of host memory, at most slots x piece_length."""

    def __init__(self, layout, storage=None, device: int = 0, shard=None, flush_pieces=_AUTO, flush_age_ms=_AUTO,
                 on_verified: Optional[Callable[[int, bool], None]] = None, slots: Optional[int] = None,
                 leaf_source: Optional[Callable[[int], Optional[bytes]]] = None,
                 on_bad_blocks: Optional[Callable[[int, List[int]], None]] = None):
        super().__init__(layout, storage, device, shard, flush_pieces, flush_age_ms, on_verified, slots)
        self.leaf_source = leaf_source
        self.on_bad_blocks = on_bad_blocks
        self._kept: Dict[int, bytearray] = {}    # pending piece -> its host bytes

    def _stage(self, index: int, buf) -> None:
        super()._stage(index, buf)
        self._kept[index] = buf

    def _flush_pending(self):
        out = super()._flush_pending()
        kept, self._kept = self._kept, {}
        lay = self.layout
        failed = []
        for i, ok in out:
            layer = None if ok or self.leaf_source is None else self.leaf_source(i)
            if layer is not None and i in kept:
                failed.append((i, _pad_layer(lay, i, layer)))
        if not failed:
            return out
        # the flush freed every slot, and at most `slots` pieces were pending: the failed ones fit again
        W = lay.piece_length // LEAF_BYTES
        idx = [i for i, _ in failed]
        for i in idx:
            IncrementalVerifierV2._stage(self, i, kept[i])
        bits = self.ctx.v2_check_blocks(idx, [lay.piece_bytes[i] for i in idx], [lay.tree_leaves[i] for i in idx],
                                        b"".join(layer for _, layer in failed), None, release=True)
        pitch = (W + 7) // 8
        for k, i in enumerate(idx):
            nblocks = -(-lay.piece_bytes[i] // BLOCK_SIZE)
            row = bits[k * pitch:(k + 1) * pitch]
            good = {b for b in range(nblocks) if row[b >> 3] & (0x80 >> (b & 7))}
            if len(good) == nblocks:            # the layer contradicts the piece's hash: nothing can be trusted
                good = set()
            if good:                            # back to assembling, the good blocks present
                self._bufs[i] = kept[i]
                self._have_blocks[i] = good
            if self.on_bad_blocks is not None:
                self.on_bad_blocks(i, [b for b in range(nblocks) if b not in good])
        return out
