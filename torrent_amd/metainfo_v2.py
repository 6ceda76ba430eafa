"""BitTorrent v2 (BEP 52) metainfo: parse_metainfo_v2 and the piece table a verify needs (V2Layout).

The reference's metainfo.ts knows v1 only (`pieces`, 20-byte SHA-1 digests).  A v2 info dict has `meta version` 2 and
a `file tree` (nested dictionaries of path components; a file is the dictionary under the empty key, holding `length`
and, when length > 0, `pieces root`); the top-level `piece layers` maps the pieces root of every file longer than one
piece to its layer of 32-byte piece hashes.  A hybrid torrent carries both descriptions and parses with both parsers.

Rules restated (they decide what the GPU is asked to hash, torrent_amd/v2.py):
* `piece length` L is a power of two >= 16 KiB; every file starts a new piece, and pieces are numbered in file-tree
  order as if pad files aligned each file to L; a zero-length file has no piece and no `pieces root`;
* a file longer than L: piece p's expected hash is entry p of its layer (32 * ceil(len / L) bytes), the root of the
  L / 16 KiB-leaf subtree of that piece with the missing leaves of the last piece zero hashes;
* a file of 1 .. L bytes is one piece, its expected hash is `pieces root` itself, and its tree is only
  next_pow2(ceil(len / 16 KiB)) leaves wide -- so the tree width is part of the table, not derivable from the bytes.
Any error returns None, the convention of parse_metainfo.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

from .bencode import bdecode_raw

LEAF_BYTES = 16384


@dataclass
class FileV2:
    path: List[str]
    length: int
    pieces_root: Optional[bytes]      # None for a zero-length file


@dataclass
class V2Layout:
    """The piece table of a v2 torrent, one row per piece, and where each file sits in the ALIGNED linear space the
    library addresses (piece p at p * piece_length)."""
    piece_length: int
    piece_file: List[int]             # index into files
    piece_offset: List[int]           # offset of the piece in its file
    piece_bytes: List[int]            # valid bytes (1 .. piece_length)
    tree_leaves: List[int]            # width of the piece's merkle tree
    hashes: bytes                     # 32 bytes per piece (b"" when the expected hashes are unknown: creation mode)
    file_offset: List[int]            # aligned linear offset of each file (a zero-length file: where the next starts)
    file_first_piece: List[int]       # first piece of each file

    @property
    def n_pieces(self) -> int:
        return len(self.piece_bytes)

    @property
    def total_length(self) -> int:
        """Length of the aligned space: the last piece ends at its valid bytes."""
        P = self.n_pieces
        return (P - 1) * self.piece_length + self.piece_bytes[-1] if P else 0


@dataclass
class MetainfoV2:
    info_hash_v2: bytes
    name: str
    piece_length: int
    files: List[FileV2]
    piece_layers: Dict[bytes, bytes] = field(repr=False, default_factory=dict)
    announce: Optional[str] = None
    hybrid: bool = False              # the info dict also holds the v1 keys (`pieces`)
    _layout: Optional[V2Layout] = field(default=None, repr=False, compare=False)

    @property
    def layout(self) -> V2Layout:
        if self._layout is None:
            self._layout = make_layout([f.length for f in self.files], self.piece_length,
                                       [f.pieces_root for f in self.files], self.piece_layers)
        return self._layout

    @property
    def n_pieces(self) -> int:
        return self.layout.n_pieces


def next_pow2(n: int) -> int:
    return 1 << max(0, n - 1).bit_length()


def valid_piece_length(L) -> bool:
    return isinstance(L, int) and L >= LEAF_BYTES and L & (L - 1) == 0


def make_layout(lengths, L: int, roots=None, layers=None) -> V2Layout:
    """The piece table of files of `lengths` (file-tree order) under piece length L.  roots / layers (pieces root per
    file, {pieces root: layer}) give the expected hashes; without them the table is a creation-mode one."""
    lay = V2Layout(L, [], [], [], [], b"", [], [])
    hashes = []
    W = L // LEAF_BYTES
    for f, n in enumerate(lengths):
        lay.file_offset.append(lay.n_pieces * L)
        lay.file_first_piece.append(lay.n_pieces)
        if n == 0:
            continue
        count = -(-n // L)
        for q in range(count):
            lay.piece_file.append(f)
            lay.piece_offset.append(q * L)
            lay.piece_bytes.append(min(L, n - q * L))
            lay.tree_leaves.append(W if n > L else next_pow2(-(-n // LEAF_BYTES)))
        if roots is not None:
            hashes.append(roots[f] if n <= L else bytes(layers[roots[f]]))
    lay.hashes = b"".join(hashes)
    return lay


def _reduce(row: List[bytes]) -> bytes:
    while len(row) > 1:
        row = [hashlib.sha256(row[i] + row[i + 1]).digest() for i in range(0, len(row), 2)]
    return row[0]


def layer_root(layer: bytes, L: int) -> bytes:
    """`pieces root` of a file from its piece layer: the layer padded to a power of two with the root of an all-zero-
    leaf piece subtree (NOT zero bytes), then reduced.  P - 1 small hashes: host work (hashlib), like the info-hash."""
    row = [layer[i:i + 32] for i in range(0, len(layer), 32)]
    pad = _reduce([bytes(32)] * (L // LEAF_BYTES))
    return _reduce(row + [pad] * (next_pow2(len(row)) - len(row)))


def _walk(tree: dict, prefix: List[str], out: List[FileV2]) -> None:
    for key, node in tree.items():                       # the order of the file: it numbers the pieces
        if not isinstance(node, dict) or key == b"":
            raise ValueError("malformed file tree")
        path = prefix + [key.decode("utf-8", "replace")]
        if b"" in node:
            leaf = node[b""]
            if len(node) != 1 or not isinstance(leaf, dict) or not isinstance(leaf.get(b"length"), int):
                raise ValueError("malformed file entry")
            n = leaf[b"length"]
            root = leaf.get(b"pieces root")
            if n < 0 or (n == 0) != (root is None) or (root is not None and len(root) != 32):
                raise ValueError("pieces root / length mismatch")
            out.append(FileV2(path, n, None if root is None else bytes(root)))
        else:
            _walk(node, path, out)


def parse_metainfo_v2(data) -> Optional[MetainfoV2]:
    """A v2-only or hybrid .torrent -> MetainfoV2, or None (not v2, or any error)."""
    try:
        d, spans = bdecode_raw(data, spans=True)
        info = d[b"info"]
        if info.get(b"meta version") != 2 or not isinstance(info.get(b"file tree"), dict):
            return None
        L = info.get(b"piece length")
        if not valid_piece_length(L):
            return None
        files: List[FileV2] = []
        _walk(info[b"file tree"], [], files)
        layers_in = d.get(b"piece layers", {})
        if not isinstance(layers_in, dict):
            return None
        layers = {}
        for f in files:
            if f.length > L:
                layer = layers_in.get(f.pieces_root)
                if layer is None or len(layer) != 32 * -(-f.length // L):
                    return None
                layer = bytes(layer)
                if layer_root(layer, L) != f.pieces_root:   # a layer that is not the one the info-hash commits to
                    return None
                layers[f.pieces_root] = layer
        a, b = spans[b"info"]
        return MetainfoV2(
            # SHA-256 over the raw bytes of the info dict as they stand in the file: one serial hash per torrent,
            # on the host (as the v1 info-hash)
            info_hash_v2=hashlib.sha256(memoryview(data)[a:b]).digest(),
            name=bytes(info[b"name"]).decode("utf-8", "replace"),
            piece_length=L, files=files, piece_layers=layers,
            announce=bytes(d[b"announce"]).decode("utf-8", "replace") if b"announce" in d else None,
            hybrid=b"pieces" in info)
    except Exception:
        return None
