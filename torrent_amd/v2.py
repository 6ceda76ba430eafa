"""BitTorrent v2 (BEP 52) verify and create on MI355X: SHA-256 merkle piece roots in libtorrent_verify.so.

A v2 piece hash is the root of a SHA-256 tree over the piece's 16 KiB blocks, so the GPU's serial unit is 16 KiB, not
a piece: the leaf kernel hashes every block of the resident shard side by side and a level-by-level reduce yields the
piece roots (torrent_amd/csrc/tv_v2_kernels.hip).  The host's part is the piece table (metainfo_v2.V2Layout) and the
staging: every file starts a new piece, so file k is staged at its ALIGNED linear offset (first piece x piece length).

    verify_payload_v2(meta, files_bytes, devices=None, stream=False) -> bytearray    one buffer per file
    verify_files_v2(meta, dir_path, devices=None, threads=None, stream=False) -> bytearray
    verify_stream_v2(meta, read, devices=None, avail=None, chunk=0, ...) -> bytearray    read(file, offset, length)
    verify_piece_v2(meta, index, data) -> bool
    hash_files_v2(dir_path, piece_length, files=None, ...) -> per-file pieces roots and layers (creation mode)
    hash_stream_v2(lengths, piece_length, read, ...) -> bytes      piece roots through the bounded ring
    make_torrent_v2(path, tracker, ...) -> bytes of a v2-only .torrent

All of them shard over `devices` with shard_ranges, as the v1 calls do.  There is no CPU fallback for piece hashing
(only a file's P - 1 layer hashes and the info-hash are host work).  By default a shard must fit the device's resident
budget and a larger one raises; stream=True (and verify_stream_v2) verify through the library's bounded pinned ring
instead (tv_v2_stream_begin / tv_v2_stream_file_table): two chunk buffers within the budget, whatever the shard's
size.  Creation is resident by default too; hash_stream_v2 and stream=True (hash_files_v2, make_torrent_v2) hash through
the same ring (tv_v2_stream_hash_begin / tv_v2_stream_hash_file_table).  Windowed resident v2 layouts are not built.
"""
from __future__ import annotations

import hashlib
import os
import time
from typing import List, Optional, Sequence

from . import _native
from .bencode import bencode
from .metainfo_v2 import LEAF_BYTES, MetainfoV2, V2Layout, layer_root, make_layout, valid_piece_length
from .verify import (_PIECE_SLOT, _bits_shards, _context, _file_options, _hash_shards, _layout, _require_resident,
                     _safe_paths, _set_bit, _shard_avail, _stream_rows)

CREATED_BY = "torrent_amd make_torrent_v2"


def _resident_layout(ctx, lay: V2Layout, first: int, count: int, hashes: Optional[bytes], budget: Optional[int],
                     total: Optional[int] = None, what: str = "v2 verify",
                     remedy: str = "use more devices, or stream=True to verify through the bounded ring") -> None:
    """set_layout over the aligned space (total: a hybrid torrent's v1 length instead) + the piece table; raises when the
    shard does not fit the resident budget."""
    _layout(ctx, lay.total_length if total is None else total, lay.piece_length, lay.n_pieces, first, count, budget)
    _require_resident(ctx, what, count, lay.piece_length, remedy)
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, hashes)


def _file_paths(meta_name: str, files: Sequence, dir_path: str) -> List[str]:
    """Where the files live under dir_path, by the rule of verify_files: a single-file torrent is [dir, name], a
    multi-file one [dir, *path] (without the torrent's name)."""
    if len(files) == 1 and list(files[0].path) == [meta_name]:
        return [os.path.join(dir_path, meta_name)]
    return [os.path.join(dir_path, *f.path) for f in files]


def verify_stream_v2(meta: MetainfoV2, read, devices=None, avail: Optional[bytes] = None, chunk: int = 0,
                     threads: Optional[int] = None, budget: Optional[int] = None) -> bytearray:
    """Resume check of a v2 torrent through the library's BOUNDED pinned ring (tv_v2_stream_begin, tv_stream_*): no
    resident shard and no whole-shard host buffer, so a torrent of any size verifies within `budget` bytes of device
    memory (default 1 GiB) and 3 x 64 MiB of host memory per device.  read(file_index, offset, length) -> bytes | None
    supplies one row of a request: `length` bytes of file `file_index` (file-tree order) from `offset` -- a v2 piece
    never spans files, so a row is one call; None or a short result makes that piece unreadable (bit 0).  By default
    the rows are whole pieces (or the widest power-of-two part of one that the budget holds 64 of); chunk=C > 0 asks
    for columns of C bytes (a power of two >= 16 KiB) across the whole shard.  The reads of a request are in flight
    together on `threads` threads, each writing its own row of the slot (as verify_stream)."""
    lay = meta.layout

    def shard(ctx, first: int, count: int) -> bytes:
        # no resident payload; the geometry comes from the budget or the chunk
        _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False, chunk=chunk)
        return _stream_rows(
            ctx, threads, lambda i, offset, n: read(lay.piece_file[i], lay.piece_offset[i] + offset, n),
            lambda: ctx.v2_stream_begin(lay.piece_bytes, lay.tree_leaves, lay.hashes, _shard_avail(avail, first, count)))

    return _bits_shards(devices, lay.n_pieces, shard)


def _stage_file_buffers(ctx, lay: V2Layout, views: Sequence, lengths: Sequence[int], first: int,
                        count: int) -> bytearray:
    """Stage the files held in host memory (views[k]: file k's bytes, or None) that meet the shard, each at its aligned
    offset (the library keeps the shard's part); bytes past a file's declared length are not staged.  -> the shard's
    availability bits: the pieces whose bytes are all there."""
    L = lay.piece_length
    avail = bytearray((count + 7) // 8)
    for j in range(count):
        i = first + j
        mv = views[lay.piece_file[i]]
        if mv is not None and mv.nbytes >= lay.piece_offset[i] + lay.piece_bytes[i]:
            _set_bit(avail, j)
    parts = []
    for k, mv in enumerate(views):
        n = 0 if mv is None else min(mv.nbytes, lengths[k])
        if n and lay.file_offset[k] < (first + count) * L and lay.file_offset[k] + n > first * L:
            parts.append((lay.file_offset[k], mv[:n]))
    ctx.stage_many(parts)
    return avail


def verify_payload_v2(meta: MetainfoV2, files_bytes: Sequence, devices=None, budget: Optional[int] = None,
                      stream: bool = False) -> bytearray:
    """Have-bitfield of a v2 torrent whose files are in host memory: files_bytes[k] is file k's bytes (file-tree
    order).  None, or a buffer shorter than the file, makes exactly the pieces it cannot supply unreadable (bit 0).
    stream=True verifies through the bounded ring (verify_stream_v2 reading the buffers) and never raises for size;
    the default needs every shard resident within the budget."""
    lay = meta.layout
    if len(files_bytes) != len(meta.files):
        raise ValueError("verify_payload_v2: one buffer per file")
    views = [None if b is None else memoryview(b).cast("B") for b in files_bytes]
    if stream:
        def read(k: int, offset: int, n: int):
            mv = views[k]
            return None if mv is None or mv.nbytes < offset + n else mv[offset:offset + n]

        return verify_stream_v2(meta, read, devices=devices, budget=budget)
    lengths = [f.length for f in meta.files]

    def shard(ctx, first: int, count: int) -> bytes:
        _resident_layout(ctx, lay, first, count, lay.hashes, budget)
        return ctx.v2_verify(_stage_file_buffers(ctx, lay, views, lengths, first, count))

    return _bits_shards(devices, lay.n_pieces, shard)


def _stage_files_v2(ctx, lay: V2Layout, lengths: Sequence[int], paths: Sequence[str], first: int, count: int,
                    threads: int, must: Optional[str] = None) -> None:
    """One tv_stage_files segment per file that meets the shard, at its aligned offset, opened read-only.  The library
    marks the pieces a missing or short file cannot supply; must="<the caller>": creation mode, where one is an error."""
    L = lay.piece_length
    lo, hi = first * L, (first + count) * L
    safe = _safe_paths(paths)
    seg_paths, foff, lin, nbytes = [], [], [], []
    for k, n in enumerate(lengths):
        a, b = max(lo, lay.file_offset[k]), min(hi, lay.file_offset[k] + n)
        if b > a:
            seg_paths.append(safe[k])
            foff.append(a - lay.file_offset[k])
            lin.append(a)
            nbytes.append(b - a)
    _file_options(ctx, threads, False)          # a verify writes nothing: read-only
    try:
        status = ctx.stage_files(seg_paths, foff, lin, nbytes)
    finally:
        ctx.set_option(_native.TV_OPT_OPEN_RW, 1)
    if must and any(st != _native.TV_OK for st in status):
        raise FileNotFoundError(f"{must}: a file is missing or shorter than its declared length")


def verify_files_v2(meta: MetainfoV2, dir_path: str, devices=None, threads: Optional[int] = None,
                    budget: Optional[int] = None, stream: bool = False) -> bytearray:
    """Resume check of a v2 torrent from disk: the have-bitfield of the files under dir_path.  A missing or short file
    gives 0 bits for exactly the pieces it cannot supply (the library's per-piece marking); nothing is created.
    stream=True reads the files through the bounded ring in the library's own threads (tv_v2_stream_file_table, files
    opened read-only) and never raises for size; the default needs every shard resident within the budget."""
    lay = meta.layout
    paths = _file_paths(meta.name, meta.files, dir_path)
    lengths = [f.length for f in meta.files]

    def stream_shard(ctx, first: int, count: int) -> bytes:
        _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False)
        _file_options(ctx, threads or ctx.thread_budget, False)          # a verify writes nothing: read-only
        try:
            return ctx.v2_stream_file_table(lay.piece_bytes, lay.tree_leaves, lay.hashes, lengths, _safe_paths(paths))[0]
        finally:
            ctx.set_option(_native.TV_OPT_OPEN_RW, 1)

    def shard(ctx, first: int, count: int) -> bytes:
        if stream:
            return stream_shard(ctx, first, count)
        _resident_layout(ctx, lay, first, count, lay.hashes, budget)
        _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget)
        return ctx.v2_verify()

    return _bits_shards(devices, lay.n_pieces, shard)


def verify_piece_v2(meta: MetainfoV2, index: int, data) -> bool:
    """One piece of a v2 torrent against its expected hash (its layer entry, or the pieces root of a one-piece file).
    Raises ValueError for an index out of range; a piece of the wrong length is False."""
    lay = meta.layout
    if index < 0 or index >= lay.n_pieces:
        raise ValueError(f"verify_piece_v2: invalid piece index {index}")
    n = memoryview(data).nbytes
    if n != lay.piece_bytes[index]:
        return False
    with _context(0, _PIECE_SLOT) as ctx:      # its own context: never evicts a bulk call's payload
        _layout(ctx, n, lay.piece_length, 1, 0, 1, None)
        ctx.v2_set_pieces([n], [lay.tree_leaves[index]], lay.hashes[32 * index:32 * index + 32])
        ctx.stage(0, data)
        return bool(ctx.v2_verify()[0] & 0x80)


class FileHashV2:
    """A file's v2 hashes: `pieces_root` (None for a zero-length file) and its piece `layer` (b"" unless the file is
    longer than one piece)."""

    def __init__(self, path: List[str], length: int, pieces_root: Optional[bytes], layer: bytes):
        self.path, self.length, self.pieces_root, self.layer = path, length, pieces_root, layer


def collect_files_v2(dir_path: str) -> List[tuple]:
    """[(path components, length)] of the files under dir_path in file-tree order: every level sorted by the raw
    bytes of its names, as a bencoded dictionary must be."""
    out = []
    for dp, dirs, names in os.walk(dir_path):
        for name in names:
            p = os.path.join(dp, name)
            out.append((os.path.relpath(p, dir_path).split(os.sep), os.stat(p).st_size))
    out.sort(key=lambda e: [os.fsencode(c) for c in e[0]])
    return out


def _creation_layout(dir_path: str, piece_length: int, files: Optional[Sequence[tuple]]) -> tuple:
    """(files, their lengths, the piece table, their paths under dir_path) of a creation call; files: [(path components,
    length)] in file-tree order (default: collect_files_v2(dir_path))."""
    if not valid_piece_length(piece_length):
        raise ValueError("a v2 piece length is a power of two >= 16 KiB")
    files = collect_files_v2(dir_path) if files is None else list(files)
    lengths = [n for _, n in files]
    return files, lengths, make_layout(lengths, piece_length), [os.path.join(dir_path, *comps) for comps, _ in files]


def _file_hashes(files: Sequence[tuple], lay: V2Layout, roots: bytes) -> List[FileHashV2]:
    """Every file's pieces root and piece layer from the piece roots of the whole layout (32 bytes per piece): the host
    reduces a longer file's layer to its pieces root with hashlib (P - 1 small hashes)."""
    L = lay.piece_length
    out = []
    for k, (comps, n) in enumerate(files):
        p0 = lay.file_first_piece[k]
        layer = roots[32 * p0:32 * (p0 + -(-n // L))]
        if n == 0:
            out.append(FileHashV2(list(comps), 0, None, b""))
        elif n <= L:
            out.append(FileHashV2(list(comps), n, layer, b""))
        else:
            out.append(FileHashV2(list(comps), n, layer_root(layer, L), layer))
    return out


def hash_stream_v2(lengths: Sequence[int], piece_length: int, read, devices=None, chunk: int = 0,
                   threads: Optional[int] = None, budget: Optional[int] = None) -> bytes:
    """Creation mode through the library's BOUNDED pinned ring (tv_v2_stream_hash_begin, tv_stream_*): the 32-byte merkle
    root of every piece of the files of these lengths (file-tree order; the aligned layout of make_layout), in piece
    order, within `budget` bytes of device memory (default 1 GiB) whatever the size.  read(file_index, offset, length)
    -> bytes is verify_stream_v2's, and so are the geometry and `chunk`.  Creation cannot skip a piece: a read that
    returns None or a short result raises FileNotFoundError."""
    if not valid_piece_length(piece_length):
        raise ValueError("a v2 piece length is a power of two >= 16 KiB")
    lay = make_layout(list(lengths), piece_length)

    def shard(ctx, first: int, count: int) -> bytes:
        _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False, chunk=chunk)
        return _stream_rows(
            ctx, threads, lambda i, offset, n: read(lay.piece_file[i], lay.piece_offset[i] + offset, n),
            lambda: ctx.v2_stream_hash_begin(lay.piece_bytes, lay.tree_leaves), end=ctx.stream_hash_end,
            must="hash_stream_v2")

    return _hash_shards(devices, lay.n_pieces, shard)


def _stream_hash_table(ctx, call, lay: V2Layout, lengths: Sequence[int], paths: Sequence[str], threads: int, what: str):
    """A creation stream's file-table call (ctx.v2_stream_hash_file_table or its hybrid form) after its layout: files
    opened read-only; a missing or short file raises, as the resident creation calls do."""
    _file_options(ctx, threads, False)
    try:
        out, _ = call(lay.piece_bytes, lay.tree_leaves, lengths, _safe_paths(paths))
    finally:
        ctx.set_option(_native.TV_OPT_OPEN_RW, 1)
    if out is None:
        raise FileNotFoundError(f"{what}: a file is missing or shorter than its declared length")
    return out


def hash_files_v2(dir_path: str, piece_length: int, files: Optional[Sequence[tuple]] = None, devices=None,
                  threads: Optional[int] = None, budget: Optional[int] = None,
                  stream: bool = False) -> List[FileHashV2]:
    """Creation mode from disk: the pieces root and piece layer of every file (files: [(path components, length)] in
    file-tree order; default: collect_files_v2(dir_path)).  The GPU emits the piece roots (tv_v2_hash); the host
    reduces each longer file's layer to its pieces root (_file_hashes).  Raises if a file is missing or short.  Files
    are opened read-only.  stream=True hashes through the bounded ring in the library's own threads
    (tv_v2_stream_hash_file_table) and never raises for size; the default needs every shard resident within the
    budget."""
    files, lengths, lay, paths = _creation_layout(dir_path, piece_length, files)

    def shard(ctx, first: int, count: int) -> bytes:
        if stream:
            _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False)
            return _stream_hash_table(ctx, ctx.v2_stream_hash_file_table, lay, lengths, paths,
                                      threads or ctx.thread_budget, "hash_files_v2")
        _resident_layout(ctx, lay, first, count, None, budget)
        _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget, must="hash_files_v2")
        return ctx.v2_hash()

    return _file_hashes(files, lay, _hash_shards(devices, lay.n_pieces, shard))


def piece_length_for_v2(size: int) -> int:
    """A power of two near size / 1000, within 16 KiB .. 1 MiB (the v1 rule of make_torrent.ts:17-21 with v2's floor)."""
    L = LEAF_BYTES
    while L < (1 << 20) and L * 2000 <= size:
        L *= 2
    return L


def _source_files(path: str) -> tuple:
    """(name, directory, [(path components, length)], whether it is a single file) of what a .torrent is made for."""
    path = os.path.abspath(path)
    name = os.path.basename(path)
    if os.path.isdir(path):
        return name, path, collect_files_v2(path), False
    return name, os.path.dirname(path), [([name], os.stat(path).st_size)], True


def _file_tree(hashed: Sequence[FileHashV2]) -> dict:
    tree: dict = {}
    for fh in hashed:
        node = tree
        for comp in fh.path:
            node = node.setdefault(os.fsencode(comp), {})
        node[b""] = {"length": fh.length, "pieces root": fh.pieces_root}   # (a None value is not written)
    return tree


def _torrent(tracker: str, comment: Optional[str], creation_date: Optional[int], created_by: str, info: dict,
             hashed: Sequence[FileHashV2]) -> bytes:
    """The bencoded .torrent around `info`, with the `piece layers` of the files longer than a piece."""
    layers = {fh.pieces_root: fh.layer for fh in hashed if fh.layer}
    return bencode({
        "announce": tracker,
        "comment": comment,
        "created by": created_by,
        "creation date": int(time.time()) if creation_date is None else creation_date,
        "info": info,
        "piece layers": {k: layers[k] for k in sorted(layers)},
    })


def make_torrent_v2(path: str, tracker: str, comment: Optional[str] = None, creation_date: Optional[int] = None,
                    piece_length: Optional[int] = None, devices=None, budget: Optional[int] = None,
                    stream: bool = False) -> bytes:
    """A v2-only .torrent (meta version 2: `file tree` + `piece layers`) for a file or a directory, piece roots hashed
    on the GPU.  Dictionary keys are written sorted, so the file is canonical bencoding.  stream=True hashes through the
    bounded ring (hash_files_v2), so a payload larger than `budget` bytes of device memory still makes its torrent."""
    name, base, files, _ = _source_files(path)
    L = piece_length or piece_length_for_v2(sum(n for _, n in files))
    hashed = hash_files_v2(base, L, files=files, devices=devices, budget=budget, stream=stream)
    info = {"file tree": _file_tree(hashed), "meta version": 2, "name": name, "piece length": L}
    return _torrent(tracker, comment, creation_date, CREATED_BY, info, hashed)


def info_hash_v2(torrent: bytes) -> bytes:
    """SHA-256 over the raw info dict of a .torrent (host work, one hash per torrent)."""
    from .bencode import bdecode_raw
    _, spans = bdecode_raw(torrent, spans=True)
    a, b = spans[b"info"]
    return hashlib.sha256(torrent[a:b]).digest()
