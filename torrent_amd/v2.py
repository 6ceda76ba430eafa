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
    make_torrent_v2(path, tracker, ...) -> bytes of a v2-only .torrent

All of them shard over `devices` with shard_ranges, as the v1 calls do.  There is no CPU fallback for piece hashing
(only a file's P - 1 layer hashes and the info-hash are host work).  By default a shard must fit the device's resident
budget and a larger one raises; stream=True (and verify_stream_v2) verify through the library's bounded pinned ring
instead (tv_v2_stream_begin / tv_v2_stream_file_table): two chunk buffers within the budget, whatever the shard's
size.  Creation (hash_files_v2) is resident only; windowed resident v2 layouts are not built.
"""
from __future__ import annotations

import hashlib
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

from . import _native
from .bencode import bencode
from .metainfo_v2 import LEAF_BYTES, MetainfoV2, V2Layout, layer_root, make_layout, valid_piece_length
from .storage import copy_bytes
from .verify import (_PIECE_SLOT, _chunked_map, _concat, _context, _devices, _run_shards, _set_bit, _shard_avail,
                     _storage_threads)

CREATED_BY = "torrent_amd make_torrent_v2"


def _v2_layout(ctx, lay: V2Layout, first: int, count: int, hashes: Optional[bytes], budget: Optional[int]) -> None:
    """set_layout over the aligned space + the piece table; raises when the shard does not fit the resident budget."""
    ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, int(budget or 0))
    ctx.set_layout(lay.total_length, lay.piece_length, lay.n_pieces, first, count)
    if ctx.counter(_native.TV_COUNTER_WINDOW_PIECES):
        held = ctx.counter(_native.TV_COUNTER_BUDGET)
        raise MemoryError(f"v2 verify needs its shard resident: {count} pieces of {lay.piece_length} bytes exceed the "
                          f"device budget of {held} bytes (use more devices, or stream=True to verify through the "
                          f"bounded ring)")
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, hashes)


def _file_paths(meta_name: str, files: Sequence, dir_path: str) -> List[str]:
    """Where the files live under dir_path, by the rule of verify_files: a single-file torrent is [dir, name], a
    multi-file one [dir, *path] (without the torrent's name)."""
    if len(files) == 1 and list(files[0].path) == [meta_name]:
        return [os.path.join(dir_path, meta_name)]
    return [os.path.join(dir_path, *f.path) for f in files]


def _v2_stream_layout(ctx, lay: V2Layout, first: int, count: int, budget: Optional[int], chunk: int) -> None:
    """The layout of a streamed v2 check: no resident payload; the geometry comes from the budget or the chunk."""
    ctx.set_option(_native.TV_OPT_RESIDENT, 0)
    try:
        ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, int(budget or 0))
        ctx.set_option(_native.TV_OPT_STREAM_CHUNK, int(chunk or 0))
        ctx.set_layout(lay.total_length, lay.piece_length, lay.n_pieces, first, count)
    finally:
        ctx.set_option(_native.TV_OPT_RESIDENT, 1)


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
    P = lay.n_pieces

    def shard(ctx, first: int, count: int) -> bytes:
        _v2_stream_layout(ctx, lay, first, count, budget, chunk)
        nthr = _storage_threads(ctx, threads)
        pool = ThreadPoolExecutor(nthr) if nthr > 1 else None
        try:
            ctx.v2_stream_begin(lay.piece_bytes, lay.tree_leaves, lay.hashes, _shard_avail(avail, first, count))
            while True:
                req = ctx.stream_next()
                if not req.rows:
                    break

                def fill(q: int, req=req):
                    """Row q into the slot; returns the piece index when it is unreadable."""
                    n = ctx.row_bytes(req, q)
                    if n == 0:
                        return None
                    i = req.piece + q
                    data = read(lay.piece_file[i], lay.piece_offset[i] + req.offset, n)
                    if data is None or len(data) != n:
                        return i
                    copy_bytes(req.slot + q * req.width, data, n)
                    return None

                for i in _chunked_map(pool, fill, req.rows, nthr):
                    if i is not None:
                        ctx.stream_unreadable(i)
                ctx.stream_commit(req)
            return ctx.stream_end()
        except BaseException:
            ctx.stream_abort()
            raise
        finally:
            if pool is not None:
                pool.shutdown()
            ctx.set_option(_native.TV_OPT_STREAM_CHUNK, 0)

    if P == 0:
        return bytearray()
    ranges, slices = _run_shards(_devices(devices), P, shard)
    return _concat(slices, ranges, P)


def verify_payload_v2(meta: MetainfoV2, files_bytes: Sequence, devices=None, budget: Optional[int] = None,
                      stream: bool = False) -> bytearray:
    """Have-bitfield of a v2 torrent whose files are in host memory: files_bytes[k] is file k's bytes (file-tree
    order).  None, or a buffer shorter than the file, makes exactly the pieces it cannot supply unreadable (bit 0).
    stream=True verifies through the bounded ring (verify_stream_v2 reading the buffers) and never raises for size;
    the default needs every shard resident within the budget."""
    lay = meta.layout
    P, L = lay.n_pieces, lay.piece_length
    if len(files_bytes) != len(meta.files):
        raise ValueError("verify_payload_v2: one buffer per file")
    views = [None if b is None else memoryview(b).cast("B") for b in files_bytes]
    if stream:
        def read(k: int, offset: int, n: int):
            mv = views[k]
            return None if mv is None or mv.nbytes < offset + n else mv[offset:offset + n]

        return verify_stream_v2(meta, read, devices=devices, budget=budget)

    def shard(ctx, first: int, count: int) -> bytes:
        _v2_layout(ctx, lay, first, count, lay.hashes, budget)
        avail = bytearray((count + 7) // 8)
        for j in range(count):
            i = first + j
            mv = views[lay.piece_file[i]]
            if mv is not None and mv.nbytes >= lay.piece_offset[i] + lay.piece_bytes[i]:
                _set_bit(avail, j)
        # each file at its aligned offset (the library keeps the shard's part); bytes past a file's declared length
        # are not staged
        parts = []
        for k, mv in enumerate(views):
            n = 0 if mv is None else min(mv.nbytes, meta.files[k].length)
            if n and lay.file_offset[k] < (first + count) * L and lay.file_offset[k] + n > first * L:
                parts.append((lay.file_offset[k], mv[:n]))
        ctx.stage_many(parts)
        return ctx.v2_verify(avail)

    if P == 0:
        return bytearray()
    ranges, slices = _run_shards(_devices(devices), P, shard)
    return _concat(slices, ranges, P)


def _stage_files_v2(ctx, lay: V2Layout, lengths: Sequence[int], paths: Sequence[str], first: int, count: int,
                    threads: int) -> list:
    """One tv_stage_files segment per file that meets the shard, at its aligned offset, opened read-only.  The library
    marks the pieces a missing or short file cannot supply.  -> the per-segment statuses."""
    L = lay.piece_length
    lo, hi = first * L, (first + count) * L
    seg_paths, foff, lin, nbytes = [], [], [], []
    for k, n in enumerate(lengths):
        a, b = max(lo, lay.file_offset[k]), min(hi, lay.file_offset[k] + n)
        if b > a:
            seg_paths.append(paths[k] if "\0" not in paths[k] else "")
            foff.append(a - lay.file_offset[k])
            lin.append(a)
            nbytes.append(b - a)
    ctx.set_option(_native.TV_OPT_FILE_THREADS, max(1, threads))
    ctx.set_option(_native.TV_OPT_OPEN_RW, 0)          # a verify writes nothing: read-only
    try:
        return ctx.stage_files(seg_paths, foff, lin, nbytes)
    finally:
        ctx.set_option(_native.TV_OPT_OPEN_RW, 1)


def verify_files_v2(meta: MetainfoV2, dir_path: str, devices=None, threads: Optional[int] = None,
                    budget: Optional[int] = None, stream: bool = False) -> bytearray:
    """Resume check of a v2 torrent from disk: the have-bitfield of the files under dir_path.  A missing or short file
    gives 0 bits for exactly the pieces it cannot supply (the library's per-piece marking); nothing is created.
    stream=True reads the files through the bounded ring in the library's own threads (tv_v2_stream_file_table, files
    opened read-only) and never raises for size; the default needs every shard resident within the budget."""
    lay = meta.layout
    P = lay.n_pieces
    paths = _file_paths(meta.name, meta.files, dir_path)
    lengths = [f.length for f in meta.files]

    def stream_shard(ctx, first: int, count: int) -> bytes:
        _v2_stream_layout(ctx, lay, first, count, budget, 0)
        ctx.set_option(_native.TV_OPT_FILE_THREADS, max(1, threads or ctx.thread_budget))
        ctx.set_option(_native.TV_OPT_OPEN_RW, 0)          # a verify writes nothing: read-only
        try:
            safe = [p if "\0" not in p else "" for p in paths]
            return ctx.v2_stream_file_table(lay.piece_bytes, lay.tree_leaves, lay.hashes, lengths, safe)[0]
        finally:
            ctx.set_option(_native.TV_OPT_OPEN_RW, 1)

    def shard(ctx, first: int, count: int) -> bytes:
        if stream:
            return stream_shard(ctx, first, count)
        _v2_layout(ctx, lay, first, count, lay.hashes, budget)
        _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget)
        return ctx.v2_verify()

    if P == 0:
        return bytearray()
    ranges, slices = _run_shards(_devices(devices), P, shard)
    return _concat(slices, ranges, P)


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
        ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, 0)
        ctx.set_layout(n, lay.piece_length, 1, 0, 1)
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


def hash_files_v2(dir_path: str, piece_length: int, files: Optional[Sequence[tuple]] = None, devices=None,
                  threads: Optional[int] = None, budget: Optional[int] = None) -> List[FileHashV2]:
    """Creation mode from disk: the pieces root and piece layer of every file (files: [(path components, length)] in
    file-tree order; default: collect_files_v2(dir_path)).  The GPU emits the piece roots (tv_v2_hash); the host
    reduces each longer file's layer to its pieces root with hashlib (P - 1 small hashes).  Raises if a file is
    missing or short.  Files are opened read-only."""
    if not valid_piece_length(piece_length):
        raise ValueError("a v2 piece length is a power of two >= 16 KiB")
    files = collect_files_v2(dir_path) if files is None else list(files)
    lengths = [n for _, n in files]
    lay = make_layout(lengths, piece_length)
    paths = [os.path.join(dir_path, *comps) for comps, _ in files]
    P = lay.n_pieces

    def shard(ctx, first: int, count: int) -> bytes:
        _v2_layout(ctx, lay, first, count, None, budget)
        status = _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget)
        if any(st != _native.TV_OK for st in status):
            raise FileNotFoundError("hash_files_v2: a file is missing or shorter than its declared length")
        return ctx.v2_hash()

    roots = b""
    if P:
        _, slices = _run_shards(_devices(devices), P, shard)
        roots = b"".join(slices)
    out = []
    for k, (comps, n) in enumerate(files):
        p0 = lay.file_first_piece[k]
        count = -(-n // piece_length)
        layer = roots[32 * p0:32 * (p0 + count)]
        if n == 0:
            out.append(FileHashV2(list(comps), 0, None, b""))
        elif n <= piece_length:
            out.append(FileHashV2(list(comps), n, layer, b""))
        else:
            out.append(FileHashV2(list(comps), n, layer_root(layer, piece_length), layer))
    return out


def piece_length_for_v2(size: int) -> int:
    """A power of two near size / 1000, within 16 KiB .. 1 MiB (the v1 rule of make_torrent.ts:17-21 with v2's floor)."""
    L = LEAF_BYTES
    while L < (1 << 20) and L * 2000 <= size:
        L *= 2
    return L


def make_torrent_v2(path: str, tracker: str, comment: Optional[str] = None, creation_date: Optional[int] = None,
                    piece_length: Optional[int] = None, devices=None) -> bytes:
    """A v2-only .torrent (meta version 2: `file tree` + `piece layers`) for a file or a directory, piece roots hashed
    on the GPU.  Dictionary keys are written sorted, so the file is canonical bencoding."""
    path = os.path.abspath(path)
    name = os.path.basename(path)
    if os.path.isdir(path):
        base, files = path, collect_files_v2(path)
    else:
        base, files = os.path.dirname(path), [([name], os.stat(path).st_size)]
    L = piece_length or piece_length_for_v2(sum(n for _, n in files))
    hashed = hash_files_v2(base, L, files=files, devices=devices)
    tree: dict = {}
    for fh in hashed:
        node = tree
        for comp in fh.path:
            node = node.setdefault(os.fsencode(comp), {})
        node[b""] = {"length": fh.length, "pieces root": fh.pieces_root}   # (a None value is not written)
    layers = {fh.pieces_root: fh.layer for fh in hashed if fh.layer}
    return bencode({
        "announce": tracker,
        "comment": comment,
        "created by": CREATED_BY,
        "creation date": int(time.time()) if creation_date is None else creation_date,
        "info": {"file tree": tree, "meta version": 2, "name": name, "piece length": L},
        "piece layers": {k: layers[k] for k in sorted(layers)},
    })


def info_hash_v2(torrent: bytes) -> bytes:
    """SHA-256 over the raw info dict of a .torrent (host work, one hash per torrent)."""
    from .bencode import bdecode_raw
    _, spans = bdecode_raw(torrent, spans=True)
    a, b = spans[b"info"]
    return hashlib.sha256(torrent[a:b]).digest()
