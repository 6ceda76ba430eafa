"""Hybrid torrents on MI355X: the v1 (SHA-1 `pieces`) and the v2 (SHA-256 merkle, BEP 52) description of one payload,
verified or created from ONE staging (tv_hybrid_verify / tv_hybrid_hash in libtorrent_verify.so).

A hybrid info dict carries both descriptions; its v1 file list holds BEP 47 pad files (`attr` containing `p`) after every
file that does not end a piece, so every file starts a piece and the v1 linear space IS the aligned space the v2 calls
address.  A client must check both hash sets: a torrent whose descriptions disagree can feed different payloads to v1
and v2 peers, and BEP 52 tells clients to refuse it.  The library zeroes the pad ranges of the resident rows itself (pad
files are never looked for on disk, staged or read) and runs the SHA-1 kernel and the v2 kernels over the same bytes.

    parse_metainfo_hybrid(data) -> MetainfoHybrid | None          None unless v2 with v1 keys AND the two are consistent
    verify_payload_hybrid(meta, files_bytes, devices=None, stream=False) -> HybridResult     one buffer per (real) file
    verify_files_hybrid(meta, dir_path, devices=None, threads=None, stream=False) -> HybridResult
    verify_stream_hybrid(meta, read, devices=None, ...) -> HybridResult      through the bounded ring, any size
    hash_files_hybrid(dir_path, piece_length, ...) -> (v1 `pieces`, per-file v2 hashes)      creation mode
    hash_stream_hybrid(lengths, piece_length, read, ...) -> (v1 `pieces`, piece roots)       through the bounded ring
    make_torrent_hybrid(path, tracker, ...) -> bytes of a hybrid .torrent

They shard over `devices` as the v2 calls do.  The resident forms need every shard within the device budget;
verify_stream_hybrid and stream=True run both hash sets over the chunk buffers of one stream instead
(tv_hybrid_stream_begin / tv_hybrid_stream_file_table) and verify any size.

Pieces as they complete: verify_piece_hybrid(meta, index, data) -> (ok, v1_ok, v2_ok) checks one piece against both
descriptions, and incremental.IncrementalVerifierHybrid batches completed pieces on a slot pool; both are one
tv_hybrid_verify_list call (the pad range of each listed row zeroed on the device, then the SHA-1 list launch and the v2
list launch over the same bytes).
"""
from __future__ import annotations

import hashlib
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

from .bencode import bdecode_raw
from .metainfo_v2 import FileV2, MetainfoV2, V2Layout, make_layout, parse_metainfo_v2, valid_piece_length
from . import _native
from .v2 import (_creation_layout, _file_hashes, _file_paths, _file_tree, _resident_layout, _source_files,
                 _stage_file_buffers, _stage_files_v2, _stream_hash_table, _torrent, piece_length_for_v2)
from .verify import (_PIECE_SLOT, _bits_shards, _context, _file_options, _hash_shards, _layout, _safe_paths,
                     _shard_avail, _stream_rows)

CREATED_BY = "torrent_amd make_torrent_hybrid"


@dataclass
class MetainfoHybrid:
    """A consistent hybrid torrent: the v2 description, the v1 `pieces` string (20 bytes per piece of the v2 layout) and
    the v1 length, pad files included -- the layout's total_length, which gives every piece's v1 length: piece_length,
    except a last piece that no pad file follows."""
    v2: MetainfoV2
    pieces: bytes
    total_length: int
    info_hash: bytes                  # v1: SHA-1 over the raw info dict
    info_hash_v2: bytes               # v2: SHA-256 over the same bytes

    @property
    def name(self) -> str:
        return self.v2.name

    @property
    def piece_length(self) -> int:
        return self.v2.piece_length

    @property
    def files(self) -> List[FileV2]:
        return self.v2.files

    @property
    def layout(self) -> V2Layout:
        return self.v2.layout

    @property
    def n_pieces(self) -> int:
        return self.v2.layout.n_pieces


@dataclass
class HybridResult:
    """Have-bits of a hybrid verify: `bitfield` = v1 AND v2; `v1` and `v2` are the two descriptions' own bitfields."""
    bitfield: bytearray
    v1: bytearray
    v2: bytearray

    @property
    def disagree(self) -> List[int]:
        """The pieces one description accepts and the other refuses."""
        out = []
        for k, (a, b) in enumerate(zip(self.v1, self.v2)):
            x = a ^ b
            out += [8 * k + q for q in range(8) if x & (0x80 >> q)]
        return out


def _is_pad(entry: dict) -> bool:
    attr = entry.get(b"attr")
    return attr is not None and b"p" in bytes(attr)


def parse_metainfo_hybrid(data) -> Optional[MetainfoHybrid]:
    """A hybrid .torrent -> MetainfoHybrid, or None: not v2, no v1 keys, or the two descriptions are not consistent.
    Consistent: the v1 file list without its pad entries is the file tree's files, in order, with the same paths and
    lengths (`length` and `name` for a single-file torrent); every pad has exactly (-len_prev) mod piece_length bytes
    and follows a file that needs it, before the next file that holds bytes (one after the last file is accepted: the
    last v1 piece is then full); and `pieces` holds 20 bytes per piece of the v2 layout.  Both descriptions read the one
    `piece length` key, so a v1 side made for another piece length shows as wrong pads or a wrong `pieces` length."""
    try:
        v2 = parse_metainfo_v2(data)
        if v2 is None or not v2.hybrid:
            return None
        d, spans = bdecode_raw(data, spans=True)
        info = d[b"info"]
        L = v2.piece_length
        if info.get(b"piece length") != L:
            return None
        pieces = bytes(info[b"pieces"])
        if b"files" in info:
            entries = info[b"files"]
            if not isinstance(entries, list) or b"length" in info:
                return None
        else:
            entries = [{b"length": info[b"length"], b"path": [info[b"name"]]}]
        k, total, need_pad = 0, 0, 0
        for e in entries:
            n = e[b"length"]
            if not isinstance(n, int) or n < 0:
                return None
            if _is_pad(e):
                if need_pad == 0 or n != need_pad:         # a pad where none is needed, or of the wrong length
                    return None
                need_pad = 0
            else:
                if need_pad and n:                         # a missing pad (a zero-length file takes no bytes: the
                    return None                            # pad may stand on either side of it)
                path = [bytes(c).decode("utf-8", "replace") for c in e[b"path"]]
                if k >= len(v2.files) or path != v2.files[k].path or n != v2.files[k].length:
                    return None
                if n:
                    need_pad = -n % L
                k += 1
            total += n
        lay = v2.layout
        if k != len(v2.files) or len(pieces) != 20 * lay.n_pieces or -(-total // L) != lay.n_pieces:
            return None
        a, b = spans[b"info"]
        return MetainfoHybrid(v2=v2, pieces=pieces, total_length=total,
                              info_hash=hashlib.sha1(memoryview(data)[a:b]).digest(), info_hash_v2=v2.info_hash_v2)
    except Exception:
        return None


def _hybrid_layout(ctx, lay: V2Layout, total: int, first: int, count: int, hashes: Optional[bytes],
                   pieces: Optional[bytes], budget: Optional[int]) -> None:
    """set_layout over the v1 space (= the aligned space), the v2 piece table and, for a verify, the v1 digests."""
    _resident_layout(ctx, lay, first, count, hashes, budget, total, "a hybrid verify", "use more devices")
    if pieces is not None:
        ctx.set_digests(pieces)


def verify_stream_hybrid(meta: MetainfoHybrid, read, devices=None, avail: Optional[bytes] = None, chunk: int = 0,
                         threads: Optional[int] = None, budget: Optional[int] = None) -> HybridResult:
    """Both have-bitfields of a hybrid torrent through the library's BOUNDED pinned ring (tv_hybrid_stream_begin,
    tv_stream_*): one pass over the bytes, no resident shard, so a torrent of any size verifies within `budget` bytes of
    device memory (default 1 GiB).  read(file_index, offset, length) -> bytes | None is verify_stream_v2's: one row of
    a request, `length` bytes of REAL file `file_index` (file-tree order) from `offset`; None or a short result makes
    that piece unreadable (0 in all three bitfields).  Pad ranges are never asked for: the library writes their zeros
    on the device.  chunk=C > 0 asks for columns of C bytes (a power of two >= 16 KiB) across the whole shard."""
    lay = meta.layout

    def shard(ctx, first: int, count: int) -> tuple:
        _layout(ctx, meta.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False,
                chunk=chunk, digests=meta.pieces)
        return _stream_rows(
            ctx, threads, lambda i, offset, n: read(lay.piece_file[i], lay.piece_offset[i] + offset, n),
            lambda: ctx.hybrid_stream_begin(lay.piece_bytes, lay.tree_leaves, lay.hashes,
                                            _shard_avail(avail, first, count)),
            end=ctx.hybrid_stream_end)

    return HybridResult(*_bits_shards(devices, lay.n_pieces, shard, fields=3))


def verify_payload_hybrid(meta: MetainfoHybrid, files_bytes: Sequence, devices=None,
                          budget: Optional[int] = None, stream: bool = False) -> HybridResult:
    """Both have-bitfields of a hybrid torrent whose files are in host memory: files_bytes[k] is file k's bytes (the
    file tree's order; pad files have no buffer).  None, or a buffer shorter than the file, makes exactly the pieces it
    cannot supply unreadable (0 in all three bitfields).  stream=True verifies through the bounded ring
    (verify_stream_hybrid reading the buffers) and never raises for size; the default needs every shard resident within
    the budget."""
    lay = meta.layout
    if len(files_bytes) != len(meta.files):
        raise ValueError("verify_payload_hybrid: one buffer per file")
    views = [None if b is None else memoryview(b).cast("B") for b in files_bytes]
    if stream:
        def read(k: int, offset: int, n: int):
            mv = views[k]
            return None if mv is None or mv.nbytes < offset + n else mv[offset:offset + n]

        return verify_stream_hybrid(meta, read, devices=devices, budget=budget)
    lengths = [f.length for f in meta.files]

    def shard(ctx, first: int, count: int) -> tuple:
        _hybrid_layout(ctx, lay, meta.total_length, first, count, lay.hashes, meta.pieces, budget)
        return ctx.hybrid_verify(_stage_file_buffers(ctx, lay, views, lengths, first, count))

    return HybridResult(*_bits_shards(devices, lay.n_pieces, shard, fields=3))


def verify_files_hybrid(meta: MetainfoHybrid, dir_path: str, devices=None, threads: Optional[int] = None,
                        budget: Optional[int] = None, stream: bool = False) -> HybridResult:
    """Resume check of a hybrid torrent from disk.  Each real file is staged at its aligned offset (opened read-only);
    pad files are never looked for.  A missing or short file gives 0 bits for exactly the pieces it cannot supply.
    stream=True reads the files through the bounded ring in the library's own threads (tv_hybrid_stream_file_table) and
    never raises for size; the default needs every shard resident within the budget."""
    lay = meta.layout
    paths = _file_paths(meta.name, meta.files, dir_path)
    lengths = [f.length for f in meta.files]

    def stream_shard(ctx, first: int, count: int) -> tuple:
        _layout(ctx, meta.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False,
                digests=meta.pieces)
        _file_options(ctx, threads or ctx.thread_budget, False)          # a verify writes nothing: read-only
        try:
            return ctx.hybrid_stream_file_table(lay.piece_bytes, lay.tree_leaves, lay.hashes, lengths,
                                                _safe_paths(paths))[0]
        finally:
            ctx.set_option(_native.TV_OPT_OPEN_RW, 1)

    def shard(ctx, first: int, count: int) -> tuple:
        if stream:
            return stream_shard(ctx, first, count)
        _hybrid_layout(ctx, lay, meta.total_length, first, count, lay.hashes, meta.pieces, budget)
        _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget)
        return ctx.hybrid_verify()

    return HybridResult(*_bits_shards(devices, lay.n_pieces, shard, fields=3))


def verify_piece_hybrid(meta: MetainfoHybrid, index: int, data) -> tuple:
    """One piece of a hybrid torrent against both descriptions: (ok, v1_ok, v2_ok), ok = v1 AND v2.  `data` is the
    piece's file bytes (layout.piece_bytes[index] of them; the pad's zeros are written on the device, never passed);
    v1_ok: SHA-1 of the bytes and the pad zeros out to the piece's v1 length equals its `pieces` slice; v2_ok: the
    merkle root equals the piece's expected hash.  Raises ValueError for an index out of range; a piece of the wrong
    length is (False, False, False)."""
    lay = meta.layout
    if index < 0 or index >= lay.n_pieces:
        raise ValueError(f"verify_piece_hybrid: invalid piece index {index}")
    n = memoryview(data).nbytes
    if n != lay.piece_bytes[index]:
        return False, False, False
    L = lay.piece_length
    v1_len = min(L, meta.total_length - index * L)
    with _context(0, _PIECE_SLOT) as ctx:      # its own context: never evicts a bulk call's payload
        _layout(ctx, v1_len, L, 1, 0, 1, None, digests=meta.pieces[20 * index:20 * index + 20])
        ctx.stage(0, data)
        ok, v1, v2 = ctx.hybrid_verify_list([0], [n], [lay.tree_leaves[index]], lay.hashes[32 * index:32 * index + 32])
        return bool(ok[0]), bool(v1[0]), bool(v2[0])


def hash_stream_hybrid(lengths: Sequence[int], piece_length: int, read, devices=None, chunk: int = 0,
                       threads: Optional[int] = None, budget: Optional[int] = None) -> tuple:
    """Creation mode through the library's BOUNDED pinned ring (tv_hybrid_stream_hash_begin, tv_stream_*), both hash sets
    from one pass: (the v1 `pieces` string over the padded linear space -- no pad after the last file --, the 32-byte
    merkle root of every piece, in piece order) of the files of these lengths (file-tree order).  read(file_index,
    offset, length) -> bytes is verify_stream_hybrid's: pad ranges are never asked for.  A read that returns None or a
    short result raises FileNotFoundError."""
    if not valid_piece_length(piece_length):
        raise ValueError("a v2 piece length is a power of two >= 16 KiB")
    lay = make_layout(list(lengths), piece_length)

    def shard(ctx, first: int, count: int) -> tuple:
        _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False, chunk=chunk)
        return _stream_rows(
            ctx, threads, lambda i, offset, n: read(lay.piece_file[i], lay.piece_offset[i] + offset, n),
            lambda: ctx.hybrid_stream_hash_begin(lay.piece_bytes, lay.tree_leaves), end=ctx.stream_hash_end,
            must="hash_stream_hybrid")

    return _hash_shards(devices, lay.n_pieces, shard, fields=2)


def hash_files_hybrid(dir_path: str, piece_length: int, files: Optional[Sequence[tuple]] = None, devices=None,
                      threads: Optional[int] = None, budget: Optional[int] = None, stream: bool = False) -> tuple:
    """Creation mode from disk, both hash sets from one staging (tv_hybrid_hash): (the v1 `pieces` string over the
    padded linear space -- no pad after the last file --, [FileHashV2] as hash_files_v2 returns them).  files:
    [(path components, length)] in file-tree order (default: collect_files_v2).  Raises if a file is missing or short.
    stream=True hashes through the bounded ring in the library's own threads (tv_hybrid_stream_hash_file_table) and never
    raises for size; the default needs every shard resident within the budget."""
    files, lengths, lay, paths = _creation_layout(dir_path, piece_length, files)

    def shard(ctx, first: int, count: int) -> tuple:
        if stream:
            _layout(ctx, lay.total_length, lay.piece_length, lay.n_pieces, first, count, budget, resident=False)
            return _stream_hash_table(ctx, ctx.hybrid_stream_hash_file_table, lay, lengths, paths,
                                      threads or ctx.thread_budget, "hash_files_hybrid")
        _hybrid_layout(ctx, lay, lay.total_length, first, count, None, None, budget)
        _stage_files_v2(ctx, lay, lengths, paths, first, count, threads or ctx.thread_budget, must="hash_files_hybrid")
        return ctx.hybrid_hash()

    pieces, roots = _hash_shards(devices, lay.n_pieces, shard, fields=2)
    return pieces, _file_hashes(files, lay, roots)


def make_torrent_hybrid(path: str, tracker: str, comment: Optional[str] = None, creation_date: Optional[int] = None,
                        piece_length: Optional[int] = None, devices=None, budget: Optional[int] = None,
                        stream: bool = False) -> bytes:
    """A hybrid .torrent for a file or a directory: one info dict with the v1 keys (`files` with a pad entry --
    `attr` "p", path [".pad", "<length>"] -- after every file that does not end a piece, none after the last file that
    holds bytes; `length`
    for a single file; `pieces`) and the v2 keys (`meta version` 2, `file tree`), and the top-level `piece layers`.
    Both hash sets come from one staging on the GPU.  Dictionary keys are written sorted (canonical bencoding).
    stream=True hashes through the bounded ring (hash_files_hybrid), so a payload larger than `budget` bytes of device
    memory still makes its torrent."""
    name, base, files, single = _source_files(path)
    L = piece_length or piece_length_for_v2(sum(n for _, n in files))
    pieces, hashed = hash_files_hybrid(base, L, files=files, devices=devices, budget=budget, stream=stream)
    info: dict = {"file tree": _file_tree(hashed)}          # (bencode writes keys in insertion order: keep them sorted)
    if single:
        info["length"] = hashed[0].length
    else:
        v1_files = []
        for k, fh in enumerate(hashed):
            v1_files.append({"length": fh.length, "path": [os.fsencode(c) for c in fh.path]})
            pad = -fh.length % L
            if pad and any(later.length for later in hashed[k + 1:]):
                v1_files.append({"attr": "p", "length": pad, "path": [".pad", str(pad)]})
        info["files"] = v1_files
    info.update({"meta version": 2, "name": name, "piece length": L, "pieces": pieces})
    return _torrent(tracker, comment, creation_date, CREATED_BY, info, hashed)
