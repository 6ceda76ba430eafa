"""Many v1 torrents verified in one launch: the host side of the library's batch layout (tv_set_batch_layout,
tv_batch_select, tv_batch_verify; include/torrent_verify.h).

The reference client holds a map of torrents (client.ts: `torrents: Map<string, Torrent>`) and re-checks every one of
them when it starts.  SHA-1 is serial inside a piece, so a launch per torrent costs at least one piece's serial hash
each; a batch stages the torrents side by side in device memory and hashes all their pieces, of whatever piece
lengths, in ONE launch.

verify_payload_batch / verify_files_batch return, item by item, what verify_payload / verify_files return for the item
alone.  plan_batches cuts the items into consecutive batches that fit the device budget; an item that alone exceeds it
goes through the single-torrent call, which windows or streams."""
from __future__ import annotations

from typing import List, Optional, Sequence

from . import _native
from .metainfo import InfoDict
from .piece import piece_length
from .verify import (_bits_shards, _context, _file_options, _files_shard, _layout, _safe_paths, _set_bit, verify_files,
                     verify_payload)

_SLACK = 256          # bytes after the last region of a batch (tv_set_batch_layout)
_PAD = 256            # the library's stride pad: a row is the piece length rounded up to 64, plus this


def region_bytes(info: InfoDict) -> int:
    """The device bytes of a torrent's region in a batch: n_pieces rows of stride bytes, rounded up to 256 (every
    region starts 256-byte aligned)."""
    stride = -(-info.piece_length // 64) * 64 + _PAD
    return -(-info.n_pieces * stride // 256) * 256


def plan_batches(sizes: Sequence[int], budget: Optional[int]) -> List[tuple]:
    """Cut items of `sizes[k]` device bytes each (region_bytes) into consecutive runs under `budget` bytes (None or 0:
    no bound): [("batch", [k, ...]) | ("single", [k]), ...] in item order.  A batch is a greedy fill: the next item
    joins while the regions and the slack after them still fit the budget.  An item that alone does not fit is a
    "single": it goes through the single-torrent call, which windows or streams."""
    out: List[tuple] = []
    run: List[int] = []
    used = 0
    for k, size in enumerate(sizes):
        if budget and size + _SLACK > budget:
            if run:
                out.append(("batch", run))
            out.append(("single", [k]))
            run, used = [], 0
            continue
        if budget and run and used + size + _SLACK > budget:
            out.append(("batch", run))
            run, used = [], 0
        run.append(k)
        used += size
    if run:
        out.append(("batch", run))
    return out


def _run(items, device: int, budget: Optional[int], single, stage) -> List[bytearray]:
    """The batches of plan_batches on the cached context of `device`: stage(ctx, info, source) -> the item's
    availability bits or None, with the item selected and its digests set; single(info, source) -> its bitfield."""
    items = list(items)
    out: List[Optional[bytearray]] = [None] * len(items)
    for kind, ks in plan_batches([region_bytes(info) for info, _ in items], budget):
        if kind == "single":
            out[ks[0]] = bytearray(single(*items[ks[0]]))
            continue
        infos = [items[k][0] for k in ks]
        with _context(device) as ctx:
            ctx.set_option(_native.TV_OPT_RESIDENT, 1)
            ctx.set_option(_native.TV_OPT_RESIDENT_BUDGET, int(budget or 0))
            ctx.set_batch_layout([i.length for i in infos], [i.piece_length for i in infos],
                                 [i.n_pieces for i in infos])
            avail = bytearray()
            for t, k in enumerate(ks):
                info, source = items[k]
                ctx.batch_select(t)
                ctx.set_digests(info.pieces_raw)
                bits = stage(ctx, info, source) if info.n_pieces else None
                avail += bits if bits is not None else b"\xff" * ((info.n_pieces + 7) // 8)
            for k, bits in zip(ks, ctx.batch_verify(bytes(avail))):
                out[k] = bits
    return out


def verify_payload_batch(items, device: int = 0, budget: Optional[int] = None) -> List[bytearray]:
    """items = [(InfoDict, payload), ...], each payload the torrent's linear bytes in host memory -> one bitfield per
    item, equal to verify_payload(info, payload) for that item alone.  budget: device bytes a batch may take (default:
    the library's automatic budget)."""

    def stage(ctx, info: InfoDict, payload) -> bytearray:
        mv = memoryview(payload).cast("B")
        P, L = info.n_pieces, info.piece_length
        hi = min(P * L, len(mv))
        if hi:
            ctx.stage(0, mv[:hi])
        have = bytearray((P + 7) // 8)   # (verify_payload's rule: pieces whose bytes are not all present are unreadable)
        for i in range(P):
            if i * L + piece_length(i, info) <= len(mv):
                _set_bit(have, i)
        return have

    return _run(items, device, budget, lambda info, payload: verify_payload(info, payload, devices=[device], budget=budget),
                stage)


def verify_files_batch(items, device: int = 0, budget: Optional[int] = None, threads: Optional[int] = None,
                       open_rw: bool = True) -> List[bytearray]:
    """items = [(InfoDict, dir_path), ...] -> one bitfield per item, equal to verify_files(info, dir_path) for that item
    alone.  Each torrent's files are staged with one tv_stage_file_table call on the selected torrent: the library
    walks the file table as Storage.get does and marks the unreadable pieces itself.  threads: the library's reader
    threads; open_rw: files are opened read + write, as fsStorage.get opens them (False: read-only)."""
    from .storage import Storage, fs_storage

    def stage(ctx, info: InfoDict, dir_path) -> None:
        _file_options(ctx, threads or ctx.thread_budget, open_rw)
        lengths = [info.length] if info.files is None else [f.length for f in info.files]
        ctx.stage_file_table(lengths, _safe_paths(Storage(fs_storage, info, dir_path).file_paths()))
        return None

    def single(info: InfoDict, dir_path) -> bytearray:
        if open_rw:
            return verify_files(info, dir_path, devices=[device], threads=threads, budget=budget)
        storage = Storage(fs_storage, info, dir_path)

        def shard(ctx, first: int, count: int) -> bytes:
            _layout(ctx, info.length, info.piece_length, info.n_pieces, first, count, budget)
            ctx.set_digests(info.pieces_raw)
            return ctx.verify(_files_shard(ctx, info, storage, first, count, threads or ctx.thread_budget,
                                           open_rw=False))

        return _bits_shards([device], info.n_pieces, shard)

    return _run(items, device, budget, single, stage)
