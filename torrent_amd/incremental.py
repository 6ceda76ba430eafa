"""Incremental verification on piece completion.

The reference's piece-message handler (torrent.ts:183-193) validates a received block
(validateReceivedBlock, piece.ts:39-65) and writes it through Storage.set (storage.ts:67-87), but
never checks a completed piece: Torrent.bitfield stays all zero (torrent.ts:60).  This class adds
that check with the same inputs:

    v = IncrementalVerifier(info, storage)          # storage: the reference's Storage (optional)
    v.on_block(PieceMsg(index, offset, block))      # per received block; True when the piece is complete
    for index, ok in v.flush():                     # ONE GPU launch (tv_verify_list) for all pending pieces
        if ok: send_have(index)                     # v.bitfield already has the bit (torrent.ts:147-149)

A completed piece's bytes are staged into HBM as soon as its last block arrives; flush() verifies
every pending piece in one list launch.  A piece that fails verification is forgotten (its blocks
may be received again), as a client would re-request it.

Device memory is bounded by the pieces AWAITING verification, not by the torrent: the context is a slot
pool of K = `slots` pieces (TV_OPT_LIST_SLOTS; default the flush count, 4,096), a completed piece takes a
slot when it is staged and gives it back when its flush returns, and when all K slots are taken the next
completed piece first flushes the pending ones.  A 200 GiB torrent of 4 MiB pieces holds K x 4 MiB of HBM.

Flush policy.  A list flush costs about one piece's serial SHA-1 whatever the list length, ~0.73 us per
64-B block: 3.0 ms for 256 KiB pieces, whether 1 or 4,096 of them (3.00 / 3.01 / 3.15 ms for 1 / 64 /
4,096; profiles/r02/latency_twin.json, r03 latency).  Flushing per piece therefore costs ~3 ms of GPU time
per piece; batching is the point.  The verifier flushes by itself when
  * `flush_pieces` pieces are pending (default 4,096: the flush time is still flat there), or
  * the oldest pending piece has waited `flush_age_ms` (default 10 x the flush cost, at least 5 ms: 30 ms
    for 256 KiB pieces), checked on every on_block() and by poll() -- so the GPU spends at most ~10 % of
    its time on flushes while pieces trickle in, and a have-bit is at most ~1.1 x flush_age_ms late.
Results of automatic flushes go to `on_verified(index, ok)` when given, else they are returned by the
next flush() / poll().  flush_pieces=1 restores flush-per-piece; flush_age_ms=None with
flush_pieces=None leaves flushing to the caller.

IncrementalVerifierV2 is the same for a BitTorrent v2 torrent: a flush is one tv_v2_verify_list launch (SHA-256
merkle roots, each piece's tree inside one workgroup), whose serial unit is one 16 KiB leaf plus log2 W tree nodes
whatever the piece length (flush_cost_ms_v2), so its age bound does not grow with the piece length.
merkle_v2.BlockRepairVerifierV2 extends it: a failed piece whose leaf layer is known keeps its good blocks and only
the bad ones are named for re-download.

IncrementalVerifierHybrid is the same for a hybrid torrent (hybrid.MetainfoHybrid): a flush is one
tv_hybrid_verify_list call, both hashes of every pending piece from its one staging; a piece's have-bit is v1 AND v2,
and `disagree` names the pieces exactly one description accepted.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, List, Optional, Tuple

from . import _native
from .metainfo import InfoDict
from .metainfo_v2 import V2Layout
from .piece import BLOCK_SIZE, PieceMsg, _stringify, piece_length, validate_received_block

US_PER_BLOCK = 0.73       # list-flush time per 64-B block of one piece (kernel 2.94-2.98 ms / 4,097 blocks)
DEFAULT_FLUSH_PIECES = 4096
_AUTO = object()


def flush_cost_ms(piece_len: int) -> float:
    """Estimated GPU time of one list flush of pieces of `piece_len` bytes: one piece's serial SHA-1."""
    return ((piece_len + 8) // 64 + 1) * US_PER_BLOCK / 1e3 + 0.06


class _Incremental:
    """What the v1 and v2 verifiers share: block assembly, the slot pool's forced flushes, the flush policy and the
    result hand-out.  A subclass sets up its context and says what a piece is: _validate, _piece_bytes,
    _storage_offset, _stage and _verify_list."""

    def _init_policy(self, n_pieces: int, shard, flush_pieces, flush_age_ms, flush_cost: float, on_verified,
                     slots) -> None:
        self.flush_pieces = DEFAULT_FLUSH_PIECES if flush_pieces is _AUTO else flush_pieces
        self.flush_age_ms = max(5.0, 10 * flush_cost) if flush_age_ms is _AUTO else flush_age_ms
        self.on_verified = on_verified
        self.auto_flushes = 0
        self._oldest = 0.0                # time.monotonic() of the oldest pending piece
        self._results: List[Tuple[int, bool]] = []   # automatic flushes' results not yet handed out
        self.first, self.count = shard if shard is not None else (0, n_pieces)
        # the slot pool: K pieces of HBM awaiting verification (at least the count bound, so it never forces
        # a flush the policy would not make)
        if slots is None:
            slots = self.flush_pieces if isinstance(self.flush_pieces, int) else DEFAULT_FLUSH_PIECES
        self.slots = max(1, min(int(slots), max(1, self.count)))
        self.forced_flushes = 0
        self.bitfield = bytearray((n_pieces + 7) // 8)   # torrent.ts:60
        self._bufs: Dict[int, bytearray] = {}
        self._have_blocks: Dict[int, set] = {}
        self._pending: List[int] = []
        self._pending_set: set = set()

    # -- what a piece is (subclasses) --------------------------------------------------------------
    def _validate(self, msg: PieceMsg) -> None:
        raise NotImplementedError

    def _piece_bytes(self, index: int) -> int:
        raise NotImplementedError

    def _storage_offset(self, index: int, offset: int) -> int:
        raise NotImplementedError

    def _stage(self, index: int, buf) -> None:
        raise NotImplementedError

    def _verify_list(self, pending: List[int]) -> bytes:
        raise NotImplementedError

    # -- blocks ------------------------------------------------------------------------------------
    def on_block(self, msg: PieceMsg) -> bool:
        """Handle one received block (torrent.ts:183-193).  Raises ValueError for an invalid block
        (piece.ts:39-65).  Returns True when this block completed its piece."""
        self._validate(msg)
        self._auto_flush()                                # the age bound, checked on every block
        i = msg.index
        if not (self.first <= i < self.first + self.count):
            raise ValueError(f"piece {i} is outside this verifier's shard")
        if self.storage is not None:
            self.storage.set(self._storage_offset(i, msg.offset), msg.block)
        if self.bitfield[i >> 3] & (0x80 >> (i & 7)):
            return False                                  # already verified
        if i in self._pending_set:
            return False                                  # complete and staged, waiting for flush()
        plen = self._piece_bytes(i)
        if msg.offset >= plen:
            return False
        block = memoryview(msg.block)[:plen - msg.offset]  # never past the piece (L % BLOCK_SIZE != 0)
        buf = self._bufs.get(i)
        if buf is None:
            buf = self._bufs[i] = bytearray(plen)
            self._have_blocks[i] = set()
        buf[msg.offset:msg.offset + len(block)] = block
        blocks = self._have_blocks[i]
        blocks.add(msg.offset // BLOCK_SIZE)
        done = False
        if len(blocks) == -(-plen // BLOCK_SIZE):
            if len(self._pending) >= self.slots:          # every slot awaits a flush: make room
                self.forced_flushes += 1
                self._deliver(self._flush_pending())
            self._stage(i, buf)
            del self._bufs[i], self._have_blocks[i]
            if not self._pending:
                self._oldest = time.monotonic()
            self._pending.append(i)
            self._pending_set.add(i)
            done = True
            self._auto_flush()                            # the count bound
        return done

    # -- the flush policy --------------------------------------------------------------------------
    def due(self) -> bool:
        """Would the flush policy flush now (enough pieces pending, or the oldest old enough)?"""
        if not self._pending:
            return False
        if self.flush_pieces is not None and len(self._pending) >= self.flush_pieces:
            return True
        return (self.flush_age_ms is not None and
                (time.monotonic() - self._oldest) * 1e3 >= self.flush_age_ms)

    def _deliver(self, res: List[Tuple[int, bool]]) -> None:
        if self.on_verified is not None:
            for i, ok in res:
                self.on_verified(i, ok)
        else:
            self._results.extend(res)

    def _auto_flush(self) -> None:
        if self.due():
            self.auto_flushes += 1
            self._deliver(self._flush_pending())

    def poll(self) -> List[Tuple[int, bool]]:
        """For a client's event loop: flush if the policy says so, and hand out every result the automatic
        flushes have not yet returned."""
        self._auto_flush()
        out, self._results = self._results, []
        return out

    def _flush_pending(self) -> List[Tuple[int, bool]]:
        if not self._pending:
            return []
        pending, self._pending = self._pending, []
        self._pending_set.clear()
        ok = self._verify_list(pending)
        out = []
        for i, r in zip(pending, ok):
            if r:
                self.bitfield[i >> 3] |= 0x80 >> (i & 7)
            out.append((i, bool(r)))
        return out

    def flush(self) -> List[Tuple[int, bool]]:
        """Verify every completed, not yet verified piece in one launch; set have-bits.  Returns its results
        after those of earlier automatic flushes not yet handed out (none when on_verified is set)."""
        out, self._results = self._results, []
        return out + self._flush_pending()

    def device_payload_bytes(self) -> int:
        """HBM the verifier's payload holds (TV_COUNTER_PAYLOAD_BYTES): the K slots, whatever the torrent."""
        return self.ctx.counter(_native.TV_COUNTER_PAYLOAD_BYTES)

    def close(self) -> None:
        self.ctx.close()


class IncrementalVerifier(_Incremental):
    def __init__(self, info: InfoDict, storage=None, device: int = 0,
                 shard: Optional[Tuple[int, int]] = None, flush_pieces=_AUTO, flush_age_ms=_AUTO,
                 on_verified: Optional[Callable[[int, bool], None]] = None, slots: Optional[int] = None):
        self.info = info
        self.storage = storage
        P = info.n_pieces
        self._init_policy(P, shard, flush_pieces, flush_age_ms, flush_cost_ms(info.piece_length), on_verified, slots)
        self.ctx = _native.Context(device)
        self.ctx.set_option(_native.TV_OPT_LIST_SLOTS, self.slots)
        self.ctx.set_layout(info.length, info.piece_length, P, self.first, self.count)
        self.ctx.set_digests(info.pieces_raw)

    def _validate(self, msg: PieceMsg) -> None:
        validate_received_block(self.info, msg)

    def _piece_bytes(self, index: int) -> int:
        return piece_length(index, self.info)

    def _storage_offset(self, index: int, offset: int) -> int:
        return index * self.info.piece_length + offset

    def _stage(self, index: int, buf) -> None:
        self.ctx.stage(index * self.info.piece_length, buf)

    def _verify_list(self, pending: List[int]) -> bytes:
        return self.ctx.verify_list(pending)


# ---- BitTorrent v2 (BEP 52) ----------------------------------------------------------------------------------------
# A v2 list flush (tv_v2_verify_list) costs one 16 KiB leaf (257 compressions: 256 of data and the padding block) and
# log2 W two-compression tree nodes in series, whatever the piece length.  Microseconds per serial SHA-256 compression
# in a flush and the fixed part of a call, from profiles/v2/list_latency.json: kernel_ms of the 1- and 64-piece
# flushes, 0.67-0.78 ms at 256 KiB pieces (265 serial compressions) and 0.69-0.70 ms at 4 MiB (273), i.e. 2.5-2.9 us
# each (one wave per SIMD: latency, not throughput); total_ms - kernel_ms is 0.02-0.04 ms.
US_PER_COMPRESSION_V2 = 2.6
FLUSH_FIXED_MS_V2 = 0.03
LEAF_COMPRESSIONS_V2 = 257


def flush_cost_ms_v2(piece_len: int) -> float:
    """Estimated GPU time of one v2 list flush of pieces of `piece_len` bytes: one leaf and log2 W tree levels."""
    levels = max(1, piece_len // BLOCK_SIZE).bit_length() - 1
    return (LEAF_COMPRESSIONS_V2 + 2 * levels) * US_PER_COMPRESSION_V2 / 1e3 + FLUSH_FIXED_MS_V2


def validate_received_block_v2(layout: V2Layout, msg: PieceMsg) -> None:
    """validate_received_block for a v2 torrent: every file's last piece can be short (piece_bytes[index] valid
    bytes), not only the torrent's last one, so the last block of ANY piece is checked against its own length."""
    if not 0 <= msg.index < layout.n_pieces:
        raise ValueError(f"piece message with invalid piece index {_stringify(msg)}")
    plen = layout.piece_bytes[msg.index]
    if msg.offset % BLOCK_SIZE != 0 or not 0 <= msg.offset < plen:
        raise ValueError(f"piece message with invalid block offset {_stringify(msg)}")
    if len(msg.block) != min(BLOCK_SIZE, plen - msg.offset):
        raise ValueError(f"piece message with invalid block length {_stringify(msg)}")


class IncrementalVerifierV2(_Incremental):
    """IncrementalVerifier for a v2 torrent (metainfo_v2.V2Layout): the same methods and flush policy; a flush is
    one tv_v2_verify_list launch carrying the pending pieces' rows of the layout (valid bytes, tree width, expected
    root), so the context holds no piece table and no digests.  The slot pool addresses the ALIGNED space (piece p at
    p * piece_length); `storage` is addressed in the unaligned concatenation of the files, as Storage is."""

    def __init__(self, layout: V2Layout, storage=None, device: int = 0,
                 shard: Optional[Tuple[int, int]] = None, flush_pieces=_AUTO, flush_age_ms=_AUTO,
                 on_verified: Optional[Callable[[int, bool], None]] = None, slots: Optional[int] = None):
        if len(layout.hashes) != 32 * layout.n_pieces:
            raise ValueError("the layout has no expected hashes (a creation-mode table)")
        self._init_v2(layout, storage)
        P = layout.n_pieces
        self._init_policy(P, shard, flush_pieces, flush_age_ms, flush_cost_ms_v2(layout.piece_length), on_verified,
                          slots)
        self.ctx = _native.Context(device)
        self.ctx.set_option(_native.TV_OPT_LIST_SLOTS, self.slots)
        self.ctx.set_layout(layout.total_length, layout.piece_length, P, self.first, self.count)

    def _init_v2(self, layout: V2Layout, storage) -> None:
        self.layout = layout
        self.storage = storage
        # start of each file in the unaligned concatenation: a file's length is where its last piece ends
        ends = list(layout.file_first_piece[1:]) + [layout.n_pieces]
        self._file_start, pos = [], 0
        for a, b in zip(layout.file_first_piece, ends):
            self._file_start.append(pos)
            if b > a:
                pos += layout.piece_offset[b - 1] + layout.piece_bytes[b - 1]

    def _validate(self, msg: PieceMsg) -> None:
        validate_received_block_v2(self.layout, msg)

    def _piece_bytes(self, index: int) -> int:
        return self.layout.piece_bytes[index]

    def _storage_offset(self, index: int, offset: int) -> int:
        return self._file_start[self.layout.piece_file[index]] + self.layout.piece_offset[index] + offset

    def _stage(self, index: int, buf) -> None:
        self.ctx.stage(index * self.layout.piece_length, buf)

    def _verify_list(self, pending: List[int]) -> bytes:
        lay = self.layout
        return self.ctx.v2_verify_list(pending, [lay.piece_bytes[i] for i in pending],
                                       [lay.tree_leaves[i] for i in pending],
                                       b"".join(lay.hashes[32 * i:32 * i + 32] for i in pending))


# ---- hybrid torrents (v1 + v2 descriptions of one payload) -----------------------------------------------------------

def flush_cost_ms_hybrid(piece_len: int) -> float:
    """Estimated GPU time of one hybrid list flush: the SHA-1 list launch and the v2 list launch run one after the
    other on one stream, so the two models' sum (the pad launch is not modelled: its cost depends on the tails)."""
    return flush_cost_ms(piece_len) + flush_cost_ms_v2(piece_len)


class IncrementalVerifierHybrid(IncrementalVerifierV2):
    """IncrementalVerifier for a hybrid torrent (hybrid.MetainfoHybrid): the same methods and flush policy; a flush is
    one tv_hybrid_verify_list call, which zeroes the pad range of every pending piece's slot and runs the SHA-1 list
    launch and the v2 list launch over the same bytes.  Blocks are the v2 side's (validate_received_block_v2 against
    meta.layout: a block lies inside the file bytes of its piece; pads are never received) and `storage` is addressed
    as IncrementalVerifierV2 addresses it.  The slot pool is laid over the v1 space (meta.total_length, pads
    included) with the v1 `pieces` string as its digests.  A piece's have-bit is v1 AND v2; `disagree` lists the pieces
    exactly one description accepted, in the order they were found: the host should refuse the torrent for these."""

    def __init__(self, meta, storage=None, device: int = 0,
                 shard: Optional[Tuple[int, int]] = None, flush_pieces=_AUTO, flush_age_ms=_AUTO,
                 on_verified: Optional[Callable[[int, bool], None]] = None, slots: Optional[int] = None):
        layout = meta.layout
        if len(layout.hashes) != 32 * layout.n_pieces:
            raise ValueError("the layout has no expected hashes (a creation-mode table)")
        self.meta = meta
        self.disagree: List[int] = []
        self._init_v2(layout, storage)
        L = layout.piece_length
        self._init_policy(layout.n_pieces, shard, flush_pieces, flush_age_ms, flush_cost_ms_hybrid(L), on_verified,
                          slots)
        self.ctx = _native.Context(device)
        self.ctx.set_option(_native.TV_OPT_LIST_SLOTS, self.slots)
        self.ctx.set_layout(meta.total_length, L, layout.n_pieces, self.first, self.count)
        self.ctx.set_digests(meta.pieces)

    def _verify_list(self, pending: List[int]) -> bytes:
        lay = self.layout
        ok, v1, v2 = self.ctx.hybrid_verify_list(pending, [lay.piece_bytes[i] for i in pending],
                                                 [lay.tree_leaves[i] for i in pending],
                                                 b"".join(lay.hashes[32 * i:32 * i + 32] for i in pending))
        self.disagree += [i for i, a, b in zip(pending, v1, v2) if a != b and i not in self.disagree]
        return ok
