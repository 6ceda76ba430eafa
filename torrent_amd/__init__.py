"""torrent_amd -- MI355X-native piece verification for rclarey/torrent.

The hot path (bulk SHA-1 of every piece against info.pieces -> have-bitfield) runs in
libtorrent_verify.so (hand-written HIP for gfx950, C ABI in include/torrent_verify.h).
This package is the host-side mirror of the reference's piece/storage/metainfo API
(piece.ts, storage.ts, metainfo.ts) plus the new verify module.
"""
from .bencode import bdecode, bdecode_raw, bencode  # noqa: F401
from .metainfo import FileInfo, InfoDict, Metainfo, make_info, parse_metainfo, partition  # noqa: F401
from .piece import BLOCK_SIZE, piece_length, validate_received_block, validate_requested_block  # noqa: F401
from .storage import FsStorage, MemoryStorage, Storage, fs_storage  # noqa: F401
from .verify import (context_counters, hash_files, hash_pieces, hash_stream, release_contexts, shard_ranges,  # noqa: F401
                     verify_files, verify_payload, verify_piece, verify_piece_async, verify_pieces,
                     verify_pieces_async, verify_stream)
from .batch import plan_batches, verify_files_batch, verify_payload_batch  # noqa: F401
from .incremental import (IncrementalVerifier, IncrementalVerifierHybrid, IncrementalVerifierV2,  # noqa: F401
                          flush_cost_ms_v2, validate_received_block_v2)
from .make_torrent import make_torrent  # noqa: F401
from .metainfo_v2 import FileV2, MetainfoV2, V2Layout, parse_metainfo_v2  # noqa: F401
from .v2 import (hash_files_v2, hash_stream_v2, make_torrent_v2, verify_files_v2, verify_payload_v2,  # noqa: F401
                 verify_piece_v2, verify_stream_v2)
from .hybrid import (HybridResult, MetainfoHybrid, hash_files_hybrid, hash_stream_hybrid, make_torrent_hybrid,  # noqa: F401
                     parse_metainfo_hybrid, verify_files_hybrid, verify_payload_hybrid, verify_piece_hybrid,
                     verify_stream_hybrid)
from .merkle_v2 import (BlockRepairVerifierV2, check_blocks_v2, check_proof_v2, leaf_hashes_v2,  # noqa: F401
                        leaf_layers_files_v2, proof_v2)

__all__ = [
    "bdecode", "bencode", "FileInfo", "InfoDict", "Metainfo", "make_info", "parse_metainfo", "partition",
    "BLOCK_SIZE", "piece_length", "validate_received_block", "validate_requested_block",
    "FsStorage", "MemoryStorage", "Storage", "fs_storage",
    "hash_pieces", "shard_ranges", "verify_files", "verify_payload", "verify_piece", "verify_piece_async",
    "verify_pieces", "verify_pieces_async", "verify_stream", "release_contexts", "context_counters", "hash_files",
    "IncrementalVerifier", "make_torrent",
    "bdecode_raw", "FileV2", "MetainfoV2", "V2Layout", "parse_metainfo_v2", "hash_files_v2", "make_torrent_v2",
    "verify_files_v2", "verify_payload_v2", "verify_piece_v2", "verify_stream_v2",
    "IncrementalVerifierV2", "flush_cost_ms_v2", "validate_received_block_v2",
    "BlockRepairVerifierV2", "check_blocks_v2", "check_proof_v2", "leaf_hashes_v2", "leaf_layers_files_v2", "proof_v2",
    "HybridResult", "MetainfoHybrid", "parse_metainfo_hybrid", "verify_payload_hybrid", "verify_files_hybrid",
    "verify_stream_hybrid", "verify_piece_hybrid", "IncrementalVerifierHybrid",
    "hash_files_hybrid", "make_torrent_hybrid", "hash_stream", "hash_stream_v2", "hash_stream_hybrid",
    "plan_batches", "verify_files_batch", "verify_payload_batch",
]
