"""Shared by the hybrid list tests (tests/test_gpu_hybrid_list.py, tests/test_gpu_hybrid_list_fuzz.py): a slot pool (or a
resident shard) over a tests/hybrid_util.py Layout, pieces staged one by one over a 0xFF fill of their whole row -- so
stale bytes sit in every pad range --, and tv_hybrid_verify_list's entries built from the layout.  The expected values
are hybrid_util.Layout.verdicts (hashlib and tests/v2_ref.py)."""
from __future__ import annotations


def piece_data(lay, i: int, staged=None) -> bytes:
    """The file bytes of piece i (of `staged`, one buffer per file; default the layout's files)."""
    f, o, b, _ = lay.table[i]
    return bytes((lay.files if staged is None else staged)[f][o:o + b])


def set_pool(ctx, native, lay, slots: int, first: int = 0, count=None, pieces=None) -> None:
    """A layout over the v1 space with `slots` slots (0: the shard resident) and the v1 digests."""
    count = lay.P - first if count is None else count
    ctx.set_option(native.TV_OPT_LIST_SLOTS, slots)
    try:
        ctx.set_layout(lay.total, lay.L, lay.P, first, count)
    finally:
        ctx.set_option(native.TV_OPT_LIST_SLOTS, 0)         # (read at tv_set_layout only)
    ctx.set_digests(lay.pieces if pieces is None else pieces)


def stage_pieces(ctx, lay, order, staged=None, fill=0xFF) -> None:
    """Every piece of `order`, in that order (so slot != piece): its whole v1 row as `fill`, then its file bytes."""
    for i in order:
        if fill is not None:
            ctx.stage(i * lay.L, bytes([fill]) * lay.v1_len[i])
        ctx.stage(i * lay.L, piece_data(lay, i, staged))


def run_list(ctx, lay, listed, hashes=None, release=True, leaves=None) -> tuple:
    """tv_hybrid_verify_list over the pieces `listed` -> three lists of booleans (ok, v1, v2)."""
    hashes = lay.hashes if hashes is None else hashes
    leaves = lay.tl if leaves is None else leaves
    ok, v1, v2 = ctx.hybrid_verify_list(listed, [lay.pb[i] for i in listed], [leaves[i] for i in listed],
                                        b"".join(hashes[i] for i in listed), release=release)
    assert len(ok) == len(v1) == len(v2) == len(listed)
    assert all(x in (0, 1) for x in ok + v1 + v2)
    return [bool(x) for x in ok], [bool(x) for x in v1], [bool(x) for x in v2]


def read_row(ctx, lay, i: int) -> bytes:
    """The v1 bytes of piece i's row or slot, read back from the device."""
    out = bytearray(lay.v1_len[i])
    ctx.read(i * lay.L, out)
    return bytes(out)
