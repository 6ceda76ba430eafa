"""tv_v2_verify_list (one launch, each piece's merkle tree inside a workgroup) and IncrementalVerifierV2 on the GPU,
bit-exact against tests/v2_ref.py (hashlib).  The shapes are the smallest at which the kernel takes another path:
every tree width from one leaf (256 entries per workgroup) to two tiles of 256 leaves, list lengths around a
workgroup's entries, leaf tails around the SHA-256 padding edges mixed in one wave, ragged widths, stale slot bytes."""
import random

import pytest

from tests import synth, v2_ref
from tests.v2_util import golden, golden_files, set_bits, torrent_v2

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def flipped(data: bytes, pos: int, bit: int = 0x10) -> bytes:
    b = bytearray(data)
    b[pos] ^= bit
    return bytes(b)


def narrowest(b: int) -> int:
    return v2_ref.next_pow2(-(-b // LEAF))


def _raises(native, code, fn, *a):
    with pytest.raises(native.NativeError) as ei:
        fn(*a)
    assert ei.value.code == code, str(ei.value)


# ---- widths and group boundaries ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [16 * K, 32 * K, 64 * K, 256 * K, 4096 * K, 8192 * K])
def test_widths_and_group_boundaries(ctx, native, L):
    W = L // LEAF
    G = max(1, 256 // W)                                   # entries per workgroup
    P = max(3, G + 1)
    last = L - 5                                           # the last piece is short, in its full-width tree
    data = rnd(L // K + 1, (P - 1) * L + last)
    nbytes = [L] * (P - 1) + [last]
    want = [v2_ref.piece_root(data[i * L:i * L + nbytes[i]], W) for i in range(P)]
    staged = bytearray(data)
    staged[0] ^= 0x01                                      # piece 0: its first byte
    staged[len(data) - 1] ^= 0x80                          # piece P - 1: its last valid byte
    good = [v2_ref.piece_root(bytes(staged[i * L:i * L + nbytes[i]]), W) == want[i] for i in range(P)]
    assert good == [False] + [True] * (P - 2) + [False]
    ctx.set_layout(len(data), L, P)
    ctx.stage(0, bytes(staged))
    lists = [[1], [0], [0, 1, P - 1]] + ([list(range(P))] if G > 1 else [])
    for pieces in lists:
        ok = ctx.v2_verify_list(pieces, [nbytes[i] for i in pieces], [W] * len(pieces),
                                b"".join(want[i] for i in pieces))
        assert list(ok) == [int(good[i]) for i in pieces], (L, pieces[:4])
        assert ctx.last_kernel() == (native.KERNEL_V2_LIST, 1)
        assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-len(pieces) // G)
        k, total = ctx.last_timing()
        assert 0 < k <= total


def test_widest_tree_reduces_256_tile_roots(native):
    """L = 1 GiB (W = 65,536: 256 tiles, the most the call takes).  The tile roots are reduced by lanes of two waves,
    which no smaller piece length reaches.  Only the first 300 leaves hold bytes (the other tiles are zero hashes and
    read nothing), so the piece is staged and referenced in milliseconds; a slot pool of one slot holds it."""
    L = 1 << 30
    data = rnd(77, 300 * LEAF + 5)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(2 * L, L, 2)
        for w in (65536, 512):                             # the root after the last level / after the first tile-root level
            root = v2_ref.piece_root(data, w)
            c.stage(L, data)
            assert list(c.v2_verify_list([1], [len(data)], [w], root)) == [1], w
            assert c.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 1
            c.stage(L, flipped(data, len(data) - 1))
            assert list(c.v2_verify_list([1], [len(data)], [w], root)) == [0], w


# ---- leaf tails mixed in one wave ----------------------------------------------------------------------------------------

def test_leaf_tails_in_one_wave(ctx):
    L = 64 * K
    sizes = [1, 55, 56, 63, 64, 65, 16383, 16384, 16385, 32768, 65535, 65536]
    entries = [(b, w) for b in sizes for w in sorted({narrowest(b), 4})]      # 22 entries: G = 64, one workgroup
    assert len(entries) == 22 and (1, 1) in entries and (1, 4) in entries
    P = len(entries)
    datas = [rnd(500 + i, b) for i, (b, w) in enumerate(entries)]
    want = [v2_ref.piece_root(d, w) for d, (b, w) in zip(datas, entries)]
    bad = {4: 0, 15: entries[15][0] - 1}                  # entry -> the byte flipped (a first byte, a last valid byte)
    ctx.set_layout(P * L, L, P)
    ctx.stage(0, rnd(9, P * L))                            # the rows hold other bytes past every piece's own
    for i, d in enumerate(datas):
        ctx.stage(i * L, flipped(d, bad[i]) if i in bad else d)
    ok = ctx.v2_verify_list(list(range(P)), [b for b, w in entries], [w for b, w in entries], b"".join(want))
    assert list(ok) == [int(i not in bad) for i in range(P)]
    # the same bytes under the other width are another root: the width is part of the entry
    other = [4 if w != 4 else narrowest(b) for b, w in entries]
    ok = ctx.v2_verify_list(list(range(P)), [b for b, w in entries], other, b"".join(want))
    assert list(ok) == [int(o == w and i not in bad) for i, ((b, w), o) in enumerate(zip(entries, other))]


# ---- ragged widths across workgroups ---------------------------------------------------------------------------------------

def test_ragged_widths_across_workgroups(ctx, native):
    L = 64 * K
    P = 70                                                 # G = 64: two workgroups, the second partial
    widths = [(1, 2, 4)[i % 3] for i in range(P)]
    nbytes = [(w // 2) * LEAF + 1 + (997 * i) % (LEAF * (w - w // 2)) for i, w in enumerate(widths)]
    assert all(narrowest(b) == w for b, w in zip(nbytes, widths))
    datas = [rnd(700 + i, b) for i, b in enumerate(nbytes)]
    want = [v2_ref.piece_root(d, w) for d, w in zip(datas, widths)]
    bad = {5, 64, 69}
    ctx.set_layout(P * L, L, P)
    ctx.stage(0, rnd(10, P * L))
    for i, d in enumerate(datas):
        ctx.stage(i * L, flipped(d, len(d) // 2) if i in bad else d)
    order = list(range(P)) + [5, 6, 64, 0, 69, 33]         # some listed twice
    random.Random(7).shuffle(order)
    ok = ctx.v2_verify_list(order, [nbytes[i] for i in order], [widths[i] for i in order],
                            b"".join(want[i] for i in order))
    assert list(ok) == [int(i not in bad) for i in order]
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 2


# ---- slot pools ----------------------------------------------------------------------------------------------------------

def test_stale_slot_bytes_are_never_hashed(native):
    L = 64 * K
    full, small = rnd(20, L), rnd(21, 100)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(3 * L, L, 3)
        c.stage(0, full)
        assert list(c.v2_verify_list([0], [L], [4], v2_ref.piece_root(full, 4))) == [1]
        root = v2_ref.piece_root(small, 1)
        c.stage(2 * L, small)                              # the same slot: bytes 100 .. L - 1 are piece 0's
        assert list(c.v2_verify_list([2], [100], [1], root)) == [1]
        c.stage(2 * L, flipped(small, 99))
        assert list(c.v2_verify_list([2], [100], [1], root)) == [0]
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0


def test_slot_pool_semantics(native):
    L, P = 32 * K, 40
    nbytes = [L] * (P - 1) + [333]                         # a short last piece
    datas = [rnd(40 + i, b) for i, b in enumerate(nbytes)]
    want = [v2_ref.piece_root(d, 2) for d in datas]
    want[7] = flipped(want[7], 0)                          # piece 7 fails
    stride = L + 256

    def lst(c, pieces):
        return list(c.v2_verify_list(pieces, [nbytes[i] for i in pieces], [2] * len(pieces),
                                     b"".join(want[i] for i in pieces)))

    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 4)
        c.set_layout((P - 1) * L + 333, L, P)
        assert c.counter(native.TV_COUNTER_PAYLOAD_BYTES) == 4 * stride + 256
        for i in (39, 7, 3, 12):
            c.stage(i * L, datas[i])
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 4
        _raises(native, native.TV_ERR_STATE, c.stage, 5 * L, datas[5])         # the fifth piece: no slot
        _raises(native, native.TV_ERR_STATE, c.v2_set_pieces, nbytes, [2] * P, b"".join(want))   # as before
        extra0 = c.counter(native.TV_COUNTER_DEVICE_BYTES) - c.counter(native.TV_COUNTER_PAYLOAD_BYTES)
        assert lst(c, [3, 39, 7, 12, 3, 20]) == [1, 1, 0, 1, 1, 0]             # duplicates; 20 was never staged
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
        assert lst(c, [3]) == [0]                                              # its slot was freed
        assert c.last_kernel() == (native.KERNEL_V2_LIST, 0)                   # nothing to launch
        order = list(range(P))
        random.Random(3).shuffle(order)
        for k in range(0, P, 4):                                               # every piece, four at a time
            batch = order[k:k + 4]
            for i in batch:
                c.stage(i * L, datas[i])
            assert lst(c, batch) == [int(i != 7) for i in batch]
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
        # no node buffers: the lists' own memory is at most 64 B per entry of the longest list (at least 1,024)
        extra = c.counter(native.TV_COUNTER_DEVICE_BYTES) - c.counter(native.TV_COUNTER_PAYLOAD_BYTES)
        assert 0 < extra - extra0 <= 64 * max(6, 1024)
        _raises(native, native.TV_ERR_STATE, c.v2_set_pieces, nbytes, [2] * P, b"".join(want))
        _raises(native, native.TV_ERR_STATE, c.v2_verify)


# ---- a resident shard: the list call and the table call agree --------------------------------------------------------------

def test_resident_list_agrees_with_v2_verify(ctx, native, tmp_path):
    from torrent_amd import parse_metainfo_v2
    g = golden()["multi64k"]
    files = list(golden_files("multi64k"))
    L = g["piece_length"]
    meta = parse_metainfo_v2(torrent_v2(files, L, name="gold"))
    lay = meta.layout
    P = lay.n_pieces
    t, keep = g["truncated"]["file"], g["truncated"]["keep"]
    cut = files[:t] + [files[t][:keep]] + files[t + 1:]
    paths = []
    for k, data in enumerate(cut):
        p = tmp_path / f"f{k}.bin"
        p.write_bytes(data)
        paths.append(str(p))
    ctx.set_layout(lay.total_length, L, P)
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, lay.hashes)
    seg = [k for k, f in enumerate(files) if len(f)]
    st = ctx.stage_files([paths[k] for k in seg], [0] * len(seg), [lay.file_offset[k] for k in seg],
                         [len(files[k]) for k in seg])
    assert [s != native.TV_OK for s in st] == [k == t for k in seg]
    bits = ctx.v2_verify()
    expected = [bytes.fromhex(h) for h in g["piece_hashes"]]
    assert bits == v2_ref.expected_bitfield(cut, L, expected, have=[len(f) for f in files])
    assert bits.hex() == g["truncated"]["bitfield"] != g["bitfield"]
    order = list(range(P))
    random.Random(11).shuffle(order)
    ok = ctx.v2_verify_list(order, [lay.piece_bytes[i] for i in order], [lay.tree_leaves[i] for i in order],
                            b"".join(lay.hashes[32 * i:32 * i + 32] for i in order))
    got = bytearray(len(bits))
    for i, r in zip(order, ok):
        if r:
            got[i >> 3] |= 0x80 >> (i & 7)
    assert bytes(got) == bits
    lost = [i for i in range(P) if lay.piece_file[i] == t and lay.piece_offset[i] + lay.piece_bytes[i] > keep]
    assert lost and all(ok[order.index(i)] == 0 for i in lost)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors(native):
    ARG, STATE = native.TV_ERR_ARG, native.TV_ERR_STATE
    L = 64 * K
    h = bytes(32)
    lib = native.lib()
    with native.Context(0) as c:
        _raises(native, STATE, c.v2_verify_list, [0], [L], [4], h)              # before tv_set_layout
        for bad_L in (3 * LEAF, 8192, 16383):                                   # not a power of two / below 16 KiB
            c.set_layout(2 * bad_L, bad_L, 2)
            _raises(native, ARG, c.v2_verify_list, [0], [1], [1], h)
            assert c.v2_verify_list([], [], [], b"") == b""
        c.set_layout(24 * L, L, 24, 8, 3)                                       # the shard: pieces 8, 9, 10
        assert c.v2_verify_list([], [], [], b"") == b""                         # n == 0
        import ctypes
        import numpy as np
        pc, pb, tl = np.array([8], np.uint64), np.array([L], np.uint32), np.array([4], np.uint32)
        out = ctypes.create_string_buffer(1)
        args = [pc.ctypes.data, pb.ctypes.data, tl.ctypes.data, h, out]
        assert lib.tv_v2_verify_list(c._h, 1, *args) == native.TV_OK
        for k in range(5):                                                      # each pointer NULL with n > 0
            assert lib.tv_v2_verify_list(c._h, 1, *[None if q == k else a for q, a in enumerate(args)]) == ARG
        for piece in (0, 7, 11, 24, 1 << 40):                                        # outside the shard
            _raises(native, ARG, c.v2_verify_list, [8, piece], [L, L], [4, 4], h * 2)
        for b, w in ((0, 4), (L + 1, 4), (L, 3), (L, 0), (LEAF + 1, 1), (L, 8)):
            _raises(native, ARG, c.v2_verify_list, [8, 9], [L, b], [4, w], h * 2)
        # a stream is active
        c.set_layout(2 * L, L, 2)
        c.set_digests(bytes(40))
        c.stream_begin()
        _raises(native, STATE, c.v2_verify_list, [0], [L], [4], h)
        c.stream_abort()
        assert list(c.v2_verify_list([0], [L], [4], h)) == [0]
        # a windowed layout; no resident payload
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 4 * (L + 256) + 256)
        c.set_layout(16 * L, L, 16)
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) > 0
        _raises(native, STATE, c.v2_verify_list, [0], [L], [4], h)
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
        c.set_option(native.TV_OPT_RESIDENT, 0)
        c.set_layout(16 * L, L, 16)
        _raises(native, STATE, c.v2_verify_list, [0], [L], [4], h)
        c.set_option(native.TV_OPT_RESIDENT, 1)
        # a refused call frees no slot
        c.set_option(native.TV_OPT_LIST_SLOTS, 2)
        c.set_layout(16 * L, L, 16)
        c.stage(5 * L, rnd(1, L))
        c.stage(9 * L, rnd(2, L))
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 2
        _raises(native, ARG, c.v2_verify_list, [5, 9, 16], [L] * 3, [4] * 3, h * 3)
        _raises(native, ARG, c.v2_verify_list, [5, 9], [L, L], [4, 2], h * 2)
        assert lib.tv_v2_verify_list(c._h, 1, None, pb.ctypes.data, tl.ctypes.data, h, out) == ARG
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 2
        assert list(c.v2_verify_list([5, 9], [L, L], [4, 4],
                                     v2_ref.piece_root(rnd(1, L), 4) + v2_ref.piece_root(rnd(2, L), 4))) == [1, 1]
        assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0
        # a tree wider than 65,536 leaves (a 2 GiB piece)
        c.set_option(native.TV_OPT_LIST_SLOTS, 1)
        c.set_layout(2 << 30, 2 << 30, 1)
        _raises(native, ARG, c.v2_verify_list, [0], [LEAF], [1], h)


# ---- reporting and memory ------------------------------------------------------------------------------------------------

def test_reporting_and_no_reallocation(native):
    L, P = 32 * K, 12
    datas = [rnd(60 + i, L) for i in range(P)]
    want = b"".join(v2_ref.piece_root(d, 2) for d in datas)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, P)
        c.set_layout(P * L, L, P)
        allocs = None
        for rep in range(4):
            n = P if rep != 2 else 5                       # the same n, then a smaller one
            for i in range(n):
                c.stage(i * L, datas[i])
            assert list(c.v2_verify_list(list(range(n)), [L] * n, [2] * n, want[:32 * n])) == [1] * n
            assert c.last_kernel() == (native.KERNEL_V2_LIST, 1)
            assert c.counter(native.TV_COUNTER_LAST_WORKGROUPS) == 1
            if rep == 0:
                allocs = c.counter(native.TV_COUNTER_DEVICE_ALLOCS)
        assert c.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs


# ---- IncrementalVerifierV2 ---------------------------------------------------------------------------------------------------

def _have(bitfield, i):
    return bool(bitfield[i >> 3] & (0x80 >> (i & 7)))


def test_incremental_verifier_v2_on_a_multi_file_layout():
    from torrent_amd import (FileInfo, IncrementalVerifierV2, MemoryStorage, Storage, make_info,
                             parse_metainfo_v2)
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    g = golden()["multi64k"]
    files = golden_files("multi64k")
    L = g["piece_length"]
    meta = parse_metainfo_v2(torrent_v2(files, L, name="gold"))
    lay = meta.layout
    P = lay.n_pieces
    rng = random.Random(12)
    bad = set(rng.sample(range(P), 2))
    msgs = []
    for i in range(P):
        f, o, b = lay.piece_file[i], lay.piece_offset[i], lay.piece_bytes[i]
        d = bytearray(files[f][o:o + b])
        if i in bad:
            d[rng.randrange(b)] ^= 0x04
        msgs += [PieceMsg(i, q, bytes(d[q:q + BLOCK_SIZE])) for q in range(0, b, BLOCK_SIZE)]
    rng.shuffle(msgs)
    msgs += rng.sample(msgs, 20)                           # re-sends
    # the reference's Storage over the unaligned concatenation of the files (a v1-style file table of the same files)
    info = make_info(L, bytes(20), "gold", files=[FileInfo(len(d), ["f%d" % k]) for k, d in enumerate(files)])
    mem = MemoryStorage()
    seen = {}
    v = IncrementalVerifierV2(lay, storage=Storage(mem, info, "dl"), flush_pieces=None, flush_age_ms=None, slots=3,
                              on_verified=lambda i, ok: seen.setdefault(i, []).append(ok))
    try:
        assert v.device_payload_bytes() == 3 * (L + 256) + 256
        for m in msgs:
            v.on_block(m)
        for i, ok in v.flush():
            seen.setdefault(i, []).append(ok)
        assert v.forced_flushes >= 1
        assert v.device_payload_bytes() == 3 * (L + 256) + 256
        for i in range(P):
            assert seen[i][0] == (i not in bad), i
        # a failed piece is forgotten and may arrive again: re-sent blocks can complete it a second time
        assert all(not any(r) for i, r in seen.items() if i in bad)
        expected = [bytes.fromhex(h) for h in g["piece_hashes"]]
        assert bytes(v.bitfield) == set_bits(P, clear=bad)
        assert bytes(v.bitfield) == bytes(a & b for a, b in zip(
            v2_ref.expected_bitfield(files, L, expected), set_bits(P, clear=bad)))
        with pytest.raises(ValueError):
            v.on_block(PieceMsg(P, 0, bytes(BLOCK_SIZE)))
    finally:
        v.close()
    # storage.set got every block at its offset in the unaligned concatenation: good pieces read back as the files
    for k, d in enumerate(files):
        got = bytes(mem.files.get(("dl", "f%d" % k), b""))
        for i in range(P):
            if lay.piece_file[i] == k and i not in bad:
                o, b = lay.piece_offset[i], lay.piece_bytes[i]
                assert got[o:o + b] == d[o:o + b], (k, i)


def test_incremental_verifier_v2_on_cfg4_geometry_holds_k_slots():
    """One 200 GiB file of 51,200 x 4 MiB pieces, K = 8 slots: blocks of 24 scattered pieces arrive interleaved in
    random order (with re-sends), two pieces corrupted; the device payload stays K x stride, forced flushes make room,
    every result equals hashlib's and the have-bits follow (as the v1 test of this geometry)."""
    from torrent_amd import IncrementalVerifierV2
    from torrent_amd.metainfo_v2 import make_layout
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    L, P = 4 << 20, 51200
    rng = random.Random(4)
    chosen = sorted(rng.sample(range(P), 23) + [P - 1])
    datas = {i: bytes(synth.fill(4, i * L, L)) for i in chosen}
    layer = bytearray(rng.randbytes(32 * P))
    for i in chosen:
        layer[32 * i:32 * i + 32] = v2_ref.piece_root(datas[i], L // LEAF)
    root = bytes(32)                                       # (make_layout only looks the layer up by it)
    lay = make_layout([L * P], L, [root], {root: bytes(layer)})
    assert lay.n_pieces == P and lay.tree_leaves[0] == 256
    bad = set(rng.sample(chosen, 2))
    msgs = []
    for i in chosen:
        d = bytearray(datas[i])
        if i in bad:
            d[rng.randrange(L)] ^= 0x20
        msgs += [PieceMsg(i, o, bytes(d[o:o + BLOCK_SIZE])) for o in range(0, L, BLOCK_SIZE)]
    rng.shuffle(msgs)
    msgs += rng.sample(msgs, 50)
    seen = {}
    v = IncrementalVerifierV2(lay, flush_pieces=None, flush_age_ms=None, slots=8,
                              on_verified=lambda i, ok: seen.setdefault(i, []).append(ok))
    try:
        assert v.device_payload_bytes() == 8 * (L + 256) + 256
        for m in msgs:
            v.on_block(m)
        for i, ok in v.flush():
            seen.setdefault(i, []).append(ok)
        assert v.forced_flushes >= 2
        assert v.device_payload_bytes() == 8 * (L + 256) + 256
        for i in chosen:
            assert seen[i][0] == (i not in bad), i
            assert _have(v.bitfield, i) == (i not in bad)
        assert sum(bin(b).count("1") for b in v.bitfield) == len(chosen) - len(bad)
    finally:
        v.close()
