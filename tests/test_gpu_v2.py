"""BitTorrent v2 on the GPU: tv_v2_set_pieces / tv_v2_verify / tv_v2_hash and the Python host (torrent_amd/v2.py)
against tests/v2_ref.py (hashlib).  Every comparison is bit-exact.  The shapes are the smallest at which the kernels
can still go wrong: leaf tails around the SHA-256 padding edges, every tree width from no interior node to more leaves
than a workgroup, short last pieces, piece counts around the ballot and bitfield-word edges, both lane mappings."""
import hashlib
import os

import numpy as np
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


def table_of(files, L):
    """(piece table, expected piece hashes, aligned file offsets) from the reference."""
    table = v2_ref.piece_table([len(f) for f in files], L)
    hashes = []
    for f in files:
        hashes += v2_ref.file_hashes(f, L)[2]
    offs, p = [], 0
    for f in files:
        offs.append(p * L)
        p += -(-len(f) // L)
    return table, hashes, offs


def load(ctx, files, L, hashes=None, first=0, count=None, staged=None, with_hashes=True):
    """Layout + piece table + the files staged at their aligned offsets (staged: the bytes to stage instead)."""
    table, want, offs = table_of(files, L)
    P = len(table)
    total = (P - 1) * L + table[-1][2]
    ctx.set_layout(total, L, P, first, P - first if count is None else count)
    hs = b"".join(want if hashes is None else hashes) if with_hashes else None
    ctx.v2_set_pieces([r[2] for r in table], [r[3] for r in table], hs)
    for off, data in zip(offs, staged if staged is not None else files):
        if len(data):
            ctx.stage(off, data)
    return table, want, offs


def flipped(data: bytes, pos: int, bit: int = 0x10) -> bytes:
    b = bytearray(data)
    b[pos] ^= bit
    return bytes(b)


# ---- leaf tails -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 55, 56, 63, 64, 65, 16383, 16384, 16385, 32768 + 119])
def test_leaf_tails(ctx, n):
    data = rnd(1000 + n, n)
    table, want, _ = load(ctx, [data], 16 * K)
    assert want[0] == hashlib.sha256(data[:LEAF]).digest()
    assert ctx.v2_verify() == set_bits(len(table))
    assert ctx.v2_hash() == b"".join(want)
    assert ctx.last_kernel()[0] == 8
    # one flipped bit in the last valid byte: exactly the last piece drops
    load(ctx, [data], 16 * K, staged=[flipped(data, n - 1, 0x01)])
    assert ctx.v2_verify() == set_bits(len(table), clear={len(table) - 1})


# ---- tree widths: none, one level, a full wave, across waves, more than a workgroup -----------------------------------

@pytest.mark.parametrize("L,P", [(16 * K, 1), (16 * K, 3), (32 * K, 1), (32 * K, 3), (64 * K, 1), (64 * K, 3),
                                 (1024 * K, 1), (1024 * K, 3), (4096 * K, 1), (4096 * K, 3), (32768 * K, 1)])
def test_tree_widths(ctx, native, L, P):
    data = rnd(7 + P, P * L)
    table, want, _ = load(ctx, [data], L)
    assert [r[3] for r in table] == [L // LEAF] * P
    assert ctx.v2_hash() == b"".join(want)
    assert ctx.last_kernel() == (8, 2 + (L // LEAF).bit_length() - 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-P * (L // LEAF) // 256)
    assert ctx.v2_verify() == set_bits(P)
    # a flipped bit in the last leaf of the last piece reaches the root through every level
    ctx.stage(P * L - 9, flipped(data[P * L - 9:P * L - 8], 0))
    assert ctx.v2_verify() == set_bits(P, clear={P - 1})
    k, total = ctx.last_timing()
    assert 0 < k <= total


# ---- a long file's short last piece keeps the full width ----------------------------------------------------------------

@pytest.mark.parametrize("tail", [LEAF, 2 * LEAF, 3 * LEAF, 7 * LEAF, 7 * LEAF + 1])
def test_short_last_piece(ctx, tail):
    L = 128 * K
    data = rnd(50 + tail, L + tail)
    table, want, _ = load(ctx, [data], L)
    assert table[1] == (0, L, tail, 8)
    assert ctx.v2_hash() == b"".join(want)
    assert ctx.v2_verify() == set_bits(2)


@pytest.mark.parametrize("leaves,width", [(1, 1), (2, 2), (3, 4), (5, 8)])
def test_small_files_have_narrow_trees(ctx, leaves, width):
    L = 128 * K
    files = [rnd(60 + leaves, leaves * LEAF - 3), rnd(61, 2 * L)]   # a small file, then a long one (full width)
    table, want, _ = load(ctx, files, L)
    assert [r[3] for r in table] == [width, 8, 8]
    assert want[0] == v2_ref.piece_root(files[0], width)
    assert ctx.v2_hash() == b"".join(want)
    assert ctx.v2_verify() == set_bits(3)
    # the same bytes with the full width are a different root: the width is part of the table
    if width != 8:
        ctx.v2_set_pieces([r[2] for r in table], [8, 8, 8], b"".join(want))
        assert ctx.v2_verify() == set_bits(3, clear={0})


# ---- piece counts (ballot and bitfield-word edges) under each lane mapping ----------------------------------------------

@pytest.mark.parametrize("mapping", [1, 2])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_piece_counts_and_mappings(ctx, native, P, mapping):
    L = 16 * K
    data = rnd(80 + P, (P - 1) * L + 4321)
    bad = sorted({0, P // 2, P - 1})
    staged = bytearray(data)
    for i in bad:
        staged[i * L + 5] ^= 0x40
    ctx.set_option(native.TV_OPT_V2_MAP, mapping)
    try:
        table, want, _ = load(ctx, [data], L, staged=[bytes(staged)])
        got = ctx.v2_verify()
        ran = ctx.counter(native.TV_COUNTER_V2_MAP)
        roots = ctx.v2_hash()
    finally:
        ctx.set_option(native.TV_OPT_V2_MAP, 0)
    assert ran == (native.V2_MAP_PIECE if mapping == 2 and P >= 64 else native.V2_MAP_LEAF)
    assert got == set_bits(P, clear=set(bad))
    assert [roots[32 * i:32 * i + 32] == want[i] for i in range(P)] == [i not in bad for i in range(P)]


@pytest.mark.parametrize("mapping", [1, 2])
def test_mappings_on_wide_ragged_pieces(ctx, native, mapping):
    """Both mappings where pieces have several leaves and differ in length and width: 70 files of 1 .. 9 leaves under
    L = 128 KiB (piece-major: a wave holds one leaf index of 64 different pieces)."""
    L = 128 * K
    files = [rnd(300 + k, (k % 9) * LEAF + 1 + 37 * k) for k in range(70)]
    ctx.set_option(native.TV_OPT_V2_MAP, mapping)
    try:
        table, want, _ = load(ctx, files, L)
        roots, got = ctx.v2_hash(), ctx.v2_verify()
        assert ctx.counter(native.TV_COUNTER_V2_MAP) == mapping
    finally:
        ctx.set_option(native.TV_OPT_V2_MAP, 0)
    assert roots == b"".join(want)
    assert got == set_bits(len(table))


# ---- multi-file golden layouts through the Python host ----------------------------------------------------------------

def _meta(name):
    from torrent_amd import parse_metainfo_v2
    g = golden()[name]
    return g, parse_metainfo_v2(torrent_v2(golden_files(name), g["piece_length"], name="gold"))


def _write(tmp_path, meta, files):
    for f, data in zip(meta.files, files):
        if data is None:
            continue
        p = tmp_path.joinpath(*f.path)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)


@pytest.mark.parametrize("name", ["multi64k", "small128k", "leaf16k"])
def test_golden_layouts_payload_and_files(name, tmp_path):
    from torrent_amd import verify_files_v2, verify_payload_v2
    g, meta = _meta(name)
    files = list(golden_files(name))
    assert meta.layout.hashes.hex() == "".join(g["piece_hashes"])
    assert bytes(verify_payload_v2(meta, files)).hex() == g["bitfield"]
    m, t, keep = g["missing"]["file"], g["truncated"]["file"], g["truncated"]["keep"]
    gone = files[:m] + [None] + files[m + 1:]
    cut = files[:t] + [files[t][:keep]] + files[t + 1:]
    assert bytes(verify_payload_v2(meta, gone)).hex() == g["missing"]["bitfield"]
    assert bytes(verify_payload_v2(meta, cut)).hex() == g["truncated"]["bitfield"]
    assert g["missing"]["bitfield"] != g["bitfield"] != g["truncated"]["bitfield"]
    for sub, fs, want in (("full", files, g["bitfield"]), ("gone", gone, g["missing"]["bitfield"]),
                          ("cut", cut, g["truncated"]["bitfield"])):
        d = tmp_path / sub
        _write(d, meta, fs)
        assert bytes(verify_files_v2(meta, str(d))).hex() == want, sub
        assert sorted(p.name for p in d.rglob("*") if p.is_file()) == sorted(
            f.path[-1] for f, x in zip(meta.files, fs) if x is not None)    # nothing was created


def test_verify_piece_v2():
    from torrent_amd import verify_piece_v2
    g, meta = _meta("multi64k")
    files = golden_files("multi64k")
    lay = meta.layout
    for i in (0, 3, 4, 5, 7, lay.n_pieces - 1):     # a full piece, a short last piece, the 1-byte file, one-piece files
        f, o, b = lay.piece_file[i], lay.piece_offset[i], lay.piece_bytes[i]
        data = files[f][o:o + b]
        assert verify_piece_v2(meta, i, data) is True
        assert verify_piece_v2(meta, i, flipped(data, b - 1)) is False
        assert verify_piece_v2(meta, i, data + b"x") is False
    with pytest.raises(ValueError):
        verify_piece_v2(meta, lay.n_pieces, b"")


# ---- corruption: exactly the piece that holds the flipped bit drops ----------------------------------------------------

def test_corruptions_and_bytes_past_a_piece(ctx):
    L = 128 * K
    files = [rnd(90, 2 * L + 3 * LEAF + 100), rnd(91, 5), rnd(92, LEAF + 1), rnd(93, L)]
    table, want, offs = load(ctx, files, L)
    P = len(table)
    assert ctx.v2_verify() == set_bits(P)
    # garbage in the bytes past piece_bytes of every short piece (up to the piece's end in the aligned space)
    for i, (f, o, b, w) in enumerate(table):
        if b < L:
            ctx.stage(i * L + b, os.urandom(L - b) if i < P - 1 else os.urandom(0))
    assert ctx.v2_verify() == set_bits(P)
    for piece, pos in ((1, 0),                       # the first byte of a piece
                       (2, 3 * LEAF + 99),           # the last valid byte of a short last leaf
                       (0, 3 * LEAF + 777),          # a middle leaf
                       (3, 4), (4, LEAF), (5, L - 1)):
        f, o, b, w = table[piece]
        lin = piece * L + pos
        assert pos < b
        orig = files[f][o + pos:o + pos + 1]
        ctx.stage(lin, flipped(orig, 0, 0x80))
        assert ctx.v2_verify() == set_bits(P, clear={piece}), (piece, pos)
        ctx.stage(lin, orig)
    assert ctx.v2_verify() == set_bits(P)


# ---- sharding and availability ----------------------------------------------------------------------------------------

def test_availability_and_shards(ctx, native):
    L = 32 * K
    files = [rnd(95, 11 * L + 9), rnd(96, 3), rnd(97, 9 * L)]        # 12 + 1 + 9 = 22 pieces
    staged = [flipped(files[0], 5 * L + 1), files[1], flipped(files[2], 8 * L + 17)]
    table, want, _ = load(ctx, files, L, staged=staged)
    P = 22
    one = ctx.v2_verify()
    assert one == set_bits(P, clear={5, 21})
    avail = bytearray(set_bits(P, clear={0, 12, 21}))
    assert ctx.v2_verify(bytes(avail)) == set_bits(P, clear={0, 5, 12, 21})
    parts = []
    for first, count in ((0, 16), (16, 6)):
        load(ctx, files, L, first=first, count=count, staged=staged)
        parts.append(ctx.v2_verify())
        roots = ctx.v2_hash()
        assert [roots[32 * j:32 * j + 32] == want[first + j] for j in range(count)] == [
            first + j not in (5, 21) for j in range(count)]
    assert parts[0] + parts[1] == one
    from torrent_amd import parse_metainfo_v2, verify_payload_v2
    meta = parse_metainfo_v2(torrent_v2(files, L))
    assert bytes(verify_payload_v2(meta, staged, devices=[0, 0])) == one


# ---- creation mode -----------------------------------------------------------------------------------------------------

def test_hash_equals_the_reference_layer(ctx):
    L = 64 * K
    data = rnd(98, 6 * L + LEAF + 7)
    table, want, _ = load(ctx, [data], L, with_hashes=False)
    root, layer, _ = v2_ref.file_hashes(data, L)
    got = ctx.v2_hash()
    assert got == layer
    from torrent_amd.metainfo_v2 import layer_root
    assert layer_root(got, L) == root


def test_make_torrent_v2_round_trip(tmp_path):
    from torrent_amd import make_torrent_v2, parse_metainfo, parse_metainfo_v2, verify_files_v2
    d = tmp_path / "album"
    (d / "b" / "c").mkdir(parents=True)
    sizes = {"z.bin": 3 * 64 * K + 11, "a.txt": 0, "b/one": 1, "b/c/exact": 64 * K, "b/c/more": 64 * K + 1, "b/two": 40000}
    for rel, n in sizes.items():
        (d / rel).write_bytes(rnd(len(rel) + n, n))
    raw = make_torrent_v2(str(d), "http://example.com/announce", piece_length=64 * K, creation_date=1)
    meta = parse_metainfo_v2(raw)
    assert meta is not None and parse_metainfo(raw) is None and meta.name == "album"
    assert ["/".join(f.path) for f in meta.files] == ["a.txt", "b/c/exact", "b/c/more", "b/one", "b/two", "z.bin"]
    for f in meta.files:
        want = v2_ref.file_hashes((d / "/".join(f.path)).read_bytes(), 64 * K)
        assert f.pieces_root == want[0]
        if want[1]:
            assert meta.piece_layers[want[0]] == want[1]
    assert bytes(verify_files_v2(meta, str(d))) == set_bits(meta.n_pieces)
    one = tmp_path / "single.bin"
    one.write_bytes(rnd(5, 5 * LEAF + 1))
    m1 = parse_metainfo_v2(make_torrent_v2(str(one), "http://example.com/announce", piece_length=32 * K))
    assert m1.files[0].pieces_root == v2_ref.file_hashes(one.read_bytes(), 32 * K)[0]
    assert bytes(verify_files_v2(m1, str(tmp_path))) == set_bits(3)
    (tmp_path / "single.bin").write_bytes(flipped(one.read_bytes(), 32 * K))
    assert bytes(verify_files_v2(m1, str(tmp_path))) == set_bits(3, clear={1})


# ---- hybrid: the v1 and the v2 description of one payload agree ---------------------------------------------------------

def test_hybrid_v1_and_v2_agree():
    from torrent_amd import parse_metainfo, parse_metainfo_v2, verify_payload, verify_payload_v2
    L = 64 * K
    data = rnd(99, 9 * L)                      # whole pieces: the aligned space is the v1 linear space, pads zero
    pieces = b"".join(hashlib.sha1(data[i:i + L]).digest() for i in range(0, len(data), L))
    raw = torrent_v2([data], L, name="h.bin", paths=[["h.bin"]], hybrid_pieces=pieces)
    m1, m2 = parse_metainfo(raw), parse_metainfo_v2(raw)
    for bad in ((), (0,), (4, 8), (2, 3, 7)):
        b = bytearray(data)
        for i in bad:
            b[i * L + 1000 * i + 3] ^= 0x02
        want = set_bits(9, clear=set(bad))
        assert v2_ref.expected_bitfield([bytes(b)], L, v2_ref.file_hashes(data, L)[2]) == want
        assert bytes(verify_payload(m1.info, bytes(b))) == want
        assert bytes(verify_payload_v2(m2, [bytes(b)])) == want


# ---- errors -----------------------------------------------------------------------------------------------------------

def _raises(native, code, fn, *a):
    with pytest.raises(native.NativeError) as ei:
        fn(*a)
    assert ei.value.code == code, str(ei.value)


def test_argument_and_state_errors(native, oracle):
    ARG, STATE = native.TV_ERR_ARG, native.TV_ERR_STATE
    with native.Context(0) as c:
        _raises(native, STATE, c.v2_set_pieces, [1], [1], bytes(32))          # before tv_set_layout
        _raises(native, STATE, c.v2_verify)
        _raises(native, STATE, c.v2_hash)
        for L in (3 * LEAF, 8192, 16383):                                      # not a power of two / below 16 KiB
            c.set_layout(L, L, 1)
            _raises(native, ARG, c.v2_set_pieces, [1], [1], bytes(32))
        L = 64 * K
        c.set_layout(2 * L, L, 2)
        _raises(native, STATE, c.v2_verify)                                    # no piece table
        _raises(native, STATE, c.v2_hash)
        _raises(native, ARG, c.v2_set_pieces, [L], [4], bytes(32))             # n != n_pieces
        for pb, tl in (([0, L], [4, 4]), ([L + 1, L], [4, 4]),                 # piece_bytes 0 / above L
                       ([L, L], [3, 4]), ([L, L], [4, 0]),                     # not a power of two
                       ([L, LEAF + 1], [4, 1]),                                # below ceil(bytes / 16 KiB)
                       ([L, L], [4, 8])):                                      # above L / 16 KiB
            _raises(native, ARG, c.v2_set_pieces, pb, tl, bytes(64))
            _raises(native, STATE, c.v2_verify)                                # a refused table is no table
        c.v2_set_pieces([L, L], [4, 4], None)                                  # creation mode
        _raises(native, STATE, c.v2_verify)                                    # needs hashes
        assert len(c.v2_hash()) == 64
        c.v2_set_pieces([L, L], [4, 4], bytes(64))
        assert c.v2_verify() == b"\x00"
        c.set_layout(2 * L, L, 2)                                              # tv_set_layout drops the table
        _raises(native, STATE, c.v2_verify)
        # a stream is active
        c.set_digests(bytes(40))
        c.v2_set_pieces([L, L], [4, 4], bytes(64))
        c.stream_begin()
        _raises(native, STATE, c.v2_set_pieces, [L, L], [4, 4], bytes(64))
        _raises(native, STATE, c.v2_verify)
        _raises(native, STATE, c.v2_hash)
        c.stream_abort()
        assert c.v2_verify() == b"\x00"                                        # the table outlives the stream
        # windowed layout, slot pool, no resident payload
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 4 * (L + 256) + 256)
        c.set_layout(16 * L, L, 16)
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) > 0
        _raises(native, STATE, c.v2_set_pieces, [L] * 16, [4] * 16, bytes(32 * 16))
        _raises(native, STATE, c.v2_verify)
        _raises(native, STATE, c.v2_hash)
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
        c.set_option(native.TV_OPT_LIST_SLOTS, 4)
        c.set_layout(16 * L, L, 16)
        _raises(native, STATE, c.v2_set_pieces, [L] * 16, [4] * 16, bytes(32 * 16))
        _raises(native, STATE, c.v2_verify)
        c.set_option(native.TV_OPT_LIST_SLOTS, 0)
        c.set_option(native.TV_OPT_RESIDENT, 0)
        c.set_layout(16 * L, L, 16)
        _raises(native, STATE, c.v2_set_pieces, [L] * 16, [4] * 16, bytes(32 * 16))
        c.set_option(native.TV_OPT_RESIDENT, 1)
        # after v2 calls the same context still verifies v1 torrents
        P, total = 16, 16 * L - 777
        payload = oracle.synth_fill(13, 0, total)
        c.set_layout(total, L, P)
        c.v2_set_pieces([L] * 15 + [L - 777], [4] * 16, None)
        c.stage(0, payload)
        roots = c.v2_hash()
        assert roots == v2_ref.file_hashes(bytes(payload), L)[1]
        pieces = oracle.hash_pieces(payload, total, L, P)
        payload[3 * L + 1] ^= 1
        c.set_digests(pieces)
        c.stage(0, payload)
        assert c.verify() == oracle.verify_linear(payload, total, L, pieces)
        assert c.last_kernel()[0] != 8
        dev = c.counter(native.TV_COUNTER_DEVICE_BYTES)
        assert dev >= c.counter(native.TV_COUNTER_PAYLOAD_BYTES) + 16 * 18 * 4 + 8 * 16 * 6 * 4


def test_v2_memory_is_reused_and_counted(native):
    L = 64 * K
    with native.Context(0) as c:
        c.set_layout(8 * L, L, 8)
        before = c.counter(native.TV_COUNTER_DEVICE_BYTES)
        c.v2_set_pieces([L] * 8, [4] * 8, None)
        allocs = c.counter(native.TV_COUNTER_DEVICE_ALLOCS)
        assert c.counter(native.TV_COUNTER_DEVICE_BYTES) == before + 8 * 18 * 4 + 8 * 8 * (4 + 2) * 4
        for _ in range(3):          # the same geometry again: nothing is allocated
            c.set_layout(8 * L, L, 8)
            c.v2_set_pieces([L] * 8, [4] * 8, None)
            c.v2_hash()
        assert c.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs
        c.set_layout(1000, 1000, 1)   # a v1 layout holds no v2 memory
        assert c.counter(native.TV_COUNTER_DEVICE_BYTES) <= before


def test_over_budget_raises_a_clear_error():
    from torrent_amd import parse_metainfo_v2, release_contexts, verify_payload_v2
    L = 64 * K
    data = rnd(3, 16 * L)
    meta = parse_metainfo_v2(torrent_v2([data], L))
    with pytest.raises(MemoryError, match="resident"):
        verify_payload_v2(meta, [data], budget=4 * (L + 256) + 256)
    assert bytes(verify_payload_v2(meta, [data])) == set_bits(16)
    release_contexts()


# ---- bulk: the synthetic payload, 1 % of the pieces corrupted, under both mappings ----------------------------------------

@pytest.fixture(scope="module")
def bulk():
    L, P, seed = 1024 * K, 256, 77
    data = synth.fill(seed, 0, P * L)
    return L, P, seed, v2_ref.file_hashes(data, L)[2]


@pytest.mark.parametrize("mapping", [0, 1, 2])
def test_bulk_synthetic(ctx, native, bulk, mapping):
    L, P, seed, want = bulk
    bad = {3, 100, 255}
    ctx.set_option(native.TV_OPT_V2_MAP, mapping)
    try:
        ctx.set_layout(P * L, L, P)
        ctx.v2_set_pieces([L] * P, [L // LEAF] * P, b"".join(want))
        ctx.fill_synthetic(seed)
        assert ctx.v2_verify() == set_bits(P)
        for i in bad:
            one = bytearray(1)
            ctx.read(i * L + 12345 * (i % 7), one)
            one[0] ^= 0x08
            ctx.stage(i * L + 12345 * (i % 7), bytes(one))
        assert ctx.v2_verify() == set_bits(P, clear=bad)
        assert ctx.counter(native.TV_COUNTER_V2_MAP) in ((1, 2) if mapping == 0 else (mapping,))
    finally:
        ctx.set_option(native.TV_OPT_V2_MAP, 0)
