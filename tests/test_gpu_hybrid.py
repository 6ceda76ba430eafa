"""Hybrid torrents on the GPU: tv_hybrid_verify / tv_hybrid_hash and the Python host (torrent_amd/hybrid.py) against
hashlib SHA-1 over the padded linear bytes and tests/v2_ref.py.  Every comparison is bit-exact.  The file lengths put a
tail (the pad range of a row) at every alignment class and row position: 1, 15, 16, 17 bytes, around a 16 KiB leaf,
around the piece length, whole pieces (no tail), a zero-length file in between.  Before the files the whole shard is
staged as 0xFF, so a pad range the kernel does not zero cannot pass by luck."""
import functools
import os

import pytest

from tests import hybrid_util as hu
from tests import synth, v2_ref
from tests.v2_util import set_bits

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


class Shape:
    """The files of one piece length, their tables and both oracles' expected values (computed once)."""

    def __init__(self, L: int, trailing: bool):
        self.L, self.trailing = L, trailing
        self.lengths = [1, 15, 16, 17, LEAF - 1, LEAF, 0, LEAF + 1, L - 1, L, L + 1, 2 * L, 2 * L + 5]
        self.files = [bytes(synth.fill(300 + k, 0, n)) for k, n in enumerate(self.lengths)]
        self.table = v2_ref.piece_table(self.lengths, L)            # (file, offset, bytes, leaves) per piece
        self.P = len(self.table)
        self.pb = [r[2] for r in self.table]
        self.tl = [r[3] for r in self.table]
        self.offs, p = [], 0
        for n in self.lengths:
            self.offs.append(p * L)
            p += -(-n // L)
        self.total = self.P * L if trailing else (self.P - 1) * L + self.pb[-1]
        self.pieces = hu.v1_pieces(self.files, L, trailing)
        self.hashes = hu.v2_expected(self.files, L)
        self.v1_len = [min(L, self.total - i * L) for i in range(self.P)]
        self.tails = [i for i in range(self.P) if self.pb[i] < self.v1_len[i]]
        self.launches = (1 if self.tails else 0) + 1 + 2 + (L // LEAF).bit_length() - 1


@functools.lru_cache(maxsize=None)
def shape(L: int, trailing: bool = False) -> Shape:
    s = Shape(L, trailing)
    assert s.P == 16 and len(s.pieces) == 20 * s.P and len(s.hashes) == s.P
    assert len(s.tails) == (10 if trailing else 9)
    return s


def load(ctx, s: Shape, first=0, count=None, pieces=None, hashes=None, staged=None, total=None, with_hashes=True,
         digests=True, fill=0xFF):
    """Layout (the v1 space), piece table, digests; the whole shard staged as `fill`, then the files."""
    count = s.P - first if count is None else count
    ctx.set_layout(s.total if total is None else total, s.L, s.P, first, count)
    ctx.v2_set_pieces(s.pb, s.tl, b"".join(s.hashes if hashes is None else hashes) if with_hashes else None)
    if digests:
        ctx.set_digests(s.pieces if pieces is None else pieces)
    if count and fill is not None:
        ctx.stage(first * s.L, bytes([fill]) * (count * s.L))
    for off, data in zip(s.offs, s.files if staged is None else staged):
        if len(data):
            ctx.stage(off, data)


def flipped(data: bytes, pos: int) -> bytes:
    b = bytearray(data)
    b[pos] ^= 0x20
    return bytes(b)


def read(ctx, off, n):
    out = bytearray(n)
    ctx.read(off, out)
    return bytes(out)


@pytest.mark.parametrize("L,trailing", [(32 * K, False), (32 * K, True), (64 * K, False), (64 * K, True)])
def test_clean_data_and_the_pad_ranges(ctx, native, L, trailing):
    s = shape(L, trailing)
    load(ctx, s)
    allocs = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    both, v1, v2 = ctx.hybrid_verify()
    assert (both, v1, v2) == (set_bits(s.P),) * 3
    assert ctx.last_kernel() == (native.KERNEL_HYBRID, s.launches)
    k, tot = ctx.last_timing()
    assert 0 < k <= tot
    # the lazily allocated tail table and second bitfield are counted, and reused by the second call
    held = ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS)
    assert held - allocs <= 2
    assert ctx.hybrid_verify() == (both, v1, v2)
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == held
    # every pad range reads as zeros; the byte before each tail and the first byte of the next row are unchanged
    for i in range(s.P):
        f, o, b, _ = s.table[i]
        if i in s.tails:
            assert read(ctx, i * L + b, s.v1_len[i] - b) == bytes(s.v1_len[i] - b), i
        assert read(ctx, i * L + b - 1, 1) == s.files[f][o + b - 1:o + b], i
        assert read(ctx, i * L, 1) == s.files[f][o:o + 1], i
    # tv_verify and tv_v2_verify on the same ctx keep their own answers, and allocate what they did
    assert ctx.verify() == set_bits(s.P) and ctx.last_kernel()[1] == 1
    assert ctx.v2_verify() == set_bits(s.P) and ctx.last_kernel()[0] == native.KERNEL_V2
    assert ctx.counter(native.TV_COUNTER_DEVICE_ALLOCS) == held


@pytest.mark.parametrize("L", [32 * K, 64 * K])
def test_a_flipped_byte_in_a_files_last_piece(ctx, L):
    s = shape(L)
    for k in (3, 8, 12):                                    # 17 bytes; L - 1 bytes; 2 L + 5 bytes (its 5-byte piece)
        staged = list(s.files)
        staged[k] = flipped(s.files[k], s.lengths[k] - 1)
        load(ctx, s, staged=staged)
        bad = s.offs[k] // L + (s.lengths[k] - 1) // L
        got = ctx.hybrid_verify()
        assert got == (set_bits(s.P, clear={bad}),) * 3, k
    # stale bytes in a pad range are not an error: the range is defined as zeros
    load(ctx, s, fill=0x5A)
    assert ctx.hybrid_verify() == (set_bits(s.P),) * 3


@pytest.mark.parametrize("L", [32 * K, 64 * K])
def test_descriptions_that_disagree(ctx, L):
    from torrent_amd.hybrid import HybridResult
    s = shape(L)
    for i in (0, 7, s.P - 1):
        wrong = bytearray(s.pieces)
        wrong[20 * i + 3] ^= 1
        load(ctx, s, pieces=bytes(wrong))
        both, v1, v2 = ctx.hybrid_verify()
        assert v1 == set_bits(s.P, clear={i}) and v2 == set_bits(s.P) and both == v1
        assert HybridResult(bytearray(both), bytearray(v1), bytearray(v2)).disagree == [i]
        assert ctx.verify() == v1 and ctx.v2_verify() == v2
        hs = list(s.hashes)
        hs[i] = flipped(hs[i], 31)
        load(ctx, s, hashes=hs)
        both, v1, v2 = ctx.hybrid_verify()
        assert v1 == set_bits(s.P) and v2 == set_bits(s.P, clear={i}) and both == v2
        assert HybridResult(bytearray(both), bytearray(v1), bytearray(v2)).disagree == [i]


def test_availability_clears_all_three(ctx):
    s = shape(32 * K)
    load(ctx, s)
    avail = bytearray(set_bits(s.P, clear={2, 9}))
    assert ctx.hybrid_verify(bytes(avail)) == (set_bits(s.P, clear={2, 9}),) * 3
    assert ctx.hybrid_verify() == (set_bits(s.P),) * 3


def test_pieces_marked_unreadable_by_file_staging(ctx, tmp_path):
    s = shape(32 * K)
    load(ctx, s)
    k = 10                                                   # the file of L + 1 bytes: pieces 9 and 10 of the layout
    first = s.offs[k] // s.L
    assert ctx.stage_file(str(tmp_path / "missing.bin"), 0, s.offs[k], s.lengths[k]) is False
    assert ctx.hybrid_verify() == (set_bits(s.P, clear={first, first + 1}),) * 3


@pytest.mark.parametrize("L,trailing", [(32 * K, False), (64 * K, True)])
def test_hash_equals_both_oracles(ctx, native, L, trailing):
    s = shape(L, trailing)
    load(ctx, s, with_hashes=False, digests=False)
    assert ctx.hybrid_hash() == (s.pieces, b"".join(s.hashes))
    assert ctx.last_kernel() == (native.KERNEL_HYBRID, s.launches)
    assert ctx.hybrid_hash() == (s.pieces, b"".join(s.hashes))
    assert ctx.hash() == s.pieces and ctx.v2_hash() == b"".join(s.hashes)
    # synthetic bytes with zeroed tails
    import hashlib
    ctx.fill_synthetic(77)
    d, r = ctx.hybrid_hash()
    for i in range(s.P):
        row = bytes(synth.fill(77, i * L, s.pb[i]))
        assert d[20 * i:20 * i + 20] == hashlib.sha1(row + bytes(s.v1_len[i] - s.pb[i])).digest(), i
        assert r[32 * i:32 * i + 32] == v2_ref.piece_root(row, s.tl[i]), i


@pytest.mark.parametrize("L", [32 * K, 64 * K])
def test_two_shards_give_the_whole_bitfield(ctx, L):
    s = shape(L)
    staged = list(s.files)
    staged[3] = flipped(s.files[3], 0)                       # piece 3, in the first shard
    staged[12] = flipped(s.files[12], 2 * L + 1)             # the last piece, in the second
    load(ctx, s, staged=staged)
    whole = ctx.hybrid_verify()
    assert whole == (set_bits(s.P, clear={3, s.P - 1}),) * 3
    load(ctx, s, staged=staged, first=0, count=8)
    a = ctx.hybrid_verify()
    load(ctx, s, staged=staged, first=8, count=8)
    b = ctx.hybrid_verify()
    assert tuple(x + y for x, y in zip(a, b)) == whole
    load(ctx, s, first=8, count=8, with_hashes=False, digests=False)
    d, r = ctx.hybrid_hash()
    assert d == s.pieces[160:] and r == b"".join(s.hashes[8:])


@pytest.mark.parametrize("pad", [64, 320])
def test_other_row_strides(native, pad):
    s = shape(32 * K, True)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_STRIDE_PAD, pad)
        load(c, s)
        assert c.hybrid_verify() == (set_bits(s.P),) * 3
        for i in s.tails:
            assert read(c, i * s.L + s.pb[i], s.L - s.pb[i]) == bytes(s.L - s.pb[i])


def _code(native, fn, *a):
    with pytest.raises(native.NativeError) as ei:
        fn(*a)
    return ei.value.code


def test_error_table(native):
    s = shape(32 * K)
    lib = native.lib()
    STATE, ARG = native.TV_ERR_STATE, native.TV_ERR_ARG
    with native.Context(0) as c:
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE    # before tv_set_layout
        # without a piece table; verify without digests; verify without v2 hashes
        c.set_layout(s.total, s.L, s.P, 0, s.P)
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE
        c.v2_set_pieces(s.pb, s.tl, b"".join(s.hashes))
        assert _code(native, c.hybrid_verify) == STATE
        load(c, s, with_hashes=False)
        assert _code(native, c.hybrid_verify) == STATE
        assert c.hybrid_hash() == (s.pieces, b"".join(s.hashes))
        # NULL outputs with a non-empty shard; a refused call changes nothing
        load(c, s)
        want = c.hybrid_verify()
        allocs = c.counter(native.TV_COUNTER_DEVICE_ALLOCS)
        buf = bytearray(32 * s.P)
        a, keep = native._addr(buf, writable=True)
        assert lib.tv_hybrid_verify(c._h, None, a, a, None) == ARG
        assert lib.tv_hybrid_hash(c._h, None, a) == ARG and lib.tv_hybrid_hash(c._h, a, None) == ARG
        assert buf == bytearray(32 * s.P)
        assert c.hybrid_verify() == want == (set_bits(s.P),) * 3
        assert lib.tv_hybrid_verify(c._h, None, None, None, a) == 0 and bytes(buf[:2]) == want[0]   # v1 / v2 outputs are optional
        assert c.counter(native.TV_COUNTER_DEVICE_ALLOCS) == allocs
        # during a stream
        c.v2_stream_begin(s.pb, s.tl, b"".join(s.hashes))
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE
        c.stream_abort()
        assert c.hybrid_verify() == want
        # a piece_bytes[i] > v1_len(i): the layout's total_length ends inside the last piece's bytes
        load(c, s, total=s.total - 1, fill=None)
        assert _code(native, c.hybrid_verify) == ARG and _code(native, c.hybrid_hash) == ARG
        assert "v1 length" in c._err()
        # an empty shard
        c.set_layout(s.total, s.L, s.P, s.P, 0)
        c.v2_set_pieces(s.pb, s.tl, b"".join(s.hashes))
        c.set_digests(s.pieces)
        assert lib.tv_hybrid_verify(c._h, None, None, None, None) == 0 and lib.tv_hybrid_hash(c._h, None, None) == 0
        # a slot pool; TV_OPT_RESIDENT = 0; a windowed layout
        c.set_option(native.TV_OPT_LIST_SLOTS, 4)
        c.set_layout(s.total, s.L, s.P, 0, s.P)
        c.set_option(native.TV_OPT_LIST_SLOTS, 0)
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE
        c.set_option(native.TV_OPT_RESIDENT, 0)
        c.set_layout(s.total, s.L, s.P, 0, s.P)
        c.set_option(native.TV_OPT_RESIDENT, 1)
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 6 * s.L)
        c.set_layout(s.total, s.L, s.P, 0, s.P)
        c.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) > 0
        assert _code(native, c.hybrid_verify) == STATE and _code(native, c.hybrid_hash) == STATE
        assert "windowed" in c._err()
        # and the ctx still works
        load(c, s)
        assert c.hybrid_verify() == want
        del keep


# ---- the Python host ---------------------------------------------------------------------------------------------------

def _write(root, s: Shape):
    from tests.v2_util import file_names
    paths = file_names(len(s.files))
    for comps, d in zip(paths, s.files):
        p = os.path.join(root, *comps)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(d)
    return paths


@pytest.mark.parametrize("trailing", [False, True])
def test_verify_payload_and_files_hybrid(tmp_path, trailing):
    from torrent_amd import parse_metainfo_hybrid, verify_files_hybrid, verify_payload_hybrid
    s = shape(32 * K, trailing)
    wrong = bytearray(s.pieces)
    wrong[20 * 11] ^= 4
    paths = _write(str(tmp_path), s)
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(s.files, s.L, paths=paths, trailing_pad=trailing, pieces=bytes(wrong)))
    assert meta is not None and meta.total_length == s.total
    bufs = list(s.files)
    bufs[4] = flipped(s.files[4], 9)                          # piece 4
    bufs[9] = None                                            # the file of L bytes: piece 8
    for devices in (None, [0, 0]):
        r = verify_payload_hybrid(meta, bufs, devices=devices)
        assert bytes(r.v1) == set_bits(s.P, clear={4, 8, 11}) and bytes(r.v2) == set_bits(s.P, clear={4, 8})
        assert bytes(r.bitfield) == bytes(r.v1) and r.disagree == [11]
    # from disk: no pad file exists under the directory, and none is looked for
    os.remove(os.path.join(str(tmp_path), *paths[9]))
    with open(os.path.join(str(tmp_path), *paths[4]), "wb") as f:
        f.write(bufs[4])
    r = verify_files_hybrid(meta, str(tmp_path), devices=[0, 0])
    assert bytes(r.v1) == set_bits(s.P, clear={4, 8, 11}) and bytes(r.v2) == set_bits(s.P, clear={4, 8})
    assert r.disagree == [11]


def test_make_torrent_hybrid_then_verify(tmp_path):
    from torrent_amd import make_torrent_hybrid, parse_metainfo, parse_metainfo_hybrid, parse_metainfo_v2, verify_files_hybrid
    s = shape(32 * K)
    root = str(tmp_path / "t")
    os.makedirs(root)
    paths = _write(root, s)
    tor = make_torrent_hybrid(root, "http://example.com/announce", creation_date=1, piece_length=s.L, devices=[0, 0])
    meta = parse_metainfo_hybrid(tor)
    assert meta is not None and [f.path for f in meta.files] == paths
    assert meta.pieces == s.pieces and meta.layout.hashes == b"".join(s.hashes) and meta.total_length == s.total
    assert parse_metainfo(tor).info.pieces_raw == s.pieces and parse_metainfo_v2(tor).hybrid
    r = verify_files_hybrid(meta, root)
    assert (bytes(r.bitfield), bytes(r.v1), bytes(r.v2)) == (set_bits(s.P),) * 3 and r.disagree == []
    with open(os.path.join(root, *paths[12]), "r+b") as f:    # the last file's 5-byte last piece
        f.seek(2 * s.L + 4)
        f.write(b"\x00" if s.files[12][-1] else b"\x01")
    r = verify_files_hybrid(meta, root)
    assert bytes(r.bitfield) == set_bits(s.P, clear={s.P - 1}) and r.disagree == []
