"""Seeded random BitTorrent v2 layouts (tests/v2_fuzz.py) through every v2 entry point, bit-exact against the hashlib
reference (tests/v2_ref.py): the ABI on one and on three shards with availability bits, tv_v2_verify_list on a
resident shard and on a slot pool, the Python host paths (payload, files, incremental) and the creation round trip.
The expected bit of a piece: the disk can supply all of its bytes, and their root in the piece's tree equals the
expected hash (v2_ref.expected_bitfield with the declared file lengths)."""
import random

import pytest

from tests import v2_ref
from tests.v2_fuzz import SEEDS, draw
from tests.v2_util import file_names, set_bits, torrent_v2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def _bit(bf, i: int) -> int:
    return (bf[i >> 3] >> (7 - (i & 7))) & 1


def _and(a: bytes, b: bytes) -> bytes:
    assert len(a) == len(b)
    return bytes(x & y for x, y in zip(a, b))


def _piece(d, table, i: int) -> bytes:
    f, o, b, w = table[i]
    return d.staged[f][o:o + b]


def _load(ctx, d, table, hashes, first=0, count=None):
    """The layout, the (global) piece table and the corrupted files' bytes that meet the shard."""
    L, P = d.L, len(table)
    count = P - first if count is None else count
    ctx.set_layout((P - 1) * L + table[-1][2], L, P, first, count)
    ctx.v2_set_pieces([r[2] for r in table], [r[3] for r in table], hashes)
    lo, hi = first * L, (first + count) * L
    ctx.stage_many([(off, data) for off, data in zip(d.file_offsets(), d.staged)
                    if len(data) and off < hi and off + len(data) > lo])


# ---- the ABI: one shard under both mappings, three shards, the list call -------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_random_layouts_abi(ctx, native, seed):
    from torrent_amd.verify import shard_ranges
    d = draw(seed)
    table = d.table
    L, P = d.L, len(table)
    W = L // v2_ref.LEAF
    expected = d.expected()
    hashes = b"".join(expected)
    roots = b"".join(d.staged_roots())
    want = v2_ref.expected_bitfield(d.staged, L, expected)            # every file whole: only the corruptions drop
    assert want == set_bits(P, clear={i for i, _ in d.corrupt})
    rng = random.Random(9000 + seed)
    avail = rng.randbytes((P + 7) // 8)
    for mapping in (1, 2):
        ctx.set_option(native.TV_OPT_V2_MAP, mapping)
        try:
            _load(ctx, d, table, hashes)
            assert ctx.v2_hash() == roots, (seed, mapping)
            assert ctx.v2_verify() == want, (seed, mapping)
            assert ctx.v2_verify(avail) == _and(want, avail), (seed, mapping)
            assert ctx.counter(native.TV_COUNTER_V2_MAP) == (mapping if P >= 64 else native.V2_MAP_LEAF)
        finally:
            ctx.set_option(native.TV_OPT_V2_MAP, 0)
    # the list call on the resident shard (the bytes of the last load): a shuffled order with duplicates
    order = list(range(P)) + [rng.randrange(P) for _ in range(1 + P // 4)]
    rng.shuffle(order)
    ok = ctx.v2_verify_list(order, [table[i][2] for i in order], [table[i][3] for i in order],
                            b"".join(expected[i] for i in order))
    assert list(ok) == [_bit(want, i) for i in order], seed
    assert ctx.last_kernel() == (native.KERNEL_V2_LIST, 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-len(order) // max(1, 256 // W))
    # three shards, each with availability bits of its own (shard-local: bit 0 is the shard's first piece)
    got_bits, got_roots, all_avail = b"", b"", b""
    for first, count in shard_ranges(P, 3):
        assert first % 8 == 0 or count == 0
        if not count:
            continue
        _load(ctx, d, table, hashes, first, count)
        local = rng.randbytes((count + 7) // 8)
        got_roots += ctx.v2_hash()
        assert ctx.v2_verify() == bytes(want[first // 8:first // 8 + (count + 7) // 8]), (seed, first)
        got_bits += ctx.v2_verify(local)
        all_avail += local
    assert got_roots == roots, seed
    assert got_bits == _and(want, all_avail), seed


@pytest.mark.parametrize("seed", SEEDS)
def test_random_layouts_slot_pool(native, seed):
    d = draw(seed)
    table = d.table
    L, P = d.L, len(table)
    expected = d.expected()
    want = v2_ref.expected_bitfield(d.staged, L, expected)
    order = list(range(P))
    random.Random(9100 + seed).shuffle(order)
    with native.Context(0) as c:
        c.set_option(native.TV_OPT_LIST_SLOTS, 4)
        c.set_layout((P - 1) * L + table[-1][2], L, P)
        for k in range(0, P, 4):
            batch = order[k:k + 4]
            for i in batch:
                c.stage(i * L, _piece(d, table, i))
            assert c.counter(native.TV_COUNTER_SLOTS_USED) == len(batch)
            ok = c.v2_verify_list(batch, [table[i][2] for i in batch], [table[i][3] for i in batch],
                                  b"".join(expected[i] for i in batch))
            assert list(ok) == [_bit(want, i) for i in batch], (seed, batch)
            assert c.counter(native.TV_COUNTER_SLOTS_USED) == 0


# ---- the Python host paths --------------------------------------------------------------------------------------------------

def _write(root, paths, buffers):
    for comps, data in zip(paths, buffers):
        if data is None:
            continue
        p = root.joinpath(*comps)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_layouts_host_paths(native, tmp_path, seed):
    from torrent_amd import parse_metainfo_v2, verify_files_v2, verify_payload_v2
    d = draw(seed)
    L, P = d.L, len(d.table)
    paths = file_names(len(d.lengths))
    meta = parse_metainfo_v2(torrent_v2(d.files, L, name="fz", paths=paths))
    assert meta is not None and meta.n_pieces == P
    assert meta.layout.hashes == b"".join(d.expected())
    disk = d.disk()
    want = v2_ref.expected_bitfield(disk, L, d.expected(), have=d.lengths)
    for devices in ([0], [0, 0, 0]):
        assert bytes(verify_payload_v2(meta, disk, devices=devices)) == want, (seed, devices)
    root = tmp_path / "dl"
    root.mkdir()
    _write(root, paths, disk)
    before = sorted(str(p) for p in root.rglob("*"))
    for devices in ([0], [0, 0, 0]):
        assert bytes(verify_files_v2(meta, str(root), devices=devices, threads=3)) == want, (seed, devices)
    assert sorted(str(p) for p in root.rglob("*")) == before             # nothing was created


@pytest.mark.parametrize("seed", SEEDS)
def test_random_layouts_incremental(native, seed):
    from torrent_amd import FileInfo, IncrementalVerifierV2, MemoryStorage, Storage, make_info, parse_metainfo_v2
    from torrent_amd.piece import BLOCK_SIZE, PieceMsg
    d = draw(seed)
    table = d.table
    L, P = d.L, len(table)
    meta = parse_metainfo_v2(torrent_v2(d.files, L, name="fz"))
    lay = meta.layout
    disk = d.disk()
    want = v2_ref.expected_bitfield(disk, L, d.expected(), have=d.lengths)
    readable = [i for i, (f, o, b, w) in enumerate(table) if disk[f] is not None and len(disk[f]) >= o + b]
    rng = random.Random(9200 + seed)
    msgs = []
    for i in readable:
        f, o, b, w = table[i]
        msgs += [PieceMsg(i, q, disk[f][o + q:o + min(b, q + BLOCK_SIZE)]) for q in range(0, b, BLOCK_SIZE)]
    rng.shuffle(msgs)
    info = make_info(L, bytes(20), "fz", files=[FileInfo(n, ["f%d" % k]) for k, n in enumerate(d.lengths)])
    seen = {}
    v = IncrementalVerifierV2(lay, storage=Storage(MemoryStorage(), info, "dl"), flush_pieces=None,
                              flush_age_ms=None, slots=3, on_verified=lambda i, ok: seen.setdefault(i, []).append(ok))
    try:
        for m in msgs:
            v.on_block(m)
        for i, ok in v.flush():
            seen.setdefault(i, []).append(ok)
        assert sorted(seen) == readable, seed
        for i in readable:
            assert seen[i][0] == bool(_bit(want, i)), (seed, i)
        assert bytes(v.bitfield) == want, seed
        assert v.forced_flushes >= (1 if len(readable) > 3 else 0)
    finally:
        v.close()


# ---- creation: hash the uncorrupted files, write the .torrent, verify it against its own directory ------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_random_layouts_creation_round_trip(native, tmp_path, seed):
    from torrent_amd import make_torrent_v2, parse_metainfo_v2, verify_files_v2
    from torrent_amd.v2 import hash_files_v2
    d = draw(seed)
    L = d.L
    paths = file_names(len(d.lengths))
    root = tmp_path / "made"
    root.mkdir()
    _write(root, paths, d.files)
    for devices in ([0], [0, 0, 0]):
        hashed = hash_files_v2(str(root), L, files=list(zip(paths, d.lengths)), devices=devices)
        assert len(hashed) == len(d.files)
        for fh, data in zip(hashed, d.files):
            ref_root, ref_layer, _ = v2_ref.file_hashes(data, L)
            assert (fh.length, fh.pieces_root, fh.layer) == (len(data), ref_root, ref_layer), (seed, fh.path)
    meta = parse_metainfo_v2(make_torrent_v2(str(root), "http://example.com/announce", piece_length=L,
                                             creation_date=1))
    assert meta is not None and meta.name == "made"
    assert [(f.path, f.length) for f in meta.files] == list(zip(paths, d.lengths))
    assert meta.layout.hashes == b"".join(d.expected())
    assert bytes(verify_files_v2(meta, str(root))) == set_bits(meta.n_pieces)
