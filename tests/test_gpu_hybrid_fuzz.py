"""Seeded random hybrid torrents (tests/hybrid_fuzz.py) through the hybrid entry points, bit-exact against hashlib SHA-1
over the padded linear bytes (tests/hybrid_util.py) and the merkle reference (tests/v2_ref.py): the ABI shard by shard
(tv_hybrid_verify, tv_hybrid_hash; the shards' results joined are the whole torrent's, and one more shard ends inside
a byte of the bitfield), verify_payload_hybrid on one and on two shards, and for every third seed verify_files_hybrid
on a directory with files missing and truncated.  The expected bits of a piece: the disk can supply all of its bytes,
their SHA-1 with the pad's zeros equals the digest the torrent states (v1), their root in the piece's tree equals the
hash it states (v2); `bitfield` is the AND of the two, `disagree` the pieces where they differ."""
import pytest

from tests import hybrid_fuzz
from tests import hybrid_util as hu
from tests.hybrid_fuzz import SEEDS, draw
from tests.v2_util import file_names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cases():
    """Per seed, computed once: the draw, its layout, the stated hashes and the references of the staged bytes."""
    cache = {}

    def get(seed):
        if seed not in cache:
            d = draw(seed)
            lay = d.layout()
            pieces, hashes = d.stated(lay)
            cache[seed] = (d, lay, pieces, hashes) + lay.verdicts(d.staged, pieces, hashes)
        return cache[seed]
    return get


def _same(seed, lay, what, got, want):
    """got == want (one value per piece), or a failure naming the seed and the first differing piece."""
    got, want = list(got), list(want)
    assert len(got) == len(want), (seed, what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            f, o, b, _ = lay.table[i]
            pytest.fail("seed %d: %s differs first at piece %d (file %d, offset %d, %d bytes, v1 length %d): got %r, "
                        "want %r" % (seed, what, i, f, o, b, lay.v1_len[i], g, w))


def _split20(b: bytes) -> list:
    return [b[o:o + 20] for o in range(0, len(b), 20)]


def _split32(b: bytes) -> list:
    return [b[o:o + 32] for o in range(0, len(b), 32)]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_hybrids_abi(ctx, native, cases, seed):
    d, lay, pieces, hashes, ok1, ok2, staged1, staged2 = cases(seed)
    P = lay.P
    got = {"v1 bits": [], "v2 bits": [], "both": [], "v1 digests": [], "v2 hashes": []}
    ctx.set_option(native.TV_OPT_KERNEL, d.kernel)
    ctx.set_option(native.TV_OPT_LANE_PAIRS, d.lane_pairs)
    try:
        for first, count in d.shards:
            hu.load(ctx, lay, first, count, pieces=pieces, hashes=hashes, staged=d.staged)
            both, v1, v2 = ctx.hybrid_verify()
            assert ctx.last_kernel() == (native.KERNEL_HYBRID, lay.launches(first, count)), (seed, first, count)
            got["both"] += hu.unpack(both, count)
            got["v1 bits"] += hu.unpack(v1, count)
            got["v2 bits"] += hu.unpack(v2, count)
            dg, rt = ctx.hybrid_hash()
            got["v1 digests"] += _split20(dg)
            got["v2 hashes"] += _split32(rt)
            # the rows as the calls left them: the file bytes, zeros in the pad ranges
            rows = hu.read_shard(ctx, lay, first, count)
            at = hu.first_difference(rows, _staged_linear(d, lay)[first * lay.L:(first + count) * lay.L])
            assert at is None, (seed, "row", first + at // lay.L, "byte", at % lay.L)
        # one more shard, which ends inside a byte of the bitfield: the matching slices, spare bits 0 (hu.unpack)
        first, count = d.odd
        hu.load(ctx, lay, first, count, pieces=pieces, hashes=hashes, staged=d.staged)
        odd = [hu.unpack(f, count) for f in ctx.hybrid_verify()]
        odd_hashes = ctx.hybrid_hash()
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, 0)
    sl = slice(first, first + count)
    lead = [None] * first                                   # (so that a difference is named by its global piece)
    _same(seed, lay, "odd shard: both", lead + odd[0], lead + [a and b for a, b in zip(ok1[sl], ok2[sl])])
    _same(seed, lay, "odd shard: v1 bits", lead + odd[1], lead + ok1[sl])
    _same(seed, lay, "odd shard: v2 bits", lead + odd[2], lead + ok2[sl])
    assert odd_hashes == (staged1[20 * first:20 * (first + count)], b"".join(staged2[sl])), (seed, d.odd)
    _same(seed, lay, "v1 digests", got["v1 digests"], _split20(staged1))
    _same(seed, lay, "v2 hashes", got["v2 hashes"], staged2)
    _same(seed, lay, "v1 bits", got["v1 bits"], ok1)
    _same(seed, lay, "v2 bits", got["v2 bits"], ok2)
    _same(seed, lay, "both", got["both"], [a and b for a, b in zip(ok1, ok2)])
    assert len(got["both"]) == P


def _staged_linear(d, lay) -> bytes:
    return hu.padded_linear(d.staged, lay.L, lay.trailing)


def _disk_expected(d, ok1, ok2):
    can = d.readable()
    v1 = [a and c for a, c in zip(ok1, can)]
    v2 = [b and c for b, c in zip(ok2, can)]
    return v1, v2, [a and b for a, b in zip(v1, v2)], [i for i, (a, b) in enumerate(zip(v1, v2)) if a != b]


def _check_result(seed, lay, r, want, how):
    v1, v2, both, disagree = want
    P = lay.P
    _same(seed, lay, how + ": v1", hu.unpack(bytes(r.v1), P), v1)
    _same(seed, lay, how + ": v2", hu.unpack(bytes(r.v2), P), v2)
    _same(seed, lay, how + ": bitfield", hu.unpack(bytes(r.bitfield), P), both)
    assert r.disagree == disagree, (seed, how)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_hybrids_host_paths(native, cases, tmp_path, seed):
    from torrent_amd import parse_metainfo_hybrid, verify_files_hybrid, verify_payload_hybrid
    d, lay, pieces, hashes, ok1, ok2, _, _ = cases(seed)
    paths = file_names(len(d.lengths))
    meta = parse_metainfo_hybrid(hybrid_fuzz.torrent(d, lay, paths))
    assert meta is not None and meta.n_pieces == lay.P and meta.total_length == lay.total, seed
    assert meta.pieces == pieces and meta.layout.hashes == b"".join(hashes), seed
    disk = d.disk()
    want = _disk_expected(d, ok1, ok2)
    for devices in (None, [0, 0]):
        _check_result(seed, lay, verify_payload_hybrid(meta, disk, devices=devices), want, "payload %r" % (devices,))
    if seed % 3:
        return
    root = tmp_path / "dl"
    root.mkdir()
    for comps, data in zip(paths, disk):
        if data is None:
            continue
        p = root.joinpath(*comps)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)
    before = sorted(str(p) for p in root.rglob("*"))
    for devices in (None, [0, 0]):
        _check_result(seed, lay, verify_files_hybrid(meta, str(root), devices=devices), want, "files %r" % (devices,))
    assert sorted(str(p) for p in root.rglob("*")) == before             # nothing was created (no pad file either)
