"""The batch layout on the GPU (tv_set_batch_layout, tv_batch_select, tv_batch_verify): many v1 torrents of mixed
piece lengths verified by one launch, on every kernel form.  Expected bits are hashlib's (tests/batch_fuzz.py
Torrent.expected: tv_verify's rule); the edge batch is also held to tv_verify of every torrent alone on a second
context.  The shapes total a few MiB."""
import ctypes
import os
import random

import pytest

from tests import batch_fuzz as bf
from tests.batch_fuzz import flip_byte, flip_digest, make

pytestmark = pytest.mark.gpu

KERNELS = ("auto", "lane", "split", "twin")
FORCED = ("lane", "split", "twin")


@pytest.fixture(scope="module")
def ctx(native):
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def ctx2(native):
    with native.Context(0) as c:
        yield c


@pytest.fixture(autouse=True)
def _defaults(ctx, native):
    yield
    for key in (native.TV_OPT_KERNEL, native.TV_OPT_RESIDENT_BUDGET, native.TV_OPT_LIST_SLOTS):
        ctx.set_option(key, 0)
    ctx.set_option(native.TV_OPT_RESIDENT, 1)


def edge_batch():
    """The torrents by their index in the batch (the one without pieces is put in the middle last)."""
    rng = random.Random(4711)
    ts = [make(16384, 4 * 16384 + last, rng) for last in (1, 55, 56, 63, 64, 119, 120)]    # 0 .. 4, 6, 7: 5 pieces each
    ts.append(make(100, 70 * 100, rng))              # 8: L not a multiple of 64, 70 pieces
    ts.append(make(65536, 3 * 65536, rng))           # 9
    ts.append(make(262144, 262144, rng))             # 10: one piece of 262,144 bytes
    ts.append(make(16384, 10, rng))                  # 11: one piece shorter than a block
    ts.insert(5, make(4096, 0, rng, 0))              # 5: a torrent without pieces in the middle
    ragged = make(4096, 5 * 4096, rng)
    ragged.digests = ragged.digests[:-13]            # the last slice is 7 bytes: it never matches
    ts.append(ragged)                                # 12
    ts.append(make(4096, 3 * 4096 + 100, rng, 6))    # 13: more digests than ceil(total / L): the surplus bits are 0
    assert [t.n for t in ts] == [5, 5, 5, 5, 5, 0, 5, 5, 70, 3, 1, 1, 5, 6]
    flip_byte(ts[0], 1, 0)                           # the first byte of a piece
    flip_byte(ts[1], 4, -1)                          # the last byte of a short last piece (55 bytes)
    flip_byte(ts[6], 4, -1)                          # ... and of one of 119 bytes
    flip_byte(ts[9], 2, 65536 - 30)                  # a byte in the last full block
    flip_byte(ts[10], 0, 262144 - 64)
    flip_digest(ts[8], 33)                           # one flipped digest bit
    return ts


@pytest.fixture(scope="module")
def edges(ctx2):
    ts = edge_batch()
    want = [t.expected() for t in ts]
    assert want[0] == [1, 0, 1, 1, 1] and want[1] == [1, 1, 1, 1, 0] and want[12] == [1, 1, 1, 1, 0]
    assert want[13] == [1, 1, 1, 0, 0, 0] and want[9] == [1, 1, 0] and want[11] == [1] and sum(want[8]) == 69
    alone = [bf.run_alone(ctx2, t) if t.n else [] for t in ts]       # tv_verify of every torrent alone
    assert alone == want
    return ts, want


@pytest.mark.parametrize("kernel", KERNELS)
def test_edge_batch(ctx, native, edges, kernel):
    ts, want = edges
    got = bf.run_batch(ctx, ts, kernel)
    assert got == want
    k, launches = ctx.last_kernel()
    auto = bf.auto_kernel(sum(t.n for t in ts))
    assert (k, launches) == (bf.KERNEL_IDS[auto if kernel == "auto" else kernel], 1)
    # the grid: one workgroup per group of the plan (the lane form: one wave per group, four waves a workgroup)
    name = auto if kernel == "auto" else kernel
    groups = len(bf.ref_plan([x for t in ts for x in t.lens()], bf.SPANS[name])[2])
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == (-(-groups // 4) if name == "lane" else groups)
    kernel_ms, total_ms = ctx.last_timing()
    assert 0 < kernel_ms <= total_ms


@pytest.mark.parametrize("kernel", FORCED)
@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65])
def test_group_edges(ctx, kernel, n):
    rng = random.Random(n)
    ts = [make(4096, (n - 5) * 4096, rng), make(4096, 5 * 4096, rng)]
    flip_byte(ts[1], 4, 100)                                       # the batch's last piece is bad
    got = bf.run_batch(ctx, ts, kernel)
    assert got == [[1] * (n - 5), [1, 1, 1, 1, 0]]


@pytest.mark.parametrize("kernel", FORCED)
def test_stale_bytes_under_short_last_pieces(ctx, kernel):
    rng = random.Random(99)
    full = []
    for _ in range(3):
        t = make(4096, 8 * 4096, rng)
        t.payload = t.staged = b"\xff" * t.total
        t.digests = make_digests(t)
        full.append(t)
    assert bf.run_batch(ctx, full, kernel) == [[1] * 8] * 3
    # a smaller batch on the same context: its short last pieces lie over the 0xFF bytes the first one left
    small = [make(4096, 4096 * 2 + 1, rng), make(4096, 4096 + 55, rng), make(4096, 4096 * 3 + 120, rng),
             make(4096, 63, rng)]
    flip_byte(small[2], 3, -1)
    want = [t.expected() for t in small]
    assert want == [[1, 1, 1], [1, 1], [1, 1, 1, 0], [1]]
    assert bf.run_batch(ctx, small, kernel) == want
    assert bf.run_batch(ctx, small, kernel) == want               # and again: nothing the launch left changes it


def make_digests(t):
    import hashlib
    return b"".join(hashlib.sha1(t.staged[i * t.L:i * t.L + t.piece_len(i)]).digest() for i in range(t.n))


def _write_files(dir_path, t, cuts):
    """The torrent's bytes as files f0, f1, .. of a multi-file torrent under dir_path, cut at `cuts` -> (lengths, paths)."""
    os.makedirs(dir_path, exist_ok=True)
    edges_ = [0] + list(cuts) + [t.total]
    lengths, paths = [], []
    for k, (a, b) in enumerate(zip(edges_, edges_[1:])):
        p = os.path.join(dir_path, f"f{k}")
        with open(p, "wb") as f:
            f.write(t.staged[a:b])
        lengths.append(b - a)
        paths.append(p)
    return lengths, paths


def test_selection_and_staging(ctx, native, tmp_path):
    from torrent_amd import make_info, release_contexts, verify_files
    from torrent_amd.metainfo import FileInfo
    rng = random.Random(31337)
    ts = [make(16384, 6 * 16384 + 777, rng), make(4096, 20 * 4096 + 55, rng), make(100, 33 * 100 + 7, rng)]
    flip_byte(ts[0], 2, 5)
    flip_byte(ts[2], 33, -1)
    files = {}
    files[0] = _write_files(str(tmp_path / "t0"), ts[0], [1000, 16384 * 2, 16384 * 2, 70000])    # a zero-length file too
    files[1] = _write_files(str(tmp_path / "t1"), ts[1], [4096 * 3 + 10, 4096 * 9, 4096 * 15 + 1])
    os.remove(files[1][1][2])                                      # torrent 1's third file is missing
    info1 = make_info(4096, ts[1].digests, "t1", files=[FileInfo(n, [f"f{k}"]) for k, n in enumerate(files[1][0])])
    alone = bf.bits_list(verify_files(info1, str(tmp_path / "t1")), ts[1].n)
    release_contexts()
    assert not os.path.exists(files[1][1][2])                      # (nothing is created)
    lost = [i for i in range(ts[1].n) if not alone[i]]
    assert lost and lost == [i for i in range(ts[1].n) if i * 4096 < 4096 * 15 + 1 and (i + 1) * 4096 > 4096 * 9]
    ts[0].avail = [1, 1, 1, 0, 1, 1, 1]
    statuses = {}
    ctx.set_option(native.TV_OPT_KERNEL, 0)
    ctx.set_batch_layout([t.total for t in ts], [t.L for t in ts], [t.n for t in ts])
    for k in (2, 0, 1):                                            # staged in another order than the batch's
        t = ts[k]
        ctx.batch_select(k)
        ctx.set_digests(t.digests)
        if k == 2:
            cut = [0, 7, 100, 1500, 1501, t.total]
            ctx.stage_many([(a, t.staged[a:b]) for a, b in zip(cut, cut[1:])])
        else:
            statuses[k] = ctx.stage_file_table(*files[k])
    assert statuses[0] == [0] * 5 and statuses[1] == [0, 0, native.TV_ERR_IO, 0]
    for k in (1, 2, 0, 2):                                         # tv_read returns each torrent's own bytes
        t = ts[k]
        ctx.batch_select(k)
        out = bytearray(t.total)
        ctx.read(0, out)
        if k == 1:
            a, b = 4096 * 9, 4096 * 15 + 1                         # (the missing file's bytes were never staged)
            assert bytes(out[:a]) == t.staged[:a] and bytes(out[b:]) == t.staged[b:]
        else:
            assert bytes(out) == t.staged
        tail = bytearray(5)
        ctx.read(t.total - 5, tail)                                # an offset in the torrent's own linear space
        assert bytes(tail) == t.staged[-5:]
    got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(bf.avail_bytes(ts)), ts)]
    want1 = [int(i not in lost) for i in range(ts[1].n)]
    assert want1 == alone                                          # exactly the pieces verify_files zeroes for it alone
    assert got == [ts[0].expected(), want1, ts[2].expected()]
    assert got[0] == [1, 1, 0, 0, 1, 1, 1] and got[2] == [1] * 33 + [0]
    # the marks survive selecting other torrents; without the availability mask only its piece comes back
    ctx.batch_select(0)
    got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(None), ts)]
    assert got == [[1, 1, 0, 1, 1, 1, 1], want1, ts[2].expected()]
    # staging the missing bytes from memory clears the marks of the pieces it covers whole
    ctx.batch_select(1)
    ctx.stage(0, ts[1].staged)
    got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(None), ts)]
    assert got[1] == ts[1].expected() == [1] * 21


REFUSED = ("tv_verify", "tv_hash", "tv_verify_list", "tv_verify_host")


def _refused_names(native):
    names = [n for n, _, _ in native.SYMBOLS
             if n in REFUSED or n.startswith(("tv_stream_", "tv_v2_", "tv_hybrid_"))]
    names.remove("tv_stream_abort")                                 # (it verifies nothing: it stays a no-op)
    assert len(names) >= 30
    return names


def test_refusals(ctx, native):
    lib = native.lib()
    rng = random.Random(5)
    ts = [make(4096, 3 * 4096 + 9, rng), make(64, 64 * 5, rng)]
    assert bf.run_batch(ctx, ts) == [[1] * 4, [1] * 5]
    # every other verifying or hashing call: TV_ERR_STATE, and the text says that a batch layout is set
    req, scratch = native.StreamReq(), ctypes.create_string_buffer(64)
    for name, _, argtypes in native.SYMBOLS:
        if name not in _refused_names(native):
            continue
        args = [ctx._h]
        for a in argtypes[1:]:
            if hasattr(a, "contents"):
                args.append(ctypes.byref(req))
            elif a is ctypes.c_void_p and name == "tv_stream_commit_from" and len(args) == 2:
                args.append(ctypes.cast(scratch, ctypes.c_void_p))
            elif a in (ctypes.c_void_p, ctypes.c_char_p):
                args.append(None)
            else:
                args.append(0)
        rc = getattr(lib, name)(*args)
        assert rc == native.TV_ERR_STATE, (name, rc, ctx._err())
        assert "a batch layout is set" in ctx._err(), (name, ctx._err())
    with pytest.raises(native.NativeError) as e:
        ctx.verify()
    assert e.value.code == native.TV_ERR_STATE and "a batch layout is set" in str(e.value)
    # the batch is still there
    assert [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(), ts)] == [[1] * 4, [1] * 5]
    # tv_batch_select out of range
    with pytest.raises(native.NativeError) as e:
        ctx.batch_select(2)
    assert e.value.code == native.TV_ERR_ARG and "torrent 2" in str(e.value)
    # a torrent whose digests were never set
    ctx.set_batch_layout([t.total for t in ts], [t.L for t in ts], [t.n for t in ts])
    ctx.batch_select(0)
    ctx.set_digests(ts[0].digests)
    with pytest.raises(native.NativeError) as e:
        ctx.batch_verify()
    assert e.value.code == native.TV_ERR_STATE and "torrent 1" in str(e.value) and "tv_set_digests" in str(e.value)
    # a geometry tv_set_layout would refuse names its torrent
    with pytest.raises(native.NativeError) as e:
        ctx.set_batch_layout([10, 10], [4096, 0], [1, 1])
    assert e.value.code == native.TV_ERR_ARG and "torrent 1" in str(e.value)
    with pytest.raises(native.NativeError) as e:
        ctx.set_batch_layout([10, 10, 10], [64, 64, 64], [2 ** 31, 2 ** 31 - 1, 1])
    assert e.value.code == native.TV_ERR_ARG and "torrent 1" in str(e.value)
    # over the budget: TV_ERR_NOMEM naming the bytes and the budget; a smaller batch then succeeds on the same context
    ctx.set_option(native.TV_OPT_RESIDENT_BUDGET, 1 << 20)
    big = [make(65536, 65536 * 10, rng), make(65536, 65536 * 10, rng)]
    need = 2 * 10 * (65536 + 256) + 256
    with pytest.raises(native.NativeError) as e:
        ctx.set_batch_layout([t.total for t in big], [t.L for t in big], [t.n for t in big])
    assert e.value.code == native.TV_ERR_NOMEM and str(need) in str(e.value) and str(1 << 20) in str(e.value)
    assert bf.run_batch(ctx, big[:1]) == [[1] * 10]
    ctx.set_option(native.TV_OPT_RESIDENT_BUDGET, 0)
    # a slot pool or a layout without a resident payload
    ctx.set_option(native.TV_OPT_LIST_SLOTS, 4)
    with pytest.raises(native.NativeError) as e:
        ctx.set_batch_layout([10], [64], [1])
    assert e.value.code == native.TV_ERR_STATE and "TV_OPT_LIST_SLOTS" in str(e.value)
    ctx.set_option(native.TV_OPT_LIST_SLOTS, 0)
    ctx.set_option(native.TV_OPT_RESIDENT, 0)
    with pytest.raises(native.NativeError) as e:
        ctx.set_batch_layout([10], [64], [1])
    assert e.value.code == native.TV_ERR_STATE and "TV_OPT_RESIDENT" in str(e.value)
    ctx.set_option(native.TV_OPT_RESIDENT, 1)


def test_set_layout_ends_the_batch(ctx, native):
    rng = random.Random(6)
    t = make(4096, 9 * 4096 + 300, rng)
    flip_byte(t, 4, 17)
    before = bf.run_alone(ctx, t)
    assert before == t.expected() == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert bf.run_batch(ctx, [make(100, 550, rng), t, make(65536, 65536 * 2, rng)])[1] == before
    with pytest.raises(native.NativeError):
        ctx.verify()
    assert bf.run_alone(ctx, t) == before                          # tv_verify gives what it gave before the batch
    for call in (lambda: ctx.batch_select(0), ctx.batch_verify):   # and the batch calls need a batch layout again
        with pytest.raises(native.NativeError) as e:
            call()
        assert e.value.code == native.TV_ERR_STATE and "tv_set_batch_layout" in str(e.value)


def test_hosts(native, tmp_path):
    """verify_payload_batch / verify_files_batch on 6 small torrents under a budget that makes two batches and one
    single-torrent item equal verify_payload / verify_files item by item."""
    from torrent_amd import (make_info, plan_batches, release_contexts, verify_files, verify_files_batch, verify_payload,
                             verify_payload_batch)
    from torrent_amd.batch import region_bytes
    from torrent_amd.metainfo import FileInfo
    rng = random.Random(77)
    ts = [make(4096, 10 * 4096 + 5, rng), make(16384, 3 * 16384, rng), make(100, 4000 + 99, rng),
          make(16384, 40 * 16384 + 1, rng), make(4096, 0, rng, 0), make(65536, 2 * 65536 + 1000, rng)]
    flip_byte(ts[0], 10, -1)
    flip_byte(ts[3], 17, 0)
    flip_digest(ts[5], 1)
    infos, dirs = [], []
    for k, t in enumerate(ts):
        cuts = sorted(rng.sample(range(1, t.total), 2)) if t.total > 2 else []
        lengths, _ = _write_files(str(tmp_path / f"t{k}"), t, cuts)
        infos.append(make_info(t.L, t.digests, f"t{k}", files=[FileInfo(n, [f"f{j}"]) for j, n in enumerate(lengths)]))
        dirs.append(str(tmp_path / f"t{k}"))
    os.remove(os.path.join(dirs[2], "f1"))
    budget = 300 << 10
    plan = plan_batches([region_bytes(i) for i in infos], budget)
    assert plan == [("batch", [0, 1, 2]), ("single", [3]), ("batch", [4, 5])]
    try:
        want = [bytearray(verify_payload(i, t.staged)) for i, t in zip(infos, ts)]
        assert [bf.bits_list(w, t.n) for w, t in zip(want, ts)] == [t.expected() for t in ts]
        assert verify_payload_batch(list(zip(infos, [t.staged for t in ts])), budget=budget) == want
        short = ts[1].staged[:16384 * 2 + 5]                        # a payload that ends early: its pieces are unreadable
        assert verify_payload_batch([(infos[1], short), (infos[0], ts[0].staged)]) == [
            bytearray(verify_payload(infos[1], short)), want[0]]
        want_f = [bytearray(verify_files(i, d)) for i, d in zip(infos, dirs)]
        assert want_f[2] != want[2] and want_f[0] == want[0]
        assert verify_files_batch(list(zip(infos, dirs)), budget=budget) == want_f
        assert verify_files_batch(list(zip(infos, dirs)), budget=budget, open_rw=False, threads=2) == want_f
        assert verify_payload_batch([]) == [] and verify_files_batch([]) == []
    finally:
        release_contexts()
