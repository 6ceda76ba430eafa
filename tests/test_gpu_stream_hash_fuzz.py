"""Seeded fuzz of the creation streams: 24 draws per kind from the existing generators (tests/v1_kernel_fuzz.py,
tests/v2_fuzz.py, tests/hybrid_fuzz.py), each capped at 4 MiB, hashed through tv_stream_hash_begin /
tv_v2_stream_hash_begin / tv_hybrid_stream_hash_begin (and tv_stream_hash_file_table for the v1 draws of two windows)
and compared with the CPU: hashlib SHA-1 and the merkle roots of tests/v2_ref.py over the draw's (corrupted) bytes.  A
creation stream has no digests and no availability, so a draw's flipped digests and masks do not enter; its piece
lengths, file tables, shards, column widths and forced kernels do."""
import pytest

from tests import hybrid_fuzz, v1_kernel_fuzz, v2_fuzz
from tests import hybrid_util as hu
from tests import v1_columns as vc
from tests.hybrid_stream_util import K, window_budget
from tests.test_gpu_stream_hash import force, stream_layout, table_stream, v1_stream

pytestmark = pytest.mark.gpu
CAP = 4 << 20
SEEDS = list(range(24))


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


def capped(files, cap: int = CAP) -> list:
    """The draw's files from the front while they total at most `cap` bytes; the file that crosses it is cut there."""
    out, room = [], cap
    for f in files:
        out.append(f[:room])
        room -= len(out[-1])
        if room == 0:
            break
    assert out and sum(len(f) for f in out) <= cap
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_v1_draws(ctx, native, tmp_path, seed):
    d = v1_kernel_fuzz.draw(seed)
    assert d.total <= CAP
    want = d.staged_digests()
    C = 64 * d.c
    try:
        force(ctx, native, None if d.kernel == "auto" else d.kernel)
        stream_layout(ctx, native, d.total, d.L, d.P, d.first, d.count, chunk=C)
        ctx.stream_hash_begin()
        v1_stream(ctx, d.staged, d.L, from_src=seed % 2 == 0, fill=0xFF)
        assert ctx.stream_hash_end() == want
        assert ctx.last_kernel()[1] == -(-d.L // min(C, -(-d.L // 64) * 64))
        if d.route == "win_columns":       # windows of 2,048 pieces x columns, the library's readers as the producer
            path = tmp_path / "payload"
            path.write_bytes(d.staged)
            budget = vc.column_budget(C)
            assert vc.stream_geometry(d.L, d.count, budget)[1] == 2048 < d.count
            stream_layout(ctx, native, d.total, d.L, d.P, d.first, d.count, budget=budget)
            got, status = ctx.stream_hash_file_table([d.total], [str(path)])
            assert status == [0] and got == want
    finally:
        force(ctx, native)


@pytest.mark.parametrize("seed", SEEDS)
def test_v2_draws(ctx, native, seed):
    d = v2_fuzz.draw(seed)
    lay = hu.Layout(capped(d.staged), d.L)
    want = b"".join(lay.hashes)
    kw = {"chunk": 16 * K} if seed % 2 else {"budget": window_budget(max(16 * K, d.L // 4))}
    stream_layout(ctx, native, lay.total, lay.L, lay.P, **kw)
    ctx.v2_stream_hash_begin(lay.pb, lay.tl)
    table_stream(ctx, lay)
    assert ctx.stream_hash_end() == want
    if lay.P > 9:                          # a shard that starts inside the torrent
        first = 8
        stream_layout(ctx, native, lay.total, lay.L, lay.P, first, lay.P - first, **kw)
        ctx.v2_stream_hash_begin(lay.pb, lay.tl)
        table_stream(ctx, lay, first)
        assert ctx.stream_hash_end() == want[32 * first:]


@pytest.mark.parametrize("seed", SEEDS)
def test_hybrid_draws(ctx, native, seed):
    d = hybrid_fuzz.draw(seed)
    lay = hu.Layout(capped(d.staged), d.L, d.trailing)
    want1, want2 = lay.pieces, b"".join(lay.hashes)
    kw = {"chunk": 16 * K} if seed % 2 else {"budget": window_budget(16 * K)}
    try:
        ctx.set_option(native.TV_OPT_KERNEL, d.kernel)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, d.lane_pairs)
        shards = [(0, lay.P)] + ([(8, lay.P - 8)] if lay.P > 9 else [])
        for first, count in shards:
            # (the chunk buffers hold the stream before: stale bytes where this one's pad ranges must read as zeros)
            stream_layout(ctx, native, lay.total, lay.L, lay.P, first, count, **kw)
            ctx.hybrid_stream_hash_begin(lay.pb, lay.tl)
            table_stream(ctx, lay, first)
            got = ctx.stream_hash_end()
            assert got == (want1[20 * first:20 * (first + count)], want2[32 * first:32 * (first + count)])
    finally:
        force(ctx, native)
