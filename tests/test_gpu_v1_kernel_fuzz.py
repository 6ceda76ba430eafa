"""Seeded random BitTorrent v1 cases (tests/v1_kernel_fuzz.py) through the SHA-1 kernel forms on every path that launches
them, bit-exact against hashlib: the resident shard (tv_verify + tv_hash), a windowed layout (windows of three pieces),
streamed columns and streamed windows x columns (tv_verify_host, from pageable and page-locked memory), tv_verify_list
over a shuffled list with duplicates, and tv_verify_list on a slot pool -- each under a forced kernel form of
tests/v1_columns.py VARIANTS or the library's own choice, on a shard, with availability bits, flipped bytes, flipped
digests and sometimes a ragged digest string.  tests/test_v1_kernel_fuzz_draw.py holds the seeds to their features."""
import pytest

from tests import v1_columns as vc
from tests.v1_kernel_fuzz import SEEDS, WINDOW, draw

pytestmark = pytest.mark.gpu


def _resident(native, ctx, d, kernel):
    windowed = d.route == "windowed"
    if windowed:
        ctx.set_option(native.TV_OPT_RESIDENT_BUDGET, d.window_budget(native.WIN_BUFS_DEFAULT))
    ctx.set_layout(d.total, d.L, d.P, d.first, d.count)
    in_windows = windowed and d.windowed(native.WIN_BUFS_DEFAULT)
    assert ctx.counter(native.TV_COUNTER_WINDOW_PIECES) == (WINDOW if in_windows else 0)
    launches = -(-d.count // WINDOW) if in_windows else 1
    ctx.set_digests(d.digests)
    ctx.stage(d.first * d.L, d.shard_bytes())
    got = ctx.verify(d.avail)
    assert len(got) == (d.count + 7) // 8 and vc.bits(got, d.count) == d.expected()
    assert ctx.last_kernel() == (kernel, launches)
    if windowed:
        ctx.stage(d.first * d.L, d.shard_bytes())              # a new pass
    assert ctx.hash() == d.staged_digests()
    assert ctx.last_kernel() == (kernel, launches)


def _streamed(native, ctx, d, kernel):
    C = 64 * d.c
    ctx.set_option(native.TV_OPT_RESIDENT, 0)
    if d.route == "columns":
        ctx.set_option(native.TV_OPT_STREAM_CHUNK, C)
        units = vc.host_units(d.L, d.count, C, 0)
        assert units == -(-d.L // C)
    else:
        budget = vc.column_budget(C)
        ctx.set_option(native.TV_OPT_RESIDENT_BUDGET, budget)
        units = vc.host_units(d.L, d.count, 0, budget)
        assert vc.stream_geometry(d.L, d.count, budget) == (C, vc.MIN_WIN) and units == 2 * -(-d.L // C)
    ctx.set_layout(d.total, d.L, d.P, d.first, d.count)
    ctx.set_digests(d.digests)
    src = d.shard_bytes()
    got = ctx.verify_host(src, d.avail)
    assert len(got) == (d.count + 7) // 8 and vc.bits(got, d.count) == d.expected()
    assert ctx.last_kernel() == (kernel, units)
    with native.PinnedBuffer(len(src)) as pinned:               # page-locked: 2D copies straight from the source
        pinned.mv[:] = src
        assert ctx.verify_host(pinned.mv, d.avail) == got
    assert ctx.last_kernel() == (kernel, units)


def _listed(native, ctx, d, kernel):
    ctx.set_layout(d.total, d.L, d.P, d.first, d.count)
    ctx.set_digests(d.digests)
    ctx.stage(d.first * d.L, d.shard_bytes())
    want = {i: d.matches(i) for i in set(d.order)}
    assert list(ctx.verify_list(d.order)) == [want[i] for i in d.order]
    assert ctx.last_kernel() == (kernel, 1)
    assert vc.bits(ctx.verify(d.avail), d.count) == d.expected()   # and the shard's own bits, availability applied


def _slotted(native, ctx, d, kernel):
    ctx.set_option(native.TV_OPT_LIST_SLOTS, d.slots)
    ctx.set_layout(d.total, d.L, d.P, d.first, d.count)
    ctx.set_digests(d.digests)
    K = min(d.slots, d.count)
    assert ctx.counter(native.TV_COUNTER_PAYLOAD_BYTES) == K * d.stride() + 256
    for k in range(0, len(d.order), d.slots):
        batch = list(dict.fromkeys(d.order[k:k + d.slots]))    # up to `slots` pieces, each staged once
        for i in batch:
            ctx.stage(i * d.L, d.piece(i))
        assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == len(batch)
        never = next((i for i in range(d.first, d.first + d.count) if i not in batch), None)
        asked = batch + batch[:1] + ([never] if never is not None else [])   # a duplicate, and a piece never staged
        want = [d.matches(i) for i in batch + batch[:1]] + ([0] if never is not None else [])
        assert list(ctx.verify_list(asked)) == want, (k, asked)
        assert ctx.last_kernel() == (kernel, 1)
        assert ctx.counter(native.TV_COUNTER_SLOTS_USED) == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_random_cases_across_kernels_and_paths(native, seed):
    d = draw(seed)
    kernel, pairs, lane_pairs = vc.VARIANTS.get(d.kernel, (0, 0, 0))
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_KERNEL, kernel)
        ctx.set_option(native.TV_OPT_SPLIT_PAIRS, pairs)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, lane_pairs)
        # the library's own choice at these piece counts (at most 2,048 pieces per launch) is the twin kernel
        ran = kernel or vc.TWIN
        {"resident": _resident, "windowed": _resident, "columns": _streamed, "win_columns": _streamed,
         "list": _listed, "list_slots": _slotted}[d.route](native, ctx, d, ran)
