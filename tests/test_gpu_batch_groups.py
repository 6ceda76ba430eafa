"""tv_batch_verify on dense mixed-length groups (tests/batch_groups.py; tests/test_batch_groups_shapes.py holds the
shapes to their promises on the CPU), on every kernel form: ladders, one full group each with every block count
nb_max - T .. nb_max in it, so the masked tails of rounds_wave and of the lane form and the helper's padded-block region
run T blocks from either parity; the staircase, whose groups are nearly all cut early and padded; a digest corrupted by
index bit, which tells any two entries apart; the crowd of 16,400 short pieces (the lane form by auto, more workgroups
than CUs, the device tables at another capacity than the launch's); availability across byte-aligned neighbours.
Expected bits are hashlib's (batch_fuzz.Torrent.expected) and every comparison is exact."""
import ctypes
import dataclasses
import functools
import random

import pytest

from tests import batch_fuzz as bf
from tests import batch_groups as bg

pytestmark = pytest.mark.gpu

FORCED = ("lane", "split", "twin")
KERNELS = ("auto",) + FORCED


@pytest.fixture(scope="module")
def ctx(native):
    with native.Context(0) as c:
        yield c


@pytest.fixture(autouse=True)
def _defaults(ctx, native):
    yield
    ctx.set_option(native.TV_OPT_KERNEL, 0)


@pytest.fixture(scope="module")
def cus():
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0     # hipDeviceAttributeMultiprocessorCount
    return n.value


@functools.lru_cache(maxsize=None)
def _ladder(span, nb_max, T):
    """A ladder and its expected bits, built once for the forms that share its span."""
    ts = bg.ladder(span, nb_max, T)
    return ts, [t.expected() for t in ts]


@pytest.fixture(scope="module")
def stair():
    ts = bg.staircase()
    return ts, [t.expected() for t in ts]


@pytest.fixture(scope="module")
def crowd():
    ts = bg.crowd()
    return ts, [t.expected() for t in ts]


def _workgroups(ts, name):
    groups = len(bf.ref_plan(bg.all_lens(ts), bf.SPANS[name])[2])
    return -(-groups // 4) if name == "lane" else groups


def _check_launch(ctx, native, ts, kernel, cus):
    """The form the launch reports and its grid: one workgroup per group of the plan (lane: four groups each)."""
    name = bf.auto_kernel(sum(t.n for t in ts), cus) if kernel == "auto" else kernel
    assert ctx.last_kernel() == (bf.KERNEL_IDS[name], 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == _workgroups(ts, name)
    return name


def _bad(got, want):
    return [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8]


@pytest.mark.parametrize("nb_max", sorted({nb for nb, _ in bg.ladder_grid()}))
@pytest.mark.parametrize("kernel", FORCED)
def test_ladders(ctx, kernel, nb_max):
    span = bf.SPANS[kernel]
    for T in [T for nb, T in bg.ladder_grid() if nb == nb_max]:
        ts, want = _ladder(span, nb_max, T)
        assert sum(map(sum, want)) == span - 3                         # the longest, the shortest, the middle one
        got = bf.run_batch(ctx, ts, kernel)
        assert got == want, (kernel, nb_max, T, _bad(got, want))
        assert ctx.last_kernel() == (bf.KERNEL_IDS[kernel], 1)


@pytest.mark.parametrize("kernel", KERNELS)
def test_staircase(ctx, native, cus, stair, kernel):
    ts, want = stair
    got = bf.run_batch(ctx, ts, kernel)
    assert got == want, (kernel, _bad(got, want))
    _check_launch(ctx, native, ts, kernel, cus)
    # the same torrents in another order: where the stable sort puts an entry does not change its answer
    perm, ts2 = bg.shuffled(ts)
    got2 = bf.run_batch(ctx, ts2, kernel)
    assert got2 == [got[p] for p in perm], (kernel, _bad(got2, [got[p] for p in perm]))
    _check_launch(ctx, native, ts2, kernel, cus)


@pytest.fixture(scope="module")
def stair_index_bits(stair):
    """Per index bit k: every torrent's digests with the entries of bit k corrupted, and the bits hashlib expects."""
    ts, _ = stair
    out = []
    for k in range(bg.index_bits(sum(t.n for t in ts))):
        ds = bg.index_bit_digests(ts, k)
        out.append((ds, [dataclasses.replace(t, digests=d).expected() for t, d in zip(ts, ds)]))
    return out


@pytest.mark.parametrize("kernel", FORCED)
def test_digest_corrupted_by_index_bit(ctx, stair, stair_index_bits, kernel):
    ts, want0 = stair
    assert bf.run_batch(ctx, ts, kernel) == want0                      # stages the payload, once
    assert len(stair_index_bits) == 10
    for k, (ds, want) in enumerate(stair_index_bits):
        assert want != want0
        for q, d in enumerate(ds):
            ctx.batch_select(q)
            ctx.set_digests(d)
        got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(None), ts)]
        assert got == want, (kernel, k, _bad(got, want))


def test_crowd_forms_and_table_reuse(ctx, native, cus, crowd):
    ts, want = crowd
    n = sum(t.n for t in ts)
    assert n > 16384
    if 64 * cus < n:
        assert bf.auto_kernel(n, cus) == "lane"                        # (the MI355X: 256 CUs)
    for kernel in KERNELS:
        got = bf.run_batch(ctx, ts, kernel)
        assert got == want, (kernel, _bad(got, want))
        _check_launch(ctx, native, ts, kernel, cus)
    # the same layout through the other forms without setting it again (tv_set_batch_layout frees the launch tables):
    # groups of 32 pad differently from groups of 64, so the lane launch is longer than the twin launch that sized the
    # tables (they grow), and the twin launch after it is shorter than their capacity (d_len and d_col lie further out)
    m = {name: len(bf.ref_plan(bg.all_lens(ts), bf.SPANS[name])[0]) for name in ("twin", "lane")}
    assert m["twin"] < m["lane"] and KERNELS[-1] == "twin"
    for kernel in ("lane", "twin", "split"):
        ctx.set_option(native.TV_OPT_KERNEL, bf.KERNEL_IDS[kernel])
        got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(None), ts)]
        assert got == want, (kernel, _bad(got, want))
        _check_launch(ctx, native, ts, kernel, cus)
    # small batches on the context the crowd grew
    rng = random.Random(9)
    nine = [bf.make(4096, 4 * 4096 + 56, rng), bf.make(100, 333, rng)]
    bf.flip_byte(nine[0], 4, -1)
    bf.flip_digest(nine[1], 2)
    assert sum(t.n for t in nine) == 9
    for kernel in FORCED:
        lad, lad_want = _ladder(bf.SPANS[kernel], 10, 7)
        assert bf.run_batch(ctx, lad, kernel) == lad_want
        assert bf.run_batch(ctx, nine, kernel) == [t.expected() for t in nine] == [[1, 1, 1, 1, 0], [1, 1, 0, 1]]
    # and the crowd again, after the tables shrank and regrew
    for kernel in ("auto", "twin"):
        got = bf.run_batch(ctx, ts, kernel)
        assert got == want, (kernel, _bad(got, want))
        _check_launch(ctx, native, ts, kernel, cus)


@pytest.mark.parametrize("kernel", FORCED)
def test_availability_of_byte_aligned_neighbours(ctx, stair, kernel):
    """Every torrent's availability bitfield is whole bytes, back to back with the next one's: a one-piece torrent owns a
    byte with seven spare bits.  Every third torrent is unavailable and the caller's spare bits are all 1 (the bytes
    built by hand: batch_fuzz.avail_bytes writes zeros there): the spare bits of the answer are 0 (bits_list asserts it)
    and no neighbour's bit changes."""
    ts, want0 = stair
    masks = [[int(k % 3 != 0)] * t.n for k, t in enumerate(ts)]
    avail = bytearray()
    for t, mask in zip(ts, masks):
        field = bytearray(bf.bitfield(mask))
        if t.n % 8:
            field[-1] |= 0xFF >> (t.n % 8)
        avail += field
    assert sum(1 for t in ts if t.n % 8) >= bg.STAIR_COUNT and avail[1] == 0xFF and avail[0] == 0x7F
    want = [t.expected(avail=mask) for t, mask in zip(ts, masks)]
    assert want != want0 and all(not any(w) for w in want[::3]) and want[1::3] == want0[1::3]
    ctx.set_option(1, bf.KERNEL_IDS[kernel])
    ctx.set_batch_layout([t.total for t in ts], [t.L for t in ts], [t.n for t in ts])
    for k, t in enumerate(ts):
        ctx.batch_select(k)
        ctx.set_digests(t.digests)
        ctx.stage(0, t.staged)
    got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(bytes(avail)), ts)]
    assert got == want, (kernel, _bad(got, want))
    got = [bf.bits_list(b, t.n) for b, t in zip(ctx.batch_verify(None), ts)]      # without the mask: every torrent's own
    assert got == want0, (kernel, _bad(got, want0))
