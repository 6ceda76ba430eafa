"""Seeded random batches (tests/batch_fuzz.py draw: 1 .. 40 torrents of mixed piece lengths, 0 .. 90 pieces each, at
most 8 MiB, with flipped bytes and digests, ragged digest strings, surplus digests and availability masks) through
tv_batch_verify on every kernel form.  Expected bits are hashlib's (Torrent.expected)."""
import pytest

from tests import batch_fuzz as bf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(native):
    with native.Context(0) as c:
        yield c
        c.set_option(native.TV_OPT_KERNEL, 0)


@pytest.fixture(scope="module")
def draws():
    """Every seed's torrents and the bits expected of them, computed once for the three kernel forms."""
    out = {}
    for seed in bf.SEEDS:
        ts = bf.draw(seed)
        out[seed] = (ts, [t.expected() for t in ts])
    return out


@pytest.mark.parametrize("kernel", ["lane", "split", "twin"])
@pytest.mark.parametrize("seed", bf.SEEDS)
def test_batch_fuzz(ctx, draws, seed, kernel):
    ts, want = draws[seed]
    got = bf.run_batch(ctx, ts, kernel)
    assert got == want, (seed, kernel, [k for k, (g, w) in enumerate(zip(got, want)) if g != w])
    if sum(t.n for t in ts):
        assert ctx.last_kernel() == (bf.KERNEL_IDS[kernel], 1)
