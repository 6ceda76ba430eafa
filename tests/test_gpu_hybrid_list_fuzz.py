"""Seeded random hybrid torrents (tests/hybrid_fuzz.py, the draws of tests/test_gpu_hybrid_fuzz.py) through
tv_hybrid_verify_list on a slot pool: every piece staged over a 0xFF fill of its row, the torrent's stated `pieces` and
hashes with the draw's flips, the draw's forced SHA-1 kernel, all pieces listed in a seeded shuffle with a few
duplicates, split into two calls.  The verdicts equal hashlib SHA-1 over the padded linear bytes and the merkle
reference (tests/hybrid_util.py Layout.verdicts)."""
import random

import pytest

from tests import hybrid_list_util as hl
from tests.hybrid_fuzz import SEEDS, draw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


@pytest.mark.parametrize("seed", SEEDS)
def test_random_hybrids_on_a_slot_pool(ctx, native, seed):
    d = draw(seed)
    lay = d.layout()
    pieces, hashes = d.stated(lay)
    ok1, ok2, _, _ = lay.verdicts(d.staged, pieces, hashes)
    P = lay.P
    rng = random.Random(9100 + seed)
    order = list(range(P))
    rng.shuffle(order)
    listed = list(range(P)) + rng.sample(range(P), min(P, 3))
    rng.shuffle(listed)
    cut = rng.randrange(1, len(listed))
    ctx.set_option(native.TV_OPT_KERNEL, d.kernel)
    ctx.set_option(native.TV_OPT_LANE_PAIRS, d.lane_pairs)
    got = [[], [], []]
    try:
        hl.set_pool(ctx, native, lay, P, pieces=pieces)
        hl.stage_pieces(ctx, lay, order, d.staged)
        # (release = False for the first call: a piece listed in both calls still holds its slot for the second)
        for part, release in ((listed[:cut], False), (listed[cut:], True)):
            for k, r in enumerate(hl.run_list(ctx, lay, part, hashes=hashes, release=release)):
                got[k] += r
            assert ctx.last_kernel()[0] == native.KERNEL_HYBRID_LIST
    finally:
        ctx.set_option(native.TV_OPT_KERNEL, 0)
        ctx.set_option(native.TV_OPT_LANE_PAIRS, 0)
    for k, (i, ok, v1, v2) in enumerate(zip(listed, *got)):
        f, o, b, _ = lay.table[i]
        where = "seed %d, entry %d: piece %d (file %d, offset %d, %d bytes, v1 length %d)" % (
            seed, k, i, f, o, b, lay.v1_len[i])
        assert (v1, v2) == (ok1[i], ok2[i]), where
        assert ok == (ok1[i] and ok2[i]), where
