"""CPU tests of the batch hosts' pure parts (torrent_amd/batch.py plan_batches, torrent_amd/_native.py batch_offsets):
how a list of torrents is cut into batches under a device budget, and where each torrent's bitfield lies in
tv_batch_verify's concatenated bitfields."""
import pytest

from torrent_amd import make_info, plan_batches
from torrent_amd._native import batch_offsets
from torrent_amd.batch import region_bytes

SLACK = 256     # bytes after a batch's last region


def test_plan_batches_around_the_budget():
    B = 10_000
    fit = B - SLACK                                     # an item exactly at the budget (its region and the slack)
    assert plan_batches([], B) == []
    assert plan_batches([fit], B) == [("batch", [0])]
    assert plan_batches([fit + 1], B) == [("single", [0])]            # one byte over: the single-torrent call
    assert plan_batches([fit, fit], B) == [("batch", [0]), ("batch", [1])]
    # a greedy fill in item order: the next item joins while the regions and the slack fit
    half = fit // 2
    assert plan_batches([half, half, 1, half], B) == [("batch", [0, 1]), ("batch", [2, 3])]
    assert plan_batches([half, fit - half], B) == [("batch", [0, 1])]
    assert plan_batches([half, fit - half + 1], B) == [("batch", [0]), ("batch", [1])]
    # an item over the budget splits the run it stands in; the items keep their order
    assert plan_batches([100, B, 100, 100], B) == [("batch", [0]), ("single", [1]), ("batch", [2, 3])]
    assert plan_batches([B, B], B) == [("single", [0]), ("single", [1])]
    # empty items (torrents without pieces) take no room and join the run they stand in
    assert plan_batches([0, fit, 0, 0, fit, 0], B) == [("batch", [0, 1, 2, 3]), ("batch", [4, 5])]
    assert plan_batches([0, 0], B) == [("batch", [0, 1])]
    # no budget: one batch
    for none in (None, 0):
        assert plan_batches([1 << 40, 5, 0], none) == [("batch", [0, 1, 2])]
        assert plan_batches([], none) == []


def test_plan_batches_covers_every_item_once_in_order():
    sizes = [(k * 7919) % 5000 for k in range(200)]
    for budget in (300, 1000, 5000, 20000):
        plan = plan_batches(sizes, budget)
        assert [k for _, ks in plan for k in ks] == list(range(len(sizes)))
        for kind, ks in plan:
            if kind == "single":
                assert len(ks) == 1 and sizes[ks[0]] + SLACK > budget
            else:
                assert sum(sizes[k] for k in ks) + SLACK <= budget
        # greedy: a batch's successor would not have fitted
        for (kind, ks), (kind2, ks2) in zip(plan, plan[1:]):
            if kind == kind2 == "batch":
                assert sum(sizes[k] for k in ks) + sizes[ks2[0]] + SLACK > budget


def test_region_bytes_is_the_library_layout():
    # n_pieces rows of round_up(L, 64) + 256 bytes, the region rounded up to 256
    info = make_info(100, bytes(20 * 70), "x", length=100 * 70)
    assert region_bytes(info) == -(-70 * (128 + 256) // 256) * 256
    info = make_info(16384, bytes(20 * 5), "x", length=4 * 16384 + 1)
    assert region_bytes(info) == 5 * (16384 + 256)
    assert region_bytes(make_info(16384, b"", "x", length=0)) == 0


@pytest.mark.parametrize("counts, offsets", [
    ([0], [0, 0]), ([1], [0, 1]), ([7], [0, 1]), ([8], [0, 1]), ([9], [0, 2]),
    ([0, 1, 7, 8, 9], [0, 0, 1, 2, 3, 5]), ([9, 0, 8, 0, 1], [0, 2, 2, 3, 3, 4]), ([], [0])])
def test_concatenated_bitfield_offsets(counts, offsets):
    assert batch_offsets(counts) == offsets
