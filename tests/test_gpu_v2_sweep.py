"""Differential sweep of the BitTorrent v2 kernels against hashlib (tests/v2_ref.py), bit-exact:

a. every exit position of hash_leaf's unrolled raw-block loop in its first and second pass (0 .. 7 raw blocks, each
   followed by one or two padded blocks) and the same edges at the far end of a leaf, in waves whose leaves all have
   one length (the table path, both lane mappings);
b. the same lengths in the last leaf of four-leaf pieces, so short lanes share a wave with full leaves;
c. the list kernel on both layouts;
d. every byte of the expected hash counts, through tv_v2_set_pieces + tv_v2_verify and through tv_v2_verify_list;
e. row offsets past 2^32 bytes: the leaf kernel, the untiled and the tiled list kernel, and tv_stage's linear offsets.

A wrong root must not pass for a detected corruption: every corrupted staging is also hashed (tv_v2_hash) and compared
with the reference roots of the corrupted bytes."""
import hashlib
import random

import pytest

from tests import synth, v2_ref
from tests.v2_util import set_bits

pytestmark = pytest.mark.gpu
K = 1024
LEAF = 16384

# 0 .. 7 raw blocks and the padding edges after them (39 lengths), then the edges at a leaf's far end (6)
NS = [64 * f + r for f in range(8) for r in (0, 1, 55, 56, 63) if 64 * f + r >= 1] + \
     [LEAF - 65, LEAF - 64, LEAF - 9, LEAF - 8, LEAF - 1, LEAF]
GROUP = 64                                                 # consecutive files of one length: a wave of the leaf kernel


@pytest.fixture(scope="module")
def ctx(native):
    if native.device_count() == 0:
        pytest.fail("no HIP device visible")
    with native.Context(0) as c:
        yield c


class Layout:
    """GROUP files of base + n bytes for every n of NS, each file one piece under piece length L; the staged bytes,
    the reference roots, and the same with the last valid byte of one piece per group flipped."""

    def __init__(self, L: int, base: int, seed: int):
        assert len(NS) == 45 and len(set(NS)) == 45
        self.L = L
        self.sizes = [base + n for n in NS for _ in range(GROUP)]
        self.P = len(self.sizes)
        table = v2_ref.piece_table(self.sizes, L)
        assert [(f, o, b) for f, o, b, w in table] == [(i, 0, s) for i, s in enumerate(self.sizes)]
        self.widths = [r[3] for r in table]
        blob = memoryview(bytes(synth.fill(seed, 0, sum(self.sizes))))
        self.files, o = [], 0
        for s in self.sizes:
            self.files.append(blob[o:o + s])
            o += s
        self.roots = [v2_ref.piece_root(f, w) for f, w in zip(self.files, self.widths)]
        # one piece of every group, at a lane that moves through the wave
        self.bad = [g * GROUP + (7 * g + 3) % GROUP for g in range(len(NS))]
        self.flipped = {}
        for i in self.bad:
            b = bytearray(self.files[i])
            b[-1] ^= 0x01
            self.flipped[i] = bytes(b)
        self.bad_roots = list(self.roots)
        for i in self.bad:
            self.bad_roots[i] = v2_ref.piece_root(self.flipped[i], self.widths[i])
            assert self.bad_roots[i] != self.roots[i]

    def stage(self, ctx, table: bool):
        total = (self.P - 1) * self.L + self.sizes[-1]
        ctx.set_layout(total, self.L, self.P)
        if table:
            ctx.v2_set_pieces(self.sizes, self.widths, b"".join(self.roots))
        ctx.stage_many([(i * self.L, f) for i, f in enumerate(self.files)])

    def stage_flipped(self, ctx):
        ctx.stage_many([(i * self.L, self.flipped[i]) for i in self.bad])


@pytest.fixture(scope="module")
def uniform():
    """a: L = 16 KiB, files of n bytes: every piece is one leaf, every wave 64 leaves of one length."""
    lay = Layout(16 * K, 0, 4100)
    assert lay.P == 2880 and set(lay.widths) == {1}
    assert lay.roots == [hashlib.sha256(f).digest() for f in lay.files]     # a one-leaf piece: the leaf is the root
    return lay


@pytest.fixture(scope="module")
def mixed():
    """b: L = 64 KiB, files of 3 x 16 KiB + n bytes: four-leaf pieces whose last leaf has n bytes."""
    lay = Layout(64 * K, 3 * LEAF, 4200)
    assert lay.P == 2880 and set(lay.widths) == {4} and max(lay.sizes) == 64 * K
    return lay


def test_length_list_reaches_every_exit_of_the_raw_loop():
    """(no GPU work) fast_end = n >> 6 of the uniform waves: 0 .. 7, 254, 255 and 256 blocks, every residue mod 3."""
    assert sorted({n >> 6 for n in NS}) == [0, 1, 2, 3, 4, 5, 6, 7, 254, 255, 256]
    assert {(n >> 6) % 3 for n in NS if n >> 6} == {0, 1, 2}
    assert {n % 64 for n in NS} == {0, 1, 55, 56, 63}


def _table_path(ctx, native, lay, mapping):
    ctx.set_option(native.TV_OPT_V2_MAP, mapping)
    try:
        lay.stage(ctx, table=True)
        roots, bits = ctx.v2_hash(), ctx.v2_verify()
        assert ctx.last_kernel()[0] == native.KERNEL_V2
        assert ctx.counter(native.TV_COUNTER_V2_MAP) == mapping
        lay.stage_flipped(ctx)
        bad_roots, bad_bits = ctx.v2_hash(), ctx.v2_verify()
    finally:
        ctx.set_option(native.TV_OPT_V2_MAP, 0)
    P = lay.P
    wrong = [(i, lay.sizes[i]) for i in range(P) if roots[32 * i:32 * i + 32] != lay.roots[i]]
    assert not wrong, wrong[:8]
    assert bits == set_bits(P)
    wrong = [(i, lay.sizes[i]) for i in range(P) if bad_roots[32 * i:32 * i + 32] != lay.bad_roots[i]]
    assert not wrong, wrong[:8]
    assert bad_bits == set_bits(P, clear=set(lay.bad))


@pytest.mark.parametrize("mapping", [1, 2])
def test_uniform_waves_table_path(ctx, native, uniform, mapping):
    _table_path(ctx, native, uniform, mapping)


@pytest.mark.parametrize("mapping", [1, 2])
def test_mixed_waves_table_path(ctx, native, mixed, mapping):
    _table_path(ctx, native, mixed, mapping)


@pytest.mark.parametrize("which", ["uniform", "mixed"])
def test_list_kernel_on_the_sweep_layouts(ctx, native, uniform, mixed, which):
    lay = uniform if which == "uniform" else mixed
    P = lay.P
    lay.stage(ctx, table=False)
    pieces = list(range(P))
    ok = ctx.v2_verify_list(pieces, lay.sizes, lay.widths, b"".join(lay.roots))
    assert ctx.last_kernel() == (native.KERNEL_V2_LIST, 1)
    assert ctx.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-P // (256 // lay.widths[0]))
    wrong = [(i, lay.sizes[i]) for i in range(P) if ok[i] != 1]
    assert not wrong, wrong[:8]
    lay.stage_flipped(ctx)
    ok = ctx.v2_verify_list(pieces, lay.sizes, lay.widths, b"".join(lay.roots))
    assert [i for i in range(P) if ok[i] != 1] == lay.bad
    assert ctx.last_kernel() == (native.KERNEL_V2_LIST, 1)
    # against the roots of the flipped bytes every entry passes: the flipped pieces were hashed, and hashed right
    ok = ctx.v2_verify_list(pieces, lay.sizes, lay.widths, b"".join(lay.bad_roots))
    assert list(ok) == [1] * P


# ---- d. every byte of the expected hash counts ---------------------------------------------------------------------------

def test_every_byte_of_the_expected_hash_counts(ctx, native):
    L = 64 * K
    sizes = [1000 + k for k in range(33)] + [3 * LEAF + 100 + k for k in range(33)]     # 33 one-leaf, 33 four-leaf
    files = [bytes(synth.fill(4300 + k, 0, s)) for k, s in enumerate(sizes)]
    table = v2_ref.piece_table(sizes, L)
    widths = [r[3] for r in table]
    assert widths == [1] * 33 + [4] * 33
    P = 66
    roots = [v2_ref.piece_root(f, w) for f, w in zip(files, widths)]
    want = []
    for i, r in enumerate(roots):
        k = i % 33
        h = bytearray(r)
        if k < 32:
            h[k] ^= 1 << (k % 8)                            # piece k of either kind: byte k of its expected hash
        want.append(bytes(h))
    ctx.set_layout((P - 1) * L + sizes[-1], L, P)
    ctx.v2_set_pieces(sizes, widths, b"".join(want))
    ctx.stage_many([(i * L, f) for i, f in enumerate(files)])
    assert ctx.v2_hash() == b"".join(roots)                # the data is right: only the expected hashes differ
    assert ctx.v2_verify() == set_bits(P, clear=set(range(P)) - {32, 65})
    pieces = list(range(P))
    ok = ctx.v2_verify_list(pieces, sizes, widths, b"".join(want))
    assert [i for i in pieces if ok[i]] == [32, 65]
    assert list(ctx.v2_verify_list(pieces, sizes, widths, b"".join(roots))) == [1] * P


# ---- e. row offsets past 2^32 bytes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,P", [(4 << 20, 1030), (32 << 20, 130)])
def test_rows_past_4_gib(native, L, P):
    """A resident shard of more than 2^32 bytes: the pieces on either side of the first row offset >= 2^32, the first
    and the last (short) piece are staged and checked; the others hold whatever the allocation held, and their results
    are masked (avail_bits) or not read."""
    W = L // LEAF
    last = L - 5
    total = (P - 1) * L + last
    nbytes = [L] * (P - 1) + [last]
    rng = random.Random(L)
    with native.Context(0) as c:
        c.set_layout(total, L, P)
        assert c.counter(native.TV_COUNTER_WINDOW_PIECES) == 0          # resident
        assert c.counter(native.TV_COUNTER_PAYLOAD_BYTES) > 1 << 32
        stride = L + c.get_option(native.TV_OPT_STRIDE_PAD)
        assert c.counter(native.TV_COUNTER_PAYLOAD_BYTES) == P * stride + 256   # (a new context: nothing reused)
        cross = -(-(1 << 32) // stride)                                  # the first piece whose row offset is >= 2^32
        assert 0 < cross - 1 and cross < P - 1
        assert (cross - 1) * stride < 1 << 32 <= cross * stride
        chosen = [0, cross - 1, cross, P - 1]
        datas = {i: bytes(synth.fill(4400, i * L, nbytes[i])) for i in chosen}
        roots = {i: v2_ref.piece_root(datas[i], W) for i in chosen}
        hashes = bytearray(rng.randbytes(32 * P))
        for i in chosen:
            hashes[32 * i:32 * i + 32] = roots[i]
        c.v2_set_pieces(nbytes, [W] * P, bytes(hashes))
        for i in chosen:
            c.stage(i * L, datas[i])
        avail = bytearray((P + 7) // 8)
        for i in chosen:
            avail[i >> 3] |= 0x80 >> (i & 7)
        got = c.v2_hash()
        assert [got[32 * i:32 * i + 32] == roots[i] for i in chosen] == [True] * 4
        assert c.v2_verify(bytes(avail)) == bytes(avail)
        order = [cross, 0, P - 1, cross - 1]

        def lst():
            ok = c.v2_verify_list(order, [nbytes[i] for i in order], [W] * 4, b"".join(roots[i] for i in order))
            assert c.last_kernel() == (native.KERNEL_V2_LIST, 1)
            assert c.counter(native.TV_COUNTER_LAST_WORKGROUPS) == -(-4 // max(1, 256 // W))
            return list(ok)

        assert lst() == [1, 1, 1, 1]
        # one byte of the crossing piece flipped: only its bit drops, and its root is the flipped bytes' root
        pos = L // 2 + 77
        bad = bytearray(datas[cross])
        bad[pos] ^= 0x20
        c.stage(cross * L + pos, bytes(bad[pos:pos + 1]))
        want = bytearray(avail)
        want[cross >> 3] &= ~(0x80 >> (cross & 7)) & 0xFF
        assert c.v2_verify(bytes(avail)) == bytes(want)
        got = c.v2_hash()
        bad_root = v2_ref.piece_root(bytes(bad), W)
        assert [got[32 * i:32 * i + 32] for i in chosen] == [roots[0], roots[cross - 1], bad_root, roots[P - 1]]
        assert lst() == [0, 1, 1, 1]
