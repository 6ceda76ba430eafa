"""The twin kernel's role-split rounds streams in the generator's emulator (CPU only).

tools/gen_sha1_asm.py gen_roles (the single block of the padded tail) and the two-block-trip loop
(roles_rounds_loop_text, executed block by block as roles_rounds_stream lays it out) run here on the two lanes of a
pair: DPP reads from the partner, role-masked writes, the LDS ring under the helper's protocol.  Random data and
random chaining values: a message of a random prefix, 1 .. 7 blocks through the stream under test, and its padding;
the prefix and the padding go through the plain compression below, and the digest must be hashlib's of the whole
message.  Then the distance rule for DPP reads on every stream, a mis-ordered stream that must trip it, the loop
text's block macro against the emulated block, the split kernel's rounds loop under the same helper protocol with a
stream that reads one barrier early and must trip it, and the committed header against the generator.
"""
import hashlib
import os
import random
import re
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_sha1_asm as g  # noqa: E402

H0 = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & g.M32


def _compress(h, block):
    w = list(struct.unpack(">16I", block))
    for t in range(16, 80):
        w.append(_rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = h
    for t in range(80):
        f = ((b & c) | (~b & d)) if t < 20 else ((b & c) | (b & d) | (c & d)) if 40 <= t < 60 else b ^ c ^ d
        a, b, c, d, e = (_rotl(a, 5) + (f & g.M32) + e + g.K[t // 20] + w[t]) & g.M32, a, _rotl(b, 30), c, d
    return [(x + y) & g.M32 for x, y in zip(h, (a, b, c, d, e))]


def _pad(msg):
    return msg + b"\x80" + b"\0" * ((55 - len(msg)) % 64) + struct.pack(">Q", 8 * len(msg))


def _blocks(data):
    return [data[i:i + 64] for i in range(0, len(data), 64)]


def _message(rng, nprefix, nmid, ntail_bytes):
    """-> (message, chaining value after its first nprefix blocks)."""
    msg = rng.randbytes(64 * (nprefix + nmid) + ntail_bytes)
    h = list(H0)
    for b in _blocks(msg[:64 * nprefix]):
        h = _compress(h, b)
    return msg, h


def _finish(h, msg, done_blocks):
    for b in _blocks(_pad(msg))[done_blocks:]:
        h = _compress(h, b)
    return struct.pack(">5I", *h)


def test_plain_compression_is_sha1():
    rng = random.Random(7)
    for n in (0, 55, 56, 64, 200):
        msg = rng.randbytes(n)
        assert _finish(list(H0), msg, 0) == hashlib.sha1(msg).digest()


def _single_block(h, block, piece_lanes=(2, 3)):
    """One block through the helper's twin layout and gen_roles, for the pair reading helper lanes piece_lanes."""
    addrs = [1024 + 16 * ln for ln in piece_lanes]
    hregs = []
    for ln in range(2):
        regs = {"sel": 0x00010203, "psel": (0x03020100, 0x07060504)[ln]}
        regs.update({f"k{i}": g.K[i] for i in range(4)})
        regs.update({f"raw{i}": int.from_bytes(block[4 * i:4 * i + 4], "little") for i in range(16)})
        hregs.append(regs)
    lds = {}
    g.emulate_twin(g.gen_helper2(), hregs, lds, addrs)
    regs2 = [{f"h{i}": h[i] for i in range(5)} for _ in range(2)]
    g.emulate_twin(g.gen_roles(0), regs2, lds, addrs)
    out = [[(h[i] + regs2[ln][f"r{i}"]) & g.M32 for i in range(5)] for ln in range(2)]
    assert out[0] == out[1], "the two roles return different states"
    return out[0]


@pytest.mark.parametrize("seed", range(6))
def test_single_block_with_random_chaining_values(seed):
    rng = random.Random(100 + seed)
    nprefix = rng.randrange(1, 4)
    msg, h = _message(rng, nprefix, 1, rng.randrange(0, 64))
    assert h != H0
    h = _single_block(h, msg[64 * nprefix:64 * nprefix + 64])
    assert _finish(h, msg, nprefix + 1) == hashlib.sha1(msg).digest()


@pytest.mark.parametrize("n", range(1, 8))
def test_loop_of_1_to_7_blocks(n):
    """Odd and even entry, every register set and ring buffer: the loop body is three pairs of blocks."""
    walk = g.twin_trips_walk(n)
    assert len(walk) == n and [buf for _, buf, _ in walk] == [k % 3 for k in range(n)]
    for seed in range(3):
        rng = random.Random(1000 * n + seed)
        nprefix = rng.randrange(0, 3)
        msg, h = _message(rng, nprefix, n, rng.randrange(0, 64))
        h = g.check_twin_stream(_blocks(msg[64 * nprefix:64 * (nprefix + n)]), h)
        assert _finish(h, msg, nprefix + n) == hashlib.sha1(msg).digest(), (n, seed)
    seen = {(s, buf) for m in range(1, 8) for s, buf, _ in g.twin_trips_walk(m)}
    assert seen == {(s, buf) for s in range(2) for buf in range(3)}


def test_instruction_counts():
    blk = g.gen_roles_trip_block(0, 0)
    valu = [op for op in blk if op[0].startswith("v_")]
    assert len(valu) == 40 * 9 + 1 + 6
    assert sum(op[0] == "ds_read_b128_abs" for op in blk) == 10 and sum(op[0] == "s_waitcnt_lgkm" for op in blk) == 1
    # the 4-byte instructions of a block: its wait, and the feed-forward's adds in two adjacent pairs
    small = [i for i, op in enumerate(blk) if op[0] in ("v_add_u32", "s_waitcnt_lgkm")]
    assert small[0] == 0 and len(small) == 5
    assert small[2] == small[1] + 1 and small[4] == small[3] + 1


def test_dpp_distance_on_every_stream():
    assert g.check_dpp_distance(g.gen_roles(0))
    for n in range(1, 10):     # (8 and 9 blocks go round the loop's back edge on either parity)
        ins = g.roles_rounds_stream(n)
        assert sum(g.dpp_source(op) is not None for op in ins) >= 3 * 40 * n
        assert g.check_dpp_distance(ins)


def test_loop_text_holds_the_block_once_as_a_macro():
    """The header's loop writes the block as an assembler macro of its K+W registers, the registers its reads fill
    and their offset; expanded with each call's arguments it is, line for line, the block the emulator ran."""
    text = g.roles_rounds_loop_text()
    lines = [l.replace("\\\\", "\\") for l in re.findall(r'"([^"]*)\\n"', text)]
    i, j = lines.index(".macro tv_roles_block_%= kw, rd, off"), lines.index(".endm")
    body = lines[i + 1:j]
    assert body == g.roles_block_macro() and len(body) == len(g.gen_roles_trip_block(0, 0))
    calls = [tuple(int(x) for x in l.split(None, 1)[1].split(",")) for l in lines if l.startswith("tv_roles_block_%= ")]
    plan = g.twin_trips_plan()
    want = [plan["pre"]] + plan["loop"]
    assert len(calls) == 7
    for (kw, rd, off), (s, _, nxt) in zip(calls, want):
        assert {kw, rd} == {64, 104} and kw == 64 + 40 * s and off == nxt * g.RING_BYTES
        assert g.expand_roles_block(body, kw, rd, off) == g._emit_lines(g.gen_roles_trip_block(s, off))
    # three partner reads per pair of rounds and one in the feed-forward, and the exit conversion's two
    assert sum("row_ror:8" in l for l in lines) == 3 * 40 + 1 + 2
    k = lines.index("L_rloop_%=:")
    assert not any(l.startswith("s_nop") for l in lines[k:lines.index("L_rdone_%=:")] + body)


def test_a_misordered_stream_trips_the_distance_check():
    blk = g.gen_roles_trip_block(0, 0)
    i = next(k for k, op in enumerate(blk) if op[0] == "v_add_u32_dpp")
    rol = blk[i][2]
    j = next(k for k, op in enumerate(blk) if op[0] == "v_alignbit_b32" and op[1] == rol)
    assert i - j - 1 == g.DPP_DISTANCE
    bad = blk[:j] + blk[j + 1:i] + [blk[j]] + blk[i:]      # rotl5 moved down, right before the DPP add that reads it
    assert sorted(map(str, bad)) == sorted(map(str, blk))
    with pytest.raises(AssertionError, match="DPP read"):
        g.check_dpp_distance(bad)
    # one instruction between is still one too few
    bad = blk[:j] + blk[j + 1:i - 1] + [blk[j], blk[i - 1]] + blk[i:]
    with pytest.raises(AssertionError, match="DPP read"):
        g.check_dpp_distance(bad)
    # and the first DPP read of a stream counts from the compiler's code before it
    with pytest.raises(AssertionError, match="DPP read"):
        g.check_dpp_distance([("v_mov_b32_dpp", "h0", "h1", ("own", g.ROLE0))])


@pytest.mark.parametrize("n", range(1, 8))
def test_split_loop_of_1_to_7_blocks(n):
    """The split kernel's rounds loop as shipped (one block per message block on buffers 0, 1, 2, 0, ...) under the
    same helper protocol, with random chaining values."""
    ins = g.split_rounds_stream(n)
    assert ins == [op for k in range(n) for op in g.split_rounds_block(k)] + [("s_waitcnt_lgkm", 0)]
    assert sum(op == ("s_barrier",) for op in ins) == n and sum(op[0] == "ds_read_b128" for op in ins) == 20 * n
    for seed in range(3):
        rng = random.Random(2000 * n + seed)
        nprefix = rng.randrange(0, 3)
        msg, h = _message(rng, nprefix, n, rng.randrange(0, 64))
        h = g.check_split_stream(_blocks(msg[64 * nprefix:64 * (nprefix + n)]), h)
        assert _finish(h, msg, nprefix + n) == hashlib.sha1(msg).digest(), (n, seed)


def _split_stream_with_block_2_read_early(barrier: int, wait: bool):
    """The three-block split stream with block 2's leading reads issued before the given barrier (0 or 1; its own
    place is after barrier 1), into register quads past the ring, and its first 60 rounds taking their words from
    there: nothing differs from the shipped stream but when those reads go out."""
    good, block2 = g.split_rounds_stream(3), g.split_rounds_block(2)
    start2 = len(good) - 1 - len(block2)
    assert good[start2:-1] == block2 and all(op[0] == "ds_read_b128" for op in block2[:g.READ_AHEAD])
    spare = 20
    early = [("ds_read_b128_abs", spare + q, off) for _, q, off in block2[:g.READ_AHEAD]]
    rest, t = [], 0
    for op in block2[g.READ_AHEAD:]:
        if op[0] == "v_add_u32" and op[1].startswith("r"):       # round t's `e + KW`
            if t < 4 * g.READ_AHEAD:
                assert op[2] == g.ring_reg(t // 4, t % 4)
                op = (op[0], op[1], f"v{g.RING_BASE + 4 * (spare + t // 4) + t % 4}", op[3])
            t += 1
        rest.append(op)
    assert t == 80
    at = [i for i, op in enumerate(good) if op == ("s_barrier",)][barrier]
    return good[:at] + early + ([("s_waitcnt_lgkm", 0)] if wait else []) + good[at:start2] + rest + good[-1:]


def test_a_read_one_barrier_early_trips_the_protocol_model():
    """Block k + 1 is in LDS before the barrier that starts block k, so a block may issue the next block's leading
    reads before its own closing barrier.  One barrier earlier is too early: block k + 2 is written at the barrier
    that ends block k at the latest, into the buffer handed back at the barrier before.  Such a stream trips the
    model: the in-flight assert when the reads cross that barrier, a wrong digest when they were waited for."""
    rng = random.Random(31)
    msg, h = _message(rng, 1, 3, 17)
    blocks, want = _blocks(msg[64:256]), hashlib.sha1(msg).digest()
    for wait in (False, True):       # one barrier ahead of the shipped place: allowed
        got = g.check_split_stream(blocks, h, _split_stream_with_block_2_read_early(1, wait))
        assert _finish(got, msg, 4) == want
    with pytest.raises(AssertionError, match="rewritten while a ds_read of it is in flight"):
        g.check_split_stream(blocks, h, _split_stream_with_block_2_read_early(0, False))
    got = g.check_split_stream(blocks, h, _split_stream_with_block_2_read_early(0, True))
    assert _finish(got, msg, 4) != want


def test_generated_headers_are_current():
    with open(os.path.join(ROOT, "torrent_amd", "csrc", "sha1_asm.h")) as f:
        h = f.read()
    assert h == g.render()
    assert not os.path.exists(os.path.join(ROOT, "torrent_amd", "csrc", "sha1_roles_asm.h"))
    assert re.findall(r"^__device__ __forceinline__ void (\w+)\(", h, re.M) == [
        "tv_sha1_full", "tv_sha1_lds", "tv_sha1_helper_loop", "tv_sha1_rounds_loop", "tv_sha1_schedule_lds",
        "tv_sha1_roles_lds", "tv_sha1_roles_rounds_loop", "tv_sha1_twin_helper_loop", "tv_sha1_twin_schedule_lds"]
