#!/usr/bin/env python3
"""Generate torrent_amd/csrc/sha1_asm.h: gfx950 inline-asm SHA-1 compression blocks.

Why generated asm: hipcc (ROCm 7.2) does not fold XOR3 / Maj into v_bitop3_b32 (one
compression compiles to ~790 VALU instead of ~613), and it pads every inline-asm boundary
with `s_nop 0`, which costs a full issue slot for a lone wave.  So each compression is ONE
asm statement, and this script emits it.  The emitted instruction stream is executed by the
emulator below against hashlib before the header is written (`--check`, also run by
tests/test_abi.py::test_asm_generator_emulator), so a wrong register rotation can never reach the GPU.

Blocks emitted
--------------
SHA1_FULL   one 64-byte block, message schedule computed in-asm (16-word rolling window).
            5 VALU per round + 3 per scheduled word = 400 + 192 = 592 (+16 v_perm bswap and
            5 feed-forward adds by the compiler outside) = 613 per block.
SHA1_LDS    the 80 rounds only (400 VALU); W[0..79] comes from LDS as 20 ds_read_b128
            (layout [t/4][lane][4 words], conflict-free), kept 15 quads ahead in an 80-VGPR
            ring of PHYSICAL registers (a 128-bit asm operand cannot be split in AMDGPU asm).
            The split kernel's rounds loop runs this block once per message block, its 15
            leading reads as a burst at the block's start (split_rounds_block; 3 LDS buffers,
            the helper two blocks ahead), checked by check_split_stream against the helper's
            protocol.

Round (roles rotate statically; the new `a` is written into the old `e` register):
    E  = v_add3_u32(E, K, W[t])          # off the critical path
    T0 = v_alignbit_b32(A, A, 27)        # rotl5(a)
    T1 = f(B, C, D)                      # v_bitop3_b32 0xCA (Ch) / 0x96 (Parity) / 0xE8 (Maj)
    B  = v_alignbit_b32(B, B, 2)         # rotl30(b)
    E  = v_add3_u32(E, T0, T1)           # new a
Chaining values H are read-only inputs: the first write to each working register goes to its
R output instead (no per-block v_mov), and the caller adds H += R afterwards.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import struct
import sys

K = [0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xCA62C1D6]
M32 = 0xFFFFFFFF

# physical VGPRs used by SHA1_LDS for its K+W ring (quad-aligned; a 128-bit asm operand cannot
# be split in AMDGPU asm).  The kernel's VGPR count is therefore >= RING_BASE + 4*RING_QUADS.
# A ds_read_b128 of a wave64 returns 1 KiB and its latency under the rounds wave's VALU stream is
# long: 15 quads in flight (60 rounds ahead, lgkmcnt's 4-bit maximum) run the 80-round block in
# 1,794 cycles against 1,894 with 7 in flight (tools/gen_ubench_rounds.py, profiles/r01/ubench_rounds.log).
RING_BASE = 64
# (the TV_GEN_* environment variables select build variants for A/B measurements; the defaults are
# the shipped configuration).  A TV_GEN_* name that is not one of these is an error, not a default build
# labelled as a variant.
SWITCHES = ("RING", "RA", "WAIT", "BUFS", "PAIRXOR", "ALIGN", "LALIGN", "HWAIT", "STAMP", "TWIN_RALIGN", "TWIN_HALIGN",
            "SPLIT_RALIGN", "SPLIT_HALIGN", "TWIN_TRIP_AT")
_unknown = sorted(k for k in os.environ if k.startswith("TV_GEN_") and k[len("TV_GEN_"):] not in SWITCHES)
if _unknown:
    raise ValueError("unknown generator switch in the environment: " + ", ".join(_unknown))
RING_QUADS = int(os.environ.get("TV_GEN_RING", "16"))   # register quads of the K+W ring
READ_AHEAD = int(os.environ.get("TV_GEN_RA", "15"))   # quads in flight ahead of the one being consumed
WAIT_EVERY = int(os.environ.get("TV_GEN_WAIT", "4"))    # one s_waitcnt per WAIT_EVERY quads
LDS_BUFS = int(os.environ.get("TV_GEN_BUFS", "3"))      # K+W buffers per pair; the helper runs LDS_BUFS-1 blocks ahead
# (The split rounds stream with its reads 15 quads ahead ACROSS block boundaries, or issued mid-block or after
# round 79, K added by the rounds wave, and the helper's schedule in pairs were measured slower or no faster
# and are no longer generated: profiles/design_history_r01-r05.md section 4.)
PAIR_XOR = os.environ.get("TV_GEN_PAIRXOR", "1") == "1"   # lane compression: schedule words two at a time
ALIGN_FULL = os.environ.get("TV_GEN_ALIGN", "1") == "1"   # lane compression block starts 8-byte aligned
# Diagnostic builds only (tools/split_stamps.py): STAMP = 1 brackets the split kernel's in-loop barriers (rounds and
# helper waves) with shader-clock reads into SGPRs s[88:91] and accumulates the cycles spent at them in an SGPR
# operand; the kernels then need -DTV_STAMPS=1.  The default header is unchanged.
# STAMP = 2 also brackets the helper's two waits per block: for its prefetched global words (vmcnt) and for its
# LDS writes before the barrier (lgkmcnt), into %[svm] and %[slg].
STAMP = int(os.environ.get("TV_GEN_STAMP", "0"))


def _stamped(line: str, acc: str) -> list:
    return ["s_memtime s[88:89]", line, "s_memtime s[90:91]", "s_waitcnt lgkmcnt(0)",
            "s_sub_u32 s90, s90, s88", f"s_add_u32 %[{acc}], %[{acc}], s90"]


STAMP_SEQ = _stamped("s_barrier", "sbar")
# Split helper: where it waits for its LDS writes.  "0": lgkmcnt(0) before every barrier (block m's writes done
# before barrier m - 1).  "mid": lgkmcnt(10) before the 11th write of block m + 1 instead -- block m is read
# only after barrier m, and the next block's first 10 writes (issued after block m's, LDS counts in order) may
# still be in flight; nothing waits at the barrier.
HELPER_WAIT = os.environ.get("TV_GEN_HWAIT", "mid")
LOOP_ALIGN = os.environ.get("TV_GEN_LALIGN", "1") == "1"  # split loops: .p2align 3 before every block body
HELPER_AHEAD = LDS_BUFS - 1
# physical VGPRs of the helper (schedule) block: 16-word W window, xor3 temp, 3 output quads
HW_BASE = 80
HT = 96
HT2 = 97   # (no instruction uses it; it stays in the clobber lists, which the register allocation depends on)
HOUT_BASE = 100
HOUT_QUADS = 3


def f_kind(t: int) -> str:
    if t < 20:
        return "ch"
    if t < 40 or t >= 60:
        return "par"
    return "maj"


class Regs:
    """Map logical state slots 0..4 to asm operand names with the first-write redirect."""

    def __init__(self):
        self.cur = [f"h{i}" for i in range(5)]

    def rd(self, s: int) -> str:
        return self.cur[s]

    def wr(self, s: int) -> str:
        self.cur[s] = f"r{s}"
        return self.cur[s]


def roles(t: int):
    m = t % 5
    return [(0 - m) % 5, (1 - m) % 5, (2 - m) % 5, (3 - m) % 5, (4 - m) % 5]


def _fop(t, dst, b, c, d):
    k = f_kind(t)
    # Ch as v_bitop3 0xCA, not v_bfi_b32: same 8-byte issue cost, but v_bitop3 runs at full rate on
    # the SIMD (2 cyc per wave64) and v_bfi at half rate (4 cyc; tools/ubench_simd.hip)
    return ("v_bitop3_b32", dst, b, c, d, {"ch": 0xCA, "par": 0x96}.get(k, 0xE8))


def gen_full():
    """SHA1_FULL instruction list. Operands: r0-4 (out), w0-15 (in/out), t0-3 (tmp),
    h0-4 (in), k0-3 (sgpr in).

    With PAIR_XOR the schedule words are computed two at a time (W[u], W[u+1] for even u, in round u-1)
    so that the two 4-byte v_xor_b32 of a pair sit next to each other: every other instruction of the
    block is an 8-byte VOP3, and an odd number of 4-byte instructions between them would leave every
    following VOP3 at an address = 4 mod 8.  A lone wave issues long runs of such misaligned 8-byte
    instructions at ~5.07 instead of 4.07 cycles (tools/ubench_align, profiles/r02/ubench_align.log); the
    block starts 8-byte aligned (".p2align 3" in the emitted text, ALIGN_FULL)."""
    ins = []
    R = Regs()
    for t in range(80):
        A, B, C, D, E = roles(t)
        wt = f"w{t & 15}"
        if PAIR_XOR:
            us = [t + 1, t + 2] if t % 2 == 1 and 15 <= t <= 77 else []   # pairs (16,17) .. (78,79)
            tmps = ["t2", "t3"]
            for i, u in enumerate(us):
                ins.append(("v_bitop3_b32", tmps[i], f"w{(u - 3) & 15}", f"w{(u - 8) & 15}", f"w{(u - 14) & 15}", 0x96))
            e_src = R.rd(E)
            ins.append(("v_add3_u32", R.wr(E), e_src, f"k{t // 20}", wt))
            ins.append(("v_alignbit_b32", "t0", R.rd(A), R.rd(A), 27))
            for i, u in enumerate(us):
                ins.append(("v_xor_b32", f"w{u & 15}", tmps[i], f"w{u & 15}"))
            ins.append(_fop(t, "t1", R.rd(B), R.rd(C), R.rd(D)))
            b_src = R.rd(B)
            ins.append(("v_alignbit_b32", R.wr(B), b_src, b_src, 2))
            for u in us:
                ins.append(("v_alignbit_b32", f"w{u & 15}", f"w{u & 15}", f"w{u & 15}", 31))
            ins.append(("v_add3_u32", R.rd(E), R.rd(E), "t0", "t1"))
            continue
        u = t + 1
        sched = 16 <= u < 80
        wu = f"w{u & 15}"
        if sched:
            ins.append(("v_bitop3_b32", "t2", f"w{(u - 3) & 15}", f"w{(u - 8) & 15}", f"w{(u - 14) & 15}", 0x96))
        e_src = R.rd(E)
        ins.append(("v_add3_u32", R.wr(E), e_src, f"k{t // 20}", wt))
        ins.append(("v_alignbit_b32", "t0", R.rd(A), R.rd(A), 27))
        if sched:
            ins.append(("v_xor_b32", wu, "t2", wu))
        ins.append(_fop(t, "t1", R.rd(B), R.rd(C), R.rd(D)))
        b_src = R.rd(B)
        ins.append(("v_alignbit_b32", R.wr(B), b_src, b_src, 2))
        if sched:
            ins.append(("v_alignbit_b32", wu, wu, wu, 31))
        ins.append(("v_add3_u32", R.rd(E), R.rd(E), "t0", "t1"))
    assert R.cur == [f"r{i}" for i in range(5)]
    return ins


def ring_reg(q: int, j: int) -> str:
    return f"v{RING_BASE + 4 * (q % RING_QUADS) + j}"


def gen_lds(off_base: int = 0, lead_wait: bool = True):
    """SHA1_LDS instruction list. Operands: r0-4 (out), t0-1 (tmp), h0-4 (in), addr (vgpr in).
    Quad g (K+W[4g..4g+3], K pre-added by the helper) is read from addr + off_base + g*1024."""
    ins = [("s_waitcnt_lgkm", 0)] if lead_wait else []
    issued = -1
    for g in range(min(READ_AHEAD, 20)):
        ins.append(("ds_read_b128", g, off_base + g * 1024))
        issued = g
    R = Regs()
    for t in range(80):
        g = t // 4
        if t % 4 == 0 and g % WAIT_EVERY == 0:
            need = min(g + WAIT_EVERY - 1, 19)          # quads consumed before the next wait
            ins.append(("s_waitcnt_lgkm", min(15, max(0, issued - need))))   # (lgkmcnt is 4 bits)
        A, B, C, D, E = roles(t)
        e_src = R.rd(E)
        ins.append(("v_add_u32", R.wr(E), ring_reg(g, t % 4), e_src))
        if t % 4 == 3 and g + READ_AHEAD < 20:
            ins.append(("ds_read_b128", g + READ_AHEAD, off_base + (g + READ_AHEAD) * 1024))
            issued = g + READ_AHEAD
        ins.append(("v_alignbit_b32", "t0", R.rd(A), R.rd(A), 27))
        ins.append(_fop(t, "t1", R.rd(B), R.rd(C), R.rd(D)))
        b_src = R.rd(B)
        ins.append(("v_alignbit_b32", R.wr(B), b_src, b_src, 2))
        ins.append(("v_add3_u32", R.rd(E), R.rd(E), "t0", "t1"))
    assert R.cur == [f"r{i}" for i in range(5)]
    return ins


def split_rounds_block(k: int):
    """Block k of the split kernel's rounds loop, as rounds_loop_text writes it and check_split_stream runs it:
    the 80 rounds on ring buffer k % LDS_BUFS with their own reads, 15 as a burst at the start (a burst landing
    while the wave waits costs fewer issue cycles than LDS data returning under the VALU stream), every read
    waited for inside the block; then h += r and the workgroup barrier."""
    return (gen_lds(k % LDS_BUFS * RING_BYTES, lead_wait=False)
            + [("v_add_u32", f"h{i}", f"h{i}", f"r{i}") for i in range(5)] + [("s_barrier",)])


def hw(t: int) -> str:
    return f"v{HW_BASE + (t & 15)}"


def gen_helper(src=None, off_base: int = 0):
    """Helper (schedule) block: src = 16 registers holding the block's words as loaded
    (little-endian; default operands raw0-15), sel (sgpr 0x00010203), addr (vgpr, LDS byte address
    of this lane in ring buffer 0), k0-3 (sgpr).  Writes K+W[t] for t = 0..79 to LDS at
    addr + off_base + (t/4)*1024 as [t/4][lane][4] (one ds_write_b128 per quad)."""
    if src is None:
        src = [f"raw{i}" for i in range(16)]
    ins = []
    for i in range(16):
        ins.append(("v_perm_b32", hw(i), 0, src[i], "sel"))
    for q in range(20):
        if q >= 4:
            for i in range(4):
                t = 4 * q + i
                ins.append(("v_bitop3_b32", f"v{HT}", hw(t - 3), hw(t - 8), hw(t - 14), 0x96))
                ins.append(("v_xor_b32", hw(t), f"v{HT}", hw(t)))
                ins.append(("v_alignbit_b32", hw(t), hw(t), hw(t), 31))
        o = HOUT_BASE + 4 * (q % HOUT_QUADS)
        for j in range(4):
            ins.append(("v_add_u32", f"v{o + j}", f"k{q // 5}", hw(4 * q + j)))
        ins.append(("ds_write_b128", o, off_base + q * 1024))
    return ins


# ---- TWIN: two lanes per piece, in the rounds waves AND the helper waves ----
# A twin workgroup is 2 rounds waves + 2 helper waves over 64 pieces.
# Helper (gen_helper2): lane 2i+b of helper wave w runs piece 32w+i and owns the schedule words of PARITY b.
# Both lanes expand W[16..31] with the standard recurrence, then keep their own parity (v_perm with a per-lane
# selector) and expand W[32..79] with W[t] = rotl2(W[t-6] ^ W[t-16] ^ W[t-28] ^ W[t-32]), whose terms all have
# t's parity: 192 VALU + 10 ds_write_b128 per block and lane instead of the split helper's 308 + 20.
# Buffer layout [k][wave][lane][4 words]: helper lane 2i+b of wave w holds W[8k+b], W[8k+b+2], W[8k+b+4],
# W[8k+b+6] (+K) of piece 32w+i at k*2048 + w*1024 + lane*16, written and read as one contiguous KiB per wave,
# so a rounds lane issues 10 ds_read_b128 per block where the split kernel's issues 20 (tools/gen_ubench_dpp.py,
# profiles/r02/ubench_dpp.log).
# Rounds: the two lanes of a piece divide every pair of rounds between them as ROLES (gen_roles,
# gen_roles_trip_block, further down); role b reads the words helper lane 2i+b wrote.  The loop over the full
# blocks runs in two-block trips on two register sets (next section), its 4-byte instructions in adjacent pairs
# and no s_nop.  The single block (gen_roles: the padded tail blocks) issues its own ten reads and has two
# waits, each followed by `s_nop 0`, so that its 8-byte instructions stay 8-byte aligned (a long misaligned
# run issues at ~5.07 instead of 4.07 cycles).
# The rounds the roles replaced -- both lanes of a pair running the same five 8-byte instructions per round,
# 405 VALU per block, lane t%2's K+W word through DPP quad_perm -- are no longer generated here;
# tools/gen_ubench_dpp.py writes them itself for `trips`, the comparator the roles were measured against
# (profiles/twin_roles/ubench_roles.log).
TWIN_READ_BYTES = 2048
# 64-byte placement of the twin loops: rounds loop head at (4 + 8 k) mod 64 for TV_GEN_TWIN_RALIGN = k, helper
# loop head at 4 m mod 64 for TV_GEN_TWIN_HALIGN = m ("none": wherever the code before them puts them).  The
# rounds loop at 4 mod 64 (and the helper's at 60) is 0.7-1.6 % faster at cfg2 than at 28, 52 or 60
# (profiles/r03/twin_ralign.jsonl: 11.89-11.91 vs 11.98-12.08 ms), so both are pinned there: a code change
# before the loops no longer moves them.
TWIN_RALIGN = os.environ.get("TV_GEN_TWIN_RALIGN", "0")
TWIN_HALIGN = os.environ.get("TV_GEN_TWIN_HALIGN", "15")
TWIN_RALIGN = None if TWIN_RALIGN == "none" else TWIN_RALIGN
TWIN_HALIGN = None if TWIN_HALIGN == "none" else TWIN_HALIGN
# the same for the split kernel's loops: rounds loop head at 8 k mod 64 (TV_GEN_SPLIT_RALIGN = k; its block
# bodies start with .p2align 3), helper loop head at 4 m mod 64 (TV_GEN_SPLIT_HALIGN = m).  At 25,600 pieces
# the rounds loop's eight placements are within 0.5 % of each other (profiles/r03/split_ralign.jsonl); k = 6
# (48 mod 64) was the fastest of the two rounds by 0.2 % and is pinned so that code changes cannot move it.
SPLIT_RALIGN = os.environ.get("TV_GEN_SPLIT_RALIGN", "6")
SPLIT_HALIGN = os.environ.get("TV_GEN_SPLIT_HALIGN")
SPLIT_RALIGN = None if SPLIT_RALIGN == "none" else SPLIT_RALIGN


# ---- TWIN rounds loop: two-block trips ----
# The loop body is two consecutive blocks on two register sets for the K+W quads (set 0 = ring quads 0-9,
# set 1 = quads 10-19: v[RING_BASE .. RING_BASE + 79]; the rounds wave has a SIMD to itself and the kernel's
# VGPR count is set by the helper's registers above them).  While a block runs on one set, the ten reads of
# the next block go out as ONE group into the other set, after round TWIN_TRIP_AT, so a block has one
# s_waitcnt -- lgkmcnt(0) before its round 0 -- and the loop counter and branch are paid once per two blocks:
# s_sub_u32 borrows when no pair is left, so there is no s_cmp.  Non-VALU issue slots per block: 10 reads +
# 1 wait + 1 barrier + (s_sub + s_cbranch) / 2 = 13.  The one-block loop this replaces (next block's reads
# 0-4 after a second wait at round 40 and 5-9 after round 79 into the same ten quads; s_sub, s_cmp and
# s_cbranch per block) had 16.  cfg2, interleaved with that loop (profiles/twin_trips/): kernel 11.88-11.92 ->
# 11.76-11.79 ms, 1,732 -> 1,713 cycles per block.
# Where the reads go out (TV_GEN_TWIN_TRIP_AT, cfg2 kernel ms against 11.84 for the one-block loop,
# profiles/twin_trips/read_placement.jsonl): after round 9 11.72, 19 11.70, 29 11.73, 39 11.73, 49 11.72,
# 59 11.70, 69 11.77 (too late: the last reads are not back at the block's end).  19 leaves them 60 rounds.
TWIN_TRIP_AT = int(os.environ.get("TV_GEN_TWIN_TRIP_AT", "19"))   # the next block's reads follow this round
TWIN_SET_QUADS = 10


def twin_set_reg(s: int, k: int, j: int) -> str:
    return f"v{RING_BASE + 4 * (TWIN_SET_QUADS * s + k) + j}"


def twin_trips_plan():
    """Block parameters (register set, own buffer, next buffer) of the two-block-trip loop.  The loop body is
    lcm(2 sets, LDS_BUFS buffers) = 6 blocks: the pairs (0,1) (2,0) (1,2) on sets (0,1), with an exit test after
    each pair.  An odd block count runs `pre` first -- one block on set 1 and buffer 0 -- and enters the
    loop at the pair that starts on buffer 1 (pair index `odd_entry`)."""
    assert LDS_BUFS == 3
    loop = [(i % 2, i % LDS_BUFS, (i + 1) % LDS_BUFS) for i in range(2 * LDS_BUFS)]
    odd_entry = next(p for p in range(LDS_BUFS) if loop[2 * p][1] == 1)
    assert odd_entry > 0
    return {"pre": (1, 0, 1), "loop": loop, "odd_entry": odd_entry}


def twin_trips_walk(nsteps: int):
    """The blocks the loop text executes for nsteps blocks, in order, following its scalar control flow:
    [(register set, buffer, next buffer)]; the first entry's set and buffer are the prologue's."""
    plan = twin_trips_plan()
    out, cnt = [], nsteps >> 1
    if nsteps & 1:
        out.append(plan["pre"])
        if cnt == 0:             # s_sub_u32 cnt, cnt, 1 borrows: L_rdone
            return out
        cnt -= 1
        pair = plan["odd_entry"]
    else:
        cnt -= 1
        pair = 0
    while True:
        out += plan["loop"][2 * pair:2 * pair + 2]
        if cnt == 0:             # the pair's s_sub_u32 borrows: L_rdone
            return out
        cnt -= 1
        pair = (pair + 1) % LDS_BUFS


# ---- TWIN: role-split rounds, 4.5 instructions per round ----
# A lone wave issues one instruction per ~4.07 cycles whatever its kind, dependent or not, so the rounds wave's time
# is its instruction count.  The two lanes of a pair therefore do not run the same rounds: of each two rounds t, t+1
# (a PAIR of rounds), role 0 computes round t and role 1 round t+1.  In a rounds wave the roles of a piece sit 8
# lanes apart in a row of 16: lane 16r+p (p < 8) is role 0 of the wave's piece 8r+p, lane 16r+8+p its role 1; the
# partner is reached with DPP row_ror:8 (a swap), and bank_mask 0x3 / 0xc writes only the role-0 / role-1 lanes.
# With a_k = `a` before round k (a_0 = h0, a_-1 = h1, R a_-2 = h2, ...), R = rotl30, registers as (role 0 | role 1),
# the state at the start of the pair of rounds t, t+1 is
#     W = (a_t-1 | a_t)   C = (R a_t-2 | R a_t-1)   D = (R a_t-3 | R a_t-2)   E = (R a_t-4 | R a_t-3)
# and KW = (K+W_t | K+W_t+1) is each role's own word of the quad it read (role b reads helper lane 2i+b).  Nine
# instructions, in an order that keeps two instructions between a VALU write and a DPP read of the register:
#     1 ROL  = rotl5(W)                          6 Dn  = rotr7(ROL) = R(W at 1): the next D
#     2 F    = f(W, C, D)                        7 T   = W[partner]              (a_t | a_t+1)
#     3 G    = F + E + KW                        8 W[role 1] = ROL2[partner] + G (a_t+1 | a_t+2)
#     4 W[role 0] = ROL[partner] + G             9 Cn  = R(T): the next C; the next E is this C
#     5 ROL2 = rotl5(W)      (a_t+1 | a_t)
# F and `F + e + KW` serve both rounds at once; the serial part, rotl5 and add twice, passes between the roles.
# Both rounds of a pair fall in one 20-round group.  40 x 9 + 1 copy + 6 feed-forward = 367 VALU per block, where
# the rounds both lanes ran alike took 405.
# The chaining value stays in this form across the blocks of the loop: HW = (h1 | h0), HC = (h2 | R h1),
# HD = (h3 | h2), HE = (h4 | h3) in %[h0..h3]; the first pair reads them in place (only W is copied, step 4
# overwrites half of it), and the feed-forward is one add each, plus R(new HW) of role 0 moved into role 1 of HC.
# Both generated functions convert from and to the plain h[5] in both lanes, once per call.
ROLE0, ROLE1, BOTH = 0x3, 0xC, 0xF    # DPP bank_mask: the lanes an instruction writes
DPP_DISTANCE = 2                      # instructions between a VALU write of a register and a DPP read of it


def dpp_source(op):
    """The register an instruction reads from another lane (or its own) through DPP, or None."""
    return op[2] if op[0] in ("v_add_u32_dpp", "v_mov_b32_dpp") else None


def check_dpp_distance(ins):
    """Every DPP read in the instruction list (executed in order) is DPP_DISTANCE or more instructions after the
    last VALU write of its source; inline asm gets no hazard padding.  A register the list has not written yet
    counts as written just before its first instruction (the compiler's code, which knows of no DPP here)."""
    last = {}
    for i, op in enumerate(ins):
        src = dpp_source(op)
        if src is not None:
            gap = i - last.get(src, -1) - 1
            assert gap >= DPP_DISTANCE, f"DPP read of {src} {gap} instructions after its write (instruction {i}: {op})"
        if op[0].startswith("v_"):
            last[op[1]] = i
    return True


def _role_pairs(ins, chain, kw, reads_after=None):
    """Append the 40 pairs of rounds of one block to ins.  chain = (W, C, D, E): the registers pair 0 reads its
    state from (read-only when they are the loop's chaining registers %[h0..h3]; the tail block passes working
    registers).  kw(j) = the register holding pair j's K+W word.  reads_after = (pair index, instructions) to
    insert after that pair.  Working registers: W = r0, D = r1, G = r2, and r3, r4, t0 taken in turn for
    C / E / ROL.  Returns the registers of the final (W, C, D, E)."""
    W, D, G = "r0", "r1", "r2"
    free = [x for x in ("r3", "r4", "t0") if x not in chain]
    pool = {"r3", "r4", "t0"}
    w_rd, C, d_rd, E = chain
    if w_rd != W:
        ins.append(("v_mov_b32", W, w_rd))
    for j in range(40):
        rol = free.pop(0)
        ins.append(("v_alignbit_b32", rol, w_rd, w_rd, 27))                       # 1
        ins.append(_fop(2 * j, G, w_rd, C, d_rd))                                 # 2
        ins.append(("v_add3_u32", G, G, E, kw(j)))                                # 3
        if E in pool:
            free.append(E)
        ins.append(("v_add_u32_dpp", W, rol, G, ("ror8", ROLE0)))                 # 4
        rol2 = free.pop(0)
        ins.append(("v_alignbit_b32", rol2, W, W, 27))                            # 5
        ins.append(("v_alignbit_b32", D, rol, rol, 7))                            # 6
        ins.append(("v_mov_b32_dpp", rol, W, ("ror8", BOTH)))                     # 7
        ins.append(("v_add_u32_dpp", W, rol2, G, ("ror8", ROLE1)))                # 8
        ins.append(("v_alignbit_b32", rol, rol, rol, 2))                          # 9
        free.append(rol2)
        w_rd, C, d_rd, E = W, rol, D, C
        if reads_after is not None and reads_after[0] == j:
            ins += reads_after[1]
    return W, C, D, E


def gen_roles(off_base: int = 0):
    """One role-split TWIN rounds block with its own 10 reads issued first (tv_sha1_roles_lds: the padded tail
    blocks).  Operands as gen_lds: r0-4 (out), t0-1 (tmp), h0-4 (in, the plain chaining value in both lanes), addr
    (this lane's LDS byte address).  r = the plain state after round 79 in both lanes.  Two waits, before pair 0
    (reads 0-4) and pair 20 (reads 5-9), each with an s_nop that keeps the 8-byte instructions aligned."""
    ins = [("ds_read_b128", k, off_base + k * TWIN_READ_BYTES) for k in range(10)]
    # W = (h1 | h0), C = (h2 | R h1), D = (h3 | h2), E = (h4 | h3) in working registers
    ins += [("v_mov_b32", "r0", "h0"), ("v_mov_b32_dpp", "r0", "h1", ("own", ROLE0)),
            ("v_alignbit_b32", "r3", "h1", "h1", 2), ("v_mov_b32_dpp", "r3", "h2", ("own", ROLE0)),
            ("v_mov_b32", "r1", "h2"), ("v_mov_b32_dpp", "r1", "h3", ("own", ROLE0)),
            ("v_mov_b32", "r4", "h3"), ("v_mov_b32_dpp", "r4", "h4", ("own", ROLE0)),
            ("s_waitcnt_lgkm", 5), ("s_nop",)]
    W, C, D, E = _role_pairs(ins, ("r0", "r3", "r1", "r4"), lambda j: ring_reg(j // 4, j % 4),
                             reads_after=(19, [("s_waitcnt_lgkm", 0), ("s_nop",)]))
    # final W = (a79 | a80), C = (R a78 | R a79), D = (R a77 | R a78), E = (R a76 | R a77)  ->  plain r0..r4
    assert (W, C, D, E) == ("r0", "t0", "r1", "r3"), (W, C, D, E)
    ins += [("v_mov_b32", "r2", C), ("v_mov_b32_dpp", "r2", D, ("own", ROLE1)),      # r2 = R a78
            ("v_mov_b32_dpp", "t1", W, ("ror8", BOTH)),                              # t1 = (a80 | a79)
            ("v_mov_b32_dpp", "r4", E, ("ror8", BOTH)),
            ("v_mov_b32_dpp", "r4", E, ("own", ROLE0)),                              # r4 = R a76
            ("v_mov_b32_dpp", "r3", D, ("own", ROLE0)),                              # r3 = R a77 (E's register)
            ("v_mov_b32", "r1", W), ("v_mov_b32_dpp", "r1", "t1", ("own", ROLE1)),   # r1 = a79
            ("v_mov_b32_dpp", "r0", "t1", ("own", ROLE0))]                           # r0 = a80
    check_dpp_distance(ins)
    return ins


def gen_roles_trip_block(s: int, off_next: int):
    """One block of the two-block-trip TWIN rounds loop on register set s, chaining registers %[h0..h3] in the
    role-split form, feed-forward included (the caller adds the barrier).  On entry this block's ten reads
    (issued by the previous block, or the prologue) are the only LDS operations in flight; its single wait retires
    them.  After the pair of rounds holding TWIN_TRIP_AT it issues the ten reads of the next block (buffer at
    off_next) into the other set, whose last use was the previous block's final pair.
    The feed-forward's four adds are 4-byte instructions, in two adjacent pairs; the barrier and the next block's
    wait (or the trip's s_sub and s_cbranch) are a third pair, so every 8-byte instruction stays at 0 mod 8."""
    ins = [("s_waitcnt_lgkm", 0)]
    reads = [("ds_read_b128_abs", TWIN_SET_QUADS * (1 - s) + q, off_next + q * TWIN_READ_BYTES)
             for q in range(TWIN_SET_QUADS)]
    W, C, D, E = _role_pairs(ins, ("h0", "h1", "h2", "h3"), lambda j: twin_set_reg(s, j // 4, j % 4),
                             reads_after=(TWIN_TRIP_AT // 2, reads))
    ins += [("v_add_u32", "h0", "h0", W), ("v_add_u32", "h2", "h2", D),
            ("v_alignbit_b32", "t1", "h0", "h0", 2),              # role 0: R(new h1), for role 1 of HC
            ("v_add_u32", "h3", "h3", E), ("v_add_u32", "h1", "h1", C),
            ("v_mov_b32_dpp", "h1", "t1", ("ror8", ROLE1))]
    return ins


def roles_loop_entry():
    """Plain h0..h4 in both lanes -> HW, HC, HD, HE in %[h0..h3] (%[h4] is then unused), around the loop's three
    leading scalar instructions, which stand between the compiler's last write of h and the first DPP read."""
    return [("v_alignbit_b32", "t1", "h1", "h1", 2),
            ("s_waitcnt_lgkm", 0), ("s_text", "s_lshr_b32 %[cnt], %[nsteps], 1"), ("s_text", "s_bitcmp1_b32 %[nsteps], 0"),
            ("v_mov_b32_dpp", "h0", "h1", ("own", ROLE0)), ("v_mov_b32_dpp", "h1", "h2", ("own", ROLE0)),
            ("v_mov_b32_dpp", "h2", "h3", ("own", ROLE0)), ("v_mov_b32_dpp", "h3", "h4", ("own", ROLE0)),
            ("v_mov_b32_dpp", "h1", "t1", ("own", ROLE1))]


def roles_loop_exit():
    """HW, HC, HD, HE -> the plain h0..h4 in both lanes (after the loop's closing wait)."""
    return [("s_waitcnt_lgkm", 0),
            ("v_mov_b32_dpp", "t1", "h0", ("ror8", BOTH)),        # (h0 | h1)
            ("v_mov_b32_dpp", "h4", "h3", ("ror8", BOTH)), ("v_mov_b32_dpp", "h4", "h3", ("own", ROLE0)),
            ("v_mov_b32_dpp", "h3", "h2", ("own", ROLE0)), ("v_mov_b32_dpp", "h2", "h1", ("own", ROLE0)),
            ("v_mov_b32_dpp", "h1", "h0", ("own", ROLE0)), ("v_mov_b32_dpp", "h1", "t1", ("own", ROLE1)),
            ("v_mov_b32_dpp", "h0", "t1", ("own", ROLE0))]


def roles_rounds_stream(nsteps: int):
    """The instructions roles_rounds_loop_text executes for nsteps blocks, in order (twin_trips_walk), for the
    emulator and the DPP-distance check: entry conversion, prologue reads, the blocks with their barriers, exit
    conversion.  The s_sub / s_cbranch / s_branch between trips are left out, which only shortens distances."""
    walk = twin_trips_walk(nsteps)   # the blocks in the order the loop text's control flow runs them
    assert [buf for _, buf, _ in walk] == [k % LDS_BUFS for k in range(nsteps)]
    ins = roles_loop_entry()
    ins += [("ds_read_b128_abs", TWIN_SET_QUADS * walk[0][0] + q, q * TWIN_READ_BYTES) for q in range(TWIN_SET_QUADS)]
    for k, (s, _, nxt) in enumerate(walk):
        assert k == 0 or (walk[k - 1][0] != s and walk[k - 1][2] == walk[k][1])   # the reads the block before issued
        ins += gen_roles_trip_block(s, nxt * RING_BYTES) + [("s_barrier",)]
    return ins + roles_loop_exit()


def _roles_block_lines(s: int, nxt: int):
    return _emit_lines(gen_roles_trip_block(s, nxt * RING_BYTES))


def _set_base(s: int) -> int:
    return RING_BASE + 4 * TWIN_SET_QUADS * s


def roles_block_macro():
    """The body of the assembler macro `kw, rd, off` that stands for a block of the loop: the block on register set 0
    with its K+W registers written v[\\kw+i], the registers its reads fill v[\\rd+i:\\rd+j] and their offsets
    \\off+n.  The seven blocks of the loop text differ in nothing else, so the header holds the block once."""
    kw0, rd0, off = _set_base(0), _set_base(1), RING_BYTES
    body = []
    for l in _roles_block_lines(0, 1):
        m = re.match(r"ds_read_b128 v\[(\d+):(\d+)\], (\S+) offset:(\d+)$", l)
        if m:
            lo, hi, n = int(m.group(1)), int(m.group(2)), int(m.group(4))
            body.append(f"ds_read_b128 v[\\rd+{lo - rd0}:\\rd+{hi - rd0}], {m.group(3)} offset:\\off+{n - off}")
        else:
            body.append(re.sub(r"\bv(\d+)\b", lambda m: f"v[\\kw+{int(m.group(1)) - kw0}]", l))
    return body


def expand_roles_block(body, kw: int, rd: int, off: int):
    """What the assembler makes of the macro for these arguments, as the lines _emit_lines would have written."""
    out = []
    for l in body:
        l = re.sub(r"v\[\\rd\+(\d+):\\rd\+(\d+)\]", lambda m: f"v[{rd + int(m.group(1))}:{rd + int(m.group(2))}]", l)
        l = re.sub(r"v\[\\kw\+(\d+)\]", lambda m: f"v{kw + int(m.group(1))}", l)
        out.append(re.sub(r"offset:\\off\+(\d+)", lambda m: f"offset:{off + int(m.group(1))}", l))
    return out


def roles_rounds_loop_text() -> str:
    """The TWIN rounds wave over nsteps (>= 1) blocks from ring buffer 0 in two-block trips (twin_trips_plan), with
    gen_roles_trip_block as the block (written once, as a macro, and checked here to expand to every block's own
    lines) between the entry and exit conversions of the chaining value.
    LDS ordering, with the helper two blocks ahead: block j + 1 was written before the barrier that started
    block j, so block j may read it at any round; and the lgkmcnt(0) that starts block j + 1 retires those
    reads of buffer (j + 1) % 3 before the barrier that ends block j + 1, after which the helper may rewrite
    that buffer.  No read is in flight across more than one barrier.  The reads the final block issues (of the
    helper's spare block) are drained at L_rdone."""
    plan = twin_trips_plan()
    body = roles_block_macro()
    assert all("\\" not in l for l in _roles_block_lines(0, 1))

    def prologue(s):
        return _emit_lines([("ds_read_b128_abs", TWIN_SET_QUADS * s + q, q * TWIN_READ_BYTES)
                            for q in range(TWIN_SET_QUADS)])

    def block(s, nxt):
        # 4-byte instructions only in adjacent pairs (gen_roles_trip_block): every 8-byte instruction sits at
        # 0 mod 8 and the loop needs no s_nop
        args = (_set_base(s), _set_base(1 - s), nxt * RING_BYTES)
        assert expand_roles_block(body, *args) == _roles_block_lines(s, nxt), (s, nxt)
        return ["tv_roles_block_%= {}, {}, {}".format(*args)] + (STAMP_SEQ if STAMP else ["s_barrier"])

    L = [".macro tv_roles_block_%= kw, rd, off"] + body + [".endm"]
    L += _emit_lines(roles_loop_entry()) + ["s_cbranch_scc1 L_rodd_%="]
    L += prologue(0) + ["s_sub_u32 %[cnt], %[cnt], 1", "s_branch L_rloop_%="]
    # odd block count: one single-block trip on set 1, then into the loop at the pair starting on buffer 1
    s, _, nxt = plan["pre"]
    L += ["L_rodd_%=:"] + prologue(s) + [".p2align 3", "s_nop 0"] + block(s, nxt)
    L += ["s_sub_u32 %[cnt], %[cnt], 1", "s_cbranch_scc1 L_rdone_%=", f"s_branch L_rpair{plan['odd_entry']}_%="]
    if TWIN_RALIGN is not None:
        L += [".p2align 6"] + ["s_nop 0"] * (1 + 2 * int(TWIN_RALIGN))
    else:
        L += [".p2align 3", "s_nop 0"]
    L.append("L_rloop_%=:")
    for p in range(LDS_BUFS):
        if p:
            L.append(f"L_rpair{p}_%=:")
        for s, _, nxt in plan["loop"][2 * p:2 * p + 2]:
            L += block(s, nxt)
        L += ["s_sub_u32 %[cnt], %[cnt], 1",
              "s_cbranch_scc1 L_rdone_%=" if p < LDS_BUFS - 1 else "s_cbranch_scc0 L_rloop_%="]
    L += ["L_rdone_%=:"] + _emit_lines(roles_loop_exit())
    if TWIN_RALIGN is not None:
        # the statement ends at 8 mod 64 whatever its length: the code that follows (the loop over the padded
        # tail blocks) keeps its 64-byte placement
        L += [".p2align 6", "s_nop 0", "s_nop 0"]
    return "\n".join('    "{}\\n"'.format(l.replace("\\", "\\\\")) for l in L)


def rounds_loop_text() -> str:
    """The split kernel's rounds wave over nsteps (>= 1) blocks in which every lane updates, starting
    at ring buffer 0: split_rounds_block on buffers 0, 1, 2, 0, ... -- 80 rounds from K+W in LDS, h += r,
    barrier per block.  One asm statement, so no compiler bookkeeping or asm-boundary s_nop between
    blocks."""
    L = ["s_waitcnt lgkmcnt(0)", "s_mov_b32 %[cnt], %[nsteps]"]
    if SPLIT_RALIGN is not None:
        L.append(".p2align 6")
        L.extend(["s_nop 0"] * (2 * int(SPLIT_RALIGN)))
    L.append("L_rloop_%=:")
    for k in range(LDS_BUFS):
        if LOOP_ALIGN:
            L.append(".p2align 3")
        block = split_rounds_block(k)
        assert block[-1] == ("s_barrier",)   # (every LDS read of the block has been waited for)
        L.extend(_emit_lines(block[:-1]))
        L.extend(STAMP_SEQ if STAMP else ["s_barrier"])
        L += ["s_sub_u32 %[cnt], %[cnt], 1", "s_cmp_eq_u32 %[cnt], 0",
              "s_cbranch_scc1 L_rdone_%=" if k < LDS_BUFS - 1 else "s_cbranch_scc0 L_rloop_%="]
    L += ["L_rdone_%=:", "s_waitcnt lgkmcnt(0)"]
    return "\n".join(f'    "{l}\\n"' for l in L)


H2_F, H2_P, H2_T, H2_O = 160, 192, 232, 236   # helper2 physical VGPRs: W[0..31], own-parity P[0..39], tmp, 3 out quads


def gen_helper2(src=None, off_base: int = 0):
    """TWIN helper block for a lane pair: src = the 16 registers holding the block's words as loaded
    (little-endian; default raw0-15, identical in both lanes), sel (sgpr 0x00010203), psel (vgpr: 0x03020100 in
    lane 0, 0x07060504 in lane 1 of each pair), addr (vgpr, this lane's LDS byte address), k0-3 (sgpr).  Lane b
    writes K+W[8k+b+2i] (i = 0..3) to addr + off_base + k*2048 for k = 0..9."""
    if src is None:
        src = [f"raw{i}" for i in range(16)]
    F = lambda t: f"v{H2_F + t}"      # noqa: E731  W[t], t < 32 (both parities)
    P = lambda j: f"v{H2_P + j}"      # noqa: E731  W[2j + b]
    T = f"v{H2_T}"
    ins = []
    nq = [0]

    def quad(k):   # K+W of own-parity words 4k..4k+3 -> LDS
        o = H2_O + 4 * (nq[0] % 3)
        nq[0] += 1
        for i in range(4):
            ins.append(("v_add_u32", f"v{o + i}", f"k{(4 * k + i) // 10}", P(4 * k + i)))
        ins.append(("ds_write_b128", o, off_base + k * TWIN_READ_BYTES))

    for i in range(16):
        ins.append(("v_perm_b32", F(i), 0, src[i], "sel"))
    for t in range(16, 32):
        ins.append(("v_bitop3_b32", T, F(t - 3), F(t - 8), F(t - 14), 0x96))
        ins.append(("v_xor_b32", F(t), T, F(t - 16)))
        ins.append(("v_alignbit_b32", F(t), F(t), F(t), 31))
    for j in range(16):
        ins.append(("v_perm_b32", P(j), F(2 * j + 1), F(2 * j), "psel"))
        if j % 4 == 3:
            quad(j // 4)
    for j in range(16, 40):
        ins.append(("v_bitop3_b32", T, P(j - 3), P(j - 8), P(j - 14), 0x96))
        ins.append(("v_xor_b32", P(j), T, P(j - 16)))
        ins.append(("v_alignbit_b32", P(j), P(j), P(j), 30))
        if j % 4 == 3:
            quad(j // 4)
    return ins


P0_BASE, P1_BASE, VL = 112, 128, 144   # prefetch buffers (2 blocks) and the running load pointer
RING_BYTES = 80 * 64 * 4               # one K+W buffer (also used by rounds_loop_text)


def helper_loop_text(twin: bool = False) -> str:
    """The helper wave's steady state as ONE asm statement (text, not emulated: its body is
    gen_helper, which the emulator checks).  For each raw block: wait for its prefetched words,
    byte-swap them, issue the loads 2 blocks ahead into the freed registers, expand the schedule,
    write K+W to LDS, barrier.  Loads land in physical registers the compiler never sees, so no
    compiler copy can touch an in-flight register and no compiler wait drains the prefetch."""
    L = []

    def loads(base):
        for q in range(4):
            L.append(f"global_load_dwordx4 v[{base + 4 * q}:{base + 4 * q + 3}], v[{VL}:{VL + 1}], off offset:{16 * q}")

    def advance():
        L.append("s_cmp_gt_u32 %[adv], 0")
        L.append("s_cselect_b64 %[inc], 64, 0")
        L.append("s_subb_u32 %[adv], %[adv], 0")
        L.append(f"v_lshl_add_u64 v[{VL}:{VL + 1}], v[{VL}:{VL + 1}], 0, %[inc]")

    def step(pbase, off_base, barrier=True):
        L.extend(_stamped("s_waitcnt vmcnt(4)", "svm") if STAMP >= 2 else ["s_waitcnt vmcnt(4)"])
        body = (gen_helper2 if twin else gen_helper)([f"v{pbase + i}" for i in range(16)], off_base)
        perms, rest = body[:16], body[16:]
        if LOOP_ALIGN:
            L.append(".p2align 3")
        L.extend(_emit_lines(perms))
        loads(pbase)    # the perms have read pbase: refill it with the block 2 ahead
        advance()
        if LOOP_ALIGN:
            L.append(".p2align 3")
        if HELPER_WAIT == "mid" and not twin:
            assert HELPER_AHEAD >= 2
            k = [i for i, op in enumerate(rest) if op[0] == "ds_write_b128"][10]
            rest = rest[:k] + [("s_waitcnt_lgkm", 10)] + rest[k:]
        L.extend(_emit_lines(rest))
        if barrier and HELPER_WAIT == "mid" and not twin:
            L.extend(STAMP_SEQ if STAMP else ["s_barrier"])
        elif barrier:
            L.extend(_stamped("s_waitcnt lgkmcnt(0)", "slg") if STAMP >= 2 else ["s_waitcnt lgkmcnt(0)"])
            L.extend(STAMP_SEQ if STAMP else ["s_barrier"])

    L.append("s_sub_u32 %[adv], %[nraw], 1")
    L.append(f"v_mov_b64 v[{VL}:{VL + 1}], %[va]")
    loads(P0_BASE)
    advance()
    loads(P1_BASE)
    advance()
    # block 0 into buffer 0; with the helper A = HELPER_AHEAD blocks ahead no barrier follows its first A - 1
    # writes: its first barrier (the rounds wave's starting one) follows the write of block A - 1, and block m
    # (m >= A - 1) is followed by barrier m - A + 2 -- the C++ tail's rule (b - b0 + 1 >= kAhead) -- so the
    # helper, whose A - 1 extra barriers end it, executes as many barriers as the rounds wave
    step(P0_BASE, 0, barrier=HELPER_AHEAD == 1)
    L.append("s_sub_u32 %[cnt], %[nraw], 1")
    L.append("s_cmp_eq_u32 %[cnt], 0")
    L.append("s_cbranch_scc1 L_hdone_%=")
    first_loop_blk = max(1, HELPER_AHEAD - 1)
    for m in range(1, first_loop_blk):   # blocks 1 .. A - 2 (A >= 3): written before the first barrier
        step((P0_BASE, P1_BASE)[m % 2], (m % LDS_BUFS) * RING_BYTES, barrier=False)
        L.append("s_sub_u32 %[cnt], %[cnt], 1")
        L.append("s_cmp_eq_u32 %[cnt], 0")
        L.append("s_cbranch_scc1 L_hdone_%=")
    if twin and TWIN_HALIGN is not None:
        L.append(".p2align 6")
        L.extend(["s_nop 0"] * int(TWIN_HALIGN))
    if not twin and SPLIT_HALIGN is not None:
        L.append(".p2align 6")
        L.extend(["s_nop 0"] * int(SPLIT_HALIGN))
    L.append("L_hloop_%=:")
    period = 2 * LDS_BUFS // (2 if LDS_BUFS % 2 == 0 else 1)   # lcm(prefetch register sets 2, LDS buffers)
    for k in range(period):
        blk = k + first_loop_blk     # block index (mod period) of this step
        step((P0_BASE, P1_BASE)[blk % 2], (blk % LDS_BUFS) * RING_BYTES)
        L.append("s_sub_u32 %[cnt], %[cnt], 1")
        L.append("s_cmp_eq_u32 %[cnt], 0")
        L.append("s_cbranch_scc1 L_hdone_%=" if k < period - 1 else "s_cbranch_scc0 L_hloop_%=")
    L.append("L_hdone_%=:")
    if HELPER_WAIT == "mid" and not twin:
        L.append("s_waitcnt lgkmcnt(0)")   # (no write of this statement left in flight for the compiler's code)
    L.append("s_waitcnt vmcnt(0)")
    return "\n".join(f'    "{l}\\n"' for l in L)


# ---------------------------------------------------------------- emulator -------------

def emulate(ins, regs: dict, lds: dict | None = None, addr: int = 0, on_barrier=None, drain: bool = True,
            pending: list | None = None):
    """Execute an instruction list on a dict of 32-bit registers (one lane).  ds_read results
    land only when an s_waitcnt lgkmcnt(N) retires them (in order); reading a register whose
    load is still in flight, or overwriting one, raises -- so the wait counts are checked too.
    `pending` (the lane's in-flight reads) may be passed in to carry it across calls."""
    if pending is None:
        pending = []  # [(regs, values, lds addresses)] oldest first

    def v(x):
        if isinstance(x, str):
            for rs, _, _ in pending:
                if x in rs:
                    raise AssertionError(f"read of {x} before its ds_read retired")
            return regs[x]
        return x

    def wr(x, val):
        for rs, _, _ in pending:
            if x in rs:
                raise AssertionError(f"write of {x} while its ds_read is in flight")
        regs[x] = val

    for op in ins:
        o = op[0]
        if o == "v_add3_u32":
            wr(op[1], (v(op[2]) + v(op[3]) + v(op[4])) & M32)
        elif o == "v_alignbit_b32":
            s_ = op[4] & 31
            cat = (v(op[2]) << 32) | v(op[3])
            wr(op[1], (cat >> s_) & M32)
        elif o == "v_bfi_b32":
            a, b, c = v(op[2]), v(op[3]), v(op[4])
            wr(op[1], ((a & b) | (~a & c)) & M32)
        elif o == "v_bitop3_b32":
            a, b, c, imm = v(op[2]), v(op[3]), v(op[4]), op[5]
            r = 0
            for bit in range(32):
                idx = (((a >> bit) & 1) << 2) | (((b >> bit) & 1) << 1) | ((c >> bit) & 1)
                r |= ((imm >> idx) & 1) << bit
            wr(op[1], r)
        elif o == "v_xor_b32":
            wr(op[1], v(op[2]) ^ v(op[3]))
        elif o == "v_add_u32":
            wr(op[1], (v(op[2]) + v(op[3])) & M32)
        elif o == "v_mov_b32":
            wr(op[1], v(op[2]))
        elif o == "v_perm_b32":   # D.byte[i] = byte sel.byte[i] of {S0:S1} (0-3: S1, 4-7: S0; 12: 0x00)
            cat = ((v(op[2]) << 32) | v(op[3])).to_bytes(8, "little")
            sel = v(op[4]).to_bytes(4, "little")
            assert all(x < 8 or x == 12 for x in sel), "v_perm selector outside the emulated subset"
            wr(op[1], int.from_bytes(bytes(cat[x] if x < 8 else 0 for x in sel), "little"))
        elif o == "ds_write_b128":
            base, off = op[1], op[2]
            for j in range(4):
                lds[addr + off + 4 * j] = v(f"v{base + j}")
        elif o in ("ds_read_b128", "ds_read_b128_abs"):
            q, off = op[1], op[2]
            rs = [ring_reg(q, j) if o == "ds_read_b128" else f"v{RING_BASE + 4 * q + j}" for j in range(4)]
            for x in rs:
                for prs, _, _ in pending:
                    assert x not in prs, f"ds_read into {x} while it is in flight"
            # (an address nothing wrote reads as garbage: a prefetch past the last block, never consumed)
            pending.append((rs, [lds.get(addr + off + 4 * j, 0xBAD0BAD0) for j in range(4)],
                            [addr + off + 4 * j for j in range(4)]))
        elif o == "s_waitcnt_lgkm":
            while len(pending) > op[1]:
                rs, vals, _ = pending.pop(0)
                for x, val in zip(rs, vals):
                    regs[x] = val
        elif o == "s_barrier":
            if on_barrier is not None:
                on_barrier({a for _, _, adrs in pending for a in adrs})
        elif o in ("s_nop", "s_text"):   # (s_text: a scalar instruction of the loop's control flow, as written)
            pass
        else:
            raise ValueError(o)
    if drain:
        assert not pending, "ds_read still in flight at the end of the block"
    return regs


def emulate_twin(ins, regs2, lds, addrs, on_barrier=None, pend=None, drain: bool = True):
    """Run an instruction list on the two lanes of a TWIN pair in lockstep (regs2 / addrs per lane: lane b is
    helper lane 2i + b, or role b of a rounds wave).  v_add_u32_dpp and v_mov_b32_dpp end with (ctrl, bank_mask):
    they read their first source through DPP -- ctrl "ror8" = from the partner, "own" = from the lane itself -- and
    write only the lanes of bank_mask (ROLE0, ROLE1 or BOTH).  Every other instruction runs per lane through
    emulate(), with each lane's in-flight reads carried across instructions."""
    pend = pend if pend is not None else ([], [])
    for op in ins:
        if op[0] in ("v_add_u32_dpp", "v_mov_b32_dpp"):
            dst, src, (ctrl, bank) = op[1], op[2], op[-1]
            src1 = op[3] if op[0] == "v_add_u32_dpp" else None
            assert bank in (ROLE0, ROLE1, BOTH) and ctrl in ("ror8", "own"), op
            vals = {}
            for ln in range(2):
                if not bank & (ROLE0, ROLE1)[ln]:
                    continue
                frm = 1 - ln if ctrl == "ror8" else ln
                assert all(src not in rs for rs, _, _ in pend[frm]), f"DPP read of {src} in flight"
                assert all(src1 not in rs and dst not in rs for rs, _, _ in pend[ln]), "in-flight register"
                vals[ln] = (regs2[frm][src] + (regs2[ln][src1] if src1 is not None else 0)) & M32
            for ln, val in vals.items():
                regs2[ln][dst] = val
        elif op[0] == "s_barrier":
            if on_barrier is not None:
                on_barrier({a for ln in range(2) for _, _, adrs in pend[ln] for a in adrs})
        else:
            for ln in range(2):
                emulate([op], regs2[ln], lds, addrs[ln], drain=False, pending=pend[ln])
    if drain:
        assert not pend[0] and not pend[1], "ds_read still in flight at the end of the block"
    return regs2


def _check_block(block: bytes, h):
    w = list(struct.unpack(">16I", block))
    # expected: reference compress
    def rotl(x, n):
        return ((x << n) | (x >> (32 - n))) & M32
    ww = w + [0] * 64
    for t in range(16, 80):
        ww[t] = rotl(ww[t - 3] ^ ww[t - 8] ^ ww[t - 14] ^ ww[t - 16], 1)
    a, b, c, d, e = h
    for t in range(80):
        if t < 20:
            f = (b & c) | (~b & d)
        elif t < 40 or t >= 60:
            f = b ^ c ^ d
        else:
            f = (b & c) | (b & d) | (c & d)
        tmp = (rotl(a, 5) + (f & M32) + e + K[t // 20] + ww[t]) & M32
        e, d, c, b, a = d, c, rotl(b, 30), a, tmp
    exp = [(x + y) & M32 for x, y in zip(h, (a, b, c, d, e))]

    base = {f"h{i}": h[i] for i in range(5)}
    base.update({f"k{i}": K[i] for i in range(4)})
    # FULL
    regs = dict(base)
    regs.update({f"w{i}": w[i] for i in range(16)})
    emulate(gen_full(), regs)
    got = [(h[i] + regs[f"r{i}"]) & M32 for i in range(5)]
    assert got == exp, "SHA1_FULL mismatch"
    # HELPER: raw little-endian words -> K+W[0..79] in LDS
    regs = {"sel": 0x00010203}
    regs.update({f"k{i}": K[i] for i in range(4)})
    regs.update({f"raw{i}": int.from_bytes(block[4 * i:4 * i + 4], "little") for i in range(16)})
    lds = {}
    emulate(gen_helper(), regs, lds, 0)
    for t in range(80):
        assert lds[split_word_addr(t)] == (ww[t] + K[t // 20]) & M32, "SHA1_HELPER mismatch"
    # LDS rounds consume the helper's output
    regs = dict(base)
    emulate(gen_lds(), regs, lds, 0)
    got = [(h[i] + regs[f"r{i}"]) & M32 for i in range(5)]
    assert got == exp, "SHA1_LDS mismatch"
    # TWIN: the helper's twin layout for piece 33 (helper lane 33; rounds wave 1, lanes 2 and 3)
    hregs = []
    for ln in range(2):
        regs = {"sel": 0x00010203, "psel": (0x03020100, 0x07060504)[ln]}
        regs.update({f"k{i}": K[i] for i in range(4)})
        regs.update({f"raw{i}": int.from_bytes(block[4 * i:4 * i + 4], "little") for i in range(16)})
        hregs.append(regs)
    lds = {}
    # piece 33: lanes 2 and 3 of wave 1 (helper wave 3 writes where rounds wave 1 reads)
    emulate_twin(gen_helper2(), hregs, lds, [1024 + 2 * 16, 1024 + 3 * 16])
    for t in range(80):
        assert lds[1024 + 2 * 16 + twin_word_addr(t)] == (ww[t] + K[t // 20]) & M32, "SHA1_HELPER2 mismatch"
    # the rounds: roles 0 and 1 of that piece read helper lanes 2 and 3's words
    regs2 = [dict(base), dict(base)]
    emulate_twin(gen_roles(0), regs2, lds, [1024 + 2 * 16, 1024 + 3 * 16])
    for ln in range(2):
        got = [(h[i] + regs2[ln][f"r{i}"]) & M32 for i in range(5)]
        assert got == exp, f"SHA1_ROLES mismatch (role {ln})"
    return exp


def _kw_words(block: bytes):
    def rotl(x, n):
        return ((x << n) | (x >> (32 - n))) & M32
    ww = list(struct.unpack(">16I", block)) + [0] * 64
    for t in range(16, 80):
        ww[t] = rotl(ww[t - 3] ^ ww[t - 8] ^ ww[t - 14] ^ ww[t - 16], 1)
    return [(ww[t] + K[t // 20]) & M32 for t in range(80)]


def split_word_addr(t: int) -> int:
    """Where the split helper's lane 0 writes K+W[t] of a block, from its buffer's base ([t/4][lane][4 words])."""
    return 1024 * (t // 4) + 4 * (t % 4)


def twin_word_addr(t: int) -> int:
    """The same for the lane pair 0, 1 of the twin layout ([k][wave][lane][4 words], lane t%2 owns word t)."""
    return (t // 8) * TWIN_READ_BYTES + (t % 2) * 16 + 4 * ((t % 8) // 2)


class HelperProtocol:
    """The helper wave as a rounds wave may rely on it, and no kinder.  Blocks 0 and 1 are in LDS at the start.  At
    the barrier that ends block k, block k+3's buffer is poisoned (it is handed back: the real helper may be
    writing it from then on) and block k+2 is written (the latest moment the protocol allows).  A read of a block
    too early, or of a buffer after it was handed back, returns wrong words, and a write to an address whose read
    is still in flight fails.  word_addr(t) places K+W[t] in a buffer: the layout under test."""

    def __init__(self, blocks, word_addr):
        self.lds, self.word_addr, self.ended = {}, word_addr, 0
        self.kws = [_kw_words(b) for b in blocks]
        for m in range(min(2, len(blocks))):
            self.put(m, self.kws[m])

    def put(self, block, words, in_flight=frozenset()):
        base = (block % LDS_BUFS) * RING_BYTES
        for t in range(80):
            a = base + self.word_addr(t)
            assert a not in in_flight, f"LDS {a} rewritten while a ds_read of it is in flight"
            self.lds[a] = words[t]

    def on_barrier(self, in_flight):
        k = self.ended               # the block that just ended
        self.ended = k + 1
        self.put(k + 3, [0xDEADBEEF ^ t for t in range(80)], in_flight)   # handed back to the helper
        if k + 2 < len(self.kws):
            self.put(k + 2, self.kws[k + 2], in_flight)


def split_rounds_stream(nsteps: int):
    """The instructions rounds_loop_text executes for nsteps blocks, in order (without its scalar control flow)."""
    return [op for k in range(nsteps) for op in split_rounds_block(k)] + [("s_waitcnt_lgkm", 0)]


def check_split_stream(blocks, h, ins=None):
    """The split kernel's rounds loop over consecutive blocks (split_rounds_stream, or the stream `ins` given in
    its place) for lane 0, against the helper protocol; returns the chaining value."""
    helper = HelperProtocol(blocks, split_word_addr)
    regs = {f"h{i}": h[i] for i in range(5)}
    emulate(split_rounds_stream(len(blocks)) if ins is None else ins, regs, helper.lds, 0, on_barrier=helper.on_barrier)
    return [regs[f"h{i}"] for i in range(5)]


def check_twin_stream(blocks, h):
    """The TWIN rounds loop over consecutive blocks as roles_rounds_loop_text lays it out (roles_rounds_stream, with
    the DPP-distance rule checked over the whole stream), for the lane pair of piece 0, against the helper
    protocol; returns the chaining value."""
    helper = HelperProtocol(blocks, twin_word_addr)
    regs2 = [{f"h{i}": h[i] for i in range(5)} for _ in range(2)]
    ins = roles_rounds_stream(len(blocks))
    check_dpp_distance(ins)
    emulate_twin(ins, regs2, helper.lds, [0, 16], on_barrier=helper.on_barrier)
    assert all(regs2[0][f"h{i}"] == regs2[1][f"h{i}"] for i in range(5)), "twin roles disagree"
    return [regs2[0][f"h{i}"] for i in range(5)]


def self_check():
    """Hash several messages through the emulated instruction streams; compare with hashlib."""
    import random
    rng = random.Random(1)
    for n in [0, 3, 55, 56, 64, 119, 200]:
        msg = bytes(rng.randrange(256) for _ in range(n))
        bits = 8 * n
        padded = msg + b"\x80" + b"\0" * ((55 - n) % 64) + struct.pack(">Q", bits)
        h = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
        for i in range(0, len(padded), 64):
            h = _check_block(padded[i:i + 64], h)
        assert struct.pack(">5I", *h) == hashlib.sha1(msg).digest(), n
    # the split and the TWIN rounds loops over 1 .. 7, 8, 13 and 15 consecutive blocks: every buffer phase, and both
    # parities of the block count go round the twin loop's six-block body
    # (the protocol model is the helper two blocks ahead, which takes three buffers)
    for n in ([0, 55, 64, 119, 200, 310, 400, 500, 800, 900] if LDS_BUFS == 3 else []):
        msg = bytes(rng.randrange(256) for _ in range(n))
        padded = msg + b"\x80" + b"\0" * ((55 - n) % 64) + struct.pack(">Q", 8 * n)
        blocks = [padded[i:i + 64] for i in range(0, len(padded), 64)]
        h0 = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
        h = check_split_stream(blocks, h0)
        assert struct.pack(">5I", *h) == hashlib.sha1(msg).digest(), ("split stream", n)
        h = check_twin_stream(blocks, h0)
        assert struct.pack(">5I", *h) == hashlib.sha1(msg).digest(), ("twin stream", n)
    return True


# ---------------------------------------------------------------- emitter --------------

def _opnd(x, full: bool):
    if isinstance(x, int):
        return str(x)
    if x.startswith("v") and x[1:].isdigit():
        return x  # physical ring register
    return f"%[{x}]"


def _emit_lines(ins, full: bool = False):
    lines = []
    for op in ins:
        o = op[0]
        if o == "s_waitcnt_lgkm":
            lines.append(f"s_waitcnt lgkmcnt({op[1]})")
        elif o == "ds_read_b128":
            q, off = op[1], op[2]
            lo = RING_BASE + 4 * (q % RING_QUADS)
            a, off = ("%[addr2]", off - 65536) if off >= 65536 else ("%[addr]", off)   # (16-bit DS offsets)
            lines.append(f"ds_read_b128 v[{lo}:{lo + 3}], {a} offset:{off}")
        elif o == "ds_read_b128_abs":   # quad index without the ring's wrap (the twin loop's register sets)
            lo = RING_BASE + 4 * op[1]
            assert op[2] < 65536
            lines.append(f"ds_read_b128 v[{lo}:{lo + 3}], %[addr] offset:{op[2]}")
        elif o == "v_bitop3_b32":
            lines.append(f"v_bitop3_b32 {_opnd(op[1], full)}, {_opnd(op[2], full)}, {_opnd(op[3], full)}, "
                         f"{_opnd(op[4], full)} bitop3:0x{op[5]:02x}")
        elif o == "v_alignbit_b32":
            lines.append(f"v_alignbit_b32 {_opnd(op[1], full)}, {_opnd(op[2], full)}, {_opnd(op[3], full)}, {op[4]}")
        elif o in ("v_xor_b32", "v_add_u32"):
            lines.append(f"{o} {_opnd(op[1], full)}, {_opnd(op[2], full)}, {_opnd(op[3], full)}")
        elif o == "v_perm_b32":
            lines.append(f"v_perm_b32 {_opnd(op[1], full)}, {_opnd(op[2], full)}, {_opnd(op[3], full)}, {_opnd(op[4], full)}")
        elif o == "ds_write_b128":
            a, off = ("%[addr2]", op[2] - 65536) if op[2] >= 65536 else ("%[addr]", op[2])
            lines.append(f"ds_write_b128 {a}, v[{op[1]}:{op[1] + 3}] offset:{off}")
        elif o == "s_barrier":
            lines.append("s_barrier")
        elif o == "s_nop":
            lines.append("s_nop 0")
        elif o in ("v_add_u32_dpp", "v_mov_b32_dpp"):
            ctrl, bank = op[-1]
            lines.append(f"{o} " + ", ".join(_opnd(x, full) for x in op[1:-1]) + " "
                         + {"ror8": "row_ror:8", "own": "quad_perm:[0,1,2,3]"}[ctrl] + f" row_mask:0xf bank_mask:0x{bank:x}")
        elif o == "v_mov_b32":
            lines.append(f"v_mov_b32_e64 {_opnd(op[1], full)}, {_opnd(op[2], full)}")   # (8 bytes, as every VALU here)
        elif o == "s_text":
            lines.append(op[1])
        else:
            lines.append(f"{o} " + ", ".join(_opnd(x, full) for x in op[1:]))
    return lines


def emit(ins, full: bool) -> str:
    return "\n".join(f'    "{l}\\n"' for l in _emit_lines(ins, full))


HEADER = """// GENERATED by tools/gen_sha1_asm.py -- do not edit.  Regenerate with:
//   python3 tools/gen_sha1_asm.py
// The instruction streams below are checked against hashlib by the generator's emulator
// (tests/test_abi.py::test_asm_generator_emulator) before they are written.
#pragma once
#include <stdint.h>

#define TV_SHA1_RING_BASE {ring_base}
#define TV_SHA1_RING_QUADS {ring_quads}
// K+W buffers per split-kernel pair, and how many blocks the helper wave runs ahead of the rounds wave
// (its first HELPER_AHEAD - 1 writes are not followed by a barrier; it ends with as many extra barriers)
#define TV_SHA1_LDS_BUFS {lds_bufs}
#define TV_SHA1_HELPER_AHEAD {helper_ahead}

// One SHA-1 compression, schedule in-asm.  w[16] holds the big-endian message words and is
// clobbered.  On return r = working state after round 79; caller does h += r.
__device__ __forceinline__ void tv_sha1_full(const uint32_t h[5], uint32_t r[5], uint32_t w[16],
                                             uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    uint32_t t0, t1, t2, t3;
    // volatile + "memory": the compiler may not move the caller's prefetch loads across the block
    // (otherwise it sinks them next to their use and the load latency is exposed every block).
    asm volatile(
{full}
    : [r0] "=&v"(r[0]), [r1] "=&v"(r[1]), [r2] "=&v"(r[2]), [r3] "=&v"(r[3]), [r4] "=&v"(r[4]),
      [w0] "+v"(w[0]), [w1] "+v"(w[1]), [w2] "+v"(w[2]), [w3] "+v"(w[3]),
      [w4] "+v"(w[4]), [w5] "+v"(w[5]), [w6] "+v"(w[6]), [w7] "+v"(w[7]),
      [w8] "+v"(w[8]), [w9] "+v"(w[9]), [w10] "+v"(w[10]), [w11] "+v"(w[11]),
      [w12] "+v"(w[12]), [w13] "+v"(w[13]), [w14] "+v"(w[14]), [w15] "+v"(w[15]),
      [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
    : [h0] "v"(h[0]), [h1] "v"(h[1]), [h2] "v"(h[2]), [h3] "v"(h[3]), [h4] "v"(h[4]),
      [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : "memory");
}}

// The 80 rounds of one compression with K+W[0..79] read from LDS at byte address `addr`
// (+ g*1024 for quad g), as written by tv_sha1_schedule_lds.  Waits for all of its own LDS reads
// before returning.
__device__ __forceinline__ void tv_sha1_lds(const uint32_t h[5], uint32_t r[5], uint32_t addr,
                                            uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    uint32_t t0, t1;
    asm volatile(
{lds}
    : [r0] "=&v"(r[0]), [r1] "=&v"(r[1]), [r2] "=&v"(r[2]), [r3] "=&v"(r[3]), [r4] "=&v"(r[4]),
      [t0] "=&v"(t0), [t1] "=&v"(t1)
    : [h0] "v"(h[0]), [h1] "v"(h[1]), [h2] "v"(h[2]), [h3] "v"(h[3]), [h4] "v"(h[4]), [addr] "v"(addr){addr2},
      [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {ring_clobbers}, "memory");
}}

// The split kernel's helper wave over its nraw (>= 1) raw blocks: va = address of the first
// block of this lane's piece, addr = LDS byte address of this lane in ring buffer 0.  One
// workgroup barrier per block (matching the rounds wave).  Returns with no load in flight.
__device__ __forceinline__ void tv_sha1_helper_loop(const void* va, uint32_t nraw, uint32_t addr,
                                                    uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    uint32_t cnt, adv;
    uint64_t inc;
    asm volatile(
{helper_loop}
    : [cnt] "=&s"(cnt), [adv] "=&s"(adv), [inc] "=&s"(inc)
    : [va] "v"(va), [nraw] "s"(nraw), [addr] "v"(addr){addr2}, [sel] "s"(0x00010203u),
      [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {loop_clobbers}, "scc", "memory");
}}

// The split kernel's rounds wave over nsteps (>= 1) consecutive blocks starting with ring buffer 0,
// in which every lane updates its chaining value: 80 rounds from LDS, h += r, workgroup barrier.
__device__ __forceinline__ void tv_sha1_rounds_loop(uint32_t h[5], uint32_t addr, uint32_t nsteps,
                                                    uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    uint32_t r[5], t0, t1, cnt;
    asm volatile(
{rounds_loop}
    : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [h4] "+v"(h[4]),
      [r0] "=&v"(r[0]), [r1] "=&v"(r[1]), [r2] "=&v"(r[2]), [r3] "=&v"(r[3]), [r4] "=&v"(r[4]),
      [t0] "=&v"(t0), [t1] "=&v"(t1), [cnt] "=&s"(cnt)
    : [addr] "v"(addr){addr2}, [nsteps] "s"(nsteps), [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {ring_clobbers}, "scc", "memory");
}}

// Message schedule of one block for the split kernel's helper wave: raw[16] are the block's words
// as loaded (little-endian); writes K+W[0..79] to LDS at `addr` (+ q*1024 for quad q).  The LDS
// writes are left in flight (the caller's barrier waits lgkmcnt(0)).
__device__ __forceinline__ void tv_sha1_schedule_lds(const uint32_t raw[16], uint32_t addr,
                                                     uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    asm volatile(
{helper}
    :
    : [raw0] "v"(raw[0]), [raw1] "v"(raw[1]), [raw2] "v"(raw[2]), [raw3] "v"(raw[3]),
      [raw4] "v"(raw[4]), [raw5] "v"(raw[5]), [raw6] "v"(raw[6]), [raw7] "v"(raw[7]),
      [raw8] "v"(raw[8]), [raw9] "v"(raw[9]), [raw10] "v"(raw[10]), [raw11] "v"(raw[11]),
      [raw12] "v"(raw[12]), [raw13] "v"(raw[13]), [raw14] "v"(raw[14]), [raw15] "v"(raw[15]),
      [addr] "v"(addr){addr2}, [sel] "s"(0x00010203u), [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {helper_clobbers}, "memory");
}}
"""


TWIN_HEADER = """
// ---- TWIN kernel: two lanes per piece in the rounds and helper waves (tools/gen_sha1_asm.py gen_helper2,
// gen_roles, gen_roles_trip_block).  K+W buffer layout [k][wave][lane][4 words]; a helper lane's `addr` is
// ring + (wave & 1)*1024 + lane*16, its `psel` 0x03020100 (even lane) / 0x07060504 (odd lane).
// Rounds: lane 16r+p (p < 8) of a rounds wave is role 0 of the wave's piece 8r+p, lane 16r+8+p its role 1, and
// role b's `addr` is that of helper lane 2(8r+p)+b: ring + (wave & 1)*1024 + (2(8r+p)+b)*16.  Both rounds
// functions take and return the plain chaining value / state in BOTH lanes of a pair, and need every lane of the
// wave active (the roles exchange values through DPP).

// One block of 80 rounds for a lane pair, with its own 10 LDS reads (waits for them before returning).
__device__ __forceinline__ void tv_sha1_roles_lds(const uint32_t h[5], uint32_t r[5], uint32_t addr) {{
    uint32_t t0, t1;
    asm volatile(
{roles_lds}
    : [r0] "=&v"(r[0]), [r1] "=&v"(r[1]), [r2] "=&v"(r[2]), [r3] "=&v"(r[3]), [r4] "=&v"(r[4]),
      [t0] "=&v"(t0), [t1] "=&v"(t1)
    : [h0] "v"(h[0]), [h1] "v"(h[1]), [h2] "v"(h[2]), [h3] "v"(h[3]), [h4] "v"(h[4]), [addr] "v"(addr){addr2}
    : {ring_clobbers}, "memory");
}}

// The TWIN rounds wave over nsteps (>= 1) blocks from ring buffer 0 in which every lane updates.  The block is
// written once, as an assembler macro of its K+W registers, the registers its reads fill and their offset.
__device__ __forceinline__ void tv_sha1_roles_rounds_loop(uint32_t h[5], uint32_t addr, uint32_t nsteps) {{
    uint32_t r[5], t0, t1, cnt;
    asm volatile(
{roles_rounds_loop}
    : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [h4] "+v"(h[4]),
      [r0] "=&v"(r[0]), [r1] "=&v"(r[1]), [r2] "=&v"(r[2]), [r3] "=&v"(r[3]), [r4] "=&v"(r[4]),
      [t0] "=&v"(t0), [t1] "=&v"(t1), [cnt] "=&s"(cnt)
    : [addr] "v"(addr){addr2}, [nsteps] "s"(nsteps)
    : {twin_ring_clobbers}, "scc", "memory");
}}

// The TWIN helper wave (64 pieces, one lane each) over its nraw (>= 1) raw blocks: as
// tv_sha1_helper_loop, writing the twin layout.
__device__ __forceinline__ void tv_sha1_twin_helper_loop(const void* va, uint32_t nraw, uint32_t addr, uint32_t psel,
                                                         uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    uint32_t cnt, adv;
    uint64_t inc;
    asm volatile(
{twin_helper_loop}
    : [cnt] "=&s"(cnt), [adv] "=&s"(adv), [inc] "=&s"(inc)
    : [va] "v"(va), [nraw] "s"(nraw), [addr] "v"(addr){addr2}, [sel] "s"(0x00010203u), [psel] "v"(psel),
      [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {twin_loop_clobbers}, "scc", "memory");
}}

// Message schedule of one block into the twin layout (the helper's padded tail blocks).
__device__ __forceinline__ void tv_sha1_twin_schedule_lds(const uint32_t raw[16], uint32_t addr, uint32_t psel,
                                                          uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {{
    asm volatile(
{twin_helper}
    :
    : [raw0] "v"(raw[0]), [raw1] "v"(raw[1]), [raw2] "v"(raw[2]), [raw3] "v"(raw[3]),
      [raw4] "v"(raw[4]), [raw5] "v"(raw[5]), [raw6] "v"(raw[6]), [raw7] "v"(raw[7]),
      [raw8] "v"(raw[8]), [raw9] "v"(raw[9]), [raw10] "v"(raw[10]), [raw11] "v"(raw[11]),
      [raw12] "v"(raw[12]), [raw13] "v"(raw[13]), [raw14] "v"(raw[14]), [raw15] "v"(raw[15]),
      [addr] "v"(addr){addr2}, [sel] "s"(0x00010203u), [psel] "v"(psel), [k0] "s"(k0), [k1] "s"(k1), [k2] "s"(k2), [k3] "s"(k3)
    : {twin_helper_clobbers}, "memory");
}}
"""


def render() -> str:
    ring = ", ".join(f'"v{RING_BASE + i}"' for i in range(4 * RING_QUADS))
    hregs = list(range(HW_BASE, HW_BASE + 16)) + [HT, HT2] + list(range(HOUT_BASE, HOUT_BASE + 4 * HOUT_QUADS))
    helper = ", ".join(f'"v{i}"' for i in hregs)
    # (the two-block-trip twin loop: two sets of ten quads)
    twin_ring = ", ".join(f'"v{RING_BASE + i}"' for i in range(4 * max(RING_QUADS, 2 * TWIN_SET_QUADS)))
    loop = ", ".join(f'"v{i}"' for i in hregs + list(range(P0_BASE, VL + 2)))
    h2regs = list(range(H2_F, H2_O + 12))
    h2 = ", ".join(f'"v{i}"' for i in h2regs)
    h2loop = ", ".join(f'"v{i}"' for i in h2regs + list(range(P0_BASE, VL + 2)))
    # a K+W ring past 64 KiB (LDS_BUFS >= 4) addresses its upper buffers from a second register: DS offsets are 16-bit
    addr2 = ', [addr2] "v"(addr + 65536u)' if LDS_BUFS * RING_BYTES > 65536 else ""
    return HEADER.format(addr2=addr2, ring_base=RING_BASE, ring_quads=RING_QUADS, lds_bufs=LDS_BUFS, helper_ahead=HELPER_AHEAD,
                         full=('    ".p2align 3\\n"\n' if ALIGN_FULL else "") + emit(gen_full(), True),
                         lds=emit(gen_lds(), False), helper=emit(gen_helper(), False),
                         helper_loop=helper_loop_text(), rounds_loop=rounds_loop_text(),
                         ring_clobbers=ring, helper_clobbers=helper,
                         loop_clobbers=loop) + TWIN_HEADER.format(
                             roles_lds='    ".p2align 3\\n"\n' + emit(gen_roles(0), False),
                             roles_rounds_loop=roles_rounds_loop_text(),
                             twin_helper_loop=helper_loop_text(twin=True),
                             twin_helper=emit(gen_helper2(), False),
                             ring_clobbers=ring, twin_ring_clobbers=twin_ring, twin_helper_clobbers=h2, twin_loop_clobbers=h2loop, addr2=addr2)


STAMP_FNS = (("tv_sha1_rounds_loop", "uint32_t nsteps,\n", '[cnt] "=&s"(cnt)\n'),
             ("tv_sha1_helper_loop", "uint32_t nraw, uint32_t addr,\n", '[inc] "=&s"(inc)\n'),
             ("tv_sha1_roles_rounds_loop", "uint32_t nsteps) {\n", '[cnt] "=&s"(cnt)\n'),
             ("tv_sha1_twin_helper_loop", "uint32_t addr, uint32_t psel,\n", '[inc] "=&s"(inc)\n'))


def _stamp_patch(txt: str) -> str:
    """STAMP builds: give the four loops an accumulator argument `sbar` (cycles at the in-loop barriers; the helper
    loops at level 2 also `svm` and `slg`) and the SGPRs the stamps use as clobbers."""
    for fn, sig_old, out_old in STAMP_FNS:
        extra = fn in ("tv_sha1_helper_loop", "tv_sha1_twin_helper_loop") and STAMP >= 2
        i = txt.index(f"void {fn}(")
        j = txt.index("\n}\n", i)
        seg = txt[i:j]
        if sig_old.endswith(") {\n"):   # (a signature ending the parameter list: add before the parenthesis)
            sig_new = sig_old[:-4] + ", uint32_t& sbar) {\n"
        else:
            sig_new = sig_old[:-2] + (", uint32_t& sbar, uint32_t& svm, uint32_t& slg,\n" if extra else ", uint32_t& sbar,\n")
        for old, new in ((sig_old, sig_new),
                         (out_old, out_old[:-1] + ', [sbar] "+s"(sbar)' + (', [svm] "+s"(svm), [slg] "+s"(slg)' if extra
                                                                          else "") + "\n"),
                         ('"scc", "memory");', '"s88", "s89", "s90", "s91", "scc", "memory");')):
            assert seg.count(old) == 1, (fn, old)
            seg = seg.replace(old, new)
        txt = txt[:i] + seg + txt[j:]
    assert txt.count("#define TV_SHA1_RING_BASE") == 1
    return txt.replace("#define TV_SHA1_RING_BASE", f"#define TV_SHA1_STAMP {STAMP}\n#define TV_SHA1_RING_BASE")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "torrent_amd", "csrc", "sha1_asm.h"))
    ap.add_argument("--check", action="store_true", help="only run the emulator self-check")
    a = ap.parse_args()
    self_check()
    if a.check:
        print("emulator self-check: ok")
        return
    txt = render()
    if STAMP:
        txt = _stamp_patch(txt)
    with open(a.out, "w") as f:
        f.write(txt)
    print(f"wrote {a.out}: FULL {len(gen_full())} instr, LDS {len(gen_lds())} instr, "
          f"HELPER {len(gen_helper())} instr")


if __name__ == "__main__":
    sys.exit(main())
