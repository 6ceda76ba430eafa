#!/usr/bin/env python3
"""Kernel time of tv_hybrid_verify against the two separate calls it replaces, on one staging.

    python tools/hybrid_bench.py [--out profiles/hybrid/bench.json]

Two geometries, both filled by tv_fill_synthetic:
    cfg2        16,384 pieces of 1 MiB as one file: no tail piece, so the pad launch is skipped;
    many_files  10,000 files of U[0, 512 KiB] (20 zero-length, 5 under 64 B: cfg3's draw) on 256 KiB pieces, every file
                at its aligned offset: a tail after nearly every file.
Per geometry, in one session on one context: tv_hybrid_hash makes both hash sets (a sample of pieces is checked against
hashlib SHA-1 over the padded bytes and a hashlib merkle root), then ROUNDS rounds of tv_verify, tv_v2_verify and
tv_hybrid_verify, one after the other, every bitfield checked; the medians of tv_last_timing's kernel ms are recorded.
Acceptance (cfg2, where nothing but the two hash launch sets runs): the hybrid span <= BOUND x the sum of the two
separate spans (5 %: the clock spread under load README reports for one build).  On many_files the pad kernel's
own time (TV_OPT_HYBRID_PAD_PROBE) is recorded next to one hipMemsetAsync per tail over the same ranges; it must not be
slower.  A reported result, not a test.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import synth  # noqa: E402  (the generator in numpy: nothing under oracle/ runs here)
from torrent_amd import _native as N  # noqa: E402
from torrent_amd.metainfo_v2 import make_layout  # noqa: E402

LEAF = 16384
ROUNDS, WARMUP = 5, 2
BOUND = 1.05
SEED = 9


def many_file_lengths() -> list:
    """cfg3's draw (tests/layouts.py): 10,000 files of U[0, 512 KiB], 20 of them empty and 5 under 64 bytes."""
    rng = random.Random(3)
    sizes = [rng.randrange((512 << 10) + 1) for _ in range(10000)]
    idx = rng.sample(range(10000), 25)
    for k in idx[:20]:
        sizes[k] = 0
    for k in idx[20:]:
        sizes[k] = rng.randrange(1, 64)
    return sizes


def merkle_root(data: bytes, width: int) -> bytes:
    row = [hashlib.sha256(data[o:o + LEAF]).digest() for o in range(0, len(data), LEAF)]
    row += [bytes(32)] * (width - len(row))
    while len(row) > 1:
        row = [hashlib.sha256(row[i] + row[i + 1]).digest() for i in range(0, len(row), 2)]
    return row[0]


def geometry(ctx, name: str, lengths: list, L: int) -> dict:
    lay = make_layout(lengths, L)
    P = lay.n_pieces
    total = lay.total_length
    ctx.set_layout(total, L, P)
    ctx.fill_synthetic(SEED)
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, None)
    digests, roots = ctx.hybrid_hash()
    v1_len = [min(L, total - i * L) for i in range(P)]
    tails = [i for i in range(P) if lay.piece_bytes[i] < v1_len[i]]
    sample = sorted(set([0, P // 2, P - 1] + tails[:3] + tails[-2:]))
    for i in sample:                                     # both hash sets against hashlib, tails included
        row = bytes(synth.fill(SEED, i * L, lay.piece_bytes[i]))
        assert digests[20 * i:20 * i + 20] == hashlib.sha1(row + bytes(v1_len[i] - len(row))).digest(), (name, i)
        assert roots[32 * i:32 * i + 32] == merkle_root(row, lay.tree_leaves[i]), (name, i)
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, roots)
    ctx.set_digests(digests)
    full = bytearray(b"\xff" * ((P + 7) // 8))
    if P % 8:
        full[-1] = (0xFF00 >> (P % 8)) & 0xFF
    full = bytes(full)

    calls = {"verify": lambda: (ctx.verify(),), "v2_verify": lambda: (ctx.v2_verify(),),
             "hybrid_verify": ctx.hybrid_verify}
    times = {k: [] for k in calls}
    launches = {}
    for step in range(WARMUP + ROUNDS):                  # the three calls alternate, so a clock drift meets them alike
        for k, call in calls.items():
            assert all(b == full for b in call()), (name, k)
            launches[k] = ctx.last_kernel()[1]
            if step >= WARMUP:
                times[k].append(ctx.last_timing()[0])
    row = {"name": name, "piece_length": L, "pieces": P, "files": len(lengths), "bytes": total, "tail_pieces": len(tails),
           "tail_bytes": sum(v1_len[i] - lay.piece_bytes[i] for i in tails)}
    for k, v in times.items():
        row[k] = {"kernel_ms": round(statistics.median(v), 4), "kernel_ms_min": round(min(v), 4),
                  "kernel_ms_max": round(max(v), 4), "launches": launches[k]}
    separate = row["verify"]["kernel_ms"] + row["v2_verify"]["kernel_ms"]
    row["separate_sum_ms"] = round(separate, 4)
    row["hybrid_over_separate"] = round(row["hybrid_verify"]["kernel_ms"] / separate, 4)
    if tails:
        pad = {"kernel": [], "memset_per_tail": []}
        for step in range(WARMUP + ROUNDS):
            for mode, k in ((1, "kernel"), (2, "memset_per_tail")):
                ctx.set_option(N.TV_OPT_HYBRID_PAD_PROBE, mode)
                if step >= WARMUP:
                    pad[k].append(ctx.counter(N.TV_COUNTER_HYBRID_PAD_NS) / 1e6)
        row["pad_kernel_ms"] = round(statistics.median(pad["kernel"]), 4)
        row["pad_memset_per_tail_ms"] = round(statistics.median(pad["memset_per_tail"]), 4)
        row["pad_kernel_not_slower"] = row["pad_kernel_ms"] <= row["pad_memset_per_tail_ms"]
        assert ctx.hybrid_verify()[0] == full             # (the probes left the rows as the calls do)
    else:
        row["bound"] = BOUND
        row["pass"] = row["hybrid_verify"]["kernel_ms"] <= BOUND * separate
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"build_id": N.build_id(), "rounds": ROUNDS, "warmup": WARMUP}
    with N.Context(0) as ctx:
        res["rows"] = [geometry(ctx, "cfg2", [16384 << 20], 1 << 20),
                       geometry(ctx, "many_files", many_file_lengths(), 256 << 10)]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
