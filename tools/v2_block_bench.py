#!/usr/bin/env python3
"""Kernel time of the v2 block calls against the v2 list verify on the same staged pieces.

    python tools/v2_block_bench.py [--out profiles/v2/block_latency.json]

Per shape of the README's list-latency row (1 / 64 / 4,096 pieces of 256 KiB, 1 / 64 / 1,024 of 4 MiB): n resident
pieces of the synthetic payload, then tv_last_timing's kernel ms of
    tv_v2_leaf_hashes            every leaf of the n pieces (one checked against hashlib),
    tv_v2_check_blocks           every block of the n pieces against those leaves,
    tv_v2_verify_list            the yardstick: the same leaves hashed, then the tree levels,
all in one session on one context: the median of RUNS timed calls after WARMUP.  The block calls hash the same leaves
as the list call and no tree, so they should take at most BOUND x its kernel time (15 %: the spread the list row
itself shows, 0.67-0.78 ms); each shape's `pass` says whether it did.  A reported result, not a test.  One more row:
one wanted block of one 4 MiB piece (a block checked on arrival).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torrent_amd import _native as N  # noqa: E402

LEAF = 16384
SHAPES = ((256 << 10, (1, 64, 4096)), (4 << 20, (1, 64, 1024)))
RUNS, WARMUP = 5, 2
BOUND = 1.15


def _timed(ctx, call, check) -> dict:
    kernel, total = [], []
    for step in range(WARMUP + RUNS):
        assert check(call()), "a timed call's result is wrong"
        if step >= WARMUP:
            k, t = ctx.last_timing()
            kernel.append(k)
            total.append(t)
    return {"kernel_ms": round(statistics.median(kernel), 4), "total_ms": round(statistics.median(total), 4),
            "kernel_ms_min": round(min(kernel), 4), "kernel_ms_max": round(max(kernel), 4),
            "workgroups": ctx.counter(N.TV_COUNTER_LAST_WORKGROUPS)}


def shape(ctx, L: int, n: int) -> dict:
    W = L // LEAF
    ctx.set_layout(n * L, L, n)
    ctx.fill_synthetic(5)
    pieces, nbytes, widths = list(range(n)), [L] * n, [W] * n
    ctx.v2_set_pieces(nbytes, widths, None)
    roots = ctx.v2_hash()
    leaves = ctx.v2_leaf_hashes(pieces, nbytes, widths)
    buf = bytearray(L)
    ctx.read((n - 1) * L, buf)
    assert leaves[-32 * W:] == b"".join(hashlib.sha256(buf[o:o + LEAF]).digest() for o in range(0, L, LEAF)), \
        "the last piece's leaves differ from hashlib"
    every = b"\xff" * ((W + 7) // 8 * n)
    row = {"piece_length": L, "pieces": n, "blocks": n * W}
    row["v2_verify_list"] = _timed(ctx, lambda: ctx.v2_verify_list(pieces, nbytes, widths, roots),
                                   lambda ok: ok == b"\x01" * n)
    row["v2_leaf_hashes"] = _timed(ctx, lambda: ctx.v2_leaf_hashes(pieces, nbytes, widths), lambda h: h == leaves)
    row["v2_check_blocks"] = _timed(ctx, lambda: ctx.v2_check_blocks(pieces, nbytes, widths, leaves),
                                    lambda b: b == every)
    bound = row["v2_verify_list"]["kernel_ms"] * BOUND
    row["bound_ms"] = round(bound, 4)
    row["pass"] = {k: row[k]["kernel_ms"] <= bound for k in ("v2_leaf_hashes", "v2_check_blocks")}
    return row


def one_block(ctx) -> dict:
    """One wanted block (the last) of one resident 4 MiB piece."""
    L = 4 << 20
    W = L // LEAF
    ctx.set_layout(L, L, 1)
    ctx.fill_synthetic(5)
    leaves = ctx.v2_leaf_hashes([0], [L], [W])
    want = bytearray(W // 8)
    want[-1] = 0x01
    row = {"piece_length": L, "pieces": 1, "blocks": 1}
    row["v2_check_blocks"] = _timed(ctx, lambda: ctx.v2_check_blocks([0], [L], [W], leaves, bytes(want)),
                                    lambda b: b == bytes(want))
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"build_id": N.build_id(), "runs": RUNS, "warmup": WARMUP, "bound": BOUND}
    with N.Context(0) as ctx:
        res["rows"] = [shape(ctx, L, n) for L, counts in SHAPES for n in counts]
        res["one_wanted_block"] = one_block(ctx)
    res["all_pass"] = all(all(r["pass"].values()) for r in res["rows"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
