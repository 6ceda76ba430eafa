#!/usr/bin/env python3
"""Throughput of the creation streams next to the verify streams of the same kind.

    python tools/stream_hash_bench.py [--out profiles/stream_hash/bench.json]

Two geometries (those of tools/hybrid_bench.py --stream), the bytes from the host generator
(tv_stream_fill_synthetic fills every request's rows):
    cfg2        16,384 pieces of 1 MiB as one file (16 GiB);
    many_files  10,000 files of U[0, 512 KiB] (20 zero-length, 5 under 64 B: cfg3's draw) on 256 KiB pieces, every file
                at its aligned offset.
Per geometry, in one session on one ctx over the same bytes: the resident calls make the reference hashes (tv_hash,
tv_v2_hash, tv_hybrid_hash); then, under the default 1 GiB budget and under 0.25 GiB, for each kind (v1 in whole-piece
rows, TV_OPT_STREAM_ROWS = 1; v2; hybrid) RUNS timed passes of the verify stream and of the creation stream, alternating
(a clock drift meets them alike), after WARMUP untimed ones.  Every verify bitfield must be all ones and every creation
output must equal the resident call's.  Recorded: GB/s (aligned bytes / wall time of begin .. end) per run, median and
range, the kernel span and the launches.

Expectation: a creation stream's median is not below the slowest of the verify stream's runs -- the launches differ in
the final store only, and a creation stream uploads no digest table.  `pass` records whether that held; nothing is tuned
to it.  A reported result, not a test.  The tool also writes an index (README.md) beside the json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.hybrid_bench import SEED, many_file_lengths  # noqa: E402
from torrent_amd import _native as N  # noqa: E402
from torrent_amd.metainfo_v2 import make_layout  # noqa: E402

RUNS, WARMUP = 5, 1


def one_pass(ctx, nbytes: int, begin, end):
    t0 = time.perf_counter()
    begin()
    while True:
        req = ctx.stream_next()
        if not req.rows:
            break
        ctx.stream_fill_synthetic(req, SEED)
        ctx.stream_commit(req)
    got = end()
    el = time.perf_counter() - t0
    return got, nbytes / el / 1e9, ctx.last_timing()[0], ctx.last_kernel()


def summary(runs: list) -> dict:
    gbs = [r[1] for r in runs]
    return {"GBps_runs": [round(g, 2) for g in gbs], "GBps_median": round(statistics.median(gbs), 2),
            "GBps_min": round(min(gbs), 2), "GBps_max": round(max(gbs), 2),
            "kernel_span_ms_median": round(statistics.median(r[2] for r in runs), 2),
            "kernel": runs[-1][3][0], "launches": runs[-1][3][1]}


def pair(ctx, nbytes: int, verify: tuple, create: tuple) -> dict:
    """verify / create: (begin, end, the result every pass must give).  The two streams alternate."""
    runs = {"verify": [], "create": []}
    for step in range(WARMUP + RUNS):
        for name, (begin, end, want) in (("verify", verify), ("create", create)):
            r = one_pass(ctx, nbytes, begin, end)
            assert r[0] == want, "a timed %s stream's result is wrong" % name
            if step >= WARMUP:
                runs[name].append(r)
    out = {k: summary(v) for k, v in runs.items()}
    out["floor_GBps"] = out["verify"]["GBps_min"]            # the slowest of the verify stream's runs
    out["pass"] = out["create"]["GBps_median"] >= out["floor_GBps"]
    return out


def geometry_rows(ctx, name: str, lengths: list, L: int) -> dict:
    lay = make_layout(lengths, L)
    P, total = lay.n_pieces, lay.total_length
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    ctx.set_layout(total, L, P)
    ctx.fill_synthetic(SEED)
    plain = ctx.hash()                                   # tv_hash: the v1 stream's digests, the pads as the generator fills them
    ctx.v2_set_pieces(lay.piece_bytes, lay.tree_leaves, None)
    roots = ctx.v2_hash()                                # tv_v2_hash
    digests, roots_h = ctx.hybrid_hash()                 # tv_hybrid_hash
    assert roots_h == roots
    full = bytearray(b"\xff" * ((P + 7) // 8))
    if P % 8:
        full[-1] = (0xFF00 >> (P % 8)) & 0xFF
    full = bytes(full)
    pb, tl = np.asarray(lay.piece_bytes, dtype=np.uint32), np.asarray(lay.tree_leaves, dtype=np.uint32)
    row = {"name": name, "piece_length": L, "pieces": P, "files": len(lengths), "bytes": total, "budgets": {}}
    ctx.set_option(N.TV_OPT_RESIDENT, 0)
    ctx.set_option(N.TV_OPT_STREAM_CHUNK, 0)
    for tag, budget in (("default_1GiB", 0), ("quarter_GiB", 256 << 20)):
        ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
        legs = {}
        ctx.set_option(N.TV_OPT_STREAM_ROWS, 1)
        ctx.set_layout(total, L, P)
        ctx.set_digests(plain)
        legs["v1"] = pair(ctx, total, (ctx.stream_begin, ctx.stream_end, full),
                          (ctx.stream_hash_begin, ctx.stream_hash_end, plain))
        ctx.set_option(N.TV_OPT_STREAM_ROWS, 0)
        ctx.set_layout(total, L, P)
        legs["v2"] = pair(ctx, total, (lambda: ctx.v2_stream_begin(pb, tl, roots), ctx.stream_end, full),
                          (lambda: ctx.v2_stream_hash_begin(pb, tl), ctx.stream_hash_end, roots))
        ctx.set_digests(digests)
        legs["hybrid"] = pair(ctx, total,
                              (lambda: ctx.hybrid_stream_begin(pb, tl, roots), ctx.hybrid_stream_end, (full, full, full)),
                              (lambda: ctx.hybrid_stream_hash_begin(pb, tl), ctx.stream_hash_end, (digests, roots)))
        row["budgets"][tag] = legs
    ctx.set_option(N.TV_OPT_RESIDENT, 1)
    ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
    return row


def index(res: dict) -> str:
    lines = ["# Streamed creation next to streamed verify", "",
             "`bench.json`: `python tools/stream_hash_bench.py --out profiles/stream_hash/bench.json` (build %s; %d timed "
             "passes after %d warm-up, verify and creation alternating; GB/s = aligned bytes / wall time of begin .. end, "
             "the rows filled by the host generator on %d threads)." % (res["build_id"], res["runs"], res["warmup"],
                                                                         res["threads"]), "",
             "| geometry | budget | kind | verify median (min-max) | creation median (min-max) | creation >= slowest verify run |",
             "|---|---|---|---|---|---|"]
    for r in res["rows"]:
        for tag, legs in r["budgets"].items():
            for kind, p in legs.items():
                v, c = p["verify"], p["create"]
                lines.append("| %s | %s | %s | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %s |" % (
                    r["name"], tag, kind, v["GBps_median"], v["GBps_min"], v["GBps_max"], c["GBps_median"], c["GBps_min"],
                    c["GBps_max"], "yes" if p["pass"] else "no"))
    missed = ["%s / %s / %s" % (r["name"], tag, kind) for r in res["rows"] for tag, legs in r["budgets"].items()
              for kind, p in legs.items() if not p["pass"]]
    lines += ["", "Every creation output equalled tv_hash / tv_v2_hash / tv_hybrid_hash over the same bytes (asserted by the "
              "tool).  Expectation (the creation median is not below the slowest of the verify stream's runs): %s."
              % ("met on every row" if not missed else "NOT met on " + ", ".join(missed) + "; met on the other rows"), ""]
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"build_id": N.build_id(), "runs": RUNS, "warmup": WARMUP, "threads": N.cpu_share()}
    with N.Context(0) as ctx:
        ctx.set_option(N.TV_OPT_FILE_THREADS, N.cpu_share())
        res["rows"] = [geometry_rows(ctx, "cfg2", [16384 << 20], 1 << 20),
                       geometry_rows(ctx, "many_files", many_file_lengths(), 256 << 10)]
    res["pass"] = all(p["pass"] for r in res["rows"] for legs in r["budgets"].values() for p in legs.values())
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md"), "w") as f:
            f.write(index(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
