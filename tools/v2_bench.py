"""BitTorrent v2 throughput on one GPU: tv_v2_verify (SHA-256 merkle piece roots) on the cfg2 shape (one 16 GiB file,
1 MiB pieces) and on cfg4's piece geometry (4 MiB pieces, as many as fit), with three comparisons in the same run:
tv_verify (SHA-1) on the same resident bytes, hashlib SHA-256 on this host's cores, and the A/B of the leaf kernel's
lane mappings (TV_OPT_V2_MAP), alternated step by step.

    python tools/v2_bench.py [--steps 10] [--warmup 3] [--out profiles/v2/v2_bench.json]
    python tools/v2_bench.py --list [--parent-json FILE] [--out profiles/v2/list_latency.json]
    python tools/v2_bench.py --list-resident-only [--out FILE]
    python tools/v2_bench.py --stream [--out profiles/v2/stream_bench.json]

--list is the incremental-verify leg: the flush time of tv_v2_verify_list (one launch, the trees in LDS) for 1 / 64 /
4,096 pieces of 256 KiB and 1 / 64 / 1,024 pieces of 4 MiB, against (a) tv_verify_list (SHA-1) on the same bytes and
(b) the resident tv_v2_verify over the same pieces (leaf launch + one launch per level + finish).  Medians of 10 after
2 warm-ups.  --list-resident-only runs (b) alone and uses nothing newer than tv_v2_verify, so a copy of this tool
beside an older build of the package measures that build; --parent-json takes its output as (b).  Acceptance: at the
largest list of each size the fused kernel_ms is at most (b)'s times (b)'s own max / min spread (at least 1.05).

--stream is the streamed leg: cfg2's bytes (16,384 x 1 MiB of the synthetic payload) through the bounded pinned ring
as v2 pieces (tv_v2_stream_begin) and, in the same session over the same bytes and the same options (TV_OPT_STREAM_CHUNK
0, TV_OPT_RESIDENT_BUDGET 1 GiB), as v1 pieces (tv_stream_begin: its automatic columns; and with TV_OPT_STREAM_ROWS, whose
windows of whole pieces are the v2 stream's shape).  Two producers each: the host generator
(tv_stream_fill_synthetic) and a 256 MiB page-locked pool of 256 pieces repeated, DMA'd in place
(tv_stream_commit_from), as bench.py's cfg5 leg (not for v1's columns: a column request spans more pieces than the pool
holds).  The expected roots and digests come from the resident calls on the
same bytes (tv_fill_synthetic + tv_v2_hash / tv_hash).  Five timed runs after one warm-up.  Both paths are bound by
the same PCIe copies, so the acceptance is: the v2 stream's median GB/s is no lower than the MINIMUM of the v1 stream's
five runs (v1's own run-to-run spread as the margin), per producer, against the faster of the two v1 forms; the
bitfields are all ones, and exact with 1 % of the expected hashes corrupted.  One point under a 0.25 GiB budget is
recorded beside it (information, not a gate).

Times are the library's HIP events around the kernels (tv_last_timing); the shader clock is the clock probe's
(TV_OPT_CLOCK_PROBE).  The expected hashes come from tv_v2_hash, and a sample of pieces read back with tv_read is
checked against hashlib, so the timed verify is an exact one.  The only pass condition: the GPU beats the CPU figure.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torrent_amd import _native as N  # noqa: E402

LEAF = 16384
# 1,400 VALU per SHA-256 compression in the emitted ISA, 833 half-rate (~4 cycles per wave64
# instruction: v_alignbit, v_add3, v_perm) and 567 full-rate (~2): 4,466 SIMD cycles per 64 lanes x 64 B
CYCLES_PER_BLOCK = 833 * 4 + 567 * 2
R_VALU_256 = 1024 * 64 * 64 * 2.4e9 / CYCLES_PER_BLOCK / 1e9      # GB/s at 2.4 GHz


def merkle_root(data, width: int) -> bytes:
    row = [hashlib.sha256(data[o:o + LEAF]).digest() for o in range(0, len(data), LEAF)]
    row += [bytes(32)] * (width - len(row))
    while len(row) > 1:
        row = [hashlib.sha256(row[i] + row[i + 1]).digest() for i in range(0, len(row), 2)]
    return row[0]


def cpu_sha256(buf, threads: int) -> float:
    """GB/s of hashlib SHA-256 over the 16 KiB leaves of `buf` on `threads` threads (hashlib releases the GIL)."""
    mv = memoryview(buf)
    n = len(mv)
    part = -(-n // threads // LEAF) * LEAF

    def run(t):
        for o in range(t * part, min(n, (t + 1) * part), LEAF):
            hashlib.sha256(mv[o:o + LEAF]).digest()

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(run, range(threads)))          # warm-up
        t0 = time.perf_counter()
        list(ex.map(run, range(threads)))
        return n / (time.perf_counter() - t0) / 1e9


def shape(ctx, name: str, total: int, L: int, steps: int, warmup: int, sample: int, sha1: bool) -> dict:
    P = total // L
    W = L // LEAF
    ctx.set_layout(total, L, P)
    ctx.fill_synthetic(5)
    ctx.v2_set_pieces([L] * P, [W] * P, None)
    roots = ctx.v2_hash()
    # exactness on a sample of pieces read back from HBM
    buf = bytearray(L)
    for i in sorted({0, P - 1, *(P * k // sample for k in range(sample))}):
        ctx.read(i * L, buf)
        assert roots[32 * i:32 * i + 32] == merkle_root(bytes(buf), W), f"piece {i} differs from hashlib"
    ctx.v2_set_pieces([L] * P, [W] * P, roots)
    out = {"shape": name, "bytes": total, "piece_length": L, "pieces": P, "leaves": P * W, "mappings": {}}
    ms = {1: [], 2: []}
    khz = {1: [], 2: []}
    for step in range(warmup + steps):
        for m in (1, 2):                           # alternated: both see the same clock and neighbours
            ctx.set_option(N.TV_OPT_V2_MAP, m)
            bits = ctx.v2_verify()
            assert bits == b"\xff" * (P // 8), "v2_verify: not all ones"
            assert ctx.counter(N.TV_COUNTER_V2_MAP) == m
            if step >= warmup:
                ms[m].append(ctx.last_timing()[0])
                khz[m].append(ctx.last_clock_khz())
    ctx.set_option(N.TV_OPT_V2_MAP, 0)
    for m, label in ((1, "leaf_linear"), (2, "piece_major")):
        med = statistics.median(ms[m])
        clock = statistics.median(khz[m])
        gbs = total / med / 1e6
        out["mappings"][label] = {
            "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms[m]), 4), "kernel_ms_max": round(max(ms[m]), 4),
            "GBps": round(gbs, 1), "clock_khz": clock,
            "fraction_of_R_valu_2400": round(gbs / R_VALU_256, 4),
            "fraction_of_R_valu_live_clock": round(gbs / (R_VALU_256 * clock / 2.4e6), 4) if clock else None}
    ctx.v2_verify()
    out["default_mapping"] = ctx.counter(N.TV_COUNTER_V2_MAP)
    out["launches"] = ctx.last_kernel()[1]
    if sha1:
        ctx.set_digests(ctx.hash())
        t = []
        for step in range(warmup + steps):
            assert ctx.verify() == b"\xff" * (P // 8)
            if step >= warmup:
                t.append(ctx.last_timing()[0])
        med = statistics.median(t)
        out["sha1_tv_verify"] = {"kernel_ms_median": round(med, 4), "GBps": round(total / med / 1e6, 1),
                                 "kernel": ctx.last_kernel()[0]}
    return out


LIST_SHAPES = ((256 << 10, (1, 64, 4096)), (4 << 20, (1, 64, 1024)))
LIST_STEPS, LIST_WARMUP = 10, 2


def _stats(kernel, total) -> dict:
    return {"kernel_ms": round(statistics.median(kernel), 4), "total_ms": round(statistics.median(total), 4),
            "kernel_ms_min": round(min(kernel), 4), "kernel_ms_max": round(max(kernel), 4)}


def _timed(ctx, call, check) -> dict:
    kernel, total = [], []
    for step in range(LIST_WARMUP + LIST_STEPS):
        assert check(call()), "a timed call's result is wrong"
        if step >= LIST_WARMUP:
            k, t = ctx.last_timing()
            kernel.append(k)
            total.append(t)
    return _stats(kernel, total)


def list_legs(ctx, resident_only: bool) -> list:
    """Per (piece length, list length): n resident pieces of the synthetic payload, their roots from tv_v2_hash (one
    checked against hashlib), then the timed legs on those bytes."""
    out = []
    for L, counts in LIST_SHAPES:
        W = L // LEAF
        for n in counts:
            ctx.set_layout(n * L, L, n)
            ctx.fill_synthetic(5)
            ctx.v2_set_pieces([L] * n, [W] * n, None)
            roots = ctx.v2_hash()
            buf = bytearray(L)
            ctx.read((n - 1) * L, buf)
            assert roots[-32:] == merkle_root(bytes(buf), W), "the last piece differs from hashlib"
            ctx.v2_set_pieces([L] * n, [W] * n, roots)
            row = {"piece_length": L, "pieces": n, "serial_compressions": 257 + 2 * (W.bit_length() - 1)}
            all_ones = bytes([0xFF] * (n // 8)) + (bytes([0xFF00 >> (n % 8) & 0xFF]) if n % 8 else b"")
            row["resident_v2_verify"] = dict(_timed(ctx, ctx.v2_verify, lambda b: b == all_ones),
                                             launches=ctx.last_kernel()[1])
            if not resident_only:
                pieces = list(range(n))
                row["v2_verify_list"] = dict(
                    _timed(ctx, lambda: ctx.v2_verify_list(pieces, [L] * n, [W] * n, roots),
                           lambda ok: ok == b"\x01" * n),
                    launches=ctx.last_kernel()[1], workgroups=ctx.counter(N.TV_COUNTER_LAST_WORKGROUPS))
                ctx.set_digests(ctx.hash())
                row["sha1_verify_list"] = dict(_timed(ctx, lambda: ctx.verify_list(pieces), lambda ok: ok == b"\x01" * n),
                                               kernel=ctx.last_kernel()[0])
            out.append(row)
    return out


def list_main(a) -> int:
    res = {"build_id": N.build_id(), "steps": LIST_STEPS, "warmup": LIST_WARMUP}
    with N.Context(0) as ctx:
        res["rows"] = list_legs(ctx, a.list_resident_only)
    if a.list and a.parent_json:
        with open(a.parent_json) as f:
            parent = json.load(f)
        res["parent_build_id"] = parent["build_id"]
        by = {(r["piece_length"], r["pieces"]): r["resident_v2_verify"] for r in parent["rows"]}
        for r in res["rows"]:
            r["resident_v2_verify_parent_build"] = by[(r["piece_length"], r["pieces"])]
    if a.list:
        res["acceptance"] = []
        for L, counts in LIST_SHAPES:
            r = next(x for x in res["rows"] if x["piece_length"] == L and x["pieces"] == counts[-1])
            b = r.get("resident_v2_verify_parent_build") or r["resident_v2_verify"]
            spread = max(1.05, b["kernel_ms_max"] / b["kernel_ms_min"])
            res["acceptance"].append({
                "piece_length": L, "pieces": counts[-1], "fused_kernel_ms": r["v2_verify_list"]["kernel_ms"],
                "resident_kernel_ms": b["kernel_ms"], "resident_spread": round(spread, 4),
                "resident_from": "parent build" if "resident_v2_verify_parent_build" in r else "this build",
                "bound_ms": round(b["kernel_ms"] * spread, 4),
                "pass": r["v2_verify_list"]["kernel_ms"] <= b["kernel_ms"] * spread})
        for r in res["rows"]:
            if r["pieces"] == 1:   # reported, not gated
                r["single_piece_sha1_over_v2"] = round(r["sha1_verify_list"]["kernel_ms"] / r["v2_verify_list"]["kernel_ms"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


STREAM_RUNS, STREAM_WARMUP = 5, 1
POOL_PIECES = 256


def _stream_pass(ctx, begin, produce) -> tuple:
    """One streamed pass: (bitfield, seconds, requests, {phase: seconds}, kernel_ms, launches)."""
    ph = {"next_s": 0.0, "produce_commit_s": 0.0, "end_s": 0.0}
    t0 = time.perf_counter()
    begin()
    reqs = 0
    while True:
        ta = time.perf_counter()
        req = ctx.stream_next()
        tb = time.perf_counter()
        ph["next_s"] += tb - ta
        if not req.rows:
            break
        produce(req)
        ph["produce_commit_s"] += time.perf_counter() - tb
        reqs += 1
    ta = time.perf_counter()
    bits = ctx.stream_end()
    t1 = time.perf_counter()
    ph["end_s"] = t1 - ta
    return bits, t1 - t0, reqs, {k: round(v, 4) for k, v in ph.items()}, ctx.last_timing()[0], ctx.last_kernel()


def _stream_leg(ctx, total: int, begin, produce, want: bytes) -> dict:
    gbs, kms, last = [], [], None
    for run in range(STREAM_WARMUP + STREAM_RUNS):
        bits, el, reqs, ph, k_ms, kern = _stream_pass(ctx, begin, produce)
        assert bits == want, "a timed stream's bitfield is wrong"
        if run >= STREAM_WARMUP:
            gbs.append(total / el / 1e9)
            kms.append(k_ms)
            last = (reqs, ph, kern)
    return {"GBps_runs": [round(g, 2) for g in gbs], "GBps_median": round(statistics.median(gbs), 2),
            "GBps_min": round(min(gbs), 2), "GBps_max": round(max(gbs), 2),
            "kernel_span_ms_median": round(statistics.median(kms), 2), "requests": last[0], "last_run_phases_s": last[1],
            "kernel": last[2][0], "launches": last[2][1], "clock_khz": ctx.last_clock_khz()}


def _corrupt_every(hashes: bytes, width: int, step: int = 100) -> tuple:
    """Every `step`-th expected hash with one byte flipped -> (hashes, MSB-first bits with those pieces 0)."""
    n = len(hashes) // width
    h = bytearray(hashes)
    bits = bytearray(b"\xff" * (n // 8))
    for i in range(7, n, step):
        h[width * i + 3] ^= 0x55
        bits[i >> 3] &= ~(0x80 >> (i & 7)) & 0xFF
    return bytes(h), bytes(bits)


def stream_main(a) -> int:
    from tests import synth
    L, W, seed = 1 << 20, (1 << 20) // LEAF, 5
    P = (a.cfg2_gib << 30) // L
    total = P * L
    ones = b"\xff" * (P // 8)
    res = {"build_id": N.build_id(), "bytes": total, "piece_length": L, "pieces": P, "runs": STREAM_RUNS,
           "warmup": STREAM_WARMUP, "threads": N.cpu_share(), "legs": {}}
    with N.Context(0) as ctx:
        ctx.set_clock_probe(True)
        ctx.set_option(N.TV_OPT_FILE_THREADS, N.cpu_share())
        # the expected values, from the resident calls: the generated torrent, then the pool's 256 pieces
        ctx.set_layout(total, L, P)
        ctx.fill_synthetic(seed)
        ctx.v2_set_pieces([L] * P, [W] * P, None)
        roots = ctx.v2_hash()
        digests = ctx.hash()
        buf = bytearray(L)
        ctx.read((P - 1) * L, buf)
        assert roots[-32:] == merkle_root(bytes(buf), W), "the last piece differs from hashlib"
        pool = N.PinnedBuffer(POOL_PIECES * L)
        synth.fill_into(pool.mv, seed + 100, 0, threads=N.cpu_share())
        ctx.set_layout(POOL_PIECES * L, L, POOL_PIECES)
        ctx.stage(0, pool.mv)
        ctx.v2_set_pieces([L] * POOL_PIECES, [W] * POOL_PIECES, None)
        pool_roots = ctx.v2_hash() * (P // POOL_PIECES)
        pool_digests = ctx.hash() * (P // POOL_PIECES)
        # streamed-only from here on
        ctx.set_option(N.TV_OPT_RESIDENT, 0)
        ctx.set_option(N.TV_OPT_STREAM_CHUNK, 0)
        import numpy as np
        table = (np.full(P, L, dtype=np.uint32), np.full(P, W, dtype=np.uint32))   # (no list conversion in the timed begin)

        def gen(req):
            ctx.stream_fill_synthetic(req, seed)
            ctx.stream_commit(req)

        def from_pool(req):
            ctx.stream_commit_from(req, pool.mv, L, (req.piece % POOL_PIECES) * L + req.offset)

        def legs(tag: str, budget: int, v1_forms) -> None:
            ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, budget)
            ctx.set_option(N.TV_OPT_STREAM_ROWS, 0)
            ctx.set_layout(total, L, P)
            for name, prod, hs in (("generated", gen, roots), ("pinned_pool", from_pool, pool_roots)):
                res["legs"][f"v2_{name}{tag}"] = _stream_leg(
                    ctx, total, lambda: ctx.v2_stream_begin(table[0], table[1], hs), prod, ones)
                bad, want = _corrupt_every(hs, 32)
                bits = _stream_pass(ctx, lambda: ctx.v2_stream_begin(table[0], table[1], bad), prod)[0]
                assert bits == want, "1 % corrupted: the bitfield is not exact"
                res["legs"][f"v2_{name}{tag}"]["exact_with_1pct_corrupted"] = True
            for form, rows in v1_forms:
                ctx.set_option(N.TV_OPT_STREAM_ROWS, rows)
                ctx.set_layout(total, L, P)
                for name, prod, dg in (("generated", gen, digests), ("pinned_pool", from_pool, pool_digests)):
                    if name == "pinned_pool" and not rows:
                        continue      # (a column request spans 1,024 pieces: more than the pool holds in a row)
                    ctx.set_digests(dg)
                    res["legs"][f"v1_{form}_{name}{tag}"] = _stream_leg(ctx, total, ctx.stream_begin, prod, ones)
                    bad, want = _corrupt_every(dg, 20)
                    ctx.set_digests(bad)
                    assert _stream_pass(ctx, ctx.stream_begin, prod)[0] == want
            ctx.set_option(N.TV_OPT_STREAM_ROWS, 0)

        legs("", 1 << 30, (("columns", 0), ("rows", 1)))
        legs("_budget_quarter_GiB", 256 << 20, (("rows", 1),))
        ctx.set_option(N.TV_OPT_RESIDENT, 1)
        ctx.set_option(N.TV_OPT_RESIDENT_BUDGET, 0)
        pool.close()
    res["acceptance"] = []
    ok = True
    for name in ("generated", "pinned_pool"):
        v2 = res["legs"][f"v2_{name}"]
        forms = [f for f in ("columns", "rows") if f"v1_{f}_{name}" in res["legs"]]
        best = max(forms, key=lambda f: res["legs"][f"v1_{f}_{name}"]["GBps_median"])
        v1 = res["legs"][f"v1_{best}_{name}"]
        row = {"producer": name, "v2_GBps_median": v2["GBps_median"], "v1_GBps_min_of_runs": v1["GBps_min"],
               "v1_form": best,
               "pass": v2["GBps_median"] >= v1["GBps_min"]}
        ok = ok and row["pass"]
        res["acceptance"].append(row)
    res["pass"] = ok
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true", help="the streamed leg (see the module docstring)")
    ap.add_argument("--list", action="store_true", help="the incremental-verify leg (see the module docstring)")
    ap.add_argument("--list-resident-only", action="store_true", help="leg (b) of --list alone")
    ap.add_argument("--parent-json", default=None, help="--list: a --list-resident-only output to take (b) from")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cfg2-gib", type=int, default=16)
    ap.add_argument("--cfg4-gib", type=int, default=200)
    ap.add_argument("--cpu-gib", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if N.device_count() == 0:
        raise SystemExit("no HIP device visible: this measures the GPU")
    if a.list or a.list_resident_only:
        return list_main(a)
    if a.stream:
        return stream_main(a)
    res = {"R_valu_sha256_GBps_2400": round(R_VALU_256, 1), "cycles_per_block": CYCLES_PER_BLOCK,
           "build_id": N.build_id(), "steps": a.steps, "warmup": a.warmup, "shapes": []}
    with N.Context(0) as ctx:
        ctx.set_clock_probe(True)
        res["shapes"].append(shape(ctx, "cfg2", a.cfg2_gib << 30, 1 << 20, a.steps, a.warmup, 8, True))
        # the CPU figure: hashlib over bytes of the same payload, read back
        threads = N.cpu_share()
        host = bytearray(int(a.cpu_gib * (1 << 30)) // LEAF * LEAF)
        ctx.read(0, host)
        res["cpu_sha256"] = {"threads": threads, "bytes": len(host), "GBps": round(cpu_sha256(host, threads), 2)}
        del host
        gib = a.cfg4_gib                          # (0: cfg2 alone)
        while gib >= 8:                            # cfg4's piece geometry at whatever fits resident
            try:
                ctx.set_layout(gib << 30, 4 << 20, (gib << 30) >> 22)
                if ctx.counter(N.TV_COUNTER_WINDOW_PIECES) == 0:
                    break
            except N.NativeError as e:
                if e.code != N.TV_ERR_NOMEM:
                    raise
            gib //= 2
        if gib >= 8:
            res["shapes"].append(shape(ctx, f"cfg4_geometry_{gib}GiB", gib << 30, 4 << 20, a.steps, a.warmup, 4, True))
    best = max(m["GBps"] for m in res["shapes"][0]["mappings"].values())
    res["gpu_beats_cpu"] = best > res["cpu_sha256"]["GBps"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["gpu_beats_cpu"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
