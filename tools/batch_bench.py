"""Measure the batch layout (tv_set_batch_layout / tv_batch_verify) against a launch per torrent.

    python tools/batch_bench.py [--out profiles/batch/bench.json] [--gib 16]

One session on one context, synthetic fill, kernel ms of tv_last_timing, median of 5:

  a  cfg2's 16 GiB cut into 256 torrents of 64 x 1 MiB pieces, as ONE batch launch
  b  the same torrents one by one: tv_set_layout + tv_verify each, the kernel ms summed
  c  the same bytes as the one uniform cfg2 torrent through tv_verify: the ceiling
  mixed  a library of about 16 GiB drawn from piece lengths 256 KiB / 1 MiB / 4 MiB, torrents of 1 .. 2,048 pieces, every
         torrent with a short last piece, as a batch and as the loop; every bitfield of the batch is checked against the
         loop's (some digests are corrupted, so the bits are not all ones)

Expectations, recorded and not tuned to: a <= 1.05 x c (the same twin grid over the same blocks by another route);
a below b (SHA-1 is serial in a piece: a launch per torrent pays one piece's serial hash each).  Digests come from
tv_hash of the same bytes on the GPU; a sample of them is checked against the CPU oracle.  Writes the JSON and the
index profiles/batch/README.md beside it; the resident path's A/B (bench.py on the parent commit and on this one,
alternating) is read from profiles/batch/bench_ab.json when that file is there."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torrent_amd import _native  # noqa: E402

MiB = 1 << 20
REPS = 5
SEED = 2


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def corrupt(digests: bytes, every: int) -> bytes:
    d = bytearray(digests)
    for i in range(every - 1, len(d) // 20, every):
        d[20 * i + 7] ^= 0x20
    return bytes(d)


def loop_leg(ctx, torrents, digests, reps: int = REPS):
    """A launch per torrent: (per-repetition sums of kernel ms, the bitfields of the last repetition)."""
    sums, bits = [], []
    for _ in range(reps):
        total, bits = 0.0, []
        for t, (tot, L, n) in enumerate(torrents):
            ctx.set_layout(tot, L, n)
            ctx.fill_synthetic(SEED + t)
            ctx.set_digests(digests[t])
            bits.append(bytes(ctx.verify()))
            total += ctx.last_timing()[0]
        sums.append(total)
    return sums, bits


def make_digests(ctx, torrents, every: int = 0):
    """tv_hash of every torrent's synthetic bytes (the loop's layout), optionally with every `every`-th digest bad."""
    out = []
    for t, (tot, L, n) in enumerate(torrents):
        ctx.set_layout(tot, L, n)
        ctx.fill_synthetic(SEED + t)
        d = ctx.hash()
        out.append(corrupt(d, every) if every else d)
    return out


def batch_leg(ctx, torrents, digests, reps: int = REPS):
    ctx.set_batch_layout([t[0] for t in torrents], [t[1] for t in torrents], [t[2] for t in torrents])
    for t in range(len(torrents)):
        ctx.batch_select(t)
        ctx.fill_synthetic(SEED + t)
        ctx.set_digests(digests[t])
    ms, bits = [], []
    ctx.batch_verify()                                   # warm-up
    for _ in range(reps):
        bits = [bytes(b) for b in ctx.batch_verify()]
        ms.append(ctx.last_timing()[0])
    return ms, bits, {"kernel": ctx.last_kernel()[0], "workgroups": ctx.counter(_native.TV_COUNTER_LAST_WORKGROUPS)}


def check_sample(torrents, digests) -> int:
    """A few torrents' first and last digests against the CPU oracle's synthetic payload."""
    import hashlib

    from oracle import oracle
    oracle.build()
    checked = 0
    for t in sorted({0, len(torrents) // 2, len(torrents) - 1}):
        tot, L, n = torrents[t]
        for i in {0, n - 1}:
            ln = tot - i * L if i == n - 1 else L
            want = hashlib.sha1(bytes(oracle.synth_fill(SEED + t, i * L, ln))).digest()
            assert digests[t][20 * i:20 * i + 20] == want, (t, i)
            checked += 1
    return checked


def mixed_library(target: int):
    rng = random.Random(16)
    out, total = [], 0
    while total < target:
        L = rng.choice([256 << 10, MiB, 4 * MiB])
        n = rng.randrange(1, 2049)
        n = max(1, min(n, (target - total) // L + 1))
        tot = (n - 1) * L + rng.randrange(1, L)          # every torrent has a short last piece
        out.append((tot, L, n))
        total += tot
    return out


def write_readme(res: dict, folder: str) -> None:
    """profiles/batch/README.md from bench.json (and bench_ab.json, when present)."""
    def row(name):
        r = res[name]
        return f"{r['median']:.2f} (min {r['min']:.2f}, max {r['max']:.2f})"
    met = lambda ok: "met" if ok else "NOT met"  # noqa: E731
    m = res["mixed"]
    lines = [
        "# profiles/batch", "",
        "| file | what |", "|---|---|",
        "| `bench.json` | `python tools/batch_bench.py`: one session on one context, synthetic fill, kernel ms of "
        "`tv_last_timing`, median of 5 (the loop of the mixed library: 3). Legs a / b / c are cfg2's bytes as a batch of "
        f"{16 * res['gib']} torrents of 64 x 1 MiB, as a launch per torrent, and as the one uniform torrent; `mixed` is a "
        "library drawn from 256 KiB / 1 MiB / 4 MiB pieces, every torrent with a short last piece, whose batch "
        "bitfields are checked against the loop's |",
        "| `bench_ab.json` | `bench.py --gpus 1` on the parent commit and on this one, alternating, 5 runs each, in one "
        "session: the resident single-torrent path |",
        "| `group_tests.md` | the tests of the batch launch's mixed-length groups (`tests/batch_groups.py`, "
        "`tests/test_batch_groups_shapes.py`, `tests/test_gpu_batch_groups.py`): what they reach, their wall time, and "
        "which tests two deliberate edits of the digest-update mask fail; hand-written, repeated at the end of this file |",
        "",
        f"Build `{res['build']}`, {res['gib']} GiB per leg.", "",
        "| leg | kernel ms | expectation |", "|---|---|---|",
        f"| a: {16 * res['gib']} torrents, one batch launch ({res['a_batch']['workgroups']} workgroups) | {row('a_batch')} | "
        f"a / c = {res['a_over_c']:.3f} against the bound 1.05: {met(res['a_over_c_met'])} |",
        f"| b: the same torrents, a launch each (summed) | {row('b_loop')} | a below b: {met(res['a_below_b_met'])}, "
        f"b / a = {res['b_over_a']:.1f} |",
        f"| c: the one uniform torrent, `tv_verify` ({res['c_uniform']['workgroups']} workgroups) | {row('c_uniform')} | "
        "the ceiling |",
        f"| mixed library, batch: {m['torrents']} torrents, {m['pieces']} pieces, {m['bytes'] / 2 ** 30:.2f} GiB "
        f"({m['batch']['workgroups']} workgroups, kernel form {m['batch']['kernel']}) | "
        f"{m['batch']['median']:.2f} (min {m['batch']['min']:.2f}, max {m['batch']['max']:.2f}) | every bitfield equals "
        "the loop's |",
        f"| mixed library, a launch per torrent (summed) | {m['loop']['median']:.2f} (min {m['loop']['min']:.2f}, max "
        f"{m['loop']['max']:.2f}) | loop / batch = {m['loop_over_batch']:.1f} |", ""]
    ab_path = os.path.join(folder, "bench_ab.json")
    if os.path.exists(ab_path):
        ab = json.load(open(ab_path))
        p, b = ab["parent_GBps"], ab["branch_GBps"]
        ok = statistics.median(b) >= min(p)
        lines += ["The resident single-torrent path (`bench.py --gpus 1`, cfg2, verified GB/s, the runs alternating):", "",
                  "| build | runs | median | slowest |", "|---|---|---|---|",
                  f"| parent `{ab['parent_build']}` | {', '.join(f'{v:.1f}' for v in p)} | {statistics.median(p):.1f} | {min(p):.1f} |",
                  f"| this commit `{ab['branch_build']}` | {', '.join(f'{v:.1f}' for v in b)} | {statistics.median(b):.1f} | {min(b):.1f} |",
                  "", f"This commit's median is not below the parent's slowest run: {met(ok)}.", ""]
    notes_path = os.path.join(folder, "group_tests.md")    # hand-written: the tests of the mixed-length groups
    if os.path.exists(notes_path):
        lines += open(notes_path).read().rstrip("\n").split("\n") + [""]
    with open(os.path.join(folder, "README.md"), "w") as f:
        f.write("\n".join(lines))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench.json"))
    ap.add_argument("--gib", type=int, default=16, help="bytes of each leg, GiB (16: cfg2)")
    ap.add_argument("--readme-only", action="store_true", help="rewrite README.md from the JSON files, measure nothing")
    a = ap.parse_args()
    if a.readme_only:
        write_readme(json.load(open(a.out)), os.path.dirname(a.out))
        return 0
    nt = 16 * a.gib                                       # 256 torrents of 64 x 1 MiB at 16 GiB
    same = [(64 * MiB, MiB, 64)] * nt
    res = {"build": _native.build_id(), "gib": a.gib, "reps": REPS}
    with _native.Context(0) as ctx:
        # c: the one uniform torrent
        ctx.set_layout(nt * 64 * MiB, MiB, nt * 64)
        ctx.fill_synthetic(SEED)
        ctx.set_digests(ctx.hash())
        ctx.verify()
        c_ms = []
        for _ in range(REPS):
            bits = ctx.verify()
            c_ms.append(ctx.last_timing()[0])
        assert bits == b"\xff" * (nt * 8)
        res["c_uniform"] = dict(med(c_ms), kernel=ctx.last_kernel()[0],
                                workgroups=ctx.counter(_native.TV_COUNTER_LAST_WORKGROUPS))
        # b, then a, on the same torrents and digests
        digests = make_digests(ctx, same, every=37)
        res["digests_checked_against_oracle"] = check_sample(same, digests)
        b_ms, b_bits = loop_leg(ctx, same, digests)
        a_ms, a_bits, a_info = batch_leg(ctx, same, digests)
        assert a_bits == b_bits and any(x != b"\xff" * 8 for x in a_bits)
        res["a_batch"] = dict(med(a_ms), **a_info)
        res["b_loop"] = med(b_ms)
        res["a_over_c"] = statistics.median(a_ms) / statistics.median(c_ms)
        res["a_over_c_bound"] = 1.05
        res["a_over_c_met"] = res["a_over_c"] <= 1.05
        res["b_over_a"] = statistics.median(b_ms) / statistics.median(a_ms)
        res["a_below_b_met"] = statistics.median(a_ms) < statistics.median(b_ms)
        # the mixed library
        lib = mixed_library(a.gib << 30)
        digests = make_digests(ctx, lib, every=53)
        l_ms, l_bits = loop_leg(ctx, lib, digests, reps=3)
        m_ms, m_bits, m_info = batch_leg(ctx, lib, digests)
        assert m_bits == l_bits and sum(b.count(b"\xff") for b in m_bits) > 0
        res["mixed"] = {"torrents": len(lib), "pieces": sum(t[2] for t in lib), "bytes": sum(t[0] for t in lib),
                        "by_piece_length": {str(L): sum(1 for t in lib if t[1] == L) for L in (256 << 10, MiB, 4 * MiB)},
                        "batch": dict(med(m_ms), **m_info), "loop": med(l_ms),
                        "loop_over_batch": statistics.median(l_ms) / statistics.median(m_ms),
                        "bitfields_equal": True}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_readme(res, os.path.dirname(a.out))
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print(json.dumps({"a": res["a_batch"]["median"], "b": res["b_loop"]["median"], "c": res["c_uniform"]["median"],
                      "mixed_batch": res["mixed"]["batch"]["median"], "mixed_loop": res["mixed"]["loop"]["median"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
