"""Interleaved A/B of two builds of libtorrent_verify.so under bench.py (the flagship cfg2 step), one GPU.

    python tools/ab_bench_pairs.py <parent.so> <branch.so> [--pairs 5] [--steps 20] [--warmup 5] [--out FILE]

Runs `bench.py --gpus 1` `pairs` times per library, alternating parent, branch, parent, ... (one process per
run; the library is chosen with TORRENT_VERIFY_LIB), and takes roofline.kernel_ms_median and value from
each result line.  The gate: the noise yardstick is the PARENT's own spread, max - min of its
kernel_ms_median over the runs; the branch counts as faster if its slowest median is below the parent's
fastest AND the mean improvement is at least 3 x that spread.  Every run must report bitfield_exact.
Prints (and with --out writes) one JSON record with the runs and the verdict."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(lib, steps, warmup):
    env = dict(os.environ, TORRENT_VERIFY_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError(f"bench.py failed on {lib} (exit {r.returncode}): {r.stderr[-600:]}")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if not out["bitfield_exact"]:
        raise RuntimeError(f"bitfield not exact on {lib}")
    return {"kernel_ms_median": out["roofline"]["kernel_ms_median"], "kernel_ms_avg": out["roofline"]["kernel_ms_avg"],
            "value": out["value"], "ms_per_step": out["ms_per_step"], "clock_ghz": out["roofline"]["clock_ghz"]}


def verdict(parent, branch):
    pm = [x["kernel_ms_median"] for x in parent]
    bm = [x["kernel_ms_median"] for x in branch]
    spread = max(pm) - min(pm)
    gain = statistics.mean(pm) - statistics.mean(bm)
    return {"parent_median_min_max": [min(pm), max(pm)], "branch_median_min_max": [min(bm), max(bm)],
            "parent_spread_ms": round(spread, 4), "mean_improvement_ms": round(gain, 4),
            "mean_improvement_pct": round(100 * gain / statistics.mean(pm), 3),
            "parent_value_mean": round(statistics.mean(x["value"] for x in parent), 2),
            "branch_value_mean": round(statistics.mean(x["value"] for x in branch), 2),
            "branch_slowest_below_parent_fastest": max(bm) < min(pm),
            "improvement_at_least_3x_spread": gain >= 3 * spread,
            "gain": max(bm) < min(pm) and gain >= 3 * spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    runs = {"parent": [], "branch": []}
    for i in range(a.pairs):
        for name, lib in (("parent", a.parent), ("branch", a.branch)):
            rec = run(lib, a.steps, a.warmup)
            runs[name].append(rec)
            print(json.dumps(dict(rec, pair=i, build=name)), file=sys.stderr, flush=True)
    rec = {"workload": "bench.py --gpus 1 (cfg2)", "steps": a.steps, "warmup": a.warmup, "pairs": a.pairs,
           "parent": runs["parent"], "branch": runs["branch"], "verdict": verdict(runs["parent"], runs["branch"])}
    txt = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
