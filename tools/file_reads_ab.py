"""File-read paths of two builds of libtorrent_verify.so, alternating in separate processes (TORRENT_VERIFY_LIB).

    python tools/file_reads_ab.py <dir> <parent.so> <branch.so> [--pairs 5] [--out FILE]

One 16 GiB file of 1 MiB pieces (tools/storage_paths_bench.write_layout "single16", written once under <dir>, 1 % of
the digests corrupted) through verify_files staged (tv_stage_file_table) and streamed under a 0.5 GiB budget
(tv_stream_file_table): `pairs` alternations parent, branch, ... on a warm page cache (best of 3 calls per process),
then `pairs` on files evicted before every call (tools/fsutil.drop_cache; the residency left is recorded).  Every
bitfield is checked against hashlib's.  Per leg: the parent's runs and min-max, the branch's runs and median, and
whether that median lies inside the parent's range.  This process never opens the GPU; it stops at the first child
that fails."""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LEGS = [("verify_files", {}), ("verify_files stream", {"stream": True, "budget": 512 << 20})]


def child(pk, cache):
    import fsutil
    from torrent_amd import _native, verify_files
    root, info, expect, paths = pickle.load(open(pk, "rb"))
    cold = cache == "cold"
    os.chdir(root)
    out = {"cache": cache, "build_id": _native.build_id(), "legs": {}}
    for leg, kw in LEGS:
        best, res, exact = None, None, True
        for _ in range(1 if cold else 3):
            res = fsutil.drop_cache(paths) if cold else fsutil.resident(paths)
            t0 = time.perf_counter()
            bf = verify_files(info, root, **kw)
            el = time.perf_counter() - t0
            exact = exact and bytes(bf) == expect
            best = el if best is None else min(best, el)
        out["legs"][leg] = {"best_s": round(best, 4), "gbps": round(info.length / best / 1e9, 2), "exact": exact,
                            "resident": round(res, 4)}
    print(json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(*sys.argv[2:4])
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    from storage_paths_bench import write_layout
    root = os.path.join(a.dir, "single16")
    info, expect, paths = write_layout("single16", root)
    pk = os.path.join(a.dir, "single16.pickle")
    pickle.dump((root, info, expect, paths), open(pk, "wb"))
    runs = []
    try:
        for cache in ("warm", "cold"):
            for k in range(a.pairs):
                for which, lib in (("parent", a.parent), ("branch", a.branch)):
                    env = dict(os.environ, TORRENT_VERIFY_LIB=os.path.abspath(lib))
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pk, cache], env=env,
                                       capture_output=True, text=True, timeout=600)
                    if r.returncode:
                        raise RuntimeError(f"{which} ({cache}) failed, exit {r.returncode}: {r.stderr[-800:]}")
                    runs.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), lib=which, pair=k))
    finally:
        for p in paths + [pk]:
            if os.path.exists(p):
                os.unlink(p)
    summary = {}
    for cache in ("warm", "cold"):
        for leg, _ in LEGS:
            p, b = ([r["legs"][leg]["gbps"] for r in runs if r["cache"] == cache and r["lib"] == w]
                    for w in ("parent", "branch"))
            summary[f"{cache}: {leg}"] = {"parent_gbps": p, "parent_min_max": [min(p), max(p)], "branch_gbps": b,
                                          "branch_median": statistics.median(b),
                                          "branch_median_inside_parent_range": min(p) <= statistics.median(b) <= max(p)}
    rec = {"layout": "single16 (one 16 GiB file, 1 MiB pieces)", "pairs": a.pairs,
           "build_ids": {w: next(r["build_id"] for r in runs if r["lib"] == w) for w in ("parent", "branch")},
           "exact": all(l["exact"] for r in runs for l in r["legs"].values()), "summary": summary, "runs": runs}
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}, indent=1))
    if a.out:
        json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
