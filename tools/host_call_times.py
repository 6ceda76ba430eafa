"""Host time of the calls whose work is mostly on the host: wall clock around each call (the packing and planning that
runs before the call's first event is outside tv_last_timing's total), median of REPS after WARM warm-ups, no
reallocation in the timed calls.

    python tools/host_call_times.py [--out FILE]

One context, 4,096 pieces of 256 KiB filled by tv_fill_synthetic (the last piece short, so a list that holds it takes
the split launch order): tv_verify_list and tv_v2_verify_list at n = 1, 64, 1024 (and n = 1024 with the short last
piece), tv_v2_check_blocks over 64 pieces, tv_v2_verify, tv_hybrid_verify, tv_v2_set_pieces and tv_set_digests.  Every
result is checked (all pieces good).  To compare two builds run it once per library (TORRENT_VERIFY_LIB), alternating."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torrent_amd import _native as N  # noqa: E402

L, P, LEAF = 256 << 10, 4096, 16384
W = L // LEAF
REPS, WARM = 25, 3


def timed(ctx, call, want):
    """Wall clock around the call, and the library's own events inside it (tv_last_timing: the kernels; the call from
    its first event to its last) where the call records them (want is not None)."""
    us, kernel, total = [], [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        got = call()
        t1 = time.perf_counter()
        assert want is None or got == want
        if k >= WARM:
            us.append((t1 - t0) * 1e6)
            if want is not None:
                kms, tms = ctx.last_timing()
                kernel.append(kms * 1e3)
                total.append(tms * 1e3)
    row = {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1)}
    if kernel:
        row.update(kernel_median_us=round(statistics.median(kernel), 1), events_median_us=round(statistics.median(total), 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    total = L * (P - 1) + 1000
    pb, tl = [L] * (P - 1) + [1000], [W] * (P - 1) + [1]
    res = {"build_id": N.build_id(), "pieces": P, "piece_length": L, "reps": REPS, "rows": {}}
    with N.Context(0) as ctx:
        ctx.set_layout(total, L, P)
        ctx.fill_synthetic(3)
        ctx.v2_set_pieces(pb, tl, None)
        digests, roots = ctx.hybrid_hash()
        ones = bytes([0xFF] * (P // 8))
        rows = res["rows"]
        rows["tv_set_digests"] = timed(ctx, lambda: ctx.set_digests(digests), None)
        rows["tv_v2_set_pieces"] = timed(ctx, lambda: ctx.v2_set_pieces(pb, tl, roots), None)
        rows["tv_v2_verify"] = timed(ctx, ctx.v2_verify, ones)
        rows["tv_hybrid_verify"] = timed(ctx, ctx.hybrid_verify, (ones, ones, ones))
        for n, with_last in ((1, False), (64, False), (1024, False), (1024, True)):
            lst = list(range(0, P - 1, (P - 1) // n))[:n]
            if with_last:
                lst[n // 2] = P - 1
            name = f"n={n}" + (" with the short last piece" if with_last else "")
            ok = b"\x01" * n
            rows[f"tv_verify_list {name}"] = timed(ctx, lambda: ctx.verify_list(lst), ok)
            ent = ([pb[i] for i in lst], [tl[i] for i in lst], b"".join(roots[32 * i:32 * i + 32] for i in lst))
            rows[f"tv_v2_verify_list {name}"] = timed(ctx, lambda: ctx.v2_verify_list(lst, *ent), ok)
        lst = list(range(64))
        leaves = ctx.v2_leaf_hashes(lst, [L] * 64, [W] * 64)
        rows["tv_v2_check_blocks n=64"] = timed(ctx, lambda: ctx.v2_check_blocks(lst, [L] * 64, [W] * 64, leaves),
                                                b"\xff\xff" * 64)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
