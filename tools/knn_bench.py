"""kernel.segment_knn against what a user runs without it: pad the clouds to
the longest one, (B, max_n, D), torch.cdist (squared), mask the padding with
+inf, torch.topk(largest=False) and the id arithmetic back to global rows.
That composition makes a B x max_n x max_n distance tensor; the kernel writes
none. Four shapes:

  (a) clouds-d3    32 clouds x 1024 points, D = 3,  k = 20
  (b) clouds-d64   32 clouds x 1024 points, D = 64, k = 20
  (c) one-cloud    one cloud of 65,536 points, D = 3, k = 16
  (d) molecules    256 segments of 30..50 rows, D = 32, k = 8

The two versions alternate in one process; each is warmed up, then every call
is timed with device events until each version has about WINDOW_MS of calls.
The report is the median and the 10th / 90th percentile per call. Inputs are
normal draws (no ties); the two float32 formulas round differently, so the
check at the timed size is on sets: the share of rows whose k ids agree as a
set, and the largest difference of the sorted distances.

A GPU-only tool: it fails without a device.

  python tools/knn_bench.py [--out profiles/r40/knn/bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]

WINDOW_MS = 400.0


def _timed(fns, warmup=3):
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    first = [once(fn) for fn in fns]
    rounds = max(5, min(400, int(math.ceil(WINDOW_MS / max(max(first), 1e-3)))))
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ts[i].append(once(fn))
    out = []
    for t in ts:
        t.sort()
        out.append({"median_ms": t[len(t) // 2], "p10_ms": t[len(t) // 10],
                    "p90_ms": t[(9 * len(t)) // 10], "calls": len(t)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r40", "knn", "bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("knn_bench needs a ROCm device", file=sys.stderr)
        return 1
    from dgl import kernel
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    shapes = [("clouds-d3", [1024] * 32, 3, 20), ("clouds-d64", [1024] * 32, 64, 20),
              ("one-cloud", [65536], 3, 16),
              ("molecules", rng.integers(30, 51, 256).tolist(), 32, 8)]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    results = []
    for name, sizes, D, k in shapes:
        B, N, max_n = len(sizes), sum(sizes), max(sizes)
        segs = kernel.SegmentOffsets(sizes=sizes)
        x = torch.randn(N, D, generator=gen, device=dev)
        first = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]])).to(dev)
        # where row i of x lands in the padded (B * max_n, D) matrix, and which
        # padded rows are points
        pos = torch.from_numpy(np.concatenate(
            [b * max_n + np.arange(n) for b, n in enumerate(sizes)])).to(dev)
        real = torch.zeros(B * max_n, dtype=torch.bool, device=dev)
        real[pos] = True

        def ours():
            return kernel.segment_knn(x, segs, k)

        def composed():
            pad = x.new_zeros(B * max_n, D)
            pad[pos] = x
            pad = pad.view(B, max_n, D)
            d = torch.cdist(pad, pad).square_()
            d.masked_fill_(~real.view(B, 1, max_n), float("inf"))
            dist, idx = torch.topk(d, k, dim=2, largest=False)
            idx = idx + first.view(B, 1, 1)
            return idx.view(B * max_n, k)[pos], dist.view(B * max_n, k)[pos]

        fwd = _timed([ours, composed])
        (ia, da), (ib, db) = ours(), composed()
        same = (ia.sort(1).values == ib.sort(1).values).all(1).float().mean().item()
        rec = {"shape": name, "segments": B, "rows": N, "longest": max_n, "D": D, "k": k,
               "hip": fwd[0], "composed": fwd[1],
               "speedup": fwd[1]["median_ms"] / fwd[0]["median_ms"],
               "composed_distance_tensor_mib": B * max_n * max_n * 4 / 2.0 ** 20,
               "rows_with_equal_id_sets": same,
               "max_abs_distance_diff": (da - db.sort(1).values).abs().max().item()}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del x, pos, real
        torch.cuda.empty_cache()
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"window_ms": WINDOW_MS, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
