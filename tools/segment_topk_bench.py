"""kernel.segment_topk against the composition a user writes without it: pad
every segment to the longest one with -inf, (B, max_n, F), and torch.topk along
dim 1; for sortby=-1, torch.topk on the padded key column and a gather of the
rows. Three shapes, one per path of csrc/segment_topk.hip:

  (a) molecules  256 graphs of 10..60 nodes, F = 64, k = 30   packed segments
  (b) lds        64 graphs of 1800..2048 nodes, F = 128, k = 64  one chunk each
  (c) one-long   one segment of 232,965 rows, F = 128, k = 64  chunks + merge

each for sortby=None and sortby=-1, forward alone and forward + backward. The
two versions alternate in one process; each is warmed up, then every call is
timed with device events until each version has about WINDOW_MS of calls. The
report is the median and the 10th / 90th percentile per call. Inputs are
normal draws (no ties), so the composition's values must equal the kernel's
wherever the slot is a row: checked at the timed size.

A GPU-only tool: it fails without a device.

  python tools/segment_topk_bench.py [--out profiles/r38/segment_topk/bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r38", "segment_topk",
                                                  "bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("segment_topk_bench needs a ROCm device", file=sys.stderr)
        return 1
    from dgl import kernel
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    shapes = [("molecules", rng.integers(10, 61, 256).tolist(), 64, 30),
              ("lds", rng.integers(1800, 2049, 64).tolist(), 128, 64),
              ("one-long", [232965], 128, 64)]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    results, ok = [], True
    for name, sizes, F, k in shapes:
        B, N, max_n = len(sizes), sum(sizes), max(sizes)
        segs = kernel.SegmentOffsets(sizes=sizes)
        x = torch.randn(N, F, generator=gen, device=dev).requires_grad_(True)
        dy = torch.randn(B, k, F, generator=gen, device=dev)
        # where row i of x lands in the padded (B * max_n, F) matrix
        pos = torch.from_numpy(np.concatenate(
            [b * max_n + np.arange(n) for b, n in enumerate(sizes)])).to(dev)
        for sortby in (None, -1):
            def ours():
                return kernel.segment_topk(x, segs, k, True, sortby)[0]

            def composed():
                pad = x.new_full((B * max_n, F), float("-inf"))
                pad[pos] = x
                pad = pad.view(B, max_n, F)
                if sortby is None:
                    return torch.topk(pad, k, dim=1)[0]
                idx = torch.topk(pad[:, :, sortby], k, dim=1)[1]
                return pad.gather(1, idx[:, :, None].expand(-1, -1, F))

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        fn()
                return run

            def step(fn):
                def run():
                    x.grad = None
                    fn().backward(dy)
                return run

            fwd = _timed([no_grad(ours), no_grad(composed)])
            fb = _timed([step(ours), step(composed)])
            x.grad = None
            with torch.no_grad():
                a, idx = kernel.segment_topk(x, segs, k, True, sortby)
                b = composed()
                live = (idx >= 0) if sortby is None else (idx >= 0)[:, :, None].expand_as(a)
                same = bool(torch.equal(a[live], b[live]))
            ok = ok and same
            rec = {"shape": name, "segments": B, "rows": N, "longest": max_n, "F": F, "k": k,
                   "sortby": sortby, "hip_fwd": fwd[0], "composed_fwd": fwd[1],
                   "hip_fwd_bwd": fb[0], "composed_fwd_bwd": fb[1],
                   "speedup_fwd": fwd[1]["median_ms"] / fwd[0]["median_ms"],
                   "speedup_fwd_bwd": fb[1]["median_ms"] / fb[0]["median_ms"],
                   "values_equal_composed": same}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        del x, dy, pos
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"window_ms": WINDOW_MS, "results": results, "ok": ok}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
