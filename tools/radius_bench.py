"""kernel.segment_radius against what a user runs without it: pad the clouds
and the query sets to the longest ones, torch.cdist (squared) into a (B, max_m,
max_n) distance tensor, mask by the radius (and the padding), a stable
descending sort of the mask whose first k indices are the first k members in
row order, the counts, the first-member padding and the id arithmetic back to
global rows. The kernel writes no distance tensor. Four shapes, points uniform
in the unit cube, D = 3:

  (a) sa1        32 clouds x 1024 points, 512 FPS centroids each, r 0.2, k 32
  (b) sa2        32 clouds x 512 points, 128 FPS centroids each, r 0.4, k 64
  (c) one-cloud  one cloud of 65,536 points, 16,384 queries (its first rows),
                 r 0.03877 (about 16 members), k 32
  (d) molecules  the neighbour lists of radius_graph: 256 segments of 30..50
                 rows, q = x without self, r 0.3, k 32 (both sides stop at the
                 lists; the boolean index that turns them into edges is the
                 same plumbing after either)

The two versions alternate in one process; each is warmed up, then every call
is timed with device events until each version has about WINDOW_MS of calls.
The report is the median and the 10th / 90th percentile per call. cdist rounds
differently from the kernel's fma chain, so the check at the timed size is the
share of queries whose lists and counts agree.

A GPU-only tool: it fails without a device.

  python tools/radius_bench.py [--out profiles/r42/radius/bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]

from tools.knn_bench import WINDOW_MS, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r42", "radius", "bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("radius_bench needs a ROCm device", file=sys.stderr)
        return 1
    import dgl
    from dgl import kernel
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    # (name, cloud sizes, queries per cloud (None: q = x, no self), r, k)
    shapes = [("sa1", [1024] * 32, 512, 0.2, 32), ("sa2", [512] * 32, 128, 0.4, 64),
              ("one-cloud", [65536], 16384, 0.03877, 32),
              ("molecules", rng.integers(30, 51, 256).tolist(), None, 0.3, 32)]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    results = []
    for name, sizes, m, r, k in shapes:
        B, N, max_n = len(sizes), sum(sizes), max(sizes)
        x = torch.rand(N, 3, generator=gen, device=dev)
        if m is None:
            q, qsizes, self_query = x, sizes, True
        elif B == 1:
            q, qsizes, self_query = x[:m].clone(), [m], False
        else:  # the centroids a set abstraction samples
            idx = dgl.geometry.farthest_point_sampler(x.view(B, max_n, 3), m)
            q = torch.gather(x.view(B, max_n, 3), 1, idx[:, :, None].expand(-1, -1, 3))
            q, qsizes, self_query = q.reshape(B * m, 3).contiguous(), [m] * B, False
        M, max_m = sum(qsizes), max(qsizes)
        segs, qsegs = kernel.SegmentOffsets(sizes=sizes), kernel.SegmentOffsets(sizes=qsizes)
        first = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]])).to(dev)

        def slots(szs, longest):  # where row i lands in the padded (B * longest) rows
            return torch.from_numpy(np.concatenate(
                [b * longest + np.arange(n) for b, n in enumerate(szs)])).to(dev)

        xpos, qpos = slots(sizes, max_n), slots(qsizes, max_m)
        real = torch.zeros(B * max_n, dtype=torch.bool, device=dev)
        real[xpos] = True
        r2 = float(np.float32(r) * np.float32(r))

        def ours():
            if self_query:
                return kernel.segment_radius(x, segs, r, k, exclude_self=True, pad_first=True)[:2]
            return kernel.segment_radius(x, segs, r, k, q, qsegs, pad_first=True)[:2]

        def composed():
            xp = x.new_zeros(B * max_n, 3)
            xp[xpos] = x
            qp = x.new_zeros(B * max_m, 3)
            qp[qpos] = q
            d = torch.cdist(qp.view(B, max_m, 3), xp.view(B, max_n, 3)).square_()
            inside = (d < r2) & real.view(B, 1, max_n)
            if self_query:
                inside &= ~torch.eye(max_n, dtype=torch.bool, device=dev)
            order = torch.sort(inside.to(torch.uint8), dim=2, descending=True,
                               stable=True).indices[:, :, :k]
            cnt = inside.sum(2).clamp_(max=k)
            order = torch.where(torch.arange(k, device=dev) < cnt[:, :, None], order,
                                order[:, :, :1])
            nbr = torch.where(cnt[:, :, None] > 0, order + first.view(B, 1, 1), -1)
            return nbr.view(B * max_m, k)[qpos], cnt.view(B * max_m)[qpos].int()

        timed = _timed([ours, composed])
        (na, ca), (nb, cb) = ours(), composed()
        same = ((na == nb).all(1) & (ca == cb)).float().mean().item()
        rec = {"shape": name, "segments": B, "rows": N, "queries": M, "r": r, "k": k,
               "mean_members_kept": ca.float().mean().item(),
               "hip": timed[0], "composed": timed[1],
               "speedup": timed[1]["median_ms"] / timed[0]["median_ms"],
               "composed_distance_tensor_mib": B * max_m * max_n * 4 / 2.0 ** 20,
               "queries_with_equal_lists": same}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del x, q, xpos, qpos, real
        torch.cuda.empty_cache()
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"window_ms": WINDOW_MS, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
