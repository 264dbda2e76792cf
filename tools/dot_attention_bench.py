"""Fused scaled dot-product graph attention on the headline Reddit-shaped
graph (the generator bench.py uses: 232,965 nodes, 114,848,857 edges with the
self-loops): kernel.dot_attention against the composition of the three
operators it fuses, at the same commit and in forward slot order (no edge-id
indirection, the composition's best case):

    s = g-SDDMM dot(q, k) * scale                   (E x H, with its backward)
    a = kernel.edge_softmax(adj, s, "dst", "slot")  (E x H)
    out = kernel.gspmm(adj, "u_mul_e", "sum", v, a, edge_order="slot")

at H x D = 8 x 16 and 8 x 64, forward alone and forward + backward. The
composition is the baseline, not the code under test. The two alternate in one
process; each is warmed up and then timed call by call with device events, and
the mean, the fastest and the slowest call are reported.

The algorithmic bytes come from the shapes: the forward reads q and writes out
once (4 N H D each), gathers a k row and a v row per edge (8 E H D, mostly from
cache) and reads the column ids (4 E) and the row pointer. The results check
is the largest ratio of |fused - composed| to the forward bound of
tests/test_dot_attention.py, 1e-5 * sum_j a_j |v_j| (the composition run on
|v|).

A GPU-only tool: it fails without a device.

  python tools/dot_attention_bench.py [--out profiles/r33/dot_attention/bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]

WINDOW_MS = 600.0


def _timed(fns, warmup=2):
    """Per version of ``fns`` the event-timed ms of each call, alternated:
    warm-up, one call each to size the window, then rounds of one call each
    until every version has about WINDOW_MS of calls."""
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
    rounds = max(3, min(200, int(math.ceil(WINDOW_MS / max(max(first), 1e-3)))))
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(once(fn))
    return [{"mean_ms": sum(t) / len(t), "min_ms": min(t), "max_ms": max(t), "calls": len(t)}
            for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33", "dot_attention",
                                                  "bench.json"))
    ap.add_argument("--graph-scale", type=float, default=1.0,
                    help="testing knob: a smaller graph of the same family")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("dot_attention_bench needs a ROCm device", file=sys.stderr)
        return 1
    from dgl import data, kernel
    from dgl.kernel.gat import _dot_attention_composed
    dev = torch.device("cuda", 0)
    if args.graph_scale == 1.0:
        src, dst, n = data.reddit_like(scale=1, seed=0, device=dev)
    else:
        src, dst, n = data.chung_lu(int(data.REDDIT_NODES * args.graph_scale),
                                    int(data.REDDIT_EDGES * args.graph_scale),
                                    data.REDDIT_MAX_OVER_MEAN, seed=0, device=dev)
    E = int(src.numel())
    adj = kernel.from_coo(n, n, dst, src, device=dev)
    del src, dst
    adj.bwd  # both CSRs built before anything is timed
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    results = []
    for H, D in ((8, 16), (8, 64)):
        q, k, v, dout = (torch.randn(n, H, D, generator=gen, device=dev) for _ in range(4))
        scale = D ** -0.5
        for t in (q, k, v):
            t.requires_grad_(True)

        def fused():
            return kernel.dot_attention(adj, q, k, v)

        def composed():
            return _dot_attention_composed(adj, q, k, v, scale, None)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        def step(fn):
            def run():
                q.grad = k.grad = v.grad = None
                fn().backward(dout)
            return run

        f_fwd, c_fwd = _timed([no_grad(fused), no_grad(composed)])
        f_fb, c_fb = _timed([step(fused), step(composed)])
        q.grad = k.grad = v.grad = None
        with torch.no_grad():
            a, b = fused(), composed()
            bound = 1e-5 * _dot_attention_composed(adj, q, k, v.abs(), scale, None)
            ratio = float(((a - b).abs() / bound.clamp(min=1e-30)).max().item())
            del a, b, bound
        F = H * D
        unique = 2 * 4 * n * F + 4 * E + 8 * (n + 1)
        gathered = 2 * 4 * E * F
        rec = {"H": H, "D": D, "nodes": n, "edges": E, "max_in_degree": adj.fwd.max_degree,
               "max_out_degree": adj.bwd.max_degree,
               "fused_fwd": f_fwd, "composed_fwd": c_fwd,
               "fused_fwd_bwd": f_fb, "composed_fwd_bwd": c_fb,
               "speedup_fwd": c_fwd["mean_ms"] / f_fwd["mean_ms"],
               "speedup_fwd_bwd": c_fb["mean_ms"] / f_fb["mean_ms"],
               "fwd_bytes_streamed": unique, "fwd_bytes_gathered": gathered,
               "fused_fwd_gathered_gbs": gathered / f_fwd["mean_ms"] / 1e6,
               "composed_edge_tensor_bytes": 4 * E * H,
               "max_diff_over_forward_bound": ratio}
        results.append(rec)
        print("%dx%d fwd %.3f ms [%.3f, %.3f] vs %.3f ms x%.2f | fwd+bwd %.3f [%.3f, %.3f] vs "
              "%.3f ms x%.2f | diff / bound %.3g"
              % (H, D, f_fwd["mean_ms"], f_fwd["min_ms"], f_fwd["max_ms"], c_fwd["mean_ms"],
                 rec["speedup_fwd"], f_fb["mean_ms"], f_fb["min_ms"], f_fb["max_ms"],
                 c_fb["mean_ms"], rec["speedup_fwd_bwd"], ratio), flush=True)
        del q, k, v, dout
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
