"""Fused GATv2 attention on the headline Reddit-shaped graph (the generator
bench.py uses: 232,965 nodes, 114,848,857 edges with the self-loops):
kernel.gatv2_attention at H x D = 8 x 16 and 8 x 64, forward alone and forward
+ backward. The composition it replaces cannot run at this size (its
E x H x D intermediate is 59 GB at 8 x 16), so the baselines are, at the same
commit,

    kernel.dot_attention(adj, fd, fs, fs)   two gathered rows per edge (k and
                                            v) where GATv2 gathers one
    kernel.gat_aggregate(adj, fs, el, er)   GATConv's fused aggregation, for
                                            context (its attention is static)

They alternate in one process; each is warmed up and then timed call by call
with device events, and the mean, the fastest and the slowest call are
reported.

The algorithmic bytes come from the shapes: the GATv2 forward reads fd and
writes out once (4 N H D each), gathers one fs row per edge (4 E H D, mostly
from cache) and reads the column ids (4 E) and the row pointer;
dot_attention's gathers 8 E H D.

The composition is run against the fused operator on a graph small enough for
it (--small-nodes nodes of --small-degree in-edges on average, the same
family): the time ratio and the largest |fused - composed| as a fraction of
the forward bound of tests/test_gatv2_attention.py, 1e-5 * sum_j a_j |fs_j|
(the fused operator run on attention from fs, values |fs|: dot-free, so the
composition's softmax with a u_mul_e sum over |fs|).

A GPU-only tool: it fails without a device.

  python tools/gatv2_bench.py [--out profiles/r37/gatv2_attention/bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd"), os.path.join(ROOT, "tools")]

from dot_attention_bench import _timed  # noqa: E402


def _no_grad(fn):
    import torch

    def run():
        with torch.no_grad():
            fn()
    return run


def _step(fn, leaves, dout):
    def run():
        for t in leaves:
            t.grad = None
        fn().backward(dout)
    return run


def _fmt(r):
    return "%.3f ms [%.3f, %.3f]" % (r["mean_ms"], r["min_ms"], r["max_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37", "gatv2_attention",
                                                  "bench.json"))
    ap.add_argument("--graph-scale", type=float, default=1.0,
                    help="testing knob: a smaller graph of the same family")
    ap.add_argument("--small-nodes", type=int, default=1 << 16)
    ap.add_argument("--small-degree", type=int, default=64)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("gatv2_bench needs a ROCm device", file=sys.stderr)
        return 1
    from dgl import data, kernel
    from dgl.kernel.gat import _gatv2_attention_composed
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def tensors(n, H, D):
        fs, fd, dout = (torch.randn(n, H, D, generator=gen, device=dev) for _ in range(3))
        attn = torch.randn(H, D, generator=gen, device=dev) * D ** -0.5
        for t in (fs, fd, attn):
            t.requires_grad_(True)
        return fs, fd, attn, dout

    # -- the composition against the fused operator, where the composition fits
    n = args.small_nodes
    src, dst, n = data.chung_lu(n, n * args.small_degree, data.REDDIT_MAX_OVER_MEAN, seed=0,
                                device=dev)
    adj = kernel.from_coo(n, n, dst, src, device=dev)
    small_edges = int(src.numel())
    del src, dst
    adj.bwd
    small = []
    for H, D in ((8, 16), (8, 64)):
        fs, fd, attn, dout = tensors(n, H, D)

        def fused():
            return kernel.gatv2_attention(adj, fs, fd, attn)

        def composed():
            return _gatv2_attention_composed(adj, fs, fd, attn, 0.2)

        f_fwd, c_fwd = _timed([_no_grad(fused), _no_grad(composed)])
        f_fb, c_fb = _timed([_step(fused, (fs, fd, attn), dout),
                             _step(composed, (fs, fd, attn), dout)])
        with torch.no_grad():
            a, b = fused(), composed()
            # sum_j a_j |fs_j|: the composition's attention over |fs|
            z = fs.index_select(0, adj.fwd.indices.long()) + fd.index_select(0, adj.fwd.row_ids())
            s = (torch.nn.functional.leaky_relu(z, 0.2) * attn).sum(-1)
            del z
            att = kernel.edge_softmax(adj, s, "dst", "slot")
            bound = 1e-5 * kernel.gspmm(adj, "u_mul_e", "sum", fs.abs(), att.unsqueeze(-1),
                                        edge_order="slot")
            ratio = float(((a - b).abs() / bound.clamp(min=1e-30)).max().item())
            del a, b, s, att, bound
        rec = {"H": H, "D": D, "nodes": n, "edges": small_edges,
               "fused_fwd": f_fwd, "composed_fwd": c_fwd, "fused_fwd_bwd": f_fb,
               "composed_fwd_bwd": c_fb, "speedup_fwd": c_fwd["mean_ms"] / f_fwd["mean_ms"],
               "speedup_fwd_bwd": c_fb["mean_ms"] / f_fb["mean_ms"],
               "composed_intermediate_bytes": 4 * small_edges * H * D,
               "max_diff_over_forward_bound": ratio}
        small.append(rec)
        print("small %dx%d fwd %s vs composed %s x%.2f | fwd+bwd %s vs %s x%.2f | diff / bound "
              "%.3g" % (H, D, _fmt(f_fwd), _fmt(c_fwd), rec["speedup_fwd"], _fmt(f_fb),
                        _fmt(c_fb), rec["speedup_fwd_bwd"], ratio), flush=True)
        del fs, fd, attn, dout
    del adj
    torch.cuda.empty_cache()

    # -- the Reddit-shaped graph: GATv2 against dot_attention and gat_aggregate
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
    results = []
    for H, D in ((8, 16), (8, 64)):
        fs, fd, attn, dout = tensors(n, H, D)
        el, er = (torch.randn(n, H, generator=gen, device=dev).requires_grad_(True)
                  for _ in range(2))

        def gatv2():
            return kernel.gatv2_attention(adj, fs, fd, attn)

        def dot():
            return kernel.dot_attention(adj, fd, fs, fs)

        def gat():
            return kernel.gat_aggregate(adj, fs, el, er, training=False)[0]

        fwd = _timed([_no_grad(gatv2), _no_grad(dot), _no_grad(gat)])
        fb = _timed([_step(gatv2, (fs, fd, attn), dout), _step(dot, (fs, fd), dout),
                     _step(gat, (fs, el, er), dout)])
        F = H * D
        unique = 2 * 4 * n * F + 4 * E + 8 * (n + 1)
        rec = {"H": H, "D": D, "nodes": n, "edges": E, "max_in_degree": adj.fwd.max_degree,
               "max_out_degree": adj.bwd.max_degree,
               "gatv2_fwd": fwd[0], "dot_attention_fwd": fwd[1], "gat_aggregate_fwd": fwd[2],
               "gatv2_fwd_bwd": fb[0], "dot_attention_fwd_bwd": fb[1],
               "gat_aggregate_fwd_bwd": fb[2],
               "fwd_vs_dot_attention": fwd[1]["mean_ms"] / fwd[0]["mean_ms"],
               "fwd_bwd_vs_dot_attention": fb[1]["mean_ms"] / fb[0]["mean_ms"],
               "fwd_bytes_streamed": unique, "gatv2_fwd_bytes_gathered": 4 * E * F,
               "dot_attention_fwd_bytes_gathered": 8 * E * F,
               "gatv2_fwd_gathered_gbs": 4 * E * F / fwd[0]["mean_ms"] / 1e6,
               "composition_intermediate_bytes": 4 * E * F,
               "bwd_workspace_bytes": kernel.gat._gatv2_workspace(adj, H, D, dev, True).numel()}
        results.append(rec)
        print("%dx%d fwd gatv2 %s | dot_attention %s x%.2f | gat_aggregate %s" %
              (H, D, _fmt(fwd[0]), _fmt(fwd[1]), rec["fwd_vs_dot_attention"], _fmt(fwd[2])),
              flush=True)
        print("%dx%d fwd+bwd gatv2 %s | dot_attention %s x%.2f | gat_aggregate %s" %
              (H, D, _fmt(fb[0]), _fmt(fb[1]), rec["fwd_bwd_vs_dot_attention"], _fmt(fb[2])),
              flush=True)
        del fs, fd, attn, dout, el, er
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"results": results, "small_graph": small}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
