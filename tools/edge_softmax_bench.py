"""Edge softmax on the headline Reddit-shaped graph (the generator bench.py
uses: 232,965 nodes, 114,848,857 edges with the self-loops, numbered
source-major): kernel.edge_softmax against what the package could do before
it, the composition

    xs = x[kernel.slot_permutation(adj)]            (edge_order="eid" only)
    m  = kernel.segment_reduce(xs, indptr, "max")
    e  = torch.exp(xs - m[row_ids])
    s  = kernel.segment_reduce(e, indptr, "sum")
    ys = e / s[row_ids]
    y[perm] = ys                                    (edge_order="eid" only)

at H = 8 and H = 1, norm_by="dst", both edge orders, forward alone and forward
+ backward. The two versions alternate in one process; each is warmed up and
then timed with device events over enough calls to fill about a second.

The algorithmic bytes come from the shapes: x read once and y written once
(4 E H each), the row pointer, and the edge ids where the kernel reads them
(8 E, edge_order="eid" on this numbering). The forward's bytes over its time
are quoted against the HBM rate a float4 copy reaches on the MI355X (6.29 TB/s
measured, 8.0 TB/s datasheet). The two versions' outputs are compared at the
timed size within the forward bound of tests/test_edge_softmax.py, 1e-5 of the
value, and the longest row against float64.

A GPU-only tool: it fails without a device.

  python tools/edge_softmax_bench.py [--out profiles/r31/edge_softmax_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]

HBM_COPY_GBS = 6290.0
WINDOW_MS = 1000.0


def _timed(fns, warmup=2):
    """Mean ms per call of each of ``fns``, alternated: warm-up, one call each
    to size the window, then rounds of one event-timed call each until every
    version has about WINDOW_MS of calls."""
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
    rounds = max(3, min(400, int(math.ceil(WINDOW_MS / max(min(first), 1e-3)))))
    rounds = min(rounds, max(3, int(math.ceil(2 * WINDOW_MS / max(first)))))
    tot = [0.0] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            tot[i] += once(fn)
    return [t / rounds for t in tot], rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31",
                                                  "edge_softmax_bench.json"))
    ap.add_argument("--graph-scale", type=float, default=1.0,
                    help="testing knob: a smaller graph of the same family")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("edge_softmax_bench needs a ROCm device", file=sys.stderr)
        return 1
    from dgl import data, kernel
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
    fwd = adj.fwd
    perm = kernel.slot_permutation(adj)
    uses_eid = fwd.slot_eid is not None
    rows = fwd.row_ids()
    segs = kernel.SegmentOffsets(offsets=fwd.indptr)
    max_deg = fwd.max_degree
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    results = []
    ok = True
    for H in (8, 1):
        x = (torch.randn(E, H, generator=gen, device=dev) *
             torch.randn(E, H, generator=gen, device=dev).exp()).clamp_(-8, 8)
        dy = torch.randn(E, H, generator=gen, device=dev)
        x.requires_grad_(True)
        for order in ("eid", "slot"):
            def ours():
                return kernel.edge_softmax(adj, x, "dst", order)

            def composed():
                xs = x[perm] if order == "eid" else x
                m = kernel.segment_reduce(xs, segs, "max")
                e = torch.exp(xs - m[rows])
                s = kernel.segment_reduce(e, segs, "sum")
                ys = e / s[rows]
                if order == "slot":
                    return ys
                y = torch.empty_like(ys)
                y[perm] = ys
                return y

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

            (t_f, tb_f), r_f = _timed([no_grad(ours), no_grad(composed)])
            (t_fb, tb_fb), r_fb = _timed([step(ours), step(composed)])
            x.grad = None
            with torch.no_grad():
                a, b = ours(), composed()
                diff = ((a - b).abs() / b).max().item()
                beyond = int(((a - b).abs() > 1e-5 * b).sum().item())
                # the longest row against float64
                r = int(torch.argmax(fwd.degrees()).item())
                k0, k1 = int(fwd.indptr[r].item()), int(fwd.indptr[r + 1].item())
                at = torch.arange(k0, k1, device=dev) if order == "slot" else perm[k0:k1]
                want = torch.softmax(x.detach()[at].double(), 0)
                hub = ((a[at].double() - want).abs() / want).max().item()
                del a, b
            eid_bytes = 8 * E if (order == "eid" and uses_eid) else 0
            nbytes = 2 * 4 * E * H + 8 * (n + 1) + eid_bytes
            gbs = nbytes / t_f / 1e6
            rec = {"H": H, "edge_order": order, "nodes": n, "edges": E, "max_degree": max_deg,
                   "kernel_reads_eid": bool(eid_bytes),
                   "hip_fwd_ms": t_f, "composed_fwd_ms": tb_f, "fwd_calls": r_f,
                   "hip_fwd_bwd_ms": t_fb, "composed_fwd_bwd_ms": tb_fb, "fwd_bwd_calls": r_fb,
                   "speedup_fwd": tb_f / t_f, "speedup_fwd_bwd": tb_fb / t_fb,
                   "fwd_algorithmic_bytes": nbytes, "hip_fwd_gbs": gbs,
                   "hip_fwd_frac_of_hbm_copy": gbs / HBM_COPY_GBS,
                   "max_rel_diff_vs_composed": diff, "elements_beyond_1e-5": beyond,
                   "longest_row_max_rel_err_vs_float64": hub}
            results.append(rec)
            print("H=%d %-4s fwd %.3f ms (%.0f GB/s, %.0f%% of copy) vs %.3f ms x%.2f | fwd+bwd "
                  "%.3f vs %.3f ms x%.2f | diff %.2g, hub %.2g"
                  % (H, order, t_f, gbs, 100 * gbs / HBM_COPY_GBS, tb_f, tb_f / t_f, t_fb, tb_fb,
                     tb_fb / t_fb, diff, hub), flush=True)
            if beyond or not hub <= 1e-5 or t_f >= tb_f or t_fb >= tb_fb:
                ok = False
        del x, dy
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"hbm_copy_gbs": HBM_COPY_GBS, "results": results, "ok": ok}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
