"""DGLGraph.subgraph on the Reddit-shaped bench graph: the device route (node
ids on the GPU, csrc/induced_subgraph.hip) against the host route (the native
index's VertexSubgraph), each timed up to a ready device adjacency of the
subgraph.

  (a) device: GraphIndex.node_subgraph_device(ids on the GPU) -> the
      subgraph's forward CSR on the GPU (built from the device edge list);
  (b) host:   GraphIndex.node_subgraph(ids on the host) -> the same CSR
      (native VertexSubgraph, one upload of the edge list, the same builder).

Random node sets of 1 %, 10 % and 50 % of the nodes. Every figure is the
median over the repeats after a warm-up. ``wall_ms`` is host time from the
call to the end of a stream synchronize (the device route's host read is part
of the call, so wall clock is the honest figure for both); ``device_ms`` is the
span between two events recorded around route (a). The parent's adjacency and
its source-major CSR are built before anything is timed, as they are after a
training step's backward pass. Both routes must give the same edges: the tool
checks the parent edge ids before timing.

  python tools/subgraph_bench.py [--scale 1.0] [--out profiles/r08/subgraph.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.01, 0.10, 0.50)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="graph size as a fraction of Reddit")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3,
                    help="repeats of the host route (seconds per call at 50 %%)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch

    import dgl
    from dgl import data, kernel

    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    src, dst, n = data.reddit_like(scale=args.scale, seed=0, device=dev)
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src.cpu(), dst.cpu())
    del src, dst
    gi = g._graph
    adj = gi.adjacency(dev)
    bwd = adj.bwd
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    result = {"tool": "subgraph_bench", "nodes": n, "edges": gi.number_of_edges(),
              "chunk": kernel.SUBGRAPH_CHUNK, "graph_build_s": round(build_s, 2),
              "warmup": args.warmup, "reps": args.reps, "host_reps": args.host_reps,
              "cases": []}
    gen = torch.Generator().manual_seed(1)
    for frac in FRACTIONS:
        k = max(1, int(n * frac))
        sel_host = torch.randperm(n, generator=gen)[:k].contiguous()
        sel_dev = sel_host.to(dev)
        deg = (bwd.indptr[1:] - bwd.indptr[:-1])[sel_dev]
        slots = int(deg.sum())

        def device_route():
            sgi = gi.node_subgraph_device(sel_dev)
            sgi.adjacency(dev)
            return sgi

        def host_route():
            sgi = gi.node_subgraph(sel_host)
            sgi.adjacency(dev)
            return sgi

        a, b = device_route(), host_route()  # also the first warm-up of both
        torch.cuda.synchronize()
        same = (a.number_of_edges() == b.number_of_edges() and
                torch.equal(a.induced_edges.cpu(), b.induced_edges) and
                torch.equal(a.adjacency(dev).fwd.indices, b.adjacency(dev).fwd.indices))
        m = a.number_of_edges()
        del a, b

        def timed(fn, warmup, reps, events):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            wall, span = [], []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                if events:
                    e0.record()
                fn()
                if events:
                    e1.record()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t) * 1e3)
                if events:
                    span.append(e0.elapsed_time(e1))
            return _median(wall), (_median(span) if events else None), [min(wall), max(wall)]

        dev_wall, dev_span, dev_range = timed(device_route, args.warmup, args.reps, True)
        host_wall, _, host_range = timed(host_route, 0, args.host_reps, False)
        case = {"fraction": frac, "selected": k, "candidate_slots": slots, "sub_edges": m,
                "routes_agree": bool(same), "device_wall_ms": round(dev_wall, 3),
                "device_ms": round(dev_span, 3), "host_wall_ms": round(host_wall, 3),
                "host_over_device": round(host_wall / dev_wall, 2),
                "device_wall_min_max_ms": [round(x, 3) for x in dev_range],
                "host_wall_min_max_ms": [round(x, 3) for x in host_range]}
        result["cases"].append(case)
        print("# %4.0f%%: %d nodes, %d slots, %d edges | device %.3f ms wall (%.3f ms on the "
              "stream) | host %.1f ms wall | x%.1f | agree=%s"
              % (frac * 100, k, slots, m, dev_wall, dev_span, host_wall, host_wall / dev_wall,
                 same), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(c["routes_agree"] for c in result["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
