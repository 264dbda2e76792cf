"""DGLGraph.line_graph at the sizes its users run: the device route
(csrc/line_graph.hip) against the host route (the native index's line_graph),
each timed from the call to a ready forward CSR of the line graph on the GPU.

  (a) device: GraphIndex.line_graph_device(ctx) -> adjacency(ctx) built from
      the device edge list;
  (b) host:   GraphIndex.line_graph() -> adjacency(ctx): the native
      line_graph, one upload of the edge list, the same builder.

Workloads, generated from a seed:
  trees_40, trees_4000  a JTNN-like batch of random trees of 10 to 40 nodes,
                        both directions of every tree edge;
  sbm                   two equal blocks, 10^5 nodes, average degree 10;
  skewed                data.reddit_like at --scale, halved until the line
                        graph's edge list (16 M bytes, M read from the count
                        stage) is under a quarter of the free device memory
                        and M is at most --max-line-edges, which keeps the
                        host route to seconds per call.

Every figure is the median over the repeats after a warm-up, with min and max
beside it. ``wall_ms`` is host time from the call to the end of a stream
synchronize (the device route's host read is part of the call); ``device_ms``
is the span between two events recorded around route (a). The parent's
adjacency and its source-major CSR are built before anything is timed. Both
routes must give the same edges: the tool checks that before timing.
``count_wall_ms`` is stage A alone with its host read, on the host clock.
``fill`` times stage B alone between two events and divides its algorithmic
bytes by that: 16 M written, 8 M of eid, 4 K of indices when not backtracking,
and cand_ptr once (8 (E + 1)).

  python tools/line_graph_bench.py [--out profiles/r13/line_graph/line_graph.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def tree_batch(num_trees, rng):
    """(n, src, dst) of a batch of random trees: node j > 0 of a tree hangs
    under a random earlier node; both directions of every tree edge."""
    src, dst, off = [], [], 0
    for size in rng.integers(10, 41, num_trees):
        child = np.arange(1, size)
        parent = (rng.random(size - 1) * child).astype(np.int64)
        src += [parent + off, child + off]
        dst += [child + off, parent + off]
        off += int(size)
    return off, np.concatenate(src), np.concatenate(dst)


def sbm_like(n, avg_degree, rng, p_in=0.8):
    """(n, src, dst): n * avg_degree / 2 random pairs in both directions, a
    pair inside one of two equal blocks with probability p_in."""
    pairs = n * avg_degree // 2
    half = n // 2
    u = rng.integers(0, n, pairs)
    inside = rng.random(pairs) < p_in
    v = rng.integers(0, half, pairs) + np.where(inside, u >= half, u < half) * half
    return n, np.concatenate([u, v]), np.concatenate([v, u])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0 / 64,
                    help="first size of the skewed graph as a fraction of Reddit")
    ap.add_argument("--max-line-edges", type=float, default=4e8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch

    import dgl
    from dgl import data, kernel

    dev = torch.device("cuda", 0)
    bt = False  # as the line-graph network and JTNN call it
    free0 = torch.cuda.mem_get_info(dev)[0]

    def graph_of(n, src, dst):
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(n)
        g.add_edges(torch.as_tensor(src), torch.as_tensor(dst))
        gi = g._graph
        gi.adjacency(dev).bwd
        torch.cuda.synchronize()
        return g

    def counted(gi):
        s, d, _ = gi._id_order()
        s, d = s.to(dev), d.to(dev)
        ws, status = kernel.line_graph_count(gi.adjacency(dev).bwd, s, d, bt)
        return s, d, ws, status

    def skewed():
        scale = args.scale
        while True:
            src, dst, n = data.reddit_like(scale=scale, seed=0, device=dev)
            g = graph_of(n, src.cpu(), dst.cpu())
            del src, dst
            m = counted(g._graph)[3][0]
            free = torch.cuda.mem_get_info(dev)[0]
            print("# skewed: scale %.6f -> M = %d" % (scale, m), file=sys.stderr, flush=True)
            if 16 * m < free // 4 and m <= args.max_line_edges:
                return g, {"scale": scale}
            del g
            scale /= 2

    rng = np.random.default_rng(0)
    workloads = [
        ("trees_40", lambda: (graph_of(*tree_batch(40, rng)), {"trees": 40})),
        ("trees_4000", lambda: (graph_of(*tree_batch(4000, rng)), {"trees": 4000})),
        ("sbm", lambda: (graph_of(*sbm_like(100000, 10, rng)), {})),
        ("skewed", skewed),
    ]
    if args.only:
        workloads = [w for w in workloads if w[0] in args.only.split(",")]

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
        return wall, span

    def stats(xs):
        return {"median": round(_median(xs), 4), "min": round(min(xs), 4),
                "max": round(max(xs), 4)}

    result = {"tool": "line_graph_bench", "tile": kernel.LINE_GRAPH_TILE, "backtracking": bt,
              "free_bytes": free0, "warmup": args.warmup, "reps": args.reps,
              "host_reps": args.host_reps, "cases": []}
    for name, make in workloads:
        g, extra = make()
        gi = g._graph

        def device_route():
            lgi = gi.line_graph_device(dev, bt)
            lgi.adjacency(dev)
            return lgi

        def host_route():
            lgi = gi.line_graph(bt)
            lgi.adjacency(dev)
            return lgi

        a, b = device_route(), host_route()  # also the first warm-up of both
        torch.cuda.synchronize()
        hs, hd, _ = b.edges()
        same = (a.number_of_edges() == b.number_of_edges() and
                torch.equal(a._dev_coo[0].cpu(), hs) and torch.equal(a._dev_coo[1].cpu(), hd) and
                torch.equal(a.adjacency(dev).fwd.indices, b.adjacency(dev).fwd.indices))
        del a, b, hs, hd

        s, d, ws, (m, k, invalid, units) = counted(gi)
        bwd = gi.adjacency(dev).bwd
        fill_wall, fill_span = timed(lambda: kernel.line_graph_fill(bwd, s, d, bt, ws, units, m),
                                     args.warmup, args.reps, True)
        del fill_wall
        count_wall, _ = timed(lambda: kernel.line_graph_count(bwd, s, d, bt), args.warmup,
                              args.reps, False)
        E = gi.number_of_edges()
        fill_bytes = 16 * m + 8 * m + (0 if bt else 4 * k) + 8 * (E + 1)
        del s, d, ws

        dev_wall, dev_span = timed(device_route, args.warmup, args.reps, True)
        host_wall, _ = timed(host_route, 0, args.host_reps, False)
        fill_ms = _median(fill_span)
        case = dict(extra)
        case.update({
            "name": name, "nodes": gi.number_of_nodes(), "edges": E, "candidates": k,
            "line_edges": m, "units": units, "routes_agree": bool(same),
            "device_wall_ms": stats(dev_wall), "device_ms": stats(dev_span),
            "host_wall_ms": stats(host_wall),
            "host_over_device": round(_median(host_wall) / _median(dev_wall), 2),
            "count_wall_ms": stats(count_wall), "fill_ms": stats(fill_span), "fill_bytes": fill_bytes,
            "fill_gb_per_s": round(fill_bytes / (fill_ms * 1e-3) / 1e9, 1) if fill_ms > 0 else None,
        })
        result["cases"].append(case)
        print("# %-10s E=%d K=%d M=%d | device %.3f ms wall (%.3f ms on the stream) | host "
              "%.3f ms wall | x%.1f | count %.4f ms | fill %.4f ms (%s GB/s) | agree=%s"
              % (name, E, k, m, _median(dev_wall), _median(dev_span), _median(host_wall),
                 case["host_over_device"], _median(count_wall), fill_ms, case["fill_gb_per_s"], same),
              file=sys.stderr, flush=True)
        del g, gi, bwd
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(c["routes_agree"] for c in result["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
