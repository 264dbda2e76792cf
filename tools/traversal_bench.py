"""BFS and topological frontiers on the Reddit-shaped bench graph: the device
route (csrc/traversal.hip over the cached device adjacency) against the host
route (the native index's queue loops), each timed up to finished frontiers.

  bfs:   bfs_nodes from one source (the node of the largest out-degree) over
         the whole graph;
  topo:  topological_nodes of the graph's DAG part (the edges with src < dst).

Every figure is the median over the repeats after a warm-up. ``wall_ms`` is
host time from the call to the end of a stream synchronize: the device route
reads one status per level on the host, so wall clock is the honest figure for
both routes. ``per_level_ms`` is wall_ms over the number of frontiers. The
device adjacency (both CSRs) and the native index's CSRs are built before
anything is timed. Both routes must give the same frontiers: the tool compares
them before timing. ``deep`` is the same BFS on a path of ``--path`` nodes: the
many-narrow-levels case, where the device route pays its host read per level.

  python tools/traversal_bench.py [--scale 1.0] [--out profiles/r09/traversal.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="graph size as a fraction of Reddit")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3, help="repeats of the host route")
    ap.add_argument("--path", type=int, default=2000, help="nodes of the deep case's path")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch

    import dgl
    from dgl import data, kernel

    dev = torch.device("cuda", 0)

    def build(n, src, dst):
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(n)
        g.add_edges(src, dst)
        adj = g._graph.adjacency(dev)
        adj.bwd  # both directions' CSRs, as after a training step's backward pass
        return g

    def timed(fn, warmup, reps):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        wall = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t) * 1e3)
        return _median(wall), [min(wall), max(wall)]

    def case(name, g, device_route, host_route):
        (ids_d, sec_d), (ids_h, sec_h) = device_route(), host_route()  # first warm-up of both
        torch.cuda.synchronize()
        same = sec_d == sec_h and torch.equal(ids_d.cpu(), ids_h)
        levels = len(sec_d)
        dev_wall, dev_range = timed(device_route, args.warmup, args.reps)
        host_wall, host_range = timed(host_route, 0, args.host_reps)
        out = {"case": name, "nodes": g.number_of_nodes(), "edges": g.number_of_edges(),
               "levels": levels, "visited": int(ids_h.numel()),
               "largest_frontier": max(sec_h) if sec_h else 0, "routes_agree": bool(same),
               "device_wall_ms": round(dev_wall, 3), "host_wall_ms": round(host_wall, 3),
               "device_per_level_ms": round(dev_wall / max(levels, 1), 6),
               "host_per_level_ms": round(host_wall / max(levels, 1), 6),
               "host_over_device": round(host_wall / dev_wall, 4),
               "device_wall_min_max_ms": [round(x, 3) for x in dev_range],
               "host_wall_min_max_ms": [round(x, 3) for x in host_range]}
        print("# %-5s %d nodes, %d edges, %d levels | device %.3f ms wall (%.5f per level) | "
              "host %.3f ms wall (%.5f per level) | x%.4f | agree=%s"
              % (name, out["nodes"], out["edges"], levels, dev_wall, out["device_per_level_ms"],
                 host_wall, out["host_per_level_ms"], host_wall / dev_wall, same),
              file=sys.stderr, flush=True)
        return out

    t0 = time.perf_counter()
    src, dst, n = data.reddit_like(scale=args.scale, seed=0, device=dev)
    src, dst = src.cpu(), dst.cpu()
    g = build(n, src, dst)
    up = src < dst
    dag = build(n, src[up], dst[up])
    del up
    path = build(args.path, torch.arange(args.path - 1), torch.arange(1, args.path))
    torch.cuda.synchronize()
    result = {"tool": "traversal_bench", "chunk": kernel.TRAVERSAL_CHUNK,
              "graph_build_s": round(time.perf_counter() - t0, 2), "warmup": args.warmup,
              "reps": args.reps, "host_reps": args.host_reps, "cases": []}

    start = torch.bincount(src, minlength=n).argmax().reshape(1)
    del src, dst
    start_dev = start.to(dev)
    gi = g._graph
    result["cases"].append(case("bfs", g, lambda: gi.bfs_nodes_device(start_dev),
                                lambda: gi.bfs_nodes(start)))
    di = dag._graph
    result["cases"].append(case("topo", dag, lambda: di.topological_nodes_device(dev),
                                lambda: di.topological_nodes()))
    pi = path._graph
    zero, zero_dev = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64).to(dev)
    result["cases"].append(case("deep", path, lambda: pi.bfs_nodes_device(zero_dev),
                                lambda: pi.bfs_nodes(zero)))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(c["routes_agree"] for c in result["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
