"""A UDF reduce over the Reddit-shaped bench graph, per call: the host route of
degree bucketing (the schedule from dglhip_degree_bucketing_host over host
ids, each bucket's ids uploaded) against the device route (the schedule from
csrc/degree_buckets.hip, kept on the index's CSR), alternating in one process.

Messages are copy_src of F float32 features, materialised once on the device
and shared by both routes; the reducer is the UDF mean
(``mailbox.mean(1)``, the one bench_models.mean_bucketing_cpu restates). Each
figure covers one whole-graph bucket_reduce, from the call to the end of its
work on the stream:

  host_call      runtime.degree_bucketing._bucket_reduce_host
  device_first   _bucket_reduce_device with no cached schedule (build, two
                 host reads, then the buckets)
  device_cached  _bucket_reduce_device with the schedule on the CSR
  build          kernel.degree_buckets alone

``ms`` is the span between two device events around the call, ``wall_ms`` host
time to the end of a stream synchronize; median over the calls, with min and
max as the run's own spread. Both routes must give the same tensor: checked
with torch.equal before anything is timed.

  python tools/udf_reduce_percall.py [--edge-fraction 0.125] [--calls 10]
                                     [--out profiles/r29/udf_reduce.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge-fraction", type=float, default=1.0,
                    help="keep this fraction of the graph's edges (a random sample, all nodes)")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch

    import dgl
    from dgl import data, kernel
    from dgl.runtime import degree_bucketing as db

    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    src, dst, n = data.reddit_like(scale=1, seed=0, device=dev)
    if args.edge_fraction < 1.0:
        gen = torch.Generator(device=dev).manual_seed(3)
        keep = torch.rand(src.numel(), generator=gen, device=dev) < args.edge_fraction
        src, dst = src[keep], dst[keep]
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src.cpu(), dst.cpu())
    gi = g._graph
    dst_host = gi.dst()
    csr = gi.adjacency(dev).fwd
    h = torch.rand(n, args.feat, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    g.ndata["h"] = h
    msgs = {"m": h.index_select(0, src)}
    del src, dst
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    def mean(nodes):
        return {"o": nodes.mailbox["m"].mean(1)}

    def host_call():
        return db._bucket_reduce_host(g, mean, None, dst_host, msgs, g._node_frame)["o"]

    def device_cached():
        return db._bucket_reduce_device(g, mean, None, dst_host, msgs, g._node_frame, dev)["o"]

    def device_first():
        csr._plans.pop(db._PLAN_KEY, None)
        return device_cached()

    def build():
        return kernel.degree_buckets(csr, csr.eid)

    routes = [("host_call", host_call), ("device_first", device_first),
              ("device_cached", device_cached), ("build", build)]
    a, b = host_call(), device_first()
    same = torch.equal(a, b)
    buckets = csr._plans[db._PLAN_KEY].num_buckets
    max_degree = csr._plans[db._PLAN_KEY].max_degree
    del a, b
    for _ in range(args.warmup):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    span = {name: [] for name, _ in routes}
    wall = {name: [] for name, _ in routes}
    for _ in range(args.calls):  # alternating: every route once per round
        for name, fn in routes:
            if name == "device_cached":  # device_first ran just before and left its schedule
                assert db._PLAN_KEY in csr._plans
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t) * 1e3)
            span[name].append(e0.elapsed_time(e1))
            del out
    result = {"tool": "udf_reduce_percall", "nodes": n, "edges": gi.number_of_edges(),
              "edge_fraction": args.edge_fraction, "feat": args.feat, "reducer": "mailbox.mean(1)",
              "buckets": buckets, "max_degree": max_degree, "chunk": kernel.BUCKET_CHUNK,
              "message_bytes": msgs["m"].numel() * 4, "setup_s": round(build_s, 2),
              "warmup": args.warmup, "calls": args.calls, "routes_agree": bool(same),
              "ms": {k: _stats(v) for k, v in span.items()},
              "wall_ms": {k: _stats(v) for k, v in wall.items()}}
    result["host_over_device_cached"] = round(
        result["wall_ms"]["host_call"]["median"] / result["wall_ms"]["device_cached"]["median"], 2)
    for name, _ in routes:
        print("# %-13s %10.3f ms on the stream, %10.3f ms wall (min %.3f, max %.3f)"
              % (name, result["ms"][name]["median"], result["wall_ms"][name]["median"],
                 result["wall_ms"][name]["min"], result["wall_ms"][name]["max"]),
              file=sys.stderr, flush=True)
    print("# %d buckets, max degree %d, agree=%s" % (buckets, max_degree, same), file=sys.stderr)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
