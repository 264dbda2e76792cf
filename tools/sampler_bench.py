"""Neighbour sampling on the Reddit-shaped bench graph: the device route
(seeds on the GPU, csrc/neighbor_sample.hip) against the host route (the
native index's uniform sampler), each timed up to the sampled subgraph's ids
and edge list on the GPU.

  (a) device: GraphIndex.neighbor_sampling([seeds on the GPU], seed=...) ->
      vertices, parent edge ids and the edge list, on the GPU;
  (b) host:   GraphIndex.neighbor_sampling([seeds on the host]) (the native
      sampler, which exists without this tool's subject) -> the same arrays,
      read from the native subgraph and uploaded.

1,000 random seeds, 2 hops, direction 'in', fan-out 10 and 25. Every figure is
the median over the repeats after a warm-up, each repeat on a fresh seed set.
``wall_ms`` is host time from the call to the end of a stream synchronize (the
device route's host reads are part of the call, so wall clock is the honest
figure for both). ``hops_ms`` / ``final_ms`` split route (a) between the init
+ hop launches (with their host reads) and the final stage, from device events
in a run of their own. The parent's adjacency is built before anything is
timed. The two routes draw differently, so the tool checks the device route
against the seeded host twin instead, before timing.

``--node-prob`` adds the weighted leg (NeighborSampler's node_prob; weights =
in-degree + 1, so hubs are favoured) on the same seed sets and protocol:

  (c) weighted device: route (a) with node_prob, the weights already on the GPU;
  (d) weighted host twin: the same call over host seeds with ``seed=`` (the
      only host route of a weighted draw), its arrays uploaded as in (b).

(c) is checked against the weighted host twin before timing. Each case then
carries a ``weighted`` entry: (c)'s wall time, its ratio to the uniform device
route (a) of the same run, (d)'s wall time and its ratio to (c), and (c)'s
hops / final split.

  python tools/sampler_bench.py [--scale 1.0] [--node-prob]
                                [--out profiles/r11/sampler/sampler.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUTS = (10, 25)
NUM_HOPS = 2


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="graph size as a fraction of Reddit")
    ap.add_argument("--seeds", type=int, default=1000, help="seed nodes per batch")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--node-prob", action="store_true",
                    help="also time weighted sampling (weights = in-degree + 1)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch

    from dgl import data, kernel
    from dgl.graph_index import NodeProb, _from_edges

    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    src, dst, n = data.reddit_like(scale=args.scale, seed=0, device=dev)
    gi = _from_edges(n, src.cpu(), dst.cpu(), True, True)
    del src, dst
    fwd = gi.adjacency(dev).fwd
    host_fwd = gi.adjacency("cpu").fwd
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    deg = fwd.degrees()
    result = {"tool": "sampler_bench", "nodes": n, "edges": gi.number_of_edges(),
              "max_in_degree": int(deg.max()), "reg_slots": kernel.SAMPLE_REG_SLOTS,
              "seeds": args.seeds, "num_hops": NUM_HOPS, "graph_build_s": round(build_s, 2),
              "warmup": args.warmup, "reps": args.reps, "host_reps": args.host_reps,
              "cases": []}
    if args.node_prob:
        prob = NodeProb((deg + 1).to(torch.float32), n)  # checked and uploaded once
        result["node_prob"] = "in-degree + 1"
        result["lds_slots"] = kernel.SAMPLE_LDS_SLOTS
    gen = torch.Generator().manual_seed(1)
    batches = [torch.randperm(n, generator=gen)[:args.seeds].contiguous()
               for _ in range(args.warmup + args.reps)]
    dev_batches = [b.to(dev) for b in batches]

    for k in FANOUTS:
        def device_route(i):
            sgi = gi.neighbor_sampling([dev_batches[i]], k, NUM_HOPS, "in", None, seed=i)[0]
            return sgi.induced_nodes, sgi.induced_edges, sgi._dev_coo

        def host_route(i):
            sgi = gi.neighbor_sampling([batches[i]], k, NUM_HOPS, "in", None)[0]
            u, v, _ = sgi.edges("eid")
            return [t.to(dev) for t in (sgi.induced_nodes, sgi.induced_edges, u, v)]

        # the device route against the seeded host twin, on the first batch
        want = kernel.neighbor_sample(host_fwd, batches[0], NUM_HOPS, k, kernel.sample_mix(0))
        nid, eid, (s, d) = device_route(0)
        same = (torch.equal(nid.cpu(), want[0]) and torch.equal(eid.cpu(), want[4]) and
                torch.equal(s.cpu(), want[2]) and torch.equal(d.cpu(), want[3]))
        nv, m = nid.numel(), eid.numel()
        host_route(0)
        torch.cuda.synchronize()

        def timed(fn, warmup, reps):
            for i in range(warmup):
                fn(i)
            torch.cuda.synchronize()
            wall = []
            for i in range(warmup, warmup + reps):
                t = time.perf_counter()
                fn(i)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t) * 1e3)
            return _median(wall), [min(wall), max(wall)]

        dev_wall, dev_range = timed(device_route, args.warmup, args.reps)
        host_wall, host_range = timed(host_route, 1, args.host_reps)
        hops, final = [], []
        for i in range(args.warmup, args.warmup + args.reps):
            tm = {}
            kernel.neighbor_sample(fwd, dev_batches[i], NUM_HOPS, k, kernel.sample_mix(i),
                                   timings=tm)
            hops.append(tm["hops_ms"])
            final.append(tm["final_ms"])
        if args.node_prob:
            def weighted_route(i):
                sgi = gi.neighbor_sampling([dev_batches[i]], k, NUM_HOPS, "in", prob, seed=i)[0]
                return sgi.induced_nodes, sgi.induced_edges, sgi._dev_coo

            def weighted_twin(i):
                sgi = gi.neighbor_sampling([batches[i]], k, NUM_HOPS, "in", prob, seed=i)[0]
                arrays = [sgi.induced_nodes, sgi.induced_edges] + list(sgi._dev_coo)
                return [t.to(dev) for t in arrays]

            w_host, w_dev = prob.on("cpu"), prob.on(dev)
            want = kernel.neighbor_sample(host_fwd, batches[0], NUM_HOPS, k, kernel.sample_mix(0),
                                          node_weight=w_host)
            wnid, weid, (ws, wd) = weighted_route(0)
            w_same = (torch.equal(wnid.cpu(), want[0]) and torch.equal(weid.cpu(), want[4]) and
                      torch.equal(ws.cpu(), want[2]) and torch.equal(wd.cpu(), want[3]))
            w_wall, w_range = timed(weighted_route, args.warmup, args.reps)
            t_wall, t_range = timed(weighted_twin, 1, args.host_reps)
            w_hops, w_final = [], []
            for i in range(args.warmup, args.warmup + args.reps):
                tm = {}
                kernel.neighbor_sample(fwd, dev_batches[i], NUM_HOPS, k, kernel.sample_mix(i),
                                       timings=tm, node_weight=w_dev)
                w_hops.append(tm["hops_ms"])
                w_final.append(tm["final_ms"])
            weighted = {"sub_nodes": wnid.numel(), "sub_edges": weid.numel(),
                        "matches_host_twin": bool(w_same), "device_wall_ms": round(w_wall, 3),
                        "over_uniform_device": round(w_wall / dev_wall, 2),
                        "host_twin_wall_ms": round(t_wall, 3),
                        "host_twin_over_device": round(t_wall / w_wall, 2),
                        "hops_ms": round(_median(w_hops), 3),
                        "final_ms": round(_median(w_final), 3),
                        "device_wall_min_max_ms": [round(x, 3) for x in w_range],
                        "host_twin_wall_min_max_ms": [round(x, 3) for x in t_range]}
            print("# fan-out %d weighted: %d nodes, %d edges | device %.3f ms wall (hops %.3f "
                  "ms, final %.3f ms) = x%.2f the uniform device route | host twin %.2f ms wall "
                  "| x%.1f | twin=%s"
                  % (k, weighted["sub_nodes"], weighted["sub_edges"], w_wall, weighted["hops_ms"],
                     weighted["final_ms"], w_wall / dev_wall, t_wall, t_wall / w_wall, w_same),
                  file=sys.stderr, flush=True)
        case = {"fanout": k, "sub_nodes": nv, "sub_edges": m, "matches_host_twin": bool(same),
                "device_wall_ms": round(dev_wall, 3), "host_wall_ms": round(host_wall, 3),
                "host_over_device": round(host_wall / dev_wall, 2),
                "hops_ms": round(_median(hops), 3), "final_ms": round(_median(final), 3),
                "device_wall_min_max_ms": [round(x, 3) for x in dev_range],
                "host_wall_min_max_ms": [round(x, 3) for x in host_range]}
        if args.node_prob:
            case["weighted"] = weighted
        result["cases"].append(case)
        print("# fan-out %d: %d nodes, %d edges | device %.3f ms wall (hops %.3f ms, final "
              "%.3f ms on the stream) | host %.2f ms wall | x%.1f | twin=%s"
              % (k, nv, m, dev_wall, case["hops_ms"], case["final_ms"], host_wall,
                 host_wall / dev_wall, same), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(c["matches_host_twin"] and c.get("weighted", c)["matches_host_twin"]
             for c in result["cases"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
