"""typed_linear_spmm (the f32-MFMA grouped GEMM, csrc/typed_linear.hip) against
the route the same call took before it, typed_block_spmm with one block, on
the AIFB-shaped graph of examples/rgcn/entity_classify.py: forward and forward
+ backward of one layer per (Fi, Fo). The two routes alternate in rounds of
``--reps`` calls timed with device events after a warm-up; per route the
median, minimum and maximum of the rounds' per-call means. Needs a ROCm device.

  python tools/typed_linear_bench.py --out profiles/typed_linear_bench.json
"""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-1_amd"))
from dgl import kernel  # noqa: E402


def example():
    spec = importlib.util.spec_from_file_location(
        "entity_classify", os.path.join(ROOT, "examples", "rgcn", "entity_classify.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="16x16,16x4,64x64,128x128")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--out", default="")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    src, dst, rel, norm, _, _, _, R = example().synthetic_entities()
    n = norm.size
    adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src), kernel.ORDER_EID, dev)
    etype, nrm = torch.from_numpy(rel).to(dev), torch.from_numpy(norm).to(dev)
    results = []
    for shape in args.shapes.split(","):
        Fi, Fo = (int(v) for v in shape.split("x"))
        assert kernel._typed_linear_ok(dev, adj.fwd.nnz, R, Fi, Fo)
        h = torch.randn(n, Fi, device=dev, requires_grad=True)
        W = (torch.randn(R, Fi, Fo, device=dev) * 0.3).requires_grad_(True)
        G = torch.randn(n, Fo, device=dev)
        routes = {
            "mfma": lambda: kernel.typed_linear_spmm(adj, h, W, etype, row_scale=nrm),
            "one_block": lambda: kernel.typed_block_spmm(adj, h, W.view(R, 1, Fi, Fo), etype,
                                                         row_scale=nrm),
        }

        def fwd(f):
            with torch.no_grad():
                f()

        def fwd_bwd(f):
            h.grad = W.grad = None
            f().backward(G)

        for mode, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            times = {k: [] for k in routes}
            for k, f in routes.items():
                for _ in range(args.warmup):
                    run(f)
            for _ in range(args.rounds):
                for k, f in routes.items():
                    times[k].append(per_call_ms(lambda: run(f), args.reps))
            row = {"Fi": Fi, "Fo": Fo, "mode": mode, "edges": int(adj.fwd.nnz), "relations": R}
            for k, t in times.items():
                t.sort()
                row[k + "_ms"] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}
                # the library's own launches alone (an event pair around each;
                # torch's gathers of the norms and the autograd glue excluded)
                kernel.timing_enable(True)
                for _ in range(20):
                    run(routes[k])
                ms, launches = kernel.timing_read()
                kernel.timing_enable(False)
                row[k + "_kernels_ms"] = ms / 20
                row[k + "_launches"] = launches / 20
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
