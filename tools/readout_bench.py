"""Batched-graph readout: kernel.segment_reduce against the reference's
formulation run by torch on the same device (scatter_add_ for sum and mean, a
loop of torch.max per graph for max: python/dgl/batched_graph.py), forward
alone and forward + backward, timed with device events around the calls (the
median of the repeats after a warm-up).

Shapes: batches of 256 and 4096 graphs of 10..100 nodes at F = 64 and 256, and
one 232,965-row segment at F = 128. The forward reads x once, so its
algorithmic bandwidth is 4 N F bytes over the forward time, quoted against
the HBM rate a float4 copy reaches on the MI355X (6.29 TB/s measured, 8.0 TB/s
datasheet).

Every shape runs in a process of its own under its own time limit; the first
one that fails or times out ends the run.

  python tools/readout_bench.py [--out profiles/r07/readout/readout_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_COPY_GBS = 6290.0
SHAPES = [("b256_f64", 256, 64), ("b256_f256", 256, 256), ("b4096_f64", 4096, 64),
          ("b4096_f256", 4096, 256), ("single_232965_f128", 1, 128)]
STEP_LIMIT_S = 300


def _sizes(name, B):
    import numpy as np
    if B == 1:
        return [232965]
    return np.random.default_rng(B).integers(10, 101, B).tolist()


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def run_case(index):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dgl-1_amd")]
    import torch
    from dgl import kernel
    name, B, F = SHAPES[index]
    dev = torch.device("cuda", 0)
    sizes = _sizes(name, B)
    N = sum(sizes)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(N, F, generator=gen).to(dev).requires_grad_(True)
    dy = torch.randn(B, F, generator=gen).to(dev)
    segs = kernel.SegmentOffsets(sizes=sizes)
    seg = torch.arange(B).repeat_interleave(torch.tensor(sizes)).to(dev)
    seg2 = seg[:, None].expand(-1, F)
    bounds = [0]
    for n in sizes:
        bounds.append(bounds[-1] + n)

    def ref(reduce):
        if reduce == "max":
            return torch.stack([torch.max(x[a:b], 0)[0] for a, b in zip(bounds[:-1], bounds[1:])])
        y = torch.zeros(B, F, device=dev).scatter_add_(0, seg2, x)
        if reduce == "mean":
            cnt = torch.zeros(B, device=dev).scatter_add_(0, seg, torch.ones(N, device=dev))
            y = y / cnt.clamp(min=1)[:, None]
        return y

    def step(fwd):
        def run():
            x.grad = None
            fwd().backward(dy)
        return run

    def no_grad(fwd):
        def run():
            with torch.no_grad():
                fwd()
        return run

    out = []
    for reduce in ("sum", "mean", "max"):
        ours = lambda: kernel.segment_reduce(x, segs, reduce)  # noqa: E731
        theirs = lambda: ref(reduce)  # noqa: E731
        slow = reduce == "max" and B > 1  # one launch per graph: few repeats are enough
        reps, warm = (5, 1) if slow else (31, 5)
        rec = {"shape": name, "graphs": B, "rows": N, "feat": F, "reduce": reduce,
               "hip_fwd_ms": _median_ms(no_grad(ours), 5, 31),
               "hip_fwd_bwd_ms": _median_ms(step(ours), 5, 31),
               "torch_fwd_ms": _median_ms(no_grad(theirs), warm, reps),
               "torch_fwd_bwd_ms": _median_ms(step(theirs), warm, reps)}
        rec["fwd_read_bytes"] = 4 * N * F
        rec["hip_fwd_gbs"] = rec["fwd_read_bytes"] / rec["hip_fwd_ms"] / 1e6
        rec["hip_fwd_frac_of_hbm_copy"] = rec["hip_fwd_gbs"] / HBM_COPY_GBS
        rec["speedup_fwd_bwd"] = rec["torch_fwd_bwd_ms"] / rec["hip_fwd_bwd_ms"]
        with torch.no_grad():
            err = (ours() - theirs()).abs().max().item()
        rec["max_abs_diff_vs_torch"] = err
        out.append(rec)
    print("READOUT_BENCH " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "readout",
                                                  "readout_bench.json"))
    ap.add_argument("--case", type=int, default=None, help="internal: run one shape")
    args = ap.parse_args()
    if args.case is not None:
        run_case(args.case)
        return 0
    results, failed = [], None
    for i, (name, _, _) in enumerate(SHAPES):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)],
                                 capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            failed = "%s: no result within %d s" % (name, STEP_LIMIT_S)
            break
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("READOUT_BENCH ")]
        if res.returncode != 0 or not lines:
            failed = "%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:])
            break
        results.extend(json.loads(lines[-1][len("READOUT_BENCH "):]))
        for r in results[-3:]:
            print("%-20s %-4s hip fwd %.4f ms (%.0f GB/s) fwd+bwd %.4f ms | torch fwd %.4f "
                  "fwd+bwd %.4f ms | x%.1f" % (r["shape"], r["reduce"], r["hip_fwd_ms"],
                                               r["hip_fwd_gbs"], r["hip_fwd_bwd_ms"],
                                               r["torch_fwd_ms"], r["torch_fwd_bwd_ms"],
                                               r["speedup_fwd_bwd"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"hbm_copy_gbs": HBM_COPY_GBS, "results": results, "failed": failed}, f,
                  indent=1)
        f.write("\n")
    if failed:
        print("stopped: " + failed, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
