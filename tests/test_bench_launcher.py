"""bench.py's launcher and its multi-rank lines, on the host (gloo, CPU).

`python bench.py --gpus N` (N > 1, no WORLD_SIZE) must start N ranks itself as
a child torchrun, relay rank 0's JSON line and exit with the child's code; an
outer launcher whose WORLD_SIZE disagrees with --gpus is an error. With
`--full` the multi-rank line carries cpu_baseline, a per-rank rmat roofline and the
halo_exchange block (VERDICT r02 "Next" 1). `--device cpu` runs the same
plumbing through the library's host kernels.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _args(argv):
    return bench.build_parser().parse_args(argv)


def test_launch_command_decision():
    argv = ["--gpus", "4", "--steps", "3"]
    cmd = bench.launch_command(_args(argv), argv, {}, port=12345)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "12345"
    assert cmd[-len(argv) - 1] == os.path.abspath(bench.__file__)
    assert cmd[-len(argv):] == argv
    # one GPU, or already a rank of an outer launcher: run in-process
    assert bench.launch_command(_args(["--gpus", "1"]), [], {}) is None
    assert bench.launch_command(_args(argv), argv, {"WORLD_SIZE": "4"}) is None


def test_world_mismatch_is_an_error():
    assert bench.world_mismatch(_args(["--gpus", "8"]), {"WORLD_SIZE": "8"}) is None
    assert bench.world_mismatch(_args([]), {}) is None
    assert "WORLD_SIZE 2" in bench.world_mismatch(_args(["--gpus", "8"]), {"WORLD_SIZE": "2"})
    assert bench.world_mismatch(_args(["--gpus", "2"]), {}) is not None
    assert bench.world_mismatch(_args(["--gpus", "1", "--dist-rehearsal"]),
                                {"WORLD_SIZE": "1"}) is None
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4",
                        "--device", "cpu"], env=dict(os.environ, WORLD_SIZE="2"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and p.stdout == b""


def test_relay_passes_output_and_exit_code(capfd):
    """The child's JSON line reaches stdout, anything else it printed there
    (e.g. gloo's connection notices) goes to stderr; the exit code is the
    child's."""
    rc = bench.relay([sys.executable, "-c",
                      "import sys; print('line one'); print('{\"k\": 1}'); sys.exit(3)"])
    assert rc == 3
    cap = capfd.readouterr()
    assert cap.out.strip() == '{"k": 1}'
    assert "line one" in cap.err


def test_bench_two_ranks_without_outer_launcher():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--device", "cpu", "--graph-scale", "0.002", "--rmat-scale", "12",
                        "--steps", "2", "--warmup", "1", "--cpu-sample-edges", "20000",
                        "--full"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    # stdout holds rank 0's JSON line and nothing else (the gloo groups'
    # connection notices go to stderr)
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), lines[:3]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak"
    assert "2-way 1-D dst-row partition" in r["config"]["parallelism"]
    assert [x["rank"] for x in r["roofline"]["per_rank"]] == [0, 1]
    assert r["halo_exchange"]["mode"] in ("allgather", "alltoall")
    cb = r["cpu_baseline"]
    assert cb["kind"] == "reference" and cb["value"] > 0
    assert cb["build_kernel"]["bit_identical_to_reference"]
    # the fixed-graph block beside the weak-scaled line (r03 verdict "Next" 6)
    st = r["strong"]
    assert st["scaling"] == "strong" and st["n_gpus"] == 2 and st["value"] > 0
    assert "the N = 1 graph" in st["config"]
    assert [x["rank"] for x in st["roofline"]["per_rank"]] == [0, 1]
    assert st["halo_exchange"]["mode"] in ("allgather", "alltoall")
    rm = r["rmat12"]
    assert rm["n_gpus"] == 2 and rm["scaling"] == "strong"
    assert [x["rank"] for x in rm["roofline"]["per_rank"]] == [0, 1]
    assert all(x["bytes_per_step"] > 0 for x in rm["roofline"]["per_rank"])
    assert rm["halo_exchange"] is not None and rm["cpu_baseline"]["value"] > 0
    # the two ranks' rmat partitions cover the graph's edges
    assert sum(x["bytes_per_step"] for x in rm["roofline"]["per_rank"]) >= \
        bench.algorithmic_bytes(1 << 16, 0, bench.FEAT)


_LEGS = ("one_launch", "train_step", "gcn_reddit", "gat", "sage", "gat_pubmed", "rgcn", "rmat12",
         "sage_rmat12", "halo_exchange", "halo_bf16", "strong")


def test_plain_run_is_the_headline_alone_and_dumps_its_output(tmp_path):
    """Without --full: the line with its headline fields and no secondary leg;
    --dump-outputs writes the last timed step's rows, the same from run to
    run, and they are the step's (copy_u + sum of the seeded features)."""
    import numpy as np
    lines, outs = [], []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                            "--device", "cpu", "--graph-scale", "0.002", "--rmat-scale", "12",
                            "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / d)],
                           env=_bench_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines.append(_line(p.stdout))
        assert os.listdir(str(tmp_path / d)) == ["h_out.npy"]
        outs.append(np.load(str(tmp_path / d / "h_out.npy")))
    r = lines[0]
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert r["unit"] == "edges/s" and r["higher_is_better"] is True and r["dtype"] == "fp32"
    assert r["metric"] == "edges/sec on update_all g-SpMM (copy_u+sum, feat=128)"
    edges = int(r["config"]["workload"].split(" nodes, ")[1].split(" edges")[0])
    assert abs(r["value"] - edges / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    assert r["cpu_baseline"] is None and r["roofline"]["traffic"] is None
    assert not [k for k in _LEGS if k in r]
    assert outs[0].dtype == np.float32 and outs[0].shape == (r["config"]["global_batch"], 128)
    assert np.array_equal(outs[0], outs[1])
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0


def test_dump_outputs_samples_rows_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 8 * 10)  # ten fp32 rows of width 8
    t = torch.arange(33 * 8, dtype=torch.float32).reshape(33, 8)
    small = torch.arange(6, dtype=torch.float64).reshape(3, 2)
    bench.dump_outputs(str(tmp_path / "x"), {"t": t})
    bench.dump_outputs(str(tmp_path / "y"), {"t": t.clone(), "small": small})
    a = np.load(str(tmp_path / "x" / "t.npy"))
    b = np.load(str(tmp_path / "y" / "t.npy"))
    assert a.shape == (10, 8) and a.dtype == np.float32
    rows = (a[:, 0] / 8).astype(int)
    assert (np.diff(rows) > 0).all() and np.array_equal(a, t.numpy()[rows])  # whole rows, in order
    assert b.shape == (5, 8) and np.array_equal(b, t.numpy()[(b[:, 0] / 8).astype(int)])
    s = np.load(str(tmp_path / "y" / "small.npy"))
    assert s.dtype == np.float64 and np.array_equal(s, small.numpy())
    total = sum(os.path.getsize(str(tmp_path / "y" / f)) - 128 for f in ("t.npy", "small.npy"))
    assert total <= 4 * 8 * 10


def _bench_env(**extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
              "DGLHIP_BENCH_FAIL"):
        env.pop(k, None)
    env.update(extra)
    return env


_SMALL = ["--gpus", "2", "--device", "cpu", "--graph-scale", "0.002", "--rmat-scale", "12",
          "--steps", "2", "--warmup", "1", "--cpu-sample-edges", "20000", "--full"]


def _line(stdout):
    lines = [l for l in stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), lines[:3]  # the line, nothing else
    return json.loads(lines[0])


def test_rank1_setup_failure_in_rmat_leg_keeps_the_line():
    """A failure in rank 1's setup of the rmat leg (injected): every rank
    skips the leg together, rank 0 prints the headline line with the leg's
    error, and the job exits promptly (no collective left waiting) with the
    failed-leg code (r04 ADVICE: a lost leg is not a clean run)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + _SMALL +
                       ["--dist-timeout", "60", "--leg-deadline", "40"],
                       env=_bench_env(DGLHIP_BENCH_FAIL="rmat12:1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    # rank 0 exits EXIT_LEG_FAILED; torchrun (which the launcher relays)
    # reports a failed child as 1
    assert p.returncode != 0 and "exitcode: %d" % bench.EXIT_LEG_FAILED in p.stderr.decode()
    r = _line(p.stdout)
    assert r["value"] > 0 and r["n_gpus"] == 2
    assert "rank 1 (setup)" in r["rmat12"]["error"] and "injected" in r["rmat12"]["error"]
    assert r["train_step"]["value"] > 0 and r["strong"]["value"] > 0


def test_rank1_failure_inside_a_collective_leg_is_bounded():
    """Rank 1 fails inside the train_step leg's run phase, so rank 0 waits in
    a collective rank 1 never joins: rank 0's leg deadline prints the line
    (headline intact, the leg's error) well within the collective timeout."""
    import time
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + _SMALL +
                       ["--dist-timeout", "60", "--leg-deadline", "15"],
                       env=_bench_env(DGLHIP_BENCH_FAIL="train_step:1:run"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    took = time.time() - t0
    assert p.returncode != 0 and "exitcode: %d" % bench.EXIT_LEG_FAILED in p.stderr.decode()
    r = _line(p.stdout)  # exactly one line, though the timer and the main thread race
    assert r["value"] > 0 and r["halo_exchange"]["mode"] in ("allgather", "alltoall")
    assert "still running after 15 s" in r["train_step"]["error"]
    assert took < 100


def test_relay_sigterm_kills_every_rank():
    """SIGTERM to the launching parent (the driver's kill) takes the torchrun
    child and every rank down with it: no descendant survives."""
    import signal
    import time
    psutil = pytest.importorskip("psutil")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--device", "cpu", "--graph-scale", "0.002", "--steps", "100000",
                          "--warmup", "1", "--no-rmat-leg", "--no-cpu-baseline"],
                         env=_bench_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        parent = psutil.Process(p.pid)
        kids = []
        t0 = time.time()
        while time.time() - t0 < 120:  # the agent and both ranks are up
            kids = parent.children(recursive=True)
            if sum("bench.py" in " ".join(k.cmdline()) for k in kids
                   if k.is_running()) >= 3:
                break
            time.sleep(0.5)
        assert len(kids) >= 3
        time.sleep(3)  # the ranks are past their imports
        p.send_signal(signal.SIGTERM)
        rc = p.wait(timeout=60)
        assert rc == 128 + signal.SIGTERM
        gone, alive = psutil.wait_procs(kids, timeout=30)
        assert not alive, [k.pid for k in alive]
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
