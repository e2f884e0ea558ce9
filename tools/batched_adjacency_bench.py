"""GACN(72 -> 24) forward + backward through `ops.gacn` at B = 32, N = 883, T = 12 (PEMSD7-like synthetic graph) with a
shared and with a per-sample adjacency, alternated in one process and timed by HIP events after warm-up:

  (a) shared    the [N,N] path
  (b) dense     [32,N,N]: one pattern, 32 different weightings, through the dense-tensor path (batched_graph_of): a new
                tensor every step (a rotating pool larger than the cache), so every step fills the values with
                k_edge_values and reads the 4-byte outside count back
  (c) update    the same weightings through BatchedGraph.update_ (k_edge_values, nothing read back)
  eager         the reference's formulation (oracle.dense_torch.gacn_dense, adjacency [32,N,N]) on PyTorch-ROCm eager

and k_edge_values alone: its algorithmic bytes (4 V N^2 read + 4 V nnz written) next to its time from
`rocprofv3 --kernel-trace --stats` (a child process of this script, `--profile`) and from HIP events.

    python tools/batched_adjacency_bench.py [--steps 30] [--warmup 5] [--profile]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import ops  # noqa: E402
from oracle import dense_torch  # noqa: E402

B, C, O, N, T, EDGES = 32, 72, 24, 883, 12, 866
DEV = torch.device("cuda:0")


def setup():
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    w = torch.rand(B, N, N, generator=g) + 0.5
    batched = (adj.unsqueeze(0) * w).to(DEV)                      # one pattern, 32 weightings
    x = (torch.randn(B, C, N, T, generator=g)).to(DEV).requires_grad_(True)
    alpha = (torch.rand(C, generator=g) * 2 - 1).mul_(C ** -0.5).to(DEV).requires_grad_(True)
    Wg = (torch.randn(T, T, generator=g) * 0.3).to(DEV).requires_grad_(True)
    W = (torch.randn(O, C, generator=g) * 0.2).to(DEV).requires_grad_(True)
    dz = torch.randn(B, O, N, T, generator=g).to(DEV)
    return adj.to(DEV), batched, x, alpha, Wg, W, dz


def edge_values_only(reps=50):
    _, batched, *_ = setup()
    bg = ms_gat_amd.BatchedGraph(batched)
    for _ in range(5):
        bg.update_(batched)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        bg.update_(batched)
        ev[i + 1].record()
    torch.cuda.synchronize()
    bg.check()
    return bg, statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))


def profile_edge_values():
    """k_edge_values' mean time from rocprofv3 --kernel-trace --stats in a child process (None when unavailable)."""
    out = tempfile.mkdtemp(prefix="ev_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ev", "--", sys.executable,
           os.path.abspath(__file__), "--edge-values-only"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        print(f"rocprofv3 not run: {e}", flush=True)
        return None
    if r.returncode != 0:
        print(f"rocprofv3 exited {r.returncode}: {r.stderr[-500:]}", flush=True)
        return None
    paths = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    for path in paths:
        with open(path) as f:
            for row in csv.DictReader(f):
                if "k_edge_values" in row.get("Name", ""):
                    return float(row["AverageNs"]) / 1e3, int(row["Calls"])
    print(f"no k_edge_values row in {paths or 'no *kernel_stats.csv'} under {out}", flush=True)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--edge-values-only", action="store_true")
    a = ap.parse_args()
    if a.edge_values_only:
        edge_values_only()
        return

    adj, batched, x, alpha, Wg, W, dz = setup()
    pool = [batched.clone() for _ in range(20)]                    # > the dense-path cache (16): every step misses
    bg = ms_gat_amd.BatchedGraph(batched)
    it = {"i": 0}

    def step(adjacency):
        x.grad = alpha.grad = Wg.grad = W.grad = None
        ops.gacn(x, alpha, Wg, W, adjacency).backward(dz)

    def form_b():
        it["i"] += 1
        step(pool[it["i"] % len(pool)])

    def form_c():
        bg.update_(batched)
        step(bg)

    def eager():
        xs, al, wg, w = (t.detach().requires_grad_(True) for t in (x, alpha, Wg, W))
        dense_torch.gacn_dense(xs, batched, wg, al, w).backward(dz)

    forms = {"a_shared": lambda: step(adj), "b_dense_readback": form_b, "c_update": form_c, "eager_rocm": eager}
    for _ in range(a.warmup):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.steps):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    bg.check()
    for k, v in times.items():
        q = sorted(v)
        print(f"{k:18s} median {statistics.median(v):8.4f} ms   p10 {q[len(q) // 10]:8.4f}   p90 {q[9 * len(q) // 10]:8.4f}", flush=True)

    g, ev_ms = edge_values_only()
    nbytes = 4 * B * N * N + 4 * B * g.nnz
    print(f"k_edge_values: V = {B}, N = {N}, nnz = {g.nnz}: {nbytes / 1e6:.1f} MB algorithmic "
          f"(4 V N^2 read + 4 V nnz written); HIP events (launch to launch, median) {ev_ms * 1e3:.1f} us = "
          f"{nbytes / (ev_ms * 1e-3) / 1e12:.2f} TB/s", flush=True)
    if a.profile:
        prof = profile_edge_values()
        if prof is not None:
            us, calls = prof
            print(f"k_edge_values: rocprofv3 --kernel-trace --stats {us:.1f} us mean over {calls} calls = "
                  f"{nbytes / (us * 1e-6) / 1e12:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
