"""Learned edge weights (msgat_edge_weight_grad) at R = 3, B = 32, N = 883, T = 12 (PEMSD7-like synthetic graph),
through `ops.gacn` on the [R*B, ...] relation-major batch, timed by HIP events after warm-up:

  (a) GACN 72 -> 24 (project first)     Cu = 24
  (b) GACN  1 -> 24 (aggregate first)   Cu = 1

For each case, forward + backward three ways: the adjacency frozen (dense), learned sparse (`ops.edge_adjacency`: a
weight per stored edge, its gradient at the edges only) and learned dense (the [N,N] tensor requiring grad,
msgat_adjacency_grad); plus the eager PyTorch-ROCm autograd of the reference's formulation (oracle.dense_torch.gacn_dense,
float32, adjacency requiring grad).  `--profile` adds the kernel's own time from `rocprofv3 --kernel-trace --stats` (two
child processes of this script per case, one timing only the sparse-learned step and one only the dense-learned step;
the reductions of the split partial sums share their kernel names with the backward's own and are not listed) against
its memory bound: dv and feat read once,
2 * 4 G Cu N T bytes, plus q, kW and lse, at the measured 6.29 TB/s copy rate.

    python tools/edge_weight_grad_bench.py [--steps 20] [--warmup 3] [--profile]
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

R, B, N, T, EDGES = 3, 32, 883, 12, 866
HBM_TBS = 6.29    # measured float4 copy rate
DEV = torch.device("cuda:0")
CASES = {"a": (72, 24), "b": (1, 24)}


def setup(case):
    C, O = CASES[case]
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    x = torch.randn(R * B, C, N, T, generator=g).to(DEV)
    alpha = ((torch.rand(R, C, generator=g) * 2 - 1) * C ** -0.5).to(DEV).requires_grad_(True)
    Wg = (torch.randn(R, T, T, generator=g) * 0.3).to(DEV).requires_grad_(True)
    W = (torch.randn(R, O, C, generator=g) * 0.2).to(DEV).requires_grad_(True)
    dz = torch.randn(R * B, O, N, T, generator=g).to(DEV)
    return adj.to(DEV), x.requires_grad_(True), alpha, Wg, W, dz


def kernel_bytes(case):
    C, O = CASES[case]
    Cu = O if C > O else C
    G = R * B
    return 2.0 * 4 * G * Cu * N * T + 4.0 * G * N * (2 * T + 1)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t)


def run_case(case, steps, warmup, eager=True, modes=("frozen", "sparse", "dense")):
    adj, x, alpha, Wg, W, dz = setup(case)
    pattern = adj.to_sparse_csr()
    crow, col = pattern.crow_indices(), pattern.col_indices()
    weight = pattern.values().clone().requires_grad_(True)
    dense = adj.clone().requires_grad_(True)

    def step(make):
        x.grad = alpha.grad = Wg.grad = W.grad = None
        weight.grad = dense.grad = None
        ops.gacn(x, alpha, Wg, W, make()).backward(dz)

    makers = {"frozen": lambda: adj, "sparse": lambda: ops.edge_adjacency(crow, col, weight), "dense": lambda: dense}
    out = {mode: timed(lambda: step(makers[mode]), steps, warmup) for mode in modes}
    if eager:
        def eager_step():
            a = adj.clone().requires_grad_(True)
            xs = x.detach().requires_grad_(True)
            zs = []
            for r in range(R):
                zs.append(dense_torch.gacn_dense(xs[r * B:(r + 1) * B], a, Wg[r].detach(), alpha[r].detach(), W[r].detach()))
            torch.cat(zs).backward(dz)
        out["eager_rocm"] = timed(eager_step, max(3, steps // 4), 1)
    return out, int(crow[-1])


def profile(case, mode):
    """The kernels of the `mode` step alone (its gradient kernel and the partial sums' reduction) from rocprofv3
    --kernel-trace --stats in a child process"""
    out = tempfile.mkdtemp(prefix="ew_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ew", "--", sys.executable,
           os.path.abspath(__file__), "--only", case, "--mode", mode, "--no-eager", "--steps", "10", "--warmup", "2"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        print(f"rocprofv3 not run: {e}", flush=True)
        return None
    if r.returncode != 0:
        print(f"rocprofv3 exited {r.returncode}: {r.stderr[-500:]}", flush=True)
        return None
    rows = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                rows[row["Name"]] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only", choices=sorted(CASES))
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--mode", choices=["frozen", "sparse", "dense"], help="time only this step (the profiler's children)")
    a = ap.parse_args()
    for case in ([a.only] if a.only else sorted(CASES)):
        C, O = CASES[case]
        if a.mode:
            t, nnz = run_case(case, a.steps, a.warmup, eager=False, modes=(a.mode,))
            print(f"({case}) {a.mode}: fwd+bwd {t[a.mode]:.3f} ms", flush=True)
            continue
        t, nnz = run_case(case, a.steps, a.warmup, eager=not a.no_eager)
        line = (f"({case}) GACN {C}->{O} R={R} B={B} N={N} T={T} nnz={nnz}: fwd+bwd frozen {t['frozen']:.3f} ms, "
                f"learned sparse {t['sparse']:.3f} ms (+{t['sparse'] - t['frozen']:.3f}), "
                f"learned dense {t['dense']:.3f} ms (+{t['dense'] - t['frozen']:.3f})")
        if "eager_rocm" in t:
            line += f"; eager PyTorch-ROCm autograd {t['eager_rocm']:.3f} ms"
        print(line, flush=True)
        for mode in (("sparse", "dense") if a.profile and not a.only else ()):
            rows = profile(case, mode)
            print(f"  kernels of the {mode}-learned step alone:", flush=True)
            if rows:
                for name, (us, calls) in sorted(rows.items()):
                    if "k_edge_weight_grad" in name or "k_adjacency_grad" in name:
                        extra = ""
                        if "k_edge_weight_grad" in name:
                            nb = kernel_bytes(case)
                            bound = nb / (HBM_TBS * 1e12) * 1e6
                            extra = (f"  {nb / 1e6:.0f} MB: {nb / (us * 1e-6) / 1e12:.2f} TB/s, bound {bound:.0f} us, "
                                     f"{bound / us:.2f} of the {HBM_TBS} TB/s copy rate")
                        print(f"    {name}: {us:.1f} us mean over {calls} calls{extra}", flush=True)


if __name__ == "__main__":
    main()
