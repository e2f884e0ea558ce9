"""The gradient of the adjacency (msgat_adjacency_grad) at R = 3, B = 32, N = 883, T = 12 (PEMSD7-like synthetic graph),
through `ops.gacn` on the [R*B, ...] relation-major batch, timed by HIP events after warm-up:

  (a) GACN 72 -> 24 (project first), one [N,N] adjacency      dadj summed over all 96 groups
  (b) GACN  1 -> 24 (aggregate first), one [N,N] adjacency    Cu = 1: the score product and the exp set the cost
  (c) as (a) with a per-sample [32,N,N] adjacency             100 MB of dadj written

For each case: forward + backward with the adjacency frozen and with it requiring grad (the difference is what the
gradient adds), the eager PyTorch-ROCm autograd of the reference's formulation (oracle.dense_torch.gacn_dense, float32,
adjacency requiring grad) on the same batch, and with `--profile` the kernel's own time from `rocprofv3 --kernel-trace
--stats` (a child process of this script per case), against the matrix-core bound 2 G N^2 (Cu + 1) T / 155 TF.

    python tools/adjacency_grad_bench.py [--steps 20] [--warmup 3] [--profile]
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
PEAK_TF = 155.0   # measured FP32 matrix-core rate, v_mfma_f32_16x16x4_f32
DEV = torch.device("cuda:0")
CASES = {"a": (72, 24, False), "b": (1, 24, False), "c": (72, 24, True)}


def setup(case):
    C, O, batched = CASES[case]
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    if batched:
        adj = adj.unsqueeze(0) * (torch.rand(B, N, N, generator=g) + 0.5)
    x = torch.randn(R * B, C, N, T, generator=g).to(DEV)
    alpha = ((torch.rand(R, C, generator=g) * 2 - 1) * C ** -0.5).to(DEV).requires_grad_(True)
    Wg = (torch.randn(R, T, T, generator=g) * 0.3).to(DEV).requires_grad_(True)
    W = (torch.randn(R, O, C, generator=g) * 0.2).to(DEV).requires_grad_(True)
    dz = torch.randn(R * B, O, N, T, generator=g).to(DEV)
    return adj.to(DEV), x.requires_grad_(True), alpha, Wg, W, dz


def flops(case):
    C, O, _ = CASES[case]
    Cu = O if C > O else C
    G = R * B
    return 2.0 * G * N * N * Cu * T, 2.0 * G * N * N * T


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


def run_case(case, steps, warmup, eager=True):
    adj, x, alpha, Wg, W, dz = setup(case)
    learned = adj.clone().requires_grad_(True)

    def step(a):
        x.grad = alpha.grad = Wg.grad = W.grad = None
        learned.grad = None
        ops.gacn(x, alpha, Wg, W, a).backward(dz)

    out = {"frozen": timed(lambda: step(adj), steps, warmup), "learned": timed(lambda: step(learned), steps, warmup)}
    if eager:
        def eager_step():
            a = adj.clone().requires_grad_(True)
            xs = x.detach().requires_grad_(True)
            zs = []
            for r in range(R):
                zs.append(dense_torch.gacn_dense(xs[r * B:(r + 1) * B], a, Wg[r].detach(), alpha[r].detach(), W[r].detach()))
            torch.cat(zs).backward(dz)
        out["eager_rocm"] = timed(eager_step, max(3, steps // 4), 1)
    return out


def profile(case):
    """k_adjacency_grad (and the partial sums' reduction) from rocprofv3 --kernel-trace --stats in a child process"""
    out = tempfile.mkdtemp(prefix="ag_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ag", "--", sys.executable,
           os.path.abspath(__file__), "--only", case, "--no-eager", "--steps", "10", "--warmup", "2"]
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
    a = ap.parse_args()
    for case in ([a.only] if a.only else sorted(CASES)):
        C, O, batched = CASES[case]
        t = run_case(case, a.steps, a.warmup, eager=not a.no_eager)
        fh, fs = flops(case)
        line = (f"({case}) GACN {C}->{O} R={R} B={B} N={N} T={T} adjacency {'[32,N,N]' if batched else '[N,N]'}: "
                f"fwd+bwd frozen {t['frozen']:.3f} ms, learned {t['learned']:.3f} ms (+{t['learned'] - t['frozen']:.3f})")
        if "eager_rocm" in t:
            line += f"; eager PyTorch-ROCm autograd {t['eager_rocm']:.3f} ms"
        print(line, flush=True)
        if a.profile and not a.only:
            rows = profile(case)
            if rows:
                for name, (us, calls) in sorted(rows.items()):
                    if "k_adjacency_grad" in name or "k_reduce_few" in name or "k_bwd_dense_col" in name:
                        extra = ""
                        if "k_adjacency_grad" in name:
                            bound = (fh + fs) / (PEAK_TF * 1e12) * 1e6
                            extra = (f"  H {fh / 1e9:.1f} + S {fs / 1e9:.1f} GFLOP: bound {bound:.0f} us, "
                                     f"{bound / us:.2f} of the {PEAK_TF:.0f} TF peak")
                        print(f"    {name}: {us:.1f} us mean over {calls} calls{extra}", flush=True)


if __name__ == "__main__":
    main()
