"""Per-sample learned edge weights (msgat_edge_weight_grad_sets) at R = 3, B = 32, N = 883, T = 12 (PEMSD7-like
synthetic graph), timed by HIP events after warm-up.

  kernels   the gradient entry points alone on the buffers of one forward, Cu = 24: msgat_edge_weight_grad (ONE [N,N]
            value set: the split kernel plus the reduction of its partial sums) against msgat_edge_weight_grad_sets with
            V = B (a set per sample, shared by the R relations) and V = R*B (a set per group); `calls` launches per
            event pair.  With a lab build (`python -m ms_gat_amd.build --lab`, `--lib build/lab/libmsgat_lab.so`)
            MSGAT_LAB_EWS_LINEAR=1 in the environment maps blocks to (set, tile) in plain order instead of one set per
            XCD label.  `--batch` sets B.
  steps     forward + backward through `ops.gacn` on the [R*B, ...] relation-major batch,
              (a) GACN 72 -> 24 (project first, Cu = 24)      (b) GACN 1 -> 24 (aggregate first, Cu = 1)
            with the adjacency frozen [N,N]; learned sparse [N,N] (`ops.edge_adjacency`, weight [nnz]); learned sparse
            per sample (`ops.edge_adjacency`, weight [B,nnz]: this feature); learned dense per sample (a [B,N,N] tensor
            that requires grad, msgat_adjacency_grad: the only way before).
  --profile the kernels' own times from `rocprofv3 --kernel-trace --stats` (a child process that runs `--kernels` only).

    python tools/batched_edge_weight_bench.py [--steps 20] [--warmup 3] [--kernels | --steps-only] [--profile] [--batch B] [--lib PATH]
"""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, ops  # noqa: E402
from ms_gat_amd.graph import graph_of  # noqa: E402

R, B, N, T, EDGES = 3, 32, 883, 12, 866
DEV = torch.device("cuda:0")
CASES = {"a": (72, 24), "b": (1, 24)}
MAPS = {"1": "linear", "0": "xcd"}    # MSGAT_LAB_EWS_LINEAR of a lab build


def timed(fn, steps, warmup, calls=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / calls)
    return statistics.median(t), min(t)


def kernels(steps, warmup, calls=20, Cu=24, sets_of=None):
    sets_of = sets_of or (B, R * B)
    L = _lib.lib()
    G = R * B
    g = torch.Generator().manual_seed(0)
    graph = graph_of(ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1))
    gstruct, keep = graph.on(DEV)
    nnz = graph.nnz
    shape = _lib.Shape(R, B, Cu, 0, N, T)
    dv, feat = (torch.randn(G, Cu, N, T, generator=g).to(DEV) for _ in range(2))
    q, kW = (torch.randn(G, N, T, generator=g).mul_(0.3).to(DEV) for _ in range(2))
    lse = torch.full((G, N), 8.0, device=DEV)
    stream = _lib.stream_handle(DEV)
    sp, gp = C.byref(shape), C.byref(gstruct)
    rows = []

    def one():
        nb = int(L.msgat_edge_weight_grad_workspace_bytes(sp, gp, Cu))
        ws = torch.empty(max(nb, 1), device=DEV, dtype=torch.uint8)
        out = torch.empty(nnz, device=DEV)
        return lambda: _lib.check(L.msgat_edge_weight_grad(sp, gp, Cu, dv.data_ptr(), 0, feat.data_ptr(), q.data_ptr(),
                                                           kW.data_ptr(), lse.data_ptr(), out.data_ptr(), ws.data_ptr(), nb,
                                                           stream), "msgat_edge_weight_grad"), out

    def sets(V):
        out = torch.empty((V, nnz), device=DEV)
        return lambda: _lib.check(L.msgat_edge_weight_grad_sets(sp, gp, Cu, dv.data_ptr(), 0, feat.data_ptr(), q.data_ptr(),
                                                                kW.data_ptr(), lse.data_ptr(), None, V, out.data_ptr(), None,
                                                                0, stream), "msgat_edge_weight_grad_sets"), out

    fn1, out1 = one()
    rows.append(("msgat_edge_weight_grad [N,N] (split kernel + reduction)", timed(fn1, steps, warmup, calls)))
    for V in sets_of:
        fn, out = sets(V)
        rows.append((f"msgat_edge_weight_grad_sets V = {V}", timed(fn, steps, warmup, calls)))
        torch.cuda.synchronize()
        # the sets add up to the one-set gradient (fp32 rounding of another order of additions)
        err = float((out.sum(0) - out1).abs().max() / out1.abs().max())
        assert err < 1e-4, err
    print(f"kernels at R={R} B={B} N={N} T={T} Cu={Cu} nnz={nnz}, {calls} launches per event pair, "
          f"map {MAPS.get(os.environ.get('MSGAT_LAB_EWS_LINEAR'), 'xcd')} "
          f"({os.path.basename(_lib.LIB_PATH)}):", flush=True)
    for name, (med, lo) in rows:
        print(f"  {name}: median {med * 1e3:.1f} us, fastest {lo * 1e3:.1f} us", flush=True)


def run_case(case, steps, warmup):
    C_, O = CASES[case]
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1).to(DEV)
    x = torch.randn(R * B, C_, N, T, generator=g).to(DEV).requires_grad_(True)
    alpha = ((torch.rand(R, C_, generator=g) * 2 - 1) * C_ ** -0.5).to(DEV).requires_grad_(True)
    Wg = (torch.randn(R, T, T, generator=g) * 0.3).to(DEV).requires_grad_(True)
    W = (torch.randn(R, O, C_, generator=g) * 0.2).to(DEV).requires_grad_(True)
    dz = torch.randn(R * B, O, N, T, generator=g).to(DEV)
    pattern = adj.to_sparse_csr()
    crow, col = pattern.crow_indices(), pattern.col_indices()
    weight = pattern.values().clone().requires_grad_(True)
    weights = (pattern.values()[None, :] * (0.5 + torch.rand(B, weight.numel(), device=DEV))).requires_grad_(True)
    dense = torch.zeros(B, N, N, device=DEV)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), crow[1:] - crow[:-1])
    dense[:, rows, col] = weights.detach()
    dense.requires_grad_(True)

    def step(make):
        x.grad = alpha.grad = Wg.grad = W.grad = None
        weight.grad = weights.grad = dense.grad = None
        ops.gacn(x, alpha, Wg, W, make()).backward(dz)

    makers = {"frozen [N,N]": lambda: adj,
              "learned sparse [N,N]": lambda: ops.edge_adjacency(crow, col, weight),
              "learned sparse [B,nnz]": lambda: ops.edge_adjacency(crow, col, weights),
              "learned dense [B,N,N]": lambda: dense}
    t = {mode: timed(lambda: step(make), steps, warmup)[0] for mode, make in makers.items()}
    print(f"({case}) GACN {C_}->{O} R={R} B={B} N={N} T={T} nnz={weight.numel()}: fwd+bwd "
          + ", ".join(f"{mode} {ms:.3f} ms" for mode, ms in t.items()), flush=True)


def profile(lib):
    out = tempfile.mkdtemp(prefix="bew_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "bew", "--", sys.executable,
           os.path.abspath(__file__), "--kernels", "--per-sample-only", "--steps", "5", "--warmup", "2"] + (["--lib", lib] if lib else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        print(f"rocprofv3 not run: {e}", flush=True)
        return
    if r.returncode != 0:
        print(f"rocprofv3 exited {r.returncode}: {r.stderr[-500:]}", flush=True)
        return
    print("rocprofv3 --kernel-trace --stats of the kernels run (V = B):", flush=True)
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "k_edge_weight_grad" in row["Name"] or "k_reduce" in row["Name"]:
                    print(f"  {row['Name']}: {float(row['AverageNs']) / 1e3:.1f} us mean over {row['Calls']} calls", flush=True)


def main():
    global B
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="the kernel timings only")
    ap.add_argument("--steps-only", action="store_true", help="the forward + backward steps only")
    ap.add_argument("--per-sample-only", action="store_true", help="of the sets kernel, V = B only")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--batch", type=int, default=B, help="samples B (the kernel timings: V = B and V = R*B)")
    ap.add_argument("--lib", help="another build of the library (a lab build)")
    a = ap.parse_args()
    B = a.batch
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if not a.steps_only:
        kernels(a.steps, a.warmup, sets_of=(B,) if a.per_sample_only else (B, R * B))
    if a.profile:
        profile(a.lib)
    if not a.kernels:
        for case in sorted(CASES):
            run_case(case, a.steps, a.warmup)


if __name__ == "__main__":
    main()
