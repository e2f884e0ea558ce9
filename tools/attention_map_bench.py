"""Reading the graph attention (need_weights), timed by HIP events after warm-up on a PEMSD7-like synthetic graph:

  map    msgat_attention_map alone on a saved forward: G = 32, N = 883, T = 12 (99.8 MB of writes) and G = 64, N = 8192
         (17.2 GB), against the write bound at the measured 6.29 TB/s copy rate
  fwd    GACN 72 -> 24 forward, B = 32, N = 883: plain vs need_weights=True (masked: one G nnz copy more)
  bwd    the same GACN's backward, the adjacency frozen: plain; with an extra edge gradient at the weights' values as the
         autograd Function hands them out (msgat_gacn_backward_edge_grad: the library's own difference); and the same
         through the sparse COO tensor the caller gets (+ torch's sparse autograd nodes)

    python tools/attention_map_bench.py [--steps 20] [--warmup 3] [--skip-large]
    python tools/attention_map_bench.py --trace-bwd plain|extra     # only that backward, 50 times: for
        rocprofv3 --kernel-trace --stats -- python tools/attention_map_bench.py --trace-bwd extra
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
HBM_TBS = 6.29
T = 12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def gacn_module(C, Co):
    torch.manual_seed(0)
    m = ms_gat_amd.GACN(C, Co, T).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.2)
    return m


def map_case(G, N, steps, warmup):
    """The map kernel alone: q / kW / lse of a real forward, then msgat_attention_map into a preallocated output."""
    from ms_gat_amd import _lib
    import ctypes as C
    adj = ms_gat_amd.synthetic_adjacency(N, N, seed=1).to(DEV)
    q, kW, lse = torch.randn(G, N, T, device=DEV), torch.empty(G, N, T, device=DEV), torch.empty(G, N, device=DEV)
    Wg = torch.randn(1, T, T, device=DEV) * 0.3
    graph = ms_gat_amd.graph_of(adj)
    plan = ops._gacn_plan(graph, DEV, 1, G, 1, 0, N, T, False, own_q=False)
    buf = torch.empty(plan.total, device=DEV)
    _, kWp, lsep, _, E, _, _ = plan.pointers(buf)
    dense = torch.empty(plan.ndense, device=DEV, dtype=torch.uint8) if plan.ndense else None
    L = _lib.lib()
    stream = _lib.stream_handle(DEV)
    _lib.check(L.msgat_stage_scores(C.byref(plan.shape), C.byref(plan.gstruct), q.data_ptr(), Wg.data_ptr(), kWp, lsep,
                                    None, E, None, None if dense is None else dense.data_ptr(), stream), "scores")
    out = torch.empty(G, N, N, device=DEV)
    us = timed(lambda: L.msgat_attention_map(C.byref(plan.shape), q.data_ptr(), kWp, lsep, out.data_ptr(), stream),
               steps, warmup)
    rows = out[0].sum(-1)
    nbytes = 4.0 * G * N * N
    return us, nbytes, float((rows - 1).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--trace-bwd", choices=["plain", "extra"], default=None)
    a = ap.parse_args()
    if a.trace_bwd:
        return trace_bwd(a.trace_bwd)
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, median of {a.steps} after {a.warmup} warm-up")
    for G, N in ((32, 883),) + (() if a.skip_large else ((64, 8192),)):
        us, nbytes, rs = map_case(G, N, a.steps, a.warmup)
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        print(f"map    G={G:3d} N={N:5d} T={T}: {us:9.1f} us  {nbytes / 1e6:9.1f} MB written  {nbytes / us / 1e6:5.2f} TB/s"
              f"  (write bound at {HBM_TBS} TB/s: {bound:.1f} us)  max|row sum - 1| = {rs:.1e}")
        torch.cuda.empty_cache()

    B, N, C, Co = 32, 883, 72, 24
    adj = ms_gat_amd.synthetic_adjacency(N, 866, seed=1).to(DEV)
    m = gacn_module(C, Co)
    x = torch.randn(B, C, N, T, device=DEV, requires_grad=True)
    dz = torch.randn(B, Co, N, T, device=DEV)
    nnz = ms_gat_amd.graph_of(adj).nnz
    with torch.no_grad():
        f0 = timed(lambda: m(x, adj), a.steps, a.warmup)
        f1 = timed(lambda: m(x, adj, need_weights=True), a.steps, a.warmup)
    print(f"fwd    [{B}, {C}->{Co}, {N}, {T}] nnz={nnz}: plain {f0:.1f} us, need_weights (masked) {f1:.1f} us "
          f"(+{f1 - f0:.1f} us; the copy is {4 * B * nnz / 1e6:.2f} MB)")

    y, yv, wv, dM = bwd_setup(m, x, adj)
    yw, w = m(x, adj, need_weights=True)
    b0 = timed(lambda: torch.autograd.grad(y, [x], dz, retain_graph=True), a.steps, a.warmup)
    b1 = timed(lambda: torch.autograd.grad([yv, wv], [x], [dz, dM], retain_graph=True), a.steps, a.warmup)
    b2 = timed(lambda: torch.autograd.grad([yw, w.values()], [x], [dz, dM.reshape(-1)], retain_graph=True), a.steps,
               a.warmup)
    print(f"bwd    [{B}, {C}->{Co}, {N}, {T}]: plain {b0:.1f} us; with the weights' edge gradient {b1:.1f} us "
          f"(+{b1 - b0:.1f} us); the same through the sparse tensor {b2:.1f} us (+{b2 - b0:.1f} us)")


def bwd_setup(m, x, adj):
    """(plain output, output and [G,nnz] weight values of a call that hands out its weights, their gradient)"""
    y = m(x, adj)
    with ops.collect_weights("masked") as seen:
        yv = m(x, adj)
    wv = seen[0][0]
    return y, yv, wv, torch.randn_like(wv)


def trace_bwd(which):
    B, N, C, Co = 32, 883, 72, 24
    adj = ms_gat_amd.synthetic_adjacency(N, 866, seed=1).to(DEV)
    m = gacn_module(C, Co)
    x = torch.randn(B, C, N, T, device=DEV, requires_grad=True)
    dz = torch.randn(B, Co, N, T, device=DEV)
    y, yv, wv, dM = bwd_setup(m, x, adj)
    for _ in range(50):
        if which == "plain":
            torch.autograd.grad(y, [x], dz, retain_graph=True)
        else:
            torch.autograd.grad([yv, wv], [x], [dz, dM], retain_graph=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
