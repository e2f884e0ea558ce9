"""A gradient at the dense softmax map (weights="softmax_grad"), timed by HIP events after warm-up on a PEMSD7-like
synthetic graph, in one process:

  (a) map    msgat_attention_map alone: it writes the 4 G N^2 bytes that the map gradient reads, the yardstick
  (b) grad   msgat_softmax_map_grad alone (row pass, column pass, the dWg partials and their sum) on a saved forward:
             G = 32, N = 883, T = 12 (99.8 MB of dP, read twice) and G = 8, N = 8192 (2.1 GB)
  (c) bwd    GACN 72 -> 24 backward, B = 32, N = 883: plain, and with a gradient at the map
  (d) dense  the same loss <dz, y> + <dP, att> through the dense PyTorch-ROCm autograd formulation, forward + backward

    python tools/softmax_grad_bench.py [--steps 20] [--warmup 3] [--skip-large]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, ops  # noqa: E402

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


def kernel_case(G, N, steps, warmup):
    """(map us, map-gradient us) on the q / kW / lse of a real score pass."""
    adj = ms_gat_amd.synthetic_adjacency(N, N, seed=1).to(DEV)
    q, Wg = torch.randn(G, N, T, device=DEV), torch.randn(1, T, T, device=DEV) * 0.3
    graph = ms_gat_amd.graph_of(adj)
    plan = ops._gacn_plan(graph, DEV, 1, G, 1, 0, N, T, False, own_q=False)
    buf = torch.empty(plan.total, device=DEV)
    _, kW, lse, _, E, _, _ = plan.pointers(buf)
    dense = torch.empty(plan.ndense, device=DEV, dtype=torch.uint8) if plan.ndense else None
    L = _lib.lib()
    stream = _lib.stream_handle(DEV)
    shape = C.byref(plan.shape)
    _lib.check(L.msgat_stage_scores(shape, C.byref(plan.gstruct), q.data_ptr(), Wg.data_ptr(), kW, lse, None, E, None,
                                    None if dense is None else dense.data_ptr(), stream), "scores")
    dP = torch.empty(G, N, N, device=DEV)
    t_map = timed(lambda: L.msgat_attention_map(shape, q.data_ptr(), kW, lse, dP.data_ptr(), stream), steps, warmup)
    dP.normal_()
    dq, dWg = torch.zeros_like(q), torch.zeros_like(Wg)
    ws = torch.empty(max(int(L.msgat_softmax_map_grad_workspace_bytes(shape)), 256), device=DEV, dtype=torch.uint8)
    t_grad = timed(lambda: _lib.check(L.msgat_softmax_map_grad(shape, q.data_ptr(), kW, lse, Wg.data_ptr(), dP.data_ptr(),
                                                               dq.data_ptr(), dWg.data_ptr(), ws.data_ptr(), ws.numel(),
                                                               stream), "map_grad"), steps, warmup)
    return t_map, t_grad, 4.0 * G * N * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; HIP events, median of {a.steps} after {a.warmup} warm-up")
    for G, N in ((32, 883),) + (() if a.skip_large else ((8, 8192),)):
        t_map, t_grad, nbytes = kernel_case(G, N, a.steps, a.warmup)
        print(f"(a) map   G={G:3d} N={N:5d} T={T}: {t_map:9.1f} us  {nbytes / 1e6:8.1f} MB written  {nbytes / t_map / 1e6:5.2f} TB/s")
        print(f"(b) grad  G={G:3d} N={N:5d} T={T}: {t_grad:9.1f} us  {2 * nbytes / 1e6:8.1f} MB read (dP twice)  "
              f"{2 * nbytes / t_grad / 1e6:5.2f} TB/s = {2 * nbytes / t_grad / 1e6 / HBM_TBS * 100:.0f} % of the {HBM_TBS} TB/s copy rate;"
              f"  {t_grad / t_map:.2f} x (a)")
        torch.cuda.empty_cache()

    B, N, Ci, Co = 32, 883, 72, 24
    adj = ms_gat_amd.synthetic_adjacency(N, 866, seed=1).to(DEV)
    torch.manual_seed(0)
    m = ms_gat_amd.GACN(Ci, Co, T).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.2)
    x = torch.randn(B, Ci, N, T, device=DEV, requires_grad=True)
    dz = torch.randn(B, Co, N, T, device=DEV)
    dP = torch.randn(B, N, N, device=DEV)
    y = m(x, adj)
    yw, w = m(x, adj, need_weights=True, weights="softmax_grad")
    b0 = timed(lambda: torch.autograd.grad(y, [x], dz, retain_graph=True), a.steps, a.warmup)
    b1 = timed(lambda: torch.autograd.grad([yw, w], [x], [dz, dP], retain_graph=True), a.steps, a.warmup)
    print(f"(c) bwd   [{B}, {Ci}->{Co}, {N}, {T}]: plain {b0:.1f} us; with the gradient at the map {b1:.1f} us (+{b1 - b0:.1f} us)")
    del y, yw, w

    def dense_step():
        q = torch.einsum("c,bcnt->bnt", m.gatt.alpha, x)
        att = torch.softmax(q @ m.gatt.Wg @ q.transpose(1, 2), dim=-1)
        z = torch.einsum("oc,bcnt->bont", m.W, torch.einsum("bnm,bcmt->bcnt", att * adj, x))
        torch.autograd.grad([z, att], [x, m.gatt.alpha, m.gatt.Wg, m.W], [dz, dP])

    def ours_step():
        z, att = m(x, adj, need_weights=True, weights="softmax_grad")
        torch.autograd.grad([z, att], [x, m.gatt.alpha, m.gatt.Wg, m.W], [dz, dP])

    d = timed(dense_step, a.steps, a.warmup)
    o = timed(ours_step, a.steps, a.warmup)
    print(f"(d) step  forward + backward of <dz, y> + <dP, att>: dense PyTorch-ROCm autograd {d:.1f} us; this library {o:.1f} us"
          f" ({d / o:.1f} x)")


if __name__ == "__main__":
    main()
