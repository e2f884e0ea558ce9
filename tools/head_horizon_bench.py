"""Times the prediction head at long forecast horizons (T_out > 16 runs as ceil(T_out / 16) output tiles of 16) at PEMSD7
size, x [96,72,883,12] (three stacked components of a batch of 32), and the msgat72 R = 3 training step at T_out = 12
and 24.  HIP events; prints one JSON line.

    python tools/head_horizon_bench.py [--no-step] [--reps 20]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/head_horizon_bench.py
--no-step --reps 5` (k_head_fwd, k_lnhead_bwd, k_head_dW: one template each, T_out <= 16 is its one-tile instance)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ms_gat_amd import _lib, ops  # noqa: E402

HORIZONS = (12, 24, 36, 48, 64)


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3   # us


def head_entries(To, reps, dev):
    """The four head entry points, called directly (no autograd), at [96,72,883,12] with R = 3 stacked weights."""
    L = _lib.lib()
    B, R, C, N, T = 96, 3, 72, 883, 12
    g = torch.Generator(device="cpu").manual_seed(To)
    x = torch.randn(B, C, N, T, generator=g).to(dev)
    W = (torch.randn(R, To, T, 1, C, generator=g) * (T * C) ** -0.5).to(dev)
    hb, lw, lb = torch.zeros(R, To, device=dev), torch.ones(R, T, device=dev), torch.zeros(R, T, device=dev)
    dout = torch.randn(B, N, To, generator=g).to(dev)
    out = torch.empty(B, N, To, device=dev)
    xn, dx = torch.empty_like(x), torch.empty_like(x)
    dlw, dlb = torch.empty(R, T, device=dev), torch.empty(R, T, device=dev)
    dWc = torch.empty(R, C, To, T, device=dev)
    fwd_part = torch.empty(int(L.msgat_head_forward_partial_floats(B, C, N, To)), device=dev)
    bwd_part = torch.empty(int(L.msgat_layernorm_head_backward_partial_floats(B, C, N, T)), device=dev)
    dw_part = torch.empty(int(L.msgat_head_grad_weight_partial_floats(C, T, To, R)), device=dev)
    s = _lib.stream_handle(dev)
    p = ops._ptr

    def fwd(keep):
        _lib.check(L.msgat_head_forward_ln(p(x), p(lw), p(lb), 1e-5, p(W), p(hb), p(out), p(xn) if keep else None,
                                           p(fwd_part), B, C, N, T, To, R, s), "msgat_head_forward_ln")

    def bwd():
        _lib.check(L.msgat_layernorm_head_backward(p(dout), p(W), p(x), p(lw), p(dx), p(dlw), p(dlb), p(bwd_part), B, C, N,
                                                   T, To, R, 1e-5, 1, s), "msgat_layernorm_head_backward")

    def dw():
        _lib.check(L.msgat_head_grad_weight(p(dout), p(xn), p(dWc), p(dw_part), B, C, N, T, To, R, s),
                   "msgat_head_grad_weight")

    return {"fwd_inference_us": round(timeit(lambda: fwd(False), reps), 1),
            "fwd_training_us": round(timeit(lambda: fwd(True), reps), 1),
            "ln_head_backward_us": round(timeit(bwd, reps), 1),
            "grad_weight_us": round(timeit(dw, reps), 1)}


def training_step(To, hip_graph, reps, dev, tmp):
    """msgat72, R = 3 components (in_hours 1, 2, 3), PEMSD7-sized graph (883 nodes), batch 32: ms per Trainer step."""
    from ms_gat_amd import data, engine, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=883, n_edges=866, n_channels=1, in_hours=[1, 2, 3], out_timesteps=To, batch_size=32,
                            days=4)
    net = model.msgat72(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=To, use_te=True, adj=ds.adj).to(dev)
    batch = [t.to(dev) for t in next(iter(ds.training))]
    tr = engine.Trainer(net, 50.0, os.path.join(tmp, f"to{To}_{int(hip_graph)}"), hip_graph=hip_graph)
    batches = [batch] * reps
    tr.run_epoch(batches[:3], gpu_id=0, epoch=1, mode="train")   # warm-up (and, replayed, the capture)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    tr.run_epoch(batches, gpu_id=0, epoch=2, mode="train")
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / reps, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="head entry points only (the rocprofv3 run)")
    ap.add_argument("--horizons", default=",".join(map(str, HORIZONS)), help="comma-separated T_out values")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "head_horizon_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"shape": [96, 72, 883, 12], "R": 3, "head": {}}
    for To in map(int, args.horizons.split(",")):
        res["head"][str(To)] = head_entries(To, args.reps, dev)
    if not args.no_step:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            res["train_step_ms"] = {f"{To}_{'replayed' if g else 'eager'}": training_step(To, g, args.reps, dev, tmp)
                                    for To in (12, 24) for g in (False, True)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
