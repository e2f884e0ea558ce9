"""Times the masked step tail beside the unmasked one, in one process on one GPU:

    python tools/masked_tail_bench.py [--iters 200]

For [rows, T_out] = [32 * 883, 12] and [32 * 883, 64]: the metrics pass (main kernel + finish launch) and the gradient
kernel of `msgat_huber_*` and of `msgat_masked_huber_*`, through the C ABI, as the mean of `iters` back-to-back calls
between two device events after a warm-up (the tensors stay in the Infinity Cache: these are the times a training step
sees, not HBM-cold ones).  Prints one line per measurement and a JSON line at the end.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ms_gat_amd import _lib  # noqa: E402


def timed(fn, iters):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_tail_bench.py needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    out = {}
    for rows, t_out in ((32 * 883, 12), (32 * 883, 64)):
        g = torch.Generator().manual_seed(0)
        truth = (20 + 380 * torch.rand(rows, t_out, generator=g))
        truth[torch.rand(rows, t_out, generator=g) < 0.2] = 0.0
        pred = (truth + 60 * torch.randn(rows, t_out, generator=g)).to(dev)
        truth = truth.to(dev)
        n = rows * t_out
        stream = torch.cuda.current_stream(dev).cuda_stream
        part = torch.empty(int(L.msgat_huber_partial_doubles(n)), device=dev, dtype=torch.float64)
        mpart = torch.empty(int(L.msgat_masked_huber_partial_doubles(rows, t_out)), device=dev, dtype=torch.float64)
        loss, valid, dloss = torch.empty((), device=dev), torch.empty(1, device=dev), torch.ones((), device=dev)
        sums = torch.zeros(4, device=dev, dtype=torch.float64)
        msums = torch.zeros(t_out + 1, 5, device=dev, dtype=torch.float64)
        dpred = torch.empty_like(pred)
        p, y = pred.data_ptr(), truth.data_ptr()
        calls = {
            "huber_metrics": lambda: L.msgat_huber_metrics(p, y, n, 50.0, 0.0, part.data_ptr(), loss.data_ptr(), sums.data_ptr(), 1.0, stream),
            "masked_huber_metrics": lambda: L.msgat_masked_huber_metrics(p, y, rows, t_out, 50.0, 0.0, 0.0, mpart.data_ptr(), loss.data_ptr(),
                                                                         valid.data_ptr(), msums.data_ptr(), stream),
            "huber_grad": lambda: L.msgat_huber_grad(p, y, dloss.data_ptr(), n, 50.0, dpred.data_ptr(), stream),
            "masked_huber_grad": lambda: L.msgat_masked_huber_grad(p, y, dloss.data_ptr(), valid.data_ptr(), rows, t_out, 50.0, 0.0,
                                                                   dpred.data_ptr(), stream),
        }
        for name, fn in calls.items():
            assert fn() == 0, name
            us = timed(fn, args.iters)
            out[f"{name}[{rows},{t_out}]"] = round(us, 2)
            print(f"[{rows:6d},{t_out:3d}] {name:22s} {us:8.2f} us  ({part.numel() if 'masked' not in name else mpart.numel()} partial doubles)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
