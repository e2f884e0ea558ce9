#!/usr/bin/env python3
"""Generate the golden vectors of the Gauss loss by running the REFERENCE's `gauss_loss` (loss.py:75-95).

Run where the reference's sources are importable (`MSGAT_REFERENCE_SRC`, default as in make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss.py

Inputs are fp32 (what the kernels see); the loss and, through autograd, its gradient with respect to the prediction are
taken in float64 on exactly those values.  Data only: nothing of the reference's source travels.

  gauss_loss_ref.npz, case i under the keys `i.pred`, `i.truth` (fp32), `i.sigma_delta` [2], `i.loss`, `i.dpred` (fp64):
    0   [2,23,12]  errors ~30    sigma 1,  delta 0.05   the reference's defaults at flow-sized errors: mostly saturated
    1   the tensors of case 0    sigma 20, delta 0.5    both regimes
    2   [2,23,12]  errors ~1e-3  sigma 1,  delta 0      the cancellation case: 1 - exp(-t) with t ~ 5e-7
    3   [3,7,1]    errors ~4     sigma 1,  delta 0      five entries with pred == truth (gradient exactly 0 there)
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("MSGAT_REFERENCE_SRC", "/root/reference/src"))

from loss import gauss_loss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(1)


def tensors(shape, scale, seed, n_equal=0):
    g = torch.Generator().manual_seed(seed)
    truth = (20.0 + 380.0 * torch.rand(shape, generator=g)).float()
    pred = (truth + scale * torch.randn(shape, generator=g)).float()
    if n_equal:
        where = torch.randperm(truth.numel(), generator=g)[:n_equal]
        pred.reshape(-1)[where] = truth.reshape(-1)[where]
    return pred, truth


def case(pred, truth, sigma, delta):
    p = pred.double().requires_grad_(True)
    loss = gauss_loss(p, truth.double(), sigma, delta)
    loss.backward()
    return dict(pred=pred, truth=truth, sigma_delta=np.array([sigma, delta], dtype=np.float64), loss=loss.detach(), dpred=p.grad)


if __name__ == "__main__":
    big = tensors((2, 23, 12), 30.0, 401)
    cases = [case(*big, 1.0, 0.05), case(*big, 20.0, 0.5), case(*tensors((2, 23, 12), 1e-3, 402), 1.0, 0.0),
             case(*tensors((3, 7, 1), 4.0, 403, n_equal=5), 1.0, 0.0)]
    out = {f"{i}.{k}": (v.detach().numpy() if isinstance(v, torch.Tensor) else v) for i, c in enumerate(cases) for k, v in c.items()}
    path = os.path.join(HERE, "gauss_loss_ref.npz")
    np.savez_compressed(path, **out)
    print(f"gauss_loss_ref.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    for i, c in enumerate(cases):
        print(i, tuple(c["pred"].shape), c["sigma_delta"], float(c["loss"]), float(c["dpred"].abs().max()))
