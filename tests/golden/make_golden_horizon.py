#!/usr/bin/env python3
"""Generate the golden vectors of long forecast horizons (T_out > 16) by running the REFERENCE.

Run where the reference's sources are importable (`MSGAT_REFERENCE_SRC`, default as in make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_horizon.py

The horizon is the reference's `--out-timesteps` (main.py:34); it sizes the component head Conv2d(T_in -> T_out, [1, C])
(msgat.py:153,159) and the time embedding (msgat.py:187).  Each fixture is a whole model forward, HuberLoss(50)
(loss.py:51-52) and every gradient, as msgat72_n32.npz is for T_out = 12, except that the two time-embedding tables and
their gradients are stored as the rows H and D select (`rows.*`, `grows.*`; every other row is zero in the gradient and
cannot influence the forward).  Inputs are fp16-exact (stored as fp16).
Data only: nothing of the reference's source travels.

  msgat72_to24_n32.npz   msgat72, R = 3, C = 3, T = 12, T_out = 24, N = 32, B = 2   (two output tiles, the second partial)
  msgat48_to40_n23.npz   msgat48, R = 2, C = 1, T = 8,  T_out = 40, N = 23, B = 2   (three tiles, the last partial)
  msgat48_to64_n24.npz   msgat48, R = 1, C = 2, T = 16, T_out = 64, N = 24, B = 2   (four full tiles: the limit)
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("MSGAT_REFERENCE_SRC", "/root/reference/src"))

from models.msgat import msgat48, msgat72  # noqa: E402
from loss import HuberLoss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


def synthetic_adjacency(n, n_edges, seed):
    """N nodes, E distinct undirected non-self edges, then D^-1/2 (A+I) D^-1/2 (as make_golden.py)."""
    rng = np.random.default_rng(seed)
    a = np.eye(n, dtype=np.float64)
    got = 0
    while got < n_edges:
        s, d = rng.integers(0, n, size=2)
        if s == d or a[s, d] != 0:
            continue
        a[s, d] = a[d, s] = 1.0
        got += 1
    r = 1.0 / np.sqrt(a.sum(1))
    return (r[:, None] * a * r[None, :]).astype(np.float32)


def save(name, **arrays):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def model_case(name, factory, R, C, T, To, N, B, seed):
    torch.manual_seed(seed)
    adj = synthetic_adjacency(N, N, seed + 1)
    net = factory(n_components=R, in_channels=C, in_timesteps=T, out_timesteps=To, use_te=True,
                  adj=torch.from_numpy(adj))
    X = torch.randn(B, R, C, N, T).half().float()
    H = torch.randint(0, 24, (B,))
    D = torch.randint(0, 7, (B,))
    Y = (torch.randn(B, N, To) * 60.0).half().float()   # large enough that both Huber branches are taken at delta = 50
    pred = net(X, H, D)
    loss = HuberLoss(50.0)(pred, Y)
    loss.backward()
    # the time-embedding tables are [24 | 7, R*N*T_out]: only the rows H and D select can influence the forward, and
    # only those rows receive a gradient -- both are stored as those rows (as msgat72_cfg1_pemsd4.npz does)
    arrays = {}
    for k, v in net.state_dict().items():
        rows = {"te.h_ebd.weight": H, "te.d_ebd.weight": D}.get(k)
        arrays[f"p.{k}" if rows is None else f"rows.{k}"] = v if rows is None else v[rows]
    for k, p in net.named_parameters():
        rows = {"te.h_ebd.weight": H, "te.d_ebd.weight": D}.get(k)
        if p.grad is not None:
            arrays[f"g.{k}" if rows is None else f"grows.{k}"] = p.grad if rows is None else p.grad[rows]
    save(name, X=X.half(), H=H, D=D, Y=Y.half(), pred=pred, loss=loss, **arrays)


if __name__ == "__main__":
    model_case("msgat72_to24_n32.npz", msgat72, R=3, C=3, T=12, To=24, N=32, B=2, seed=301)
    model_case("msgat48_to40_n23.npz", msgat48, R=2, C=1, T=8, To=40, N=23, B=2, seed=302)
    model_case("msgat48_to64_n24.npz", msgat48, R=1, C=2, T=16, To=64, N=24, B=2, seed=303)
