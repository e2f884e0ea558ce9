#!/usr/bin/env python3
"""Generate the golden vectors of the adjacency's gradient by running the REFERENCE.

Run where the reference's sources are importable (`MSGAT_REFERENCE_SRC`, default as in make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adjacency.py

The reference's `att * adjacency` (attention.py:36) is an ordinary product, so an adjacency that requires grad gets
dadj = sum over the batch of softmax(S) * (dout . x^T): dense, non-zero where the adjacency is 0.  Every fixture runs the
reference's module on the CPU with `adjacency.requires_grad_(True)` and records the forward, every gradient and dadj.
The adjacencies have zeros, asymmetric weights and one all-zero row.  Inputs and output gradients are fp16-exact
(stored as fp16) or int8 multiples of 1/32 (the 72-channel case).  Data only: nothing of the reference's source travels.

  adjgrad_gatt_b2c3n64.npz       GraphAttention(C = 3), N = 64, B = 2, one [N,N] adjacency
  adjgrad_gacn_b2c3n64.npz       GACN(3 -> 24), N = 64, B = 2      (aggregate first)
  adjgrad_gacn_b2c72n47.npz      GACN(72 -> 24), N = 47, B = 2     (project first; N % 4 != 0)
  adjgrad_gacn_b3c3n64_bnn.npz   GACN(3 -> 24), N = 64, B = 3, a per-sample [B,N,N] adjacency
  adjgrad_meam_72to72_n32.npz    MEAM(72 -> 72), N = 32, B = 2     (the merged branches: attention core), its state_dict
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("MSGAT_REFERENCE_SRC", "/root/reference/src"))

from models.attention import GraphAttention  # noqa: E402
from models.msgat import GACN, MEAM  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


def learned_adjacency(N, seed, B=None):
    """[N,N] (or [B,N,N]): a random sparse pattern (about N/2 undirected edges + self loops) with independent weights in
    [0.25, 1.5) per direction -- asymmetric -- and row 5 all zero."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B or 1):
        a = np.eye(N)
        got = 0
        while got < N // 2:
            s, d = rng.integers(0, N, size=2)
            if s == d or a[s, d] != 0:
                continue
            a[s, d] = a[d, s] = 1.0
            got += 1
        a = a * rng.uniform(0.25, 1.5, size=(N, N))
        a[5] = 0.0
        out.append(a.astype(np.float32))
    return np.stack(out) if B else out[0]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def save(name, **arrays):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def params(rng, C, T, O):
    Wg = (rng.standard_normal((T, T)) * (2.0 / (T + T)) ** 0.5).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, size=C).astype(np.float32)
    W = (rng.standard_normal((O, C)) * (2.0 / (O + C)) ** 0.5).astype(np.float32) if O else None
    return Wg, alpha, W


def gatt_case(B, C, N, seed):
    T = 12
    rng = np.random.default_rng(seed)
    x16 = rng.standard_normal((B, C, N, T)).astype(np.float16)
    dy16 = rng.standard_normal((B, C, N, T)).astype(np.float16)
    adj = learned_adjacency(N, seed + 1)
    Wg, alpha, _ = params(rng, C, T, 0)
    m = GraphAttention(C, T)
    with torch.no_grad():
        m.Wg.copy_(t(Wg))
        m.alpha.copy_(t(alpha))
    xt = t(x16.astype(np.float32)).requires_grad_(True)
    at = t(adj).requires_grad_(True)
    y = m(xt, at)
    y.backward(t(dy16.astype(np.float32)))
    save(f"adjgrad_gatt_b{B}c{C}n{N}.npz", x=x16, adj=adj, Wg=Wg, alpha=alpha, dy=dy16, y=y, dx=xt.grad,
         dWg=m.Wg.grad, dalpha=m.alpha.grad, dadj=at.grad)


def gacn_case(B, C, O, N, seed, int8_inputs=False, batched=False):
    T = 12
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, N, T))
    x = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)     # LayerNorm output, as msgat.py:122 feeds it
    dz = rng.standard_normal((B, O, N, T))
    if int8_inputs:   # multiples of 1/32: exact in fp32, a quarter of the bytes
        xs = np.clip(np.rint(x * 32), -127, 127).astype(np.int8)
        dzs = np.clip(np.rint(dz * 32), -127, 127).astype(np.int8)
        x32, dz32 = xs.astype(np.float32) / 32, dzs.astype(np.float32) / 32
        stored = dict(x_q32=xs, dz_q32=dzs)
    else:
        xs, dzs = x.astype(np.float16), dz.astype(np.float16)
        x32, dz32 = xs.astype(np.float32), dzs.astype(np.float32)
        stored = dict(x=xs, dz=dzs)
    adj = learned_adjacency(N, seed + 1, B if batched else None)
    Wg, alpha, W = params(rng, C, T, O)
    g = GACN(C, O, T)
    with torch.no_grad():
        g.gatt.Wg.copy_(t(Wg))
        g.gatt.alpha.copy_(t(alpha))
        g.W.copy_(t(W))
    xt = t(x32).requires_grad_(True)
    at = t(adj).requires_grad_(True)
    z = g(xt, at)
    z.backward(t(dz32))
    save(f"adjgrad_gacn_b{B}c{C}n{N}{'_bnn' if batched else ''}.npz", adj=adj, Wg=Wg, alpha=alpha, W=W, z=z, dx=xt.grad,
         dWg=g.gatt.Wg.grad, dalpha=g.gatt.alpha.grad, dW=g.W.grad, dadj=at.grad, **stored)


def meam_case(B, cin, cout, N, seed, dilations=(1, 2)):
    torch.manual_seed(seed)
    T = 12
    m = MEAM(cin, cout, n_nodes=N, n_timesteps=T, dilations=list(dilations))
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim >= 2:
                torch.nn.init.xavier_normal_(p)
            else:
                torch.nn.init.uniform_(p, -p.size(0) ** -0.5, p.size(0) ** -0.5)
    adj = learned_adjacency(N, seed + 1)
    at = t(adj).requires_grad_(True)
    x = torch.randn(B, cin, N, T).half().float().requires_grad_(True)
    dout = torch.randn(B, cout, N, T).half().float()
    out = m(x, at)
    out.backward(dout)
    arrays = {f"p.{k}": v for k, v in m.state_dict().items()}
    arrays.update({f"g.{k}": p.grad for k, p in m.named_parameters()})
    save(f"adjgrad_meam_{cin}to{cout}_n{N}.npz", x=x.detach().half(), adj=adj, dout=dout.half(), out=out, dx=x.grad,
         dadj=at.grad, **arrays)


if __name__ == "__main__":
    gatt_case(2, 3, 64, seed=201)
    gacn_case(2, 3, 24, 64, seed=202)
    gacn_case(2, 72, 24, 47, seed=203, int8_inputs=True)
    gacn_case(3, 3, 24, 64, seed=204, batched=True)
    meam_case(2, 72, 72, 32, seed=205)
