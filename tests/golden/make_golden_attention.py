#!/usr/bin/env python3
"""Generate the golden vectors of the attention weights by running the REFERENCE.

Run where the reference's sources are importable (`MSGAT_REFERENCE_SRC`, default as in make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attention.py

The reference's graph attention forms `att = softmax(k Wg q^T)` and `att * adjacency` (attention.py:34, :36) as ordinary
tensors.  While its module runs on the CPU, `torch.softmax` and `torch.einsum` are wrapped to capture them: `att` is the
softmax whose output is [B,N,N], and `att * adjacency` is the first operand of the aggregation einsum "bni,bcit->bcnt".
The loss is <dY, y> + <dM, att * adjacency>, with dM zero off the graph's structure (the non-zeros of the adjacency, the
union of the samples' for a per-sample one): the library hands out the weights at those indices only.  Recorded: att,
att * adjacency, y and every gradient, the adjacency's included.  Inputs and output gradients are fp16-exact (stored as
fp16) or int8 multiples of 1/32 (the 72-channel cases).  Data only: nothing of the reference's source travels.

  attw_gatt_b2c3n64.npz        GraphAttention(C = 3), N = 64, B = 2, an all-zero row, asymmetric weights
  attw_gacn_b2c3n64.npz        GACN(3 -> 24), N = 64, B = 2       (aggregate first)
  attw_gacn_b2c72n47.npz       GACN(72 -> 24), N = 47, B = 2      (project first; N % 4 != 0)
  attw_gacn_b3c3n64_bnn.npz    GACN(3 -> 24), N = 64, B = 3, a per-sample [B,N,N] adjacency that requires grad
  attw_meam_72to72_n32.npz     MEAM(72 -> 72), N = 32, B = 2      (the merged branches: attention core), its state_dict
"""
import contextlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("MSGAT_REFERENCE_SRC", "/root/reference/src"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from models.attention import GraphAttention  # noqa: E402
from models.msgat import GACN, MEAM  # noqa: E402

from make_golden_adjacency import learned_adjacency, params, t  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


@contextlib.contextmanager
def capture(N):
    """Yields a dict that receives `att` (the [B,N,N] softmax) and `M` (the operand `att * adjacency` of the
    aggregation) of the graph attention that runs inside the block."""
    seen = {}
    softmax, einsum = torch.softmax, torch.einsum

    def softmax_(x, *a, **k):
        out = softmax(x, *a, **k)
        if out.dim() == 3 and out.shape[-2:] == (N, N):
            assert "att" not in seen, "one graph attention per captured call"
            seen["att"] = out
        return out

    def einsum_(eq, *ops):
        if eq == "bni,bcit->bcnt":
            seen["M"] = ops[0]
        return einsum(eq, *ops)

    torch.softmax, torch.einsum = softmax_, einsum_
    try:
        yield seen
    finally:
        torch.softmax, torch.einsum = softmax, einsum


def structure_dM(rng, B, adj):
    mask = (adj != 0) if adj.ndim == 2 else (adj != 0).any(axis=0)
    return (rng.standard_normal((B,) + mask.shape) * mask).astype(np.float16)


def save(name, **arrays):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def inputs(rng, B, C, O, N, int8_inputs):
    T = 12
    x = rng.standard_normal((B, C, N, T))
    x = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)
    dy = rng.standard_normal((B, O, N, T))
    if int8_inputs:
        xs = np.clip(np.rint(x * 32), -127, 127).astype(np.int8)
        dys = np.clip(np.rint(dy * 32), -127, 127).astype(np.int8)
        return xs.astype(np.float32) / 32, dys.astype(np.float32) / 32, dict(x_q32=xs, dy_q32=dys)
    xs, dys = x.astype(np.float16), dy.astype(np.float16)
    return xs.astype(np.float32), dys.astype(np.float32), dict(x=xs, dy=dys)


def gatt_case(B, C, N, seed):
    T = 12
    rng = np.random.default_rng(seed)
    x, dy, stored = inputs(rng, B, C, C, N, False)
    adj = learned_adjacency(N, seed + 1)
    dM = structure_dM(rng, B, adj)
    Wg, alpha, _ = params(rng, C, T, 0)
    m = GraphAttention(C, T)
    with torch.no_grad():
        m.Wg.copy_(t(Wg))
        m.alpha.copy_(t(alpha))
    xt, at = t(x).requires_grad_(True), t(adj).requires_grad_(True)
    with capture(N) as seen:
        y = m(xt, at)
    ((y * t(dy)).sum() + (seen["M"] * t(dM.astype(np.float32))).sum()).backward()
    save(f"attw_gatt_b{B}c{C}n{N}.npz", adj=adj, Wg=Wg, alpha=alpha, dM=dM, y=y, att=seen["att"], M=seen["M"], dx=xt.grad,
         dWg=m.Wg.grad, dalpha=m.alpha.grad, dadj=at.grad, **stored)


def gacn_case(B, C, O, N, seed, int8_inputs=False, batched=False):
    T = 12
    rng = np.random.default_rng(seed)
    x, dy, stored = inputs(rng, B, C, O, N, int8_inputs)
    adj = learned_adjacency(N, seed + 1, B if batched else None)
    dM = structure_dM(rng, B, adj)
    Wg, alpha, W = params(rng, C, T, O)
    g = GACN(C, O, T)
    with torch.no_grad():
        g.gatt.Wg.copy_(t(Wg))
        g.gatt.alpha.copy_(t(alpha))
        g.W.copy_(t(W))
    xt, at = t(x).requires_grad_(True), t(adj).requires_grad_(True)
    with capture(N) as seen:
        y = g(xt, at)
    ((y * t(dy)).sum() + (seen["M"] * t(dM.astype(np.float32))).sum()).backward()
    save(f"attw_gacn_b{B}c{C}n{N}{'_bnn' if batched else ''}.npz", adj=adj, Wg=Wg, alpha=alpha, W=W, dM=dM, y=y,
         att=seen["att"], M=seen["M"], dx=xt.grad, dWg=g.gatt.Wg.grad, dalpha=g.gatt.alpha.grad, dW=g.W.grad,
         dadj=at.grad, **stored)


def meam_case(B, cin, cout, N, seed, dilations=(1, 2)):
    torch.manual_seed(seed)
    T = 12
    rng = np.random.default_rng(seed)
    m = MEAM(cin, cout, n_nodes=N, n_timesteps=T, dilations=list(dilations))
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim >= 2:
                torch.nn.init.xavier_normal_(p)
            else:
                torch.nn.init.uniform_(p, -p.size(0) ** -0.5, p.size(0) ** -0.5)
    adj = learned_adjacency(N, seed + 1)
    dM = structure_dM(rng, B, adj)
    at = t(adj).requires_grad_(True)
    x = torch.randn(B, cin, N, T).half().float().requires_grad_(True)
    dout = torch.randn(B, cout, N, T).half().float()
    with capture(N) as seen:
        out = m(x, at)
    ((out * dout).sum() + (seen["M"] * t(dM.astype(np.float32))).sum()).backward()
    arrays = {f"p.{k}": v for k, v in m.state_dict().items()}
    arrays.update({f"g.{k}": p.grad for k, p in m.named_parameters()})
    save(f"attw_meam_{cin}to{cout}_n{N}.npz", x=x.detach().half(), adj=adj, dout=dout.half(), dM=dM, out=out,
         att=seen["att"], M=seen["M"], dx=x.grad, dadj=at.grad, **arrays)


if __name__ == "__main__":
    gatt_case(2, 3, 64, seed=301)
    gacn_case(2, 3, 24, 64, seed=302)
    gacn_case(2, 72, 24, 47, seed=303, int8_inputs=True)
    gacn_case(3, 3, 24, 64, seed=304, batched=True)
    meam_case(2, 72, 72, 32, seed=305)
