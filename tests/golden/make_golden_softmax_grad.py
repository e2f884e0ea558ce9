#!/usr/bin/env python3
"""Generate the golden vectors of a loss on the dense attention map by running the REFERENCE.

Run where the reference's sources are importable (`MSGAT_REFERENCE_SRC`, default as in make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_softmax_grad.py

The reference's `att = softmax(k Wg q^T)` (attention.py:34) is an ordinary autograd tensor.  While its module runs on the
CPU, `torch.softmax` is wrapped to capture it (make_golden_attention.capture), and the loss is <dY, y> + <dP, att> with a
DENSE random dP [B,N,N]: the mass the attention puts off the road graph takes part.  Recorded: y, att and every gradient
(dx, dalpha, dWg, dW; W and the adjacency get nothing from the map).  Inputs and output gradients are fp16-exact (stored
as fp16) or int8 multiples of 1/32 (the 72-channel case).  Data only: nothing of the reference's source travels.

  attp_gatt_b2c3n64.npz     GraphAttention(C = 3), N = 64, B = 2
  attp_gacn_b2c72n47.npz    GACN(72 -> 24), N = 47, B = 2      (project first; N % 4 != 0)
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("MSGAT_REFERENCE_SRC", "/root/reference/src"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from models.attention import GraphAttention  # noqa: E402
from models.msgat import GACN  # noqa: E402

from make_golden_adjacency import learned_adjacency, params, t  # noqa: E402
from make_golden_attention import capture, inputs, save  # noqa: E402

torch.set_num_threads(4)


def dense_dP(rng, B, N):
    return rng.standard_normal((B, N, N)).astype(np.float16)


def gatt_case(B, C, N, seed):
    T = 12
    rng = np.random.default_rng(seed)
    x, dy, stored = inputs(rng, B, C, C, N, False)
    adj = learned_adjacency(N, seed + 1)
    dP = dense_dP(rng, B, N)
    Wg, alpha, _ = params(rng, C, T, 0)
    m = GraphAttention(C, T)
    with torch.no_grad():
        m.Wg.copy_(t(Wg))
        m.alpha.copy_(t(alpha))
    xt = t(x).requires_grad_(True)
    with capture(N) as seen:
        y = m(xt, t(adj))
    ((y * t(dy)).sum() + (seen["att"] * t(dP.astype(np.float32))).sum()).backward()
    save(f"attp_gatt_b{B}c{C}n{N}.npz", adj=adj, Wg=Wg, alpha=alpha, dP=dP, y=y, att=seen["att"], dx=xt.grad,
         dWg=m.Wg.grad, dalpha=m.alpha.grad, **stored)


def gacn_case(B, C, O, N, seed, int8_inputs=False):
    T = 12
    rng = np.random.default_rng(seed)
    x, dy, stored = inputs(rng, B, C, O, N, int8_inputs)
    adj = learned_adjacency(N, seed + 1)
    dP = dense_dP(rng, B, N)
    Wg, alpha, W = params(rng, C, T, O)
    g = GACN(C, O, T)
    with torch.no_grad():
        g.gatt.Wg.copy_(t(Wg))
        g.gatt.alpha.copy_(t(alpha))
        g.W.copy_(t(W))
    xt = t(x).requires_grad_(True)
    with capture(N) as seen:
        y = g(xt, t(adj))
    ((y * t(dy)).sum() + (seen["att"] * t(dP.astype(np.float32))).sum()).backward()
    save(f"attp_gacn_b{B}c{C}n{N}.npz", adj=adj, Wg=Wg, alpha=alpha, W=W, dP=dP, y=y, att=seen["att"], dx=xt.grad,
         dWg=g.gatt.Wg.grad, dalpha=g.gatt.alpha.grad, dW=g.W.grad, **stored)


if __name__ == "__main__":
    gatt_case(2, 3, 64, seed=311)
    gacn_case(2, 72, 24, 47, seed=313, int8_inputs=True)
