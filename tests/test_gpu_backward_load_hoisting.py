"""GPU: the streaming kernels of the GACN backward at the smallest shapes where their load scheduling can go wrong.

`k_agg_sddmm` asks for everything of a slot's chain that does not depend on the dv slab ahead of its use: the first
two colptr pairs in front of the slab, the first slot's edge window and own u across the barrier, every later slot's
pair and own u one slot ahead -- all clamped and unconditional, and the slab's last element is stored once more by every
lane past its end.  The cases also pin the kernels around it at the sizes where their loops change shape:
`k_edge_grad_csc` / `_x` (trips of eight chunk partials and the tail loop), `k_bwd_rows` (trips of four edges) and
`k_aggfirst_bwd` (chunks of eight channels).  Every case runs through `StackedGACN` (R = 2, B = 2) on a graph with one column of
12 in-edges (the `> 8` loop of the fused pass' gather), one row of 9 out-edges (three trips of `k_bwd_rows`) and nodes
that have their self loop only (at N = 5 a column or a row holds 5 edges at most, and does), is compared with
oracle/gat_oracle.py in float64 under `conftest.assert_parity`, and must give the same bits on a second call.

The fused pass keeps as many channels per LDS slab as fit 64 KB, so its chunk count is cdiv(Co, channels per slab): one
or two chunks at N <= 257, and one chunk per channel only when N T > 8192.  The N = 700 cases are there for that: 9,
24 and 25 chunks, i.e. trips of eight with and without a tail in the edge pass.  At (16, 9, 257, 12) five channels
share a slab of 3855 float4, more than the four trips of 768 lanes that go through registers; N = 769 at T = 16 is
3076 slots, four more than the four slot iterations whose loads are asked for ahead (on a sparser graph: the slab and
the per-edge shares must leave room for two blocks per CU, or the fused pass is not chosen).
"""
import functools

import numpy as np
import pytest
import torch

import ms_gat_amd
from conftest import assert_parity
from oracle import gat_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R, B = 2, 2
WHAT = "backward_load_hoisting"


def _adjacency(N, seed):
    """Self loops everywhere; column 1 with min(N, 12) in-edges; row 2 with min(N, 9) out-edges; at N >= 64 a few more
    edges among the first N / 2 nodes.  The nodes of the upper half keep their self loop only."""
    rng = np.random.default_rng(seed)
    a = np.zeros((N, N), dtype=bool)
    a[np.arange(N), np.arange(N)] = True
    a[:min(N, 12), 1] = True
    a[2, :min(N, 9)] = True
    if N >= 64:
        extra = 2 * N if N <= 700 else N // 2
        a[rng.integers(0, N // 2, extra), rng.integers(0, N // 2, extra)] = True
        a[:, 1] = False
        a[:12, 1] = True
        a[2, :] = False
        a[2, :9] = True
    assert a[:, 1].sum() == min(N, 12) and a[2].sum() == min(N, 9) and a.sum() >= 8
    assert N < 64 or (a[N // 2:].sum(axis=1) == 1).all()
    return (a * rng.uniform(0.5, 1.5, (N, N))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problem(C, Co, N, T):
    rng = np.random.default_rng(1000 * C + 100 * Co + N + T)
    return dict(x=rng.standard_normal((R * B, C, N, T)).astype(np.float32),
                adj=_adjacency(N, N + T),
                Wg=(rng.standard_normal((R, T, T)) * (1.0 / T) ** 0.5).astype(np.float32),
                alpha=rng.uniform(-C ** -0.5, C ** -0.5, (R, C)).astype(np.float32),
                W=(rng.standard_normal((R, Co, C)) * (2.0 / (Co + C)) ** 0.5).astype(np.float32),
                dz=rng.standard_normal((R * B, Co, N, T)).astype(np.float32),
                dM=(rng.standard_normal((R * B, N, N))).astype(np.float32))


def _edge_term_backward(x, adj, Wg, alpha, dy, dM):
    """gat_oracle.gatt_backward with a second gradient dM [B,N,N] that arrives at E = P * adj itself: the same lines,
    dE + dM in the place of dE."""
    _, c = gat_oracle.gatt_forward(x, adj, Wg, alpha, return_cache=True)
    q, kW, P, E = c["q"], c["kW"], c["P"], c["E"]
    g = P * adj * (np.einsum("bcnt,bcmt->bnm", dy, x) + dM)
    dS = g - g.sum(axis=-1, keepdims=True) * P
    dkW = dS @ q
    dq = dS.transpose(0, 2, 1) @ kW + dkW @ Wg.T
    dx = np.einsum("bnm,bcnt->bcmt", E, dy) + alpha[None, :, None, None] * dq[:, None, :, :]
    return dx, np.einsum("bnt,bns->ts", q, dkW), np.einsum("bnt,bcnt->c", dq, x)


@functools.lru_cache(maxsize=None)
def _oracle(C, Co, N, T, edge_term=False):
    p = {k: np.asarray(v, dtype=np.float64) for k, v in _problem(C, Co, N, T).items()}
    out = dict(z=[], dx=[], dWg=[], dalpha=[], dW=[])
    for r in range(R):
        sl = slice(r * B, (r + 1) * B)
        x, Wg, alpha, W, dz = p["x"][sl], p["Wg"][r], p["alpha"][r], p["W"][r], p["dz"][sl]
        out["z"].append(gat_oracle.gacn_forward(x, p["adj"], Wg, alpha, W))
        dx, dWg, dalpha, dW = gat_oracle.gacn_backward(x, p["adj"], Wg, alpha, W, dz)
        if edge_term:
            dy = np.einsum("oc,bont->bcnt", W, dz)
            plain = _edge_term_backward(x, p["adj"], Wg, alpha, dy, np.zeros_like(p["dM"][sl]))
            for a, b in zip(plain, (dx, dWg, dalpha)):       # the copied lines are the oracle's
                assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
            dx, dWg, dalpha = _edge_term_backward(x, p["adj"], Wg, alpha, dy, p["dM"][sl] * (p["adj"] != 0))
        for k, v in zip(("dx", "dWg", "dalpha", "dW"), (dx, dWg, dalpha, dW)):
            out[k].append(v)
    return {k: (np.concatenate(v) if k in ("z", "dx") else np.stack(v)) for k, v in out.items()}


class _GradArrivesAsSlice(torch.autograd.Function):
    """Identity whose gradient reaches the producer as the channel slice [:, a:b] of a wider tensor."""

    @staticmethod
    def forward(ctx, z):
        return z.clone()

    @staticmethod
    def backward(ctx, g):
        G, Ck, N, T = g.shape
        wide = torch.full((G, 2 * Ck + 5, N, T), float("nan"), device=g.device)   # neighbours must never be read
        wide[:, 3:Ck + 3] = g
        return wide[:, 3:Ck + 3]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_once(C, Co, N, T, sliced, edge_term):
    p = _problem(C, Co, N, T)
    m = ms_gat_amd.StackedGACN(R, C, Co, T).to(DEV)
    with torch.no_grad():
        m.Wg.copy_(_dev(p["Wg"])), m.alpha.copy_(_dev(p["alpha"])), m.W.copy_(_dev(p["W"]))
    x = _dev(p["x"]).view(R, B, C, N, T).requires_grad_(True)
    adj, dz = _dev(p["adj"]), _dev(p["dz"]).view(R, B, Co, N, T)
    if edge_term:
        z, w = m(x, adj, need_weights=True)
        ((z * dz).sum() + (w.to_dense() * _dev(p["dM"]).view(R, B, N, N)).sum()).backward()
    else:
        z = m(x, adj)
        if sliced:
            z5 = _GradArrivesAsSlice.apply(z.view(R * B, Co, N, T)).view(R, B, Co, N, T)
            z5.backward(dz)
        else:
            z.backward(dz)
    torch.cuda.synchronize()
    return dict(z=z.detach().reshape(R * B, Co, N, T), dx=x.grad.reshape(R * B, C, N, T), dWg=m.Wg.grad,
                dalpha=m.alpha.grad, dW=m.W.grad)


def _check(C, Co, N, T, sliced=False, edge_term=False):
    got = _run_once(C, Co, N, T, sliced, edge_term)
    again = _run_once(C, Co, N, T, sliced, edge_term)
    want = _oracle(C, Co, N, T, edge_term)
    key = f"C{C}_Co{Co}_N{N}_T{T}" + ("_slice" if sliced else "") + ("_edge" if edge_term else "")
    for k in want:
        assert torch.equal(got[k], again[k]), f"{key}: {k} differs between two calls"
        assert_parity(got[k], want[k], WHAT, f"{key}:{k}")


# ---- PROJ_FIRST: k_agg_sddmm, k_edge_grad_csc, k_bwd_rows<T, 0> -----------------------------------------------------

PROJ_FIRST = [(8, 4, 5, 4),        # fewer slots than lanes; the edge pass' tail loop only
              (16, 9, 257, 12),    # 771 slots: a second slot iteration with 3 live lanes
              (72, 24, 64, 16),
              (72, 25, 70, 8),
              (16, 9, 700, 12),    # one channel per slab: 9 chunks = a trip of 8 + 1
              (26, 24, 700, 12),   # 24 chunks: three trips of 8
              (26, 25, 700, 12),   # 25 chunks: three trips of 8 + 1
              (12, 5, 769, 16)]    # 3076 slots: a fifth slot iteration with 4 live lanes


@pytest.mark.parametrize("C,Co,N,T", PROJ_FIRST)
def test_proj_first_backward(C, Co, N, T):
    _check(C, Co, N, T)


def test_proj_first_backward_reads_a_channel_slice_of_dz():
    _check(72, 24, 64, 16, sliced=True)


@pytest.mark.parametrize("C,Co,N,T", [(72, 24, 64, 16), (26, 25, 700, 12)])
def test_proj_first_backward_with_a_gradient_at_the_edge_weights(C, Co, N, T):
    """msgat_gacn_backward_edge_grad: the `_x` form of the edge pass"""
    _check(C, Co, N, T, edge_term=True)


# ---- AGG_FIRST: k_aggfirst_bwd, k_bwd_rows<T, C> ---------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(5, 4), (86, 12)])     # 5 float4 positions; 258: a second block with 2 live lanes
@pytest.mark.parametrize("Co", [4, 9, 24])              # below one chunk, not a multiple of 8, three chunks
@pytest.mark.parametrize("C", [1, 3])
def test_agg_first_backward(C, Co, N, T):
    _check(C, Co, N, T)


@pytest.mark.parametrize("Co", [9, 24])
def test_agg_first_backward_reads_a_channel_slice_of_dz(Co):
    _check(3, Co, 86, 12, sliced=True)
