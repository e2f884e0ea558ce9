"""What the group-count tests (test_gpu_group_counts.py, test_group_splits_cpu.py) share: the tables of shapes with the
split each one must take, seeded inputs of the kernels that re-create the softmax map, and their float64 restatements.

Every kernel here re-creates P = 2^(S log2 e - lse) from q, kW [G,N,T] and the fp32 lse [G,N] it is GIVEN (include/
msgat_hip.h); the restatements do the same in float64 with those fp32 lse values, so that what is compared is the
kernel's own arithmetic and group bookkeeping, not the rounding of lse."""
import math

import torch

LOG2E = 1.0 / math.log(2.0)

# msgat_adjacency_grad: (N, V, G, Cu, nsplit, per, what it exercises).  Split counts follow csrc/adjacency_grad.hip with
# kAgTile = 64, kAgTargetBlocks = 1024, kAgMaxSplit = 16; a case asserts its count from the workspace size, so a later
# change of the constants cannot quietly move it off its branch.
ADJACENCY_GRAD_CASES = [
    (64, 1, 35, 3, 12, 3, "last split has 2 groups; one staged step per group"),
    (64, 1, 16, 5, 16, 1, "the split cap"),
    (64, 1, 17, 5, 9, 2, "last split has 1 group"),
    (64, 2, 36, 6, 9, 2, "two value sets interleave, g % 2"),
    (70, 1, 20, 6, 10, 2, "four tiles with clamped rows; dead channels in the last staged step"),
    (512, 16, 48, 3, 1, 3, "no split: straight write to the output, no workspace"),
]

# msgat_edge_weight_grad on SparseGraph(synthetic_adjacency(N, E, seed)), nnz = N + 2 E:
# (N, E, G, Cu, nsplit, per, what it exercises); kEwEdges = 64, kEwTargetBlocks = 4096, kEwMaxSplit = 48
EDGE_WEIGHT_GRAD_CASES = [
    (64, 70, 16, 3, 16, 1, "the one-lane-per-column reduction at its limit of 16 partials"),
    (64, 70, 17, 3, 17, 1, "first split count past it"),
    (64, 70, 48, 3, 48, 1, "the split cap"),
    (64, 70, 96, 3, 48, 2, "the training step's split"),
    (64, 70, 100, 3, 34, 3, "last split has 1 group"),
    (20, 15, 5, 3, 5, 1, "nnz = 50 < 64: the wave-per-partial reduction with few partials"),
    (4096, 129100, 3, 2, 1, 3, "4099 edge tiles: no split, straight write"),
]


def nnz_of(N, E):
    return N + 2 * E


def draw(G, Cu, N, T, seed, device="cpu"):
    """Seeded O(1) normals q, kW [G,N,T], dv, feat [G,Cu,N,T] and lse [G,N]: log2 sum_m exp(S) in float64, S = kW q^T,
    rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    q, kW = torch.randn(G, N, T, generator=g), torch.randn(G, N, T, generator=g)
    dv, feat = torch.randn(G, Cu, N, T, generator=g), torch.randn(G, Cu, N, T, generator=g)
    q, kW, dv, feat = (t.to(device) for t in (q, kW, dv, feat))
    lse = torch.empty(G, N, device=device)
    for k in range(G):   # one [N,N] at a time: 134 MB in float64 at N = 4096
        S = kW[k].double() @ q[k].double().T
        lse[k] = (torch.logsumexp(S, dim=-1) * LOG2E).float()
    return q, kW, lse, dv, feat


def softmax_map(q, kW, lse):
    """P [G,N,N] in float64 from the fp32 lse that is passed in"""
    S = torch.einsum("gnt,gmt->gnm", kW.double(), q.double())
    return torch.exp2(S * LOG2E - lse.double()[..., None])


def dense_adjacency_grad(q, kW, lse, dv, feat, V):
    """dadj[v] = sum_{g % V == v} P_g (.) H_g,  H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t];  [V,N,N] float64"""
    G, N = lse.shape
    out = torch.zeros(V, N, N, dtype=torch.float64, device=q.device)
    for g in range(G):
        P = softmax_map(q[g:g + 1], kW[g:g + 1], lse[g:g + 1])[0]
        out[g % V] += P * torch.einsum("cnt,cmt->nm", dv[g].double(), feat[g].double())
    return out


def edge_adjacency_grad(q, kW, lse, dv, feat, V, rows, cols, dE_extra=None):
    """The same at the edges (rows[e], cols[e]) only, plus P dE_extra where given: [V,nnz] float64.  Nothing [N,N]."""
    G = lse.shape[0]
    out = torch.zeros(V, rows.numel(), dtype=torch.float64, device=q.device)
    for g in range(G):
        P = edge_softmax(q, kW, lse, g, rows, cols)
        H = (dv[g].double()[:, rows] * feat[g].double()[:, cols]).sum(dim=(0, 2))
        out[g % V] += P * (H if dE_extra is None else H + dE_extra[g].double())
    return out


def edge_softmax(q, kW, lse, g, rows, cols):
    S = (kW[g].double()[rows] * q[g].double()[cols]).sum(-1)
    return torch.exp2(S * LOG2E - lse[g].double()[rows])


def softmax_map_grad(q, kW, lse, Wg, dP, Bg):
    """(dq [G,N,T], dWg [R,T,T]) in float64 of a gradient dP at the map: r = sum_m P dP, dS = P (.) (dP - r), dkW = dS q,
    dq = dS^T kW + dkW Wg^T, dWg[rel] = sum_{g in rel} q^T dkW (msgat_softmax_map_grad)."""
    G, N, T = q.shape
    P = softmax_map(q, kW, lse)
    X = P * dP.double()
    dS = X - X.sum(-1, keepdim=True) * P
    dkW = dS @ q.double()
    Wgg = Wg.double().repeat_interleave(Bg, dim=0)
    dq = dS.transpose(1, 2) @ kW.double() + dkW @ Wgg.transpose(1, 2)
    dWg = torch.einsum("gnt,gns->gts", q.double(), dkW).view(G // Bg, Bg, T, T).sum(1)
    return dq, dWg
