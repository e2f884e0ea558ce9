"""GPU: reading the graph attention (`need_weights`): the masked weights `att * adjacency` (sparse, differentiable) and
the dense softmax map `att` (msgat_attention_map), their gradients (msgat_*_backward_edge_grad, msgat_edge_softmax_grad)
against a float64 restatement of the reference (attention.py:32-36, msgat.py:25-28), every adjacency form, the outputs
left bit for bit as they were, and `MSGAT.attention_maps`.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden

import ms_gat_amd
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rng(seed):
    return np.random.default_rng(seed)


def _adjacency(N, seed, zero_row=True):
    a = ms_gat_amd.synthetic_adjacency(N, 3 * N, seed=seed).numpy().copy()
    r = _rng(seed + 7)
    a = a * r.uniform(0.5, 1.5, a.shape)           # asymmetric weights
    if zero_row:
        a[N // 3, :] = 0.0                          # a row without edges
    return a.astype(np.float32)


def _params(C, Co, T, seed, R=None):
    r = _rng(seed)
    lead = () if R is None else (R,)
    p = {"Wg": (r.standard_normal(lead + (T, T)) * 0.3).astype(np.float32),
         "alpha": r.uniform(-C ** -0.5, C ** -0.5, lead + (C,)).astype(np.float32)}
    if Co:
        p["W"] = (r.standard_normal(lead + (Co, C)) * 0.2).astype(np.float32)
    return p


def _ref(x, alpha, Wg, W, adj):
    """float64 reference: (y, att, att * adj) for one relation; adj [N,N] or [B,N,N]."""
    q = torch.einsum("c,bcnt->bnt", alpha, x)
    att = torch.softmax(torch.einsum("bnt,ts,bms->bnm", q, Wg, q), dim=-1)
    M = att * adj
    y = torch.einsum("bnm,bcmt->bcnt", M, x)
    if W is not None:
        y = torch.einsum("oc,bcnt->bont", W, y)
    return y, att, M


def _ref_grads(x, p, adj, dY, dM, adj_grad=True):
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in p.items()}
    xt = torch.from_numpy(x).double().requires_grad_(True)
    at = torch.from_numpy(adj).double().requires_grad_(adj_grad)
    y, att, M = _ref(xt, t["alpha"], t["Wg"], t.get("W"), at)
    ((y * torch.from_numpy(dY).double()).sum() + (M * torch.from_numpy(dM).double()).sum()).backward()
    out = {"y": y.detach().numpy(), "att": att.detach().numpy(), "M": M.detach().numpy(), "dx": xt.grad.numpy()}
    for k, v in t.items():
        out["d" + k] = v.grad.numpy()
    if adj_grad:
        out["dadj"] = at.grad.numpy()
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float32)


def _module(C, Co, T, p):
    m = ms_gat_amd.GACN(C, Co, T) if Co else ms_gat_amd.GraphAttention(C, T)
    prefix = "gatt." if Co else ""
    with torch.no_grad():
        for k, v in p.items():
            m.get_parameter(("" if k == "W" else prefix) + k).copy_(torch.from_numpy(v))
    return m.to(DEV)


def _grads(m, Co):
    g = {"dWg": (m.gatt.Wg if Co else m.Wg).grad, "dalpha": (m.gatt.alpha if Co else m.alpha).grad}
    if Co:
        g["dW"] = m.W.grad
    return g


def _structure_mask(adj):
    return (adj != 0) if adj.ndim == 2 else (adj != 0).any(axis=0)


# ---- masked weights: values and gradients against float64 autograd ------------------------------------------------

@pytest.mark.parametrize("C,Co,N,B,sell", [(3, 0, 64, 2, None), (1, 24, 64, 2, None), (3, 24, 64, 2, None),
                                            (72, 24, 47, 2, None), (8, 0, 64, 2, None), (8, 0, 64, 2, "always"),
                                            (72, 24, 64, 2, "always"), (8, 16, 64, 2, None)])
def test_masked_weights_and_gradients(C, Co, N, B, sell):
    """PLAIN, AGG_FIRST with the direct row form (C = 1, 3), PROJ_FIRST with the fused CSC form (C = 72, N % 4 != 0),
    and the SDDMM + k_edge_grad_x forms: PLAIN / AGG_FIRST with more than 4 channels (C = 8), and on a graph forced to
    SELL (`sell="always"`: CSR partials in SELL position order, PROJ_FIRST unfused).  A prebuilt SparseGraph gets no
    adjacency gradient."""
    T = 12
    r = _rng(N + C)
    p = _params(C, Co, T, seed=C + Co)
    adj = _adjacency(N, seed=N)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((B, Co or C, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * _structure_mask(adj)).astype(np.float32)
    want = _ref_grads(x, p, adj, dY, dM)

    m = _module(C, Co, T, p)
    xt = _dev(x).requires_grad_(True)
    at = _dev(adj).requires_grad_(True) if sell is None else ms_gat_amd.SparseGraph(torch.from_numpy(adj), sell=sell)
    y, w = m(xt, at, need_weights=True)
    assert w.is_sparse and w.is_coalesced() and tuple(w.shape) == (B, N, N)
    ((y * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    key = f"C{C}_Co{Co}_N{N}_{sell}"
    assert_parity(y, want["y"], "attention_weights", key + ":y")
    assert_parity(w.to_dense(), want["M"], "attention_weights", key + ":weights")
    assert_parity(xt.grad, want["dx"], "attention_weights", key + ":dx")
    for k, v in _grads(m, Co).items():
        assert_parity(v, want[k], "attention_weights", f"{key}:{k}")
    if sell is None:
        assert_parity(at.grad, want["dadj"], "attention_weights", key + ":dadj")
    # the indices are the graph's non-zeros in row-major order, per sample
    nz = np.argwhere(adj != 0)
    idx = w.indices().cpu().numpy()
    assert idx.shape[1] == B * len(nz)
    assert np.array_equal(idx[1:, : len(nz)].T, nz)


def test_weights_only_loss_reaches_inputs_and_adjacency():
    """Only the weights reach the loss: W gets no gradient term from them (E does not depend on W)."""
    C, Co, N, B, T = 3, 24, 64, 2, 12
    r = _rng(5)
    p = _params(C, Co, T, seed=5)
    adj = _adjacency(N, seed=3)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * _structure_mask(adj)).astype(np.float32)
    want = _ref_grads(x, p, adj, np.zeros((B, Co, N, T), np.float32), dM)
    m = _module(C, Co, T, p)
    xt, at = _dev(x).requires_grad_(True), _dev(adj).requires_grad_(True)
    _, w = m(xt, at, need_weights=True)
    (w.to_dense() * _dev(dM)).sum().backward()
    assert_parity(xt.grad, want["dx"], "attention_weights", "weights_only:dx")
    assert_parity(m.gatt.Wg.grad, want["dWg"], "attention_weights", "weights_only:dWg")
    assert_parity(m.gatt.alpha.grad, want["dalpha"], "attention_weights", "weights_only:dalpha")
    assert float(m.W.grad.abs().max()) == 0.0
    assert_parity(at.grad, want["dadj"], "attention_weights", "weights_only:dadj")


def test_batched_adjacency_weights_and_gradient():
    """Per-sample [B,N,N]: the union structure, explicit zeros where a sample has no edge, the gradient per sample."""
    C, Co, N, B, T = 3, 24, 64, 3, 12
    r = _rng(11)
    p = _params(C, Co, T, seed=11)
    adj = np.stack([_adjacency(N, seed=20 + b, zero_row=(b == 0)) for b in range(B)])
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((B, Co, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * _structure_mask(adj)).astype(np.float32)
    want = _ref_grads(x, p, adj, dY, dM)
    m = _module(C, Co, T, p)
    xt, at = _dev(x).requires_grad_(True), _dev(adj).requires_grad_(True)
    y, w = m(xt, at, need_weights=True)
    ((y * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    assert w.values().numel() == B * int(_structure_mask(adj).sum())
    assert (w.values() == 0).any()                 # a sample's own zero at a union edge
    assert_parity(w.to_dense(), want["M"], "attention_weights", "bnn:weights")
    assert_parity(xt.grad, want["dx"], "attention_weights", "bnn:dx")
    assert_parity(at.grad, want["dadj"], "attention_weights", "bnn:dadj")


def test_sparse_adjacency_explicit_zeros_unsorted():
    C, Co, N, B, T = 72, 24, 47, 2, 12
    r = _rng(13)
    p = _params(C, Co, T, seed=13)
    adj = _adjacency(N, seed=9)
    nz = np.argwhere(adj != 0)
    extra = np.array([[1, 2], [5, 40], [30, 3]])               # explicit zeros
    extra = extra[adj[extra[:, 0], extra[:, 1]] == 0]
    ij = np.concatenate([nz, extra])
    perm = r.permutation(len(ij))                              # unsorted
    ij = ij[perm]
    vals = adj[ij[:, 0], ij[:, 1]]
    dense_struct = np.zeros((N, N), bool)
    dense_struct[ij[:, 0], ij[:, 1]] = True
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((B, Co, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * dense_struct).astype(np.float32)
    want = _ref_grads(x, p, adj, dY, dM)
    v = _dev(vals).requires_grad_(True)
    sp = torch.sparse_coo_tensor(torch.from_numpy(ij.T.copy()).to(DEV), v, (N, N))
    m = _module(C, Co, T, p)
    xt = _dev(x).requires_grad_(True)
    y, w = m(xt, sp, need_weights=True)
    ((y * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    assert w.values().numel() == B * len(ij)
    assert np.array_equal(w.indices()[1:, : len(ij)].cpu().numpy().T, np.argwhere(dense_struct))
    assert_parity(w.to_dense(), want["M"], "attention_weights", "sparse:weights")
    assert_parity(xt.grad, want["dx"], "attention_weights", "sparse:dx")
    dval = want["dadj"][ij[:, 0], ij[:, 1]]
    assert_parity(v.grad, dval, "attention_weights", "sparse:dvalues")


def test_edge_adjacency_weight_gradient():
    """Learned sparse edge weights (`ops.edge_adjacency`): the weights' gradient reaches `weight` [nnz]."""
    C, Co, N, B, T = 3, 24, 64, 2, 12
    r = _rng(17)
    p = _params(C, Co, T, seed=17)
    adj = _adjacency(N, seed=4)
    csr = torch.from_numpy(adj).to_sparse_csr()
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((B, Co, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * (adj != 0)).astype(np.float32)
    want = _ref_grads(x, p, adj, dY, dM)
    weight = csr.values().to(DEV).clone().requires_grad_(True)
    sp = ops.edge_adjacency(csr.crow_indices().to(DEV), csr.col_indices().to(DEV), weight)
    m = _module(C, Co, T, p)
    y, w = m(_dev(x), sp, need_weights=True)
    ((y * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    nz = np.argwhere(adj != 0)
    assert_parity(weight.grad, want["dadj"][nz[:, 0], nz[:, 1]], "attention_weights", "edge_adjacency:dweight")


def test_stacked_gacn_weights_r3():
    R, C, Co, N, B, T = 3, 72, 24, 64, 2, 12
    r = _rng(19)
    p = _params(C, Co, T, seed=19, R=R)
    adj = _adjacency(N, seed=6)
    x = r.standard_normal((R, B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((R, B, Co, N, T)).astype(np.float32)
    dM = (r.standard_normal((R, B, N, N)) * (adj != 0)).astype(np.float32)
    m = ms_gat_amd.StackedGACN(R, C, Co, T)
    with torch.no_grad():
        for k, v in p.items():
            m.get_parameter(k).copy_(torch.from_numpy(v))
    m = m.to(DEV)
    xt, at = _dev(x).requires_grad_(True), _dev(adj).requires_grad_(True)
    y, w = m(xt, at, need_weights=True)
    assert tuple(w.shape) == (R, B, N, N)
    ((y * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    dadj = 0
    for rel in range(R):
        want = _ref_grads(x[rel], {k: v[rel] for k, v in p.items()}, adj, dY[rel], dM[rel])
        assert_parity(w.to_dense()[rel], want["M"], "attention_weights", f"stacked:r{rel}:weights")
        assert_parity(xt.grad[rel], want["dx"], "attention_weights", f"stacked:r{rel}:dx")
        assert_parity(m.Wg.grad[rel], want["dWg"], "attention_weights", f"stacked:r{rel}:dWg")
        assert_parity(m.alpha.grad[rel], want["dalpha"], "attention_weights", f"stacked:r{rel}:dalpha")
        dadj = dadj + want["dadj"]
    assert_parity(at.grad, dadj, "attention_weights", "stacked:dadj")


def test_attention_core_weights_and_gradient():
    """The attention core (MEAM's merged branch): z = (att * adj) u with q given."""
    Cu, N, B, T = 24, 32, 2, 12
    r = _rng(23)
    adj = _adjacency(N, seed=8)
    u = r.standard_normal((B, Cu, N, T)).astype(np.float32)
    q = r.standard_normal((B, N, T)).astype(np.float32)
    Wg = (r.standard_normal((1, T, T)) * 0.3).astype(np.float32)
    dY = r.standard_normal((B, Cu, N, T)).astype(np.float32)
    dM = (r.standard_normal((B, N, N)) * (adj != 0)).astype(np.float32)
    ud, qd, wd, ad = (torch.from_numpy(a).double().requires_grad_(True) for a in (u, q, Wg, adj))
    att = torch.softmax(torch.einsum("bnt,ts,bms->bnm", qd, wd[0], qd), dim=-1)
    M = att * ad
    z = torch.einsum("bnm,bcmt->bcnt", M, ud)
    ((z * torch.from_numpy(dY).double()).sum() + (M * torch.from_numpy(dM).double()).sum()).backward()
    ut, qt, wt, at = (_dev(a).requires_grad_(True) for a in (u, q, Wg, adj))
    zz, w = ops.attention_core(ut, qt, wt, at, need_weights=True)
    ((zz * _dev(dY)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
    assert_parity(w.to_dense(), M.detach().numpy(), "attention_weights", "core:weights")
    for got, want, k in ((ut.grad, ud.grad, "du"), (qt.grad, qd.grad, "dq"), (wt.grad, wd.grad, "dWg"), (at.grad, ad.grad, "dadj")):
        assert_parity(got, want.numpy(), "attention_weights", "core:" + k)
    with torch.no_grad():
        _, P = ops.attention_core(ut, qt, wt, at, need_weights=True, weights="softmax")
    assert_parity(P, att.detach().numpy(), "attention_weights", "core:softmax")


# ---- the dense softmax map ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,B,C", [(64, 2, 3), (307, 2, 3), (883, 2, 72), (1600, 2, 3), (1600, 32, 1)])
def test_softmax_map_against_float64(N, B, C):
    """Below and above the split-operand threshold (N = 1536); B = 32, C = 1 at N = 1600 for a large batch."""
    T = 12
    r = _rng(N + B)
    p = _params(C, 0, T, seed=N)
    adj = _adjacency(N, seed=N, zero_row=False)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    m = _module(C, 0, T, p)
    with torch.no_grad():
        _, P = m(_dev(x), _dev(adj), need_weights=True, weights="softmax")
    assert P.dtype == torch.float32 and tuple(P.shape) == (B, N, N) and not P.is_sparse
    xd = torch.from_numpy(x).double()
    for b in range(0, B, max(1, B // 4)):
        q = torch.einsum("c,cnt->nt", torch.from_numpy(p["alpha"]).double(), xd[b])
        Pref = torch.softmax(q @ torch.from_numpy(p["Wg"]).double() @ q.T, dim=-1).numpy()
        got = P[b].double().cpu().numpy()
        assert np.abs(got - Pref).max() <= 1e-5, (N, b, np.abs(got - Pref).max())
        assert np.abs(got.sum(axis=1) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("form", ["dense", "batched", "sparse", "sell"])
def test_masked_equals_softmax_times_adjacency(form):
    C, Co, N, B, T = 3, 24, 80, 2, 12
    r = _rng(29)
    p = _params(C, Co, T, seed=29)
    adj = _adjacency(N, seed=12)
    x = _dev(r.standard_normal((B, C, N, T)).astype(np.float32))
    if form == "dense":
        a, dense = _dev(adj), adj[None]
    elif form == "batched":
        bn = np.stack([adj, _adjacency(N, seed=13)])
        a, dense = _dev(bn), bn
    elif form == "sparse":
        a, dense = _dev(adj).to_sparse(), adj[None]
    else:
        a, dense = ms_gat_amd.SparseGraph(torch.from_numpy(adj), sell="always"), adj[None]
    m = _module(C, Co, T, p)
    with torch.no_grad():
        z0 = m(x, a)
        z1, w = m(x, a, need_weights=True)
        z2, P = m(x, a, need_weights=True, weights="softmax")
    assert torch.equal(z0, z1) and torch.equal(z0, z2)
    idx = w.indices()
    Pd = P.cpu().numpy()
    want = Pd[idx[0].cpu(), idx[1].cpu(), idx[2].cpu()] * torch.from_numpy(dense)[
        (idx[0].cpu() % dense.shape[0]), idx[1].cpu(), idx[2].cpu()].numpy()
    got = w.values().cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max())


# ---- bits ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,Co", [(3, 24), (72, 24), (3, 0)])
def test_unused_weights_leave_every_bit(C, Co):
    """Weights asked for but not differentiated: output and every gradient bit for bit the plain call's."""
    N, B, T = 64, 2, 12
    r = _rng(31)
    p = _params(C, Co, T, seed=31)
    adj = _adjacency(N, seed=14)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = _dev(r.standard_normal((B, Co or C, N, T)).astype(np.float32))
    outs = []
    for need in (False, True):
        m = _module(C, Co, T, p)
        xt, at = _dev(x).requires_grad_(True), _dev(adj).requires_grad_(True)
        res = m(xt, at, need_weights=need)
        y = res[0] if need else res
        (y * dY).sum().backward()
        outs.append([y.detach(), xt.grad, at.grad] + list(_grads(m, Co).values()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_readouts_are_deterministic():
    C, Co, N, B, T = 72, 24, 64, 2, 12
    r = _rng(37)
    p = _params(C, Co, T, seed=37)
    adj = _adjacency(N, seed=15)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = _dev(r.standard_normal((B, Co, N, T)).astype(np.float32))
    dM = _dev((r.standard_normal((B, N, N)) * (adj != 0)).astype(np.float32))
    runs = []
    for _ in range(2):
        m = _module(C, Co, T, p)
        xt, at = _dev(x).requires_grad_(True), _dev(adj).requires_grad_(True)
        y, w = m(xt, at, need_weights=True)
        ((y * dY).sum() + (w.to_dense() * dM).sum()).backward()
        with torch.no_grad():
            _, P = m(xt, at, need_weights=True, weights="softmax")
        runs.append([w.values().detach(), P, xt.grad, at.grad, m.gatt.Wg.grad])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_softmax_weights_refused_under_grad():
    m = _module(3, 24, 12, _params(3, 24, 12, seed=1))
    x = torch.randn(2, 3, 16, 12, device=DEV)
    adj = _dev(_adjacency(16, seed=1))
    with pytest.raises(ValueError, match="masked"):
        m(x, adj, need_weights=True, weights="softmax")


# ---- the model-level readout ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("weights", ["masked", "softmax"])
def test_msgat_attention_maps(learn, weights):
    N, B, R, T = 32, 2, 3, 12
    adj = torch.from_numpy(_adjacency(N, seed=21, zero_row=False))
    torch.manual_seed(0)
    model = ms_gat_amd.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj,
                               learn_edge_weights=learn).to(DEV)
    X = torch.randn(B, R, 1, N, T, device=DEV)
    H = torch.randint(0, 24, (B,), device=DEV)
    D = torch.randint(0, 7, (B,), device=DEV)
    model.stack_components = True
    a = model.attention_maps(X, H, D, weights=weights)
    model.stack_components = False
    b = model.attention_maps(X, H, D, weights=weights)
    keys = [f"tpcs.{r}.tgacns.{l}.gacn" for r in range(R) for l in range(2)]
    assert sorted(a) == sorted(keys) and sorted(b) == sorted(keys)
    for k in keys:
        assert all(isinstance(model.get_submodule(k), ms_gat_amd.GACN) for k in keys)
        wa = a[k].to_dense() if a[k].is_sparse else a[k]
        wb = b[k].to_dense() if b[k].is_sparse else b[k]
        assert tuple(wa.shape) == (B, N, N)
        assert torch.equal(wa, wb), k
        if weights == "softmax":
            assert float((wa.sum(-1) - 1).abs().max()) < 1e-5
    # the first block's GACN of component 0 called directly on its input gives the same map
    with torch.no_grad():
        tpc = model.tpcs[0]
        blk = tpc.tgacns[0]
        normed = blk.ln(X[:, 0])
        _, w0 = blk.gacn(normed, model.adjacency(), need_weights=True, weights=weights)
    w0 = w0.to_dense() if w0.is_sparse else w0
    wa = a["tpcs.0.tgacns.0.gacn"]
    wa = wa.to_dense() if wa.is_sparse else wa
    assert torch.allclose(w0, wa, rtol=1e-5, atol=1e-6)


def test_merged_branch_map_against_float64():
    """A level-1 block takes the merged-branch attention core: its map against float64 from that block's own input."""
    N, B, R, T = 32, 2, 3, 12
    adj = torch.from_numpy(_adjacency(N, seed=22, zero_row=False))
    torch.manual_seed(1)
    model = ms_gat_amd.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=T, use_te=True,
                               adj=adj).to(DEV)
    X = torch.randn(B, R, 1, N, T, device=DEV)
    H = torch.randint(0, 24, (B,), device=DEV)
    D = torch.randint(0, 7, (B,), device=DEV)
    model.stack_components = False
    blk = model.tpcs[1].tgacns[1]
    assert blk.in_channels > blk.out_channels // 3 and blk.dilations          # the merged branches
    seen = {}
    hook = blk.register_forward_pre_hook(lambda mod, args: seen.__setitem__("x", args[0].detach().clone()))
    try:
        soft = model.attention_maps(X, H, D, weights="softmax")
        masked = model.attention_maps(X, H, D, weights="masked")
    finally:
        hook.remove()
    x = seen["x"].double()
    normed = torch.nn.functional.layer_norm(x, [T], blk.ln.weight.double(), blk.ln.bias.double(), blk.ln.eps)
    q = torch.einsum("c,bcnt->bnt", blk.gacn.gatt.alpha.double(), normed)
    att = torch.softmax(q @ blk.gacn.gatt.Wg.double() @ q.transpose(1, 2), dim=-1)
    key = "tpcs.1.tgacns.1.gacn"
    assert float((soft[key].double() - att).abs().max()) <= 1e-5
    want = (att * adj.to(DEV).double())
    assert float((masked[key].to_dense().double() - want).abs().max()) <= 1e-5


# ---- the reference's own fixtures (tests/golden/make_golden_attention.py) --------------------------------------------

def _fixture_inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g["dy_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g["dy"].astype(np.float32)


@pytest.mark.parametrize("name", ["attw_gatt_b2c3n64.npz", "attw_gacn_b2c3n64.npz", "attw_gacn_b2c72n47.npz",
                                  "attw_gacn_b3c3n64_bnn.npz"])
def test_weights_match_reference_fixture(name):
    g = load_golden(name)
    x, dy = _fixture_inputs(g)
    C, Co = x.shape[1], (g["W"].shape[0] if "W" in g else 0)
    p = {k: g[k] for k in ("Wg", "alpha", "W") if k in g}
    m = _module(C, Co, 12, p)
    xt, at = _dev(x).requires_grad_(True), _dev(g["adj"]).requires_grad_(True)
    y, w = m(xt, at, need_weights=True)
    ((y * _dev(dy)).sum() + (w.to_dense() * _dev(g["dM"].astype(np.float32))).sum()).backward()
    assert_parity(y, g["y"], name, "y")
    assert_parity(w.to_dense(), g["M"], name, "masked")
    for k, v in _grads(m, Co).items():
        assert_parity(v, g[k], name, k)
    assert_parity(xt.grad, g["dx"], name, "dx")
    assert_parity(at.grad, g["dadj"], name, "dadj")
    with torch.no_grad():       # (an inference forward skips what only backward needs: compare it with its own kind)
        y0 = m(_dev(x), _dev(g["adj"]))
        y2, P = m(_dev(x), _dev(g["adj"]), need_weights=True, weights="softmax")
    assert_parity(P, g["att"], name, "softmax")
    assert torch.equal(y2, y0)


def test_meam_weights_match_reference_fixture():
    """MEAM(72 -> 72): the merged branches' attention core, its weights collected (differentiable) while the block runs."""
    name = "attw_meam_72to72_n32.npz"
    g = load_golden(name)
    m = ms_gat_amd.MEAM(72, 72, n_nodes=32, n_timesteps=12, dilations=[1, 2])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")})
    m = m.to(DEV)
    x = _dev(g["x"].astype(np.float32)).requires_grad_(True)
    adj = _dev(g["adj"]).requires_grad_(True)
    with ops.collect_weights("masked") as seen:
        out = m(x, adj)
    assert len(seen) == 1
    w = ops.weights_of(seen[0], "masked", (2,))
    ((out * _dev(g["dout"].astype(np.float32))).sum() + (w.to_dense() * _dev(g["dM"].astype(np.float32))).sum()).backward()
    assert_parity(out, g["out"], name, "out")
    assert_parity(w.to_dense(), g["M"], name, "masked")
    assert_parity(x.grad, g["dx"], name, "dx")
    assert_parity(adj.grad, g["dadj"], name, "dadj")
    for k, prm in m.named_parameters():
        assert_parity(prm.grad, g[f"g.{k}"], name, k)
    with torch.no_grad(), ops.collect_weights("softmax") as seen:
        m(x, adj)
    assert_parity(ops.weights_of(seen[0], "softmax", (2,)), g["att"], name, "softmax")
