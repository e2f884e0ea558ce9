"""GPU: a sparse adjacency (torch COO / CSR) with a gradient at its stored edges (msgat_edge_weight_grad).

Parity with the reference's fixtures (graph attention, both GACN modes, the attention core via MEAM) with the adjacency
passed sparse, its pattern widened by explicit zeros; float64 autograd of the dense restatement, SELL-sized graphs and
every T included; bit-identity with the dense path; determinism; a HIP-graph capture that re-reads the weights; and
MSGAT(learn_edge_weights=True) under the Trainer, captured and eager.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden, rel_err
from oracle import dense_torch

import ms_gat_amd
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _load_module(m, state):
    with torch.no_grad():
        for k, v in state.items():
            m.get_parameter(k).copy_(_dev(v))
    return m.to(DEV)


def _pattern(adj, seed, extra=7):
    """(rows, cols) of the non-zeros of `adj` plus `extra` explicit-zero positions, row-major sorted."""
    rng = np.random.default_rng(seed)
    mask = adj != 0
    zeros = np.argwhere(~mask)
    for i, j in zeros[rng.choice(len(zeros), size=min(extra, len(zeros)), replace=False)]:
        mask[i, j] = True
    r, c = np.nonzero(mask)
    return r, c


def _sparse(adj, layout, seed=0):
    """(sparse adjacency on the device, its leaf values, rows, cols)"""
    n = adj.shape[0]
    r, c = _pattern(adj, seed)
    vals = torch.nn.Parameter(_dev(adj[r, c]))
    if layout == "coo":
        a = torch.sparse_coo_tensor(_dev(np.stack([r, c]), torch.int64), vals, (n, n), is_coalesced=True)
    else:
        crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
        a = torch.sparse_csr_tensor(_dev(crow, torch.int64), _dev(c, torch.int64), vals, (n, n))
    return a, vals, r, c


def _inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g["dz_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g["dz"].astype(np.float32)


# ---- the reference's fixtures -------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_graph_attention_matches_reference_fixture(layout):
    g = load_golden("adjgrad_gatt_b2c3n64.npz")
    m = _load_module(ms_gat_amd.GraphAttention(3, 12), {"Wg": g["Wg"], "alpha": g["alpha"]})
    x = _dev(g["x"]).requires_grad_(True)
    adj, vals, r, c = _sparse(g["adj"], layout)
    y = m(x, adj)
    y.backward(_dev(g["dy"]))
    for got, key in ((y, "y"), (x.grad, "dx"), (m.Wg.grad, "dWg"), (m.alpha.grad, "dalpha")):
        assert_parity(got, g[key], "adjgrad_gatt_b2c3n64 " + layout, key)
    assert_parity(vals.grad, g["dadj"][r, c], "adjgrad_gatt_b2c3n64 " + layout, "dval")


@pytest.mark.parametrize("layout", ["coo", "csr"])
@pytest.mark.parametrize("name", ["adjgrad_gacn_b2c3n64.npz", "adjgrad_gacn_b2c72n47.npz"])
def test_gacn_matches_reference_fixture(name, layout):
    g = load_golden(name)
    xn, dzn = _inputs(g)
    C, O = xn.shape[1], g["W"].shape[0]
    m = _load_module(ms_gat_amd.GACN(C, O, 12), {"gatt.Wg": g["Wg"], "gatt.alpha": g["alpha"], "W": g["W"]})
    x = _dev(xn).requires_grad_(True)
    adj, vals, r, c = _sparse(g["adj"], layout, seed=1)
    z = m(x, adj)
    z.backward(_dev(dzn))
    for got, key in ((z, "z"), (x.grad, "dx"), (m.gatt.Wg.grad, "dWg"), (m.gatt.alpha.grad, "dalpha"), (m.W.grad, "dW")):
        assert_parity(got, g[key], name + " " + layout, key)
    assert_parity(vals.grad, g["dadj"][r, c], name + " " + layout, "dval")


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_meam_matches_reference_fixture(layout):
    g = load_golden("adjgrad_meam_72to72_n32.npz")
    m = ms_gat_amd.MEAM(72, 72, n_nodes=32, n_timesteps=12, dilations=[1, 2])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")})
    m = m.to(DEV)
    x = _dev(g["x"].astype(np.float32)).requires_grad_(True)
    adj, vals, r, c = _sparse(g["adj"], layout, seed=2)
    out = m(x, adj)
    out.backward(_dev(g["dout"].astype(np.float32)))
    what = "adjgrad_meam_72to72_n32 " + layout
    assert_parity(out, g["out"], what, "out")
    assert_parity(x.grad, g["dx"], what, "dx")
    assert_parity(vals.grad, g["dadj"][r, c], what, "dval")
    for k, p in m.named_parameters():
        assert_parity(p.grad, g[f"g.{k}"], what, k)


# ---- float64 autograd of the dense restatement --------------------------------------------------------------------

def _case(B, C, O, N, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, N, T)).astype(np.float32)
    dz = rng.standard_normal((B, O or C, N, T)).astype(np.float32)
    Wg = (rng.standard_normal((T, T)) * (1.0 / T) ** 0.5).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, C).astype(np.float32)
    W = (rng.standard_normal((O, C)) * (2.0 / (O + C)) ** 0.5).astype(np.float32) if O else None
    adj = ms_gat_amd.synthetic_adjacency(N, N + 6, seed).numpy() * rng.uniform(0.25, 1.5, (N, N)).astype(np.float32)
    return x, dz, Wg, alpha, W, adj


def _oracle(x, dz, Wg, alpha, W, adj):
    a = torch.from_numpy(adj).to(DEV, torch.float64).requires_grad_(True)
    f = lambda t: torch.from_numpy(t).to(DEV, torch.float64)  # noqa: E731
    z = dense_torch.graph_attention_dense(f(x), a, f(Wg), f(alpha)) if W is None else \
        dense_torch.gacn_dense(f(x), a, f(Wg), f(alpha), f(W))
    z.backward(f(dz))
    return z, a.grad


@pytest.mark.parametrize("B,C,O,N,T", [(2, 72, 24, 307, 12), (2, 3, 24, 97, 12), (2, 5, 0, 64, 4), (2, 5, 0, 64, 8),
                                       (1, 2, 0, 2048, 4), (1, 2, 0, 2048, 8), (1, 2, 0, 2048, 12), (1, 2, 3, 2048, 16),
                                       (1, 2, 0, 4096, 12)])
def test_matches_float64_autograd(B, C, O, N, T):
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=N + T)
    zo, dao = _oracle(x, dz, Wg, alpha, W, adj)
    r, c = _pattern(adj, seed=3)
    vals = torch.nn.Parameter(_dev(adj[r, c]))
    crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])
    a = torch.sparse_csr_tensor(_dev(crow, torch.int64), _dev(c, torch.int64), vals, (N, N))
    xt = _dev(x).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), None if W is None else _dev(W), a)
    z.backward(_dev(dz))
    # from N = 2048 the structure carries the SELL layouts (at N = 4096, T = 12 an [N,T] slab no longer fits LDS and
    # the SELL kernels run)
    assert ms_gat_amd.graph.sparse_pattern_of(a.detach()).structure.has_sell == (N >= 2048)
    what = f"sparse b{B}c{C}o{O}n{N}t{T}"
    assert_parity(z, zo.detach().cpu().numpy(), what, "z")
    assert_parity(vals.grad, dao.cpu().numpy()[r, c], what, "dval")


# ---- the same bits as the dense path; determinism ------------------------------------------------------------------

@pytest.mark.parametrize("O", [0, 24, 3])
def test_sparse_path_is_bit_identical_to_dense_path(O):
    B, C, N, T = 2, 72 if O == 24 else 3, 307, 12
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=5)
    res = []
    for sparse in (False, True):
        xt = _dev(x).requires_grad_(True)
        ps = [_dev(alpha).requires_grad_(True), _dev(Wg).requires_grad_(True)]
        Wt = None if W is None else _dev(W).requires_grad_(True)
        if sparse:
            r, c = np.nonzero(adj)
            vals = torch.nn.Parameter(_dev(adj[r, c]))
            idx = _dev(np.stack([r, c]), torch.int64)
            a = torch.sparse_coo_tensor(idx, vals, (N, N), is_coalesced=True)
        else:
            a = _dev(adj)
        z = ops.gacn(xt, ps[0], ps[1], Wt, a)
        z.backward(_dev(dz))
        res.append([z, xt.grad, ps[0].grad, ps[1].grad] + ([Wt.grad] if Wt is not None else []))
        if sparse:
            dval1 = vals.grad.clone()
            vals.grad = None
            a = torch.sparse_coo_tensor(idx, vals, (N, N), is_coalesced=True)
            ops.gacn(_dev(x), _dev(alpha), _dev(Wg), None if W is None else _dev(W), a).backward(_dev(dz))
            assert torch.equal(vals.grad, dval1)          # deterministic
    for d, s in zip(*res):
        assert torch.equal(d, s)


# ---- HIP-graph capture ---------------------------------------------------------------------------------------------

def test_hip_graph_capture_rereads_the_weights():
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=9)
    m = _load_module(ms_gat_amd.GACN(C, O, T), {"gatt.Wg": Wg, "gatt.alpha": alpha, "W": W})
    r, c = np.nonzero(adj)
    crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])
    crow_t, col_t = _dev(crow, torch.int64), _dev(c, torch.int64)
    w = torch.nn.Parameter(_dev(adj[r, c]))
    xs, dzs = _dev(x), _dev(dz)
    out = torch.empty((B, O, N, T), device=DEV)

    def step():
        m.zero_grad(set_to_none=False)
        w.grad.zero_()
        z = m(xs, ops.edge_adjacency(crow_t, col_t, w))
        out.copy_(z.detach())
        z.backward(dzs)

    m(xs, ops.edge_adjacency(crow_t, col_t, w)).backward(dzs)     # warm-up: the structure is built, the grads exist
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    rng = np.random.default_rng(4)
    for _ in range(2):
        with torch.no_grad():
            w.mul_(_dev(rng.uniform(0.5, 1.5, w.numel())))
        graph.replay()
        torch.cuda.synchronize()
        replayed_z, replayed_dw, replayed_dx = out.clone(), w.grad.clone(), m.W.grad.clone()
        w.grad.zero_()
        m.zero_grad(set_to_none=False)
        z = m(xs, ops.edge_adjacency(crow_t, col_t, w))
        z.backward(dzs)
        assert torch.equal(replayed_z, z.detach())
        assert torch.equal(replayed_dw, w.grad)
        assert torch.equal(replayed_dx, m.W.grad)


def test_first_sight_of_a_pattern_inside_a_capture_raises():
    N = 40
    adj = ms_gat_amd.synthetic_adjacency(N, 50, seed=77).numpy()
    r, c = np.nonzero(adj)
    a = torch.sparse_coo_tensor(_dev(np.stack([r, c]), torch.int64), _dev(adj[r, c]), (N, N), is_coalesced=True)
    x = torch.randn(1, 3, N, 12, device=DEV)
    m = ms_gat_amd.GraphAttention(3, 12).to(DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(Exception, match="not cached yet"):
        with torch.cuda.graph(graph):
            m(x, a)


# ---- MSGAT(learn_edge_weights=True) under the Trainer ------------------------------------------------------------

def test_learned_edge_weights_train_captured_and_eager(tmp_path):
    import copy
    from ms_gat_amd import data, engine, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=32, n_edges=40, n_channels=1, in_hours=[1, 2, 3], batch_size=8, days=2)
    base = model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj)
    keys = set(base.state_dict())
    assert not any(k.startswith("edge_") for k in keys)
    torch.manual_seed(0)
    net = model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                        learn_edge_weights=True)
    assert set(net.state_dict()) == keys | {"edge_crow", "edge_col", "edge_weight"}
    nz = ds.adj[ds.adj != 0]
    assert torch.equal(net.edge_weight.detach(), nz)                  # initialised from adj after reset_parameters
    net.to(DEV)
    twin = copy.deepcopy(net)
    w0 = net.edge_weight.detach().clone()
    batches = [b for _, b in zip(range(4), ds.training)]
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True)
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
    assert len(graphed._graphs) == 1
    assert rel_err(twin.edge_weight.detach().cpu(), net.edge_weight.detach().cpu()) < 2e-2
    assert (net.edge_weight.detach() - w0).abs().max() > 1e-4                  # the weights move
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    net.stack_components = False                                       # the per-component loop takes the same path
    X, H, D = (t.to(DEV) for t in batches[0][:3])
    with torch.no_grad():
        a = net(X, H, D)
        net.stack_components = True
        b = net(X, H, D)
    assert rel_err(a.cpu(), b.cpu()) < 1e-4


# ---- values in another order or layout than the library's ---------------------------------------------------------

def _dense_reference(x, dz, Wg, alpha, W, adj):
    """z, dx and the dense dadj of the dense path for the same values"""
    xt = _dev(x).requires_grad_(True)
    a = _dev(adj).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), _dev(W), a)
    z.backward(_dev(dz))
    return z.detach(), xt.grad, a.grad.cpu().numpy()


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_strided_values_match_the_dense_path(layout):
    """values that are a column of a [nnz, 2] parameter: not contiguous, read through the pattern's own buffer"""
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=21)
    z0, dx0, da0 = _dense_reference(x, dz, Wg, alpha, W, adj)
    r, c = np.nonzero(adj)
    both = torch.nn.Parameter(torch.stack([_dev(adj[r, c]), _dev(adj[r, c] * 3)], 1))      # [nnz, 2]
    vals = both[:, 0]
    if layout == "coo":
        a = torch.sparse_coo_tensor(_dev(np.stack([r, c]), torch.int64), vals, (N, N), is_coalesced=True)
        assert not a._values().is_contiguous()
    else:
        crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])
        a = torch.sparse_csr_tensor(_dev(crow, torch.int64), _dev(c, torch.int64), vals, (N, N))
        assert not a.values().is_contiguous()
    xt = _dev(x).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), _dev(W), a)
    z.backward(_dev(dz))
    assert torch.equal(z, z0) and torch.equal(xt.grad, dx0)
    assert_parity(both.grad[:, 0], da0[r, c], "strided " + layout, "dval")
    assert torch.count_nonzero(both.grad[:, 1]) == 0


def test_unsorted_columns_go_through_the_permutation():
    """edge_adjacency with the columns of every row reversed: values gathered into library order, the gradient back"""
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=22)
    z0, dx0, da0 = _dense_reference(x, dz, Wg, alpha, W, adj)
    r, c = np.nonzero(adj)
    crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])
    perm = np.concatenate([np.arange(crow[i], crow[i + 1])[::-1] for i in range(N)]).astype(np.int64)
    rs, cs = r[perm], c[perm]
    crow_t, col_t = _dev(crow, torch.int64), _dev(cs, torch.int64)
    w = torch.nn.Parameter(_dev(adj[rs, cs]))
    a = ops.edge_adjacency(crow_t, col_t, w)
    assert not ms_gat_amd.graph.sparse_pattern_of(a).identity
    xt = _dev(x).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), _dev(W), a)
    z.backward(_dev(dz))
    assert torch.equal(z, z0) and torch.equal(xt.grad, dx0)
    assert_parity(w.grad, da0[rs, cs], "unsorted columns", "dval")
    # the same bits as the sorted order, permuted
    ws = torch.nn.Parameter(_dev(adj[r, c]))
    ops.gacn(_dev(x), _dev(alpha), _dev(Wg), _dev(W), ops.edge_adjacency(crow_t, _dev(c, torch.int64), ws)).backward(_dev(dz))
    assert torch.equal(w.grad, ws.grad[_dev(perm, torch.int64)])


def test_uncoalesced_coo_duplicates_add():
    """a COO index stored twice: the forward sees the sum, and both entries get the gradient of that edge"""
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W, adj = _case(B, C, O, N, T, seed=23)
    r, c = np.nonzero(adj)
    dup = np.arange(0, len(r), 5)                         # every fifth edge stored twice, its weight split in two parts
    part = adj[r[dup], c[dup]] * np.float32(0.25)
    vals_np = np.concatenate([adj[r, c], part]).astype(np.float32)
    vals_np[dup] = adj[r[dup], c[dup]] - part
    summed = adj.copy()
    summed[r[dup], c[dup]] = vals_np[dup] + part          # float32 sums, as coalesce forms them
    z0, dx0, da0 = _dense_reference(x, dz, Wg, alpha, W, summed)
    ri, ci = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    vals = torch.nn.Parameter(_dev(vals_np))
    a = torch.sparse_coo_tensor(_dev(np.stack([ri, ci]), torch.int64), vals, (N, N))
    assert not a.is_coalesced()
    xt = _dev(x).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), _dev(W), a)
    z.backward(_dev(dz))
    assert torch.equal(z, z0) and torch.equal(xt.grad, dx0)
    assert_parity(vals.grad, da0[ri, ci], "uncoalesced coo", "dval")
