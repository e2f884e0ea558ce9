"""GPU: signal-dependent edge weights, `w[b,e] = base[e] + sum_k a[b,row(e),k] * b[b,col(e),k]` with `ab = (a, b)` [B,N,2d]
(msgat_edge_signal_weights{,_backward}, `ops.edge_signal_weights`, `model.EdgeSignalWeights`,
`MSGAT(learn_edge_weights="signal")`).

The kernels through the C ABI and through the op, on DIRECTED patterns built by hand (a kernel that walks the CSR where it
needs the CSC fails on them): the forward within the rounding bound of a length-d fp32 dot product plus one addition of a
float64 reference; the backward's dbase bit-equal to a float32 loop from +0 in ascending sample order, da / db within the
rounding bound of a (degree)-term fp32 sum of float64, exact zero rows for nodes without edges, NULL outputs, determinism;
a HIP-graph capture whose replay follows new `ab` and `dout`.  The model: a fresh "signal" model against a `True` model, a
trained state against the same model fed the weights formed by torch ops (also on a directed graph), `EdgeSignalWeights`
feeding a GACN, the attention maps, and the Trainer eager / captured / "auto" and with the guard and a null value.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import assert_parity, rel_err

import ms_gat_amd
from ms_gat_amd import _lib, graph, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -24


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---- directed patterns -----------------------------------------------------------------------------------------------

def _csr(n, edges):
    """(crow [n+1], col [nnz], row [nnz]) int64 of the distinct directed edges (i, j), in CSR order"""
    keys = np.unique(np.array([i * n + j for i, j in edges], dtype=np.int64))
    row, col = keys // n, keys % n
    crow = np.zeros(n + 1, np.int64)
    np.add.at(crow, row + 1, 1)
    return np.cumsum(crow), col, row


def _ring():
    n = 7
    return n, [(i, (i + 1) % n) for i in range(n)] + [(0, 3), (2, 5), (5, 1), (6, 2)]


def _hub():
    n = 70      # row 0 and column 3 are longer than one wave
    return n, [(0, j) for j in range(n)] + [(i, 3) for i in range(n)] + [(i, i) for i in (10, 20, 30)]


NO_OUT, NO_IN, NEITHER = (5, 6), (7, 8), (9, 64)


def _holes():
    n, edges = 65, []
    for i in range(n):
        if i in NO_OUT or i in NEITHER:
            continue
        for j in ((3 * i + 11) % n, (i + 1) % n):
            while j in NO_IN or j in NEITHER:
                j = (j + 1) % n
            edges.append((i, j))
    return n, edges


def _road():
    adj = ms_gat_amd.synthetic_adjacency(883, 866, seed=1)
    i, j = np.nonzero(adj.numpy())
    return 883, list(zip(i.tolist(), j.tolist()))


PATTERNS = {"ring7": _ring, "hub70": _hub, "holes65": _holes, "loop1": lambda: (1, [(0, 0)]), "empty5": lambda: (5, []),
            "road883": _road}


@functools.lru_cache(maxsize=None)
def _pattern(name):
    """(n, crow, col, row as numpy, device crow / col, the library's structure on the device)"""
    n, edges = PATTERNS[name]()
    crow, col, row = _csr(n, edges)
    crow_t, col_t = _dev(crow, torch.int64), _dev(col, torch.int64)
    pat = graph.edge_pattern_of(crow_t, col_t)
    assert pat.identity and pat.structure.nnz == len(col)
    return n, crow, col, row, crow_t, col_t, pat.structure.on(DEV)[0]


def test_the_patterns_are_directed_and_have_the_degrees_they_are_meant_to_have():
    for name in ("ring7", "hub70", "holes65"):
        n, crow, col, row = _pattern(name)[:4]
        edges = set(zip(row.tolist(), col.tolist()))
        assert any((j, i) not in edges for i, j in edges), name              # not symmetric
    n, crow, col, row = _pattern("hub70")[:4]
    assert crow[1] - crow[0] == 70 and np.count_nonzero(col == 3) == 70
    n, crow, col, row = _pattern("holes65")[:4]
    out_deg, in_deg = np.diff(crow), np.bincount(col, minlength=n)
    assert all(out_deg[i] == 0 and in_deg[i] > 0 for i in NO_OUT)
    assert all(in_deg[i] == 0 and out_deg[i] > 0 for i in NO_IN)
    assert all(in_deg[i] == 0 and out_deg[i] == 0 for i in NEITHER)
    assert _pattern("road883")[2].size == 2615


# ---- references, computed once per case ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name, B, d):
    """Inputs (float32) and float64 references with their per-entry bounds."""
    n, crow, col, row = _pattern(name)[:4]
    nnz = col.size
    rng = np.random.default_rng(1000 * B + d + n)
    base = rng.standard_normal(nnz).astype(np.float32)
    ab = rng.standard_normal((B, n, 2 * d)).astype(np.float32)
    dout = rng.standard_normal((B, nnz)).astype(np.float32)
    a, b = ab[..., :d].astype(np.float64), ab[..., d:].astype(np.float64)
    prod = a[:, row, :] * b[:, col, :]                                      # [B,nnz,d]
    w = base.astype(np.float64)[None] + prod.sum(-1)
    w_bound = (d + 2) * EPS * (np.abs(base.astype(np.float64))[None] + np.abs(prod).sum(-1))
    g = dout.astype(np.float64)[..., None]
    ta, tb = g * b[:, col, :], g * a[:, row, :]                             # the terms of da (at row), db (at col)
    dab, mag = np.zeros((B, n, 2 * d)), np.zeros((B, n, 2 * d))
    for e in range(nnz):
        dab[:, row[e], :d] += ta[:, e]
        mag[:, row[e], :d] += np.abs(ta[:, e])
        dab[:, col[e], d:] += tb[:, e]
        mag[:, col[e], d:] += np.abs(tb[:, e])
    deg = np.concatenate([np.repeat(np.diff(crow)[:, None], d, 1), np.repeat(np.bincount(col, minlength=n)[:, None], d, 1)], 1)
    dab_bound = (deg[None] + 1) * EPS * mag
    dbase = np.zeros(nnz, np.float32)
    for s in range(B):                                                      # float32, from +0, ascending b
        dbase += dout[s]
    return dict(base=base, ab=ab, dout=dout, w=w, w_bound=w_bound, dab=dab, dab_bound=dab_bound, dbase=dbase, deg=deg)


def _forward_abi(name, base, ab, B, d):
    nnz = _pattern(name)[2].size
    out = torch.full((B, nnz), float("nan"), device=DEV)
    st = _lib.lib().msgat_edge_signal_weights(_pattern(name)[6], base.data_ptr(), ab.data_ptr(), B, d, out.data_ptr(),
                                              _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return out


def _backward_abi(name, dout, ab, B, d, want=(True, True)):
    """(dbase, dab), each pre-filled with NaN, None where not asked for"""
    n, nnz = _pattern(name)[0], _pattern(name)[2].size
    outs = [torch.full(shape, float("nan"), device=DEV) if on else None for shape, on in zip(((nnz,), (B, n, 2 * d)), want)]
    st = _lib.lib().msgat_edge_signal_weights_backward(_pattern(name)[6], dout.data_ptr(), ab.data_ptr(), B, d,
                                                       *[None if t is None else t.data_ptr() for t in outs],
                                                       _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return outs


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32))


SMALL = [(name, B, d) for name in ("ring7", "hub70", "holes65", "loop1", "empty5") for B in (1, 3, 32) for d in (4, 8, 32)]
CASES = SMALL + [("road883", 32, 8)]
AHEAD = 8         # kEsAhead of csrc/edge_signal.hip: the samples of dout a dbase lane loads before it adds them


def _check_forward(got: torch.Tensor, c, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - c["w"])
    worst = float((err / np.maximum(c["w_bound"], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: forward worst error / bound {worst:.3f}")
    assert (err <= c["w_bound"]).all(), (what, worst)


def _check_dab(got: torch.Tensor, c, what):
    g = got.cpu().numpy()
    assert np.isfinite(g).all(), what                                       # the NaN pre-fill is gone: every entry written
    err = np.abs(g.astype(np.float64) - c["dab"])
    worst = float((err / np.maximum(c["dab_bound"], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: da / db worst error / bound {worst:.3f}")
    assert (err <= c["dab_bound"]).all(), (what, worst)
    lonely = np.broadcast_to(c["deg"][None] == 0, g.shape)
    assert not g.view(np.int32)[lonely].any(), what                         # +0, not -0, where a node has no edge


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,d", CASES)
def test_forward_is_within_the_dot_product_bound_of_float64(name, B, d):
    c = _case(name, B, d)
    got = _forward_abi(name, _dev(c["base"]), _dev(c["ab"]), B, d)
    assert got.numel() == 0 or bool(torch.isfinite(got).all())
    _check_forward(got, c, f"edge_signal {name} b{B} d{d}")


# ("ring7", AHEAD + 3, 4): one full load-ahead group plus a tail of three -- B = 1, 3 and 32 never mix the two
@pytest.mark.parametrize("name,B,d", CASES + [("ring7", AHEAD + 3, 4)])
def test_backward_sums_in_order_and_writes_every_entry(name, B, d):
    c = _case(name, B, d)
    dout, ab = _dev(c["dout"]), _dev(c["ab"])
    what = f"edge_signal {name} b{B} d{d}"
    dbase, dab = _backward_abi(name, dout, ab, B, d)
    assert _same_bits(dbase, c["dbase"]), what
    _check_dab(dab, c, what)
    again = _backward_abi(name, dout, ab, B, d)                             # two calls give the same bits
    assert _same_bits(again[0], dbase.cpu().numpy()) and _same_bits(again[1], dab.cpu().numpy()), what


@pytest.mark.parametrize("name", ["hub70", "holes65"])
def test_backward_null_outputs_leave_the_other_unchanged(name):
    B, d = 3, 8
    c = _case(name, B, d)
    dout, ab = _dev(c["dout"]), _dev(c["ab"])
    full = _backward_abi(name, dout, ab, B, d)
    only_base = _backward_abi(name, dout, ab, B, d, want=(True, False))
    only_dab = _backward_abi(name, dout, ab, B, d, want=(False, True))
    assert only_base[1] is None and only_dab[0] is None
    assert torch.equal(only_base[0], full[0]) and torch.equal(only_dab[1], full[1])


def test_empty_sizes_write_what_they_must_and_nothing_else():
    L, s = _lib.lib(), _lib.stream_handle(DEV)
    g = _pattern("empty5")[6]
    guard = torch.full((64,), float("nan"), device=DEV)
    ab = torch.randn(3, 5, 16, device=DEV)
    assert L.msgat_edge_signal_weights(g, guard.data_ptr(), ab.data_ptr(), 3, 8, guard.data_ptr(), s) == 0
    dab = torch.full((3, 5, 16), float("nan"), device=DEV)
    assert L.msgat_edge_signal_weights_backward(g, None, ab.data_ptr(), 3, 8, guard.data_ptr(), dab.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all()) and not dab.cpu().numpy().view(np.int32).any()         # no edge: dab is +0
    # B = 0: nothing written
    g = _pattern("ring7")[6]
    assert L.msgat_edge_signal_weights(g, guard.data_ptr(), guard.data_ptr(), 0, 8, guard.data_ptr(), s) == 0
    assert L.msgat_edge_signal_weights_backward(g, guard.data_ptr(), guard.data_ptr(), 0, 8, guard.data_ptr(),
                                                guard.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all())


# ---- the op ----------------------------------------------------------------------------------------------------------

def _torch_weights(base, ab, crow, col):
    """the torch-op formulation: two gathers, a product, a reduction in ascending k (fp32 torch ops contract nothing, so its
    bits are defined -- the kernel's order); torch autograd scatters with index_add_"""
    d = ab.shape[-1] // 2
    rows = torch.repeat_interleave(torch.arange(crow.numel() - 1, device=crow.device), crow[1:] - crow[:-1])
    p = ab[:, rows, :d] * ab[:, col, d:]
    s = p[..., 0]
    for k in range(1, d):
        s = s + p[..., k]
    return base + s


@pytest.mark.parametrize("name,B,d", [("hub70", 3, 4), ("holes65", 32, 32), ("road883", 32, 8)])
def test_op_forward_and_backward(name, B, d):
    c = _case(name, B, d)
    n, crow, col = _pattern(name)[0], _pattern(name)[4], _pattern(name)[5]
    what = f"edge_signal op {name} b{B} d{d}"
    base, ab = _dev(c["base"]).requires_grad_(True), _dev(c["ab"]).requires_grad_(True)
    dout = _dev(c["dout"])
    w = ops.edge_signal_weights(base, ab, crow, col)
    assert w.shape == (B, col.numel()) and w.is_contiguous() and w.dtype == torch.float32
    _check_forward(w.detach(), c, what)
    w.backward(dout)
    assert _same_bits(base.grad, c["dbase"])
    _check_dab(ab.grad, c, what)
    # torch autograd of the torch-op formulation
    base_t, ab_t = base.detach().clone().requires_grad_(True), ab.detach().clone().requires_grad_(True)
    w_t = _torch_weights(base_t, ab_t, crow, col)
    assert torch.equal(w.detach(), w_t.detach()), what                      # the bits of the torch ops in the kernel's order
    assert_parity(w.detach(), base.detach() + (ab.detach()[:, _dev(_pattern(name)[3], torch.int64), :d] * ab.detach()[:, col, d:]).sum(-1),
                  what, "w against sum(-1)")
    w_t.backward(dout)
    assert_parity(base.grad, base_t.grad, what, "dbase")
    assert_parity(ab.grad, ab_t.grad, what, "dab")
    # the structure is the one edge_adjacency(crow, col, .) resolves to
    sets = graph.sparse_graph_for(ops.edge_adjacency(crow, col, w.detach()), B, 1)[1]
    assert sets.structure is graph.edge_pattern_of(crow, col).structure
    # gradients only where they are asked for
    frozen = ab.detach().clone()
    (g_base,) = torch.autograd.grad(ops.edge_signal_weights(base, frozen, crow, col), (base,), dout)
    assert torch.equal(g_base, base.grad) and frozen.grad is None
    (g_ab,) = torch.autograd.grad(ops.edge_signal_weights(base.detach(), ab, crow, col), (ab,), dout)
    assert torch.equal(g_ab, ab.grad)
    # honours autocast like the other ops: float32 in and out, half-precision operands are cast back at the boundary
    with torch.autocast("cuda", dtype=torch.float16):
        wa = ops.edge_signal_weights(base, ab, crow, col)
        wh = ops.edge_signal_weights(base.detach().half(), ab.detach().half(), crow, col)
    assert wa.dtype == torch.float32 and torch.equal(wa, w) and wh.dtype == torch.float32
    with pytest.raises(RuntimeError, match="differentiate twice"):
        w2 = ops.edge_signal_weights(base, ab, crow, col)
        (g,) = torch.autograd.grad(w2, base, dout.clone().requires_grad_(True), create_graph=True)
        g.sum().backward()


def test_op_refuses_what_it_cannot_run():
    n, crow, col = _pattern("ring7")[0], _pattern("ring7")[4], _pattern("ring7")[5]
    base, ab = torch.zeros(col.numel(), device=DEV), torch.zeros(2, n, 16, device=DEV)
    for bad in (torch.zeros(2, n, 12, device=DEV), torch.zeros(2, n, 72, device=DEV), torch.zeros(2, n, 4, device=DEV),
                torch.zeros(2, n, 15, device=DEV), torch.zeros(2, n + 1, 16, device=DEV), torch.zeros(n, 16, device=DEV)):
        with pytest.raises(ValueError, match="edge_signal_weights"):
            ops.edge_signal_weights(base, bad, crow, col)
    with pytest.raises(ValueError, match="edge_signal_weights"):
        ops.edge_signal_weights(base[:-1], ab, crow, col)
    with pytest.raises(ValueError, match="edge_signal_weights"):
        ops.edge_signal_weights(base, ab, crow.cpu(), col)
    with pytest.raises(ValueError, match="edge_signal_weights"):
        ops.edge_signal_weights(base, ab, crow, col.cpu())
    with pytest.raises(TypeError, match="float32"):
        ops.edge_signal_weights(base, ab.double(), crow, col)


def test_op_takes_columns_in_any_order_inside_a_row():
    """(crow, col) with a row's columns reversed: values and gradients stay in the caller's order"""
    name, B, d = "hub70", 3, 8
    c = _case(name, B, d)
    n, crow_np, col_np = _pattern(name)[0], _pattern(name)[1], _pattern(name)[2]
    perm = np.concatenate([np.arange(crow_np[i], crow_np[i + 1])[::-1] for i in range(n)])
    crow, col = _pattern(name)[4], _dev(col_np[perm], torch.int64)
    base, ab = _dev(c["base"][perm]).requires_grad_(True), _dev(c["ab"]).requires_grad_(True)
    w = ops.edge_signal_weights(base, ab, crow, col)
    sorted_w = ops.edge_signal_weights(_dev(c["base"]), _dev(c["ab"]), crow, _pattern(name)[5])
    assert torch.equal(w.detach(), sorted_w[:, _dev(perm, torch.int64)])
    w.backward(_dev(c["dout"][:, perm]))
    assert _same_bits(base.grad, c["dbase"][perm])
    _check_dab(ab.grad, c, "edge_signal reversed rows")


def test_hip_graph_replay_follows_new_contents():
    name, B, d = "road883", 32, 8
    c = _case(name, B, d)
    n, crow, col = _pattern(name)[0], _pattern(name)[4], _pattern(name)[5]
    base, ab = torch.nn.Parameter(_dev(c["base"])), torch.nn.Parameter(_dev(c["ab"]))
    dout = _dev(c["dout"])
    out = torch.empty((B, col.numel()), device=DEV)

    def step():
        base.grad.zero_()
        ab.grad.zero_()
        w = ops.edge_signal_weights(base, ab, crow, col)
        out.copy_(w.detach())
        w.backward(dout)

    ops.edge_signal_weights(base, ab, crow, col).backward(dout)             # the grads exist
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured):
        step()
    first = out.clone()
    for seed in (1, 2):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            ab.copy_(torch.randn(ab.shape, generator=gen))
        dout.copy_(torch.randn(dout.shape, generator=gen))
        captured.replay()
        torch.cuda.synchronize()
        replayed = [out.clone(), base.grad.clone(), ab.grad.clone()]
        assert not torch.equal(replayed[0], first)
        step()
        torch.cuda.synchronize()
        for u, v in zip(replayed, (out, base.grad, ab.grad)):
            assert torch.equal(u, v), seed
        assert torch.equal(out, _torch_weights(base.detach(), ab.detach(), crow, col)), seed


# ---- the model -------------------------------------------------------------------------------------------------------

N_NODES, N_EDGES, R, BATCH = 32, 40, 3, 8


def _dataset():
    from ms_gat_amd import data
    torch.manual_seed(0)
    return data.SyntheticPEMS(n_nodes=N_NODES, n_edges=N_EDGES, n_channels=1, in_hours=[1, 2, 3], batch_size=BATCH, days=2)


def _model(adj, learn, seed=0):
    from ms_gat_amd import model
    torch.manual_seed(seed)
    return model.msgat48(n_components=R, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=adj,
                         learn_edge_weights=learn)


def _randomise_proj(net, seed=1, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        t = net.edge_proj.weight
        t.copy_((torch.randn(t.shape, generator=g) * scale).to(t.device))


def _step(net, X, H, D, dY):
    net.zero_grad(set_to_none=True)
    out = net(X, H, D)
    (out * dY).sum().backward()
    return out.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def _torch_adjacency(twin):
    """`adjacency` of a "signal" model with the weights formed by torch ops"""
    def adjacency(H=None, D=None, X=None):
        ab = twin.edge_proj(twin.edge_features(X))
        return ops.edge_adjacency(twin.edge_crow, twin.edge_col, _torch_weights(twin.edge_weight, ab, twin.edge_crow, twin.edge_col))
    return adjacency


@pytest.fixture(scope="module")
def batch():
    ds = _dataset()
    X, H, D, Y = (t.to(DEV) for t in next(iter(ds.training)))
    dY = torch.randn(Y.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    return ds, X, H, D, dY


@pytest.mark.parametrize("stack", [True, False])
def test_fresh_signal_model_is_the_static_model(batch, stack):
    """A zero column half: every sample's weights are the base, so the model computes what a `True` model with the same
    parameters computes -- through the per-sample path (B value sets) instead of one set: the bar of the per-sample tests
    against another route (assert_parity), not bits."""
    ds, X, H, D, dY = batch
    static = _model(ds.adj, True).to(DEV)
    signal = _model(ds.adj, "signal", seed=3)
    missing = signal.load_state_dict({k: v.cpu() for k, v in static.state_dict().items()}, strict=False)
    assert missing.missing_keys == ["edge_proj.weight"]
    signal.to(DEV)
    static.stack_components = signal.stack_components = stack
    want, want_g = _step(static, X, H, D, dY)
    got, got_g = _step(signal, X, H, D, dY)
    what = f"signal vs static, stacked={stack}"
    assert_parity(got, want, what, "out")
    assert set(got_g) == set(want_g) | {"edge_proj.weight"}
    gscale = max(float(v.abs().max()) for v in want_g.values())
    for k, v in want_g.items():
        if float(v.abs().max()) < 1e-2 * gscale:      # a near-cancelling scalar: judged on the scale of the largest gradient
            assert float((got_g[k] - v).abs().max()) < 1e-4 * 1e-2 * gscale, k
        else:
            assert_parity(got_g[k], v, what, k)
    # at step 0 the column half moves (its gradient is the row side's values), the row half's gradient is exactly zero
    gp, rank = got_g["edge_proj.weight"], signal.edge_rank
    assert float(gp[rank:].abs().max()) > 0 and torch.count_nonzero(gp[:rank]) == 0


def _directed(adj):
    """the dataset's graph with a few entries zeroed on one side of the diagonal only"""
    adj = adj.clone()
    i, j = torch.nonzero(torch.triu(adj, 1), as_tuple=True)
    adj[i[::3], j[::3]] = 0
    assert not torch.equal(adj != 0, (adj != 0).T)
    return adj


@pytest.mark.parametrize("stack,directed", [(True, False), (False, False), (True, True)])
def test_trained_state_equals_the_torch_op_formulation(batch, stack, directed):
    """A random non-zero projection; the reference is the same model fed `ops.edge_adjacency(crow, col, torch expression)`,
    whose gradients torch autograd sums."""
    ds, X, H, D, dY = batch
    net = _model(_directed(ds.adj) if directed else ds.adj, "signal").to(DEV)
    _randomise_proj(net)
    twin = copy.deepcopy(net)
    net.stack_components = twin.stack_components = stack
    got, got_g = _step(net, X, H, D, dY)
    twin.adjacency = _torch_adjacency(twin)
    want, want_g = _step(twin, X, H, D, dY)
    what = f"signal vs torch ops, stacked={stack}, directed={directed}"
    assert torch.equal(got, want), what
    for k in ("edge_weight", "edge_proj.weight"):
        assert float(want_g[k].abs().max()) > 0
        assert_parity(got_g[k], want_g[k], what, k)
    rank = net.edge_rank
    assert float(got_g["edge_proj.weight"][:rank].abs().max()) > 0 and float(got_g["edge_proj.weight"][rank:].abs().max()) > 0
    for k, v in want_g.items():
        if not k.startswith("edge_"):
            assert torch.equal(got_g[k], v), k                                # the same weights, the same kernels


def test_edge_signal_weights_feeds_a_gacn(batch):
    from ms_gat_amd import model
    ds, X, H, D, dY = batch
    csr = _directed(ds.adj).to_sparse_csr()
    emb = model.EdgeSignalWeights(csr.crow_indices(), csr.col_indices(), csr.values(), in_features=12, rank=4).to(DEV)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        emb.proj.weight.copy_(torch.randn(emb.proj.weight.shape, generator=g) * 0.1)
    f = model.MSGAT.edge_features(X).clone().requires_grad_(True)
    w = emb.weights(f)
    assert torch.equal(w, _torch_weights(emb.weight, emb.proj(f), emb.crow, emb.col))
    adj = emb(f)
    assert adj.layout == torch.sparse_csr and tuple(adj.shape) == (BATCH, N_NODES, N_NODES)
    rows = torch.repeat_interleave(torch.arange(N_NODES, device=DEV), emb.crow[1:] - emb.crow[:-1])
    dense = torch.zeros(BATCH, N_NODES, N_NODES, device=DEV)
    dense[:, rows, emb.col] = w.detach()
    gacn = ms_gat_amd.GACN(3, 24, 12).to(DEV)
    with torch.no_grad():
        for p in gacn.parameters():
            p.normal_(0, 0.3, generator=None)
    x = torch.randn(BATCH, 3, N_NODES, 12, device=DEV)
    dz = torch.randn(BATCH, 24, N_NODES, 12, device=DEV)
    dense.requires_grad_(True)
    want = gacn(x, dense)
    want.backward(dz)
    got = gacn(x, adj)
    emb.zero_grad()
    got.backward(dz)
    assert_parity(got, want, "EdgeSignalWeights", "z")
    dw = dense.grad[:, rows, emb.col]                                         # [B,nnz]: the gradient at the weights
    assert_parity(emb.weight.grad, dw.double().sum(0).cpu().numpy(), "EdgeSignalWeights", "dweight")
    # the projection and the features through torch autograd of the torch-op formulation, from the same dw
    f_t = f.detach().clone().requires_grad_(True)
    proj_t = emb.proj.weight.detach().clone().requires_grad_(True)
    _torch_weights(emb.weight.detach(), f_t @ proj_t.T, emb.crow, emb.col).backward(dw)
    assert_parity(emb.proj.weight.grad, proj_t.grad, "EdgeSignalWeights", "dproj")
    assert_parity(f.grad, f_t.grad, "EdgeSignalWeights", "df")


def test_attention_maps_follow_the_samples_own_weights(batch):
    ds, X, H, D, dY = batch
    net = _model(ds.adj, "signal").to(DEV)
    _randomise_proj(net, scale=0.3)
    with torch.no_grad():
        w = ops.edge_signal_weights(net.edge_weight, net.edge_proj(net.edge_features(X)), net.edge_crow, net.edge_col)
    rows = torch.repeat_interleave(torch.arange(N_NODES, device=DEV), net.edge_crow[1:] - net.edge_crow[:-1])
    cols = net.edge_col
    assert float((w[0] - w[1]).abs().max()) > 1e-2           # two samples, two graphs
    keys = sorted(f"tpcs.{r}.tgacns.{l}.gacn" for r in range(R) for l in range(2))
    for stack in (True, False):
        net.stack_components = stack
        soft = net.attention_maps(X, H, D, weights="softmax")
        masked = net.attention_maps(X, H, D, weights="masked")
        assert sorted(soft) == keys and sorted(masked) == keys
        for k in keys:
            att, m = soft[k], masked[k].to_dense()
            assert tuple(att.shape) == (BATCH, N_NODES, N_NODES) and tuple(m.shape) == (BATCH, N_NODES, N_NODES)
            want = att[:, rows, cols] * w                      # att * the sample's own adjacency, at the stored edges
            assert torch.allclose(m[:, rows, cols], want, rtol=1e-5, atol=1e-6), (k, stack)
            off = torch.ones(N_NODES, N_NODES, dtype=torch.bool, device=DEV)
            off[rows, cols] = False
            assert torch.count_nonzero(m[:, off]) == 0


# ---- the Trainer -----------------------------------------------------------------------------------------------------

def test_signal_model_trains_eager_captured_and_auto(tmp_path):
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds.adj, "signal").to(DEV)
    twin, auto = copy.deepcopy(net), copy.deepcopy(net)
    w0 = net.edge_weight.detach().clone()
    p0 = net.edge_proj.weight.detach().clone()
    batches = [b for _, b in zip(range(4), ds.training)]
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True)
    lazily = engine.Trainer(auto, 50.0, str(tmp_path / "auto"), hip_graph="auto")
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        la = lazily.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        print(f"epoch {epoch}: loss eager {le!r}, captured {lg!r}, auto {la!r}")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
        assert abs(le - la) < 1e-4 * abs(le), (epoch, le, la)
    assert len(graphed._graphs) == 1 and len(lazily._graphs) == 1
    rank = net.edge_rank
    proj = net.edge_proj.weight.detach()
    assert float(proj[rank:].abs().max()) > 1e-4                              # the column half leaves zero
    assert float((proj[:rank] - p0[:rank]).abs().max()) > 1e-5                # and then the row half moves too
    assert (net.edge_weight.detach() - w0).abs().max() > 1e-4
    for other, tag in ((twin, "captured"), (auto, "auto")):
        for (name, p), q in zip(net.named_parameters(), other.parameters()):
            assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, (tag, name)


def test_signal_model_trains_with_the_guard_and_a_null_value(tmp_path):
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds.adj, "signal").to(DEV)
    twin = copy.deepcopy(net)
    batches = [b for _, b in zip(range(4), ds.training)]
    kwargs = dict(null_value=0.0, max_grad_norm=0.25, skip_nonfinite=True)
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, **kwargs)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True, **kwargs)
    le = eager.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    lg = graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    assert abs(le - lg) < 1e-4 * abs(le), (le, lg)
    for tr in (eager, graphed):
        assert tr.last_stats["skipped_steps"] == 0 and 0.0 < tr.last_stats["grad_norm_max"] < float("inf")
    assert len(graphed._graphs) == 1
    assert float(net.edge_proj.weight.detach()[net.edge_rank:].abs().max()) > 1e-4
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
