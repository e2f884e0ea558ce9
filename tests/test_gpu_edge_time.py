"""GPU: hour- and day-dependent edge weights, `w[b,e] = (base[e] + h_w[H[b]][e]) + d_w[D[b]][e]`
(msgat_edge_time_weights{,_backward}, `ops.edge_time_weights`, `model.EdgeTimeEmbedding`, `MSGAT(learn_edge_weights="time")`).

The kernels through the C ABI and through the op: the forward bit-equal to the torch expression, the backward bit-equal
to a float32 loop that starts every sum at +0 and adds in ascending sample order (only additions: the bits are defined) and
within the per-entry parity rule of the float64 index_add; every row written, NULL outputs, empty sizes, clamped indices,
more table rows than a block keeps, more samples than a tile stages; determinism; a HIP-graph capture whose replay follows
new H / D.  The model: a fresh "time" model against a `True` model, a trained state against the same model fed the
weights formed by torch ops, the Trainer eager / captured / "auto" and with the guard and a null value, the attention maps.
"""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_parity, rel_err

import ms_gat_amd
from ms_gat_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TILE = 256        # kEtSamples of csrc/edge_time.hip: the samples whose table rows a block stages at a time


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---- cases -----------------------------------------------------------------------------------------------------------

def _index_patterns(B, nh, nd):
    """name -> (H, D as handed over, H, D as the kernel must read them)"""
    b = np.arange(B)
    out = {
        "arange": (b % nh, b % nd),
        "one row": (np.full(B, min(5, nh - 1)), np.full(B, min(3, nd - 1))),
        "boundary rows": (np.where(b % 2 == 0, 0, nh - 1), np.where(b % 3 == 0, nd - 1, 0)),
    }
    out = {k: (h, d, h, d) for k, (h, d) in out.items()}
    h = np.array([-1, nh, 5 % nh, nh + 76])[b % 4]
    d = np.array([nd, -1, -9, 3 % nd])[b % 4]
    out["out of range"] = (h, d, np.clip(h, 0, nh - 1), np.clip(d, 0, nd - 1))
    return out


def _tables(nnz, nh, nd, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(nnz).astype(np.float32), rng.standard_normal((nh, nnz)).astype(np.float32),
            rng.standard_normal((nd, nnz)).astype(np.float32))


def _forward_abi(base, h_w, d_w, H, D, B, nnz, nh, nd):
    out = torch.full((B, nnz), float("nan"), device=DEV)
    st = _lib.lib().msgat_edge_time_weights(base.data_ptr(), h_w.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                            H.data_ptr(), None if D is None else D.data_ptr(), out.data_ptr(), B, nnz, nh, nd,
                                            _lib.stream_handle(DEV))
    assert st == 0, st
    return out


def _backward_abi(dout, H, D, B, nnz, nh, nd, want=(True, True, True)):
    """(dbase, dh_w, dd_w), each pre-filled with NaN, None where not asked for"""
    outs = [torch.full(shape, float("nan"), device=DEV) if on else None
            for shape, on in zip(((nnz,), (nh, nnz), (nd, nnz)), want)]
    st = _lib.lib().msgat_edge_time_weights_backward(
        dout.data_ptr(), H.data_ptr(), D.data_ptr(), *[None if t is None else t.data_ptr() for t in outs], B, nnz, nh, nd,
        _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return outs


def _loop_f32(dout, H, D, nh, nd):
    """float32, every sum from +0 in ascending b (numpy float32 rows: one rounding per addition, as the kernel's)"""
    B, nnz = dout.shape
    dbase, dh, dd = np.zeros(nnz, np.float32), np.zeros((nh, nnz), np.float32), np.zeros((nd, nnz), np.float32)
    for b in range(B):
        dbase += dout[b]
        dh[H[b]] += dout[b]
        dd[D[b]] += dout[b]
    return dbase, dh, dd


def _index_add_f64(dout, H, D, nh, nd):
    d64 = torch.from_numpy(dout).double()
    nnz = dout.shape[1]
    return (d64.sum(0).numpy(),
            torch.zeros(nh, nnz, dtype=torch.float64).index_add_(0, torch.from_numpy(H).long(), d64).numpy(),
            torch.zeros(nd, nnz, dtype=torch.float64).index_add_(0, torch.from_numpy(D).long(), d64).numpy())


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32))


SHAPES = [(nnz, B) for nnz in (1, 63, 64, 65, 257, 2615) for B in (1, 3, 32, 70)] + [(65, TILE + 1), (65, 2 * TILE + 9)]


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nnz,B", SHAPES)
def test_forward_has_the_bits_of_the_torch_expression(nnz, B):
    nh, nd = 24, 7
    base, h_w, d_w = (_dev(t) for t in _tables(nnz, nh, nd, seed=nnz + B))
    for name, (h, d, hc, dc) in _index_patterns(B, nh, nd).items():
        H, D, Hc, Dc = (_dev(t, torch.int64) for t in (h, d, hc, dc))
        want = (base + h_w[Hc]) + d_w[Dc]
        assert torch.equal(_forward_abi(base, h_w, d_w, H, D, B, nnz, nh, nd), want), name
        assert torch.equal(_forward_abi(base, h_w, None, H, None, B, nnz, nh, nd), base + h_w[Hc]), name + ", hours only"


@pytest.mark.parametrize("nnz,B", SHAPES)
def test_backward_adds_in_sample_order_and_writes_every_row(nnz, B):
    nh, nd = 24, 7
    dout = np.random.default_rng(7 * nnz + B).standard_normal((B, nnz)).astype(np.float32)
    dout_t = _dev(dout)
    for name, (h, d, hc, dc) in _index_patterns(B, nh, nd).items():
        H, D = _dev(h, torch.int64), _dev(d, torch.int64)
        got = _backward_abi(dout_t, H, D, B, nnz, nh, nd)
        loop, f64 = _loop_f32(dout, hc, dc, nh, nd), _index_add_f64(dout, hc, dc, nh, nd)
        for key, g, w32, w64 in zip(("dbase", "dh_w", "dd_w"), got, loop, f64):
            what = f"edge_time nnz{nnz} b{B} {name}"
            assert bool(torch.isfinite(g).all()), (what, key)          # the NaN pre-fill is gone: every entry written
            assert _same_bits(g, w32), (what, key)
            assert_parity(g, w64, what, key)
        if name == "one row":                 # one row takes everything, every other row is (+)0
            dh = got[1].cpu().numpy()
            assert _same_bits(got[1][hc[0]], loop[0]) and not np.delete(dh, hc[0], axis=0).view(np.int32).any()
        # two runs give the same bits
        again = _backward_abi(dout_t, H, D, B, nnz, nh, nd)
        assert all(_same_bits(a, b.cpu().numpy()) for a, b in zip(again, got)), name


def test_backward_null_outputs_leave_the_others_unchanged():
    nnz, B, nh, nd = 257, 32, 24, 7
    dout = _dev(np.random.default_rng(3).standard_normal((B, nnz)).astype(np.float32))
    h, d, _, _ = _index_patterns(B, nh, nd)["out of range"]
    H, D = _dev(h, torch.int64), _dev(d, torch.int64)
    full = _backward_abi(dout, H, D, B, nnz, nh, nd)
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        got = _backward_abi(dout, H, D, B, nnz, nh, nd, want=want)
        assert got[skip] is None
        for i in range(3):
            if i != skip:
                assert torch.equal(got[i], full[i]), (skip, i)
    only_base = _backward_abi(dout, H, D, B, nnz, nh, nd, want=(True, False, False))
    assert torch.equal(only_base[0], full[0])


def test_backward_more_table_rows_than_a_block_keeps():
    """40 + 9 rows: two row chunks of 32, the hour table split across them, the day table inside the second"""
    nnz, B, nh, nd = 65, 70, 40, 9
    dout = np.random.default_rng(11).standard_normal((B, nnz)).astype(np.float32)
    for name, (h, d, hc, dc) in _index_patterns(B, nh, nd).items():
        got = _backward_abi(_dev(dout), _dev(h, torch.int64), _dev(d, torch.int64), B, nnz, nh, nd)
        for key, g, w32 in zip(("dbase", "dh_w", "dd_w"), got, _loop_f32(dout, hc, dc, nh, nd)):
            assert _same_bits(g, w32), (name, key)


def test_empty_sizes():
    L, s = _lib.lib(), _lib.stream_handle(DEV)
    H, D = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    one = torch.zeros(1, device=DEV)
    p = one.data_ptr()
    assert L.msgat_edge_time_weights(p, p, p, H.data_ptr(), D.data_ptr(), p, 4, 0, 24, 7, s) == 0
    assert L.msgat_edge_time_weights_backward(p, H.data_ptr(), D.data_ptr(), p, p, p, 4, 0, 24, 7, s) == 0
    torch.cuda.synchronize()
    assert float(one) == 0.0
    # B = 0 with nnz > 0: the forward has nothing to write, the backward still writes its zeros
    nnz = 65
    assert L.msgat_edge_time_weights(p, p, p, None, None, p, 0, nnz, 24, 7, s) == 0
    outs = [torch.full(shape, float("nan"), device=DEV) for shape in ((nnz,), (24, nnz), (7, nnz))]
    assert L.msgat_edge_time_weights_backward(None, None, None, *[t.data_ptr() for t in outs], 0, nnz, 24, 7, s) == 0
    torch.cuda.synchronize()
    assert all(not t.cpu().numpy().view(np.int32).any() for t in outs)       # +0 everywhere


# ---- the op ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nnz,B", [(65, 3), (2615, 32)])
def test_op_forward_and_backward(nnz, B):
    nh, nd = 24, 7
    tables = _tables(nnz, nh, nd, seed=5)
    dout = np.random.default_rng(6).standard_normal((B, nnz)).astype(np.float32)
    h, d, hc, dc = _index_patterns(B, nh, nd)["out of range"]
    base, h_w, d_w = (_dev(t).requires_grad_(True) for t in tables)
    for cast in (torch.int64, torch.int32):              # nn.Embedding takes int32 too
        for t in (base, h_w, d_w):
            t.grad = None
        w = ops.edge_time_weights(base, h_w, d_w, _dev(h, cast), _dev(d, cast))
        assert w.shape == (B, nnz) and w.is_contiguous() and w.dtype == torch.float32
        assert torch.equal(w.detach(), (base.detach() + h_w.detach()[_dev(hc, torch.int64)]) + d_w.detach()[_dev(dc, torch.int64)])
        w.backward(_dev(dout))
        for key, p, w32 in zip(("dbase", "dh_w", "dd_w"), (base, h_w, d_w), _loop_f32(dout, hc, dc, nh, nd)):
            assert _same_bits(p.grad, w32), key
    # gradients only where they are asked for
    frozen = _dev(tables[1])
    w = ops.edge_time_weights(base, frozen, d_w, _dev(h, torch.int64), _dev(d, torch.int64))
    g_base, g_d = torch.autograd.grad(w, (base, d_w), _dev(dout))
    assert torch.equal(g_base, base.grad) and torch.equal(g_d, d_w.grad) and frozen.grad is None
    # honours autocast like the other ops: float32 in and out, half-precision operands are cast back at the boundary
    with torch.autocast("cuda", dtype=torch.float16):
        wa = ops.edge_time_weights(base, h_w, d_w, _dev(h, torch.int64), _dev(d, torch.int64))
        wh = ops.edge_time_weights(base.detach().half(), h_w.detach().half(), d_w.detach().half(), _dev(h, torch.int64),
                                   _dev(d, torch.int64))
    assert wa.dtype == torch.float32 and torch.equal(wa, w) and wh.dtype == torch.float32
    with pytest.raises(ValueError, match="do not match"):
        ops.edge_time_weights(base, h_w, d_w[:, :-1], _dev(h, torch.int64), _dev(d, torch.int64))
    with pytest.raises(RuntimeError, match="differentiate twice"):
        w2 = ops.edge_time_weights(base, h_w, d_w, _dev(h, torch.int64), _dev(d, torch.int64))
        (g,) = torch.autograd.grad(w2, base, _dev(dout).requires_grad_(True), create_graph=True)
        g.sum().backward()


def test_hip_graph_replay_follows_new_indices():
    nnz, B, nh, nd = 2615, 32, 24, 7
    base, h_w, d_w = (torch.nn.Parameter(_dev(t)) for t in _tables(nnz, nh, nd, seed=8))
    params = (base, h_w, d_w)
    dout = _dev(np.random.default_rng(9).standard_normal((B, nnz)).astype(np.float32))
    pats = _index_patterns(B, nh, nd)
    H, D = _dev(pats["arange"][0], torch.int64), _dev(pats["arange"][1], torch.int64)
    out = torch.empty((B, nnz), device=DEV)

    def step():
        for p in params:
            p.grad.zero_()
        w = ops.edge_time_weights(base, h_w, d_w, H, D)
        out.copy_(w.detach())
        w.backward(dout)

    ops.edge_time_weights(base, h_w, d_w, H, D).backward(dout)          # the grads exist
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for name in ("one row", "out of range", "boundary rows"):
        H.copy_(_dev(pats[name][0], torch.int64))
        D.copy_(_dev(pats[name][1], torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [out.clone()] + [p.grad.clone() for p in params]
        step()
        torch.cuda.synchronize()
        for u, v in zip(replayed, [out] + [p.grad for p in params]):
            assert torch.equal(u, v), name
        for key, p, w32 in zip(("dbase", "dh_w", "dd_w"), params,
                               _loop_f32(dout.cpu().numpy(), pats[name][2], pats[name][3], nh, nd)):
            assert _same_bits(p.grad, w32), (name, key)


# ---- the model -------------------------------------------------------------------------------------------------------

N_NODES, N_EDGES, R, BATCH = 32, 40, 3, 8


def _dataset():
    from ms_gat_amd import data
    torch.manual_seed(0)
    return data.SyntheticPEMS(n_nodes=N_NODES, n_edges=N_EDGES, n_channels=1, in_hours=[1, 2, 3], batch_size=BATCH, days=2)


def _model(ds, learn, seed=0):
    from ms_gat_amd import model
    torch.manual_seed(seed)
    return model.msgat48(n_components=R, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                         learn_edge_weights=learn)


def _randomise_tables(net, seed=1, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
            t.copy_((torch.randn(t.shape, generator=g) * scale).to(t.device))


def _step(net, X, H, D, dY):
    net.zero_grad(set_to_none=True)
    out = net(X, H, D)
    (out * dY).sum().backward()
    return out.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def batch():
    ds = _dataset()
    X, H, D, Y = (t.to(DEV) for t in next(iter(ds.training)))
    dY = torch.randn(Y.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    return ds, X, H, D, dY


@pytest.mark.parametrize("stack", [True, False])
def test_fresh_time_model_is_the_static_model(batch, stack):
    """Zero tables: every sample's weights are the base, so the model computes what a `True` model with the same
    parameters computes -- through the per-sample path (B value sets) instead of one set: the bar of the per-sample tests
    against another route (assert_parity), not bits; whether the bits agree as well is printed."""
    ds, X, H, D, dY = batch
    static = _model(ds, True).to(DEV)
    timed = _model(ds, "time", seed=3)
    missing = timed.load_state_dict({k: v.cpu() for k, v in static.state_dict().items()}, strict=False)
    assert sorted(missing.missing_keys) == ["edge_d_ebd.weight", "edge_h_ebd.weight"]
    timed.to(DEV)
    static.stack_components = timed.stack_components = stack
    want, want_g = _step(static, X, H, D, dY)
    got, got_g = _step(timed, X, H, D, dY)
    what = f"time vs static, stacked={stack}"
    assert_parity(got, want, what, "out")
    assert set(got_g) == set(want_g) | {"edge_h_ebd.weight", "edge_d_ebd.weight"}
    gscale = max(float(v.abs().max()) for v in want_g.values())
    for k, v in want_g.items():
        if float(v.abs().max()) < 1e-2 * gscale:      # a near-cancelling scalar: judged on the scale of the largest gradient
            assert float((got_g[k] - v).abs().max()) < 1e-4 * 1e-2 * gscale, k
        else:
            assert_parity(got_g[k], v, what, k)
    print(f"{what}: out bit-equal {torch.equal(got, want)}; gradients that are not bit-equal: "
          f"{sorted(k for k in want_g if not torch.equal(got_g[k], want_g[k])) or 'none'}")
    # the table gradients at zero tables: what the samples of each hour / day contribute to the base's gradient
    assert float(got_g["edge_h_ebd.weight"].abs().max()) > 0
    assert_parity(got_g["edge_h_ebd.weight"].sum(0), got_g["edge_weight"], what, "sum of the hour rows = dbase")
    assert_parity(got_g["edge_d_ebd.weight"].sum(0), got_g["edge_weight"], what, "sum of the day rows = dbase")


@pytest.mark.parametrize("stack", [True, False])
def test_trained_state_equals_the_torch_op_formulation(batch, stack):
    """Random non-zero tables; the reference is the same model fed `ops.edge_adjacency(crow, col, (base + h[H]) + d[D])`
    formed by torch ops, whose gradients torch autograd sums."""
    ds, X, H, D, dY = batch
    net = _model(ds, "time").to(DEV)
    _randomise_tables(net)
    twin = copy.deepcopy(net)
    net.stack_components = twin.stack_components = stack
    got, got_g = _step(net, X, H, D, dY)
    twin.adjacency = lambda H, D: ops.edge_adjacency(
        twin.edge_crow, twin.edge_col, (twin.edge_weight + twin.edge_h_ebd.weight[H]) + twin.edge_d_ebd.weight[D])
    want, want_g = _step(twin, X, H, D, dY)
    assert torch.equal(got, want)
    what = f"time vs torch ops, stacked={stack}"
    for k in ("edge_weight", "edge_h_ebd.weight", "edge_d_ebd.weight"):
        assert float(want_g[k].abs().max()) > 0
        assert_parity(got_g[k], want_g[k], what, k)
    used = torch.zeros(24, dtype=torch.bool, device=DEV)
    used[H] = True
    assert torch.count_nonzero(got_g["edge_h_ebd.weight"][~used]) == 0      # rows no sample selected
    for k, v in want_g.items():
        if not k.startswith("edge_"):
            assert torch.equal(got_g[k], v), k                                # the same weights, the same kernels


def test_edge_time_embedding_feeds_a_gacn(batch):
    from ms_gat_amd import model
    ds, X, H, D, dY = batch
    csr = ds.adj.to_sparse_csr()
    emb = model.EdgeTimeEmbedding(csr.crow_indices(), csr.col_indices(), csr.values()).to(DEV)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        emb.h_ebd.weight.copy_(torch.randn(emb.h_ebd.weight.shape, generator=g) * 0.05)
        emb.d_ebd.weight.copy_(torch.randn(emb.d_ebd.weight.shape, generator=g) * 0.05)
    w = emb.weights(H, D)
    assert torch.equal(w, (emb.weight + emb.h_ebd(H)) + emb.d_ebd(D))
    adj = emb(H, D)
    assert adj.layout == torch.sparse_csr and tuple(adj.shape) == (BATCH, N_NODES, N_NODES)
    dense = torch.zeros(BATCH, N_NODES, N_NODES, device=DEV)
    rows = torch.repeat_interleave(torch.arange(N_NODES, device=DEV), emb.crow[1:] - emb.crow[:-1])
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
    assert_parity(got, want, "EdgeTimeEmbedding", "z")
    dw = dense.grad[:, rows, emb.col]                                         # [B,nnz]: the gradient at the weights
    assert_parity(emb.weight.grad, dw.double().sum(0).cpu().numpy(), "EdgeTimeEmbedding", "dweight")
    want_h = torch.zeros(24, dw.shape[1], dtype=torch.float64, device=DEV).index_add_(0, H, dw.double())
    assert_parity(emb.h_ebd.weight.grad, want_h.cpu().numpy(), "EdgeTimeEmbedding", "dh_ebd")


def test_attention_maps_follow_the_samples_own_weights(batch):
    ds, X, H, D, dY = batch
    net = _model(ds, "time").to(DEV)
    _randomise_tables(net, scale=0.2)
    with torch.no_grad():
        w = ops.edge_time_weights(net.edge_weight, net.edge_h_ebd.weight, net.edge_d_ebd.weight, H, D)     # [B,nnz]
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
            e, b = 7, 5                                        # one edge of one sample, spelled out
            assert abs(float(m[b, rows[e], cols[e]]) - float(att[b, rows[e], cols[e]]) * float(w[b, e])) <= \
                1e-5 * abs(float(want[b, e])) + 1e-6
            off = torch.ones(N_NODES, N_NODES, dtype=torch.bool, device=DEV)
            off[rows, cols] = False
            assert torch.count_nonzero(m[:, off]) == 0


# ---- the Trainer -----------------------------------------------------------------------------------------------------

def test_time_model_trains_eager_captured_and_auto(tmp_path):
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds, "time").to(DEV)
    twin, auto = copy.deepcopy(net), copy.deepcopy(net)
    w0 = net.edge_weight.detach().clone()
    batches = [b for _, b in zip(range(4), ds.training)]
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True)
    lazily = engine.Trainer(auto, 50.0, str(tmp_path / "auto"), hip_graph="auto")
    assert all(isinstance(t.optimizer, engine.FlatAdam) for t in (eager, graphed, lazily))
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        la = lazily.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        print(f"epoch {epoch}: loss eager {le!r}, captured {lg!r}, auto {la!r}")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
        assert abs(le - la) < 1e-4 * abs(le), (epoch, le, la)
    assert len(graphed._graphs) == 1 and len(lazily._graphs) == 1
    for name in ("edge_h_ebd.weight", "edge_d_ebd.weight"):
        assert float(net.get_parameter(name).detach().abs().max()) > 1e-4, name          # the tables leave zero
    assert (net.edge_weight.detach() - w0).abs().max() > 1e-4
    for other, tag in ((twin, "captured"), (auto, "auto")):
        worst = max((rel_err(q.detach().cpu(), p.detach().cpu()), n)
                    for (n, p), q in zip(net.named_parameters(), other.parameters()))
        print(f"{tag} vs eager: worst parameter {worst[1]} rel err {worst[0]:.3e}")
        for (name, p), q in zip(net.named_parameters(), other.parameters()):
            assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, (tag, name)
    X, H, D = (t.to(DEV) for t in batches[0][:3])
    net.stack_components = False                              # the per-component loop takes the same path
    with torch.no_grad():
        a = net(X, H, D)
        net.stack_components = True
        b = net(X, H, D)
    assert rel_err(a.cpu(), b.cpu()) < 1e-4


def test_time_model_trains_with_the_guard_and_a_null_value(tmp_path):
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds, "time").to(DEV)
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
        assert "horizons" in tr.last_stats
    assert len(graphed._graphs) == 1
    for name in ("edge_h_ebd.weight", "edge_d_ebd.weight"):
        assert float(net.get_parameter(name).detach().abs().max()) > 1e-4, name
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
