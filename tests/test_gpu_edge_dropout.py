"""GPU: edge dropout (msgat_edge_dropout{,_backward}, `ops.edge_dropout`, `model.EdgeDropout`, `MSGAT(edge_dropout=p)`).

The kernels through the C ABI against the numpy restatement of tests/edge_dropout_ref.py, bit for bit: the forward over
sizes either side of a quad and of a block, both weight forms, high words in seed and step, a sample offset, exempt edges;
the step bookkeeping; both backward forms; sharding invariance; a captured forward + backward whose replays draw steps
t, t+1, t+2.  The model: every `learn_edge_weights` on both evaluation paths against a twin fed `w * m_ref` through torch
ops, eval mode, the masked attention weights, the exempt diagonal.  The Trainer eager / captured / "auto".
"""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_parity, rel_err

import edge_dropout_ref as ref
import ms_gat_amd
from ms_gat_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SEED, STEP = (1 << 32) + 5, (1 << 32) + 3         # the high words of key and counter are exercised
NNZ = (1, 3, 4, 5, 255, 256, 257, 1027)
VS = (1, 2, 5, 33)
TILE = 64         # kEbSumSamples of csrc/edge_batch.hpp: the samples whose terms a block of a summing backward forms at a time
TILE_VS = (TILE, TILE + 1, 2 * TILE + 1)          # exactly a tile, a tile plus one, two tiles plus one
TILE_NNZ = (5, 65)                                # a partial quad; a second block that holds one edge
PS = (0.0, 0.1, 0.5, 0.9)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _state(seed=SEED, step=STEP):
    return torch.tensor([seed, step], dtype=torch.int64, device=DEV)


def _exempt(nnz):
    return (np.arange(nnz) % 3 == 0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _forward_abi(w, V, nnz, p, state, offset=0, exempt=None, advance=1):
    """(out pre-filled with NaN, used pre-filled with -1)"""
    thr, scale = ref.constants(p)
    out = torch.full((V, nnz), float("nan"), device=DEV)
    used = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    st = _lib.lib().msgat_edge_dropout(_ptr(w), _ptr(exempt), _ptr(state), _ptr(used), _ptr(out), V, nnz, int(w.dim() == 2),
                                       offset, thr, float(scale), advance, _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return out, used


def _backward_abi(dout, sets, V, nnz, p, state, used, offset=0, exempt=None):
    thr, scale = ref.constants(p)
    dw = torch.full((V, nnz) if sets else (nnz,), float("nan"), device=DEV)
    st = _lib.lib().msgat_edge_dropout_backward(_ptr(dout), _ptr(exempt), _ptr(state), _ptr(used), _ptr(dw), V, nnz, int(sets),
                                                offset, thr, float(scale), _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return dw


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32))


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nnz", NNZ)
def test_forward_has_the_bits_of_the_restatement(nnz):
    rng = np.random.default_rng(nnz)
    ex = _exempt(nnz)
    ex_t = _dev(ex, torch.uint8)
    for V in VS:
        w2 = rng.standard_normal((V, nnz)).astype(np.float32)
        for w in (w2[0], w2):
            w_t = _dev(w)
            for offset in (0, 7):
                for p in PS:
                    for exempt, exempt_t in ((None, None), (ex, ex_t)):
                        state = _state()
                        out, used = _forward_abi(w_t, V, nnz, p, state, offset, exempt_t)
                        want = ref.forward(w, SEED, STEP, V, p, offset, exempt)
                        assert _same_bits(out, want), (V, w.ndim, offset, p, exempt is not None)
                        assert used.tolist() == [STEP] and state.tolist() == [SEED, STEP + 1]
                        if p == 0.0:      # nothing dropped: the bits of the weights, broadcast
                            assert _same_bits(out, np.broadcast_to(w, (V, nnz)))


def test_step_bookkeeping():
    V, nnz, p = 5, 257, 0.5
    w = _dev(np.random.default_rng(1).standard_normal(nnz).astype(np.float32))
    state = _state(9, 40)
    a, used = _forward_abi(w, V, nnz, p, state, advance=0)
    assert used.tolist() == [40] and state.tolist() == [9, 40]           # advance = 0: the step stays
    b, used = _forward_abi(w, V, nnz, p, state, advance=0)
    assert torch.equal(a, b)                                              # and the same masks are drawn again
    c, used = _forward_abi(w, V, nnz, p, state)
    assert torch.equal(a, c) and used.tolist() == [40] and state.tolist() == [9, 41]
    d, used = _forward_abi(w, V, nnz, p, state)
    assert not torch.equal(c, d) and used.tolist() == [41] and state.tolist() == [9, 42]
    assert _same_bits(d, ref.forward(w.cpu().numpy(), 9, 41, V, p))
    # a negative seed is the same 64 bits read unsigned
    neg = _state(-3, 0)
    e, _ = _forward_abi(w, V, nnz, p, neg)
    assert _same_bits(e, ref.forward(w.cpu().numpy(), (1 << 64) - 3, 0, V, p))


@pytest.mark.parametrize("nnz", NNZ + tuple(n for n in TILE_NNZ if n not in NNZ))
def test_backward_forms_have_the_bits_of_the_restatement(nnz):
    rng = np.random.default_rng(100 + nnz)
    ex = _exempt(nnz)
    # 70: more samples than an LDS tile of the summing form holds; the tile's own edges at TILE_NNZ
    for V in (VS + (70,) if nnz in NNZ else ()) + (TILE_VS if nnz in TILE_NNZ else ()):
        dout = rng.standard_normal((V, nnz)).astype(np.float32)
        dout_t = _dev(dout)
        for p in (0.0, 0.1, 0.5, 0.9):
            for offset, exempt in ((0, None), (7, ex)):
                exempt_t = None if exempt is None else _dev(exempt, torch.uint8)
                state, used = _state(SEED, 12345), _state(STEP, 0)[:1].clone()      # backward reads `used`, not the step
                m = ref.multipliers(SEED, STEP, V, nnz, p, offset, exempt)
                got = _backward_abi(dout_t, True, V, nnz, p, state, used, offset, exempt_t)
                assert _same_bits(got, ref.backward_sets(dout, m)), ("sets", V, p, offset)
                assert torch.equal(got, dout_t * _dev(m))                           # the torch expression
                got = _backward_abi(dout_t, False, V, nnz, p, state, used, offset, exempt_t)
                assert bool(torch.isfinite(got).all())                              # every entry written
                assert _same_bits(got, ref.backward_shared(dout, m)), ("shared", V, p, offset)
                assert state.tolist() == [SEED, 12345] and used.tolist() == [STEP]


def test_two_forwards_then_their_two_backwards_see_their_own_masks():
    V, nnz, p = 5, 1027, 0.5
    rng = np.random.default_rng(2)
    w = _dev(rng.standard_normal(nnz).astype(np.float32)).requires_grad_(True)
    w2 = _dev(rng.standard_normal((V, nnz)).astype(np.float32)).requires_grad_(True)
    dout = rng.standard_normal((V, nnz)).astype(np.float32)
    state = ops.edge_dropout_state(31, DEV)
    a = ops.edge_dropout(w, p, state, samples=V)                  # step 0
    b = ops.edge_dropout(w2, p, state)                            # step 1
    assert state.tolist() == [31, 2]
    assert a.shape == (V, nnz) and a.is_contiguous() and a.dtype == torch.float32
    assert _same_bits(a.detach(), ref.forward(w.detach().cpu().numpy(), 31, 0, V, p))
    assert _same_bits(b.detach(), ref.forward(w2.detach().cpu().numpy(), 31, 1, V, p))
    (ga,) = torch.autograd.grad(a, w, _dev(dout))
    (gb,) = torch.autograd.grad(b, w2, _dev(dout))
    assert _same_bits(ga, ref.backward_shared(dout, ref.multipliers(31, 0, V, nnz, p)))
    assert _same_bits(gb, ref.backward_sets(dout, ref.multipliers(31, 1, V, nnz, p)))
    assert state.tolist() == [31, 2]                              # backward moves nothing
    # a weight without a gradient: no backward node; bool exempt flags; p = 0 still runs and advances
    frozen = w.detach()
    ex = torch.zeros(nnz, dtype=torch.bool, device=DEV)
    ex[::2] = True
    c = ops.edge_dropout(frozen, 0.0, state, samples=2, exempt=ex, sample_offset=3)
    assert not c.requires_grad and torch.equal(c, frozen.expand(2, nnz)) and state.tolist() == [31, 3]
    d = ops.edge_dropout(frozen, 0.9, state, samples=2, exempt=ex)
    assert state.tolist() == [31, 4] and torch.equal(d[:, ::2], frozen[::2].expand(2, -1))
    with pytest.raises(RuntimeError, match="differentiate twice"):
        out = ops.edge_dropout(w, p, state, samples=V)
        (g,) = torch.autograd.grad(out, w, _dev(dout).requires_grad_(True), create_graph=True)
        g.sum().backward()


def test_null_outputs_and_empty_sizes_write_nothing():
    L, s = _lib.lib(), _lib.stream_handle(DEV)
    thr, scale = ref.constants(0.5)
    one = torch.zeros(4, device=DEV)
    state, used = _state(1, 6), torch.full((1,), -1, dtype=torch.int64, device=DEV)
    p = one.data_ptr()
    for V, nnz in ((0, 9), (4, 0)):
        assert L.msgat_edge_dropout(p, None, state.data_ptr(), used.data_ptr(), p, V, nnz, 0, 0, thr, float(scale), 1, s) == 0
        assert L.msgat_edge_dropout_backward(p, None, state.data_ptr(), used.data_ptr(), p, V, nnz, 0, 0, thr, float(scale), s) == 0
    dout = torch.ones(2, 2, device=DEV)
    assert L.msgat_edge_dropout_backward(dout.data_ptr(), None, state.data_ptr(), used.data_ptr(), None, 2, 2, 1, 0, thr,
                                         float(scale), s) == 0
    torch.cuda.synchronize()
    # an empty forward draws nothing: `used` is not written and the step does not move
    assert not one.cpu().numpy().view(np.int32).any() and state.tolist() == [1, 6] and used.tolist() == [-1]
    # the op on an empty batch / an empty pattern
    w = torch.ones(5, device=DEV, requires_grad=True)
    out = ops.edge_dropout(w, 0.5, state, samples=0)
    assert out.shape == (0, 5)
    out.sum().backward()
    assert torch.count_nonzero(w.grad) == 0 and state.tolist() == [1, 6]


@pytest.mark.parametrize("V,nnz", [(7, 257), (33, 1027)])
def test_rows_of_a_draw_are_the_shards_draw_at_its_offset(V, nnz):
    p = 0.5
    rng = np.random.default_rng(V)
    w2 = _dev(rng.standard_normal((V, nnz)).astype(np.float32))
    dout = _dev(rng.standard_normal((V, nnz)).astype(np.float32))
    for w in (w2[0].contiguous(), w2):
        whole, used = _forward_abi(w, V, nnz, p, _state())
        g_whole = _backward_abi(dout, True, V, nnz, p, _state(), used)
        for world in (2, 3):
            for rank in range(world):
                lo, hi = ms_gat_amd.parallel.shard_bounds(V, rank, world)
                part, used_r = _forward_abi(w if w.dim() == 1 else w[lo:hi].contiguous(), hi - lo, nnz, p, _state(), offset=lo)
                assert torch.equal(part, whole[lo:hi]), (world, rank)
                g = _backward_abi(dout[lo:hi].contiguous(), True, hi - lo, nnz, p, _state(), used_r, offset=lo)
                assert torch.equal(g, g_whole[lo:hi]), (world, rank)


def test_hip_graph_replays_draw_consecutive_steps():
    V, nnz, p, t0 = 32, 2615, 0.1, (1 << 32) - 2            # the step's low word wraps during the replays
    rng = np.random.default_rng(5)
    w = torch.nn.Parameter(_dev(rng.standard_normal(nnz).astype(np.float32)))
    w2 = torch.nn.Parameter(_dev(rng.standard_normal((V, nnz)).astype(np.float32)))
    dout_np = rng.standard_normal((V, nnz)).astype(np.float32)
    dout = _dev(dout_np)
    ex_np = _exempt(nnz)
    ex = _dev(ex_np, torch.uint8)
    state = ops.edge_dropout_state(SEED, DEV)
    outs = [torch.empty((V, nnz), device=DEV) for _ in range(2)]

    def step():
        for q in (w, w2):
            q.grad.zero_()
        a = ops.edge_dropout(w, p, state, samples=V, exempt=ex)            # step t
        b = ops.edge_dropout(w2, p, state, sample_offset=7)                # step t + 1
        outs[0].copy_(a.detach())
        outs[1].copy_(b.detach())
        (a + b).backward(dout)

    def check(t):
        torch.cuda.synchronize()
        assert _same_bits(outs[0], ref.forward(w.detach().cpu().numpy(), SEED, t, V, p, 0, ex_np)), t
        assert _same_bits(outs[1], ref.forward(w2.detach().cpu().numpy(), SEED, t + 1, V, p, 7)), t
        assert _same_bits(w.grad, ref.backward_shared(dout_np, ref.multipliers(SEED, t, V, nnz, p, 0, ex_np))), t
        # autograd ADDS into the zeroed .grad: (+0) + dout * m, which turns the -0 of a dropped edge under a negative dout into +0
        want2 = np.zeros((V, nnz), np.float32) + ref.backward_sets(dout_np, ref.multipliers(SEED, t + 1, V, nnz, p, 7))
        assert _same_bits(w2.grad, want2), t

    w.grad, w2.grad = torch.zeros_like(w), torch.zeros_like(w2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                              # the warm-up draws too
    torch.cuda.current_stream().wait_stream(s)
    with torch.no_grad():
        state.copy_(torch.tensor([SEED, t0]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    assert state.tolist() == [SEED, t0]                     # the capture itself executes nothing
    for i in range(3):                                      # each replay is two draws: steps t, t + 2, t + 4
        graph.replay()
        check(t0 + 2 * i)
        assert state.tolist() == [SEED, t0 + 2 * i + 2]
    step()                                                  # an eager step continues where the replays stopped
    check(t0 + 6)
    assert state.tolist() == [SEED, t0 + 8]


# ---- the model -------------------------------------------------------------------------------------------------------

N_NODES, N_EDGES, R, BATCH = 32, 40, 3, 8
LEARN = [False, True, "time", "signal"]
P_MODEL, SEED_MODEL = 0.25, 77


def _dataset():
    from ms_gat_amd import data
    torch.manual_seed(0)
    return data.SyntheticPEMS(n_nodes=N_NODES, n_edges=N_EDGES, n_channels=1, in_hours=[1, 2, 3], batch_size=BATCH, days=2)


def _model(ds, learn, seed=0, **kwargs):
    from ms_gat_amd import model
    torch.manual_seed(seed)
    net = model.msgat48(n_components=R, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                        learn_edge_weights=learn, **kwargs)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                        # every sample its own weights
        if learn == "time":
            for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
                t.copy_(torch.randn(t.shape, generator=g) * 0.05)
        if learn == "signal":
            half = net.edge_proj.weight[net.edge_rank:]
            half.copy_(torch.randn(half.shape, generator=g) * 0.05)
    return net


def _pattern(ds):
    csr = ds.adj.to_sparse_csr()
    crow, col = csr.crow_indices(), csr.col_indices()
    rows = torch.repeat_interleave(torch.arange(N_NODES), crow[1:] - crow[:-1])
    return crow.to(DEV), col.to(DEV), rows.to(DEV), (rows == col).numpy()


def _weights_by_torch(net, H, D, X):
    """[nnz] or [B,nnz]: the weights before the mask, from torch ops where the package forms them with torch ops or one
    fused launch whose bits are those of the torch expression ("time"); "signal" through its own op."""
    learn = net.learn_edge_weights
    if learn is False:
        at = net.adj.detach().cpu().to_sparse_csr()
        rows = torch.repeat_interleave(torch.arange(N_NODES), at.crow_indices()[1:] - at.crow_indices()[:-1])
        return net.adj.detach()[rows.to(DEV), at.col_indices().to(DEV)]
    if learn is True:
        return net.edge_weight
    if learn == "time":
        return (net.edge_weight + net.edge_h_ebd.weight[H]) + net.edge_d_ebd.weight[D]
    return ops.edge_signal_weights(net.edge_weight, net.edge_proj(net.edge_features(X)), net.edge_crow, net.edge_col)


def _twin(net, crow, col, m_ref):
    """`net`'s parameters with edge_dropout = 0 and the adjacency formed as `edge_adjacency(crow, col, w_torch * m_ref)`."""
    twin = copy.deepcopy(net)
    twin.edge_dropout = 0.0

    def adjacency(H=None, D=None, X=None):
        w = _weights_by_torch(twin, H, D, X)
        return ops.edge_adjacency(crow, col, (w if w.dim() == 2 else w[None, :]) * m_ref)
    twin.adjacency = adjacency
    twin.batch_adjacency = lambda X, H, D: adjacency(H, D, X)
    return twin


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
@pytest.mark.parametrize("learn", LEARN)
def test_model_equals_its_twin_fed_the_restatements_mask(batch, learn, stack):
    ds, X, H, D, dY = batch
    crow, col, rows, diag = _pattern(ds)
    nnz = col.numel()
    net = _model(ds, learn, edge_dropout=P_MODEL, edge_dropout_seed=SEED_MODEL).to(DEV)
    plain = _model(ds, learn).to(DEV)
    plain.load_state_dict(net.state_dict())
    net.stack_components = plain.stack_components = stack
    # eval mode: the bits of the model without dropout, nothing drawn
    net.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(net(X, H, D), plain(X, H, D))
    net.attention_maps(X, H, D)
    assert net.edge_dropout_state() == {"seed": SEED_MODEL, "step": 0}
    net.train()
    with torch.no_grad():                                   # training mode under no_grad draws nothing either
        assert torch.equal(net(X, H, D), plain.train()(X, H, D))
    assert net.edge_dropout_state() == {"seed": SEED_MODEL, "step": 0}
    # training mode, two steps: the model's own offset and step
    net.edge_dropout_sample_offset = 5
    what = f"edge dropout, learn={learn!r}, stacked={stack}"
    for step in (0, 1):
        m_np = ref.multipliers(SEED_MODEL, step, BATCH, nnz, P_MODEL, sample_offset=5, exempt=diag)
        assert (m_np == 0).any() and (m_np[:, diag] == 1).all()
        twin = _twin(net, crow, col, _dev(m_np))
        twin.stack_components = stack
        got, got_g = _step(net, X, H, D, dY)
        want, want_g = _step(twin, X, H, D, dY)
        assert net.edge_dropout_state() == {"seed": SEED_MODEL, "step": step + 1}
        assert torch.equal(got, want), (what, step)
        assert set(got_g) == set(want_g)
        edge_keys = [k for k in want_g if k.startswith("edge_")]
        assert bool(edge_keys) == bool(learn)
        for k, v in want_g.items():
            if k in edge_keys:
                assert float(v.abs().max()) > 0, k
                assert_parity(got_g[k], v, what, f"{k} step {step}")
            else:
                assert torch.equal(got_g[k], v), (what, step, k)     # the same weights, the same kernels
    assert not torch.equal(got, plain(X, H, D))                          # and the masks do change the forecast


@pytest.mark.parametrize("stack", [True, False])
def test_a_dropped_edge_contributes_exactly_zero_and_the_diagonal_is_never_dropped(batch, stack):
    ds, X, H, D, dY = batch
    crow, col, rows, diag = _pattern(ds)
    nnz = col.numel()
    net = _model(ds, "time", edge_dropout=0.5, edge_dropout_seed=3).to(DEV).train()
    net.stack_components = stack
    diag_t = torch.from_numpy(diag).to(DEV)
    for step in range(8):
        with ops.collect_weights("masked") as seen:
            net(X, H, D)
        dropped = torch.from_numpy(ref.dropped(3, step, BATCH, nnz, 0.5, exempt=diag)).to(DEV)
        assert dropped.any() and not dropped[:, diag_t].any()
        entries = [ops.weights_of(e, "masked", (BATCH,), slice(r * BATCH, (r + 1) * BATCH)) for e in seen for r in range(R)] \
            if stack else [ops.weights_of(e, "masked", (BATCH,)) for e in seen]
        assert len(entries) == R * 2
        for m in entries:
            at_edges = m.detach().to_dense()[:, rows, col]                # [B,nnz]
            assert torch.count_nonzero(at_edges[dropped]) == 0            # exactly zero, sample by sample
            assert torch.count_nonzero(at_edges[~dropped]) > 0.9 * int((~dropped).sum())
            assert torch.count_nonzero(at_edges[:, diag_t]) == BATCH * int(diag.sum())    # the +I is never zeroed
    assert net.edge_dropout_state() == {"seed": 3, "step": 8}
    # keep_self=False: the diagonal is drawn like every other edge
    bare = _model(ds, "time", edge_dropout=0.5, edge_dropout_seed=3, edge_dropout_keep_self=False).to(DEV).train()
    adj = bare.adjacency(H, D)
    assert torch.count_nonzero(adj.values()[:, diag_t]) < BATCH * int(diag.sum())


def test_edge_dropout_module_feeds_a_gacn(batch):
    from ms_gat_amd import model
    ds, X, H, D, dY = batch
    crow, col, rows, diag = _pattern(ds)
    nnz = col.numel()
    values = ds.adj.to_sparse_csr().values().to(DEV).requires_grad_(True)
    drop = model.EdgeDropout(0.5, seed=9, exempt=torch.from_numpy(diag)).to(DEV)
    assert drop.edge_drop_state.device.type == "cuda" and drop.state_dict() == {}
    gacn = ms_gat_amd.GACN(3, 24, 12).to(DEV)
    with torch.no_grad():
        for q in gacn.parameters():
            q.normal_(0, 0.3)
    x = torch.randn(BATCH, 3, N_NODES, 12, device=DEV)
    w = drop(values, samples=BATCH)
    assert _same_bits(w.detach(), ref.forward(values.detach().cpu().numpy(), 9, 0, BATCH, 0.5, exempt=diag))
    z = gacn(x, ops.edge_adjacency(crow, col, w))
    z.sum().backward()
    assert values.grad is not None and float(values.grad.abs().max()) > 0 and drop.state() == {"seed": 9, "step": 1}
    drop.eval()
    assert drop(values, samples=BATCH) is values and drop.state() == {"seed": 9, "step": 1}
    drop.set_state({"seed": 9, "step": 0})
    assert torch.equal(drop.train()(values, samples=BATCH), w)


# ---- the Trainer -----------------------------------------------------------------------------------------------------

def _train_three_ways(tmp_path, learn, **kwargs):
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds, learn, edge_dropout=0.2, edge_dropout_seed=13).to(DEV)
    twin, auto = copy.deepcopy(net), copy.deepcopy(net)
    batches = [b for _, b in zip(range(4), ds.training)]
    val = [b for _, b in zip(range(2), ds.validation)]
    trainers = [engine.Trainer(m, 50.0, str(tmp_path / tag), hip_graph=hg, **kwargs)
                for m, tag, hg in ((net, "eager", False), (twin, "graph", True), (auto, "auto", "auto"))]
    for epoch in (1, 2):
        losses = [t.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train") for t in trainers]
        print(f"learn={learn!r} epoch {epoch}: loss eager {losses[0]!r}, captured {losses[1]!r}, auto {losses[2]!r}")
        for other in losses[1:]:
            assert abs(losses[0] - other) < 1e-4 * abs(losses[0]), (epoch, losses)
        positions = [m.edge_dropout_state()["step"] for m in (net, twin, auto)]
        assert positions == [4 * epoch] * 3, positions
        for t in trainers:                       # a validation epoch draws nothing
            t.run_epoch(val, gpu_id=0, epoch=epoch, mode="validate")
        assert [m.edge_dropout_state()["step"] for m in (net, twin, auto)] == positions
    assert [m.edge_dropout_state() for m in (net, twin, auto)] == [{"seed": 13, "step": 8}] * 3
    assert sum(1 for k in trainers[1]._graphs if k[0]) == 1 and sum(1 for k in trainers[2]._graphs if k[0]) == 1
    for other, tag in ((twin, "captured"), (auto, "auto")):
        worst = max((rel_err(q.detach().cpu(), p.detach().cpu()), n)
                    for (n, p), q in zip(net.named_parameters(), other.parameters()))
        print(f"{tag} vs eager: worst parameter {worst[1]} rel err {worst[0]:.3e}")
        for (name, p), q in zip(net.named_parameters(), other.parameters()):
            assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, (tag, name)
    return trainers


@pytest.mark.parametrize("learn", [False, "time"])
def test_dropout_model_trains_eager_captured_and_auto(tmp_path, learn):
    trainers = _train_three_ways(tmp_path, learn)
    # the checkpoint carries the stream: a fresh trainer continues at step 8
    from ms_gat_amd import engine
    trainers[1].save(tmp_path / "ck.pkl")
    fresh = _model(_dataset(), learn, edge_dropout=0.2, edge_dropout_seed=0).to(DEV)
    engine.Trainer(fresh, 50.0, str(tmp_path / "fresh"), hip_graph=False).load(tmp_path / "ck.pkl")
    assert fresh.edge_dropout_state() == {"seed": 13, "step": 8}


def test_dropout_model_trains_with_the_guard_and_a_null_value(tmp_path):
    trainers = _train_three_ways(tmp_path, True, null_value=0.0, max_grad_norm=0.25, skip_nonfinite=True)
    for tr in trainers:
        assert tr.last_stats is not None
