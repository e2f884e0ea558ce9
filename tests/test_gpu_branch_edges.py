"""GPU: the channel and temporal branches of a MEAM block at their numerical and shape edges, held to what the graph
branch is held to (test_gpu_score_edges.py, test_gpu_group_counts.py): the float64 restatement of the same op sequence
under the per-entry parity bar (conftest.assert_parity).

A  the two small softmaxes (csrc/smallatt.hip) at large scores, saturated scores, magnitudes far from one, tied and
   zero rows -- through ops.channel_attention_mix and ops.temporal_attention_taps;
B  the trip boundaries of the node loops: the temporal attention's tiles of 128 nodes and trips of 1024 lanes, the pools'
   64 / 256 nodes and 16 channels, k_tmix / k_tmix_dA with one matrix pair per sample at T = 4, 8, 16;
C  a whole block at T_in = 4, 8, 16, every registry width, below, at and above the 512 positions from which the
   one-pass channel-mixing forms run, and both schedules of msgat72 at those T_in;
D  the channel attention beyond the LDS of its kernels: what the C ABI returns there, and that a block of that width
   trains.

Cases, inputs and restatements: branch_edge_fixtures.py; test_branch_edges_cpu.py shows, without a GPU, that the
restatements evaluated in fp32 meet every bar applied here."""
import functools

import pytest
import torch

from conftest import assert_parity, record_err, rel_err
from oracle import dense_torch

import branch_edge_fixtures as fx
from ms_gat_amd import _lib, model, ops
from test_gpu_branches import _GradArrivesAsSlice

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "branch_edges"
TOL = 1e-4


def _channel(case, **kw):
    p, Wc, conv, dMc = fx.channel_inputs(case, **kw)
    return (p, Wc, conv), dMc, fx.channel_attention_mix_dense, ops.channel_attention_mix, ("Mc", "dpooled", "dWc", "dconv")


def _temporal(case, **kw):
    q, W1, W2, dtaps = fx.temporal_inputs(case, **kw)
    dil = case[5]
    return ((q, W1, W2), dtaps, lambda a, b, c: fx.temporal_attention_taps_dense(a, b, c, dil),
            lambda a, b, c: ops.temporal_attention_taps(a, b, c, dil), ("taps", "dpooled", "dWt1", "dWt2"))


OPS = [(_channel, c) for c in fx.CHANNEL_CASES] + [(_temporal, c) for c in fx.TEMPORAL_CASES]
IDS = [f"{b.__name__[1:]}{c}".replace(" ", "") for b, c in OPS]


def _ours(fn, inputs, cotangent):
    """(output, gradients at every input) of the library's op"""
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    got = [out.detach()] + list(torch.autograd.grad(out, leaves, cotangent.to(DEV)))
    torch.cuda.synchronize()
    for t in got:
        assert bool(torch.isfinite(t).all())
    return got


def _all_parity(got, want, names, key):
    for name, a, b in zip(names, got, want):
        assert_parity(a, b, WHAT, f"{key}:{name}")


# ---- A: score edges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_large_scores_against_the_fp32_op_sequence(build, case):
    """Scores of 70 .. 280, about half the rows one-hot: a softmax without its running max, or an `att` re-created
    differently in the backward, shows here.  Outputs under the parity bar; no gradient further from float64 than 3 x the
    distance of the same op sequence in fp32 (or the usual 1e-4: test_branch_edges_cpu.py shows it is 1e-4 throughout)."""
    inputs, cot, dense, fused, names = build(case, scale=fx.LARGE)
    got = _ours(fused, inputs, cot)
    want, ref32 = fx.evaluate(dense, inputs, cot, torch.float64), fx.evaluate(dense, inputs, cot, torch.float32)
    key = f"large {IDS[OPS.index((build, case))]}"
    assert_parity(got[0], want[0], WHAT, f"{key}:{names[0]}")
    for name, a, b, r in zip(names[1:], got[1:], want[1:], ref32[1:]):
        bar = max(TOL, 3.0 * rel_err(r, b))
        e = rel_err(a, b)
        record_err(WHAT, f"{key}:{name}", e, bar)
        assert e < bar, (name, e, bar)


@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_saturated_scores_stay_finite_and_accurate(build, case):
    """Scores of ~1e4: every row one-hot.  Outputs under the parity bar.  The gradients are what is left of
    dS = att d - <d, att> att when its two terms cancel; they are held to 1e-5 of the size of those terms carried through
    the products that follow (the float64 oracle supplies it), as test_gpu_score_edges.py holds dWg and dalpha."""
    inputs, cot, dense, fused, names = build(case, scale=fx.SATURATED)
    got = _ours(fused, inputs, cot)
    want = fx.evaluate(dense, inputs, cot, torch.float64)
    key = f"saturated {IDS[OPS.index((build, case))]}"
    assert_parity(got[0], want[0], WHAT, f"{key}:{names[0]}")
    terms = (fx.channel_cancelling_terms(*inputs, cot) if build is _channel else
             fx.temporal_cancelling_terms(*inputs, cot, case[5]))
    assert list(terms) == list(names[1:])
    for (name, s), a, b in zip(terms.items(), got[1:], want[1:]):
        err = float((a.cpu().double() - b).abs().max())
        record_err(WHAT, f"{key}:{name} / cancelling terms", err / float(s), 1e-5)
        assert err <= 1e-5 * float(s), (name, err, float(s))


@pytest.mark.parametrize("cq,cg", fx.MAGNITUDES)
@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_magnitudes_far_from_one(build, case, cq, cg):
    """Pooled signals of magnitude cq with Wc / cq^2 (Wt1, Wt2 / cq each), so that the scores stay at unit scale;
    cotangents of magnitude cg."""
    inputs, cot, dense, fused, names = build(case, cq=cq, cg=cg)
    _all_parity(_ours(fused, inputs, cot), fx.evaluate(dense, inputs, cot, torch.float64), names,
                f"magnitudes {IDS[OPS.index((build, case))]} q~{cq:g} g~{cg:g}")


@pytest.mark.parametrize("structure", ["twins", "zero"])
@pytest.mark.parametrize("build,case", [OPS[0], OPS[len(fx.CHANNEL_CASES)]], ids=["channel", "temporal"])
def test_tied_and_zero_rows(build, case, structure):
    """Two identical pooled rows (two identical rows of the map, equal scores inside every row) and an all-zero one (a
    uniform row)."""
    inputs, cot, dense, fused, names = build(case, structure=structure)
    _all_parity(_ours(fused, inputs, cot), fx.evaluate(dense, inputs, cot, torch.float64), names,
                f"{structure} {build.__name__[1:]}")


# ---- B: trip boundaries --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", fx.TEMPORAL_TRIP_N)
def test_temporal_attention_at_the_trips_of_its_node_loops(N):
    """T = 12, R = 2: k_tempatt_fwd's double-buffered tiles of 128 nodes (the last trip prefetches its own tile again),
    k_tempatt_bwd's trips of 1024 lanes (1025: the second, 2049: the third)."""
    inputs, cot, dense, fused, names = _temporal((2, 1, N, 10, 12, 2))
    _all_parity(_ours(fused, inputs, cot), fx.evaluate(dense, inputs, cot, torch.float64), names, f"trips temporal N={N}")


def _pool_check(N, C, T, sliced):
    x, w, alpha, dpn, dpc = fx.pool_inputs(N, C, T)
    key = f"trips pools N={N} C={C} T={T}" + (" sliced" if sliced else "")
    for name, weights, cot, fused, dense in (("node_pool", w, dpn, ops.node_pool, fx.node_pool_dense),
                                             ("channel_pool", alpha, dpc, ops.channel_pool, fx.channel_pool_dense)):
        want = fx.evaluate(dense, (x, weights), cot, torch.float64)
        wl = weights.to(DEV).requires_grad_(True)
        if sliced:   # the input is channels 2 .. 2 + C of a wider tensor; the others must never be read
            wide = torch.full((x.shape[0], C + 5, N, T), float("nan"))
            wide[:, 2:2 + C] = x
            leaf = wide.to(DEV).requires_grad_(True)
            xin = leaf[:, 2:2 + C]
        else:
            leaf = xin = x.to(DEV).requires_grad_(True)
        out = fused(xin, wl)
        dx, dw = torch.autograd.grad(out, [leaf, wl], cot.to(DEV))
        if sliced:
            assert not bool(dx[:, :2].any()) and not bool(dx[:, 2 + C:].any())
            dx = dx[:, 2:2 + C]
        _all_parity([out.detach(), dx, dw], want, ("out", "dx", "dweights"), f"{key} {name}")


@pytest.mark.parametrize("N,C,T", fx.POOL_CASES)
def test_pools_at_the_trips_of_their_node_and_channel_loops(N, C, T):
    """ops.node_pool (256 nodes per trip forward, per block backward; 16 channels per block of the weight gradient) and
    ops.channel_pool with R = 2 parameter sets: forward, input gradient, weight gradient."""
    _pool_check(N, C, T, sliced=False)


def test_pools_read_a_channel_slice_whose_neighbours_are_nan():
    _pool_check(*fx.POOL_SLICE_CASE, sliced=True)


def _time_mix_check(T, Co, N, sliced):
    y, A, bias, dout = fx.time_mix_inputs(T, Co, N)
    want = fx.evaluate(fx.time_mix_dense, (y, A, bias), dout, torch.float64)
    fused = (lambda a, b, c: _GradArrivesAsSlice.apply(ops.time_mix(a, b, c))) if sliced else ops.time_mix
    _all_parity(_ours(fused, (y, A, bias), dout), want, ("out", "dy", "dA", "dbias"),
                f"trips time_mix T={T} Co={Co} N={N}" + (" sliced" if sliced else ""))


@pytest.mark.parametrize("T,Co,N", fx.TIME_MIX_CASES)
def test_time_mix_with_a_matrix_pair_per_sample(T, Co, N):
    """K = 2, bias per relation, R = 2: k_tmix<T,2,.> and k_tmix_dA<T> at T = 16 (no column mask), T = 4 (a 4 x 4 corner
    of the MFMA tile) and T = 8; Co N < 4 leaves chunks of k_tmix_dA without a row."""
    _time_mix_check(T, Co, N, sliced=False)


def test_time_mix_gradient_arriving_as_a_channel_slice():
    _time_mix_check(*fx.TIME_MIX_SLICE_CASE, sliced=True)


# ---- C: the whole block at every T_in -----------------------------------------------------------------------------------

@pytest.mark.parametrize("T,N", fx.MEAM_SHAPES)
@pytest.mark.parametrize("Ci,Co,dilations", fx.MEAM_BLOCKS)
def test_meam_block_at_every_t_in(Ci, Co, dilations, T, N):
    """model.MEAM forward and backward against dense_torch.meam_dense in float64 with the ReLU mask the library's own
    output shows: output, dx and every parameter gradient."""
    block, x, dout, adj = fx.meam_problem(Ci, Co, dilations, T, N)
    block.to(DEV)
    xl = x.to(DEV).requires_grad_(True)
    out = block(xl, adj.to(DEV))
    params = dict(block.named_parameters())
    grads = torch.autograd.grad(out, [xl] + list(params.values()), dout.to(DEV))
    got = dict(zip(["out", "dx"] + list(params), [out.detach()] + list(grads)))
    want = fx.meam_reference(block.state_dict(), x.to(DEV), dout, adj, dilations, out.detach() > 0, torch.float64)
    assert set(want) == set(got)
    key = f"meam {Ci}->{Co} {dilations} T={T} N={N}".replace(" ", "")
    for k in got:
        assert_parity(got[k], want[k], WHAT, f"{key}:{k}")


@functools.lru_cache(maxsize=None)
def _stacked_case(T, N):
    """the model on the device, its inputs, and the float64 restatement -- once for both schedules"""
    net, X, H, D, dout = fx.stacked_problem(T, N)
    net.to(DEV)
    X, H, D, dout = (t.to(DEV) for t in (X, H, D, dout))
    return net, X, H, D, dout, fx.msgat_reference(net, X, H, D, dout, torch.float64)


@pytest.mark.parametrize("stack", [True, False], ids=["stacked", "loop"])
@pytest.mark.parametrize("T,N", fx.STACKED_CASES)
def test_msgat72_schedules_at_every_t_in(T, N, stack):
    """Both schedules of msgat72 (R = 2, three input channels) against the whole-model restatement in float64: the
    prediction and every gradient at the max-norm bar of test_whole_model_matches_the_dense_op_sequence (ReLU masks cannot
    be pinned through two blocks; the restatement in fp32 stays under a quarter of it: test_branch_edges_cpu.py)."""
    net, X, H, D, dout, (pred64, g64) = _stacked_case(T, N)
    net.stack_components = stack
    pred = net(X, H, D)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(pred, [p for p in net.parameters() if p.requires_grad], dout)
    key = f"msgat72 {'stacked' if stack else 'loop'} T={T} N={N}"
    assert set(names) == set(g64)
    for k, a, b in [("pred", pred, pred64)] + [(n, g, g64[n]) for n, g in zip(names, grads)]:
        e = rel_err(a, b)
        record_err(WHAT, f"{key}:{k}", e, TOL)
        assert e < TOL, (k, e)


# ---- D: channel attention beyond its LDS envelope ----------------------------------------------------------------------

def _chanatt_statuses(C, cb, T, G=2):
    """(status of msgat_channel_attention_forward, of _backward) through the C ABI"""
    L = _lib.lib()
    gen = torch.Generator().manual_seed(C)
    p, Wc, conv, dMc = (torch.randn(*s, generator=gen).to(DEV) for s in ((G, C, T), (1, T, T), (1, cb, C), (G, cb, C)))
    att, Mc = torch.zeros(G, C, C, device=DEV), torch.zeros(G, cb, C, device=DEV)
    dp, dWc, dconv = torch.zeros_like(p), torch.zeros_like(Wc), torch.zeros_like(conv)
    part = torch.zeros(max(int(L.msgat_channel_attention_partial_floats(G, C, cb, T)), 1), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    fwd = L.msgat_channel_attention_forward(p.data_ptr(), Wc.data_ptr(), conv.data_ptr(), att.data_ptr(), Mc.data_ptr(),
                                            G, 1, C, cb, T, stream)
    bwd = L.msgat_channel_attention_backward(dMc.data_ptr(), att.data_ptr(), p.data_ptr(), Wc.data_ptr(), conv.data_ptr(),
                                             dp.data_ptr(), dWc.data_ptr(), dconv.data_ptr(), part.data_ptr(), G, 1, C, cb,
                                             T, stream)
    torch.cuda.synchronize()
    return fwd, bwd


def test_channel_attention_entry_points_at_the_edge_of_their_lds():
    """(114, 38, 12) runs both ways; at (117, 39, 12) the forward runs and the backward refuses; the restated byte
    formulas and msgat_channel_attention_fused say the same."""
    unsupported = -3     # MSGAT_ERR_UNSUPPORTED (include/msgat_hip.h)
    assert _chanatt_statuses(114, 38, 12) == (_lib.MSGAT_OK, _lib.MSGAT_OK)
    assert _chanatt_statuses(117, 39, 12) == (_lib.MSGAT_OK, unsupported)
    assert fx.chanatt_fits(114, 38, 12) == (True, True) and fx.chanatt_fits(117, 39, 12) == (True, False)
    assert ops.channel_attention_fused(114, 38, 12) and not ops.channel_attention_fused(117, 39, 12)
    C, cb, _, T = fx.WIDE
    assert fx.chanatt_fits(C, cb, T) == (True, False) and not ops.channel_attention_fused(C, cb, T)
    # the op itself refuses such a width before its forward, not in backward()
    leaves = [torch.randn(2, C, T, device=DEV, requires_grad=True), torch.randn(T, T, device=DEV), torch.randn(cb, C, device=DEV)]
    with pytest.raises(ValueError):
        ops.channel_attention_mix(*leaves)


def test_a_120_channel_cacn_trains():
    """CACN(120 -> 40): the channel matrix comes from batched torch ops (ops.channel_matrix), everything else from the
    library; forward and backward against cacn_dense in float64."""
    m, x, dout = fx.cacn_problem()
    m.to(DEV)
    xl = x.to(DEV).requires_grad_(True)
    out = m(xl)
    params = dict(m.named_parameters())
    grads = torch.autograd.grad(out, [xl] + list(params.values()), dout.to(DEV))
    leaves = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    x64 = x.to(DEV).double().requires_grad_(True)
    o64 = dense_torch.cacn_dense(x64, leaves["seq.0.Wc"], leaves["seq.0.alpha"], leaves["seq.1.weight"], leaves["seq.1.bias"])
    g64 = torch.autograd.grad(o64, [x64] + [leaves[k] for k in params], dout.to(DEV).double())
    for k, a, b in zip(["out", "dx"] + list(params), [out.detach()] + list(grads), [o64.detach()] + list(g64)):
        assert_parity(a, b, WHAT, f"cacn 120->40:{k}")


def test_both_schedules_agree_on_120_channel_blocks():
    """Two components of two blocks, 3 -> 120 -> 120: the stacked schedule against the component loop at the bars of
    test_stacked_components_equal_the_component_loop."""
    net, X, H, D, dout = fx.wide_model_problem()
    net.to(DEV)
    X, H, D, dout = (t.to(DEV) for t in (X, H, D, dout))
    params = [p for p in net.parameters() if p.requires_grad]
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    results = []
    for stack in (True, False):
        net.stack_components = stack
        pred = net(X, H, D)
        results.append((pred, torch.autograd.grad(pred, params, dout)))
    (p1, g1), (p2, g2) = results
    assert bool(torch.isfinite(p1).all())
    e = rel_err(p1, p2)
    record_err(WHAT, "msgat120 stacked vs loop:pred", e, 1e-5)
    assert e < 1e-5
    for n, a, b in zip(names, g1, g2):
        e = rel_err(a, b)
        record_err(WHAT, f"msgat120 stacked vs loop:{n}", e, 2e-5)
        assert e < 2e-5, n
