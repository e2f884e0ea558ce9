"""No GPU: the conditions test_gpu_branch_edges.py rests on, so that a failure there blames the kernel and not the inputs.

* The large-score cases and the 40 block cases: the float64 restatement evaluated in fp32 on the CPU meets the bar the
  GPU test applies to the kernels, with room (the kernels do the same arithmetic in the same format).
* The score regimes are the intended ones: every softmax row one-hot at the saturated scale, a third to 95 % of them at
  the large scale.
* The whole-model seeds keep the fp32 restatement under a quarter of the 1e-4 bar.
* The restated LDS formulas of the channel attention give the channel counts quoted in README.md and model.py."""
import pytest
import torch

from conftest import elementwise_violations, rel_err

import branch_edge_fixtures as fx

TOL = 1e-4


def _channel(case, scale):
    p, Wc, conv, dMc = fx.channel_inputs(case, scale)
    return (p, Wc, conv), dMc, fx.channel_attention_mix_dense


def _temporal(case, scale):
    q, W1, W2, dtaps = fx.temporal_inputs(case, scale)
    return (q, W1, W2), dtaps, lambda a, b, c: fx.temporal_attention_taps_dense(a, b, c, case[5])


OPS = [(_channel, c) for c in fx.CHANNEL_CASES] + [(_temporal, c) for c in fx.TEMPORAL_CASES]
IDS = [f"{b.__name__[1:]}{c}" for b, c in OPS]


def _parity(got, want, what):
    assert rel_err(got, want) < TOL, what
    assert elementwise_violations(got, want, 1e-4, 1e-5) == 0.0, what


@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_large_scores_leave_the_fp32_op_sequence_inside_the_bar(build, case):
    """Output under the parity bar in both its forms; every gradient within 1e-4 / 3 of float64, so that the GPU test's
    max(1e-4, 3 x this distance) IS 1e-4 for every case."""
    inputs, cot, fn = build(case, fx.LARGE)
    r64, r32 = fx.evaluate(fn, inputs, cot, torch.float64), fx.evaluate(fn, inputs, cot, torch.float32)
    _parity(r32[0], r64[0], "output")
    for a, b in zip(r32[1:], r64[1:]):
        assert 3.0 * rel_err(a, b) < TOL


@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_score_regimes_are_the_intended_ones(build, case):
    for scale, lo, hi in ((fx.SATURATED, 1.0, 1.0), (fx.LARGE, 0.3, 0.95)):
        inputs, _, _ = build(case, scale)
        a, b = inputs[0].double(), inputs[1].double()
        att = fx.channel_attention(a, b) if build is _channel else fx.temporal_attention(a, b, inputs[2].double())
        assert lo <= fx.one_hot_fraction(att) <= hi, scale


@pytest.mark.parametrize("build,case", OPS, ids=IDS)
def test_saturated_scores_leave_the_fp32_op_sequence_inside_the_bars(build, case):
    """Output under the parity bar; the gradients within 1e-5 of their cancelling terms."""
    inputs, cot, fn = build(case, fx.SATURATED)
    r64, r32 = fx.evaluate(fn, inputs, cot, torch.float64), fx.evaluate(fn, inputs, cot, torch.float32)
    _parity(r32[0], r64[0], "output")
    terms = (fx.channel_cancelling_terms(*inputs, cot) if build is _channel else
             fx.temporal_cancelling_terms(*inputs, cot, case[5]))
    for (k, s), a, b in zip(terms.items(), r32[1:], r64[1:]):
        assert torch.isfinite(a).all() and float(s) > 0
        assert float((a.double() - b).abs().max()) <= 1e-5 * float(s), k


@pytest.mark.parametrize("T,N", fx.MEAM_SHAPES)
@pytest.mark.parametrize("Ci,Co,dilations", fx.MEAM_BLOCKS)
def test_block_oracle_in_fp32_meets_the_parity_bar(Ci, Co, dilations, T, N):
    """dense_torch.meam_dense with the ReLU mask pinned: output, dx and every parameter gradient."""
    block, x, dout, adj = fx.meam_problem(Ci, Co, dilations, T, N)
    state = block.state_dict()
    mask = fx.meam_reference(state, x, dout, adj, dilations, None, torch.float64)["out"] > 0
    r64 = fx.meam_reference(state, x, dout, adj, dilations, mask, torch.float64)
    r32 = fx.meam_reference(state, x, dout, adj, dilations, mask, torch.float32)
    assert set(r64) == {"out", "dx"} | {n for n, _ in block.named_parameters()}
    for k in r64:
        _parity(r32[k], r64[k], k)


@pytest.mark.parametrize("T,N", fx.STACKED_CASES)
def test_whole_model_seeds_keep_the_fp32_restatement_under_a_quarter_of_the_bar(T, N):
    net, X, H, D, dout = fx.stacked_problem(T, N)
    p64, g64 = fx.msgat_reference(net, X, H, D, dout, torch.float64)
    p32, g32 = fx.msgat_reference(net, X, H, D, dout, torch.float32)
    assert rel_err(p32, p64) < 2.5e-5
    assert len(g64) == sum(1 for p in net.parameters() if p.requires_grad)
    for k in g64:
        assert rel_err(g32[k], g64[k]) < 2.5e-5, k


def test_pool_and_time_mix_tables_cover_what_they_name():
    assert {n for n, _, _ in fx.POOL_CASES} == {63, 64, 65, 255, 256, 257, 1025}
    assert {c for _, c, _ in fx.POOL_CASES} == {1, 16, 17} and {t for _, _, t in fx.POOL_CASES} == {4, 8, 12, 16}
    assert fx.POOL_SLICE_CASE in fx.POOL_CASES and fx.TIME_MIX_SLICE_CASE in fx.TIME_MIX_CASES
    assert any(Co * N < 4 for _, Co, N in fx.TIME_MIX_CASES)
    assert {T * N for T, N in fx.MEAM_SHAPES if T * N >= 512} == {512, 1024}


def test_channel_attention_lds_formulas_give_the_quoted_channel_counts():
    """T = 12, cb = C / 3: 114 fits both directions, 117 .. 165 only the forward, from 168 neither."""
    def fits(C):
        return fx.chanatt_fits(C, C // 3, 12)
    assert fx.CHANATT_LDS_FLOATS == 40704
    assert fits(114) == (True, True)
    assert fits(117) == (True, False) and fits(165) == (True, False)
    assert fits(168) == (False, False)
    assert all(fits(C) == (True, True) for C in range(3, 115, 3))
    assert all(fits(C) == (True, False) for C in range(117, 166, 3))
    # the cases of the score-edge table are inside the envelope, the last one at its edge
    assert all(fx.chanatt_fits(C, cb, T) == (True, True) for _, _, C, cb, T in fx.CHANNEL_CASES)
    assert fx.CHANNEL_CASES[-1][2:] == (114, 38, 12)


def test_the_library_reports_the_same_envelope():
    """msgat_channel_attention_fused (what model.CACN and stacked.py ask before they launch) against the restatement."""
    from ms_gat_amd import _lib
    L = _lib.lib()
    for T in (4, 8, 12, 16):
        for C in (1, 3, 72, 96, 114, 115, 117, 120, 165, 168, 256):
            for cb in (1, C // 3 or 1, C):
                assert bool(L.msgat_channel_attention_fused(C, cb, T)) == all(fx.chanatt_fits(C, cb, T)), (C, cb, T)
    assert L.msgat_channel_attention_fused(72, 24, 5) == 0 and L.msgat_channel_attention_fused(0, 24, 12) == 0
    assert L.msgat_channel_attention_fused(257, 24, 4) == 0
