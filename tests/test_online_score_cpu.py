"""CPU: scoring online forecasts -- the numpy restatement of `msgat_forecast_store` / `msgat_forecast_score` against a
brute-force scorer, and `OnlineForecaster(score=True)` on a torch stand-in model against the same brute force over the
forecasts `step` returned.  Counts and hits are exact; every other sum agrees within (n - 1) 2^-53 sum |term|, the bound of
a double sum of n terms, computed from the brute force's own terms.  Every case asserts that it settles something at
every horizon, nothing at the dead node, masks an entry by the null value and leaves one out of MAPE."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from conftest import ROOT
from online_fixtures import DEAD, HOURS, NULL, Q as T_OUT, bits, history, raw_series
from online_score_ref import (NEVER, assert_equal_brute_force, brute_force, columns, score_ref, store_ref)

TAU = 4
L = history(TAU)
MASK = 30.0                      # readings are 60 +- 20, at least 1: some valid ones lie at or below it
LEVELS = (0.1, 0.5, 0.9)
HEADS = {"point": ((), T_OUT), "quantile": (LEVELS, 2)}      # levels, T_out


def _exercised(want, t_out):
    """What every case must show, from the brute force: a case that settles nothing is a failure, not a pass."""
    assert (want["n"][:t_out, 0] > 0).all(), "a horizon settled nothing"
    assert want["node_n"][DEAD, 0] == 0 and want["node_n"][:, 0].sum() > 0
    assert want["null_masked"] > 0 and want["mape_left_out"] > 0


# ---- the restatement against the brute force -----------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("extra_rows,chunk", [(0, 1), (2, 1), (0, 2), (3, 4)])
def test_the_restatement_agrees_with_the_brute_force(head, extra_rows, chunk):
    levels, t_out = HEADS[head]
    raw = raw_series(3, 9).numpy()
    N, total = raw.shape[1], raw.shape[2]
    out, P, point = max(len(levels), 1) * t_out, t_out + extra_rows, 1 if levels else 0
    rng = np.random.default_rng(7 + t_out + extra_rows)
    book, issued = np.zeros((P, N, out), np.float32), np.full(P, NEVER, np.int64)
    sums, node_sums = np.zeros((t_out + 1, columns(len(levels)))), np.zeros((N, 3))
    start, pairs = 5, []
    for a in range(start, total, chunk):                       # a forecast, then `chunk` readings: chunk > 1 leaves origins out
        clock = np.array([a, 0], np.int64)
        forecast = (60 + 25 * rng.standard_normal((N, out))).astype(np.float32)
        store_ref(forecast, book, issued, clock)
        pairs.append((a, forecast))
        readings = np.ascontiguousarray(raw[:, :, a: a + chunk].transpose(2, 0, 1))
        score_ref(readings, book, issued, clock, t_out, levels, point, NULL, MASK, sums, node_sums)
    want = brute_force(pairs, raw, total, t_out, levels, point, NULL, MASK, first_step=start)
    _exercised(want, t_out)
    assert_equal_brute_force(sums, node_sums, want, len(levels), (head, extra_rows, chunk))


def test_the_restatement_ignores_cold_negative_and_wild_clocks():
    N, t_out = 9, 3
    raw = np.ascontiguousarray(raw_series(3, 9).numpy()[:, :, 20:25].transpose(2, 0, 1))
    book = np.ones((t_out, N, t_out), np.float32)
    for issued in (np.full(t_out, NEVER, np.int64), np.array([-3, -2, -1], np.int64)):
        for now in (0, -2, -7, 2 ** 62 + 1):
            sums, node_sums = np.zeros((t_out + 1, 5)), np.zeros((N, 3))
            score_ref(raw, book, issued, np.array([now, 0], np.int64), t_out, (), 0, NULL, 0.0, sums, node_sums)
            assert not sums.any() and not node_sums.any(), (issued, now)


# ---- the forecaster on a stand-in model -----------------------------------------------------------------------------------
class StandIn(nn.Module):
    """(X [B,R,C,N,T], H [B], D [B]) -> [B,N,out] near the scale of the readings: every input moves the output."""

    def __init__(self, in_channels, out):
        super().__init__()
        self.in_channels = in_channels
        self.proj = nn.Linear(len(HOURS) * in_channels * TAU, out)
        self.h_ebd, self.d_ebd = nn.Embedding(24, out), nn.Embedding(7, out)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        y = self.proj(X.permute(0, 3, 1, 2, 4).reshape(B, N, R * C_ * T)) + (self.h_ebd(H) + self.d_ebd(D))[:, None]
        return 55.0 + 20.0 * y


def _forecaster(raw, head="point", start=0, out=None, **kw):
    from ms_gat_amd import OnlineForecaster, data
    levels, t_out = HEADS[head]
    torch.manual_seed(3)
    stats = data.series_stats(raw, HOURS, T_OUT, TAU, input_null_value=NULL)
    model = StandIn(stats.input_channels, max(len(levels), 1) * t_out if out is None else out)
    kw.setdefault("score", True)
    if kw["score"]:
        kw.setdefault("score_quantiles", levels or None)
        kw.setdefault("score_mask_value", MASK)
    return OnlineForecaster(model, stats, start, **kw)


def _steps(f, raw, first, stop, pairs):
    """step() with the readings of the steps first .. stop - 1; the forecasts it returned, cloned, go to `pairs`."""
    for t in range(first, stop):
        pairs.append((t + 1, f.step(raw[:, :, t]).clone().numpy()))


def _brute(f, pairs, raw, stop, head, first_step=0):
    levels, t_out = HEADS[head]
    return brute_force(pairs, raw.numpy(), stop, t_out, levels, 1 if levels else 0, NULL, MASK, first_step=first_step)


def _totals(f):
    return f._score_state[2].numpy(), f._score_state[3].numpy()


@pytest.mark.parametrize("head", list(HEADS))
def test_scores_of_the_forecaster_equal_the_brute_force(head):
    levels, t_out = HEADS[head]
    raw = raw_series(3, 9)
    total = raw.shape[-1]
    f = _forecaster(raw, head)
    assert f.scores()["count"] == 0 and f.scores()["horizons"]["MAE"] == [] and f.node_scores()[:, 0].tolist() == [0.0] * 9
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    pairs = []
    _steps(f, raw, L - 1, total, pairs)
    want = _brute(f, pairs, raw, total, head)
    _exercised(want, t_out)
    assert_equal_brute_force(*_totals(f), want, len(levels), head)
    # scores() and node_scores(): Metrics' ratios of those totals
    got, s, n = f.scores(), want["sums"], np.maximum(want["sums"][:, 0], 1.0)
    approx = lambda v: pytest.approx(v, rel=1e-12, abs=1e-12)  # noqa: E731
    assert got["count"] == s[-1, 0] and got["horizons"]["count"] == s[:-1, 0].tolist()
    assert got["MAE"] == approx(s[-1, 1] / n[-1]) and got["MAPE"] == approx(s[-1, 2] / n[-1])
    assert got["RMSE"] == approx((s[-1, 3] / n[-1]) ** 0.5) and got["bias"] == approx(s[-1, 4] / n[-1])
    assert got["horizons"]["MAE"] == approx((s[:-1, 1] / n[:-1]).tolist())
    assert got["horizons"]["bias"] == approx((s[:-1, 4] / n[:-1]).tolist())
    assert got["horizons"]["RMSE"] == approx(((s[:-1, 3] / n[:-1]) ** 0.5).tolist())
    at = f.scores(at=[t_out, 1])["horizons"]
    assert at["MAE"] == [got["horizons"]["MAE"][t_out - 1], got["horizons"]["MAE"][0]]
    with pytest.raises(IndexError):
        f.scores(at=[t_out + 1])
    if levels:
        q = len(levels)
        summary = got["quantiles"]
        assert set(summary) == {"levels", "coverage", "pinball", "crossing", "width"} and summary["levels"] == list(levels)
        assert summary["coverage"] == approx((s[-1, 7:7 + q] / n[-1]).tolist())
        assert summary["pinball"] == approx((s[-1, 7 + q:7 + 2 * q] / n[-1]).tolist())
        assert summary["crossing"] == approx(s[-1, 5] / n[-1]) and summary["width"] == approx(s[-1, 6] / n[-1])
        assert s[-1, 5] > 0, "no entry's levels cross: the column is not exercised"
        assert len(at["coverage"]) == q and len(at["coverage"][0]) == 2
    else:
        assert "quantiles" not in got
    nodes = f.node_scores()
    assert nodes.shape == (9, 3) and nodes.dtype == torch.float64
    assert nodes[DEAD, 0] == 0 and bool(torch.isnan(nodes[DEAD, 1:]).all())
    live = want["node"][:, 0] > 0
    assert nodes[:, 0].tolist() == want["node"][:, 0].tolist()
    assert nodes[live, 1].tolist() == approx((want["node"][live, 1] / want["node"][live, 0]).tolist())
    assert nodes[live, 2].tolist() == approx((want["node"][live, 2] / want["node"][live, 0]).tolist())


def test_a_cold_book_settles_only_the_horizons_already_issued():
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    f.push(raw[:, :, :L].permute(2, 0, 1))
    first = f.forecast().clone().numpy()                        # origin L, into a cold book
    assert f._score_state[1].tolist().count(NEVER) == T_OUT - 1
    f.push(raw[:, :, L])
    sums, node_sums = _totals(f)
    assert sums[0, 0] > 0 and not sums[1:T_OUT].any() and np.array_equal(sums[T_OUT], sums[0])
    assert_equal_brute_force(sums, node_sums, _brute(f, [(L, first)], raw, L + 1, "point"), 0)


def test_pushes_of_several_readings_skip_the_origins_never_issued():
    """K = 3 and K = T_out + 2 readings with no forecast in between: the second push runs past the last issued origin's
    horizons and over the row that still holds it -- a stale row settles nothing."""
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    f.push(raw[:, :, :L].permute(2, 0, 1))
    pairs = [(L, f.forecast().clone().numpy())]
    f.push(raw[:, :, L: L + 3].permute(2, 0, 1))
    assert_equal_brute_force(*_totals(f), _brute(f, pairs, raw, L + 3, "point"), 0, "K = 3")
    pairs.append((L + 3, f.forecast().clone().numpy()))
    f.push(raw[:, :, L + 3: L + 3 + T_OUT + 2].permute(2, 0, 1))
    want = _brute(f, pairs, raw, L + 5 + T_OUT, "point")
    _exercised(want, T_OUT)
    assert_equal_brute_force(*_totals(f), want, 0, "K = T_out + 2")
    assert sorted(f._score_state[1].tolist()) == [NEVER, NEVER, L + 3]      # L + 3 took the row of L; L + 6 would be next
    assert f.clock.tolist()[0] == L + 5 + T_OUT


def test_forecast_twice_at_one_origin_changes_nothing():
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    f.push(raw[:, :, :L].permute(2, 0, 1))
    f.forecast()
    book, issued = f._score_state[0].clone(), f._score_state[1].clone()
    f.forecast()
    assert torch.equal(bits(f._score_state[0]), bits(book)) and torch.equal(f._score_state[1], issued)
    assert not f._score_state[2].any() and not f._score_state[3].any()


def test_reset_scores_zeroes_the_totals_and_keeps_the_book():
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    pairs = []
    _steps(f, raw, L - 1, L + 10, pairs)
    sums, node_sums = f._score_state[2], f._score_state[3]
    book, issued = f._score_state[0].clone(), f._score_state[1].clone()
    assert bool(sums.any()) and bool(node_sums.any())
    f.reset_scores()
    assert f._score_state[2] is sums and f._score_state[3] is node_sums          # in place
    assert not sums.any() and not node_sums.any() and f.scores()["count"] == 0
    assert torch.equal(bits(f._score_state[0]), bits(book)) and torch.equal(f._score_state[1], issued)
    _steps(f, raw, L + 10, L + 20, pairs)                       # the forecasts in flight at the reset are still settled
    want = _brute(f, pairs, raw, L + 20, "point", first_step=L + 10)
    _exercised(want, T_OUT)
    assert_equal_brute_force(*_totals(f), want, 0)


@pytest.mark.parametrize("head", list(HEADS))
def test_a_state_dict_round_trip_continues_to_the_same_bits(head):
    raw = raw_series(3, 9)
    f = _forecaster(raw, head, start=2)
    f.push(raw[:, :, 2: L + 1].permute(2, 0, 1))
    _steps(f, raw, L + 1, L + 9, [])
    state = f.state_dict()
    assert set(state) == {"ring", "clock", "start_step", "book", "issued", "score_sums", "score_node_sums"}
    g = _forecaster(raw, head)
    g.model.load_state_dict(f.model.state_dict())
    g.load_state_dict(state)
    for t in state.values():                                    # the state is a copy, and so is what was loaded
        if torch.is_tensor(t):
            t.zero_()
    for t in range(L + 9, L + 20):
        assert torch.equal(bits(g.step(raw[:, :, t])), bits(f.step(raw[:, :, t]))), t
    words = lambda t: t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)  # noqa: E731
    for a, b in zip(f._score_state, g._score_state):
        assert torch.equal(words(a), words(b))
    assert bool(g._score_state[2].any())
    with pytest.raises(ValueError, match="book"):
        g.load_state_dict({**f.state_dict(), "book": torch.zeros(5, 9, 3)})


def test_a_state_from_a_forecaster_without_scoring_loads_cold():
    raw = raw_series(3, 9)
    plain = _forecaster(raw, score=False)
    plain.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(plain, raw, L - 1, L + 6, [])
    g = _forecaster(raw)
    g.model.load_state_dict(plain.model.state_dict())
    g.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(g, raw, L - 1, L + 3, [])
    sums = g._score_state[2]
    assert bool(sums.any())
    g.load_state_dict(plain.state_dict())
    assert g._score_state[2] is sums and not sums.any() and not g._score_state[3].any()
    assert g._score_state[1].tolist() == [NEVER] * T_OUT and g.clock.tolist() == [L + 6, L]
    pairs = []
    _steps(g, raw, L + 6, L + 20, pairs)                        # what was in g's book before the load settles nothing
    want = _brute(g, pairs, raw, L + 20, "point")
    _exercised(want, T_OUT)
    assert_equal_brute_force(*_totals(g), want, 0)
    fresh = _forecaster(raw)                                    # before its first forecast: nothing to make cold
    fresh.load_state_dict(plain.state_dict())
    assert fresh._score_state is None and fresh.ready


def test_without_score_nothing_is_added():
    raw = raw_series(3, 9)
    f = _forecaster(raw, score=False)
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(f, raw, L - 1, L + 3, [])
    assert set(f.state_dict()) == {"ring", "clock", "start_step"} and f._score_state is None and not f.score
    for call in (f.scores, f.node_scores, f.reset_scores):
        with pytest.raises(RuntimeError, match="score=True"):
            call()


def test_a_head_that_is_not_levels_times_horizons_is_refused():
    raw = raw_series(3, 9)
    f = _forecaster(raw, "quantile", out=5)                     # three levels, five outputs
    f.push(raw[:, :, :L].permute(2, 0, 1))
    with pytest.raises(ValueError, match="Q \\* T_out"):
        f.forecast()
    with pytest.raises(ValueError, match="quantile levels"):
        _forecaster(raw, score_quantiles=(0.5, 0.4))
    g = _forecaster(raw, out=65)                                # a point head beyond 64 horizons
    g.push(raw[:, :, :L].permute(2, 0, 1))
    with pytest.raises(ValueError, match="Q \\* T_out"):
        g.forecast()


# ---- ABI and build ------------------------------------------------------------------------------------------------------
_NEW = {"msgat_forecast_store": (8, C.c_int), "msgat_forecast_score_partial_doubles": (3, C.c_size_t),
        "msgat_forecast_score": (19, C.c_int)}


def test_entry_points_are_declared_prototyped_bound_and_exported():
    from ms_gat_amd import _lib, build, ops
    path = build.build(verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgat_hip.h")).read(), flags=re.S)
    lib = C.CDLL(path)
    for name, (n_args, res) in _NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/msgat_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_lib._PROTOTYPES[name][1]) == n_args and _lib._PROTOTYPES[name][0] is res
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 10 and lib.msgat_abi_version() == 10
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", text)
    assert "online_score.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "online_score.hip"))
    assert callable(ops.forecast_store) and callable(ops.forecast_score)
    assert ops.SCORE_NEVER == NEVER and ops.score_columns(0) == 5 and ops.score_columns(3) == 13


def test_entry_points_refuse_bad_arguments_on_the_host():
    """NULL, shape and size checks come before any launch: no device needed."""
    from ms_gat_amd import _lib
    lib = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below fails its checks
    NULL_, SHAPE, UNSUPPORTED = -1, -2, -3
    store = lambda *a: lib.msgat_forecast_store(*a, None)  # noqa: E731
    assert store(None, p, p, p, 4, 3, 3) == NULL_ and store(p, p, p, None, 4, 3, 3) == NULL_
    for N, out, P in ((0, 3, 3), (4, 0, 3), (4, 3, 0)):
        assert store(p, p, p, p, N, out, P) == SHAPE, (N, out, P)
    assert store(p, p, p, p, 2 ** 31 - 1, 3, 3) == UNSUPPORTED
    levels = (C.c_float * 3)(0.1, 0.5, 0.9)

    def score(K=1, C_=1, N=4, T=3, Q=0, lv=None, point=0, P=3, ptrs=(p,) * 7):
        return lib.msgat_forecast_score(*ptrs[:4], K, C_, N, T, Q, lv, point, P, 1, 0.0, 0.0, *ptrs[4:], None)

    for hole in range(7):
        assert score(ptrs=tuple(None if i == hole else p for i in range(7))) == NULL_, hole
    assert score(Q=3, T=2, lv=None) == NULL_
    for kw in (dict(K=0), dict(C_=0), dict(N=0), dict(T=0), dict(Q=-1), dict(P=2), dict(Q=3, T=2, lv=levels, point=3),
               dict(Q=3, T=2, lv=levels, point=-1), dict(Q=3, T=2, lv=(C.c_float * 3)(0.5, 0.5, 0.9)),
               dict(Q=3, T=2, lv=(C.c_float * 3)(0.1, float("nan"), 0.9)), dict(Q=1, T=2, lv=(C.c_float * 1)(1.0))):
        assert score(**kw) == SHAPE, kw
    big = (C.c_float * 9)(*[0.1 * (i + 1) for i in range(9)])
    for kw in (dict(Q=9, T=1, lv=big, P=64), dict(Q=3, T=22, lv=levels, P=64), dict(T=65, P=65), dict(N=2 ** 31 - 1)):
        assert score(**kw) == UNSUPPORTED, kw
    size = lib.msgat_forecast_score_partial_doubles
    assert size(300, 12, 0) == 5 * 12 * 300 and size(40, 4, 3) == 13 * 4 * 40 and size(6, 8, 8) == 23 * 8 * 6
    assert size(0, 12, 0) == size(4, 0, 0) == size(4, 65, 0) == size(4, 8, 9) == size(4, 22, 3) == size(4, 4, -1) == 0
