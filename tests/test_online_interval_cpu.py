"""CPU: calibrated intervals for online forecasts -- the numpy restatement of `msgat_interval_update` /
`msgat_interval_apply` against a brute force that knows nothing of rings, EXACTLY (radii and lo/hi bit for bit, counts as
integers); the rank table; the finite-sample coverage of the procedure on i.i.d. errors; and
`OnlineForecaster(score=True, intervals=...)` on a torch stand-in model against the same brute force over the forecasts
`step` returned.  Every case asserts that it inserts at every horizon, wraps a cursor, judges something, leaves the dead
node without an interval and masks a null reading."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from online_fixtures import DEAD, HOURS, NULL, Q as T_OUT, bits, history, raw_series
from online_interval_ref import (INF, NEVER, BruteForce, StandIn, apply_ref, fresh_state, rank_of, store_ref, update_ref)

TAU = 4
L = history(TAU)
LEVELS = (0.5, 0.8)
W = 4                            # small enough that every live series wraps its cursor within the fixture's steps
QUANTILES = (0.1, 0.5, 0.9)
HEADS = {"point": ((), T_OUT), "quantile": (QUANTILES, 2)}      # the head's own levels, T_out


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    word = np.int64 if got.dtype.itemsize == 8 else np.int32
    return np.array_equal(got.view(word), want.view(word))


def _exercised(brute, t_out, window):
    """What every case must show, from the brute force: a case that calibrates nothing is a failure, not a pass."""
    inserts = brute.inserts()
    assert (inserts.sum(0) > 0).all(), "a horizon inserted nothing"
    assert inserts.max() >= 2 * window, "no cursor wrapped"
    assert brute.judged.sum() > 0 and 0 < brute.covered.sum() < brute.judged.sum()
    assert inserts[DEAD].sum() == 0 and brute.judged[:, DEAD].sum() == 0 and np.isinf(brute.radius()[:, DEAD]).all()
    assert brute.null_masked > 0


# ---- the restatement against the brute force -----------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("extra_rows,chunk", [(0, 1), (2, 1), (0, 2), (3, 4)])
def test_the_restatement_equals_the_brute_force(head, extra_rows, chunk):
    from ms_gat_amd.intervals import interval_ranks
    quantiles, t_out = HEADS[head]
    raw = raw_series(3, 9).numpy()
    N, total = raw.shape[1], raw.shape[2]
    out, P, point = max(len(quantiles), 1) * t_out, t_out + extra_rows, 1 if quantiles else 0
    rng = np.random.default_rng(11 + t_out + extra_rows)
    ranks = interval_ranks(LEVELS, W).numpy()
    book, issued = np.zeros((P, N, out), np.float32), np.full(P, NEVER, np.int64)
    window, cursor, radius, radius_book, counts = fresh_state(len(LEVELS), N, t_out, W, P)
    lo, hi = np.zeros((len(LEVELS), N, t_out), np.float32), np.zeros((len(LEVELS), N, t_out), np.float32)
    brute = BruteForce(raw, t_out, LEVELS, W, point=point, null_value=NULL)
    for a in range(5, total, chunk):                           # a forecast, then `chunk` readings: chunk > 1 leaves origins out
        clock = np.array([a, 0], np.int64)
        forecast = (60 + 25 * rng.standard_normal((N, out))).astype(np.float32)
        store_ref(forecast, book, issued, clock)
        apply_ref(forecast, radius, clock, lo, hi, radius_book, point)
        want_lo, want_hi, want_r = brute.issue(a, forecast)
        assert _same(lo, want_lo) and _same(hi, want_hi) and _same(radius_book[a % P], want_r), a
        readings = np.ascontiguousarray(raw[:, :, a: a + chunk].transpose(2, 0, 1))
        update_ref(readings, book, issued, clock, radius_book, ranks, window, cursor, radius, counts, point, NULL)
        for step in range(a, min(a + chunk, total)):
            brute.push(step)
        assert _same(radius, brute.radius()), a
    _exercised(brute, t_out, W)
    assert _same(counts, brute.counts()) and _same(cursor, brute.cursor())
    assert (counts[0, :, :, 0] >= counts[1, :, :, 0]).all() and (counts[0] != counts[1]).any()   # 0.8 starts later


def test_a_nan_forecast_is_judged_as_missed_and_not_inserted():
    from ms_gat_amd.intervals import interval_ranks
    raw = raw_series(3, 9).numpy()
    N, t_out, P, node = raw.shape[1], T_OUT, T_OUT, 4
    rng = np.random.default_rng(2)
    ranks = interval_ranks(LEVELS, W).numpy()
    book, issued = np.zeros((P, N, t_out), np.float32), np.full(P, NEVER, np.int64)
    window, cursor, radius, radius_book, counts = fresh_state(len(LEVELS), N, t_out, W, P)
    lo, hi = np.zeros((len(LEVELS), N, t_out), np.float32), np.zeros((len(LEVELS), N, t_out), np.float32)
    brute = BruteForce(raw, t_out, LEVELS, W, null_value=NULL)
    for a in range(5, 30):
        clock = np.array([a, 0], np.int64)
        forecast = (60 + 25 * rng.standard_normal((N, t_out))).astype(np.float32)
        if a in (15, 16):
            forecast[node] = np.nan                            # issued with finite radii, every horizon
        store_ref(forecast, book, issued, clock)
        apply_ref(forecast, radius, clock, lo, hi, radius_book)
        brute.issue(a, forecast)
        before = cursor[node].copy()
        update_ref(np.ascontiguousarray(raw[:, :, a: a + 1].transpose(2, 0, 1)), book, issued, clock, radius_book, ranks,
                   window, cursor, radius, counts, 0, NULL)
        brute.push(a)
        if a == 15:
            assert cursor[node, 0] == before[0] and (cursor[node, 1:] != before[1:]).any()   # horizon 0 met the NaN
    assert brute.nan_judged == 2 * t_out * len(LEVELS) and not np.isnan(window).any()
    assert _same(counts, brute.counts()) and _same(cursor, brute.cursor()) and _same(radius, brute.radius())


def test_the_restatement_ignores_cold_negative_and_wild_clocks():
    from ms_gat_amd.intervals import interval_ranks
    N, t_out = 9, 3
    raw = np.ascontiguousarray(raw_series(3, 9).numpy()[:, :, 20:25].transpose(2, 0, 1))
    book, ranks = np.ones((t_out, N, t_out), np.float32), interval_ranks(LEVELS, W).numpy()
    for issued in (np.full(t_out, NEVER, np.int64), np.array([-3, -2, -1], np.int64)):
        for now in (0, -2, -7, 2 ** 62 + 1, 2 ** 63 - 2):
            state = fresh_state(2, N, t_out, W, t_out)
            state[3][:] = 1.0                                   # finite radii in the book: only the stamps say no
            update_ref(raw, book, issued, np.array([now, 0], np.int64), state[3], ranks, state[0], state[1], state[2],
                       state[4])
            assert not state[0].any() and not state[1].any() and not state[4].any() and np.isinf(state[2]).all()


# ---- the rank table -----------------------------------------------------------------------------------------------------
def test_the_rank_table():
    from ms_gat_amd.intervals import interval_levels, interval_ranks
    t = interval_ranks(0.9, 200)
    assert t.dtype == torch.int32 and tuple(t.shape) == (1, 201)
    assert t[0, 9] == 9 and t[0, 8] == 0 and not t[0, :9].any() and t[0, 109] == 99     # 110 * 0.9 in floats: 99.00000000000001
    assert t[0, 199] == 180 and t[0, 200] == 181
    assert all(int(t[0, m]) == rank_of(0.9, m) for m in range(201))
    held = interval_ranks(0.9, 200, min_count=50)
    assert not held[0, :50].any() and torch.equal(held[0, 50:], t[0, 50:])
    four = interval_ranks((0.5, 0.8, 0.9, 0.99), 1024)
    assert tuple(four.shape) == (4, 1025) and four[:, 1024].tolist() == [513, 820, 923, 1015]
    assert four[3, 98] == 0 and four[3, 99] == 99 and four[0, 1] == 1 and (four[:, 0] == 0).all()
    one = interval_ranks((0.5, 0.9), 1)
    assert one.tolist() == [[0, 1], [0, 0]]                      # ceil(2 * 0.9) = 2 does not exist among one value
    assert interval_levels(0.9) == (0.9,) and interval_levels([0.8, 0.95]) == (0.8, 0.95)
    for bad in ((), (0.5, 0.6, 0.7, 0.8, 0.9), (0.9, 0.8), (0.5, 0.5), (0.0,), (1.0,), (float("nan"),), "x"):
        with pytest.raises(ValueError, match="interval"):
            interval_levels(bad)
    for window in (0, 1025):
        with pytest.raises(ValueError, match="interval_window"):
            interval_ranks(0.9, window)
    for min_count in (0, 201):
        with pytest.raises(ValueError, match="interval_min_count"):
            interval_ranks(0.9, 200, min_count)


# ---- the coverage the procedure promises ---------------------------------------------------------------------------------
def test_coverage_of_iid_errors_is_the_nominal_level():
    """W = 99, level 0.9, intervals once a window is full: the radius is the 90th smallest of 99 errors, and a fresh
    exchangeable error is at most that with probability 90 / 100.  120 series with i.i.d. |N(0, sigma_series)| errors, 700
    steps: 120 * 601 = 72 120 intervals are judged, and |coverage - 0.9| <= 4 sqrt(0.9 * 0.1 / 72 120) = 0.0045."""
    from ms_gat_amd.intervals import _interval_apply_torch, _interval_update_torch, interval_ranks, interval_state
    N, window, steps = 120, 99, 700
    g = torch.Generator().manual_seed(5)
    sigma = 0.5 + 4.0 * torch.rand(N, generator=g)
    readings = 50.0 + sigma * torch.randn(steps, N, generator=g)
    forecast = torch.full((N, 1), 50.0)
    ranks = interval_ranks(0.9, window, min_count=window)
    assert ranks[0, window] == 90 and not ranks[0, :window].any()
    book, issued = torch.zeros(1, N, 1), torch.full((1,), NEVER, dtype=torch.int64)
    win, cursor, radius, radius_book, counts = interval_state(1, N, 1, window, 1, "cpu")
    lo, hi = torch.zeros(1, N, 1), torch.zeros(1, N, 1)
    for t in range(steps):
        clock = torch.tensor([t, 0])
        book[0], issued[0] = forecast, t
        _interval_apply_torch(forecast, radius, clock, lo, hi, radius_book)
        _interval_update_torch(readings[t][None, None], book, issued, clock, radius_book, ranks, win, cursor, radius, counts)
    judged, covered = int(counts[..., 0].sum()), int(counts[..., 1].sum())
    assert judged == 72120 and (counts[0, :, 0, 0] == 601).all()
    coverage = covered / judged
    print(f"coverage {coverage:.5f} over {judged} judged intervals")
    assert abs(coverage - 0.9) <= 4 * (0.9 * 0.1 / 72120) ** 0.5


# ---- the forecaster on a stand-in model -----------------------------------------------------------------------------------
def _forecaster(raw, head="point", start=0, **kw):
    from ms_gat_amd import OnlineForecaster, data
    quantiles, t_out = HEADS[head]
    torch.manual_seed(3)
    stats = data.series_stats(raw, HOURS, T_OUT, TAU, input_null_value=NULL)
    model = StandIn(stats.input_channels, max(len(quantiles), 1) * t_out, TAU)
    kw.setdefault("score", True)
    if kw["score"]:
        kw.setdefault("score_quantiles", quantiles or None)
        kw.setdefault("intervals", LEVELS)
        kw.setdefault("interval_window", W)
    return OnlineForecaster(model, stats, start, **kw)


def _brute(f, raw, head):
    quantiles, t_out = HEADS[head]
    return BruteForce(raw.numpy(), t_out, LEVELS, W, point=1 if quantiles else 0, null_value=NULL)


def _steps(f, raw, first, stop, brute=None, check=True):
    """step() with the readings of the steps first .. stop - 1; what it returned goes to the brute force."""
    for t in range(first, stop):
        y = f.step(raw[:, :, t])
        if brute is not None:
            brute.push(t)
            want_lo, want_hi, _ = brute.issue(t + 1, y.numpy())
            lo, hi = f.intervals()
            assert not check or (_same(lo.numpy(), want_lo) and _same(hi.numpy(), want_hi)), t


def _holds(f, brute):
    window, cursor, radius, radius_book, counts = (t.numpy() for t in f._interval_state)
    assert _same(radius, brute.radius()) and _same(counts, brute.counts()) and _same(cursor, brute.cursor())


@pytest.mark.parametrize("head", list(HEADS))
def test_intervals_of_the_forecaster_equal_the_brute_force(head):
    quantiles, t_out = HEADS[head]
    raw = raw_series(3, 9)
    total = raw.shape[-1]
    f = _forecaster(raw, head)
    empty = f.interval_scores()
    assert empty["judged"] == [0, 0] and empty["horizons"]["coverage"] == [[], []] and np.isnan(empty["coverage"]).all()
    assert bool(torch.isnan(f.interval_node_scores()).all()) and tuple(f.interval_node_scores().shape) == (9, 2)
    with pytest.raises(RuntimeError, match="none was made"):
        f.intervals()
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    brute = _brute(f, raw, head)
    _steps(f, raw, L - 1, total, brute)
    _exercised(brute, t_out, W)
    _holds(f, brute)
    lo, hi = f.intervals()
    assert lo.dtype == torch.float32 and tuple(lo.shape) == tuple(hi.shape) == (2, 9, t_out)
    assert bool(torch.isinf(lo[:, DEAD]).all()) and bool((lo[0] >= lo[1]).all()) and bool((hi[0] <= hi[1]).all())
    # interval_scores() and interval_node_scores(): ratios of those integers
    got, judged, covered, r = f.interval_scores(), brute.judged, brute.covered, brute.radius().astype(np.float64)
    assert set(got) == {"levels", "judged", "coverage", "width", "horizons"} and got["levels"] == list(LEVELS)
    assert got["judged"] == judged.sum((1, 2)).tolist()
    assert got["coverage"] == pytest.approx((covered.sum((1, 2)) / judged.sum((1, 2))).tolist(), rel=1e-12)
    finite = np.isfinite(r)
    assert got["width"] == pytest.approx([2 * r[l][finite[l]].mean() for l in range(2)], rel=1e-12)
    assert got["horizons"]["judged"] == judged.sum(1).tolist()
    flat = lambda rows: [v for row in rows for v in row]  # noqa: E731
    assert np.shape(got["horizons"]["coverage"]) == np.shape(got["horizons"]["width"]) == (2, t_out)
    assert flat(got["horizons"]["coverage"]) == pytest.approx(flat((covered.sum(1) / judged.sum(1)).tolist()), rel=1e-12)
    assert flat(got["horizons"]["width"]) == pytest.approx(
        [2 * r[l, :, h][finite[l, :, h]].mean() for l in range(2) for h in range(t_out)], rel=1e-12)
    at = f.interval_scores(at=[t_out, 1])["horizons"]
    assert at["coverage"] == [[c[t_out - 1], c[0]] for c in got["horizons"]["coverage"]]
    with pytest.raises(IndexError):
        f.interval_scores(at=[t_out + 1])
    nodes = f.interval_node_scores()
    assert nodes.dtype == torch.float64 and tuple(nodes.shape) == (9, 2) and bool(torch.isnan(nodes[DEAD]).all())
    live = judged.sum(2) > 0                                    # [L, N]
    want = covered.sum(2) / np.maximum(judged.sum(2), 1)
    assert nodes.numpy().T[live].tolist() == pytest.approx(want[live].tolist(), rel=1e-12)
    assert bool(torch.isnan(nodes.t()[torch.from_numpy(~live)]).all())
    assert f.scores()["count"] > 0                              # the scores beside it are still kept


def test_pushes_of_several_readings_and_a_bare_forecast():
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    brute = _brute(f, raw, "point")
    f.push(raw[:, :, :L].permute(2, 0, 1))
    t = L
    for chunk in (3, 1, T_OUT + 2, 2, 4, 1, 5, 2, 3, 4):
        y = f.forecast()
        f.forecast()                                            # twice at one origin changes nothing
        want_lo, want_hi, _ = brute.issue(t, y.numpy())
        assert _same(f.intervals()[0].numpy(), want_lo) and _same(f.intervals()[1].numpy(), want_hi), t
        f.push(raw[:, :, t: t + chunk].permute(2, 0, 1))
        for step in range(t, t + chunk):
            brute.push(step)
        t += chunk
        _holds(f, brute)
    assert brute.judged.sum() > 0 and brute.inserts().max() >= W


def test_min_count_holds_the_intervals_back():
    raw = raw_series(3, 9)
    f, g = _forecaster(raw, interval_min_count=W), _forecaster(raw)
    for x in (f, g):
        x.push(raw[:, :, :L - 1].permute(2, 0, 1))
        _steps(x, raw, L - 1, L + 3, None)
    assert bool(torch.isinf(f._interval_state[2]).all()) and bool(torch.isfinite(g._interval_state[2][0]).any())
    assert bool(torch.isinf(f.intervals()[1]).all())


def test_reset_scores_zeroes_the_counts_and_keeps_windows_and_radii():
    raw = raw_series(3, 9)
    f = _forecaster(raw)
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    brute = _brute(f, raw, "point")
    _steps(f, raw, L - 1, L + 12, brute)
    state = f._interval_state
    kept = [t.clone() for t in state[:4]]
    assert bool(state[4].any())
    f.reset_scores()
    assert f._interval_state is state and not state[4].any() and f.interval_scores()["judged"] == [0, 0]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(state[:4], kept))
    brute.judged[:], brute.covered[:] = 0, 0
    _steps(f, raw, L + 12, L + 22, brute)                       # the intervals in flight at the reset are still judged
    _holds(f, brute)
    assert brute.judged.sum() > 0


@pytest.mark.parametrize("head", list(HEADS))
def test_a_state_dict_round_trip_continues_to_the_same_bits(head):
    raw = raw_series(3, 9)
    f = _forecaster(raw, head, start=2)
    f.push(raw[:, :, 2: L + 1].permute(2, 0, 1))
    _steps(f, raw, L + 1, L + 12, None)
    state = f.state_dict()
    assert set(state) == {"ring", "clock", "start_step", "book", "issued", "score_sums", "score_node_sums",
                          "interval_window", "interval_cursor", "interval_radius", "interval_book", "interval_counts"}
    g = _forecaster(raw, head)
    g.model.load_state_dict(f.model.state_dict())
    g.load_state_dict(state)
    with pytest.raises(RuntimeError, match="none was made"):    # lo and hi are not state: they come with a forecast
        g.intervals()
    for t in state.values():                                    # the state is a copy, and so is what was loaded
        if torch.is_tensor(t):
            t.zero_()
    for t in range(L + 12, L + 24):
        assert torch.equal(bits(g.step(raw[:, :, t])), bits(f.step(raw[:, :, t]))), t
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(g.intervals(), f.intervals())), t
    words = lambda t: t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)  # noqa: E731
    for a, b in zip(f._interval_state, g._interval_state):
        assert torch.equal(words(a), words(b))
    assert bool(g._interval_state[4].any())
    for key, bad in (("interval_window", torch.zeros(9, 2, W + 1)), ("interval_cursor", torch.zeros(9, 2)),
                     ("interval_counts", torch.zeros(2, 9, 2, 2))):
        with pytest.raises(ValueError, match=key):
            g.load_state_dict({**f.state_dict(), key: bad})


def test_a_state_without_interval_keys_loads_cold():
    raw = raw_series(3, 9)
    scored = _forecaster(raw, intervals=None)
    scored.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(scored, raw, L - 1, L + 6, None)
    g = _forecaster(raw)
    g.model.load_state_dict(scored.model.state_dict())
    g.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(g, raw, L - 1, L + 9, None)
    state = g._interval_state
    assert bool(state[4].any()) and bool(torch.isfinite(state[2]).any()) and bool(state[1].any())
    g.load_state_dict(scored.state_dict())
    assert g._interval_state is state and not state[0].any() and not state[1].any() and not state[4].any()
    assert bool(torch.isinf(state[2]).all()) and bool(torch.isinf(state[3]).all()) and g.clock.tolist() == [L + 6, L]
    brute = _brute(g, raw, "point")                             # from here on it is a fresh calibration
    for origin in range(L + 6 - T_OUT + 1, L + 7):              # the loaded book's forecasts are due, without intervals
        row = origin % T_OUT
        assert int(g._score_state[1][row]) == origin
        brute.issue(origin, g._score_state[0][row].clone().numpy())     # a copy: the row is soon another origin's
        brute.issued_radius[origin][:] = INF
    _steps(g, raw, L + 6, raw.shape[-1], brute, check=False)
    _holds(g, brute)
    assert brute.judged.sum() > 0
    fresh = _forecaster(raw)                                    # before its first forecast: nothing to make cold
    fresh.load_state_dict(scored.state_dict())
    assert fresh._interval_state is not None and not fresh._interval_state[1].any() and fresh.ready


def test_without_intervals_nothing_is_added():
    raw = raw_series(3, 9)
    f = _forecaster(raw, intervals=None)
    f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    _steps(f, raw, L - 1, L + 3, None)
    assert set(f.state_dict()) == {"ring", "clock", "start_step", "book", "issued", "score_sums", "score_node_sums"}
    assert f._interval_state is None and f.interval_levels == () and not hasattr(f, "_interval_ranks")
    plain = _forecaster(raw, score=False)
    assert set(plain.state_dict()) == {"ring", "clock", "start_step"}
    for x in (f, plain):
        for call in (x.intervals, x.interval_scores, x.interval_node_scores):
            with pytest.raises(RuntimeError, match="intervals="):
                call()


def test_arguments_that_are_refused():
    raw = raw_series(3, 9)
    with pytest.raises(ValueError, match="score=True"):
        _forecaster(raw, score=False, intervals=0.9)
    for bad in ((0.9, 0.8), (0.1, 0.2, 0.3, 0.4, 0.5), 1.0, 0.0, ()):
        with pytest.raises(ValueError, match="interval"):
            _forecaster(raw, intervals=bad)
    for window in (0, 1025):
        with pytest.raises(ValueError, match="interval_window"):
            _forecaster(raw, interval_window=window)
    with pytest.raises(ValueError, match="interval_min_count"):
        _forecaster(raw, interval_min_count=W + 1)
    assert _forecaster(raw, intervals=0.9).interval_levels == (0.9,)


# ---- ABI and build ------------------------------------------------------------------------------------------------------
_NEW = {"msgat_interval_update": 22, "msgat_interval_apply": 13}


def test_entry_points_are_declared_prototyped_and_exported():
    from ms_gat_amd import _lib, build, intervals
    path = build.build(verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgat_hip.h")).read(), flags=re.S)
    lib = C.CDLL(path)
    for name, n_args in _NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/msgat_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_lib._PROTOTYPES[name][1]) == n_args and _lib._PROTOTYPES[name][0] is C.c_int
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 10 and lib.msgat_abi_version() == 10
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", text)
    assert "online_interval.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "online_interval.hip"))
    assert os.path.join(build.CSRC, "score_clock.hpp") in build.HEADERS
    assert callable(intervals.interval_update) and callable(intervals.interval_apply)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """NULL, shape and size checks come before any launch: no device needed."""
    from ms_gat_amd import _lib
    lib = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below fails its checks
    NULL_, SHAPE, UNSUPPORTED = -1, -2, -3

    def update(K=1, C_=1, N=4, T=3, out=3, point=0, P=3, L_=2, W_=8, ptrs=(p,) * 10):
        return lib.msgat_interval_update(*ptrs, K, C_, N, T, out, point, P, L_, W_, 1, 0.0, None)

    def apply(N=4, T=3, out=3, point=0, P=3, L_=2, ptrs=(p,) * 6):
        return lib.msgat_interval_apply(*ptrs, N, T, out, point, P, L_, None)

    for hole in range(10):
        assert update(ptrs=tuple(None if i == hole else p for i in range(10))) == NULL_, hole
    for hole in range(6):
        assert apply(ptrs=tuple(None if i == hole else p for i in range(6))) == NULL_, hole
    for kw in (dict(K=0), dict(C_=0), dict(N=0), dict(T=0), dict(L_=0), dict(W_=0), dict(K=-1), dict(W_=-5), dict(P=2),
               dict(out=0), dict(point=1), dict(point=-1), dict(out=6, point=2), dict(out=4)):
        assert update(**kw) == SHAPE, kw
    for kw in (dict(N=0), dict(T=0), dict(L_=0), dict(P=2), dict(point=1), dict(point=-1), dict(out=6, point=2)):
        assert apply(**kw) == SHAPE, kw
    for kw in (dict(L_=5), dict(W_=1025), dict(T=65, out=65, P=65), dict(T=5, out=65, P=5), dict(N=2 ** 31 - 1)):
        assert update(**kw) == UNSUPPORTED, kw
    for kw in (dict(L_=5), dict(T=65, out=65, P=65), dict(T=5, out=65, P=5), dict(N=2 ** 31 - 1)):
        assert apply(**kw) == UNSUPPORTED, kw
