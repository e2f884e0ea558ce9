"""GPU: `msgat_forecast_store` / `msgat_forecast_score` and `OnlineForecaster(score=True)` on the device.

The kernels add in one fixed, documented order, so `sums`, `node_sums`, `book` and `issued` are compared BIT FOR BIT with
the numpy restatement of tests/online_score_ref.py (which test_online_score_cpu.py holds against a brute-force scorer).
Rows come from floor-mods, so a cold book, a negative clock and a clock near 2^62 must leave everything as it was -- the
in-bounds-by-construction check `test_a_cold_ring_stays_in_bounds` makes for the ring."""
import numpy as np
import pytest
import torch

from online_fixtures import HOURS, NULL, bits, raw_series
from online_score_ref import NEVER, columns, score_ref, store_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASK = 30.0
LEVELS3 = (0.1, 0.5, 0.9)
LEVELS8 = (0.05, 0.2, 0.35, 0.5, 0.6, 0.75, 0.9, 0.97)


def _words(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same(got, want):
    return torch.equal(_words(got), _words(torch.from_numpy(np.ascontiguousarray(want))))


def _case(N, C_, T, K, n_levels, start, seed=0, extra_rows=2):
    """A book in mid-flight: most rows carry the newest origin that maps to them, some a future one (inside the K
    readings), some an origin one turn too old (stale) or none at all.  Readings with nulls, a NaN and values below MASK."""
    rng = np.random.default_rng(1000 * N + 100 * T + 10 * K + C_ + seed)
    P, out = T + extra_rows, max(n_levels, 1) * T
    book = (60 + 25 * rng.standard_normal((P, N, out))).astype(np.float32)
    issued = np.full(P, NEVER, np.int64)
    for row in range(P):
        newest = start - 1 - ((start - 1 - row) % P)            # the largest origin < start in this row
        kind = rng.random()
        if kind < 0.6:
            issued[row] = newest
        elif kind < 0.75:
            issued[row] = newest + P                             # >= start: issued "inside" the pushed readings
        elif kind < 0.9:
            issued[row] = newest - P                             # stale
    issued[start % P] = start                                    # the usual state: the forecast made just before k = 0
    if P > 1:
        issued[(start - 1) % P] = start - 1
    raw = np.maximum(60 + 20 * rng.standard_normal((K, C_, N)), 1.0).astype(np.float32)
    raw[rng.random((K, C_, N)) < 0.15] = NULL
    raw[0, 0, N // 2] = np.nan
    raw[:, :, 0] = NULL                                          # a dead node
    return book, issued, raw, np.array([start, 5], np.int64)


def _score_both_ways(book, issued, raw, clock, T, levels, has_null, calls=2):
    """(device sums, node_sums, book, issued), (restated sums, node_sums) after `calls` identical calls."""
    from ms_gat_amd import ops
    N, W = book.shape[1], columns(len(levels))
    point = 1 if levels else 0
    null = NULL if has_null else None
    dev = [torch.from_numpy(a).to(DEV) for a in (raw, book, issued, clock)]
    sums = torch.zeros(T + 1, W, dtype=torch.float64, device=DEV)
    node_sums = torch.zeros(N, 3, dtype=torch.float64, device=DEV)
    want_sums, want_nodes = np.zeros((T + 1, W)), np.zeros((N, 3))
    for _ in range(calls):                                       # the totals are added to, not overwritten
        ops.forecast_score(*dev, T, sums, node_sums, levels=levels or None, point=point, null_value=null, mask_value=MASK)
        score_ref(raw, book, issued, clock, T, levels, point, null, MASK, want_sums, want_nodes)
    torch.cuda.synchronize()
    return (sums, node_sums, dev[1], dev[2], dev[3]), (want_sums, want_nodes)


def _check(N, C_, T, K, levels, has_null, start):
    book, issued, raw, clock = _case(N, C_, T, K, len(levels), start)
    (sums, node_sums, book_dev, issued_dev, clock_dev), (want_sums, want_nodes) = _score_both_ways(
        book, issued, raw, clock, T, levels, has_null)
    assert want_sums[T, 0] > 0, "the case settles nothing"
    assert (want_nodes[0, 0] == 0) == bool(has_null)             # the dead node counts only when 0 is a reading
    assert _same(sums, want_sums), "sums"
    assert _same(node_sums, want_nodes), "node_sums"
    assert _same(book_dev, book) and _same(issued_dev, issued) and _same(clock_dev, clock), "the score wrote its inputs"
    # the store: one row and its stamp, every other word as it was
    from ms_gat_amd import ops
    pred = torch.from_numpy(np.random.default_rng(N + T).standard_normal(book.shape[1:]).astype(np.float32)).to(DEV)
    pred[0, 0] = float("nan")
    for _ in range(2):                                           # twice for one origin: idempotent
        ops.forecast_store(pred, book_dev, issued_dev, clock_dev)
    store_ref(pred.cpu().numpy(), book, issued, clock)
    assert _same(book_dev, book) and _same(issued_dev, issued) and _same(clock_dev, clock), "store"


# ---- the kernels against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("has_null", [True, False])
@pytest.mark.parametrize("K", [1, 5, "T+2"])
@pytest.mark.parametrize("T", [1, 3, 12, 17, 64])
@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("N", [6, 40, 257, 300])
def test_point_heads_have_the_bits_of_the_restatement(N, C_, T, K, has_null):
    K = T + 2 if K == "T+2" else K
    _check(N, C_, T, K, (), has_null, start=2 ** 33 + 11 if C_ == 3 else 1000 + N)


@pytest.mark.parametrize("has_null", [True, False])
@pytest.mark.parametrize("K", [1, 5, "T+2"])
@pytest.mark.parametrize("levels,T", [(LEVELS3, 4), (LEVELS8, 8)], ids=["Q3", "Q8"])
@pytest.mark.parametrize("C_,N", [(1, 40), (3, 300)])
def test_quantile_heads_have_the_bits_of_the_restatement(C_, N, levels, T, K, has_null):
    K = T + 2 if K == "T+2" else K
    _check(N, C_, T, K, levels, has_null, start=2 ** 33 + 11 if C_ == 3 else 1000 + N)


@pytest.mark.parametrize("start", [3, 2 ** 32 + 7, 2 ** 40 + 1, 2 ** 62 - 9])
def test_start_steps_beyond_32_bits(start):
    _check(257, 3, 12, 5, (), True, start)


def test_a_book_of_exactly_t_out_rows_and_origins_near_zero():
    """P = T_out, the forecaster's choice; at start = 2 the origins of the larger horizons are negative and must not
    count, whatever the stamps say."""
    for start in (2, 500):
        book, issued, raw, clock = _case(300, 3, 12, 14, 0, start, extra_rows=0)
        assert (start == 2) == bool(((issued < 0) & (issued != NEVER)).any())     # stamps of negative origins
        got, want = _score_both_ways(book, issued, raw, clock, 12, (), True, calls=1)
        assert want[0][12, 0] > 0 and _same(got[0], want[0]) and _same(got[1], want[1]), start


@pytest.mark.parametrize("issued_kind", ["never", "negative"])
@pytest.mark.parametrize("now", [0, -5, -2 ** 40, 2 ** 62 + 3])
def test_cold_negative_and_wild_clocks_settle_nothing_and_stay_in_bounds(now, issued_kind):
    from ms_gat_amd import ops
    N, C_, T, K, P = 300, 3, 12, 14, 12
    book, _, raw, _ = _case(N, C_, T, K, 0, 100, extra_rows=0)
    issued = np.full(P, NEVER, np.int64) if issued_kind == "never" else -1 - np.arange(P, dtype=np.int64)[::-1].copy()
    clock = np.array([now, 0], np.int64)
    got, want = _score_both_ways(book, issued, raw, clock, T, (), True, calls=1)
    assert not want[0].any() and not want[1].any()
    assert not bool(got[0].any()) and not bool(got[1].any()), "something was settled"
    assert _same(got[0], want[0]) and _same(got[1], want[1])     # +0.0 everywhere, to the bit
    assert _same(got[2], book) and _same(got[3], issued) and _same(got[4], clock)
    # the store addresses a row inside the book for any clock; what it stamps there never counts for an origin < 0
    pred = torch.full((N, T), 7.0, device=DEV)
    ops.forecast_store(pred, got[2], got[3], got[4])
    store_ref(pred.cpu().numpy(), book, issued, clock)
    torch.cuda.synchronize()
    assert _same(got[2], book) and _same(got[3], issued)


def test_ops_check_their_arguments():
    from ms_gat_amd import ops
    book = torch.zeros(5, 40, 3, device=DEV)
    issued = torch.full((5,), NEVER, dtype=torch.int64, device=DEV)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    sums, node_sums = torch.zeros(4, 5, dtype=torch.float64, device=DEV), torch.zeros(40, 3, dtype=torch.float64, device=DEV)
    raw, pred = torch.ones(2, 3, 40, device=DEV), torch.ones(40, 3, device=DEV)
    score = lambda **kw: ops.forecast_score(**{**dict(raw=raw, book=book, issued=issued, clock=clock, t_out=3, sums=sums,  # noqa: E731
                                                      node_sums=node_sums), **kw})
    with pytest.raises(ValueError, match="pred"):
        ops.forecast_store(pred[:, :2].contiguous(), book, issued, clock)
    with pytest.raises(TypeError, match="issued"):
        ops.forecast_store(pred, book, issued.int(), clock)
    with pytest.raises(ValueError, match="issued"):
        ops.forecast_store(pred, book, issued[:4], clock)
    with pytest.raises(ValueError, match="clock"):
        ops.forecast_store(pred, book, issued, clock.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        ops.forecast_store(pred.t().contiguous().t(), book, issued, clock)
    with pytest.raises(ValueError, match="raw"):
        score(raw=raw[0])
    with pytest.raises(ValueError, match="agree in N"):
        score(raw=torch.ones(2, 3, 41, device=DEV))
    with pytest.raises(TypeError, match="sums"):
        score(sums=sums.float())
    with pytest.raises(ValueError, match="sums"):
        score(sums=torch.zeros(4, 13, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="node_sums"):
        score(node_sums=node_sums[:39])
    with pytest.raises(ValueError, match="out = 3"):
        score(t_out=1, levels=LEVELS3[:2], sums=torch.zeros(2, 11, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="P = 2"):
        score(book=book[:2].contiguous(), issued=issued[:2].contiguous())
    with pytest.raises(ValueError, match="quantile levels"):
        score(levels=(0.9, 0.1))
    with pytest.raises(ValueError, match="point"):
        score(t_out=1, levels=LEVELS3, point=3, sums=torch.zeros(2, 13, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="partials"):
        score(partials=torch.zeros(10, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="64"):
        score(t_out=65)
    score()
    torch.cuda.synchronize()
    assert not bool(sums.any()) and not bool(book.any()) and issued.tolist() == [NEVER] * 5


# ---- the forecaster ------------------------------------------------------------------------------------------------------
def _model(out, seed=0):
    import ms_gat_amd
    torch.manual_seed(seed)
    adj = ms_gat_amd.synthetic_adjacency(40, 60, seed=1)
    return ms_gat_amd.msgat48(n_components=3, in_channels=4, in_timesteps=4, out_timesteps=out, use_te=True,
                              adj=adj, missing_edges="scale").to(DEV)


class _Restated:
    """The book and totals the forecasts `step` returned must leave, by the numpy restatement."""

    def __init__(self, N, t_out, levels):
        self.t_out, self.levels, self.point = t_out, levels, 1 if levels else 0
        out = max(len(levels), 1) * t_out
        self.book, self.issued = np.zeros((t_out, N, out), np.float32), np.full(t_out, NEVER, np.int64)
        self.sums, self.nodes = np.zeros((t_out + 1, columns(len(levels)))), np.zeros((N, 3))
        self.live = False                                        # no book before the first forecast

    def step(self, t, reading, forecast):
        """The reading of step t arrives, then the forecast of origin t + 1 is issued."""
        if self.live:
            score_ref(reading[None], self.book, self.issued, np.array([t, 0]), self.t_out, self.levels, self.point,
                      NULL, MASK, self.sums, self.nodes)
        store_ref(forecast, self.book, self.issued, np.array([t + 1, 0]))
        self.live = True

    def holds(self, f, what):
        book, issued, sums, nodes = f._score_state
        assert _same(sums, self.sums), (what, "sums")
        assert _same(nodes, self.nodes), (what, "node_sums")
        assert _same(book, self.book) and _same(issued, self.issued), (what, "book")


@pytest.mark.parametrize("levels,t_out", [((), 3), (LEVELS3, 4)], ids=["point", "quantile"])
def test_graphed_and_eager_scores_have_the_bits_of_the_restatement(levels, t_out):
    from ms_gat_amd import OnlineForecaster, data
    tau, L = 4, 12
    raw = raw_series(3, 40)
    stats = data.series_stats(raw, HOURS, 3, tau, input_null_value=NULL)
    model = _model(max(len(levels), 1) * t_out, seed=len(levels))
    kw = dict(score=True, score_quantiles=levels or None, score_mask_value=MASK)
    graphed, eager = OnlineForecaster(model, stats, 0, **kw), OnlineForecaster(model, stats, 0, hip_graph=False, **kw)
    plain = OnlineForecaster(model, stats, 0)
    for f in (graphed, eager, plain):
        f.push(raw[:, :, :L - 1].permute(2, 0, 1))
    want = _Restated(40, t_out, levels)

    def run(first, stop):
        for t in range(first, stop):
            reading = raw[:, :, t]
            y = graphed.step(reading).clone()
            assert torch.equal(bits(y), bits(plain.step(reading))), ("scoring touched the forecast", t)
            assert torch.equal(bits(y), bits(eager.step(reading))), ("eager", t)
            want.step(t, reading.numpy(), y.cpu().numpy())

    run(L - 1, L + 13)
    graph = graphed._graph
    assert graph is not None and eager._graph is None
    want.holds(graphed, "graphed")
    want.holds(eager, "eager")
    assert (want.sums[:t_out, 0] > 0).all() and want.nodes[0, 0] == 0 and want.sums[t_out, 0] < 14 * 40 * t_out
    got = graphed.scores(at=[1, t_out])
    n = max(want.sums[t_out, 0], 1.0)
    assert got["count"] == want.sums[t_out, 0] and got["bias"] == pytest.approx(want.sums[t_out, 4] / n, rel=1e-12)
    assert got["horizons"]["count"] == [want.sums[0, 0], want.sums[t_out - 1, 0]] and ("quantiles" in got) == bool(levels)
    assert graphed.node_scores()[:, 0].tolist() == want.nodes[:, 0].tolist()
    # reset_scores() between replays of the captured graph: in place, the book stays
    for f in (graphed, eager):
        f.reset_scores()
    want.sums[:], want.nodes[:] = 0.0, 0.0
    run(L + 13, L + 19)
    want.holds(graphed, "graphed after the reset")
    want.holds(eager, "eager after the reset")
    assert want.sums[t_out, 0] > 0
    # load_state_dict() between replays: the graph goes on with what was loaded
    eager.reset_scores()
    for t in range(L + 19, L + 22):
        eager.step(raw[:, :, t])
    graphed.load_state_dict(eager.state_dict())
    plain.load_state_dict(eager.state_dict())
    for t in range(L + 22, L + 28):
        reading = raw[:, :, t]
        y = graphed.step(reading).clone()
        assert torch.equal(bits(y), bits(eager.step(reading))) and torch.equal(bits(y), bits(plain.step(reading))), t
    assert graphed._graph is graph
    for a, b in zip(graphed._score_state, eager._score_state):
        assert torch.equal(_words(a), _words(b))
    assert bool(graphed._score_state[2].any())
    assert set(plain.state_dict()) == {"ring", "clock", "start_step"}
