"""GPU: `msgat_interval_update` / `msgat_interval_apply` and `OnlineForecaster(score=True, intervals=...)` on the device.

Every cell of the interval state has one owner and the selection returns a window element, so window, cursor, radius,
radius_book, counts, lo and hi are compared BIT FOR BIT with the numpy restatement of tests/online_interval_ref.py (which
test_online_interval_cpu.py holds against a brute force that knows nothing of rings).  Shapes: 7 nodes x 3 horizons = 21
series leave a block of four waves with one wave of work; windows of 1, 5, 64, 65, 200 and 1024 values take every number
of registers per lane, with and without a tail in the last one."""
import numpy as np
import pytest
import torch

from online_fixtures import HOURS, NULL, bits, raw_series
from online_interval_ref import INF, NEVER, BruteForce, StandIn, apply_ref, fresh_state, store_ref, update_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEVELS4 = (0.5, 0.8, 0.9, 0.97)
NAMES = ("window", "cursor", "radius", "radius_book", "counts")


def _words(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    return got.dtype == want.dtype and torch.equal(_words(got), _words(want))


def _ranks(levels, W, min_count=None):
    from ms_gat_amd.intervals import interval_ranks
    return interval_ranks(levels, W, min_count).numpy()


class _Both:
    """The device state and the restated one, driven in lockstep: `issue` = forecast_store + interval_apply at the
    clock, `push` = interval_update with K readings and then the clock moves on by K."""

    def __init__(self, N, T, W, levels, P=None, start=1000, null=NULL, state=None, seed=0, grid=None):
        self.N, self.T, self.W, self.L, self.P, self.null = N, T, W, len(levels), P or T, null
        self.rng, self.grid = np.random.default_rng(100 * N + 10 * T + W + seed), grid
        self.ranks = _ranks(levels, W)
        self.book, self.issued = np.zeros((self.P, N, T), np.float32), np.full(self.P, NEVER, np.int64)
        self.state = list(state or fresh_state(self.L, N, T, W, self.P))
        self.lo, self.hi = np.zeros((self.L, N, T), np.float32), np.zeros((self.L, N, T), np.float32)
        self.clock = np.array([start, 0], np.int64)
        self.valid = np.zeros(N, np.int64)                       # valid readings made so far, per node
        up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
        self.d_ranks, self.d_book, self.d_issued, self.d_clock = up(self.ranks), up(self.book), up(self.issued), up(self.clock)
        self.d_state, self.d_lo, self.d_hi = [up(a) for a in self.state], up(self.lo), up(self.hi)

    def forecast(self):
        p = 60 + 25 * self.rng.standard_normal((self.N, self.T))
        return (np.round(p / self.grid) * self.grid if self.grid else p).astype(np.float32)

    def readings(self, K, C_=2):
        raw = np.maximum(60 + 20 * self.rng.standard_normal((K, C_, self.N)), 1.0)
        raw = (np.round(raw / self.grid) * self.grid if self.grid else raw).astype(np.float32)
        raw[self.rng.random((K, C_, self.N)) < 0.1] = NULL
        raw[:, :, 0] = NULL                                      # a dead node
        if self.rng.random() < 0.05:
            raw[0, 0, self.N // 2] = np.nan
        self.valid += (~np.isnan(raw[:, 0]) & (raw[:, 0] != NULL)).sum(0)
        return raw

    def issue(self, pred=None):
        from ms_gat_amd import intervals, ops
        pred = self.forecast() if pred is None else pred
        d_pred = torch.from_numpy(pred).to(DEV)
        ops.forecast_store(d_pred, self.d_book, self.d_issued, self.d_clock)
        intervals.interval_apply(d_pred, self.d_state[2], self.d_clock, self.d_lo, self.d_hi, self.d_state[3])
        store_ref(pred, self.book, self.issued, self.clock)
        apply_ref(pred, self.state[2], self.clock, self.lo, self.hi, self.state[3])

    def update(self, raw, device_only=False):
        from ms_gat_amd import intervals
        window, cursor, radius, radius_book, counts = self.d_state
        intervals.interval_update(torch.from_numpy(raw).to(DEV), self.d_book, self.d_issued, self.d_clock, radius_book,
                                  self.d_ranks, window, cursor, radius, counts, null_value=self.null)
        if not device_only:
            window, cursor, radius, radius_book, counts = self.state
            update_ref(raw, self.book, self.issued, self.clock, radius_book, self.ranks, window, cursor, radius, counts,
                       0, self.null)

    def advance(self, K):
        self.clock[0] += K
        self.d_clock.copy_(torch.from_numpy(self.clock))

    def push(self, K=1):
        self.update(self.readings(K))
        self.advance(K)

    def holds(self, what=""):
        torch.cuda.synchronize()
        for name, got, want in zip(NAMES + ("lo", "hi", "book", "issued", "clock", "ranks"),
                                   self.d_state + [self.d_lo, self.d_hi, self.d_book, self.d_issued, self.d_clock,
                                                   self.d_ranks],
                                   self.state + [self.lo, self.hi, self.book, self.issued, self.clock, self.ranks]):
            assert _same(got, want), (what, name)


# ---- the kernels against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [(0.8,), LEVELS4], ids=["L1", "L4"])
@pytest.mark.parametrize("W", [1, 5, 64, 65, 200])
@pytest.mark.parametrize("T", [3, 12])
def test_a_stream_of_steps_has_the_bits_of_the_restatement(T, W, levels):
    """A forecast and a reading per step until every live series has been inserted into more than 2W + 3 times: the
    cursor fills its window, wraps from 2W back to W and goes round again."""
    both = _Both(7, T, W, levels, P=T + (W % 3))
    steps = int((2 * W + 3 + T) / 0.7) + 10                      # a tenth of the readings are null
    for t in range(steps):
        both.issue()
        both.push()
        if t in (0, 1, T, W, 2 * W):
            both.holds(t)
    both.holds("end")
    window, cursor, radius, radius_book, counts = both.state
    assert both.valid[1:].min() - T > 2 * W + 3, "a live series was not inserted into often enough"
    assert (cursor[1:] >= W).all() and (cursor[1:] < 2 * W).all() and not cursor[0].any()
    assert not counts[:, 0].any() and np.isinf(radius[:, 0]).all()
    for l in range(len(levels)):                                 # a level whose rank never exists has no interval at all
        assert np.isfinite(radius[l, 1:]).all() == (both.ranks[l, W] > 0) == (not np.isinf(radius[l, 1:]).any())
        assert (counts[l, 1:, :, 0] > 0).all() == bool(both.ranks[l].any()) == bool(counts[l, ..., 0].any())
    assert 0 < counts[..., 1].sum() < counts[..., 0].sum() or not both.ranks[:, W].any()


@pytest.mark.parametrize("levels", [(0.8,), LEVELS4], ids=["L1", "L4"])
@pytest.mark.parametrize("T", [3, 12])
def test_a_full_window_of_1024_about_to_wrap(T, levels):
    W, N = 1024, 7
    rng = np.random.default_rng(T)
    state = list(fresh_state(len(levels), N, T, W, T))
    state[0][:] = np.abs(30 * rng.standard_normal((N, T, W))).astype(np.float32)
    state[1][:] = 2 * W - 2
    state[1][3] = rng.integers(0, 2 * W, T)                      # one node anywhere, some of its windows not yet full
    both = _Both(N, T, W, levels, state=state)
    both.update(both.readings(1))                                # nothing is due yet: the radii of the prepared windows
    both.holds("radii")
    assert np.isfinite(both.state[2][:, 1]).all()
    for t in range(T + 4):
        both.issue()
        both.push()
    both.holds("end")
    assert both.valid[1] >= 3 and W <= both.state[1][1, 0] < W + T + 3      # 2W - 2, 2W - 1, then W, W + 1, ...


@pytest.mark.parametrize("W", [5, 65])
def test_ties_and_exact_zeros(W):
    """Forecasts and readings on a grid (0.5 and, for more ties in a window of 5, 5.0): many errors are equal, exact
    zeros among them."""
    both = _Both(7, 3, W, LEVELS4, grid=0.5 if W > 5 else 5.0)
    both.forecast = lambda: np.full((7, 3), 60.0, np.float32)    # readings are 60 +- 20 on the grid: plenty meet it
    for t in range(2 * W + 12):
        both.issue()
        both.push()
    both.holds("ties")
    window = both.state[0][1:]
    assert (window == 0).any() and len(np.unique(window)) < window.size // 2
    assert any(len(np.unique(w)) < W for w in window.reshape(-1, W))
    assert (both.state[4][..., 1] > 0).any()


@pytest.mark.parametrize("W", [5, 200])
def test_one_call_with_five_readings_equals_five_calls_with_one(W):
    T, K, N = 3, 5, 7
    P = T + K + 1

    def prepared(seed):
        both = _Both(N, T, W, LEVELS4, P=P, seed=seed)
        for t in range(W + 3):                                   # windows in mid-flight
            both.issue()
            both.push()
        for o in range(int(both.clock[0]), int(both.clock[0]) + K):   # origins "inside" the readings, stamped ahead
            both.issued[o % P] = o
            both.state[3][o % P] = np.where(both.rng.random((4, N, T)) < 0.3, INF, 40.0).astype(np.float32)
        both.book[:] = (60 + 25 * both.rng.standard_normal(both.book.shape)).astype(np.float32)
        both.d_book.copy_(torch.from_numpy(both.book))
        both.d_issued.copy_(torch.from_numpy(both.issued))
        both.d_state[3].copy_(torch.from_numpy(both.state[3]))
        return both

    once, five = prepared(1), prepared(1)
    raw = once.readings(K)
    once.update(raw)
    once.holds("K = 5")
    for k in range(K):
        five.update(raw[k: k + 1].copy(), device_only=True)
        five.advance(1)
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, once.d_state, five.d_state):
        assert _same(a, b), name
    assert int(once.state[4][..., 0].sum()) > 0


def test_cold_negative_and_wild_clocks_and_an_unstamped_book_change_nothing():
    N, T, W = 7, 3, 5
    both = _Both(N, T, W, LEVELS4)
    for t in range(W + 2):
        both.issue()
        both.push()
    both.holds()
    before = [t.clone() for t in both.d_state]
    raw = both.readings(4)
    stamps = both.issued.copy()
    for issued in (stamps, np.full(T, NEVER, np.int64), np.array([-3, -2, -1], np.int64)):
        for now in (0, -2, -7, 2 ** 62 + 1, 2 ** 63 - 2, -2 ** 63):
            both.d_issued.copy_(torch.from_numpy(issued))
            both.d_clock.copy_(torch.tensor([now, 0]))
            both.update(raw, device_only=True)
            torch.cuda.synchronize()
            for name, a, b in zip(NAMES, both.d_state, before):
                assert _same(a, b), (name, now, issued)
    # the apply at a wild clock: the row its floor-mod names, nothing else
    for now in (-7, 2 ** 62 + 1, -2 ** 63):
        both.clock[0] = now
        both.d_clock.copy_(torch.from_numpy(both.clock))
        both.d_issued.copy_(torch.from_numpy(both.issued))
        both.issue()
        both.holds(now)


def test_a_wild_cursor_word_stays_inside_its_window():
    N, T, W = 7, 3, 5
    guarded = torch.full((N + 2, T, W), -77.0, device=DEV)
    both = _Both(N, T, W, LEVELS4)
    both.state[1][:] = np.array([-1, -2 ** 31, 2 ** 31 - 1, 3 * W + 2, -7, 2 * W, 123456789], np.int32)[:, None]
    both.d_state[1].copy_(torch.from_numpy(both.state[1]))
    both.d_state[0] = guarded[1:-1]                              # the window between two rows that must stay as they are
    both.d_state[0].zero_()
    for t in range(2 * W + 3):
        both.issue()
        both.push()
    both.holds("wild cursors")
    assert bool((guarded[0] == -77.0).all()) and bool((guarded[-1] == -77.0).all())
    cursor = both.state[1].astype(np.int64)
    assert ((cursor[1:] >= W) & (cursor[1:] < 2 * W)).all() and cursor[0, 0] == -1      # the dead node's word stays


def test_a_nan_forecast_is_judged_as_missed_and_not_inserted():
    N, T, W = 7, 3, 5
    both = _Both(N, T, W, (0.5,))
    for t in range(6):
        both.issue()
        both.push()
    pred = both.forecast()
    pred[2] = np.nan                                             # node 2, every horizon; its issued radii are finite
    both.issue(pred)
    assert np.isfinite(both.state[3][int(both.clock[0]) % T, 0, 2, 0]) and np.isnan(both.lo[0, 2]).all()
    cursor, counts = both.state[1].copy(), both.state[4].copy()
    raw = both.readings(1)
    raw[0, 0, 2] = 55.0
    both.update(raw)
    both.holds("NaN forecast")
    assert both.state[1][2, 0] == cursor[2, 0] and both.state[1][1, 0] >= cursor[1, 0]
    assert both.state[4][0, 2, 0].tolist() == [counts[0, 2, 0, 0] + 1, counts[0, 2, 0, 1]]


@pytest.mark.parametrize("T,L", [(3, 1), (12, 4)])
def test_apply_writes_every_element_whatever_was_there(T, L):
    from ms_gat_amd import intervals
    N, P = 7, T + 2
    rng = np.random.default_rng(T)
    pred = torch.from_numpy((60 + 25 * rng.standard_normal((N, 2 * T))).astype(np.float32)).to(DEV)
    radius = np.abs(10 * rng.standard_normal((L, N, T))).astype(np.float32)
    radius[:, 0] = INF
    clock = torch.tensor([1000, 0], device=DEV)
    found = []
    for fill in (0.0, float("nan"), 12345.0):
        lo, hi = torch.full((L, N, T), fill, device=DEV), torch.full((L, N, T), fill, device=DEV)
        radius_book = torch.full((P, L, N, T), fill, device=DEV)
        for _ in range(2):                                       # twice at one origin: idempotent
            intervals.interval_apply(pred, torch.from_numpy(radius).to(DEV), clock, lo, hi, radius_book, point=1)
        torch.cuda.synchronize()
        rows = [r for r in range(P) if r != 1000 % P]
        assert _same(radius_book[rows], torch.full((P - 1, L, N, T), fill))
        found.append((lo, hi, radius_book[1000 % P].clone()))
    want_lo, want_hi = np.zeros((L, N, T), np.float32), np.zeros((L, N, T), np.float32)
    want_book = np.zeros((P, L, N, T), np.float32)
    apply_ref(pred.cpu().numpy(), radius, np.array([1000, 0]), want_lo, want_hi, want_book, point=1)
    for lo, hi, row in found:
        assert _same(lo, want_lo) and _same(hi, want_hi) and _same(row, want_book[1000 % P])
    assert bool(torch.isinf(found[0][0][:, 0]).all())


def test_the_bindings_check_their_operands():
    from ms_gat_amd import intervals
    both = _Both(7, 3, 5, LEVELS4)
    raw = torch.from_numpy(both.readings(1)).to(DEV)
    window, cursor, radius, radius_book, counts = both.d_state

    def update(**kw):
        a = dict(raw=raw, book=both.d_book, issued=both.d_issued, clock=both.d_clock, radius_book=radius_book,
                 ranks=both.d_ranks, window=window, cursor=cursor, radius=radius, counts=counts)
        a.update(kw)
        intervals.interval_update(**a)

    with pytest.raises(TypeError, match="cursor"):
        update(cursor=cursor.long())
    with pytest.raises(ValueError, match="ranks"):
        update(ranks=both.d_ranks[:, :-1].contiguous())
    with pytest.raises(ValueError, match="counts"):
        update(counts=counts[:, :, :, :1].contiguous())
    with pytest.raises(ValueError, match="raw"):
        update(raw=raw[:, :, :6].contiguous())
    with pytest.raises(ValueError, match="window"):
        update(window=torch.zeros(7, 3, 1025, device=DEV))
    with pytest.raises(ValueError, match="share one device"):
        update(radius=radius.cpu())
    with pytest.raises(ValueError, match="level 1"):
        update(point=1)
    with pytest.raises(Exception, match="GPU only"):
        update(book=both.d_book.cpu())
    update()
    torch.cuda.synchronize()


# ---- the forecaster --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantiles,t_out", [((), 3), ((0.1, 0.5, 0.9), 2)], ids=["point", "quantile"])
def test_graphed_and_eager_intervals_are_the_same_bits_and_the_brute_force(quantiles, t_out):
    from ms_gat_amd import OnlineForecaster, data
    tau, hist, W, levels = 4, 12, 4, (0.5, 0.8)
    raw = raw_series(3, 9)
    total = raw.shape[-1]
    stats = data.series_stats(raw, HOURS, 3, tau, input_null_value=NULL)
    torch.manual_seed(3)
    model = StandIn(stats.input_channels, max(len(quantiles), 1) * t_out, tau).to(DEV)
    kw = dict(score=True, score_quantiles=quantiles or None, intervals=levels, interval_window=W)
    graphed, eager = OnlineForecaster(model, stats, 0, **kw), OnlineForecaster(model, stats, 0, hip_graph=False, **kw)
    plain = OnlineForecaster(model, stats, 0, score=True, score_quantiles=quantiles or None)
    for f in (graphed, eager, plain):
        f.push(raw[:, :, :hist - 1].permute(2, 0, 1))
    brute = BruteForce(raw.numpy(), t_out, levels, W, point=1 if quantiles else 0, null_value=NULL)

    def agree(what):
        for name, a, b in zip(NAMES, graphed._interval_state, eager._interval_state):
            assert _same(a, b), (what, name)
        for a, b in zip(graphed._score_state, eager._score_state):
            assert _same(a, b), (what, "score state")

    def run(first, stop, judge=True):
        for t in range(first, stop):
            reading = raw[:, :, t]
            y = graphed.step(reading).clone()
            assert torch.equal(bits(y), bits(plain.step(reading))), ("the intervals touched the forecast", t)
            assert torch.equal(bits(y), bits(eager.step(reading))), ("eager", t)
            for a, b in zip(graphed.intervals(), eager.intervals()):
                assert _same(a, b), ("lo, hi", t)
            if judge:
                brute.push(t)
                want_lo, want_hi, _ = brute.issue(t + 1, y.cpu().numpy())
                assert _same(graphed.intervals()[0], want_lo) and _same(graphed.intervals()[1], want_hi), t

    def holds(f):
        window, cursor, radius, radius_book, counts = f._interval_state
        assert _same(radius, brute.radius()) and _same(counts, brute.counts()) and _same(cursor, brute.cursor())

    run(hist - 1, hist + 20)
    graph, state = graphed._graph, graphed._interval_state
    assert graph is not None and eager._graph is None
    agree("first stretch")
    holds(graphed)
    assert brute.judged.sum() > 0 and brute.inserts().max() >= 2 * W and brute.null_masked > 0
    got = graphed.interval_scores(at=[1, t_out])
    assert got["judged"] == brute.judged.sum((1, 2)).tolist() and len(got["horizons"]["width"][0]) == 2
    assert got["coverage"] == pytest.approx((brute.covered.sum((1, 2)) / brute.judged.sum((1, 2))).tolist(), rel=1e-12)
    nodes = graphed.interval_node_scores()
    assert tuple(nodes.shape) == (9, 2) and bool(torch.isnan(nodes[0]).all()) and bool((nodes[3:] >= 0).all())
    # reset_scores() between replays of the captured graph: in place, windows and radii stay
    for f in (graphed, eager):
        f.reset_scores()
    brute.judged[:], brute.covered[:] = 0, 0
    run(hist + 20, hist + 27)
    assert graphed._interval_state is state and graphed._graph is graph
    agree("after the reset")
    holds(graphed)
    assert brute.judged.sum() > 0
    # load_state_dict() between replays: the graph goes on with what was loaded
    for t in range(hist + 27, hist + 30):
        eager.step(raw[:, :, t])
    graphed.load_state_dict(eager.state_dict())
    plain.load_state_dict({k: v for k, v in eager.state_dict().items() if not k.startswith("interval_")})
    run(hist + 30, total, judge=False)
    assert graphed._graph is graph and graphed._interval_state is state
    agree("after the load")
    assert set(plain.state_dict()) == {"ring", "clock", "start_step", "book", "issued", "score_sums", "score_node_sums"}
