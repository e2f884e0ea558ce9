"""Online forecasting: a trained model beside the sensors -- every new reading yields the next `T_out` steps.

The history lives on the model's device as a ring of normalised readings (`ops.ring_push`) and the model's inputs are
built there for the one origin "now" (`ops.ring_windows`): a reading goes in and a forecast comes out, on the GPU as one
replayed HIP graph, with no host arithmetic and nothing read back.  The reference has no counterpart: its loader
(data_loader.py:92-120) slices a series that exists in full and does not keep the statistics it normalised with;
`data.SeriesStats` keeps them.
"""
from __future__ import annotations

import torch
from torch import nn

from . import data as _data


class OnlineForecaster:
    """`f = OnlineForecaster(model, stats, start_step)`; then `y = f.step(reading)` per reading.

    `model`: any `nn.Module` called as `model(X, H, D)` -> [1, N, out] (`MSGAT` with any `learn_edge_weights`,
    `missing_edges` or a quantile head); it is put in `eval()` and run under `torch.no_grad()`, so `edge_dropout` draws
    nothing.  `stats`: the `data.SeriesStats` of the training series (`data.series_stats` with the arguments
    `make_loaders` got): normalisation, imputation table, validity channel, hours and tau.

    `start_step` is the ABSOLUTE index, on the time base of the training series, of the first reading pushed: step 0 is
    the first step of the training file, and the reading that follows the file's last has index `T_total`.  It fixes the
    hour of day, the day of week and the slot of the imputation table of every reading from then on, exactly as the
    loaders derived them from a window's position in the file -- a wrong `start_step` shifts all three silently (nothing
    can check it), so derive it from timestamps: (time of the first pushed reading - time of the file's first step) /
    sampling interval.  Readings must be pushed in order, one per step, none left out (a sensor that is down is a
    missing VALUE, `stats.input_null_value` or NaN, not a missing step).

    `push(reading)`: raw (un-normalised) float32 [C,N] or [K,C,N] for K consecutive steps, on the host or on the model's
    device.  `ready`: the ring holds the `history = tau * max(hours)` readings a forecast needs (counted on the host).
    `forecast()` -> [N, out] on the model's device for the origin right after the last reading; RuntimeError before
    `ready`.  `step(reading)` = push of one reading + forecast.  `capacity`: rows of the ring, a multiple of tau and at
    least `history` (the default).

    On a GPU model with `hip_graph` "auto" or True, `step` replays ONE captured graph -- push, clock advance, windows,
    model forward -- after copying the reading into a static buffer; it is captured at the first `step` that can
    forecast.  The tensor `step` returns is then STATIC: the next `step` overwrites it, so clone what must outlive it.
    `push` of several readings and a bare `forecast()` launch the same kernels eagerly.  A CPU model runs the torch
    restatements (`data._ring_push_torch`, `data._ring_windows_torch`).

    `state_dict()` / `load_state_dict()`: ring, clock and start_step -- a restarted service resumes where it stopped.
    One process, one origin per step: multi-rank serving and batched origins are not provided.

    `score=True` keeps a book of the forecasts it returned and settles it as their readings arrive, on the device
    (`ops.forecast_store` / `ops.forecast_score`): the forecast of origin o is due at horizon h when the reading of step
    o + h is pushed, its truth is channel 0 of that raw reading, valid unless NaN or equal to `score_null_value` (default
    `stats.input_null_value`).  `push` settles its K readings before it normalises them, `forecast()` and `step()` store
    what they return (`forecast()` twice at one origin changes nothing), and the captured step becomes score -> push ->
    advance -> windows -> forward -> store: still ONE replay, three more kernels.  The head's width must be Q * T_out
    with Q = len(`score_quantiles`) (1 for a point head), else ValueError at the first forecast, which sizes the book
    (T_out rows).  `scores(at=None)` reads the totals back once: {"count", "MAE", "MAPE", "RMSE", "bias", "horizons":
    {the same as lists per horizon; `at=[3, 6, 12]` picks those 1-based steps}} with `Metrics`' definitions over the
    valid entries, "bias" the mean signed error p - y, and for `score_quantiles` "quantiles": {levels, coverage, pinball,
    crossing, width} as `Metrics.quantile_summary()` gives them.  `node_scores()` -> float64 [N, 3] on the host: count,
    MAE and bias per sensor over all horizons, NaN where the count is 0.  `reset_scores()` zeroes the totals in place (the
    book stays: forecasts in flight are still settled).  `state_dict()` then also holds book, issued, score_sums and
    score_node_sums; a state without them loads as a cold book with zero totals.  Without `score` there is no buffer, no
    state key and no launch of all this.

    `intervals=0.9` or `(0.8, 0.95)` (needs `score=True`: it reads the scoring book) adds calibrated prediction intervals
    around the point forecast, for any trained point model and with no retraining: rolling split-conformal half-widths
    (`intervals.py`, csrc/online_interval.hip).  One to four nominal coverage levels, strictly increasing inside (0, 1).
    Per sensor and horizon the last `interval_window` = W (1 .. 1024) VALID settled absolute errors are kept on the device,
    and the half-width r of level c is the `ceil((m + 1) c)`-th smallest of the m held (`intervals.interval_ranks`); while
    that rank does not exist, or m < `interval_min_count`, the series has no interval: r = +inf.  Under exchangeable
    errors the interval covers with probability at least c.  `intervals()` -> `(lo, hi)`, each [L, N, T_out] on the
    model's device, of the forecast most recently returned: lo = p - r, hi = p + r (static tensors on the captured path,
    like the forecast; RuntimeError before the first forecast).  With a `score_quantiles` head the interval is around the
    point level (`score_point`); conformalising the model's own quantile levels (CQR) is not provided.  Every settled
    error is first JUDGED against the radii issued with its forecast, then inserted: `interval_scores(at=None)` reads
    back once {"levels", "judged", "coverage", "width", "horizons": {the same per horizon}} -- coverage[l] = covered /
    judged over the issued intervals that have settled, width[l] the mean 2 r over the series that now have a finite
    radius (NaN where there is nothing to divide by) -- and `interval_node_scores()` -> float64 [N, L], the coverage per
    sensor over all horizons, NaN where nothing was judged.  `reset_scores()` also zeroes the judged and covered counts
    (windows and radii stay); `state_dict()` also holds interval_window, interval_cursor, interval_radius, interval_book
    and interval_counts, and a state without them loads as empty windows, +inf radii and zero counts.  The captured step
    becomes score -> interval update -> push -> advance -> windows -> forward -> store -> interval apply: still ONE replay,
    two more kernels.  With `intervals=None` there is no buffer, no state key and no launch of all this."""

    def __init__(self, model: nn.Module, stats: "_data.SeriesStats", start_step: int, capacity: int | None = None,
                 hip_graph="auto", score: bool = False, score_quantiles=None, score_null_value="stats",
                 score_mask_value: float = 0.0, intervals=None, interval_window: int = 288, interval_min_count=None):
        if hip_graph not in (True, False, "auto"):
            raise ValueError(f"hip_graph must be True, False or 'auto', not {hip_graph!r}")
        tensors = list(model.parameters()) + list(model.buffers())
        self.device = tensors[0].device if tensors else torch.device("cpu")
        on_gpu = self.device.type == "cuda"
        if hip_graph is True and not on_gpu:
            raise ValueError("hip_graph=True needs the model on the GPU")
        self.hip_graph = bool(hip_graph) and on_gpu
        if int(start_step) < 0:
            raise ValueError(f"start_step = {start_step} must be >= 0: step 0 is the first step of the training series")
        self.model, self.stats, self.start_step = model.eval(), stats, int(start_step)
        C_, N = stats.mean.shape
        if tuple(stats.std.shape) != (C_, N):
            raise ValueError(f"stats.std {tuple(stats.std.shape)} must have the shape of stats.mean [{C_}, {N}]")
        self.mask_channel = bool(stats.mask_channel) and stats.climatology is not None
        if stats.input_channels != C_ + int(self.mask_channel):
            raise ValueError(f"stats.input_channels = {stats.input_channels} does not fit its {C_} channels and "
                             f"mask_channel = {self.mask_channel}")
        wanted = getattr(model, "in_channels", None)
        if wanted is None and hasattr(model, "tpcs"):          # an MSGAT: its first block's input width
            wanted = getattr(model.tpcs[0].tgacns[0], "in_channels", None)
        if wanted is not None and int(wanted) != stats.input_channels:
            raise ValueError(f"stats.input_channels = {stats.input_channels} but the model takes in_channels = {wanted}")
        self.hours, self.tau, self.history = list(stats.hours), int(stats.tau), stats.history
        self.capacity = self.history if capacity is None else int(capacity)
        if self.capacity < self.history or self.capacity % self.tau:
            raise ValueError(f"capacity = {capacity} must be a multiple of tau = {self.tau} and at least the history "
                             f"tau * max(hours) = {self.history}")
        dev = self.device
        self.n_channels, self.n_nodes = C_, N
        self.mean, self.std = stats.mean.to(dev).contiguous(), stats.std.to(dev).contiguous()
        self.climatology = None if stats.climatology is None else stats.climatology.to(dev).contiguous()
        self.ring = torch.full((self.capacity, C_, N), float("nan"), dtype=torch.float32, device=dev)
        self.clock = torch.tensor([self.start_step, 0], dtype=torch.int64).to(dev)
        self.resident_bytes = self.ring.numel() * 4
        self._pushed = 0                      # host mirror of clock[1] before it saturates: nothing is read back
        self._graph = self._prediction = None
        self.score = bool(score)
        self._score_state = None              # (book, issued, sums, node_sums), sized by the first forecast
        if self.score:
            from . import ops
            self.score_levels = () if score_quantiles is None else ops.quantile_levels(score_quantiles)
            self.score_point = ops.quantile_point(self.score_levels) if self.score_levels else 0
            null = stats.input_null_value if isinstance(score_null_value, str) else score_null_value   # "stats"
            self.score_null_value = None if null is None else float(null)
            self.score_mask_value = float(score_mask_value)
        self.interval_levels = ()
        self._interval_state = None           # (window, cursor, radius, radius_book, counts), sized with the book
        if intervals is not None:
            from . import intervals as _intervals
            if not self.score:
                raise ValueError("intervals needs score=True: it is calibrated on the errors the scoring book settles")
            self.interval_levels = _intervals.interval_levels(intervals)
            self.interval_window = int(interval_window)
            self._interval_ranks = _intervals.interval_ranks(self.interval_levels, interval_window,
                                                             interval_min_count).to(self.device)
            self._interval_out = None         # (lo, hi) of the forecast most recently returned
            self._interval_issued = False
        if on_gpu:
            from . import ops
            self._offsets = ops.window_offsets(self.hours, self.tau, dev)
            self._reading = torch.zeros((1, C_, N), dtype=torch.float32, device=dev)
            self._out = self._window_buffers()

    def _window_buffers(self):
        x = torch.zeros((1, len(self.hours), self.stats.input_channels, self.n_nodes, self.tau), dtype=torch.float32,
                        device=self.device)
        hd = torch.zeros((2, 1), dtype=torch.int64, device=self.device)
        return x, hd[0], hd[1]

    # ---- the three pieces, on whichever state they are handed (the live one, or a scratch copy to warm up on) ----------
    def _push(self, reading: torch.Tensor, ring: torch.Tensor, clock: torch.Tensor) -> None:
        if self.device.type == "cuda":
            from . import ops
            ops.ring_push(reading, self.mean, self.std, ring, clock, null_value=self.stats.input_null_value)
        else:
            _data._ring_push_torch(reading, self.mean, self.std, ring, clock, null_value=self.stats.input_null_value)

    def _windows(self, ring: torch.Tensor, clock: torch.Tensor, out=None):
        if self.device.type == "cuda":
            from . import ops
            return ops.ring_windows(ring, clock, self.hours, self.tau, climatology=self.climatology,
                                    mask_channel=self.mask_channel, offsets=self._offsets, out=out)
        return _data._ring_windows_torch(ring, clock, self.hours, self.tau, climatology=self.climatology,
                                         mask_channel=self.mask_channel)

    def _forward(self, batch) -> torch.Tensor:
        with torch.no_grad():
            return self.model(*batch)[0]

    # ---- scoring: the book of issued forecasts and its totals, on whichever state they are handed -------------------------
    def _score_setup(self, out: int) -> None:
        """Sizes book and totals for a head of `out` outputs per node (the first forecast knows it); cold and zero."""
        if self._score_state is not None:
            if self._score_state[0].shape[2] != out:
                raise ValueError(f"the model's head has {out} outputs per node, the book was sized for "
                                 f"{self._score_state[0].shape[2]}")
            return
        from . import ops
        n_levels = max(len(self.score_levels), 1)
        if out % n_levels or not 1 <= out <= 64:
            raise ValueError(f"score=True: the model's head has {out} outputs per node, which is not Q * T_out for Q = "
                             f"{n_levels} level(s) with Q * T_out <= 64")
        self.score_t_out = out // n_levels
        dev, N = self.device, self.n_nodes
        self._score_state = (torch.zeros((self.score_t_out, N, out), dtype=torch.float32, device=dev),
                             torch.full((self.score_t_out,), ops.SCORE_NEVER, dtype=torch.int64, device=dev),
                             torch.zeros((self.score_t_out + 1, ops.score_columns(len(self.score_levels))),
                                         dtype=torch.float64, device=dev),
                             torch.zeros((N, ops.SCORE_NODE_COLUMNS), dtype=torch.float64, device=dev))
        if dev.type == "cuda":
            need = int(ops._lib.checked().msgat_forecast_score_partial_doubles(N, self.score_t_out, len(self.score_levels)))
            self._score_partials = torch.empty(need, dtype=torch.float64, device=dev)
        if self.interval_levels:
            from . import intervals as _intervals
            n_levels = len(self.interval_levels)
            self._interval_state = _intervals.interval_state(n_levels, N, self.score_t_out, self.interval_window,
                                                             self.score_t_out, dev)
            self._interval_out = self._interval_buffers()

    def _interval_buffers(self):
        shape = (len(self.interval_levels), self.n_nodes, self.score_t_out)
        return (torch.zeros(shape, dtype=torch.float32, device=self.device),
                torch.zeros(shape, dtype=torch.float32, device=self.device))

    def _calibrate(self, reading: torch.Tensor, state, calibration, clock: torch.Tensor) -> None:
        """The readings' settled errors: judged against the radii issued with their forecasts, then into the windows."""
        from . import intervals as _intervals
        window, cursor, radius, radius_book, counts = calibration
        fn = _intervals.interval_update if self.device.type == "cuda" else _intervals._interval_update_torch
        fn(reading, state[0], state[1], clock, radius_book, self._interval_ranks, window, cursor, radius, counts,
           point=self.score_point, null_value=self.score_null_value)

    def _apply(self, pred: torch.Tensor, calibration, out, clock: torch.Tensor) -> None:
        from . import intervals as _intervals
        fn = _intervals.interval_apply if self.device.type == "cuda" else _intervals._interval_apply_torch
        fn(pred.contiguous(), calibration[2], clock, out[0], out[1], calibration[3], point=self.score_point)

    def _settle(self, reading: torch.Tensor, state, clock: torch.Tensor) -> None:
        book, issued, sums, node_sums = state
        kw = dict(levels=self.score_levels or None, point=self.score_point, null_value=self.score_null_value,
                  mask_value=self.score_mask_value)
        if self.device.type == "cuda":
            from . import ops
            ops.forecast_score(reading, book, issued, clock, self.score_t_out, sums, node_sums,
                               partials=self._score_partials, **kw)
        else:
            kw["levels"] = self.score_levels
            _data._forecast_score_torch(reading, book, issued, clock, self.score_t_out, sums, node_sums, **kw)

    def _store(self, pred: torch.Tensor, state, clock: torch.Tensor) -> None:
        if self.device.type == "cuda":
            from . import ops
            ops.forecast_store(pred.contiguous(), state[0], state[1], clock)
        else:
            _data._forecast_store_torch(pred, state[0], state[1], clock)

    # ---- public ------------------------------------------------------------------------------------------------------
    @property
    def ready(self) -> bool:
        return self._pushed >= self.history

    def _checked(self, reading: torch.Tensor) -> torch.Tensor:
        if not torch.is_tensor(reading) or reading.dtype != torch.float32:
            raise ValueError("reading must be a float32 tensor of raw (un-normalised) values")
        C_, N = self.n_channels, self.n_nodes
        if reading.dim() == 2:
            reading = reading[None]
        if reading.dim() != 3 or tuple(reading.shape[1:]) != (C_, N) or reading.shape[0] < 1:
            raise ValueError(f"reading {tuple(reading.shape)} must be [{C_}, {N}] or [K, {C_}, {N}]")
        if reading.shape[0] > self.capacity:
            raise ValueError(f"reading holds K = {reading.shape[0]} steps, more than the ring's capacity {self.capacity}")
        if reading.device.type != "cpu" and reading.device != self.device:
            raise ValueError(f"reading is on {reading.device}, the model on {self.device}: pass a host tensor or one on "
                             f"the model's device")
        return reading

    def push(self, reading: torch.Tensor) -> None:
        reading = self._checked(reading).to(self.device).contiguous()
        if self._score_state is not None:     # before the push: the clock still names the first of these steps
            self._settle(reading, self._score_state, self.clock)
            if self._interval_state is not None:
                self._calibrate(reading, self._score_state, self._interval_state, self.clock)
        self._push(reading, self.ring, self.clock)
        self._pushed = min(self._pushed + reading.shape[0], self.capacity)

    def forecast(self) -> torch.Tensor:
        if not self.ready:
            raise RuntimeError(f"forecast() needs {self.history} readings in the ring, {self._pushed} were pushed")
        out = self._out if self.device.type == "cuda" else None
        pred = self._forward(self._windows(self.ring, self.clock, out=out))
        if self.score:
            self._score_setup(pred.shape[-1])
            self._store(pred, self._score_state, self.clock)
            if self.interval_levels:
                self._apply(pred, self._interval_state, self._interval_out, self.clock)
                self._interval_issued = True
        return pred

    def step(self, reading: torch.Tensor) -> torch.Tensor:
        reading = self._checked(reading)
        if not self.hip_graph or reading.shape[0] != 1 or self._pushed + 1 < self.history:
            self.push(reading)
            return self.forecast()
        if self._graph is None:
            self._capture()
        self._reading.copy_(reading, non_blocking=True)
        self._graph.replay()
        self._pushed = min(self._pushed + 1, self.capacity)
        if self.interval_levels:
            self._interval_issued = True
        return self._prediction

    def _capture(self) -> None:
        """Warm the whole step up on a side stream and on a SCRATCH ring and clock (the live ones must not move), then
        capture it on the live ones into the static buffers."""
        ring, clock, out = self.ring.clone(), self.clock.clone(), self._window_buffers()
        scratch = calibration = None          # the scoring and interval states' scratch copies, made once they are sized
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                if scratch is not None:
                    self._settle(self._reading, scratch, clock)
                    if calibration is not None:
                        self._calibrate(self._reading, scratch, calibration, clock)
                self._push(self._reading, ring, clock)
                pred = self._forward(self._windows(ring, clock, out=out))
                if self.score:
                    self._score_setup(pred.shape[-1])
                    scratch = scratch or tuple(t.clone() for t in self._score_state)
                    self._store(pred, scratch, clock)
                    if self.interval_levels:
                        calibration = calibration or tuple(t.clone() for t in self._interval_state)
                        self._apply(pred, calibration, self._interval_buffers(), clock)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            if self.score:
                self._settle(self._reading, self._score_state, self.clock)
                if self.interval_levels:
                    self._calibrate(self._reading, self._score_state, self._interval_state, self.clock)
            self._push(self._reading, self.ring, self.clock)
            self._prediction = self._forward(self._windows(self.ring, self.clock, out=self._out))
            if self.score:
                self._store(self._prediction, self._score_state, self.clock)
                if self.interval_levels:
                    self._apply(self._prediction, self._interval_state, self._interval_out, self.clock)
        self._graph = graph

    # ---- the scores, read back -------------------------------------------------------------------------------------------
    def scores(self, at=None) -> dict:
        """The totals since the last `reset_scores()`, read back once (see the class docstring)."""
        if not self.score:
            raise RuntimeError("scores() needs OnlineForecaster(score=True)")
        n_levels = len(self.score_levels)
        if self._score_state is None:         # no forecast yet: nothing was due
            found = {"count": 0.0, "MAE": 0.0, "MAPE": 0.0, "RMSE": 0.0, "bias": 0.0,
                     "horizons": {k: [] for k in ("count", "MAE", "MAPE", "RMSE", "bias")}}
            if n_levels:
                found["quantiles"] = {"levels": list(self.score_levels), "coverage": [0.0] * n_levels,
                                      "pinball": [0.0] * n_levels, "crossing": 0.0, "width": 0.0}
            return found
        rows = self._score_state[2].cpu()
        n = rows[:, 0].clamp(min=1.0)
        named = {"count": rows[:, 0], "MAE": rows[:, 1] / n, "MAPE": rows[:, 2] / n, "RMSE": (rows[:, 3] / n).sqrt(),
                 "bias": rows[:, 4] / n}
        found = {k: float(v[-1]) for k, v in named.items()}
        horizons = {k: v[:-1].tolist() for k, v in named.items()}
        if n_levels:
            from .engine import Metrics
            horizons.update(Metrics._quantile_columns(rows[:-1], n[:-1], n_levels))
            last = Metrics._quantile_columns(rows[-1:], n[-1:], n_levels)
            found["quantiles"] = {"levels": list(self.score_levels), "coverage": [c[0] for c in last["coverage"]],
                                  "pinball": [c[0] for c in last["pinball"]], "crossing": last["crossing"][0],
                                  "width": last["width"][0]}
        if at is not None:
            for step in at:
                if not 1 <= int(step) <= self.score_t_out:
                    raise IndexError(f"horizon step {step} outside 1..{self.score_t_out}")
            pick = lambda v: [v[int(step) - 1] for step in at]  # noqa: E731
            horizons = {k: [pick(level) for level in v] if k in ("coverage", "pinball") else pick(v)
                        for k, v in horizons.items()}
        found["horizons"] = horizons
        return found

    def node_scores(self) -> torch.Tensor:
        """float64 [N, 3] on the host: valid count, MAE and bias per node over all horizons; NaN where the count is 0."""
        if not self.score:
            raise RuntimeError("node_scores() needs OnlineForecaster(score=True)")
        if self._score_state is None:
            found = torch.full((self.n_nodes, 3), float("nan"), dtype=torch.float64)
            found[:, 0] = 0.0
            return found
        rows = self._score_state[3].cpu()
        count = rows[:, 0]
        nan = torch.full((), float("nan"), dtype=torch.float64)
        safe = count.clamp(min=1.0)
        return torch.stack([count, torch.where(count > 0, rows[:, 1] / safe, nan),
                            torch.where(count > 0, rows[:, 2] / safe, nan)], dim=1)

    def reset_scores(self) -> None:
        """Zeroes the totals IN PLACE (a captured step holds their addresses); the book stays."""
        if not self.score:
            raise RuntimeError("reset_scores() needs OnlineForecaster(score=True)")
        if self._score_state is not None:
            self._score_state[2].zero_()
            self._score_state[3].zero_()
        if self._interval_state is not None:
            self._interval_state[4].zero_()

    # ---- the intervals, and how they have done ----------------------------------------------------------------------------
    def _need_intervals(self, what: str) -> None:
        if not self.interval_levels:
            raise RuntimeError(f"{what} needs OnlineForecaster(score=True, intervals=...)")

    def intervals(self):
        """`(lo, hi)`, each [L, N, T_out], of the forecast most recently returned (see the class docstring)."""
        self._need_intervals("intervals()")
        if not self._interval_issued:
            raise RuntimeError("intervals() belongs to a forecast: none was made yet")
        return self._interval_out

    def interval_scores(self, at=None) -> dict:
        """Coverage and width per level since the last `reset_scores()`, read back once (see the class docstring)."""
        self._need_intervals("interval_scores()")
        levels, nan = list(self.interval_levels), float("nan")
        if self._interval_state is None:      # no forecast yet: nothing was issued
            return {"levels": levels, "judged": [0] * len(levels), "coverage": [nan] * len(levels),
                    "width": [nan] * len(levels), "horizons": {"judged": [[] for _ in levels],
                                                               "coverage": [[] for _ in levels],
                                                               "width": [[] for _ in levels]}}
        _, _, radius, _, counts = self._interval_state
        packed = torch.cat([counts.reshape(-1), radius.view(torch.int32).reshape(-1).to(torch.int64)]).cpu()
        counts = packed[:counts.numel()].reshape(counts.shape)                                  # [L, N, T, 2]
        radius = packed[counts.numel():].to(torch.int32).view(torch.float32).reshape(radius.shape)
        per_h = counts.sum(1)                                                                   # [L, T, 2], in integers
        finite = torch.isfinite(radius)
        wide = torch.where(finite, 2.0 * radius.double(), torch.zeros((), dtype=torch.float64))
        ratio = lambda a, b: (a / b if b else nan)  # noqa: E731
        picks = range(self.score_t_out)
        if at is not None:
            for step in at:
                if not 1 <= int(step) <= self.score_t_out:
                    raise IndexError(f"horizon step {step} outside 1..{self.score_t_out}")
            picks = [int(step) - 1 for step in at]
        horizons = {"judged": [[int(per_h[l, h, 0]) for h in picks] for l in range(len(levels))],
                    "coverage": [[ratio(int(per_h[l, h, 1]), int(per_h[l, h, 0])) for h in picks]
                                 for l in range(len(levels))],
                    "width": [[ratio(float(wide[l, :, h].sum()), int(finite[l, :, h].sum())) for h in picks]
                              for l in range(len(levels))]}
        total = per_h.sum(1)
        return {"levels": levels, "judged": [int(t[0]) for t in total],
                "coverage": [ratio(int(t[1]), int(t[0])) for t in total],
                "width": [ratio(float(wide[l].sum()), int(finite[l].sum())) for l in range(len(levels))],
                "horizons": horizons}

    def interval_node_scores(self) -> torch.Tensor:
        """float64 [N, L] on the host: the coverage per sensor over all horizons; NaN where nothing was judged."""
        self._need_intervals("interval_node_scores()")
        if self._interval_state is None:
            return torch.full((self.n_nodes, len(self.interval_levels)), float("nan"), dtype=torch.float64)
        per_node = self._interval_state[4].cpu().sum(2)                                         # [L, N, 2], in integers
        judged, covered = per_node[..., 0], per_node[..., 1]
        nan = torch.full((), float("nan"), dtype=torch.float64)
        return torch.where(judged > 0, covered.double() / judged.clamp(min=1).double(), nan).t().contiguous()

    def state_dict(self) -> dict:
        state = {"ring": self.ring.detach().clone(), "clock": self.clock.detach().clone(), "start_step": self.start_step}
        if self._score_state is not None:
            state.update({k: t.detach().clone() for k, t in zip(self._SCORE_KEYS, self._score_state)})
        if self._interval_state is not None:
            from .intervals import STATE_KEYS
            state.update({k: t.detach().clone() for k, t in zip(STATE_KEYS, self._interval_state)})
        return state

    _SCORE_KEYS = ("book", "issued", "score_sums", "score_node_sums")

    def load_state_dict(self, state: dict) -> None:
        ring, clock = state["ring"], state["clock"]
        if tuple(ring.shape) != tuple(self.ring.shape) or ring.dtype != torch.float32 or tuple(clock.shape) != (2,) \
                or clock.dtype != torch.int64:
            raise ValueError(f"state holds a ring {tuple(ring.shape)} {ring.dtype} and a clock {tuple(clock.shape)} "
                             f"{clock.dtype}; this forecaster's are {tuple(self.ring.shape)} float32 and [2] int64")
        now, held = (int(v) for v in clock.cpu())
        if now < int(state["start_step"]) or not 0 <= held <= self.capacity:
            raise ValueError(f"state's clock [{now}, {held}] does not fit its start_step {state['start_step']} and a ring "
                             f"of {self.capacity} rows")
        scored = self.score and all(k in state for k in self._SCORE_KEYS)
        if scored:
            self._score_setup(int(state["book"].shape[-1]) if state["book"].dim() == 3 else 0)
            for key, mine in zip(self._SCORE_KEYS, self._score_state):
                if tuple(state[key].shape) != tuple(mine.shape) or state[key].dtype != mine.dtype:
                    raise ValueError(f"state holds {key} {tuple(state[key].shape)} {state[key].dtype}; this forecaster's "
                                     f"is {tuple(mine.shape)} {mine.dtype}")
        calibrated = False
        if scored and self.interval_levels:
            from .intervals import STATE_KEYS
            calibrated = all(k in state for k in STATE_KEYS)
            for key, mine in zip(STATE_KEYS, self._interval_state) if calibrated else ():
                if tuple(state[key].shape) != tuple(mine.shape) or state[key].dtype != mine.dtype:
                    raise ValueError(f"state holds {key} {tuple(state[key].shape)} {state[key].dtype}; this forecaster's "
                                     f"is {tuple(mine.shape)} {mine.dtype}")
        self.ring.copy_(ring)                 # in place: a captured step keeps reading these addresses
        self.clock.copy_(clock)
        self.start_step, self._pushed = int(state["start_step"]), held
        if scored:
            for key, mine in zip(self._SCORE_KEYS, self._score_state):
                mine.copy_(state[key])
        elif self._score_state is not None:   # a state without a book: cold, with zero totals
            from . import ops
            book, issued, sums, node_sums = self._score_state
            issued.fill_(ops.SCORE_NEVER)
            sums.zero_()
            node_sums.zero_()
        if calibrated:
            for key, mine in zip(STATE_KEYS, self._interval_state):
                mine.copy_(state[key])
        elif self._interval_state is not None:   # a state without them: empty windows, no intervals, zero counts
            window, cursor, radius, radius_book, counts = self._interval_state
            window.zero_()
            cursor.zero_()
            radius.fill_(float("inf"))
            radius_book.fill_(float("inf"))
            counts.zero_()
        if self.interval_levels:
            self._interval_issued = False        # lo and hi belong to a forecast of this state: the next one
