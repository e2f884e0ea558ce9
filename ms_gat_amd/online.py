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
    One process, one origin per step: multi-rank serving and batched origins are not provided."""

    def __init__(self, model: nn.Module, stats: "_data.SeriesStats", start_step: int, capacity: int | None = None,
                 hip_graph="auto"):
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
        reading = self._checked(reading)
        self._push(reading.to(self.device).contiguous(), self.ring, self.clock)
        self._pushed = min(self._pushed + reading.shape[0], self.capacity)

    def forecast(self) -> torch.Tensor:
        if not self.ready:
            raise RuntimeError(f"forecast() needs {self.history} readings in the ring, {self._pushed} were pushed")
        out = self._out if self.device.type == "cuda" else None
        return self._forward(self._windows(self.ring, self.clock, out=out))

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
        return self._prediction

    def _capture(self) -> None:
        """Warm the whole step up on a side stream and on a SCRATCH ring and clock (the live ones must not move), then
        capture it on the live ones into the static buffers."""
        ring, clock, out = self.ring.clone(), self.clock.clone(), self._window_buffers()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._push(self._reading, ring, clock)
                self._forward(self._windows(ring, clock, out=out))
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self._push(self._reading, self.ring, self.clock)
            self._prediction = self._forward(self._windows(self.ring, self.clock, out=self._out))
        self._graph = graph

    def state_dict(self) -> dict:
        return {"ring": self.ring.detach().clone(), "clock": self.clock.detach().clone(), "start_step": self.start_step}

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
        self.ring.copy_(ring)                 # in place: a captured step keeps reading these addresses
        self.clock.copy_(clock)
        self.start_step, self._pushed = int(state["start_step"]), held
