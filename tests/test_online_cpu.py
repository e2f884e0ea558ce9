"""CPU: the statistics that survive training (`data.series_stats`), the torch restatements of the ring kernels, and
`OnlineForecaster` on a torch stand-in model.  Everything selects, copies, subtracts once and divides once, so every
comparison is exact (int32 views: NaNs count)."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

from conftest import ROOT
from online_fixtures import (CONSTANT, DEAD, HOURS, NULL, ONE_CHANNEL, Q, SINGLE, bits, history, origins,
                             prepare_missing_pinned, push_series, raw_series, zscore_pinned)

TAU = 4
L = history(TAU)


def _loader_arrays(raw, **kw):
    """(normalised series [C,N,total], table or None) as `make_loaders` put them into its loaders."""
    from ms_gat_amd import data
    loader = data.make_loaders(raw, HOURS, Q, TAU, 4, device="cpu", **kw)[0]
    return loader.dataset.inputs, loader.climatology


# ---- statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(input_null_value=NULL, impute="period"),
                                dict(input_null_value=NULL, impute="mean", mask_channel=False)],
                         ids=["plain", "period", "mean"])
def test_series_stats_reproduces_what_the_loaders_hold(kw):
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    if not kw:
        raw = raw.clamp_min(1.0) + torch.arange(raw.shape[-1]) * 0.01     # the plain z-score wants spread everywhere
    stats = data.series_stats(raw, HOURS, Q, TAU, **kw)
    normed, table = _loader_arrays(raw, **kw)
    C_, N, total = raw.shape
    assert stats.mean.shape == stats.std.shape == (C_, N) and stats.mean.dtype == stats.std.dtype == torch.float32
    assert stats.train_end == data.split_intervals(total, HOURS, Q, TAU)[1]
    assert stats.hours == HOURS and stats.tau == TAU and stats.history == L
    want = (raw.float() - stats.mean[..., None]) / stats.std[..., None]
    if kw:
        missing = data.missing_entries(raw, NULL)
        assert bool(missing[:, DEAD].all()) and bool(torch.isnan(normed[missing]).all())
        want = torch.where(missing, torch.full((), float("nan")), want)
        assert torch.equal(bits(stats.climatology), bits(table))
        assert stats.period == (7 * 24 * TAU if kw["impute"] == "period" else 1) == table.shape[0]
        assert stats.input_null_value == NULL and stats.mask_channel == kw.get("mask_channel", True)
        assert stats.input_channels == C_ + int(stats.mask_channel)
        if kw["impute"] == "mean":
            assert not bool(stats.climatology.any())
        # the three special sensors: std 1, and as mean the single valid value, or 0
        assert bool((stats.std[:, [DEAD, SINGLE, CONSTANT]] == 1).all())
        assert bool((stats.mean[:, DEAD] == 0).all()) and bool((stats.mean[:, SINGLE] == 41.5).all())
        assert bool((stats.mean[:, CONSTANT] == 37.0).all())
    else:
        assert stats.climatology is None and stats.period is None and stats.input_null_value is None
        assert stats.input_channels == C_ and not stats.mask_channel
    assert torch.equal(bits(want), bits(normed))
    assert torch.equal(bits(stats.normalise(raw)), bits(normed))


def test_zscore_and_prepare_missing_return_what_they_did():
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    split = data.split_intervals(raw.shape[-1], HOURS, Q, TAU)[1]
    plain = raw + 1.0 + torch.arange(raw.shape[-1]) * 0.01
    assert torch.equal(bits(data.zscore(plain, split)), bits(zscore_pinned(plain, split)))
    for null, period in ((NULL, 7), (NULL, 1), (float("nan"), 5), (NULL, 7 * 24 * TAU)):
        series = raw.clone()
        if null != null:
            series[series == 0] = float("nan")
        got, want = data.prepare_missing(series, split, null, period), prepare_missing_pinned(series, split, null, period)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1])), (null, period)
        assert got[1].shape == (period, 3, 9)


def test_series_stats_save_and_load_round_trip(tmp_path):
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    for kw in (dict(), dict(input_null_value=NULL, impute="period")):
        stats = data.series_stats(raw + (0 if kw else 1.0), HOURS, Q, TAU, **kw)
        path = tmp_path / f"stats{len(kw)}.pt"
        stats.save(path)
        stored = torch.load(path, map_location="cpu")
        assert isinstance(stored, dict) and set(stored) == {
            "mean", "std", "climatology", "hours", "tau", "period", "input_null_value", "mask_channel", "input_channels",
            "train_end"}
        back = data.SeriesStats.load(path)
        assert torch.equal(bits(back.mean), bits(stats.mean)) and torch.equal(bits(back.std), bits(stats.std))
        if kw:
            assert torch.equal(bits(back.climatology), bits(stats.climatology))
        else:
            assert back.climatology is None
        assert (back.hours, back.tau, back.period, back.input_null_value, back.mask_channel, back.input_channels,
                back.train_end) == (stats.hours, stats.tau, stats.period, stats.input_null_value, stats.mask_channel,
                                    stats.input_channels, stats.train_end)
    with pytest.raises(ValueError, match="impute"):
        data.series_stats(raw, HOURS, Q, TAU, input_null_value=NULL, impute="median")


# ---- the torch ring -----------------------------------------------------------------------------------------------------
def _new_ring(C_, N, start, rows=L):
    return torch.full((rows, C_, N), float("nan")), torch.tensor([start, 0], dtype=torch.int64)


def _pusher(stats, ring, clock):
    from ms_gat_amd import data
    return lambda r: data._ring_push_torch(r, stats.mean, stats.std, ring, clock, null_value=stats.input_null_value)


@pytest.mark.parametrize("kw", [dict(), dict(input_null_value=NULL, impute="period"),
                                dict(input_null_value=NULL, impute="period", mask_channel=False),
                                dict(input_null_value=NULL, impute="mean")], ids=["plain", "period", "nomask", "mean"])
def test_ring_windows_equal_the_windows_of_the_full_series(kw):
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    if not kw:
        raw = raw + 1.0 + torch.arange(raw.shape[-1]) * 0.01
    stats = data.series_stats(raw, HOURS, Q, TAU, **kw)
    normed, table = _loader_arrays(raw, **kw)
    series_tm = normed.permute(2, 0, 1).contiguous()
    ring, clock = _new_ring(3, 9, 0)
    push = _pusher(stats, ring, clock)
    push_series(push, raw, 0, origins(TAU)[0])
    for t in origins(TAU):
        assert clock.tolist() == [t, min(t, L)]
        got = data._ring_windows_torch(ring, clock, HOURS, TAU, climatology=stats.climatology,
                                       mask_channel=stats.mask_channel)
        want = data._windows_torch(series_tm, raw[0], torch.tensor([t]), HOURS, TAU, Q, climatology=table,
                                   mask_channel=stats.mask_channel)[:3]
        for name, a, b in zip("XHD", got, want):
            assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous(), (t, name)
            assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b), (t, name)
        if kw:
            assert not bool(torch.isnan(got[0]).any())
        push_series(push, raw, t, t + 1)
    # the reading with one channel missing: validity 0, the observed channels keep their readings
    if stats.mask_channel:
        t = history(TAU) + 1
        ring, clock = _new_ring(3, 9, 0)
        push_series(_pusher(stats, ring, clock), raw, 0, t)
        x = data._ring_windows_torch(ring, clock, HOURS, TAU, climatology=stats.climatology, mask_channel=True)[0][0, 0]
        assert x[3, ONE_CHANNEL].tolist() == [1.0, 0.0, 0.0, 0.0]                    # steps t-4 .. t-1; t-2 on are missing
        assert torch.equal(bits(x[:2, ONE_CHANNEL]), bits(normed[:2, ONE_CHANNEL, t - TAU: t]))


@pytest.mark.parametrize("chunk", [5, L])
def test_chunked_pushes_leave_the_ring_of_single_pushes(chunk):
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    stats = data.series_stats(raw, HOURS, Q, TAU, input_null_value=NULL)
    stop = 2 * L + 7
    single, one = _new_ring(3, 9, 3)
    push_series(_pusher(stats, single, one), raw, 3, stop)
    ring, clock = _new_ring(3, 9, 3)
    push_series(_pusher(stats, ring, clock), raw, 3, stop, chunk=chunk)
    assert torch.equal(bits(ring), bits(single)) and torch.equal(clock, one) and clock.tolist() == [stop, L]
    assert bool((bits(ring)[torch.isnan(ring)] == 0x7fc00000).all()) and bool(torch.isnan(ring).any())


@pytest.mark.parametrize("period", [7, 7 * 24 * TAU])
def test_hours_days_and_slots_from_a_64_bit_clock(period):
    """start_step = 2^33 + 5, every reading missing and table[s] = s: X holds the slot of each step, which Python's
    integers give; so do H and D.  7 does not divide L."""
    from ms_gat_amd import data
    start, C_, N = 2 ** 33 + 5, 1, 3
    table = torch.arange(period, dtype=torch.float32)[:, None, None].expand(period, C_, N).contiguous()
    ring, clock = _new_ring(C_, N, start)
    mean, std = torch.zeros(C_, N), torch.ones(C_, N)
    for i in range(L + 6):
        data._ring_push_torch(torch.zeros(1, C_, N), mean, std, ring, clock, null_value=0.0)
        t = start + i + 1
        x, h, d = data._ring_windows_torch(ring, clock, HOURS, TAU, climatology=table, mask_channel=True)
        assert clock.tolist() == [t, min(i + 1, L)]
        assert h.tolist() == [(t // TAU) % 24] and d.tolist() == [(t // TAU // 24) % 7] and h.dtype == d.dtype == torch.int64
        if i + 1 >= L:
            for r, hrs in enumerate(HOURS):
                want = [float((t - hrs * TAU + k) % period) for k in range(TAU)]
                assert x[0, r, 0, 1].tolist() == want, (t, r)
            assert not bool(x[0, :, 1].any())


# ---- the forecaster on a stand-in model ---------------------------------------------------------------------------------
class StandIn(nn.Module):
    """(X [B,R,C,N,T], H [B], D [B]) -> [B,N,q]: every input moves the output."""

    def __init__(self, in_channels, q=Q):
        super().__init__()
        self.in_channels = in_channels
        self.proj = nn.Linear(len(HOURS) * in_channels * TAU, q)
        self.h_ebd, self.d_ebd = nn.Embedding(24, q), nn.Embedding(7, q)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        return self.proj(X.permute(0, 3, 1, 2, 4).reshape(B, N, R * C_ * T)) + (self.h_ebd(H) + self.d_ebd(D))[:, None]


def _forecaster(raw, start=0, **kw):
    from ms_gat_amd import OnlineForecaster, data
    torch.manual_seed(3)
    stats = data.series_stats(raw, HOURS, Q, TAU, input_null_value=NULL)
    return OnlineForecaster(StandIn(stats.input_channels), stats, start, **kw), stats


def test_forecaster_steps_equal_the_model_on_the_loader_items():
    from ms_gat_amd import data
    raw = raw_series(3, 9)
    f, stats = _forecaster(raw)
    normed, table = _loader_arrays(raw, input_null_value=NULL)
    ds = data.PeriodicWindows(normed, raw[0], (L, raw.shape[-1] - Q + 1), HOURS, Q, TAU, climatology=table, mask_channel=True)
    assert not f.ready and f.capacity == L and f.resident_bytes == 4 * L * 3 * 9
    with pytest.raises(RuntimeError, match="readings"):
        f.forecast()
    with pytest.raises(RuntimeError):
        f.step(raw[:, :, 0])
    f.push(raw[:, :, 1:L - 1].permute(2, 0, 1))
    assert not f.ready
    for t in range(L, L + 30):
        y = f.step(raw[:, :, t - 1])
        assert f.ready and tuple(y.shape) == (9, Q)
        x, h, d, _ = ds[t - L]
        with torch.no_grad():
            want = f.model(x[None], h[None], d[None])[0]
        assert torch.equal(bits(y), bits(want)), t
    assert torch.equal(bits(f.forecast()), bits(want)) and not f.model.training
    assert f.clock.tolist() == [L + 29, L]


def test_forecaster_refuses_what_it_cannot_take():
    from ms_gat_amd import OnlineForecaster
    raw = raw_series(3, 9)
    f, stats = _forecaster(raw)
    for bad in (torch.zeros(3, 8), torch.zeros(2, 9), torch.zeros(1, 2, 3, 9), torch.zeros(9), torch.zeros(0, 3, 9)):
        with pytest.raises(ValueError, match="reading"):
            f.push(bad)
    with pytest.raises(ValueError, match="capacity"):
        f.push(torch.zeros(L + 1, 3, 9))
    with pytest.raises(ValueError, match="float32"):
        f.push(torch.zeros(3, 9, dtype=torch.float64))
    f.push(torch.ones(L, 3, 9))
    assert f.ready
    with pytest.raises(ValueError, match="in_channels"):
        OnlineForecaster(StandIn(3), stats, 0)
    for capacity in (L - TAU, L + 1):
        with pytest.raises(ValueError, match="capacity"):
            OnlineForecaster(StandIn(4), stats, 0, capacity=capacity)
    with pytest.raises(ValueError, match="start_step"):
        OnlineForecaster(StandIn(4), stats, -1)
    with pytest.raises(ValueError, match="hip_graph"):
        OnlineForecaster(StandIn(4), stats, 0, hip_graph=True)
    assert OnlineForecaster(StandIn(4), stats, 0, capacity=2 * L).ring.shape == (2 * L, 3, 9)


def test_forecaster_state_round_trip():
    raw = raw_series(3, 9)
    f, _ = _forecaster(raw, start=2)
    f.push(raw[:, :, 2:L + 5].permute(2, 0, 1)[:L])
    for t in range(L + 2, L + 5):
        f.step(raw[:, :, t])
    state = f.state_dict()
    assert set(state) == {"ring", "clock", "start_step"} and state["start_step"] == 2
    g, _ = _forecaster(raw, start=0)
    g.model.load_state_dict(f.model.state_dict())
    assert not g.ready
    g.load_state_dict(state)
    assert g.ready and g.start_step == 2 and g.clock.tolist() == f.clock.tolist() == [L + 5, L]
    state["ring"].fill_(0)                                      # the state is a copy, and so is what was loaded
    for t in range(L + 5, L + 9):
        assert torch.equal(bits(g.step(raw[:, :, t])), bits(f.step(raw[:, :, t]))), t
    with pytest.raises(ValueError, match="ring"):
        g.load_state_dict({"ring": torch.zeros(L + TAU, 3, 9), "clock": state["clock"], "start_step": 0})


# ---- ABI and build ------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_prototyped_and_exported():
    import ms_gat_amd
    from ms_gat_amd import _lib, build
    path = build.build(verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgat_hip.h")).read(), flags=re.S)
    lib = C.CDLL(path)
    for name, n_args in (("msgat_ring_push", 12), ("msgat_ring_windows", 15)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/msgat_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_lib._PROTOTYPES[name][1]) == n_args and _lib._PROTOTYPES[name][0] is C.c_int
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 10 and lib.msgat_abi_version() == 10
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", text)
    assert "online.hip" in build.SOURCES and "windows.hip" in build.SOURCES
    assert "OnlineForecaster" in ms_gat_amd.__all__ and ms_gat_amd.OnlineForecaster is ms_gat_amd.online.OnlineForecaster


def test_entry_points_refuse_bad_arguments_on_the_host():
    """NULL, shape and size checks come before any launch: no device needed."""
    from ms_gat_amd import _lib
    lib = _lib.lib()
    p = 0x1000                                                   # never dereferenced: every call below fails its checks
    NULL_, SHAPE, UNSUPPORTED = -1, -2, -3
    push = lambda *a: lib.msgat_ring_push(*a, None)  # noqa: E731
    assert push(None, p, p, p, p, 1, 1, 1, 4, 0, 0.0) == NULL_ and push(p, p, p, p, None, 1, 1, 1, 4, 0, 0.0) == NULL_
    for K, C_, N, rows in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0), (5, 1, 1, 4)):
        assert push(p, p, p, p, p, K, C_, N, rows, 0, 0.0) == SHAPE, (K, C_, N, rows)
    assert push(p, p, p, p, p, 1, 2, 2 ** 30, 4, 0, 0.0) == UNSUPPORTED
    win = lambda *a: lib.msgat_ring_windows(*a, None)  # noqa: E731
    assert win(None, p, p, p, p, p, p, 1, 1, 1, 4, 4, 1, 0) == NULL_ and win(p, p, p, p, p, p, None, 1, 1, 1, 4, 4, 1, 0) == NULL_
    for R, C_, N, rows, tau, period, mask, table in ((0, 1, 1, 4, 4, 1, 0, p), (1, 1, 1, 6, 4, 1, 0, p), (1, 1, 1, 0, 4, 1, 0, p),
                                                     (1, 1, 1, 4, 4, 0, 0, p), (1, 1, 1, 4, 4, 1, 1, None)):
        assert win(p, table, p, p, p, p, p, R, C_, N, rows, tau, period, mask) == SHAPE, (R, C_, N, rows, tau, period, mask)
    assert win(p, p, p, p, p, p, p, 1, 1, 1, 10, 5, 1, 0) == UNSUPPORTED            # tau = 5
    assert win(p, p, p, p, p, p, p, 1, 1, 2 ** 30, 4, 4, 1, 0) == UNSUPPORTED
