"""GPU: `msgat_ring_push` / `msgat_ring_windows` and `OnlineForecaster` on the device.

The kernels select, copy, subtract once and divide once, so every comparison is exact (int32 views).  They are launched
through the C ABI into buffers pre-filled with a NaN pattern no input holds, with a guard band behind each: a word left
out, or one written past the end, shows.  Expected values: the CPU normalisation of `data.series_stats` for the push,
`ops.window_gather{,_imputed}` over the full uploaded series for the windows, `model(*batch)` on the `DeviceWindows`
batch of the same origin for the forecaster."""
import pytest
import torch

from online_fixtures import HOURS, NULL, ONE_CHANNEL, Q, bits, history, origins, push_series, raw_series

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 0x7fa5a5a5          # a NaN no input holds
CANONICAL = 0x7fc00000
GUARD = 64                     # words behind every buffer the kernels write


def _guarded(shape, dtype=torch.float32):
    """(flat buffer with the guard band, the view of `shape` in front of it), sentinel-filled."""
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.float32:
        flat = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        flat = torch.full((n + GUARD,), -77, dtype=torch.int64, device=DEV)
    return flat, flat[:n].view(shape)


def _guards_intact(*pairs):
    for flat, out in pairs:
        tail = flat[out.numel():]
        ok = (tail.view(torch.int32) == SENTINEL).all() if flat.dtype == torch.float32 else (tail == -77).all()
        assert bool(ok), "a word past the end of a buffer was written"


def _stats(raw, tau, **kw):
    from ms_gat_amd import data
    return data.series_stats(raw, HOURS, Q, tau, **kw)


def _stream():
    from ms_gat_amd import _lib
    return _lib.stream_handle(torch.device(DEV))


# ---- push --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_null", [True, False])
@pytest.mark.parametrize("K", [1, 5, 12])
@pytest.mark.parametrize("C_,N", [(1, 40), (3, 100), (3, 300)])
def test_push_writes_exactly_its_rows_with_the_bits_of_the_cpu_normalisation(C_, N, K, has_null):
    from ms_gat_amd import _lib
    tau, L = 4, 12
    raw = raw_series(C_, N)
    stats = _stats(raw, tau, input_null_value=NULL)
    first = 20                                                   # K steps of the series from here
    readings = raw[:, :, first: first + K].permute(2, 0, 1).contiguous().clone()        # [K,C,N]
    readings[0, 0, 7] = NAN
    assert bool((readings == 0).any()) and C_ * N in (40, 300, 900)
    t = 5 * L + (L - 1 if K == 1 else L - K // 2 - 1)           # the K rows end at or run across the ring's last row
    held = 9
    ring_flat, ring = _guarded((L, C_, N))
    clock_flat, clock = _guarded((2,), torch.int64)
    clock.copy_(torch.tensor([t, held]))
    dev = [x.to(DEV) for x in (readings, stats.mean, stats.std)]
    st = _lib.lib().msgat_ring_push(*[x.data_ptr() for x in dev], ring.data_ptr(), clock.data_ptr(), K, C_, N, L,
                                    int(has_null), NULL, _stream())
    _lib.check(st, "msgat_ring_push")
    torch.cuda.synchronize()
    _guards_intact((ring_flat, ring), (clock_flat, clock))
    assert clock.tolist() == [t + K, min(held + K, L)]
    want = (readings - stats.mean) / stats.std                  # the CPU expression: one subtract, one divide
    if has_null:
        want = torch.where(torch.isnan(readings) | (readings == NULL), torch.full((), NAN), want)
    rows = [(t + k) % L for k in range(K)]
    assert K == 1 or rows != sorted(rows), "the pushed rows must run across the end of the ring"
    got = bits(ring.cpu())
    for k, row in enumerate(rows):
        if has_null:
            assert torch.equal(got[row], bits(want[k])), (k, row)
            assert (k > 0 or int(got[row, 0, 7]) == CANONICAL) and bool((got[row][readings[k] == 0] == CANONICAL).all())
        else:
            keep = ~torch.isnan(want[k])                         # a NaN reading stays a NaN; its payload is not pinned
            assert torch.equal(got[row][keep], bits(want[k])[keep]), (k, row)
            assert bool(torch.isnan(ring[row].cpu()[~keep]).all()) and int((~keep).sum()) == (k == 0)
            assert bool((readings[k] == 0).any())               # a 0 reading is normalised like any other: none is a NaN
    others = [r for r in range(L) if r not in rows]
    assert bool((got[others] == SENTINEL).all()) and len(others) == L - K


# ---- windows -----------------------------------------------------------------------------------------------------------
def _launch_windows(ring, table, clock, offsets, R, tau, mask):
    from ms_gat_amd import _lib
    L, C_, N = ring.shape
    xf, X = _guarded((1, R, C_ + int(mask), N, tau))
    hf, H = _guarded((1,), torch.int64)
    df, D = _guarded((1,), torch.int64)
    st = _lib.lib().msgat_ring_windows(ring.data_ptr(), None if table is None else table.data_ptr(), clock.data_ptr(),
                                       offsets.data_ptr(), X.data_ptr(), H.data_ptr(), D.data_ptr(), R, C_, N, L, tau,
                                       1 if table is None else table.shape[0], int(mask), _stream())
    _lib.check(st, "msgat_ring_windows")
    torch.cuda.synchronize()
    _guards_intact((xf, X), (hf, H), (df, D))
    return X, H, D


def _series_and_table(C_, N, tau, table):
    """(raw, stats, full series on the device TIME-MAJOR, target on the device, table on the device or None)."""
    from ms_gat_amd import data
    raw = raw_series(C_, N, tau)
    if table is None:
        raw = raw + 1.0 + torch.arange(raw.shape[-1]) * 0.01    # no missing readings, spread in every row
        stats = _stats(raw, tau)
    else:
        stats = _stats(raw, tau, input_null_value=NULL)
        if table != "week":                                      # a period that does not divide L
            g = torch.Generator().manual_seed(C_ + N + tau)
            stats.climatology, stats.period = torch.randn(table, C_, N, generator=g), table
    series_dev, target_dev = data.upload_series(stats.normalise(raw), raw[0].contiguous(), DEV)
    return raw, stats, series_dev, target_dev, None if table is None else stats.climatology.to(DEV)


def _ring_follows_the_full_series(C_, N, tau, table, mask, start=0):
    from ms_gat_amd import ops
    raw, stats, series_dev, target_dev, table_dev = _series_and_table(C_, N, tau, table)
    L = history(tau)
    flat, ring = _guarded((L, C_, N))
    ring.fill_(NAN)                                              # a new ring: the canonical NaN
    clock = torch.tensor([start, 0], dtype=torch.int64, device=DEV)
    mean, std = stats.mean.to(DEV), stats.std.to(DEV)
    offsets = ops.window_offsets(HOURS, tau, torch.device(DEV))
    raw_dev = raw.to(DEV)
    push = lambda r: ops.ring_push(r, mean, std, ring, clock, null_value=stats.input_null_value)  # noqa: E731
    push_series(push, raw_dev, 0, origins(tau)[0])
    saw_missing = False
    for t in origins(tau):
        got = _launch_windows(ring, table_dev, clock, offsets, len(HOURS), tau, mask)
        o = torch.tensor([t], dtype=torch.int64, device=DEV)
        if table is None:
            want = ops.window_gather(series_dev, target_dev, o, HOURS, tau, Q, offsets=offsets)
        else:
            want = ops.window_gather_imputed(series_dev, table_dev, target_dev, o, HOURS, tau, Q, mask_channel=mask,
                                             offsets=offsets)
        assert got[0].shape == want[0].shape and torch.equal(bits(got[0]), bits(want[0])), ("X", t)
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), ("H, D", t)
        saw_missing = saw_missing or (mask and bool((got[0][0, :, C_, ONE_CHANNEL] == 0).any()))
        push_series(push, raw_dev, t, t + 1)
    torch.cuda.synchronize()
    _guards_intact((flat, ring))
    assert clock.tolist() == [start + origins(tau)[-1] + 1, L]
    assert saw_missing == bool(mask)


@pytest.mark.parametrize("table,mask", [(None, False), ("week", True), ("week", False), (7, True), (7, False)])
@pytest.mark.parametrize("C_,N", [(1, 40), (1, 300), (3, 40), (3, 300)])
@pytest.mark.parametrize("tau", [4, 12])
def test_windows_of_the_ring_equal_the_gather_over_the_full_series(tau, C_, N, table, mask):
    _ring_follows_the_full_series(C_, N, tau, table, mask)


def test_windows_with_a_64_bit_start_step():
    """The clock starts past 2^33, at a multiple of 24 * 7 * tau * period: hours, weekdays and slots then agree with those
    of the unshifted origins of the full series."""
    tau, period = 4, 7
    unit = 24 * 7 * tau * period
    start = (2 ** 33 // unit + 1) * unit
    assert start > 2 ** 33 and start % unit == 0
    _ring_follows_the_full_series(3, 40, tau, period, True, start=start)


@pytest.mark.parametrize("table", [None, 7])
def test_a_cold_ring_stays_in_bounds(table):
    """clock 0, nothing pushed: every window starts before step 0.  Rows come from the floor-mod, so the launch stays
    inside the ring (guard bands intact); with a table every reading counts as missing."""
    from ms_gat_amd import ops
    tau, C_, N, L = 4, 3, 300, 12
    flat, ring = _guarded((L, C_, N))
    ring.fill_(NAN)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    offsets = ops.window_offsets(HOURS, tau, torch.device(DEV))
    table_dev = None if table is None else torch.randn(table, C_, N, generator=torch.Generator().manual_seed(1)).to(DEV)
    X, H, D = _launch_windows(ring, table_dev, clock, offsets, len(HOURS), tau, table is not None)
    _guards_intact((flat, ring))
    assert H.tolist() == [0] and D.tolist() == [0] and clock.tolist() == [0, 0]
    if table is None:
        assert bool((bits(X) == CANONICAL).all())
    else:
        assert not bool(X[0, :, C_].any()) and not bool(torch.isnan(X).any())
        for r, h in enumerate(HOURS):
            slots = [(-h * tau + k) % table for k in range(tau)]
            assert torch.equal(bits(X[0, r, :C_]), bits(table_dev[slots].permute(1, 2, 0)))


def test_ops_check_their_arguments():
    from ms_gat_amd import ops
    ring = torch.full((12, 3, 40), NAN, device=DEV)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    stat, raw = torch.ones(3, 40, device=DEV), torch.ones(2, 3, 40, device=DEV)
    with pytest.raises(ValueError, match="raw"):
        ops.ring_push(raw[:, :2].contiguous(), stat, stat, ring, clock)
    with pytest.raises(ValueError, match="K = 13"):
        ops.ring_push(torch.ones(13, 3, 40, device=DEV), stat, stat, ring, clock)
    with pytest.raises(TypeError, match="clock"):
        ops.ring_push(raw, stat, stat, ring, clock.int())
    with pytest.raises(TypeError, match="mean"):
        ops.ring_push(raw, stat.double(), stat, ring, clock)
    with pytest.raises(ValueError, match="std"):
        ops.ring_push(raw, stat, stat.cpu(), ring, clock)
    with pytest.raises(ValueError, match="contiguous"):
        ops.ring_push(raw, stat, stat, ring.permute(0, 2, 1).contiguous().permute(0, 2, 1), clock)
    with pytest.raises(ValueError, match="tau"):
        ops.ring_windows(ring, clock, HOURS, 5)
    with pytest.raises(ValueError, match="hours"):
        ops.ring_windows(ring, clock, [0, 1], 4)
    with pytest.raises(ValueError, match="L = 12"):
        ops.ring_windows(ring, clock, [1, 2, 4], 4)
    with pytest.raises(ValueError, match="climatology"):
        ops.ring_windows(ring, clock, HOURS, 4, climatology=torch.zeros(7, 3, 41, device=DEV))
    with pytest.raises(ValueError, match="mask_channel"):
        ops.ring_windows(ring, clock, HOURS, 4, mask_channel=True)
    with pytest.raises(ValueError, match="out's X"):
        ops.ring_windows(ring, clock, HOURS, 4, out=(torch.zeros(1, 3, 4, 40, 4, device=DEV), clock[:1], clock[1:]))
    assert clock.tolist() == [0, 0] and bool(torch.isnan(ring).all())
    X, H, D = ops.ring_windows(ring, clock, HOURS, 4)
    assert tuple(X.shape) == (1, 3, 3, 40, 4) and tuple(H.shape) == tuple(D.shape) == (1,)


# ---- the forecaster ------------------------------------------------------------------------------------------------------
def _model(out_timesteps, seed=0):
    import ms_gat_amd
    torch.manual_seed(seed)
    adj = ms_gat_amd.synthetic_adjacency(40, 60, seed=1)
    return ms_gat_amd.msgat48(n_components=3, in_channels=4, in_timesteps=4, out_timesteps=out_timesteps, use_te=True,
                              adj=adj, missing_edges="scale").to(DEV)


def _device_batches(raw, stats, first, count):
    """The `DeviceWindows` batches of the origins first .. first + count - 1, one origin each."""
    from ms_gat_amd import data
    return list(data.DeviceWindows(stats.normalise(raw), raw[0].contiguous(), (first, first + count), HOURS, Q, 4, 1,
                                   device=DEV, climatology=stats.climatology, mask_channel=True))


def test_graphed_eager_and_loader_forecasts_have_the_same_bits():
    from ms_gat_amd import OnlineForecaster
    tau, L, steps = 4, 12, 30
    raw = raw_series(3, 40)
    stats = _stats(raw, tau, input_null_value=NULL)
    model = _model(Q)
    graphed, eager = OnlineForecaster(model, stats, 0), OnlineForecaster(model, stats, 0, hip_graph=False)
    assert graphed.hip_graph and not eager.hip_graph and not model.training
    for f in (graphed, eager):
        f.push(raw[:, :, :L - 1].permute(2, 0, 1))               # a host tensor, K = L - 1
        assert not f.ready
    batches = _device_batches(raw, stats, L, steps)
    resumed = None
    for i, batch in enumerate(batches):
        t = L + i
        reading = raw[:, :, t - 1] if i % 2 else raw[:, :, t - 1].to(DEV)       # host and device readings
        y = graphed.step(reading)
        with torch.no_grad():
            want = model(*batch[:3])[0]
        assert tuple(y.shape) == (40, Q) and torch.equal(bits(y), bits(want)), ("graphed", t)
        assert torch.equal(bits(eager.step(reading)), bits(want)), ("eager", t)
        if resumed is not None:
            assert torch.equal(bits(resumed.step(reading)), bits(want)), ("resumed", t)
        if i == 19:                                              # a restarted service: a fresh forecaster takes the state
            resumed = OnlineForecaster(model, stats, 0)
            resumed.load_state_dict(graphed.state_dict())
            assert resumed.ready
    assert graphed._graph is not None and eager._graph is None and resumed._graph is not None
    assert torch.equal(bits(graphed.forecast()), bits(want))     # a bare forecast: the same kernels, eagerly
    for f, pushes in ((graphed, L - 1 + steps), (eager, L - 1 + steps), (resumed, L - 1 + steps)):
        assert f.clock.tolist() == [pushes, L]
    on_host = OnlineForecaster(torch.nn.Linear(1, 1), stats, 0)  # a CPU model does not take a device reading
    with pytest.raises(ValueError, match="model on"):
        on_host.push(raw[:, :, 0].to(DEV))


def test_a_quantile_head_passes_through():
    from ms_gat_amd import OnlineForecaster
    tau, L = 4, 12
    raw = raw_series(3, 40)
    stats = _stats(raw, tau, input_null_value=NULL)
    model = _model(3 * 4, seed=1)                                # three quantiles of four steps, as QuantileLoss reads them
    f = OnlineForecaster(model, stats, 0)
    f.push(raw[:, :, :L - 1].permute(2, 0, 1).to(DEV))
    for t, batch in zip(range(L, L + 3), _device_batches(raw, stats, L, 3)):
        y = f.step(raw[:, :, t - 1])
        with torch.no_grad():
            want = model(*batch[:3])[0]
        assert tuple(y.shape) == (40, 12) and torch.equal(bits(y), bits(want)), t
