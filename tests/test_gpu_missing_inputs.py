"""GPU: `msgat_window_gather_imputed` / `ops.window_gather_imputed` -- the input windows with missing readings filled in
from the slot table and a validity channel -- and the loaders and models fed by it.

The kernel selects and copies, so every comparison is exact (int32 views: NaN payloads and -0.0 count).  Expected values
come from `data._windows_torch` with a table, run on the device; test_missing_inputs_cpu.py ties it to a per-entry loop.
The kernel is launched through the C ABI into buffers pre-filled with a NaN pattern, with a guard band behind each: a
word it leaves out, or one it writes past the end, shows.
"""
import copy
import functools

import pytest
import torch

from device_windows_fixtures import assert_batches_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 0x7fa5a5a5          # a NaN no input holds
GUARD = 64                     # words behind every output


def _on_cpu(batch):
    return [t.cpu() for t in batch]


def launch(series, table, target, origins, hours, tau, q, mask):
    """The C entry point into sentinel-filled outputs; returns (X, H, D, Y) after checking the guard bands."""
    from ms_gat_amd import _lib, ops
    T_total, C_, N = series.shape
    B, R = origins.numel(), len(hours)
    shapes = [(B, R, C_ + int(mask), N, tau), (B,), (B,), (B, N, q)]
    dtypes = [torch.float32, torch.int64, torch.int64, torch.float32]
    flats, outs = [], []
    for shape, dtype in zip(shapes, dtypes):
        n = 1
        for s in shape:
            n *= s
        if dtype == torch.float32:
            flat = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        else:
            flat = torch.full((n + GUARD,), -77, dtype=torch.int64, device=DEV)
        flats.append(flat)
        outs.append(flat[:n].view(shape))
    offsets = ops.window_offsets(hours, tau, torch.device(DEV))
    st = _lib.lib().msgat_window_gather_imputed(
        series.data_ptr(), table.data_ptr(), target.data_ptr(), origins.data_ptr(), offsets.data_ptr(),
        *[o.data_ptr() for o in outs], B, R, C_, N, T_total, tau, q, tau * max(hours), table.shape[0], int(mask),
        _lib.stream_handle(torch.device(DEV)))
    _lib.check(st, "msgat_window_gather_imputed")
    torch.cuda.synchronize()
    for flat, out in zip(flats, outs):
        tail = flat[out.numel():]
        if flat.dtype == torch.float32:
            assert bool((tail.view(torch.int32) == SENTINEL).all()), "a word past the end of an output was written"
        else:
            assert bool((tail == -77).all()), "a word past the end of an output was written"
    return outs


HOURS = {1: [24], 3: [1, 2, 24]}


@functools.lru_cache(maxsize=4)
def series_case(C_, N, tau, period):
    """(normed [C,N,total] with NaN at its missing readings, target [N,total], table [period,C,N], total), on the host.
    total is a little over two periods (and over the history), so windows cross the wrap of the period.  Nodes 0..12
    carry the hand-made patterns (N >= 100), the others random gaps."""
    history = tau * 24
    total = max(2 * period + 9, history + 64 + 40)
    g = torch.Generator().manual_seed(C_ * 1000 + N + tau + period)
    normed = torch.randn(C_, N, total, generator=g)
    gaps = torch.rand(N, total, generator=g) < 0.08            # all channels of a reading
    gaps[:13] = False
    normed[:, gaps] = NAN
    one = torch.rand(C_, N, total, generator=g) < 0.02         # single channels
    one[:, :13] = False
    normed[one] = NAN
    normed[:, :, 0], normed[:, 8, total - 1] = 0.5, NAN        # the two ends of the series
    normed[0, 0, 0] = NAN
    t = history + 3                                            # an origin the tests use
    normed[:, 1, t - tau] = NAN                                # first step of the window one hour back
    normed[:, 2, t - 1] = NAN                                  # its last step
    normed[:, 3, t - 2 * tau: t] = NAN                         # whole windows
    normed[:, 4] = NAN                                         # a whole node
    normed[C_ - 1, 5, t - tau: t] = NAN                        # one channel only: validity 0, the others untouched
    normed[0, 6, t - tau] = float("inf")
    normed[0, 6, t - tau + 1] = -0.0
    normed[0, 6, t - tau + 2] = 1e-41                          # a denormal
    normed[0, 6, t - tau + 3] = -float("inf")
    table = torch.randn(period, C_, N, generator=g)
    table[0, 0, 0] = -0.0
    target = torch.randn(N, total, generator=g) * 30
    target[torch.rand(N, total, generator=g) < 0.05] = 0.0     # null values: Y keeps them
    target.view(torch.int32)[2, t] = 0x7fa00001                # a NaN with a payload: Y keeps its bits
    target[3, t + 1] = NAN
    return normed, target, table, total


def origin_sets(history, last, B):
    t = history + 3
    if B == 1:
        return [[t], [history], [last]]
    return [[last, t, history], [t + 1, last - 1, t]]


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("period", [1, 20, "week"])
@pytest.mark.parametrize("C_,N", [(1, 100), (3, 100), (3, 257)])
@pytest.mark.parametrize("tau", [4, 8, 12, 16])
def test_kernel_equals_the_torch_restatement(tau, C_, N, period, mask):
    from ms_gat_amd import data
    period = 7 * 24 * tau if period == "week" else period
    normed, target, table, total = series_case(C_, N, tau, period)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    table_dev = table.to(DEV)
    history = tau * 24
    assert (C_ * N) % 256 and ((C_ + 1) * N) % 256 and total > 2 * period
    for B in (1, 3):
        for R in (1, 3):
            for q in (1, 12, 64):
                for origins in origin_sets(history, total - q, B):
                    o = torch.tensor(origins, dtype=torch.int64, device=DEV)
                    what = (B, R, q, origins)
                    got = launch(series_dev, table_dev, target_dev, o, HOURS[R], tau, q, mask)
                    want = data._windows_torch(series_dev, target_dev, o, HOURS[R], tau, q, climatology=table_dev,
                                               mask_channel=mask)
                    assert tuple(got[0].shape) == (B, R, C_ + mask, N, tau), what
                    assert_batches_equal(got, _on_cpu(want), what)
                    assert not bool(torch.isnan(got[0]).any()), what


def test_the_patterns_read_as_they_should():
    """What the hand-made patterns of `series_case` must give, stated directly (not through the twin)."""
    from ms_gat_amd import data, ops
    tau, C_, N, period, q = 12, 3, 100, 20, 12
    normed, target, table, total = series_case(C_, N, tau, period)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    t = tau * 24 + 3
    o = torch.tensor([t], dtype=torch.int64, device=DEV)
    x, h, d, y = _on_cpu(ops.window_gather_imputed(series_dev, table.to(DEV), target_dev, o, [1, 2, 24], tau, q))
    x, valid = x[0, 0, :C_], x[0, 0, C_]                       # the window one hour back: steps t - tau .. t - 1
    slots = torch.arange(t - tau, t) % period
    bits = lambda a: a.contiguous().view(torch.int32)  # noqa: E731
    assert valid[1].tolist() == [0.0] + [1.0] * (tau - 1) and valid[2].tolist() == [1.0] * (tau - 1) + [0.0]
    assert torch.equal(bits(x[:, 1, 0]), bits(table[slots[0], :, 1])) and torch.equal(bits(x[:, 1, 1:]), bits(normed[:, 1, t - tau + 1: t]))
    assert not valid[3].any() and not valid[4].any() and not valid[5].any() and bool(valid[6].all())
    for n in (3, 4):
        assert torch.equal(bits(x[:, n]), bits(table[slots][:, :, n].T))
    assert torch.equal(bits(x[:2, 5]), bits(normed[:2, 5, t - tau: t]))          # the observed channels keep their readings
    assert torch.equal(bits(x[2, 5]), bits(table[slots, 2, 5]))
    assert bits(x[0, 6, :4]).tolist() == [0x7f800000, -0x80000000, 7136, -0x00800000]       # inf, -0.0, 1e-41, -inf
    assert int(bits(y)[0, 2, 0]) == 0x7fa00001 and bool(torch.isnan(y[0, 3, 1])) and bool((y == 0).any())
    assert int(h[0]) == (t // tau) % 24 and int(d[0]) == (t // tau // 24) % 7


@pytest.mark.parametrize("mask", [True, False])
def test_without_missing_readings_x_is_the_plain_gather(mask):
    from ms_gat_amd import data, ops
    tau, q, hours = 12, 12, [1, 2, 24]
    g = torch.Generator().manual_seed(8)
    normed, target = torch.randn(3, 257, 400, generator=g), torch.randn(257, 400, generator=g)
    table = torch.full((20, 3, 257), 9.0)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    o = torch.tensor([288, 388, 300, 301, 333], dtype=torch.int64, device=DEV)
    plain = ops.window_gather(series_dev, target_dev, o, hours, tau, q)
    got = ops.window_gather_imputed(series_dev, table.to(DEV), target_dev, o, hours, tau, q, mask_channel=mask)
    assert_batches_equal([got[0][:, :, :3].contiguous(), *got[1:]], _on_cpu(plain))
    if mask:
        assert bool((got[0][:, :, 3] == 1).all())
    again = ops.window_gather_imputed(series_dev, table.to(DEV), target_dev, o, hours, tau, q, mask_channel=mask)
    assert_batches_equal(again, _on_cpu(got), "two calls")


@pytest.mark.parametrize("mask", [True, False])
def test_out_of_range_origins_are_clamped_as_the_plain_kernel_clamps_them(mask):
    from ms_gat_amd import data, ops
    tau, q, period = 12, 5, 20
    normed, target, table, total = series_case(3, 100, tau, period)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    lo, hi = tau * 24, total - q
    wild = torch.tensor([lo - 3, lo - 1, lo, hi, hi + 1, hi + 3, -5, 2 ** 40, -2 ** 62, 0, total, 2 ** 31 + 7], dtype=torch.int64)
    got = launch(series_dev, table.to(DEV), target_dev, wild.to(DEV), [1, 2, 24], tau, q, mask)
    want = data._windows_torch(series_dev, target_dev, wild.clamp(lo, hi).to(DEV), [1, 2, 24], tau, q,
                               climatology=table.to(DEV), mask_channel=mask)
    assert_batches_equal(got, _on_cpu(want))
    plain = ops.window_gather(series_dev, target_dev, wild.to(DEV), [1, 2, 24], tau, q)
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])                 # H, D, Y: the plain kernel's
    assert torch.equal(got[3].view(torch.int32), plain[3].view(torch.int32))


def test_more_work_items_than_the_grid_cap():
    """B = 2^18 + 3 samples of R = 4 components, C = N = 1: 2^20 + 12 X tiles and B target tiles for a grid capped at
    2^20 blocks, so the grid-stride loop runs.  X is 33.6 MB."""
    from ms_gat_amd import data
    tau, q, hours, period, B, total = 4, 1, [1, 2, 3, 6], 20, 2 ** 18 + 3, 211
    g = torch.Generator().manual_seed(12)
    normed, target = torch.randn(1, 1, total, generator=g), torch.randn(1, total, generator=g)
    normed[0, 0, torch.rand(total, generator=g) < 0.2] = NAN
    table = torch.randn(period, 1, 1, generator=g).to(DEV)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    o = torch.randint(tau * 6 - 2, total - q + 3, (B,), generator=g)
    got = launch(series_dev, table, target_dev, o.to(DEV), hours, tau, q, True)
    want = data._windows_torch(series_dev, target_dev, o.clamp(tau * 6, total - q).to(DEV), hours, tau, q,
                               climatology=table, mask_channel=True)
    assert got[0].numel() * 4 > 33e6 and B * 4 > 2 ** 20
    for name, a, b in zip("XHDY", got, want):
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), name
    assert 0 < float(got[0][:, :, 1].mean()) < 1


def _series_with_zeros():
    g = torch.Generator().manual_seed(11)
    raw = (40 + 8 * torch.randn(2, 6, 140, generator=g)).clamp_min(1.0)
    down = torch.rand(6, 140, generator=g) < 0.1
    down[4] = True
    raw[:, down] = 0.0
    raw[1, 2, 50:60] = 0.0
    return raw


@pytest.mark.parametrize("impute,mask", [("period", True), ("mean", False)])
def test_device_loaders_equal_the_cpu_loaders(impute, mask):
    from ms_gat_amd import data
    raw = _series_with_zeros()
    kw = dict(input_null_value=0.0, impute=impute, mask_channel=mask, seed=2)
    on_dev = data.make_loaders(raw, [1, 2], 3, 4, 5, device=DEV, **kw)
    on_cpu = data.make_loaders(raw, [1, 2], 3, 4, 5, device="cpu", **kw)
    assert on_dev[0].series is on_dev[2].series and on_dev[0].climatology is on_dev[1].climatology is on_dev[2].climatology
    period = 7 * 24 * 4 if impute == "period" else 1
    for d, c in zip(on_dev, on_cpu):
        assert d.climatology.is_cuda and d.resident_bytes == c.resident_bytes == 4 * 140 * 6 * 3 + 4 * period * 2 * 6
        for epoch in (0, 2):
            d.batch_sampler.set_epoch(epoch)
            c.batch_sampler.set_epoch(epoch)
            got, want = list(d), list(c)
            assert len(got) == len(want) > 1
            for k, (a, b) in enumerate(zip(got, want)):
                assert a[0].is_cuda and tuple(a[0].shape[1:]) == (2, 2 + mask, 6, 4)
                assert_batches_equal(a, b, (epoch, k))


def test_a_captured_gather_follows_new_origins():
    from ms_gat_amd import data, ops
    tau, q, hours, period = 12, 12, [1, 2, 24], 20
    normed, target, table, total = series_case(3, 100, tau, period)
    series_dev, target_dev = data.upload_series(normed, target, DEV)
    table_dev = table.to(DEV)
    offsets = ops.window_offsets(hours, tau, torch.device(DEV))
    first = torch.tensor([tau * 24 + 3, total - q, tau * 24], dtype=torch.int64)
    origins = first.to(DEV)

    def gather():
        return ops.window_gather_imputed(series_dev, table_dev, target_dev, origins, hours, tau, q, offsets=offsets)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gather()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gather()
    for o in (first, torch.tensor([300, 291, 350], dtype=torch.int64), torch.tensor([2 ** 40, -1, 333], dtype=torch.int64)):
        origins.copy_(o.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = data._windows_torch(series_dev, target_dev, o.clamp(tau * 24, total - q).to(DEV), hours, tau, q,
                                   climatology=table_dev, mask_channel=True)
        assert_batches_equal(out, _on_cpu(want), o.tolist())


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _synthetic(**kw):
    from ms_gat_amd import data
    return data.SyntheticPEMS(n_nodes=24, n_edges=30, n_channels=2, in_hours=[1, 2], batch_size=8, days=3, missing=0.05,
                              dead_sensors=2, **kw)


def test_a_model_trains_on_a_series_with_outages_and_skips_no_step(tmp_path):
    from ms_gat_amd import data, engine, model
    torch.manual_seed(0)
    ds = _synthetic(input_null_value=0.0, device=DEV)
    assert ds.input_channels == 3 and ds.num_channels == 2
    net = model.msgat48(n_components=2, in_channels=ds.input_channels, in_timesteps=12, out_timesteps=12, use_te=True,
                        adj=ds.adj).to(DEV)
    twin = copy.deepcopy(net)
    batches = [b for _, b in zip(range(5), ds.training)]
    assert tuple(batches[0][0].shape) == (8, 2, 3, 24, 12) and not any(bool(torch.isnan(b[0]).any()) for b in batches)
    assert any(bool((b[0][:, :, 2] == 0).any()) for b in batches) and any(bool((b[3] == 0).any()) for b in batches)
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, null_value=0.0, skip_nonfinite=True)
    auto = engine.Trainer(twin, 50.0, str(tmp_path / "auto"), hip_graph="auto", null_value=0.0, skip_nonfinite=True)
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        la = auto.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        print(f"epoch {epoch}: loss eager {le!r}, auto {la!r}")
        assert le == le and abs(le) < float("inf") and abs(le - la) < 1e-4 * abs(le), (epoch, le, la)
        assert eager.last_stats["skipped_steps"] == 0 and auto.last_stats["skipped_steps"] == 0
    assert len(auto._graphs) == 1
    # what the feature is for: the same series, its zeros turned to NaN to be honest about them, through the plain loaders
    raw = ds.raw.clone()
    raw[raw == 0] = NAN
    plain = data.make_loaders(raw, [1, 2], 12, 12, 8, device=DEV)[0]
    net2 = model.msgat48(n_components=2, in_channels=2, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj).to(DEV)
    tr = engine.Trainer(net2, 50.0, str(tmp_path / "plain"), hip_graph=False, null_value=0.0, skip_nonfinite=True)
    tr.run_epoch([b for _, b in zip(range(3), plain)], gpu_id=0, epoch=1, mode="train")
    assert tr.last_stats["skipped_steps"] > 0


def test_a_signal_model_sizes_its_projection_from_the_validity_channel_too(tmp_path):
    from ms_gat_amd import engine, model
    torch.manual_seed(0)
    ds = _synthetic(input_null_value=0.0, device=DEV)
    net = model.msgat48(n_components=2, in_channels=ds.input_channels, in_timesteps=12, out_timesteps=12, use_te=True,
                        adj=ds.adj, learn_edge_weights="signal").to(DEV)
    assert net.edge_proj.in_features == (ds.num_channels + 1) * 12
    tr = engine.Trainer(net, 50.0, str(tmp_path), hip_graph=False, null_value=0.0, skip_nonfinite=True)
    loss = tr.run_epoch([next(iter(ds.training))], gpu_id=0, epoch=1, mode="train")
    assert loss == loss and abs(loss) < float("inf") and tr.last_stats["skipped_steps"] == 0
