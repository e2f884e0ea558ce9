"""CPU: missing input readings -- `data.prepare_missing` (statistics and the slot table of the valid training entries),
the torch restatement of `ops.window_gather_imputed` (`data._windows_torch` with a table), the loaders that use them and
`SyntheticPEMS`'s outages.  Expected values come from plain loops written here.  Every comparison is exact (int32 views).
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from conftest import ROOT
from device_windows_fixtures import assert_batches_equal, host_loader

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


def bits(t):
    return t.contiguous().view(torch.int32)


def test_entry_point_is_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+msgat_window_gather_imputed\s*\(([^)]*)\)\s*;", code)
    assert decl, "msgat_window_gather_imputed is not declared in include/msgat_hip.h"
    n_args = len(decl.group(1).split(","))
    assert n_args == 20 and decl.group(1).strip().endswith("void* stream")
    assert "msgat_window_gather_imputed" in _lib.exported_symbols()
    assert len(_lib._PROTOTYPES["msgat_window_gather_imputed"][1]) == n_args
    assert hasattr(C.CDLL(_lib.LIB_PATH), "msgat_window_gather_imputed")
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10


def test_status_codes_come_back_before_anything_is_enqueued():
    from ms_gat_amd import _lib
    f = _lib.lib().msgat_window_gather_imputed
    p = [1] * 9      # never dereferenced: every call below is refused on its dimensions
    assert f(*[None] * 9, 1, 1, 1, 1, 100, 12, 12, 12, 7, 1, None) == -1
    for k in range(9):                                         # each pointer on its own, the table among them
        assert f(*[None if i == k else 1 for i in range(9)], 1, 1, 1, 1, 100, 12, 12, 12, 7, 1, None) == -1, k
    assert f(*p, 1, 1, 1, 1, 23, 12, 12, 12, 7, 1, None) == -2     # T_total < history + q
    assert f(*p, 0, 1, 1, 1, 100, 12, 12, 12, 7, 1, None) == -2    # B = 0
    assert f(*p, 1, 1, 1, 1, 100, 12, 12, 12, 0, 1, None) == -2    # period = 0
    assert f(*p, 1, 1, 1, 1, 100, 12, 12, 12, -3, 0, None) == -2
    assert f(*p, 1, 1, 1, 1, 100, 10, 12, 12, 7, 1, None) == -3    # tau = 10
    assert f(*p, 1, 1, 1, 1, 100, 12, 65, 12, 7, 1, None) == -3    # q = 65
    assert f(*p, 1, 1, 1, 1, 100, 12, 0, 12, 7, 0, None) == -3     # q = 0
    # C * N fits the int bound, (C + 1) * N does not -- refused with and without the validity channel
    assert f(*p, 1, 1, 1, 0x7fffff00 // 2 + 1, 100, 12, 1, 12, 7, 1, None) == -3
    assert f(*p, 1, 1, 1, 0x7fffff00 // 2 + 1, 100, 12, 1, 12, 7, 0, None) == -3


# ---- prepare_missing against a loop ---------------------------------------------------------------------------------
def _raw_with_gaps(null):
    """[2, 5, 203]: node 0 complete; node 1 with scattered gaps (null values and NaNs); node 2 all missing in channel 0
    and with ONE valid training entry in channel 1; node 3 constant; node 4 valid only after the split in channel 0."""
    g = torch.Generator().manual_seed(7)
    raw = 50 + 10 * torch.randn(2, 5, 203, generator=g)
    gaps = torch.rand(2, 203, generator=g) < 0.2
    raw[:, 1][gaps] = null
    raw[0, 1, 3] = raw[1, 1, 150] = NAN
    raw[0, 2] = null
    raw[1, 2, :120] = null
    raw[1, 2, 17] = 42.5
    raw[:, 3] = 7.25
    raw[0, 3, 5] = null
    raw[0, 4, :120] = null
    return raw


def _prepare_loop(raw, split, null, period):
    raw = raw.numpy()
    C_, N, T = raw.shape
    normed = np.full((C_, N, T), np.nan, dtype=np.float32)
    table = np.zeros((period, C_, N), dtype=np.float32)
    for c in range(C_):
        for n in range(N):
            def ok(t):
                v = raw[c, n, t]
                return not (math.isnan(v) or v == null)
            head = [float(raw[c, n, t]) for t in range(split) if ok(t)]
            mean = sum(head) / len(head) if head else 0.0
            std = 1.0
            if len(head) >= 2:
                s = math.sqrt(sum((v - mean) ** 2 for v in head) / (len(head) - 1))
                std = s if s > 0 else 1.0
            mean, std = np.float32(mean), np.float32(std)
            for t in range(T):
                if ok(t):
                    normed[c, n, t] = (raw[c, n, t] - mean) / std
            for s in range(period):
                vals = [float(normed[c, n, t]) for t in range(s, split, period) if ok(t)]
                if vals:
                    table[s, c, n] = np.float32(sum(vals) / len(vals))
    return torch.from_numpy(normed), torch.from_numpy(table)


@pytest.mark.parametrize("null,period", [(0.0, 20), (0.0, 1), (-1.0, 130), (NAN, 20)])
def test_prepare_missing_equals_a_plain_loop(null, period):
    from ms_gat_amd import data
    raw = _raw_with_gaps(0.0 if math.isnan(null) else null)
    split = 120
    normed, table = data.prepare_missing(raw, split, null, period)
    want_n, want_t = _prepare_loop(raw, split, null, period)
    assert normed.dtype == table.dtype == torch.float32
    assert tuple(normed.shape) == (2, 5, 203) and tuple(table.shape) == (period, 2, 5)
    missing = torch.isnan(raw) if math.isnan(null) else torch.isnan(raw) | (raw == null)
    assert torch.equal(torch.isnan(normed), missing) and bool(torch.isfinite(normed[~missing]).all())
    assert bool(torch.isfinite(table).all())
    assert torch.equal(bits(normed), bits(want_n)) and torch.equal(bits(table), bits(want_t))
    if math.isnan(null):
        assert int(missing.sum()) == 2                         # the two NaNs only: the zeros are readings
        return
    # degenerate rows: all missing -> (0, 1); one valid entry -> (that value, 1); constant -> (the constant, 1)
    assert bool(torch.isnan(normed[0, 2]).all()) and bool((table[:, 0, 2] == 0).all())
    assert float(normed[1, 2, 17]) == 0.0 and torch.equal(normed[1, 2, 120:], raw[1, 2, 120:] - 42.5)
    assert bool((normed[1, 3] == 0).all()) and bool((normed[0, 3][~missing[0, 3]] == 0).all())
    assert torch.equal(normed[0, 4, 120:], raw[0, 4, 120:])    # no valid training entry: mean 0, std 1
    if period == 130:
        assert bool((table[120:] == 0).all())                  # slots no training step falls into
    # the statistics ignore missing entries: the complete node 0 is the plain z-score
    assert torch.allclose(normed[:, 0], data.zscore(raw[:, :1], split)[:, 0], rtol=0, atol=1e-5)


def test_nothing_past_the_split_reaches_the_statistics_or_the_table():
    from ms_gat_amd import data
    raw = _raw_with_gaps(0.0)
    other = raw.clone()
    other[..., 120:] = torch.randn(2, 5, 83, generator=torch.Generator().manual_seed(1)) * 100
    a, ta = data.prepare_missing(raw, 120, 0.0, 20)
    b, tb = data.prepare_missing(other, 120, 0.0, 20)
    assert torch.equal(bits(ta), bits(tb)) and torch.equal(bits(a[..., :120]), bits(b[..., :120]))


# ---- the torch twin against a per-entry loop --------------------------------------------------------------------------
def _twin_loop(normed, target, table, origins, hours, tau, q, mask):
    C_, N, _ = normed.shape
    period = table.shape[0]
    x = torch.empty(len(origins), len(hours), C_ + mask, N, tau)
    for b, t in enumerate(origins):
        for r, h in enumerate(hours):
            for n in range(N):
                for k in range(tau):
                    step = t - h * tau + k
                    seen = True
                    for c in range(C_):
                        v = normed[c, n, step]
                        if math.isnan(float(v)):
                            v, seen = table[step % period, c, n], False
                        bits(x)[b, r, c, n, k] = bits(v.reshape(1))[0]
                    if mask:
                        x[b, r, C_, n, k] = 1.0 if seen else 0.0
    y = torch.stack([target[:, t: t + q] for t in origins])
    hour = torch.tensor(origins) // tau
    return x, hour % 24, (hour // 24) % 7, y


def _twin_case(C_, period, seed=3):
    tau, hours, q, N = 4, [1, 3], 3, 4
    total = 2 * period + 9 if period > 20 else 50
    g = torch.Generator().manual_seed(seed)
    normed = torch.randn(C_, N, total, generator=g)
    normed[torch.rand(C_, N, total, generator=g) < 0.15] = NAN
    normed[0, 2] = NAN                                         # a dead sensor
    normed[-1, 1, 20:30] = NAN                                 # whole windows of one channel
    normed[0, 0, 0], normed[0, 0, 1], normed[0, 3, 2] = -0.0, float("inf"), 1e-41
    table = torch.randn(period, C_, N, generator=g)
    target = torch.randn(N, total, generator=g)
    target[1, 14] = NAN
    return normed, target, table, hours, tau, q, total


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("period", [1, 20, 23])
@pytest.mark.parametrize("mask", [False, True])
def test_torch_twin_equals_a_per_entry_loop(C_, period, mask):
    from ms_gat_amd import data
    normed, target, table, hours, tau, q, total = _twin_case(C_, period)
    history = tau * max(hours)
    # both ends of the series, windows that cross the wrap of the period (a window of 4 steps from 18, 19, 21, 22, ...),
    # and origins outside the valid range, clamped as the kernel clamps them
    wild = [history, total - q, history + 7, 30, 31, 33, 34, 35, -5, 2 ** 40, history - 1, total - q + 1]
    origins = [min(max(t, history), total - q) for t in wild]
    assert period == 1 or any((t - h * tau) % period > (t - h * tau + tau - 1) % period for t in origins for h in hours)
    series_tm, target_c = data.upload_series(normed, target, "cpu")
    got = data._windows_torch(series_tm, target_c, torch.tensor(origins), hours, tau, q, climatology=table,
                              mask_channel=mask)
    want = _twin_loop(normed, target, table, origins, hours, tau, q, mask)
    assert_batches_equal(got, want, (C_, period, mask))
    assert not bool(torch.isnan(got[0]).any()) and bool(torch.isnan(got[3]).any())
    assert tuple(got[0].shape) == (len(origins), 2, C_ + mask, 4, tau)
    # without a table the function is what it was: the NaNs pass through
    plain = data._windows_torch(series_tm, target_c, torch.tensor(origins), hours, tau, q)
    observed = ~torch.isnan(plain[0])
    assert torch.equal(bits(plain[0])[observed], bits(got[0][:, :, :C_])[observed])
    # PeriodicWindows gives the same items one by one
    ds = data.PeriodicWindows(normed, target, (history, total - q + 1), hours, q, tau, climatology=table, mask_channel=mask)
    items = [ds[t - history] for t in origins]
    assert_batches_equal([torch.stack([it[j] for it in items]) for j in range(4)], want, "items")


# ---- loaders ----------------------------------------------------------------------------------------------------------
def _series_with_zeros():
    g = torch.Generator().manual_seed(11)
    raw = (40 + 8 * torch.randn(2, 6, 140, generator=g)).clamp_min(1.0)
    down = torch.rand(6, 140, generator=g) < 0.1
    down[4] = True
    raw[:, down] = 0.0
    raw[1, 2, 50:60] = 0.0                                     # one channel only
    return raw


@pytest.mark.parametrize("impute,mask", [("period", True), ("period", False), ("mean", True)])
def test_host_loaders_and_cpu_device_windows_yield_the_same_batches(impute, mask):
    from ms_gat_amd import data
    raw, hours, q, tau, bs = _series_with_zeros(), [1, 2], 3, 4, 5
    kw = dict(input_null_value=0.0, impute=impute, mask_channel=mask)
    host = data.make_loaders(raw, hours, q, tau, bs, **kw)
    dev = data.make_loaders(raw, hours, q, tau, bs, device="cpu", seed=9, **kw)
    assert all(type(l) is DataLoader for l in host) and all(type(l) is data.DeviceWindows for l in dev)
    assert dev[0].series is dev[1].series is dev[2].series and dev[0].climatology is dev[2].climatology
    period = 7 * 24 * tau if impute == "period" else 1
    assert tuple(dev[0].climatology.shape) == (period, 2, 6)
    assert (impute == "mean") == bool((dev[0].climatology == 0).all())
    assert dev[0].resident_bytes == 4 * 140 * 6 * (2 + 1) + 4 * period * 2 * 6
    assert bool(torch.isnan(dev[0].series).any())              # the resident series keeps NaN at the missing readings
    for i, (h, d) in enumerate(zip(host, dev)):
        ds = h.dataset
        assert ds.climatology is not None and ds.mask_channel == mask
        # the host DataLoader of a single process shuffles with torch's global generator: walk the dataset make_loaders
        # built with the sampler DeviceWindows walks, for every epoch
        twin = DataLoader(ds, batch_sampler=data.ShardedBatchSampler(len(ds), bs, i == 0, 0, 1, 9))
        for epoch in (0, 1, 4):
            d.batch_sampler.set_epoch(epoch)
            twin.batch_sampler.set_epoch(epoch)
            got, want = list(d), list(twin)
            assert len(got) == len(want) == len(h) > 1
            for k, (a, b) in enumerate(zip(got, want)):
                assert_batches_equal(a, b, (i, epoch, k))
                assert tuple(a[0].shape[1:]) == (2, 2 + mask, 6, tau) and not bool(torch.isnan(a[0]).any())
        if i:                                                  # the two that do not shuffle: the loader as returned
            for a, b in zip(d, h):
                assert_batches_equal(a, b, i)
    x, _, _, y = next(iter(dev[1]))
    assert bool((y == 0).any())                                # Y keeps the raw target, null values included
    if mask:
        assert bool((x[:, :, 2, 4] == 0).all()) and 0 < float(x[:, :, 2].mean()) < 1
        if impute == "mean":
            assert bool((x[:, :, :2, 4] == 0).all())           # the dead sensor reads as the z-score mean


def test_without_input_null_value_the_loaders_are_the_parents():
    from ms_gat_amd import data
    raw, hours, q, tau, bs = _series_with_zeros(), [1, 2], 3, 4, 5
    intervals, train_end = data.split_intervals(raw.size(-1), hours, q, tau)
    normed = data.zscore(raw, split=train_end)
    for kw in ({}, dict(mask_channel=True, impute="mean"), dict(input_null_value=None, mask_channel=False)):
        host = data.make_loaders(raw, hours, q, tau, bs, **kw)
        dev = data.make_loaders(raw, hours, q, tau, bs, device="cpu", **kw)
        for i, iv in enumerate(intervals):
            assert host[i].dataset.climatology is None and dev[i].climatology is None and not dev[i].mask_channel
            assert dev[i].resident_bytes == 4 * 140 * 6 * 3
            want = host_loader(normed, raw[0], iv, hours, q, tau, bs, False, 0, 1, 0)
            plain = data.DeviceWindows(normed, raw[0], iv, hours, q, tau, bs, device="cpu")
            for a, b, c in zip(plain, want, DataLoader(host[i].dataset, bs)):
                assert_batches_equal(a, b, i)
                assert_batches_equal(c, b, i)
            if i:
                for a, b in zip(dev[i], want):
                    assert_batches_equal(a, b, i)


def test_a_bad_impute_value_is_refused():
    from ms_gat_amd import data
    raw = _series_with_zeros()
    for kw in (dict(input_null_value=0.0), {}):
        with pytest.raises(ValueError, match="impute"):
            data.make_loaders(raw, [1, 2], 3, 4, 5, impute="locf", **kw)
    with pytest.raises(ValueError, match="impute"):
        data.SyntheticPEMS(5, 6, 1, [1, 2], batch_size=8, days=1, input_null_value=0.0, impute="neighbours")


def test_synthetic_series_defaults_keep_their_bits_and_outages_are_seeded():
    from ms_gat_amd import data
    from ms_gat_amd.graph import synthetic_adjacency
    a = data.SyntheticPEMS(24, 30, 2, [1, 2], batch_size=8, days=3, seed=4)
    # the parent's series, restated: generator seed + 1, base then noise
    g = torch.Generator().manual_seed(5)
    t = torch.arange(3 * 24 * 12, dtype=torch.float32)
    base = 200 + 80 * torch.rand(2, 24, 1, generator=g)
    want = (base * (1 + 0.4 * torch.sin(2 * torch.pi * t / (24 * 12))) + 15 * torch.randn(2, 24, 864, generator=g)).clamp_min(1.0)
    assert torch.equal(bits(a.raw), bits(want)) and torch.equal(a.adj, synthetic_adjacency(24, 30, 4))
    assert a.input_channels == a.num_channels == 2 and not bool((a.raw == 0).any())
    b = data.SyntheticPEMS(24, 30, 2, [1, 2], batch_size=8, days=3, seed=4, missing=0.05, dead_sensors=2)
    down = b.raw[0] == 0
    assert torch.equal(down, b.raw[1] == 0)                    # all channels of a reading go together
    assert torch.equal(bits(b.raw)[:, ~down], bits(a.raw)[:, ~down])
    dead = down.all(1)
    assert int(dead.sum()) == 2
    share = float(down[~dead].float().mean())
    assert 0.035 < share < 0.055, share                        # overlapping runs make it a little less than asked
    runs = (down[~dead][:, 1:] & ~down[~dead][:, :-1]).sum() + down[~dead][:, 0].sum()
    assert float(down[~dead].sum() / runs) > 6                 # in runs (12 steps on average), not single readings
    assert b.input_channels == 2 and type(b.training) is DataLoader    # no input_null_value: the plain loaders
    c = data.SyntheticPEMS(24, 30, 2, [1, 2], batch_size=8, days=3, seed=4, missing=0.05, dead_sensors=2,
                           input_null_value=0.0, device="cpu")
    assert torch.equal(bits(c.raw), bits(b.raw)) and c.input_channels == 3 and c.num_channels == 2
    x, _, _, y = next(iter(c.validation))
    assert tuple(x.shape) == (8, 2, 3, 24, 12) and not bool(torch.isnan(x).any())
    d = data.SyntheticPEMS(24, 30, 2, [1, 2], batch_size=8, days=3, seed=4, missing=0.05, input_null_value=0.0,
                           mask_channel=False)
    assert d.input_channels == 2 and tuple(next(iter(d.validation))[0].shape) == (8, 2, 2, 24, 12)
    e = data.SyntheticPEMS(24, 30, 2, [1, 2], batch_size=8, days=3, seed=5, missing=0.05, dead_sensors=2)
    assert not torch.equal(e.raw[0] == 0, down)


def test_msgat_data_passes_the_options_on_and_reports_the_input_channels(tmp_path):
    from ms_gat_amd import data
    raw = _series_with_zeros()                                 # [C,N,T_total]; the file holds [T_total,N,C]
    np.savez(tmp_path / "series.npz", data=raw.permute(2, 1, 0).numpy())
    (tmp_path / "adj.csv").write_text("from,to,cost\n0,1,1.0\n1,2,1.0\n4,5,1.0\n")
    meta = {"adj-file": str(tmp_path / "adj.csv"), "data-file": str(tmp_path / "series.npz"), "num-nodes": 6,
            "num-channels": 2, "timesteps-per-hour": 4}
    plain = data.MSGATData("x", [1, 2], 3, 5, meta=meta)
    assert plain.input_channels == plain.num_channels == 2 and plain.training.dataset.climatology is None
    for mask in (True, False):
        got = data.MSGATData("x", [1, 2], 3, 5, meta=meta, device="cpu", input_null_value=0.0, impute="mean", mask_channel=mask)
        want = data.make_loaders(raw, [1, 2], 3, 4, 5, device="cpu", input_null_value=0.0, impute="mean", mask_channel=mask)
        assert got.input_channels == 2 + mask and got.num_channels == 2
        for a, b in zip(got.validation, want[1]):
            assert_batches_equal(a, b, mask)
            assert a[0].shape[2] == got.input_channels


def test_the_op_checks_its_arguments_before_any_launch():
    from ms_gat_amd import ops
    from ms_gat_amd._lib import MsgatError
    series, table, target = torch.zeros(40, 2, 3), torch.zeros(5, 2, 3), torch.zeros(3, 40)
    origins = torch.tensor([30], dtype=torch.int64)
    f = ops.window_gather_imputed
    bad = [
        (series.double(), table, target, origins, [1, 2], 12, 12),
        (series, table.double(), target, origins, [1, 2], 12, 12),
        (series, table, target.double(), origins, [1, 2], 12, 12),
        (series, table, target, origins.int(), [1, 2], 12, 12),
        (series, table.to("meta"), target, origins, [1, 2], 12, 12),                   # another device
        (series, table, target.to("meta"), origins, [1, 2], 12, 12),
        (series, table, target, origins.to("meta"), [1, 2], 12, 12),
        (series[:35].contiguous(), table, target[:, :35].contiguous(), origins, [1, 2], 12, 12),   # 35 < 24 + 12
        (series, table, torch.zeros(4, 40), origins, [1, 2], 12, 12),                   # shapes that do not fit
        (series, torch.zeros(5, 2, 4), target, origins, [1, 2], 12, 12),
        (series, torch.zeros(5, 3, 3), target, origins, [1, 2], 12, 12),
        (series, torch.zeros(0, 2, 3), target, origins, [1, 2], 12, 12),                # period = 0
        (series, torch.zeros(2, 3), target, origins, [1, 2], 12, 12),
        (series, table, target, origins, [1, 2], 10, 12),                               # tau
        (series, table, target, origins, [1, 2], 12, 65),                               # q
        (series, table, target, origins, [], 12, 12),
        (series, table.transpose(1, 2).contiguous().transpose(1, 2), target, origins, [1, 2], 12, 12),   # not contiguous
    ]
    for k, args in enumerate(bad):
        with pytest.raises((ValueError, TypeError)):
            f(*args)
            pytest.fail(f"case {k} was accepted")
    for mask in (True, False):
        with pytest.raises(MsgatError, match="no CPU path"):
            f(series, table, target, origins, [1, 2], 12, 12, mask_channel=mask)        # well-formed, but no CPU path
