"""GPU: `msgat_window_gather` / `data.DeviceWindows` -- every batch built on the device from the resident series.

The kernel copies, so every comparison is exact (int32 views: NaNs count).  Expected values come from the `device="cpu"`
restatement (`data._windows_torch`), which test_device_windows_cpu.py ties to the host DataLoader and to the
reference-generated goldens.
"""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from device_windows_fixtures import assert_batches_equal, host_loader, loader_golden, slices_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_kernel_reproduces_the_slices_golden():
    from ms_gat_amd import data
    args, idx, want = slices_golden()
    dw = data.DeviceWindows(*args, batch_size=len(range(*args[2])), device=DEV)
    (x, h, d, y), = list(dw)
    assert x.is_cuda and dw.resident_bytes == 4 * args[0].shape[2] * args[0].shape[1] * (args[0].shape[0] + 1)
    assert_batches_equal((x[idx], h[idx], d[idx], y[idx]), (want["x"], want["h"], want["d"], want["y"]), "slices_small")


def test_kernel_reproduces_the_loader_golden():
    from ms_gat_amd import data
    raw, hours, q, tau, bs, want = loader_golden()
    train, val, ev = data.make_loaders(raw, hours, q, tau, bs, device=DEV)
    assert train.series is val.series is ev.series and train.series.is_cuda
    for split, loader in (("val", val), ("eval", ev)):
        batches = list(loader)
        assert_batches_equal(batches[0], [want[f"{split}_{k}"] for k in "xhdy"], split)
        assert_batches_equal(batches[-1], [want[f"{split}_last_{k}"] for k in "xhdy"], split + " last")
    ds = train.dataset
    ordered = data.DeviceWindows(ds.inputs, ds.target, (ds.start, ds.stop), hours, q, tau, bs, shuffle=False, device=DEV,
                                 resident=(train.series, train.target))
    assert_batches_equal(next(iter(ordered)), [want[f"train_{k}"] for k in "xhdy"], "train")


def _origin_sets(first, last, B):
    """Origins of one launch each.  B = 1: the first valid origin (reads index 0 of the series), then the last (reads up to
    T_total - 1; odd).  Otherwise one set holding both, every odd origin in between (no 16-byte aligned window start:
    tau is a multiple of 4), even ones to fill up, and one origin twice -- in a scrambled order."""
    if B == 1:
        return [[first], [last]]
    inner = list(range(first + 1, last))
    picked = [first, last] + [t for t in inner if t % 2] + [t for t in inner if t % 2 == 0]
    picked = picked[: B - 1] + [picked[2]]
    order = torch.randperm(B, generator=torch.Generator().manual_seed(B)).tolist()
    return [[picked[i] for i in order]]


# (C, N): a single row, fewer rows than a wave, a partial last tile of 256 rows, an exact multiple of 64, the PEMSD7 N
@pytest.mark.parametrize("C_,N", [(1, 1), (2, 7), (3, 70), (3, 128), (1, 883)])
@pytest.mark.parametrize("tau", [4, 8, 12, 16])
@pytest.mark.parametrize("q", [1, 12, 24, 64])
@pytest.mark.parametrize("hours", [[1], [1, 2, 3, 24, 168]])
@pytest.mark.parametrize("B", [1, 33])
def test_kernel_equals_the_torch_restatement(C_, N, tau, q, hours, B):
    from ms_gat_amd import data, ops
    history = tau * max(hours)
    total = history + q + B + 2                      # valid origins: history .. history + B + 2, both ends of the series
    g = torch.Generator().manual_seed(1000 * C_ + N + tau + q)
    inputs, target = torch.randn(C_, N, total, generator=g), torch.randn(N, total, generator=g)
    for flat, k in ((inputs.view(-1), 9), (target.view(-1), 5)):     # missing readings
        at = torch.randint(flat.numel(), (k,), generator=g)
        flat.view(torch.int32)[at] = 0x7fc00000
        flat.view(torch.int32)[at[:2]] = 0x7fa00001                  # another NaN payload: the bits must survive
    inputs[0, 0, 0] = inputs[-1, -1, -1] = float("nan")              # the two ends of the series are among them
    series_cpu, target_cpu = data.upload_series(inputs, target, "cpu")
    series_dev, target_dev = data.upload_series(inputs, target, DEV)
    assert tuple(series_dev.shape) == (total, C_, N) and series_dev.is_contiguous()
    for origins in _origin_sets(history, total - q, B):
        assert len(origins) == B and min(origins) >= history and max(origins) <= total - q
        assert B == 1 or (len(set(origins)) == B - 1 and {history, total - q} <= set(origins))
        o = torch.tensor(origins, dtype=torch.int64)
        want = data._windows_torch(series_cpu, target_cpu, o, hours, tau, q)
        got = ops.window_gather(series_dev, target_dev, o.to(DEV), hours, tau, q)
        assert tuple(got[0].shape) == (B, len(hours), C_, N, tau) and tuple(got[3].shape) == (B, N, q)
        assert_batches_equal(got, want, origins)


def test_out_of_range_origins_are_clamped_to_the_nearest_valid_origin():
    from ms_gat_amd import data, ops
    hours, tau, q, total = [1, 3], 12, 5, 60                         # valid origins 36 .. 55
    g = torch.Generator().manual_seed(2)
    inputs, target = torch.randn(2, 70, total, generator=g), torch.randn(70, total, generator=g)
    series_dev, target_dev = data.upload_series(inputs, target, DEV)
    wild = torch.tensor([33, 35, 36, 55, 56, 58, 34, 57], dtype=torch.int64)         # up to three steps past either end
    want = data._windows_torch(*data.upload_series(inputs, target, "cpu"), wild.clamp(36, 55), hours, tau, q)
    assert_batches_equal(ops.window_gather(series_dev, target_dev, wild.to(DEV), hours, tau, q), want)


def test_offsets_past_two_to_the_31_elements():
    """A series of 2^31 + 32768 elements ([2^22 + 64, 8, 64]: 8.6 GB, with its 1.1 GB target) filled from a formula of
    (t, c, n); windows at its far end -- every element of the last ones lies past 2^31 -- against the formula evaluated
    on the host."""
    from ms_gat_amd import ops
    if torch.cuda.mem_get_info(0)[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory")
    C_, N, total, tau, q, hours = 8, 64, 2 ** 22 + 64, 12, 12, [1, 2]
    M = C_ * N
    assert total * M > 2 ** 31

    def series_value(t, m):          # exact in fp32
        return ((t * 31 + m * 17) % 8388593).to(torch.float32)

    def target_value(n, t):
        return ((t * 7 + n * 1009) % 8388593).to(torch.float32)

    series = torch.empty((total, C_, N), device=DEV, dtype=torch.float32)
    m_dev = torch.arange(M, device=DEV)
    for t0 in range(0, total, 2 ** 15):
        t = torch.arange(t0, min(t0 + 2 ** 15, total), device=DEV)
        series[t0: t0 + 2 ** 15] = series_value(t[:, None], m_dev[None, :]).view(-1, C_, N)
    target = torch.empty((N, total), device=DEV, dtype=torch.float32)
    t_dev = torch.arange(total, device=DEV)
    for n in range(N):
        target[n] = target_value(n, t_dev)
    origins = torch.tensor([total - q, total - q - 1, total - q - 7, 2 ** 21 + 3, tau * 2], dtype=torch.int64)
    x, h, d, y = ops.window_gather(series, target, origins.to(DEV), hours, tau, q)
    rows = origins[:, None, None] - torch.tensor(hours)[None, :, None] * tau + torch.arange(tau)        # [B,R,tau]
    assert int(rows[0].min()) * M > 2 ** 31 and int(rows.max()) == total - q - 1
    want_x = series_value(rows[..., None], torch.arange(M)[None, None, None, :]).permute(0, 1, 3, 2).reshape(x.shape)
    want_y = target_value(torch.arange(N)[None, :, None], (origins[:, None] + torch.arange(q))[:, None, :])
    assert_batches_equal((x, h, d, y), (want_x.contiguous(), (origins // tau) % 24, (origins // tau // 24) % 7,
                                        want_y.contiguous()))
    del series, target, x, y
    torch.cuda.empty_cache()


def test_target_offsets_past_two_to_the_31_elements():
    """The target's read offset n * T_total + t past 2^31 (the test above takes only the series' there): N = 130 rows of
    2^24 + 64 steps, 8.7 GB each for the series and the target; Y for the last nodes against the formula."""
    from ms_gat_amd import ops
    if torch.cuda.mem_get_info(0)[0] < 20 * 2 ** 30:
        pytest.skip("needs 20 GB of free device memory")
    N, total, tau, q, hours = 130, 2 ** 24 + 64, 4, 64, [1]
    assert (N - 1) * total > 2 ** 31

    def target_value(n, t):          # exact in fp32
        return ((t * 7 + n * 1009) % 8388593).to(torch.float32)

    series = torch.empty((total, 1, N), device=DEV, dtype=torch.float32)
    t_dev = torch.arange(total, device=DEV)
    for t0 in range(0, total, 2 ** 18):
        t = t_dev[t0: t0 + 2 ** 18, None]
        series[t0: t0 + 2 ** 18, 0] = (t % 1024 + 1024 * torch.arange(N, device=DEV)[None, :]).float()
    target = torch.empty((N, total), device=DEV, dtype=torch.float32)
    for n in range(N):
        target[n] = target_value(n, t_dev)
    origins = torch.tensor([total - q, total - q - 3, tau], dtype=torch.int64)
    x, h, d, y = ops.window_gather(series, target, origins.to(DEV), hours, tau, q)
    rows = origins[:, None] - tau + torch.arange(tau)                                                   # [B,tau]
    want_x = (rows[:, None, :] % 1024 + 1024 * torch.arange(N)[None, :, None]).float().view(x.shape)
    want_y = target_value(torch.arange(N)[None, :, None], (origins[:, None] + torch.arange(q))[:, None, :])
    assert_batches_equal((x, h, d, y), (want_x, (origins // tau) % 24, (origins // tau // 24) % 7, want_y.contiguous()))
    del series, target, x, y
    torch.cuda.empty_cache()


def test_output_offsets_past_two_to_the_31_elements():
    """X of 2^31 + 2^23 elements (8.6 GB: B = 1028, R = 16 equal components, C * N = 8192, tau = 16) from a small series:
    the write offset (b * R + r) * C * N * tau passes 2^31; the last samples -- all of whose elements lie past it -- and the
    first against the torch restatement."""
    from ms_gat_amd import data, ops
    if torch.cuda.mem_get_info(0)[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory")
    C_, N, tau, q, B = 8, 1024, 16, 1, 1028
    hours = [1, 2] * 8
    total = tau * 2 + q + 40
    g = torch.Generator().manual_seed(6)
    series, target = data.upload_series(torch.randn(C_, N, total, generator=g), torch.randn(N, total, generator=g), DEV)
    origins = torch.randint(2 * tau, total - q + 1, (B,), generator=g)
    x, h, d, y = ops.window_gather(series, target, origins.to(DEV), hours, tau, q)
    assert (B - 3) * len(hours) * C_ * N * tau > 2 ** 31 and x.numel() > 2 ** 31
    for part in (slice(0, 2), slice(B - 3, B)):
        want = data._windows_torch(series.cpu(), target.cpu(), origins[part], hours, tau, q)
        assert_batches_equal((x[part], h[part], d[part], y[part]), want, part)
    del x
    torch.cuda.empty_cache()


def test_epochs_through_the_engine_equal_the_host_loader_fed_twin(tmp_path):
    """Twin msgat48 models, one fed by the host DataLoader on `ShardedBatchSampler(seed)`, one by `DeviceWindows` of the
    same seed: the inputs are bit-identical, so the runs are two runs of one step sequence."""
    from ms_gat_amd import data, engine, model
    torch.manual_seed(0)
    syn = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    raw = syn.raw.clone()
    raw[0, 3, 100:140] = 0.0                                         # a sensor that was down: missing readings
    raw[0, 17, 400:470] = 0.0
    on_dev = data.make_loaders(raw, [1, 2], 12, 12, 8, seed=3, device=DEV)
    on_host = [host_loader(l.dataset.inputs, l.dataset.target, (l.dataset.start, l.dataset.stop), [1, 2], 12, 12, 8,
                           shuffle=(i == 0), rank=0, world=1, seed=3) for i, l in enumerate(on_dev)]
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=syn.adj).to(DEV)
    twin = copy.deepcopy(net)
    host = engine.Trainer(net, 50.0, str(tmp_path / "host"), null_value=0.0)
    dev = engine.Trainer(twin, 50.0, str(tmp_path / "dev"), null_value=0.0)
    # a validation epoch on identical parameters: valid counts and per-horizon metrics agree exactly
    vh = host.run_epoch(on_host[1], gpu_id=0, epoch=0, mode="validate")
    stats_h = dict(host.last_stats)
    vd = dev.run_epoch(on_dev[1], gpu_id=0, epoch=0, mode="validate")
    stats_d = dict(dev.last_stats)
    n_val = len(on_dev[1].dataset) * 40
    assert 0 < sum(stats_h["horizons"]["valid"]) < n_val * 12       # the planted zeros are in this split
    assert stats_h["horizons"] == stats_d["horizons"] and vh == vd
    for epoch in (1, 2, 3):
        lh = host.run_epoch(on_host[0], gpu_id=0, epoch=epoch, mode="train")
        ld = dev.run_epoch(on_dev[0], gpu_id=0, epoch=epoch, mode="train")
        print(f"epoch {epoch}: host-fed {lh!r} device-fed {ld!r}")
        assert abs(lh - ld) <= 1e-4 * abs(lh), (epoch, lh, ld)
    assert len(host._graphs) == len(dev._graphs) >= 2
    assert set(host.optimizer._host_steps) == set(dev.optimizer._host_steps) == {3 * len(on_dev[0])}
    host.save(str(tmp_path / "ck.pkl"))
    ev_h = engine.Evaluator(net, 50.0, str(tmp_path / "evh"), str(tmp_path / "ck.pkl"))
    ev_d = engine.Evaluator(twin, 50.0, str(tmp_path / "evd"), str(tmp_path / "ck.pkl"))
    eh, ed = ev_h.eval(on_host[2], gpu_id=0), ev_d.eval(on_dev[2], gpu_id=0)
    print(f"evaluation: host-fed {eh!r} device-fed {ed!r}")
    assert abs(eh - ed) <= 1e-5 * abs(eh), (eh, ed)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_RANKS_CASE = dict(in_hours=[1, 3], out_timesteps=5, tau=4, batch_size=6, seed=11)


def _ranks_series():
    g = torch.Generator().manual_seed(4)
    return torch.randn(2, 7, 91, generator=g) * 10 + 50      # 75 origins: 45 / 15 / 15, no multiple of the batch


def _rank_worker(rank, world, port, out_dir):
    """A rank's loaders as `make_loaders` builds them under a process group (rank and world come from the group), all
    ranks on cuda:0; two epochs of the shuffled training split and the validation split go to a file."""
    from ms_gat_amd import data
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    train, val, _ = data.make_loaders(_ranks_series(), device=DEV, **_RANKS_CASE)
    assert train.msgat_sharded and train.batch_sampler.rank == rank and train.batch_sampler.world == world
    got = {}
    for epoch in (0, 2):
        train.batch_sampler.set_epoch(epoch)
        got[f"train{epoch}"] = [[t.cpu() for t in b] for b in train]
    got["val"] = [[t.cpu() for t in b] for b in val]
    got["sizes"] = train.batch_sampler.global_batch_sizes()
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_partition_every_global_batch(tmp_path):
    """Rank 0's and rank 1's `DeviceWindows` shards, joined, are the global batches of the single-process order."""
    from ms_gat_amd import data, parallel
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ranks = [torch.load(str(tmp_path / f"rank{r}.pt"), weights_only=False) for r in (0, 1)]
    train, val, _ = data.make_loaders(_ranks_series(), rank=0, world=1, device="cpu", **_RANKS_CASE)
    assert len(train.dataset) % 6 not in (0, 1)                      # a ragged last global batch, shared by both ranks
    for key, loader, epoch in (("train0", train, 0), ("train2", train, 2), ("val", val, 0)):
        loader.batch_sampler.set_epoch(epoch)
        whole = list(loader)
        assert len(whole) == len(ranks[0][key]) == len(ranks[1][key])
        for k, batch in enumerate(whole):
            n = batch[0].shape[0]
            for r in (0, 1):
                lo, hi = parallel.shard_bounds(n, r, 2)
                assert_batches_equal(ranks[r][key][k], [t[lo:hi] for t in batch], (key, k, r))
    assert ranks[0]["sizes"] == ranks[1]["sizes"] == train.batch_sampler.global_batch_sizes()
