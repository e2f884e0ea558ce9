"""Shared by test_device_windows_cpu.py and test_gpu_device_windows.py: the two reference-generated loader goldens as
`DeviceWindows` arguments with the batches they must give, and the host loader a `DeviceWindows` is compared with."""
import torch
from torch.utils.data import DataLoader

from conftest import load_golden


def slices_golden():
    """slices_small.npz: (arguments of a DeviceWindows over the training split, idx, {x, h, d, y} at idx)."""
    from ms_gat_amd import data
    g = load_golden("slices_small.npz")
    raw = torch.from_numpy(g["raw"]).float().transpose(0, -1).contiguous()
    hours, tau, q = g["hours"].tolist(), int(g["tau"]), int(g["q"])
    intervals, train_end = data.split_intervals(raw.size(-1), hours, q, tau)
    normed = data.zscore(raw, split=train_end)
    want = {k: torch.from_numpy(g[k]) for k in "xhdy"}
    return (normed, raw[0], intervals[0], hours, q, tau), g["idx"].tolist(), want


def loader_golden():
    """loader_tiny.npz: (raw [C,N,T_total], hours, q, tau, batch size, the golden's arrays as tensors)."""
    g = load_golden("loader_tiny.npz")
    raw = torch.from_numpy(g["series"]).float().transpose(0, -1).contiguous()
    want = {k: torch.from_numpy(v) for k, v in g.items() if k.endswith(("_x", "_h", "_d", "_y"))}
    return raw, g["hours"].tolist(), int(g["q"]), int(g["tau"]), int(g["batch_size"]), want


def host_loader(inputs, target, interval, hours, q, tau, batch_size, shuffle, rank, world, seed):
    """The host path a DeviceWindows of the same arguments must reproduce batch for batch."""
    from ms_gat_amd import data
    ds = data.PeriodicWindows(inputs, target, interval, hours, q, tau)
    return DataLoader(ds, batch_sampler=data.ShardedBatchSampler(len(ds), batch_size, shuffle, rank, world, seed))


def assert_batches_equal(got, want, what=""):
    """Bit for bit (int32 views, so NaNs count), with the shapes, dtypes and contiguity of the collated host batch."""
    assert len(got) == len(want) == 4, what
    for name, a, b in zip("XHDY", got, want):
        a = a.cpu()
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous(), (what, name, a.shape, b.shape, a.dtype)
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), (what, name)
