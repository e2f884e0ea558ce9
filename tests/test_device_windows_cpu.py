"""CPU: `data.DeviceWindows` -- the loader that builds every batch on the device from a resident series -- run with
`device="cpu"`, where the same class gathers with torch indexing: the symbol, the reference-generated goldens, the order
/ epoch / shard / ragged-batch logic against the host DataLoader it replaces, and the unchanged defaults.
"""
import ctypes as C
import os
import re

import pytest
import torch
from torch.utils.data import DataLoader

from conftest import ROOT
from device_windows_fixtures import assert_batches_equal, host_loader, loader_golden, slices_golden


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


def test_window_gather_is_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    from ms_gat_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+msgat_window_gather\s*\(([^)]*)\)\s*;", code)
    assert decl, "msgat_window_gather is not declared in include/msgat_hip.h"
    n_args = len(decl.group(1).split(","))
    assert n_args == 17 and decl.group(1).strip().endswith("void* stream")
    assert "msgat_window_gather" in _lib.exported_symbols()
    assert len(_lib._PROTOTYPES["msgat_window_gather"][1]) == n_args
    assert hasattr(C.CDLL(_lib.LIB_PATH), "msgat_window_gather")
    assert "windows.hip" in build.SOURCES
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10
    # argument errors come back as status codes before anything is enqueued (no GPU needed)
    L = _lib.lib()
    assert L.msgat_window_gather(*[None] * 8, 1, 1, 1, 1, 100, 12, 12, 12, None) == -1
    p = [1] * 8      # never dereferenced: every call below is refused on its dimensions
    assert L.msgat_window_gather(*p, 1, 1, 1, 1, 23, 12, 12, 12, None) == -2      # T_total < history + q
    assert L.msgat_window_gather(*p, 0, 1, 1, 1, 100, 12, 12, 12, None) == -2
    assert L.msgat_window_gather(*p, 1, 1, 1, 1, 100, 10, 12, 12, None) == -3     # tau = 10
    assert L.msgat_window_gather(*p, 1, 1, 1, 1, 100, 12, 65, 12, None) == -3     # q = 65


def test_cpu_device_windows_reproduces_the_slices_golden():
    from ms_gat_amd import data
    args, idx, want = slices_golden()
    dw = data.DeviceWindows(*args, batch_size=len(range(*args[2])), device="cpu")
    assert len(dw) == 1 and len(dw.dataset) == args[2][1] - args[2][0]
    (x, h, d, y), = list(dw)
    assert_batches_equal((x[idx], h[idx], d[idx], y[idx]), (want["x"], want["h"], want["d"], want["y"]), "slices_small")


def test_cpu_device_windows_reproduces_the_loader_golden():
    from ms_gat_amd import data
    raw, hours, q, tau, bs, want = loader_golden()
    train, val, ev = data.make_loaders(raw, hours, q, tau, bs, device="cpu")
    assert all(isinstance(l, data.DeviceWindows) for l in (train, val, ev))
    assert train.series is val.series is ev.series and train.target is ev.target       # one upload for the three splits
    assert train.resident_bytes == 4 * raw.shape[2] * raw.shape[1] * (raw.shape[0] + 1)
    for split, loader in (("val", val), ("eval", ev)):
        batches = list(loader)
        assert_batches_equal(batches[0], [want[f"{split}_{k}"] for k in "xhdy"], split)
        assert_batches_equal(batches[-1], [want[f"{split}_last_{k}"] for k in "xhdy"], split + " last")
    ds = train.dataset                                        # the training loader shuffles: dataset order
    ordered = data.DeviceWindows(ds.inputs, ds.target, (ds.start, ds.stop), hours, q, tau, bs, shuffle=False, device="cpu")
    assert_batches_equal(next(iter(ordered)), [want[f"train_{k}"] for k in "xhdy"], "train")


def _series(n_origins, C_=2, N=3, tau=4, hours=(1, 3), q=3, seed=0):
    history = tau * max(hours)
    total = history + q + n_origins - 1
    g = torch.Generator().manual_seed(seed)
    inputs = torch.randn(C_, N, total, generator=g)
    inputs[0, 1, 5] = float("nan")
    return inputs, torch.randn(N, total, generator=g), (history, history + n_origins), list(hours), q, tau


# 14 origins in batches of 4: a ragged last batch of 2 on every path; 13: the last global batch holds 1 sample, ragged for
# one rank and, with two ranks, fewer samples than ranks -- dropped on both paths
@pytest.mark.parametrize("n_origins", [14, 13])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_cpu_device_windows_yields_the_batches_of_the_host_loader(n_origins, rank, world, shuffle):
    from ms_gat_amd import data
    args = _series(n_origins)
    dw = data.DeviceWindows(*args, batch_size=4, shuffle=shuffle, rank=rank, world=world, seed=5, device="cpu")
    host = host_loader(*args, 4, shuffle, rank, world, 5)
    assert dw.msgat_sharded == (world > 1) and isinstance(dw.batch_sampler, data.ShardedBatchSampler)
    sizes = [4, 4, 4, 2] if n_origins == 14 else ([4, 4, 4, 1] if world == 1 else [4, 4, 4])
    firsts = []
    for epoch in (0, 3):
        dw.batch_sampler.set_epoch(epoch)
        host.batch_sampler.set_epoch(epoch)
        assert len(dw) == len(host) == len(sizes)
        assert dw.batch_sampler.global_batch_sizes() == host.batch_sampler.global_batch_sizes() == sizes
        got, want = list(dw), list(host)
        assert len(got) == len(want) == len(sizes)
        for k, (a, b) in enumerate(zip(got, want)):
            assert_batches_equal(a, b, (epoch, k))
        firsts.append(got[0][3])
    assert torch.equal(firsts[0], firsts[1]) != shuffle       # set_epoch re-draws the order exactly when shuffling


def test_loaders_are_dataloaders_unless_a_device_is_named():
    from ms_gat_amd import data
    raw, hours, q, tau, bs, _ = loader_golden()
    host = data.make_loaders(raw, hours, q, tau, bs)
    assert all(type(l) is DataLoader for l in host)
    dev = data.make_loaders(raw, hours, q, tau, bs, device="cpu")
    assert all(type(l) is data.DeviceWindows for l in dev)
    for a, b in zip(host, dev):
        assert len(a) == len(b) and len(a.dataset) == len(b.dataset)
    for a, b in zip(host[1:], dev[1:]):                       # the two that do not shuffle
        assert_batches_equal(next(iter(b)), next(iter(a)))
    syn = data.SyntheticPEMS(5, 6, 1, [1, 2], batch_size=8, days=1)
    assert type(syn.training) is DataLoader
    syn = data.SyntheticPEMS(5, 6, 1, [1, 2], batch_size=8, days=1, device="cpu")
    assert type(syn.training) is data.DeviceWindows and type(syn.evaluation) is data.DeviceWindows


def test_window_gather_checks_its_arguments_before_any_launch():
    from ms_gat_amd import ops
    series, target, origins = torch.zeros(40, 2, 3), torch.zeros(3, 40), torch.tensor([30], dtype=torch.int64)
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series.double(), target, origins, [1, 2], 12, 12)
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series, target.double(), origins, [1, 2], 12, 12)
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series, target.to("meta"), origins, [1, 2], 12, 12)           # another device
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series, target, origins.to("meta"), [1, 2], 12, 12)
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series[:35].contiguous(), target[:, :35].contiguous(), origins, [1, 2], 12, 12)   # 35 < 24 + 12
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series, torch.zeros(4, 40), origins, [1, 2], 12, 12)          # shapes that do not fit
    with pytest.raises((ValueError, TypeError)):
        ops.window_gather(series, target, origins, [1, 2], 10, 12)                      # tau
    from ms_gat_amd._lib import MsgatError
    with pytest.raises(MsgatError):
        ops.window_gather(series, target, origins, [1, 2], 12, 12)                      # well-formed, but no CPU path
