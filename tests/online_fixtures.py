"""Shared by test_online_cpu.py and test_gpu_online.py: a seeded raw series with outages and the three sensors that hit
the std = 1 rules, helpers that push it step by step, and a copy of the arithmetic `data.zscore` and
`data.prepare_missing` had before the statistics moved into helpers of their own (what they must still return)."""
import functools

import torch

HOURS = [1, 2, 3]
Q = 3
NULL = 0.0
DEAD, SINGLE, CONSTANT, ONE_CHANNEL = 0, 1, 2, 5     # nodes with a hand-made pattern (N >= 6)


def history(tau):
    return tau * max(HOURS)


def total_steps(tau):
    """Origins up to history + 30 and up to history + L + tau + 1 (L = history), and their Q-step truths, lie inside."""
    return max(history(tau) + 30, 2 * history(tau) + tau + 1) + Q + 6


def origins(tau):
    """Every origin from history to history + L + tau + 1: every window position relative to the wrap of a ring of
    L = history rows occurs, and the ring has turned over at least once."""
    return range(history(tau), 2 * history(tau) + tau + 2)


@functools.lru_cache(maxsize=None)
def raw_series(C, N, tau=4, seed=0):
    """raw [C,N,total] float32 with outages written as 0 into all channels, and
      node DEAD         0 throughout
      node SINGLE       one valid entry in the training span (step 5), valid again after it
      node CONSTANT     the same value at every step (no spread)
      node ONE_CHANNEL  readings where only the LAST channel is missing (validity 0, the other channels keep theirs)."""
    from ms_gat_amd import data
    total = total_steps(tau)
    g = torch.Generator().manual_seed(1000 * C + N + 7 * tau + seed)
    raw = (60 + 20 * torch.randn(C, N, total, generator=g)).clamp_min(1.0)
    down = torch.rand(N, total, generator=g) < 0.12
    down[:6] = False
    raw[:, down] = NULL
    train_end = data.split_intervals(total, HOURS, Q, tau)[1]
    raw[:, DEAD] = NULL
    raw[:, SINGLE, :train_end] = NULL
    raw[:, SINGLE, 5] = 41.5
    raw[:, CONSTANT] = 37.0
    raw[C - 1, ONE_CHANNEL, history(tau) - 2: history(tau) + 3] = NULL
    raw[C - 1, ONE_CHANNEL, total - 9] = NULL
    return raw


def push_series(push, raw, start, stop, chunk=1):
    """push(raw[:, :, a:b] as [K,C,N]) for the steps start..stop-1, `chunk` at a time (the last may be shorter)."""
    for a in range(start, stop, chunk):
        b = min(a + chunk, stop)
        push(raw[:, :, a:b].permute(2, 0, 1).contiguous())


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- data.zscore and data.prepare_missing as they were: the refactored ones must return these bits ---------------------
def zscore_pinned(series, split):
    std, mean = torch.std_mean(series[..., :split], dim=-1, keepdim=True)
    return (series - mean) / std


def prepare_missing_pinned(raw, split, input_null_value, period):
    valid = ~(torch.isnan(raw) | (raw == input_null_value))
    x = torch.where(valid, raw, torch.zeros((), dtype=raw.dtype)).double()
    head, head_valid = x[..., :split], valid[..., :split]
    count = head_valid.sum(-1, keepdim=True)
    mean = head.sum(-1, keepdim=True) / count.clamp(min=1)
    dev2 = (torch.where(head_valid, head - mean, torch.zeros((), dtype=torch.float64)) ** 2).sum(-1, keepdim=True)
    std = (dev2 / (count - 1).clamp(min=1)).sqrt()
    std = torch.where((count < 2) | ~(std > 0), torch.ones_like(std), std)
    mean, std = mean.float(), std.float()
    std = torch.where(std > 0, std, torch.ones_like(std))
    nan = torch.full((), float("nan"), dtype=torch.float32)
    normed = torch.where(valid, (raw.float() - mean) / std, nan)
    slot = torch.arange(split) % period
    sums = torch.zeros((period, *raw.shape[:2]), dtype=torch.float64)
    counts = torch.zeros((period, *raw.shape[:2]), dtype=torch.float64)
    train = normed[..., :split].permute(2, 0, 1)
    train_valid = head_valid.permute(2, 0, 1)
    sums.index_add_(0, slot, torch.where(train_valid, train, torch.zeros((), dtype=torch.float32)).double())
    counts.index_add_(0, slot, train_valid.double())
    climatology = torch.where(counts > 0, sums / counts.clamp(min=1), torch.zeros((), dtype=torch.float64)).float()
    return normed, climatology
