"""Input side of the path: PEMS-style series -> (X, H, D, Y) batches, and a synthetic stand-in.

Reference: /root/reference/src/data_loader.py -- adjacency csv (:49-66, in `graph.py` here),
npz series `data` of shape [T_total, N, C] (:71), z-score over the training span (:79, :118-120),
60/20/20 split (:73-78), multi-period windows (:92-115).  On-disk formats are the reference's:
csv `from,to,cost` with a header line, npz with key `data`.

The reference ships no data files, so `SyntheticPEMS` generates a seeded series of the same
layout for benchmarks and tests.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml
from torch.utils.data import DataLoader, Dataset, Sampler

from .graph import sym_norm_adjacency, synthetic_adjacency


def load_adjacency_csv(path: str, n_nodes: int) -> torch.Tensor:
    """`from,to,cost` edge list (header skipped, cost ignored) -> D^-1/2 (A+I) D^-1/2 (data_loader.py:59-66)."""
    edges = []
    with open(path) as f:
        next(f, None)
        for line in f:
            if line.strip():
                s, d = line.split(",")[:2]
                edges.append((int(s), int(d)))
    return sym_norm_adjacency(n_nodes, edges)


def zscore(series: torch.Tensor, split: int) -> torch.Tensor:
    """Per (channel, node) z-score with statistics of the first `split` steps only (data_loader.py:118-120)."""
    mean, std = _zscore_stats(series, split)
    return (series - mean) / std


def _zscore_stats(series: torch.Tensor, split: int):
    """(mean, std) [..., 1] of the first `split` steps, as `zscore` applies them (unbiased std)."""
    std, mean = torch.std_mean(series[..., :split], dim=-1, keepdim=True)
    return mean, std


def missing_entries(series: torch.Tensor, input_null_value: float) -> torch.Tensor:
    """The entries of a series that are no measurements: NaN, or equal to `input_null_value` (what
    `engine.valid_entries` says for the truth, negated).  `input_null_value = nan` marks the NaN entries only."""
    return torch.isnan(series) | (series == input_null_value)


def prepare_missing(raw: torch.Tensor, split: int, input_null_value: float, period: int):
    """raw [C,N,T_total] with missing readings -> (normed [C,N,T_total], climatology [period,C,N]), both float32.

    `normed`: the z-score per (channel, node) with the statistics of the VALID entries among the first `split` steps
    (float64, unbiased std, rounded once), every missing entry stored as NaN.  A row with fewer than two valid training
    entries or without spread gets std 1 and as mean its single valid value, or 0.
    `climatology[s]`: the mean (float64, rounded once) of the valid normalised entries at the steps t < split with
    t % period == s; 0, the mean of a z-score, where there is none.  It is what the gather puts in a missing reading's
    place (`ops.window_gather_imputed`, `_windows_torch`)."""
    if raw.dim() != 3 or period < 1 or not 0 <= split <= raw.shape[-1]:
        raise ValueError(f"prepare_missing: raw {tuple(raw.shape)} must be [C,N,T_total], period = {period} >= 1 and "
                         f"split = {split} within the series")
    valid, mean, std = _missing_stats(raw, split, input_null_value)
    head_valid = valid[..., :split]
    nan = torch.full((), float("nan"), dtype=torch.float32)
    normed = torch.where(valid, (raw.float() - mean) / std, nan)
    slot = torch.arange(split) % period
    sums = torch.zeros((period, *raw.shape[:2]), dtype=torch.float64)
    counts = torch.zeros((period, *raw.shape[:2]), dtype=torch.float64)
    train = normed[..., :split].permute(2, 0, 1)                 # [split,C,N]
    train_valid = head_valid.permute(2, 0, 1)
    sums.index_add_(0, slot, torch.where(train_valid, train, torch.zeros((), dtype=torch.float32)).double())
    counts.index_add_(0, slot, train_valid.double())
    climatology = torch.where(counts > 0, sums / counts.clamp(min=1), torch.zeros((), dtype=torch.float64)).float()
    return normed, climatology


def _missing_stats(raw: torch.Tensor, split: int, input_null_value: float):
    """(valid [C,N,T_total] bool, mean [C,N,1], std [C,N,1], both float32): the statistics `prepare_missing` normalises
    with -- float64 over the valid entries of the first `split` steps, rounded once, with its rules for rows that have
    fewer than two valid entries or no spread."""
    valid = ~missing_entries(raw, input_null_value)
    x = torch.where(valid, raw, torch.zeros((), dtype=raw.dtype)).double()
    head, head_valid = x[..., :split], valid[..., :split]
    count = head_valid.sum(-1, keepdim=True)
    mean = head.sum(-1, keepdim=True) / count.clamp(min=1)
    dev2 = (torch.where(head_valid, head - mean, torch.zeros((), dtype=torch.float64)) ** 2).sum(-1, keepdim=True)
    std = (dev2 / (count - 1).clamp(min=1)).sqrt()
    std = torch.where((count < 2) | ~(std > 0), torch.ones_like(std), std)
    mean, std = mean.float(), std.float()
    std = torch.where(std > 0, std, torch.ones_like(std))        # a spread that rounds to 0 in float32
    return valid, mean, std


def split_intervals(total_steps: int, in_hours: Sequence[int], out_timesteps: int, tau: int):
    """Training / validation / evaluation [start, stop) of forecast origins (data_loader.py:69-78)."""
    history = tau * max(in_hours)
    length = total_steps - history - out_timesteps + 1
    a, b = int(0.6 * length), int(0.8 * length)
    return [(history, history + a), (history + a, history + b), (history + b, history + length)], history + a


class PeriodicWindows(Dataset):
    """Forecast origin t -> (X [R,C,N,tau], hour-of-day, day-of-week, Y [N,q])  (data_loader.py:92-115).

    Component r looks `hours[r]` hours back: X[r] = inputs[..., t - hours[r]*tau : t - hours[r]*tau + tau].
    The target is channel 0 of the raw (un-normalised) series.
    `climatology` [period,C,N] given (`prepare_missing`): a NaN of a window becomes the table's entry of its step,
    `climatology[step % period]`, and with `mask_channel` X is [R,C+1,N,tau], its last channel 1.0 where all C channels
    of the node at that step are observed, else 0.0.
    """

    def __init__(self, inputs: torch.Tensor, target: torch.Tensor, interval: Tuple[int, int],
                 hours: Sequence[int], out_timesteps: int, timesteps_per_hour: int,
                 climatology: torch.Tensor | None = None, mask_channel: bool = False):
        self.inputs, self.target = inputs, target
        self.start, self.stop = interval
        self.hours, self.q, self.tau = list(hours), out_timesteps, timesteps_per_hour
        self.climatology, self.mask_channel = climatology, bool(mask_channel) and climatology is not None

    def __len__(self) -> int:
        return self.stop - self.start

    def _window(self, s: int) -> torch.Tensor:
        x = self.inputs[..., s: s + self.tau]
        if self.climatology is None:
            return x
        missing = torch.isnan(x)
        slots = torch.arange(s, s + self.tau) % self.climatology.shape[0]
        x = torch.where(missing, self.climatology[slots].permute(1, 2, 0), x)
        if self.mask_channel:
            x = torch.cat([x, (~missing.any(0, keepdim=True)).to(x.dtype)])
        return x

    def __getitem__(self, i: int):
        t = i + self.start
        hour = t // self.tau
        x = torch.stack([self._window(t - h * self.tau) for h in self.hours])
        y = self.target[..., t: t + self.q]
        return x, torch.tensor(hour % 24), torch.tensor((hour // 24) % 7), y


class MSGATData:
    """Adjacency + the three loaders, as `DataLoaderForMSGAT` exposes them (data_loader.py:16-47).

    `meta` is the reference's `data/meta.yaml` entry (adj-file, data-file, num-nodes, num-channels,
    timesteps-per-hour) or a path to such a yaml plus `name`.
    `input_null_value`, `impute`, `mask_channel`: `make_loaders`' handling of missing input readings; `input_channels`
    is what the model's `in_channels` must be (`num_channels`, plus one with the validity channel).
    """

    def __init__(self, name: str, in_hours: List[int], out_timesteps: int, batch_size: int, num_workers: int = 0,
                 meta_file: str = "data/meta.yaml", meta: dict | None = None, device=None,
                 input_null_value: float | None = None, impute: str = "period", mask_channel: bool = True):
        if meta is None:
            with open(meta_file) as f:
                meta = yaml.safe_load(f)[name]
        self.num_nodes, self.num_channels = meta["num-nodes"], meta["num-channels"]
        self.input_channels = self.num_channels + int(input_null_value is not None and bool(mask_channel))
        self.timesteps_per_hour = meta["timesteps-per-hour"]
        self.in_hours, self.out_timesteps = list(in_hours), out_timesteps
        self.adj = load_adjacency_csv(meta["adj-file"], self.num_nodes)
        raw = torch.from_numpy(np.load(meta["data-file"])["data"]).float().transpose(0, -1)  # [C,N,T_total]
        self.training, self.validation, self.evaluation = make_loaders(
            raw, self.in_hours, out_timesteps, self.timesteps_per_hour, batch_size, num_workers, device=device,
            input_null_value=input_null_value, impute=impute, mask_channel=mask_channel)


class ShardedBatchSampler(Sampler):
    """This rank's samples of every GLOBAL batch, for one-process-per-GPU data parallelism.

    `nn.DataParallel` (main.py:52-55) loads a batch in one process and scatters it on dim 0.  Here all ranks
    walk the same sequence of global batches of `batch_size` samples -- the same per-epoch permutation, drawn
    from `seed + epoch` on every rank -- and each yields only its contiguous shard (`parallel.shard_bounds`), so
    a rank loads 1/world of the data and the shards partition the epoch.  A last global batch with fewer samples
    than ranks is dropped on every rank alike (an empty shard would leave a rank out of the gradient collective).
    `set_epoch(e)` re-seeds the permutation; `Engine.run_epoch` calls it."""

    def __init__(self, n: int, batch_size: int, shuffle: bool, rank: int, world: int, seed: int = 0):
        if not 0 <= rank < world or batch_size < 1:
            raise ValueError(f"bad shard: rank {rank} of {world}, batch {batch_size}")
        self.n, self.batch_size, self.shuffle, self.rank, self.world, self.seed = n, batch_size, shuffle, rank, world, seed
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _starts(self):
        return [b for b in range(0, self.n, self.batch_size) if min(self.batch_size, self.n - b) >= self.world]

    def __len__(self) -> int:
        return len(self._starts())

    def global_batch_sizes(self) -> List[int]:
        """Sample count of every global batch this sampler yields a shard of, in order (the engine weights a shard's
        loss by its share of the global batch)."""
        return [min(self.batch_size, self.n - b) for b in self._starts()]

    def __iter__(self):
        from .parallel import shard_bounds
        if self.shuffle:
            order = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + self.epoch)).tolist()
        else:
            order = list(range(self.n))
        for b in self._starts():
            size = min(self.batch_size, self.n - b)
            lo, hi = shard_bounds(size, self.rank, self.world)
            yield order[b + lo: b + hi]


def upload_series(inputs: torch.Tensor, target: torch.Tensor, device):
    """The two arrays `DeviceWindows` reads, as it keeps them on `device`: inputs [C,N,T_total] -> TIME-MAJOR
    [T_total,C,N] (a window is then tau rows read coalesced over the (channel, node) axis, and a block of the gather
    kernel writes one contiguous piece of X), target [N,T_total] as it is.  4 * T_total * N * (C + 1) bytes."""
    device = torch.device(device)
    if inputs.dim() != 3 or inputs.dtype != torch.float32 or target.dtype != torch.float32 \
            or tuple(target.shape) != (inputs.shape[1], inputs.shape[2]):
        raise ValueError(f"inputs {tuple(inputs.shape)} {inputs.dtype} must be float32 [C,N,T_total] and target "
                         f"{tuple(target.shape)} {target.dtype} float32 [N,T_total]")
    return inputs.to(device).permute(2, 0, 1).contiguous(), target.to(device).contiguous()


def _windows_torch(series_tm: torch.Tensor, target: torch.Tensor, origins: torch.Tensor, hours, tau: int, q: int,
                   climatology: torch.Tensor | None = None, mask_channel: bool = False):
    """`ops.window_gather` restated with torch indexing (bit-equal to collated `PeriodicWindows` items); serves
    `DeviceWindows(device="cpu")` and states what the kernel must give.  With `climatology` [period,C,N] it restates
    `ops.window_gather_imputed`: a NaN becomes the table's entry of its step, and `mask_channel` appends the validity
    channel (1.0 where all C channels of the node at that step are observed)."""
    back = torch.tensor([h * tau for h in hours], dtype=torch.int64, device=origins.device)
    rows = origins[:, None, None] - back[None, :, None] + torch.arange(tau, device=origins.device)     # [B,R,tau]
    x = series_tm[rows]                                                                                # [B,R,tau,C,N]
    if climatology is not None:
        missing = torch.isnan(x)
        x = torch.where(missing, climatology[rows % climatology.shape[0]], x)
        if mask_channel:
            x = torch.cat([x, (~missing.any(3, keepdim=True)).to(x.dtype)], dim=3)
    x = x.permute(0, 1, 3, 4, 2).contiguous()                                                          # [B,R,C,N,tau]
    y = target[:, origins[:, None] + torch.arange(q, device=origins.device)].permute(1, 0, 2).contiguous()
    hour = origins // tau
    return x, hour % 24, (hour // 24) % 7, y


@dataclasses.dataclass
class SeriesStats:
    """What training knew about the series and a reading that arrives later needs: the per-(channel, node) `mean` and
    `std` [C,N] the inputs were normalised with, the slot table `climatology` [period,C,N] a missing reading is imputed
    from (None for a series without missing readings), and the arguments they were made for.  `series_stats` builds it;
    `save` / `load` keep it beside a checkpoint (`Trainer.save` does not hold it)."""
    mean: torch.Tensor
    std: torch.Tensor
    climatology: Optional[torch.Tensor]
    hours: List[int]
    tau: int
    period: Optional[int]
    input_null_value: Optional[float]
    mask_channel: bool
    input_channels: int
    train_end: int

    @property
    def history(self) -> int:
        return self.tau * max(self.hours)

    def normalise(self, raw: torch.Tensor) -> torch.Tensor:
        """raw [C,N,T] -> what `make_loaders` put into its loaders for these steps: the z-score, with NaN at the missing
        readings of a series that has an `input_null_value`."""
        normed = (raw.float() - self.mean[..., None]) / self.std[..., None]
        if self.input_null_value is None:
            return normed
        nan = torch.full((), float("nan"), dtype=torch.float32)
        return torch.where(missing_entries(raw, self.input_null_value), nan, normed)

    def save(self, path) -> None:
        torch.save(dataclasses.asdict(self), path)

    @classmethod
    def load(cls, path) -> "SeriesStats":
        return cls(**torch.load(path, map_location="cpu"))


def series_stats(raw: torch.Tensor, in_hours, out_timesteps: int, tau: int, input_null_value: float | None = None,
                 impute: str = "period", mask_channel: bool = True) -> SeriesStats:
    """The statistics `make_loaders` uses internally for the same arguments, as an object that outlives training:
    `stats.normalise(raw)` has the bits of the series in its loaders and `stats.climatology` those of its table."""
    if impute not in ("period", "mean"):
        raise ValueError(f"impute = {impute!r} must be 'period' or 'mean'")
    if raw.dim() != 3:
        raise ValueError(f"series_stats: raw {tuple(raw.shape)} must be [C,N,T_total]")
    hours = [int(h) for h in in_hours]
    _, train_end = split_intervals(raw.size(-1), hours, out_timesteps, tau)
    table = period = None
    if input_null_value is None:
        mean, std = _zscore_stats(raw.float(), train_end)
    else:
        period = 7 * 24 * tau if impute == "period" else 1
        _, mean, std = _missing_stats(raw, train_end, input_null_value)
        table = prepare_missing(raw, train_end, input_null_value, period)[1]
        if impute == "mean":
            table.zero_()
    with_mask = input_null_value is not None and bool(mask_channel)
    return SeriesStats(mean=mean[..., 0].contiguous(), std=std[..., 0].contiguous(), climatology=table, hours=hours,
                       tau=int(tau), period=period,
                       input_null_value=None if input_null_value is None else float(input_null_value),
                       mask_channel=with_mask, input_channels=raw.shape[0] + int(with_mask), train_end=int(train_end))


def _ring_push_torch(raw: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, ring: torch.Tensor, clock: torch.Tensor,
                     null_value: float | None = None) -> None:
    """`ops.ring_push` restated with torch indexing; serves CPU tensors and states what the kernel must give.
    raw [K,C,N], the readings of K consecutive steps starting at step clock[0], go normalised into the rows
    (clock[0] + k) mod L of `ring` [L,C,N]; with `null_value` a reading that is NaN or equal to it is stored as the
    canonical NaN.  Then clock[0] += K and clock[1] = min(clock[1] + K, L)."""
    K, L = raw.shape[0], ring.shape[0]
    value = (raw - mean) / std
    if null_value is not None:
        value = torch.where(missing_entries(raw, null_value), torch.full_like(value, float("nan")), value)
    ring[(clock[0] + torch.arange(K, device=clock.device)) % L] = value       # `%` of tensors is the floor-mod
    clock[0] += K
    clock[1] = torch.clamp(clock[1] + K, max=L)


def _ring_windows_torch(ring: torch.Tensor, clock: torch.Tensor, hours, tau: int,
                        climatology: torch.Tensor | None = None, mask_channel: bool = False):
    """`ops.ring_windows` restated with torch indexing: `_windows_torch` for the one origin t = clock[0], the row of
    absolute step s read at s mod L of `ring` [L,C,N] and its slot of the table at s mod period.  (X [1,R,C(+1),N,tau],
    H [1], D [1])."""
    t = clock[:1]
    back = torch.tensor([h * tau for h in hours], dtype=torch.int64, device=clock.device)
    steps = t[:, None, None] - back[None, :, None] + torch.arange(tau, device=clock.device)            # [1,R,tau]
    x = ring[steps % ring.shape[0]]                                                                    # [1,R,tau,C,N]
    if climatology is not None:
        missing = torch.isnan(x)
        x = torch.where(missing, climatology[steps % climatology.shape[0]], x)
        if mask_channel:
            x = torch.cat([x, (~missing.any(3, keepdim=True)).to(x.dtype)], dim=3)
    x = x.permute(0, 1, 3, 4, 2).contiguous()
    hour = torch.div(t, tau, rounding_mode="floor")
    return x, hour % 24, torch.div(hour, 24, rounding_mode="floor") % 7


def _forecast_store_torch(pred: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor) -> None:
    """`ops.forecast_store` restated with torch indexing: pred [N,out] goes into row clock[0] mod P of `book` [P,N,out]
    and that row of `issued` [P] is stamped with clock[0]."""
    row = clock[0] % book.shape[0]                                            # `%` of tensors is the floor-mod
    book[row] = pred
    issued[row] = clock[0]


def _forecast_score_torch(raw: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor, t_out: int,
                          sums: torch.Tensor, node_sums: torch.Tensor, levels=(), point: int = 0,
                          null_value: float | None = None, mask_value: float = 0.0) -> None:
    """`ops.forecast_score` restated with torch ops; serves CPU tensors and states what the kernels settle: for k in order
    and every horizon h the forecast of origin clock[0] + k - h counts if `issued` carries its stamp (and the origin is
    >= 0), against the truth raw[k, 0]; every entry's terms are formed in fp32 as the kernel forms them and widened to
    float64.  A node's totals are added in the kernel's k-then-h order; the sums over the nodes are torch's (the kernel
    adds them in node order: tests/online_score_ref.py restates that bit for bit)."""
    P, n_levels = book.shape[0], len(levels)
    start = int(clock[0])
    stamps = issued.tolist()
    tau = torch.tensor([float(q) for q in levels], dtype=torch.float32, device=raw.device)
    tau_m1 = (tau.double() - 1.0).float()
    for k in range(raw.shape[0]):
        y = raw[k, 0]
        valid = ~torch.isnan(y)
        if null_value is not None:
            valid = valid & (y != null_value)
        for h in range(t_out):
            origin = start + k - h
            row = origin % P
            if origin < 0 or stamps[row] != origin or not bool(valid.any()):
                continue
            p = book[row].reshape(book.shape[1], max(n_levels, 1), t_out)[:, :, h]                      # [N, Q]
            e = p[:, point] - y
            zero = torch.zeros_like(y, dtype=torch.float64)
            ape = torch.where(y > mask_value, 100.0 * (e / y).abs().double(), zero)
            terms = [torch.ones_like(zero), e.abs().double(), ape, e.double() * e.double(), e.double()]
            if n_levels:
                u = y[:, None] - p
                rho = torch.maximum(tau * u, tau_m1 * u)
                terms += [(p[:, :-1] > p[:, 1:]).any(1).double(), (p[:, -1] - p[:, 0]).double(),
                          *(y[:, None] <= p).double().t(), *rho.double().t()]
            terms = torch.where(valid[None], torch.stack(terms), zero)                                   # [W, N]
            sums[h] += terms.sum(1)
            sums[t_out] += terms.sum(1)
            node_sums += terms[[0, 1, 4]].t()


class DeviceWindows:
    """A loader whose series lives on the device: every batch is built there from its forecast origins, by one launch
    of `ops.window_gather` -- no per-sample Python, no collate, no pinning, no host-to-device copy of the batch.

    Takes what a split of `make_loaders` takes (the normalised series [C,N,T_total], `raw[0]`, the interval of origins,
    hours, q, tau) and always walks `ShardedBatchSampler(len, batch_size, shuffle, rank, world, seed)`; it yields the
    batches `DataLoader(PeriodicWindows(...), batch_sampler=<that sampler>)` yields, on `device`.  The whole index order
    of an epoch goes to the device in ONE copy at `__iter__`; a batch's origins are a slice of it.  `Engine.run_epoch`
    finds `batch_sampler` (`set_epoch`, `global_batch_sizes`) and `msgat_sharded` as on a sharded DataLoader.
    `resident`: the pair `upload_series` returned, to share one upload among several splits.
    With `device="cpu"` the batches come from `_windows_torch`: the host logic is the same.
    `climatology` [period,C,N] given (`prepare_missing`; `inputs` then holds NaN at its missing readings): the batches
    come from `ops.window_gather_imputed`, with the validity channel if `mask_channel`; the table lives on the device
    too, `resident` is then the triple (series, target, table) and `resident_bytes` counts the table."""

    def __init__(self, inputs: torch.Tensor, target: torch.Tensor, interval: Tuple[int, int], hours: Sequence[int],
                 out_timesteps: int, timesteps_per_hour: int, batch_size: int, shuffle: bool = False, rank: int = 0,
                 world: int = 1, seed: int = 0, device="cuda", resident=None, climatology: torch.Tensor | None = None,
                 mask_channel: bool = False):
        self.dataset = PeriodicWindows(inputs, target, interval, hours, out_timesteps, timesteps_per_hour,
                                       climatology=climatology, mask_channel=mask_channel)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        history = timesteps_per_hour * max(hours)
        if not history <= interval[0] <= interval[1] <= inputs.shape[-1] - out_timesteps + 1:
            raise ValueError(f"origins {tuple(interval)} leave the series: they must lie in [{history}, "
                             f"{inputs.shape[-1] - out_timesteps}]")
        self.climatology, self.mask_channel = None, self.dataset.mask_channel
        if climatology is None:
            self.series, self.target = upload_series(inputs, target, self.device) if resident is None else resident
        else:
            if climatology.dim() != 3 or climatology.dtype != torch.float32 or climatology.shape[0] < 1 \
                    or tuple(climatology.shape[1:]) != tuple(inputs.shape[:2]):
                raise ValueError(f"climatology {tuple(climatology.shape)} {climatology.dtype} must be float32 "
                                 f"[period, {inputs.shape[0]}, {inputs.shape[1]}]")
            self.series, self.target, self.climatology = resident if resident is not None else (
                *upload_series(inputs, target, self.device), climatology.to(self.device).contiguous())
            if self.climatology.device != self.device or self.climatology.shape != climatology.shape:
                raise ValueError("resident arrays do not belong to this series and device")
        if self.series.device != self.device or tuple(self.series.shape) != (inputs.shape[2], *inputs.shape[:2]):
            raise ValueError("resident arrays do not belong to this series and device")
        self.resident_bytes = self.series.numel() * 4 + self.target.numel() * 4
        if self.climatology is not None:
            self.resident_bytes += self.climatology.numel() * 4
        self.batch_sampler = ShardedBatchSampler(len(self.dataset), batch_size, shuffle, rank, world, seed)
        self.msgat_sharded = world > 1
        self._offsets = None
        if self.device.type == "cuda":
            from . import ops
            self._offsets = ops.window_offsets(hours, timesteps_per_hour, self.device)

    def __len__(self) -> int:
        return len(self.batch_sampler)

    def __iter__(self):
        ds = self.dataset
        batches = list(self.batch_sampler)
        if not batches:
            return
        order = (torch.tensor([i for b in batches for i in b], dtype=torch.int64) + ds.start).to(self.device)
        at = 0
        for b in batches:
            origins = order[at: at + len(b)]
            at += len(b)
            if self.device.type != "cuda":
                yield _windows_torch(self.series, self.target, origins, ds.hours, ds.tau, ds.q,
                                     climatology=self.climatology, mask_channel=self.mask_channel)
                continue
            from . import ops
            if self.climatology is None:
                yield ops.window_gather(self.series, self.target, origins, ds.hours, ds.tau, ds.q, offsets=self._offsets)
            else:
                yield ops.window_gather_imputed(self.series, self.climatology, self.target, origins, ds.hours, ds.tau,
                                                ds.q, mask_channel=self.mask_channel, offsets=self._offsets)


def make_loaders(raw: torch.Tensor, in_hours, out_timesteps, tau, batch_size, num_workers=0, pin_memory=True,
                 rank: int | None = None, world: int | None = None, seed: int = 0, device=None,
                 input_null_value: float | None = None, impute: str = "period", mask_channel: bool = True):
    """raw [C,N,T_total] -> (training, validation, evaluation) loaders; only training shuffles (data_loader.py:80-89).

    `batch_size` is the GLOBAL batch (the reference's `-b`).  Under an initialised process group (or explicit
    `rank` / `world`) the loaders are sharded (`ShardedBatchSampler`, attribute `msgat_sharded`): every rank loads
    only its part of each global batch.
    `device` given: three `DeviceWindows` over ONE upload of the series to that device instead of DataLoaders.
    `input_null_value` given: the readings of `raw` that are NaN or equal to it are missing (`prepare_missing`): they
    stay out of the z-score's statistics, and in X each becomes the training span's mean of its slot of the week
    (`impute="period"`, period = 7 * 24 * tau) or the z-score mean 0 (`impute="mean"`); with `mask_channel` X gains a
    channel that is 1.0 where the node's reading is observed, so the model's `in_channels` is C + 1.  Y stays the raw
    target (`Trainer(null_value=...)` masks it).  Without `input_null_value` the other two options have no effect
    (an `impute` that is neither of the two is a ValueError all the same)."""
    import torch.distributed as dist
    if impute not in ("period", "mean"):
        raise ValueError(f"impute = {impute!r} must be 'period' or 'mean'")
    if world is None:
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    intervals, train_end = split_intervals(raw.size(-1), in_hours, out_timesteps, tau)
    if input_null_value is None:
        normed, missing = zscore(raw, split=train_end), {}
    else:
        normed, table = prepare_missing(raw, train_end, input_null_value, 7 * 24 * tau if impute == "period" else 1)
        if impute == "mean":
            table.zero_()
        missing = dict(climatology=table, mask_channel=bool(mask_channel))
    if device is not None:
        resident = upload_series(normed, raw[0], device)
        if missing:
            resident = (*resident, missing["climatology"].to(resident[0].device).contiguous())
        return [DeviceWindows(normed, raw[0], iv, in_hours, out_timesteps, tau, batch_size, shuffle=(i == 0), rank=rank,
                              world=world, seed=seed, device=resident[0].device, resident=resident, **missing)
                for i, iv in enumerate(intervals)]
    pin = pin_memory and torch.cuda.is_available()
    loaders = []
    for i, iv in enumerate(intervals):
        ds = PeriodicWindows(normed, raw[0], iv, in_hours, out_timesteps, tau, **missing)
        if world > 1:
            loader = DataLoader(ds, batch_sampler=ShardedBatchSampler(len(ds), batch_size, i == 0, rank, world, seed),
                                pin_memory=pin, num_workers=num_workers)
            loader.msgat_sharded = True
        else:
            loader = DataLoader(ds, batch_size, shuffle=(i == 0), pin_memory=pin, num_workers=num_workers)
        loaders.append(loader)
    return loaders


class SyntheticPEMS:
    """Seeded stand-in for a PEMS dataset: same tensors, shapes and loaders, no files.

    `missing` > 0: that share of the (node, step) readings, in runs of 1 to 2 tau - 1 steps, is written as 0 into all
    channels of `raw`, as a PEMS file stores a sensor that was down; `dead_sensors` nodes are 0 throughout.  Both come from
    a generator of their own (`seed + 2`): the series without them keeps its bits.  `input_null_value`, `impute`,
    `mask_channel` and `input_channels` as in `MSGATData`."""

    def __init__(self, n_nodes: int, n_edges: int, n_channels: int, in_hours: List[int], out_timesteps: int = 12,
                 batch_size: int = 32, timesteps_per_hour: int = 12, days: int = 14, seed: int = 0,
                 num_workers: int = 0, device=None, missing: float = 0.0, dead_sensors: int = 0,
                 input_null_value: float | None = None, impute: str = "period", mask_channel: bool = True):
        if not 0.0 <= missing < 1.0 or not 0 <= dead_sensors <= n_nodes:
            raise ValueError(f"missing = {missing} must lie in [0, 1) and dead_sensors = {dead_sensors} in [0, {n_nodes}]")
        self.num_nodes, self.num_channels, self.timesteps_per_hour = n_nodes, n_channels, timesteps_per_hour
        self.input_channels = n_channels + int(input_null_value is not None and bool(mask_channel))
        self.in_hours, self.out_timesteps = list(in_hours), out_timesteps
        self.adj = synthetic_adjacency(n_nodes, n_edges, seed)
        g = torch.Generator().manual_seed(seed + 1)
        total = days * 24 * timesteps_per_hour
        t = torch.arange(total, dtype=torch.float32)
        daily = torch.sin(2 * torch.pi * t / (24 * timesteps_per_hour))
        base = 200 + 80 * torch.rand(n_channels, n_nodes, 1, generator=g)
        raw = base * (1 + 0.4 * daily) + 15 * torch.randn(n_channels, n_nodes, total, generator=g)
        self.raw = raw.clamp_min(1.0)
        if missing > 0 or dead_sensors > 0:
            self.raw[:, self.outages(n_nodes, total, timesteps_per_hour, missing, dead_sensors, seed + 2)] = 0.0
        self.training, self.validation, self.evaluation = make_loaders(
            self.raw, self.in_hours, out_timesteps, timesteps_per_hour, batch_size, num_workers, device=device,
            input_null_value=input_null_value, impute=impute, mask_channel=mask_channel)

    @staticmethod
    def outages(n_nodes: int, total: int, tau: int, missing: float, dead_sensors: int, seed: int) -> torch.Tensor:
        """bool [n_nodes, total]: runs of 1 to 2 tau - 1 steps (tau on average) at seeded places, as many as make up
        the share `missing` if none overlapped, plus `dead_sensors` whole rows."""
        g = torch.Generator().manual_seed(seed)
        n_runs = round(missing * n_nodes * total / tau)
        node, start = torch.randint(n_nodes, (n_runs,), generator=g), torch.randint(total, (n_runs,), generator=g)
        stop = (start + torch.randint(1, 2 * tau, (n_runs,), generator=g)).clamp(max=total)
        edges = torch.zeros(n_nodes, total + 1, dtype=torch.int64)
        ones = torch.ones(n_runs, dtype=torch.int64)
        edges.index_put_((node, start), ones, accumulate=True)
        edges.index_put_((node, stop), -ones, accumulate=True)
        down = edges.cumsum(1)[:, :total] > 0
        down[torch.randperm(n_nodes, generator=g)[:dead_sensors]] = True
        return down
