"""The callers of the hot path: MS-GAT's blocks around `GACN`, with the reference's
`state_dict` layout so checkpoints interchange.

Reference: /root/reference/src/models/msgat.py (GACN :17, TACN :57, CACN :83, MEAM :103,
TPC :137, MSGAT :166, factories :220-229), attention.py (TemporalAttention :42,
ChannelAttention :72), embeddings.py (TimeEmbedding :12).  Only the graph branch runs in
the HIP library at first; SURVEY.md section 8 rows f-1 and f-2 then pulled in every pass over the
[B,C,N,T] activations of a MEAM block: the LayerNorm over T (`LayerNormT`), the temporal and channel
branches (`ops.channel_pool / node_pool / mix / time_mix`) and the residual tail.  What stays in
PyTorch is tiny: the [B,T,T] / [B,C,C] attention matrices and their softmax.

Parameter names and shapes are the reference's (`tpcs.{r}.tgacns.{l}.gacn.gatt.Wg`, ...):
`tests/test_model_cpu.py` checks every key and shape against a reference checkpoint.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import torch
from torch import nn

from . import ops, stacked
from .attention import GACN


class LayerNormT(nn.LayerNorm):
    """`nn.LayerNorm([n_timesteps])` (msgat.py:114, :152) with the reference's `weight` / `bias` keys,
    evaluated by the library's one-pass kernel (`ops.layer_norm_t`): PyTorch's LayerNorm kernels spend
    a thread group per 12-element row and were 46% of the training step (profiles/r01/full_model_*)."""

    def __init__(self, n_timesteps: int, eps: float = 1e-5):
        super().__init__([n_timesteps], eps=eps)

    def forward(self, signals: torch.Tensor) -> torch.Tensor:
        return ops.layer_norm_t(signals, self.weight, self.bias, self.eps)


class TemporalAttention(nn.Module):
    """[T,T] attention from rank-10 node projections (attention.py:58-66).  signals [B,C,N,T].

    The two passes over the activation run in the library: the channel-weighted sum (`ops.channel_pool`,
    the hot path's q kernel) and the product with the [T,T] matrix (`ops.time_mix`); the rank-10
    projections and the softmax over [B,T,T] are tiny and stay in PyTorch."""

    rank = 10

    def __init__(self, n_channels: int, n_nodes: int):
        super().__init__()
        self.n_channels, self.n_nodes = n_channels, n_nodes
        self.Wt1 = nn.Parameter(torch.empty(self.rank, n_nodes))
        self.Wt2 = nn.Parameter(torch.empty(self.rank, n_nodes))
        self.alpha = nn.Parameter(torch.empty(n_channels))

    def attention(self, signals: torch.Tensor, pooled: torch.Tensor = None) -> torch.Tensor:
        """-> att [B,T,T], rows = output step.  `pooled` = sum_c alpha_c signals_c [B,N,T] when the caller has
        it already (MEAM computes it in its merged channel-mixing pass)."""
        if pooled is None:
            pooled = ops.channel_pool(signals, self.alpha)
        per_t = pooled.transpose(1, 2)                                   # [B,T,N]
        left = per_t @ self.Wt1.t()                                      # [B,T,10]
        right = per_t @ self.Wt2.t()                                     # [B,T,10]
        return torch.softmax(left @ right.transpose(1, 2), dim=-1)

    def forward(self, signals: torch.Tensor) -> torch.Tensor:
        # out[..,t] = sum_i att[t,i] x[..,i]
        return ops.time_mix(signals, self.attention(signals).unsqueeze(1))

    def extra_repr(self) -> str:
        return f"n_channels={self.n_channels}, n_nodes={self.n_nodes}"


class ChannelAttention(nn.Module):
    """[C,C] attention from node-weighted signals (attention.py:88-94).  signals [B,C,N,T]."""

    def __init__(self, n_nodes: int, n_timesteps: int):
        super().__init__()
        self.n_nodes, self.n_timesteps = n_nodes, n_timesteps
        self.Wc = nn.Parameter(torch.empty(n_timesteps, n_timesteps))
        self.alpha = nn.Parameter(torch.empty(n_nodes))

    def attention(self, signals: torch.Tensor) -> torch.Tensor:
        """-> att [B,C,C]."""
        pooled = ops.node_pool(signals, self.alpha)                      # [B,C,T]: node-weighted sum
        return torch.softmax(pooled @ self.Wc @ pooled.transpose(1, 2), dim=-1)

    def forward(self, signals: torch.Tensor) -> torch.Tensor:
        return ops.mix(signals, self.attention(signals))                 # per-sample [C,C] channel matrix

    def extra_repr(self) -> str:
        return f"n_nodes={self.n_nodes}, n_timesteps={self.n_timesteps}"


class TrimRight(nn.Module):
    """Drops the last `n` steps of the time axis: makes a padded dilated conv causal (msgat.py:34-54)."""

    def __init__(self, n: int):
        super().__init__()
        self.n = n

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x[..., : x.size(-1) - self.n]

    def extra_repr(self) -> str:
        return f"n={self.n}"


def _shift_down(att: torch.Tensor, d: int) -> torch.Tensor:
    """rows t >= d of the result are rows t - d of `att` ([..,T,T]); rows < d are zero."""
    T = att.size(-2)
    if d >= T:
        return torch.zeros_like(att)
    return torch.nn.functional.pad(att[..., : T - d, :], (0, 0, d, 0))


class TACN(nn.Module):
    """Temporal attention, then a stack of causal dilated [1,2] convolutions (msgat.py:57-80).

    `seq` keeps the reference's layout (seq.0 attention, seq.1/3/.. Conv2d weights, seq.2/4/.. trims) so
    checkpoints interchange; the forward does not run the Conv2d modules.  A padded, right-trimmed
    [1,2] convolution with dilation d is out[t] = W_0 in[t-d] + W_1 in[t]; with in = attention(x) that is
    sum_k (W_k x) applied along time with A_1 = att, A_0 = att shifted down by d.  So each layer is one
    channel-mixing pass (C -> 2 Co) and one `ops.time_mix` pass; the attention product is never stored."""

    def __init__(self, in_channels: int, out_channels: int, n_nodes: int, dilations: Sequence[int]):
        super().__init__()
        self.in_channels, self.out_channels, self.n_nodes, self.dilations = (
            in_channels, out_channels, n_nodes, list(dilations))
        layers: List[nn.Module] = [TemporalAttention(in_channels, n_nodes)]   # seq.0
        width = in_channels
        for d in self.dilations:                                              # seq.1, seq.3, ... hold weights
            layers.append(nn.Conv2d(width, out_channels, kernel_size=(1, 2), padding=(0, d), dilation=(1, d)))
            layers.append(TrimRight(d))
            width = out_channels
        self.seq = nn.Sequential(*layers)

    def stacked_taps(self, layer: int) -> torch.Tensor:
        """[2*Co, Ci]: the two taps of convolution `layer` stacked on the output axis (tap 0 acts on in[t-d])."""
        w = self.seq[1 + 2 * layer].weight
        return w.flatten(1, 2).permute(2, 0, 1).reshape(2 * w.shape[0], w.shape[1])   # [tap 0 rows; tap 1 rows], one copy

    def forward(self, signals: torch.Tensor) -> torch.Tensor:
        if not self.dilations:
            return self.seq[0](signals)
        mixed = ops.mix(signals, self.stacked_taps(0).unsqueeze(0))
        return self.finish(mixed, ops.channel_pool(signals, self.seq[0].alpha))

    def first_taps(self, pooled: torch.Tensor) -> torch.Tensor:
        """[B,2,T,T] taps of the first convolution -- (temporal attention shifted down by its dilation, temporal
        attention) -- from the alpha-weighted channel sums `pooled` [B,N,T]: one launch in the library."""
        ta = self.seq[0]
        if 2 * pooled.shape[-1] * ta.rank > 256:          # beyond the fused kernel's lane budget (T = 16): eager ops
            att = ta.attention(None, pooled=pooled)
            return torch.stack([_shift_down(att, self.dilations[0]), att], dim=1)
        return ops.temporal_attention_taps(pooled, ta.Wt1, ta.Wt2, self.dilations[0])

    def finish(self, mixed: torch.Tensor, pooled: torch.Tensor) -> torch.Tensor:
        """The stack from the channel-mixed input of its first convolution (`mixed` = stacked_taps(0) applied to
        the signals, [B,2Co,N,T]) and the pooled signals of the temporal attention (`pooled` [B,N,T])."""
        T = mixed.size(-1)
        h = None
        for i, d in enumerate(self.dilations):
            conv = self.seq[1 + 2 * i]
            if i == 0:
                taps = self.first_taps(pooled)                                                # [B,2,T,T]
            elif ops.causal_conv_fused(h.shape[1], conv.out_channels):
                # constant shift taps: channel mixing, the [B,2Co,N,T] intermediate and the time mixing are one pass
                h = ops.causal_conv(h, self.stacked_taps(i).unsqueeze(0), conv.bias, d)
                continue
            else:
                taps = ops.causal_shift_taps(T, d, mixed.device)                              # [1,2,T,T], cached constant
                mixed = ops.mix(h, self.stacked_taps(i).unsqueeze(0))
            h = ops.time_mix(mixed, taps, conv.bias)
        return h


class CACN(nn.Module):
    """Channel attention, then a 1x1 convolution (msgat.py:83-100): one pass with the per-sample
    matrix `conv.weight @ att_b`."""

    def __init__(self, in_channels: int, out_channels: int, n_nodes: int, n_timesteps: int):
        super().__init__()
        self.in_channels, self.out_channels, self.n_nodes, self.n_timesteps = (
            in_channels, out_channels, n_nodes, n_timesteps)
        self.seq = nn.Sequential(ChannelAttention(n_nodes, n_timesteps), nn.Conv2d(in_channels, out_channels, 1))

    def channel_matrix(self, signals: torch.Tensor, pooled: torch.Tensor = None) -> torch.Tensor:
        """[B,Co,C] = conv.weight @ channel attention: node pooling in one pass (or `pooled` [B,C,T], when the caller has
        it already: MEAM takes it out of its LayerNorm pass), the rest in one launch -- or, beyond the LDS budget of that
        launch's backward (from 115 channels at T = 12), in batched torch ops: `ops.channel_matrix` decides from the shapes."""
        ca, conv = self.seq[0], self.seq[1]
        if pooled is None:
            pooled = ops.node_pool(signals, ca.alpha)
        return ops.channel_matrix(pooled, ca.Wc, conv.weight.flatten(1))

    def forward(self, signals: torch.Tensor, pooled: torch.Tensor = None) -> torch.Tensor:
        return ops.mix(signals, self.channel_matrix(signals, pooled), self.seq[1].bias)


class MEAM(nn.Module):
    """LayerNorm -> {channel, temporal, graph} branches -> concat + 1x1 residual -> ReLU (msgat.py:103-134).

    The graph branch is the hot path: `self.gacn(normed, adjacency)` (msgat.py:127)."""

    def __init__(self, in_channels: int, out_channels: int, n_nodes: int, n_timesteps: int,
                 dilations: Sequence[int]):
        if out_channels % 3:
            raise ValueError("out_channels must be divisible by the 3 branches")
        super().__init__()
        self.in_channels, self.out_channels, self.n_nodes, self.n_timesteps, self.dilations = (
            in_channels, out_channels, n_nodes, n_timesteps, list(dilations))
        branch = out_channels // 3
        self.ln = LayerNormT(n_timesteps)
        self.res = nn.Conv2d(in_channels, out_channels, kernel_size=1)
        self.cacn = CACN(in_channels, branch, n_nodes=n_nodes, n_timesteps=n_timesteps)
        self.tacn = TACN(in_channels, branch, n_nodes=n_nodes, dilations=dilations)
        self.gacn = GACN(in_channels, branch, n_timesteps=n_timesteps)

    def forward(self, signals: torch.Tensor, adjacency, relu_input: bool = False, premasked: bool = False) -> torch.Tensor:
        """`relu_input` / `premasked` are for a caller that chains blocks itself (TPC): `relu_input` says `signals` is a
        ReLU output whose backward mask this block's LayerNorm applies; `premasked` says the consumer of THIS block's
        output will do the same for it, so the block skips its own mask pass.  Defaults: plain autograd semantics."""
        # (normed, signals): the residual convolution below reads the block input again (msgat.py:130); routed
        # through the LayerNorm op, its gradient is added inside the LayerNorm-backward kernel
        # ... and CACN pools the normalised input over the nodes (attention.py:89): the pooled signal comes out of the
        # LayerNorm pass, its gradients go back inside the LayerNorm-backward kernel (ops.layer_norm_pool_tee)
        normed, signals, pooled_c = ops.layer_norm_pool_tee(signals, self.ln.weight, self.ln.bias, self.ln.eps, relu_input,
                                                            self.cacn.seq[0].alpha)
        res_w = self.res.weight.flatten(1).unsqueeze(0)
        if self.in_channels <= self.out_channels // 3 or not self.dilations:
            # few input channels (the first block of a component): the graph branch aggregates before it
            # projects, nothing to merge -- branch by branch
            branches = [self.cacn(normed, pooled_c), self.tacn(normed), self.gacn(normed, adjacency)]
        else:
            branches = self._merged_branches(normed, adjacency, pooled_c)
        # relu(cat(branches) + res(signals)): the 1x1 residual convolution reads the three branch tensors as
        # its add operand (no concatenation) and applies the ReLU in its store epilogue
        return ops.mix_multi([signals], res_w, self.res.bias, adds=branches, relu=True, relu_grad_premasked=premasked)[0]

    def _merged_branches(self, normed: torch.Tensor, adjacency, pooled_c: torch.Tensor = None):
        """All channel mixings of the normalised input in ONE pass: CACN's per-sample
        matrix `conv @ att_b` (msgat.py:93-94), the two taps of TACN's first convolution (msgat.py:66-74), GACN's
        projection W (msgat.py:27, applied before the aggregation as C > out/3) and the two alpha-weighted channel
        poolings (attention.py:33 and :59) are rows of one [B, 4*Cb + 2, C] matrix.  The backward is then ONE
        transposed pass producing the gradient at the LayerNorm output, instead of five passes plus four adds."""
        B, C = normed.shape[:2]
        cb = self.out_channels // 3
        ca, ta, gatt = self.cacn.seq[0], self.tacn.seq[0], self.gacn.gatt
        conv_c = self.cacn.seq[1]
        rows = torch.cat([
            self.cacn.channel_matrix(normed, pooled_c),                          # [B,cb,C]   from the pooled signal
            self.tacn.stacked_taps(0).unsqueeze(0).expand(B, -1, -1),            # [B,2cb,C]
            self.gacn.W.unsqueeze(0).expand(B, -1, -1),                          # [B,cb,C]
            gatt.alpha.view(1, 1, C).expand(B, -1, -1),                          # [B,1,C]    q of the graph attention
            ta.alpha.view(1, 1, C).expand(B, -1, -1)], dim=1)                    # [B,1,C]    pooled signal of the temporal attention
        bias = torch.cat([conv_c.bias, conv_c.bias.new_zeros(3 * cb + 2)])
        cacn, mixed, u, q, pooled_t = ops.mix_multi([normed], rows, bias, out_channels=[cb, 2 * cb, cb, 1, 1])
        tacn = self.tacn.finish(mixed, pooled_t.flatten(1, 2))
        gacn = ops.attention_core(u, q.flatten(1, 2), gatt.Wg.unsqueeze(0), adjacency)
        return [cacn, tacn, gacn]


class TPC(nn.Module):
    """One component: a stack of MEAMs, LayerNorm, and a [1,C] convolution mapping T_in -> T_out (msgat.py:137-163)."""

    def __init__(self, channels: Sequence[int], n_nodes: int, in_timesteps: int, out_timesteps: int,
                 dilations: Sequence[Sequence[int]]):
        super().__init__()
        self.channels, self.n_nodes, self.in_timesteps, self.out_timesteps, self.dilations = (
            list(channels), n_nodes, in_timesteps, out_timesteps, [list(d) for d in dilations])
        self.tgacns = nn.ModuleList(
            MEAM(channels[i], channels[i + 1], n_nodes=n_nodes, n_timesteps=in_timesteps, dilations=d)
            for i, d in enumerate(dilations))
        self.ln = LayerNormT(in_timesteps)
        self.fc = nn.Conv2d(in_timesteps, out_timesteps, kernel_size=(1, channels[-1]))

    def forward(self, signals: torch.Tensor, adjacency) -> torch.Tensor:
        # every block's output is a ReLU output consumed by exactly one LayerNorm (the next block's, or self.ln): that
        # LayerNorm's backward kernel applies the ReLU mask, the blocks skip their own mask pass
        # (only among this package's own modules: a swapped-in block or LayerNorm gets plain autograd semantics)
        own = isinstance(self.ln, LayerNormT) and all(isinstance(b, MEAM) for b in self.tgacns)
        for i, block in enumerate(self.tgacns):
            signals = block(signals, adjacency, relu_input=i > 0, premasked=True) if own else block(signals, adjacency)
        if own:
            # LayerNorm, then fc over the transposed activation, squeezed and transposed back (msgat.py:158-160); backward
            # is one pass for the head's input gradient and the LayerNorm together
            return ops.ln_head(signals, self.ln.weight, self.ln.bias, self.ln.eps, self.fc.weight, self.fc.bias,
                               relu_input=len(self.tgacns) > 0)                    # [B,N,T_out]
        normed = self.ln(signals)
        return ops.head(normed, self.fc.weight, self.fc.bias)                      # [B,N,T_out]


class TimeEmbedding(nn.Module):
    """Hour-of-day + day-of-week gate [B,R,N,T_out] (embeddings.py:12-39)."""

    def __init__(self, n_components: int, n_nodes: int, n_timesteps: int):
        super().__init__()
        self.n_components, self.n_nodes, self.n_timesteps = n_components, n_nodes, n_timesteps
        width = n_components * n_nodes * n_timesteps
        self.d_ebd = nn.Embedding(7, width)
        self.h_ebd = nn.Embedding(24, width)

    def forward(self, H: torch.Tensor, D: torch.Tensor) -> torch.Tensor:
        gate = self.h_ebd(H) + self.d_ebd(D)
        return gate.view(-1, self.n_components, self.n_nodes, self.n_timesteps)


class EdgeTimeEmbedding(nn.Module):
    """Hour-of-day + day-of-week weights on the stored edges of one sparse pattern: the idiom of `TimeEmbedding`
    (embeddings.py:30-36) applied to the graph, `w[b,e] = weight[e] + h_ebd(H[b])[e] + d_ebd(D[b])[e]`.

    `crow` [N+1], `col` [nnz]: the CSR pattern (buffers); `init` [nnz]: the static weights the parameter `weight` starts
    from.  Both tables start at zero, so a fresh module is the static graph.  `forward(H, D)` is the batched CSR adjacency
    [B,N,N] that every op and module accepts (`ops.edge_adjacency` on `weights(H, D)`); the three parameters get dense
    gradients from one launch (`ops.edge_time_weights`)."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, init: torch.Tensor, n_hours: int = 24, n_days: int = 7):
        super().__init__()
        if init.dim() != 1 or col.shape != init.shape or crow.dim() != 1:
            raise ValueError(f"EdgeTimeEmbedding: crow {tuple(crow.shape)}, col {tuple(col.shape)} and init {tuple(init.shape)} "
                             "must be [N+1], [nnz] and [nnz]")
        self.register_buffer("crow", crow.detach().clone())
        self.register_buffer("col", col.detach().clone())
        self.weight = nn.Parameter(init.detach().clone().float())
        self.h_ebd = nn.Embedding(n_hours, init.numel())
        self.d_ebd = nn.Embedding(n_days, init.numel())
        with torch.no_grad():
            self.h_ebd.weight.zero_()
            self.d_ebd.weight.zero_()

    def weights(self, H: torch.Tensor, D: torch.Tensor) -> torch.Tensor:
        """[B,nnz] in the order of (crow, col)."""
        return ops.edge_time_weights(self.weight, self.h_ebd.weight, self.d_ebd.weight, H, D)

    def forward(self, H: torch.Tensor, D: torch.Tensor) -> torch.Tensor:
        return ops.edge_adjacency(self.crow, self.col, self.weights(H, D))


class EdgeSignalWeights(nn.Module):
    """Signal-dependent weights on the stored edges of one sparse pattern, the edge strength of the dynamic-graph traffic
    models as a rank-`rank` bilinear form of the readings at the edge's two ends: with `ab = proj(f)` [B,N,2*rank],
    `w[b,e] = weight[e] + sum_k ab[b,row(e),k] * ab[b,col(e),rank+k]`.

    `crow` [N+1], `col` [nnz]: the CSR pattern (buffers); `init` [nnz]: the static weights the parameter `weight` starts
    from; `f` [B,N,in_features]: the node features of each sample.  The rows `rank:` of `proj.weight` (the column side) start
    at zero, so a fresh module is the static graph; their gradient is not zero, so training moves -- the column side at the
    first step, the row side from then on.  `forward(f)` is the batched CSR adjacency [B,N,N] that every op and module
    accepts (`ops.edge_adjacency` on `weights(f)`); the projection is one torch matmul, the edge work one launch each way
    (`ops.edge_signal_weights`)."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, init: torch.Tensor, in_features: int, rank: int = 8):
        super().__init__()
        if init.dim() != 1 or col.shape != init.shape or crow.dim() != 1:
            raise ValueError(f"EdgeSignalWeights: crow {tuple(crow.shape)}, col {tuple(col.shape)} and init {tuple(init.shape)} "
                             "must be [N+1], [nnz] and [nnz]")
        _check_edge_rank(rank)
        self.rank = rank
        self.register_buffer("crow", crow.detach().clone())
        self.register_buffer("col", col.detach().clone())
        self.weight = nn.Parameter(init.detach().clone().float())
        self.proj = nn.Linear(in_features, 2 * rank, bias=False)
        with torch.no_grad():
            self.proj.weight[rank:].zero_()

    def weights(self, f: torch.Tensor) -> torch.Tensor:
        """[B,nnz] in the order of (crow, col)."""
        if f.dim() != 3 or f.shape[1] != self.crow.numel() - 1 or f.shape[2] != self.proj.in_features:
            raise ValueError(f"EdgeSignalWeights: f {tuple(f.shape)} must be [B, {self.crow.numel() - 1}, {self.proj.in_features}]")
        return ops.edge_signal_weights(self.weight, self.proj(f), self.crow, self.col)

    def forward(self, f: torch.Tensor) -> torch.Tensor:
        return ops.edge_adjacency(self.crow, self.col, self.weights(f))


def _check_edge_dropout(p) -> float:
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0):
        raise ValueError(f"edge_dropout must be a number in [0, 1), got {p!r}")
    return float(p)


def _read_edge_dropout_state(state: torch.Tensor) -> Dict[str, int]:
    seed, step = (int(v) for v in state.tolist())
    return {"seed": seed, "step": step}


def _write_edge_dropout_state(state: torch.Tensor, value) -> None:
    """In place: captured steps keep reading the same two words."""
    with torch.no_grad():
        state.copy_(torch.tensor([int(value["seed"]), int(value["step"])], dtype=torch.int64))


class EdgeDropout(nn.Module):
    """Dropout on the stored edges of a sparse pattern for callers of `GraphAttention`, `GACN` and `StackedGACN`:
    `forward(weights, samples=None)` takes `weights` [nnz] (shared by `samples` samples) or [V,nnz] in the order of
    (crow, col) and, in training mode, returns the [V,nnz] weights with each edge of each sample dropped with probability
    `p` and the kept ones multiplied by `1 / (1 - p)` -- ready for `ops.edge_adjacency(crow, col, ·)`; in eval mode it
    returns `weights` unchanged.  `exempt` (bool or uint8 [nnz]): edges that are never dropped or scaled, a stored diagonal
    for instance.  `sample_offset`: the index of this process's first sample in the global batch (`ops.edge_dropout`).

    The stream {seed, step} is a NON-persistent buffer (`edge_drop_state`, int64 [2]): it moves with the module, is copied
    by `copy.deepcopy`, advances on the device by one per training forward -- inside a captured step too -- and adds no
    `state_dict` key; `state()` / `set_state()` snapshot and restore it."""

    def __init__(self, p: float, seed: int = 0, exempt: Optional[torch.Tensor] = None):
        super().__init__()
        self.p = _check_edge_dropout(p)
        self.sample_offset = 0
        self.register_buffer("edge_drop_state", ops.edge_dropout_state(seed, "cpu"), persistent=False)
        self.register_buffer("edge_drop_exempt", None if exempt is None else exempt.detach().to(torch.uint8).clone(),
                             persistent=False)

    def forward(self, weights: torch.Tensor, samples: Optional[int] = None) -> torch.Tensor:
        if not self.training:
            return weights
        return ops.edge_dropout(weights, self.p, self.edge_drop_state, sample_offset=self.sample_offset,
                                exempt=self.edge_drop_exempt, samples=samples)

    def state(self) -> Dict[str, int]:
        """{"seed", "step"}: reads the two words back from the device."""
        return _read_edge_dropout_state(self.edge_drop_state)

    def set_state(self, state) -> None:
        _write_edge_dropout_state(self.edge_drop_state, state)

    def extra_repr(self) -> str:
        return f"p={self.p}"


def _check_missing_edges(mode, T: int):
    if mode is not None:
        ops.edge_validity_table(mode, T)                   # raises on anything but "scale", "drop" or an int in 1..T
    return mode


def _self_loops(crow: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """uint8 [nnz]: 1 at the stored diagonal of the CSR pattern (crow, col)."""
    rows = torch.repeat_interleave(torch.arange(crow.numel() - 1, device=crow.device), crow[1:] - crow[:-1])
    return (rows == col).to(torch.uint8)


class EdgeValidity(nn.Module):
    """Validity-gated edges of a sparse pattern for callers of `GraphAttention`, `GACN` and `StackedGACN`:
    `forward(weights, validity)` takes `weights` [nnz] or [V,nnz] in the order of (crow, col) and the validity windows
    `validity` [V,N,T] of the samples (1 = measured, 0 = imputed) and returns the [V,nnz] weights with the edges OUT OF
    each node multiplied by `ops.edge_validity_table(mode, T)[its number of valid readings]` -- ready for
    `ops.edge_adjacency(crow, col, ·)`.  `mode`: "scale" (c / T), "drop" (any missing reading silences the node) or an int m
    (at least m readings keep the edges).  `keep_self=True` leaves the stored diagonal alone.  It is a function of the
    input, not noise: training and eval mode compute the same.  No parameter, no `state_dict` key (`ops.edge_validity`)."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, mode="scale", keep_self: bool = True):
        super().__init__()
        if crow.dim() != 1 or col.dim() != 1 or crow.numel() < 1:
            raise ValueError(f"EdgeValidity: crow {tuple(crow.shape)} and col {tuple(col.shape)} must be [N+1] and [nnz]")
        if not (mode in ("scale", "drop") or (isinstance(mode, int) and not isinstance(mode, bool) and mode >= 1)):
            raise ValueError(f'EdgeValidity: mode must be "scale", "drop" or a positive int, got {mode!r}')
        self.mode = mode
        self.register_buffer("crow", crow.detach().clone(), persistent=False)
        self.register_buffer("col", col.detach().clone(), persistent=False)
        self.register_buffer("exempt", _self_loops(self.crow, self.col) if keep_self else None, persistent=False)

    def forward(self, weights: torch.Tensor, validity: torch.Tensor) -> torch.Tensor:
        return ops.edge_validity(weights, validity, self.crow, self.col, mode=self.mode, exempt=self.exempt)

    def extra_repr(self) -> str:
        return f"mode={self.mode!r}, keep_self={self.exempt is not None}"


def _check_edge_rank(rank) -> None:
    if isinstance(rank, bool) or not isinstance(rank, int) or rank < 4 or rank > 32 or rank % 4:
        raise ValueError(f"the edge rank must be one of 4, 8, ..., 32 (rows are read as 16-byte pieces), got {rank!r}")


class MSGAT(nn.Module):
    """X [B,R,C,N,T], H [B], D [B] -> [B,N,T_out]  (msgat.py:166-217).

    `use_te=False` uses the learned static gate `W [R,N,T_out]` that the reference declares
    (msgat.py:189) but cannot reach (its forward reads `self.te` unconditionally, msgat.py:203).

    `learn_edge_weights=True` learns one weight per existing edge of the road graph: the pattern of `adj != 0` is kept as
    the index buffers `edge_crow` / `edge_col` and the weights, initialised from `adj`, as the parameter `edge_weight`
    [nnz].  The forward hands every block the sparse CSR adjacency built from them, whose gradient is computed at the
    edges only (msgat_edge_weight_grad).  `adj` stays as the frozen dense parameter of the reference's layout.

    `learn_edge_weights="time"` lets those weights depend on the sample's hour of day and day of week (`EdgeTimeEmbedding`'s
    arithmetic): `edge_crow`, `edge_col` and `edge_weight` as above -- `edge_weight` is the base -- plus the tables
    `edge_h_ebd.weight` [24,nnz] and `edge_d_ebd.weight` [7,nnz], zero at the start, so a fresh model computes what a `True`
    model computes and a `True` model's checkpoint loads with `strict=False`.  The [B,nnz] weights of a batch are built once
    per forward (`ops.edge_time_weights`) and shared by the R components and by every block.

    `learn_edge_weights="signal"` lets them depend on the traffic itself (`EdgeSignalWeights`' arithmetic): `edge_crow`,
    `edge_col` and `edge_weight` as above plus `edge_proj.weight` [2*edge_rank, C*T_in], which projects every node's most
    recent input window (`edge_features`) to a row-side and a column-side vector of `edge_rank` values; the weight of edge
    i -> j is `edge_weight` plus the dot product of i's row side and j's column side.  The column half of `edge_proj.weight`
    starts at zero, so a fresh model computes what a `True` model computes and a `True` model's checkpoint loads with
    `strict=False`.  Built once per forward (`ops.edge_signal_weights`), shared by the R components and by every block.

    `edge_dropout=p` in (0,1) regularises the graph, with any `learn_edge_weights`: the layer is `(softmax(S) * A) x`, linear
    in `A`, so dropout on the masked attention is dropout on the stored edge weights.  In training mode one [B,nnz] mask per
    forward -- each edge of each sample dropped with probability p, the kept ones scaled by 1 / (1 - p), the stored
    diagonal left alone unless `edge_dropout_keep_self=False` -- is applied to the weights once they are formed
    (`ops.edge_dropout`) and shared by the R components and by every block; the frozen graph takes the per-sample sparse
    path on the pattern of `adj != 0`, without a weight gradient.  The masks come from a counter-based stream
    {`edge_dropout_seed`, step} in device memory (a non-persistent buffer: no `state_dict` key) that advances by one per
    training forward, inside a captured step too; sample b of the batch draws as global sample
    `edge_dropout_sample_offset + b`, so a sharded batch sees the masks of the whole one.  `eval()`, `attention_maps` and
    `torch.no_grad()` draw nothing.  `edge_dropout_state()` / `set_edge_dropout_state()` snapshot and restore the stream.
    The default 0 adds no buffer, key or launch.

    `missing_edges="scale" | "drop" | m` takes a sensor with missing input readings out of the graph for that sample: the
    edges OUT OF node j are multiplied by a gate from the number c of valid readings in j's most recent input window --
    c / T_in ("scale"), 1 only at c == T_in ("drop"), or 1 where c >= m (an int m in 1..T_in) -- so an imputed window
    reaches the neighbours at reduced weight or not at all.  The validity windows are `X[:, 0, -1]`, the LAST input channel
    of the most recent component: build the data with `make_loaders(..., input_null_value=..., mask_channel=True)` and the
    model with `in_channels=data.input_channels`.  Nothing can check that without reading the batch back: on inputs without
    a validity channel the last channel's readings are taken for one.  The [B,nnz] gate is applied once per forward, after
    the weights are formed and after `edge_dropout`, and shared by the R components and by every block
    (`ops.edge_validity`); with the option on the adjacency is always the batched sparse form, on the pattern of `adj != 0`
    for the frozen graph.  Unlike dropout it is a function of the input, so `eval()`, `torch.no_grad()` and
    `attention_maps` apply it too.  The stored diagonal is exempt unless `missing_edges_keep_self=False`.  The softmax
    denominators still run over all nodes and the remaining edges are not rescaled.  No parameter and no `state_dict` key:
    checkpoints interchange with and without the option.  The default None adds no buffer, key or launch.
    """

    def __init__(self, components: Sequence[Dict], in_timesteps: int, out_timesteps: int, use_te: bool,
                 adj: torch.Tensor, learn_edge_weights: Union[bool, str] = False, edge_rank: int = 8,
                 edge_dropout: float = 0.0, edge_dropout_seed: int = 0, edge_dropout_keep_self: bool = True,
                 missing_edges=None, missing_edges_keep_self: bool = True):
        if not (isinstance(learn_edge_weights, bool)
                or (isinstance(learn_edge_weights, str) and learn_edge_weights in ("time", "signal"))):
            raise ValueError(f'learn_edge_weights must be False, True, "time" or "signal", got {learn_edge_weights!r}')
        if learn_edge_weights == "signal":
            _check_edge_rank(edge_rank)
        edge_dropout = _check_edge_dropout(edge_dropout)
        missing_edges = _check_missing_edges(missing_edges, in_timesteps)
        super().__init__()
        n_nodes = len(adj)
        if use_te:
            self.te = TimeEmbedding(len(components), n_nodes, out_timesteps)
        else:
            self.te = None
            self.W = nn.Parameter(torch.empty(len(components), n_nodes, out_timesteps))
        self.adj = nn.Parameter(adj.detach().clone().float(), requires_grad=False)
        self.tpcs = nn.ModuleList(
            TPC(channels=c["channels"], n_nodes=n_nodes, in_timesteps=in_timesteps, out_timesteps=out_timesteps,
                dilations=c["dilations"]) for c in components)
        self.stack_components = True   # False: evaluate the components one by one, as the reference does
        self.learn_edge_weights = learn_edge_weights
        if self.learn_edge_weights:
            pattern = self.adj.detach().cpu().to_sparse_csr()
            self.register_buffer("edge_crow", pattern.crow_indices().clone())
            self.register_buffer("edge_col", pattern.col_indices().clone())
            self.edge_weight = nn.Parameter(pattern.values().clone())
        if self.learn_edge_weights == "time":
            self.edge_h_ebd = nn.Embedding(24, self.edge_weight.numel())
            self.edge_d_ebd = nn.Embedding(7, self.edge_weight.numel())
        if self.learn_edge_weights == "signal":
            self.edge_rank = edge_rank
            self.edge_proj = nn.Linear(components[0]["channels"][0] * in_timesteps, 2 * edge_rank, bias=False)
        self.reset_parameters()
        if self.learn_edge_weights:
            # after reset_parameters, which re-initialises every 1-D trainable tensor (and every table)
            with torch.no_grad():
                self.edge_weight.copy_(self.adj.detach().cpu().to_sparse_csr().values())
                if self.learn_edge_weights == "time":
                    self.edge_h_ebd.weight.zero_()
                    self.edge_d_ebd.weight.zero_()
                if self.learn_edge_weights == "signal":      # the row half keeps its Xavier values
                    self.edge_proj.weight[self.edge_rank:].zero_()
        self.edge_dropout = edge_dropout
        self.edge_dropout_sample_offset = 0    # this process's first sample in the global batch (the engine sets it)
        if self.edge_dropout > 0:
            # non-persistent: the state_dict keeps the reference's keys (and those of learn_edge_weights)
            pattern = self.adj.detach().cpu().to_sparse_csr()
            crow, col = pattern.crow_indices(), pattern.col_indices()
            rows = torch.repeat_interleave(torch.arange(n_nodes), crow[1:] - crow[:-1])
            self.register_buffer("edge_drop_state", ops.edge_dropout_state(edge_dropout_seed, "cpu"), persistent=False)
            self.register_buffer("edge_drop_exempt", (rows == col).to(torch.uint8) if edge_dropout_keep_self else None,
                                 persistent=False)
            if not self.learn_edge_weights:      # the frozen graph's pattern, and where its values sit in `adj`
                self.register_buffer("edge_drop_crow", crow.clone(), persistent=False)
                self.register_buffer("edge_drop_col", col.clone(), persistent=False)
                self.register_buffer("edge_drop_index", rows * n_nodes + col, persistent=False)
        self.missing_edges = missing_edges
        if self.missing_edges is not None:
            # non-persistent, and no parameter: checkpoints interchange with and without the option
            pattern = self.adj.detach().cpu().to_sparse_csr()
            crow, col = pattern.crow_indices(), pattern.col_indices()
            self.register_buffer("edge_valid_exempt", _self_loops(crow, col) if missing_edges_keep_self else None,
                                 persistent=False)
            if not self.learn_edge_weights:      # the frozen graph's pattern, and where its values sit in `adj`
                rows = torch.repeat_interleave(torch.arange(n_nodes), crow[1:] - crow[:-1])
                self.register_buffer("edge_valid_crow", crow.clone(), persistent=False)
                self.register_buffer("edge_valid_col", col.clone(), persistent=False)
                self.register_buffer("edge_valid_index", rows * n_nodes + col, persistent=False)

    def _drops_edges(self) -> bool:
        """Masks are drawn in training mode with gradients enabled only: `eval()`, `attention_maps` and any evaluation under
        `torch.no_grad()` draw nothing and leave the stream where it is."""
        return self.edge_dropout > 0 and self.training and torch.is_grad_enabled()

    def _drop_edges(self, weights: torch.Tensor, samples: int) -> torch.Tensor:
        return ops.edge_dropout(weights, self.edge_dropout, self.edge_drop_state,
                                sample_offset=int(self.edge_dropout_sample_offset), exempt=self.edge_drop_exempt,
                                samples=samples if weights.dim() == 1 else None)

    def _gate_missing(self, weights: torch.Tensor, X: torch.Tensor, crow: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
        """[B,nnz]: `weights` ([nnz] or [B,nnz]) gated by the validity windows X[:, 0, -1], read where they are."""
        return ops.edge_validity(weights, X[:, 0, -1], crow, col, mode=self.missing_edges, exempt=self.edge_valid_exempt)

    def _edge_adjacency(self, weights: torch.Tensor, crow: torch.Tensor, col: torch.Tensor, samples: Optional[int],
                        X: Optional[torch.Tensor]):
        """The adjacency of `weights` on (crow, col): dropped (`samples`: their number, or None), then gated (X, or None)."""
        if samples is not None:
            weights = self._drop_edges(weights, samples)
        if X is not None:
            weights = self._gate_missing(weights, X, crow, col)
        return ops.edge_adjacency(crow, col, weights)

    def edge_dropout_state(self) -> Optional[Dict[str, int]]:
        """{"seed", "step"} of the mask stream (reads two words back from the device); None for a model that drops nothing."""
        return _read_edge_dropout_state(self.edge_drop_state) if self.edge_dropout > 0 else None

    def set_edge_dropout_state(self, state) -> None:
        if self.edge_dropout <= 0:
            raise ValueError("set_edge_dropout_state: this model was built with edge_dropout=0 and has no mask stream")
        _write_edge_dropout_state(self.edge_drop_state, state)

    @staticmethod
    def edge_features(X: torch.Tensor) -> torch.Tensor:
        """X [B,R,C,N,T] -> f [B,N,C*T], f[b,n,c*T+t] = X[b,0,c,n,t]: every node's window of the most recent component."""
        x = X[:, 0]
        return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], x.shape[1] * x.shape[3])

    def adjacency(self, H: torch.Tensor = None, D: torch.Tensor = None, X: torch.Tensor = None):
        """What the blocks get: the frozen dense `adj`, the sparse CSR adjacency of the learned edge weights, or the batched
        CSR adjacency [B,N,N] of the weights of the batch's hours `H` and days `D` ("time") or of its inputs `X` ("signal").
        With `edge_dropout > 0`, in training mode with gradients enabled, always the batched form: one [B,nnz] draw on the
        weights once they are formed (`ops.edge_dropout`), shared by the R components and by every block; B is read from H
        (or X).  With `missing_edges`, always -- in eval mode and under no_grad too -- the batched form, gated by the validity
        windows of `X` (`ops.edge_validity`) after the dropout."""
        drop = self._drops_edges()
        gate = self.missing_edges is not None
        if gate and X is None:
            raise ValueError("missing_edges: the gate is formed from the batch's validity windows X[:, 0, -1], pass its "
                             "inputs X (batch_adjacency does)")
        samples = None
        if drop:
            batch = H if H is not None else X
            if batch is None:
                raise ValueError("edge_dropout: the masks are drawn per sample, pass the batch's H and D (or its inputs X)")
            samples = batch.shape[0]
        if not self.learn_edge_weights:
            if not drop and not gate:
                return self.adj
            crow, col, index = ((self.edge_valid_crow, self.edge_valid_col, self.edge_valid_index) if gate else
                                (self.edge_drop_crow, self.edge_drop_col, self.edge_drop_index))
            weights = self.adj.detach().reshape(-1).index_select(0, index)
            return self._edge_adjacency(weights, crow, col, samples, X if gate else None)
        if self.learn_edge_weights == "signal":
            if X is None:
                raise ValueError('learn_edge_weights="signal": the adjacency depends on the batch, pass its inputs X')
            weights = ops.edge_signal_weights(self.edge_weight, self.edge_proj(self.edge_features(X)), self.edge_crow,
                                              self.edge_col)
        elif self.learn_edge_weights == "time":
            if H is None or D is None:
                raise ValueError('learn_edge_weights="time": the adjacency depends on the batch, pass its H and D')
            weights = ops.edge_time_weights(self.edge_weight, self.edge_h_ebd.weight, self.edge_d_ebd.weight, H, D)
        else:
            weights = self.edge_weight
        return self._edge_adjacency(weights, self.edge_crow, self.edge_col, samples, X if gate else None)

    def batch_adjacency(self, X: torch.Tensor, H: torch.Tensor, D: torch.Tensor):
        """`adjacency` for one batch of `forward`'s inputs; only "signal" and `missing_edges` are handed X."""
        needs_x = self.learn_edge_weights == "signal" or self.missing_edges is not None
        return self.adjacency(H, D, X) if needs_x else self.adjacency(H, D)

    def forward(self, X: torch.Tensor, H: torch.Tensor, D: torch.Tensor) -> torch.Tensor:
        if self.stack_components and stacked.can_stack(self):
            # all components in each kernel launch (stacked.py) instead of the reference's loop (msgat.py:204)
            return stacked.forward(self, X, H, D)
        gates = self.te(H, D).unbind(1) if self.te is not None else self.W.unbind(0)
        adjacency = self.batch_adjacency(X, H, D)
        out = None
        for tpc, x, gate in zip(self.tpcs, X.unbind(1), gates):
            term = tpc(x, adjacency) * gate
            out = term if out is None else out + term
        return out

    def attention_maps(self, X: torch.Tensor, H: torch.Tensor, D: torch.Tensor, weights: str = "masked") -> Dict[str, torch.Tensor]:
        """The graph attention of every GACN for the inputs of `forward`, keyed by the reference's module names
        (`tpcs.{r}.tgacns.{l}.gacn`), one [B,N,N] tensor each: "masked" = `att * adjacency` as a sparse COO tensor,
        "softmax" = `att`, dense (`ops.gacn`'s need_weights; "softmax_grad" is accepted and gives the same tensors).  Runs the
        forward under torch.no_grad(), on whichever path `forward` takes (stacked or component by component), and returns
        no prediction; for maps that carry a gradient wrap a grad-enabled `forward` in `ops.collect_weights("softmax_grad")`."""
        R, L = len(self.tpcs), len(self.tpcs[0].tgacns)
        B = X.shape[0]
        with torch.no_grad(), ops.collect_weights(weights) as seen:
            stacked_path = self.stack_components and stacked.can_stack(self)
            self.forward(X, H, D)
        maps = {}
        if stacked_path:     # one call per level with R * B groups, relation-major
            for level, entry in enumerate(seen):
                for r in range(R):
                    maps[f"tpcs.{r}.tgacns.{level}.gacn"] = ops.weights_of(entry, weights, (B,), slice(r * B, (r + 1) * B))
        else:                # one call per (component, level), in that order
            it = iter(seen)
            for r, tpc in enumerate(self.tpcs):
                for level in range(len(tpc.tgacns)):
                    maps[f"tpcs.{r}.tgacns.{level}.gacn"] = ops.weights_of(next(it), weights, (B,))
        if len(maps) != sum(len(t.tgacns) for t in self.tpcs) or (stacked_path and len(seen) != L):
            raise RuntimeError(f"attention_maps: {len(seen)} graph-attention calls for {R} components of {L} blocks")
        return maps

    def reset_parameters(self) -> None:
        """xavier_normal_ for >= 2-D, U(-size0^-1/2, +size0^-1/2) for 1-D, every trainable tensor (msgat.py:206-217)."""
        with torch.no_grad():
            for p in self.parameters():
                if not p.requires_grad:
                    continue
                if p.dim() >= 2:
                    nn.init.xavier_normal_(p)
                else:
                    bound = p.size(0) ** -0.5
                    p.uniform_(-bound, bound)


_WIDTHS = {  # msgat.py:220-229
    "ms-gat48": dict(hidden=48, dilations=[[1, 2], [2, 4]]),
    "ms-gat72": dict(hidden=72, dilations=[[1, 2], [2, 4]]),
    "ms-gat96": dict(hidden=96, dilations=[[1, 1, 2, 2], [4, 4]]),
}
_WIDTHS["ms-gat"] = _WIDTHS["ms-gat72"]  # main.py:17


def build_msgat(name: str, n_components: int, in_channels: int, **kwargs) -> MSGAT:
    cfg = _WIDTHS[name]
    comp = {"channels": [in_channels, cfg["hidden"], cfg["hidden"]], "dilations": cfg["dilations"]}
    return MSGAT([comp] * n_components, **kwargs)


def msgat48(n_components: int, in_channels: int, **kwargs) -> MSGAT:
    return build_msgat("ms-gat48", n_components, in_channels, **kwargs)


def msgat72(n_components: int, in_channels: int, **kwargs) -> MSGAT:
    return build_msgat("ms-gat72", n_components, in_channels, **kwargs)


def msgat96(n_components: int, in_channels: int, **kwargs) -> MSGAT:
    return build_msgat("ms-gat96", n_components, in_channels, **kwargs)


models = {name: (lambda n=name: (lambda **kw: build_msgat(n, **kw)))() for name in _WIDTHS}
