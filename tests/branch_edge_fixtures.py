"""What the branch-edge tests (test_gpu_branch_edges.py, test_branch_edges_cpu.py) and the two older files that state the
same op sequences (test_gpu_branches.py, test_gpu_model.py) share: the case tables, seeded inputs, and the restatements
of the channel / temporal branch ops, of one MEAM block's parameters and of a whole model, written once and evaluated in
whatever dtype their arguments have (float64: the oracle; float32 on the CPU: the reference's own rounding).

Channel attention (attention.py:88-94 + msgat.py:93-94): p [G,C,T], Wc [R,T,T], conv [R,cb,C] -> Mc [G,cb,C].
Temporal attention (attention.py:58-66 as the taps of msgat.py:66-74): q [G,N,T], Wt1 / Wt2 [R,K,N] -> taps [G,2,T,T]."""
import torch

from oracle import dense_torch

# ---- A: score edges ------------------------------------------------------------------------------------------------
# channel (R, Bg, C, cb, T); the last is the widest the backward accepts (CHANATT_LDS_FLOATS below)
CHANNEL_CASES = [(2, 2, 72, 24, 12), (1, 2, 96, 32, 8), (1, 3, 7, 4, 4), (1, 2, 114, 38, 12)]
# by C: the first seed whose draw has no two leading scores of a row within 9 of each other at the saturated scale (a
# near-tie among ~100 scores of spread 3e3 happens in one row of 150; fp32 rounds scores of 1e4 to 1e-3, which such a
# row turns into a 1e-4 error of the map in ANY fp32 evaluation).  test_branch_edges_cpu.py asserts what they give.
CHANNEL_SEED = {72: 5, 96: 1, 7: 1, 114: 4}
# temporal (R, Bg, N, K, T, dilation)
TEMPORAL_CASES = [(1, 3, 129, 10, 12, 2), (2, 1, 1025, 10, 8, 4), (1, 2, 64, 10, 4, 1)]
LARGE, SATURATED = 3.0, 25.0
MAGNITUDES = [(1e-6, 1e-8), (1e3, 1e5), (3e7, 1e-3)]          # (cq, cg) of test_gpu_score_edges.py
ONE_HOT = 0.999                                               # a softmax row counts as one-hot from this largest entry on


def channel_inputs(case, scale=1.0, cq=1.0, cg=1.0, structure=None):
    """CPU fp32 (pooled, Wc, conv, dMc): pooled ~ scale cq N(0,1), Wc ~ 0.4 N / cq^2 (the scores stay those of cq = 1),
    conv ~ 0.5 N, dMc ~ cg N.  structure "twins": pooled rows 0 and 1 of every group are identical (two identical rows of
    the attention, two equal scores in every row); "zero": row 2 is zero (a uniform row, a zero column of scores)."""
    R, Bg, C, cb, T = case
    gen = torch.Generator().manual_seed(CHANNEL_SEED[C])
    p = torch.randn(R * Bg, C, T, generator=gen) * (scale * cq)
    Wc = torch.randn(R, T, T, generator=gen) * (0.4 / (cq * cq))
    conv = torch.randn(R, cb, C, generator=gen) * 0.5
    dMc = torch.randn(R * Bg, cb, C, generator=gen) * cg
    if structure == "twins":
        p[:, 1] = p[:, 0]
    elif structure == "zero":
        p[:, 2] = 0.0
    return p, Wc, conv, dMc


def temporal_inputs(case, scale=1.0, cq=1.0, cg=1.0, structure=None):
    """CPU fp32 (pooled, Wt1, Wt2, dtaps): pooled ~ scale cq N(0,1), Wt ~ N^-1/2 N / cq each, dtaps ~ cg N.  structure
    "twins": time steps 0 and 1 of every node are identical (two identical rows); "zero": step 2 is zero (a uniform row)."""
    R, Bg, N, K, T, _ = case
    gen = torch.Generator().manual_seed(2000 + N + T)
    q = torch.randn(R * Bg, N, T, generator=gen) * (scale * cq)
    W1 = torch.randn(R, K, N, generator=gen) * (N ** -0.5 / cq)
    W2 = torch.randn(R, K, N, generator=gen) * (N ** -0.5 / cq)
    dtaps = torch.randn(R * Bg, 2, T, T, generator=gen) * cg
    if structure == "twins":
        q[:, :, 1] = q[:, :, 0]
    elif structure == "zero":
        q[:, :, 2] = 0.0
    return q, W1, W2, dtaps


def channel_attention(p, Wc):
    """att [R,Bg,C,C] = softmax_rows((p Wc) p^T)"""
    R = Wc.shape[0]
    pv = p.view(R, p.shape[0] // R, *p.shape[1:])
    return torch.softmax(pv @ Wc.unsqueeze(1) @ pv.transpose(2, 3), dim=-1)


def channel_attention_mix_dense(p, Wc, conv):
    """Mc [G,cb,C] = conv_r att_g: the op sequence ops.channel_attention_mix replaces"""
    return (conv.unsqueeze(1) @ channel_attention(p, Wc)).reshape(p.shape[0], conv.shape[1], p.shape[1])


def temporal_attention(q, W1, W2):
    """att [G,T,T] = softmax_rows((q^T Wt1^T)(q^T Wt2^T)^T)"""
    R = W1.shape[0]
    G, N, T = q.shape
    per_t = q.view(R, G // R, N, T).transpose(2, 3)
    left, right = per_t @ W1.transpose(1, 2).unsqueeze(1), per_t @ W2.transpose(1, 2).unsqueeze(1)
    return torch.softmax(left @ right.transpose(2, 3), dim=-1).reshape(G, T, T)


def temporal_attention_taps_dense(q, W1, W2, dil):
    """taps [G,2,T,T] = (att shifted down by the dilation, att): the op sequence ops.temporal_attention_taps replaces"""
    att = temporal_attention(q, W1, W2)
    T = att.shape[-1]
    shifted = torch.zeros_like(att) if dil >= T else torch.nn.functional.pad(att[:, : T - dil], (0, 0, dil, 0))
    return torch.stack([shifted, att], dim=1)


def evaluate(fn, inputs, cotangent, dtype):
    """(output, gradients at every input) of `fn(*inputs)` by autograd on the CPU in `dtype`"""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, cotangent.to(dtype)))


def one_hot_fraction(att):
    return float((att.max(dim=-1).values > ONE_HOT).double().mean())


def _cancelling(att, d):
    """|att d| + |<d, att>| att: the size of the two terms whose difference is dS = att (d - <d, att>)"""
    X = att * d
    return X.abs() + X.sum(-1, keepdim=True).abs() * att


def channel_cancelling_terms(p, Wc, conv, dMc):
    """Per gradient of the channel op, the largest entry of the cancelling terms of its softmax backward carried through
    the products that follow them (float64): what an absolute error of the gradient is measured against where the rows
    are one-hot and the gradient itself is a rounding-sized remainder."""
    p, Wc, conv, dMc = (t.double() for t in (p, Wc, conv, dMc))
    R, (G, C, T) = Wc.shape[0], p.shape
    att = channel_attention(p, Wc)                                         # [R,Bg,C,C]
    pv, dM = p.view(R, G // R, C, T), dMc.view(R, G // R, -1, C)
    dS = _cancelling(att, conv.unsqueeze(1).transpose(2, 3) @ dM)
    t1, Wa = (pv @ Wc.unsqueeze(1)).abs(), Wc.abs().unsqueeze(1)
    dt1 = dS @ pv.abs()
    return dict(dpooled=(dS.transpose(2, 3) @ t1 + dt1 @ Wa.transpose(2, 3)).max(),
                dWc=(pv.abs().transpose(2, 3) @ dt1).sum(1).max(),
                dconv=(dM.abs() @ att.transpose(2, 3)).sum(1).max())


def temporal_cancelling_terms(q, W1, W2, dtaps, dil):
    """The same for the temporal op: d = dtaps[1] + dtaps[0] shifted up by the dilation."""
    q, W1, W2, dtaps = (t.double() for t in (q, W1, W2, dtaps))
    R, (G, N, T) = W1.shape[0], q.shape
    att = temporal_attention(q, W1, W2).view(R, G // R, T, T)
    d = dtaps[:, 1].clone()
    if dil < T:
        d[:, : T - dil] += dtaps[:, 0, dil:]
    dS = _cancelling(att, d.view(R, G // R, T, T))
    per_t = q.view(R, G // R, N, T).transpose(2, 3)                        # [R,Bg,T,N]
    A, B = W1.unsqueeze(1), W2.unsqueeze(1)                                # [R,1,K,N]
    left, right = (per_t @ A.transpose(2, 3)).abs(), (per_t @ B.transpose(2, 3)).abs()
    dleft, dright = dS @ right, dS.transpose(2, 3) @ left                  # [R,Bg,T,K]
    return dict(dpooled=(dleft @ A.abs() + dright @ B.abs()).max(),
                dWt1=(dleft.transpose(2, 3) @ per_t.abs()).sum(1).max(),
                dWt2=(dright.transpose(2, 3) @ per_t.abs()).sum(1).max())


# ---- B: trip boundaries --------------------------------------------------------------------------------------------
TEMPORAL_TRIP_N = [1, 127, 128, 129, 256, 1024, 1025, 2049]   # tiles of 128 forward, trips of 1024 lanes backward
# (N, C, T): every N next to a trip of 64 / 256 nodes, every C next to the 16 channels per block of the node pool's
# weight gradient, each T once or more
POOL_CASES = [(63, 1, 4), (64, 16, 8), (65, 17, 12), (255, 17, 16), (256, 1, 12), (257, 16, 4), (1025, 17, 8), (1025, 1, 16),
              (256, 17, 4)]
POOL_SLICE_CASE = (65, 17, 12)
TIME_MIX_CASES = [(16, 24, 33), (16, 5, 1), (4, 24, 33), (4, 3, 1), (8, 16, 65)]    # (T, Co, N); K = 2, R = 2
TIME_MIX_SLICE_CASE = (16, 24, 33)


POOL_R, POOL_BG = 2, 2


def pool_inputs(N, C, T):
    """CPU fp32 (x [4,C,N,T], node weights [2,N], channel weights [2,C], dpooled_n [4,C,T], dpooled_c [4,N,T])"""
    gen = torch.Generator().manual_seed(3000 + 31 * N + 7 * C + T)
    G = POOL_R * POOL_BG
    return (torch.randn(G, C, N, T, generator=gen), torch.randn(POOL_R, N, generator=gen) * N ** -0.5,
            torch.randn(POOL_R, C, generator=gen) * C ** -0.5, torch.randn(G, C, T, generator=gen),
            torch.randn(G, N, T, generator=gen))


def node_pool_dense(x, w):
    """pooled[g,c,t] = sum_n w[r,n] x[g,c,n,t] (attention.py:89), r = g // Bg"""
    return torch.einsum("gn,gcnt->gct", w.repeat_interleave(x.shape[0] // w.shape[0], dim=0), x)


def channel_pool_dense(x, alpha):
    """pooled[g,n,t] = sum_c alpha[r,c] x[g,c,n,t] (attention.py:59)"""
    return torch.einsum("gc,gcnt->gnt", alpha.repeat_interleave(x.shape[0] // alpha.shape[0], dim=0), x)


def time_mix_inputs(T, Co, N):
    """CPU fp32 (y [4,2 Co,N,T], A [4,2,T,T] one pair per sample, bias [2,Co], dout [4,Co,N,T])"""
    gen = torch.Generator().manual_seed(4000 + 100 * T + 3 * Co + N)
    G = POOL_R * POOL_BG
    return (torch.randn(G, 2 * Co, N, T, generator=gen), torch.randn(G, 2, T, T, generator=gen) * T ** -0.5,
            torch.randn(POOL_R, Co, generator=gen), torch.randn(G, Co, N, T, generator=gen))


def time_mix_dense(y, A, bias):
    """out[g,o,n,t] = bias[r,o] + sum_k sum_i A[g,k,t,i] y[g,k Co+o,n,i]: msgat_time_mix with a matrix pair per sample"""
    G, KC, N, T = y.shape
    K, R = A.shape[1], bias.shape[0]
    out = torch.einsum("gkti,gkoni->gont", A, y.view(G, K, KC // K, N, T))
    return out + bias.repeat_interleave(G // R, dim=0)[:, :, None, None]


# ---- C: the whole block ---------------------------------------------------------------------------------------------
MEAM_BLOCKS = [(3, 72, [1, 2]), (72, 72, [2, 4]), (1, 48, [1, 2]), (96, 96, [4, 4]), (3, 96, [1, 1, 2, 2])]
MEAM_SHAPES = [(4, 23), (4, 127), (4, 128), (8, 63), (8, 64), (16, 23), (16, 32), (16, 64)]     # (T, N); 512 = T N thrice
MEAM_BATCH = 3
STACKED_CASES = [(4, 128), (8, 64), (16, 64)]                 # (T, N) of msgat72, R = 2, three input channels


def draw_parameters(module, gen):
    """What MSGAT.reset_parameters draws (msgat.py:206-217), from `gen`: Xavier normal from two axes up, U(+-size0^-1/2)
    for vectors."""
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() >= 2:
                field = p[0][0].numel()
                std = (2.0 / ((p.shape[0] + p.shape[1]) * field)) ** 0.5
                p.copy_(torch.randn(p.shape, generator=gen) * std)
            else:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * p.shape[0] ** -0.5)


def meam_problem(Ci, Co, dilations, T, N):
    """-> (block on the CPU, x, dout, adjacency): parameters by `draw_parameters`, LayerNorm weight + 1; x, dout ~ N(0,1)
    [3,C,N,T]."""
    import ms_gat_amd
    from ms_gat_amd import model
    gen = torch.Generator().manual_seed(100 * Ci + 10 * T + N)
    block = model.MEAM(Ci, Co, n_nodes=N, n_timesteps=T, dilations=dilations)
    draw_parameters(block, gen)
    with torch.no_grad():
        block.ln.weight += 1.0
    x = torch.randn(MEAM_BATCH, Ci, N, T, generator=gen)
    dout = torch.randn(MEAM_BATCH, Co, N, T, generator=gen)
    return block, x, dout, ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5)


def meam_reference(state, x, dout, adj, dilations, relu_mask, dtype):
    """dense_torch.meam_dense with the ReLU mask pinned, in `dtype` on the device of `x`:
    -> {"out", "dx", parameter name: gradient}"""
    leaves = {k: v.detach().to(x.device, dtype).clone().requires_grad_(True) for k, v in state.items()}
    x_ = x.detach().to(dtype).clone().requires_grad_(True)
    out = dense_torch.meam_dense(x_, adj.to(x.device, dtype), leaves, dilations, relu_mask=relu_mask)
    names = list(leaves)
    grads = torch.autograd.grad(out, [x_] + [leaves[n] for n in names], dout.to(x.device, dtype))
    return dict(zip(["out", "dx"] + names, [out.detach()] + list(grads)))


def msgat_dense(leaves, adj, dilations, X, H, D, eps=1e-5):
    """A whole MSGAT with a time embedding by the reference's dense op sequence (msgat.py:203-205 around
    dense_torch.meam_dense): leaves = {state_dict key: tensor} in the dtype of the evaluation, dilations = one list per
    block, X [B,R,C,N,T] -> prediction [B,N,T_out]."""
    B, R, _, N, T = X.shape
    gate = (leaves["te.h_ebd.weight"][H] + leaves["te.d_ebd.weight"][D]).view(B, R, N, -1)
    out = 0
    for r in range(R):
        x = X[:, r]
        for l, dil in enumerate(dilations):
            prefix = f"tpcs.{r}.tgacns.{l}."
            sub = {k[len(prefix):]: v for k, v in leaves.items() if k.startswith(prefix)}
            x = dense_torch.meam_dense(x, adj, sub, dil, eps)
        x = torch.nn.functional.layer_norm(x, [T], leaves[f"tpcs.{r}.ln.weight"], leaves[f"tpcs.{r}.ln.bias"], eps)
        y = torch.nn.functional.conv2d(x.transpose(1, 3), leaves[f"tpcs.{r}.fc.weight"], leaves[f"tpcs.{r}.fc.bias"])
        out = out + y[..., 0].transpose(1, 2) * gate[:, r]
    return out


def stacked_problem(T, N):
    """-> (msgat72 on the CPU, X, H, D, dout), drawn as test_whole_model_matches_the_dense_op_sequence draws them.  Its
    seeds (7, 11) leave the fp32 evaluation of `msgat_dense` 3.1e-5 from float64 at T = 4 (a LayerNorm bias); with these
    it stays under 1.7e-5 at all three shapes, a sixth of the bar (asserted in test_branch_edges_cpu.py)."""
    import ms_gat_amd
    from ms_gat_amd import model
    torch.manual_seed(10)
    gen = torch.Generator().manual_seed(14)
    R, cin, B = 2, 3, MEAM_BATCH
    net = model.msgat72(n_components=R, in_channels=cin, in_timesteps=T, out_timesteps=T, use_te=True,
                        adj=ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5))
    X = torch.randn(B, R, cin, N, T, generator=gen)
    H = torch.randint(0, 24, (B,), generator=gen)
    D = torch.randint(0, 7, (B,), generator=gen)
    return net, X, H, D, torch.randn(B, N, T, generator=gen)


def msgat_reference(net, X, H, D, dout, dtype):
    """-> (prediction, {parameter name: gradient}) of `msgat_dense` with the parameters of `net`, in `dtype` on X's device"""
    P = {k: v.detach().to(X.device, dtype) for k, v in net.state_dict().items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items() if k != "adj"}
    dilations = [m.dilations for m in net.tpcs[0].tgacns]
    out = msgat_dense(leaves, P["adj"], dilations, X.to(dtype), H, D)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, [leaves[n] for n in names], dout.to(dtype), allow_unused=True)
    return out.detach(), {n: g for n, g in zip(names, grads) if g is not None}


# ---- D: the LDS envelope of the channel attention ---------------------------------------------------------------------
CHANATT_LDS_FLOATS = (160 * 1024 - 1024) // 4      # 40704: kLdsMax - 1024 bytes (csrc/common.hpp, csrc/smallatt.hip)


def chanatt_fwd_floats(C, cb, T):
    """p, p Wc [C,T] each, Wc [T,T], the scores [C,C+1], the convolution weight [cb,C]"""
    return 2 * C * T + T * T + C * (C + 1) + cb * C


def chanatt_bwd_floats(C, cb, T):
    """att and its gradient [C,C+1] each, p, p Wc and its gradient [C,T] each, Wc [T,T], dMc and the weight [cb,C] each"""
    return 2 * C * (C + 1) + 3 * C * T + T * T + 2 * cb * C


def chanatt_fits(C, cb, T):
    """(forward fits, backward fits)"""
    return chanatt_fwd_floats(C, cb, T) <= CHANATT_LDS_FLOATS, chanatt_bwd_floats(C, cb, T) <= CHANATT_LDS_FLOATS


WIDE = (120, 40, 33, 12)       # (C, cb, N, T): the forward kernel would fit, its backward would not


def cacn_problem():
    """-> (CACN(120 -> 40) on the CPU with `draw_parameters`, x [3,120,33,12], dout [3,40,33,12])"""
    from ms_gat_amd import model
    C, cb, N, T = WIDE
    gen = torch.Generator().manual_seed(120)
    m = model.CACN(C, cb, N, T)
    draw_parameters(m, gen)
    return m, torch.randn(MEAM_BATCH, C, N, T, generator=gen), torch.randn(MEAM_BATCH, cb, N, T, generator=gen)


def wide_model_problem():
    """-> (a two-component MSGAT of two 120-channel blocks on the CPU, X, H, D, dout)"""
    import ms_gat_amd
    from ms_gat_amd import model
    C, _, N, T = WIDE
    torch.manual_seed(120)
    gen = torch.Generator().manual_seed(121)
    comp = {"channels": [3, C, C], "dilations": [[1, 2], [2, 4]]}
    net = model.MSGAT([comp] * 2, in_timesteps=T, out_timesteps=T, use_te=True,
                      adj=ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5))
    X = torch.randn(MEAM_BATCH, 2, 3, N, T, generator=gen)
    H = torch.randint(0, 24, (MEAM_BATCH,), generator=gen)
    D = torch.randint(0, 7, (MEAM_BATCH,), generator=gen)
    return net, X, H, D, torch.randn(MEAM_BATCH, N, T, generator=gen)
