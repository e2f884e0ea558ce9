"""GPU: the prediction head at long forecast horizons, 16 < T_out <= 64 (the reference's `--out-timesteps`, main.py:34,
which sizes the component head Conv2d(T_in -> T_out, [1, C]) of msgat.py:153,159).  The head kernels run such a horizon
as ceil(T_out / 16) output tiles of 16 (csrc/branches.hip); T_out <= 16 is the one-tile instance of the same kernel
templates, picked by the same launchers.

Against the float64 op sequence (conv2d, LayerNorm) at 1e-4 relative, the reference's own model at the fixtures of
tests/golden/make_golden_horizon.py, and the engine's HIP-graph replay against eager steps."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_parity, rel_err
from horizon_fixtures import CASES, load

pytestmark = pytest.mark.gpu
TOL = 1e-4
HORIZONS = (17, 24, 32, 33, 40, 48, 64)
SHAPES = ((17, 5), (300, 9), (883, 72))   # (N, C): node counts with a tail, channel counts off the chunk sizes


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(B, R, C, N, T, To, relu, seed):
    gen = torch.Generator().manual_seed(seed)
    dev = _dev()
    x = torch.randn(B, C, N, T, generator=gen)
    if relu:
        x = torch.relu(x + 0.3)                          # a ReLU output, as the blocks hand it over
    shp = (To, T, 1, C) if R == 1 else (R, To, T, 1, C)
    W = torch.randn(*shp, generator=gen) * (T * C) ** -0.5
    hb = torch.randn(*((To,) if R == 1 else (R, To)), generator=gen) * 0.1
    lw = 1 + 0.3 * torch.randn(*((T,) if R == 1 else (R, T)), generator=gen)
    lb = 0.2 * torch.randn(*((T,) if R == 1 else (R, T)), generator=gen)
    dout = torch.randn(B, N, To, generator=gen)
    return [t.to(dev) for t in (x, W, hb, lw, lb, dout)]


def _ref64(x, W, hb, lw, lb, dout, R, ln):
    """float64: the reference's op sequence, relation by relation -> (out, grads of x, W, bias, LN weight, LN bias)."""
    B, T = x.shape[0], x.shape[-1]
    Bg = B // R
    x64 = x.double().requires_grad_(True)
    p64 = [None if t is None else t.double().requires_grad_(True) for t in (W, hb, lw, lb)]
    outs = []
    for r in range(R):
        sl = slice(r * Bg, (r + 1) * Bg)
        Wr, br, lwr, lbr = [p if (p is None or R == 1) else p[r] for p in p64]
        xr = F.layer_norm(x64[sl], [T], lwr, lbr, 1e-5) if ln else x64[sl]
        outs.append(F.conv2d(xr.transpose(1, 3), Wr, br)[..., 0].transpose(1, 2))
    out = torch.cat(outs)
    out.backward(dout.double())
    return out.detach(), x64.grad, [None if p is None else p.grad for p in p64]


def _run(x, W, hb, lw, lb, dout, ln, relu):
    from ms_gat_amd import ops
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in (x, W, hb, lw, lb)]
    xs, Ws, hbs, lws, lbs = leaves
    out = ops.ln_head(xs, lws, lbs, 1e-5, Ws, hbs, relu_input=relu) if ln else ops.head(xs, Ws, hbs)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), [None if t is None else t.grad for t in leaves]


def _case(i, T, To):
    """The i-th combination of the sweep: shapes, stacking, ReLU input and the optional parameters rotate with i."""
    N, C = SHAPES[i % 3]
    R = (1, 3)[(i // 3) % 2]
    relu = i % 2 == 1
    affine = i % 4 != 2
    return N, C, R, relu, affine


@pytest.mark.parametrize("T", (4, 8, 12, 16))
@pytest.mark.parametrize("To", HORIZONS)
def test_head_and_ln_head_match_the_float64_convolution_at_long_horizons(T, To):
    i = HORIZONS.index(To) * 4 + (4, 8, 12, 16).index(T)
    N, C, R, relu, affine = _case(i, T, To)
    B = 2 * R
    x, W, hb, lw, lb, dout = _inputs(B, R, C, N, T, To, relu, seed=1000 + i)
    if not affine:
        hb = lw = lb = None
    # the head alone
    out, (gx, gW, gb, _, _) = _run(x, W, hb, None, None, dout, ln=False, relu=False)
    o64, gx64, (gW64, gb64, _, _) = _ref64(x, W, hb, None, None, dout, R, ln=False)
    assert out.shape == (B, N, To)
    assert rel_err(out.double(), o64) < TOL, "out"
    assert rel_err(gx.double(), gx64) < TOL, "dx"
    assert rel_err(gW.double(), gW64) < TOL, "dW"
    if hb is not None:
        assert rel_err(gb.double(), gb64) < TOL, "dbias"
    # LayerNorm + head, one backward pass
    out, (gx, gW, gb, glw, glb) = _run(x, W, hb, lw, lb, dout, ln=True, relu=relu)
    o64, gx64, (gW64, gb64, glw64, glb64) = _ref64(x, W, hb, lw, lb, dout, R, ln=True)
    if relu:
        gx64 = gx64 * (x > 0)                            # the mask of the ReLU that produced x (relu_input)
    assert rel_err(out.double(), o64) < TOL, "ln out"
    for name, a, b in (("ln dx", gx, gx64), ("ln dW", gW, gW64), ("ln dbias", gb, gb64), ("dln_weight", glw, glw64),
                       ("dln_bias", glb, glb64)):
        if b is not None:
            assert rel_err(a.double(), b) < TOL, name


TILE_SWITCH_HORIZONS = (1, 15, 16, 17, 49, 64)
# (N, C): a node tail inside one wave, then one node past a whole block; a channel count one past the forward's 32-channel
# chunk, then one past the backward's 8-channel chunk
TILE_SWITCH_SHAPES = ((17, 33), (257, 9))


@pytest.mark.parametrize("shape", TILE_SWITCH_SHAPES, ids=lambda s: f"n{s[0]}c{s[1]}")
@pytest.mark.parametrize("To", TILE_SWITCH_HORIZONS)
def test_head_launchers_pick_the_tile_count_at_every_switch(To, shape):
    """One launcher per entry point picks ceil(T_out / 16) in [1, 4]: T_out on both sides of the first switch, at one output,
    inside the last tile and at the limit, output and every gradient of ops.head and ops.ln_head against float64."""
    i = TILE_SWITCH_HORIZONS.index(To) * len(TILE_SWITCH_SHAPES) + TILE_SWITCH_SHAPES.index(shape)
    T = (4, 8, 12, 16)[i % 4]
    _, _, _, relu, affine = _case(i, T, To)
    (N, C), R, B = shape, 2, 4
    x, W, hb, lw, lb, dout = _inputs(B, R, C, N, T, To, relu, seed=2000 + i)
    if not affine:
        hb = lw = lb = None
    out, (gx, gW, gb, _, _) = _run(x, W, hb, None, None, dout, ln=False, relu=False)
    o64, gx64, (gW64, gb64, _, _) = _ref64(x, W, hb, None, None, dout, R, ln=False)
    assert out.shape == (B, N, To)
    for name, a, b in (("out", out, o64), ("dx", gx, gx64), ("dW", gW, gW64), ("dbias", gb, gb64)):
        if b is not None:
            assert rel_err(a.double(), b) < TOL, name
    out, (gx, gW, gb, glw, glb) = _run(x, W, hb, lw, lb, dout, ln=True, relu=relu)
    o64, gx64, (gW64, gb64, glw64, glb64) = _ref64(x, W, hb, lw, lb, dout, R, ln=True)
    if relu:
        gx64 = gx64 * (x > 0)                            # the mask of the ReLU that produced x (relu_input)
    for name, a, b in (("ln out", out, o64), ("ln dx", gx, gx64), ("ln dW", gW, gW64), ("ln dbias", gb, gb64),
                       ("dln_weight", glw, glw64), ("dln_bias", glb, glb64)):
        if b is not None:
            assert rel_err(a.double(), b) < TOL, name


def test_ln_head_at_pemsd7_size_with_24_outputs():
    """[96,72,883,12] (PEMSD7: 883 nodes, a batch of 32 for each of three components) with T_out = 24."""
    B, R, C, N, T, To = 96, 3, 72, 883, 12, 24
    x, W, hb, lw, lb, dout = _inputs(B, R, C, N, T, To, True, seed=7)
    out, (gx, gW, gb, glw, glb) = _run(x, W, hb, lw, lb, dout, ln=True, relu=True)
    o64, gx64, (gW64, gb64, glw64, glb64) = _ref64(x, W, hb, lw, lb, dout, R, ln=True)
    gx64 = gx64 * (x > 0)
    for name, a, b in (("out", out, o64), ("dx", gx, gx64), ("dW", gW, gW64), ("dbias", gb, gb64),
                       ("dln_weight", glw, glw64), ("dln_bias", glb, glb64)):
        assert rel_err(a.double(), b) < TOL, name


def test_horizon_limit_is_64():
    from ms_gat_amd import _lib, ops
    x, W, hb, _, _, _ = _inputs(2, 1, 5, 40, 12, 64, False, seed=3)
    assert ops.head(x, W, hb).shape == (2, 40, 64)
    x, W, hb, _, _, _ = _inputs(2, 1, 5, 40, 12, 65, False, seed=3)
    with pytest.raises(_lib.MsgatError):
        ops.head(x, W, hb)
    with pytest.raises(_lib.MsgatError):
        ops.ln_head(x, None, None, 1e-5, W, hb)
    assert "T_out <= 64" in _lib.lib().msgat_status_string(-3).decode()


@pytest.mark.parametrize("To", (24, 64))
def test_long_horizon_head_is_bitwise_reproducible(To):
    B, R, C, N, T = 6, 3, 72, 300, 12
    x, W, hb, lw, lb, dout = _inputs(B, R, C, N, T, To, True, seed=11)
    for ln in (False, True):
        a = _run(x, W, hb, lw, lb, dout, ln=ln, relu=True)
        b = _run(x, W, hb, lw, lb, dout, ln=ln, relu=True)
        assert torch.equal(a[0], b[0])
        for ga, gb in zip(a[1], b[1]):
            assert (ga is None and gb is None) or torch.equal(ga, gb)


def test_first_outputs_of_a_24_step_head_agree_with_a_12_step_head():
    B, R, C, N, T = 4, 2, 72, 300, 12
    x, W, hb, lw, lb, dout = _inputs(B, R, C, N, T, 24, True, seed=13)
    for ln in (False, True):
        long = _run(x, W, hb, lw, lb, dout, ln=ln, relu=True)
        short = _run(x, W[:, :12].contiguous(), hb[:, :12].contiguous(), lw, lb, dout[..., :12].contiguous(), ln=ln, relu=True)
        assert rel_err(long[0][..., :12], short[0]) < 1e-6
        dW_long = long[1][1][:, :12]
        assert rel_err(dW_long, short[1][1]) < 1e-6       # the weight gradient of an output row sees only that row


def _net(case):
    from ms_gat_amd import model
    name, factory, R, C, T, To, _ = case
    g, state, grads = load(name)
    net = getattr(model, factory)(n_components=R, in_channels=C, in_timesteps=T, out_timesteps=To, use_te=True,
                                  adj=state["adj"])
    net.load_state_dict(state)
    return g, net.to(_dev()), grads


# One gradient deep in the MEAM blocks of msgat72_to24_n32 (max-norm error 1.6e-5) has 1.3 % of its entries outside the
# per-entry floor 1e-5 max|b|.  The same entries miss with the head computed by torch (fp32 LayerNorm + conv2d):
# test_block_rounded_gradient_does_not_depend_on_the_head pins that, so this one tensor is held to the max-norm floor.
_BLOCK_ROUNDED = {("msgat72_to24_n32.npz", "tpcs.2.tgacns.1.cacn.seq.1.weight")}


def _torch_ln_head(x, lw, lb, eps, W, b=None, relu_input=False):
    """ops.ln_head restated with torch's fp32 ops (relation by relation; relu_input: the ReLU's backward mask)."""
    if relu_input:
        x = x * (x > 0)
    B, T = x.shape[0], x.shape[-1]
    R = 1 if W.dim() == 4 else W.shape[0]
    outs = []
    for r in range(R):
        pick = lambda p: p if (p is None or R == 1 or p.dim() == 1) else p[r]  # noqa: E731
        xn = F.layer_norm(x[r * (B // R):(r + 1) * (B // R)], [T], pick(lw), pick(lb), eps)
        outs.append(F.conv2d(xn.transpose(1, 3), pick(W), pick(b))[..., 0].transpose(1, 2))
    return torch.cat(outs)


def _model_grads(case, stack, monkeypatch=None):
    from ms_gat_amd import engine, ops
    g, net, grads = _net(case)
    net.stack_components = stack
    if monkeypatch is not None:
        monkeypatch.setattr(ops, "ln_head", _torch_ln_head)
    X, H, D, Y = (torch.from_numpy(g[k]).to(_dev()) for k in ("X", "H", "D", "Y"))
    engine.HuberLoss(50.0)(net(X, H, D), Y).backward()
    return dict(net.named_parameters()), grads


@pytest.mark.parametrize("stack", [True, False])
def test_block_rounded_gradient_does_not_depend_on_the_head(stack, monkeypatch):
    """The tensors of _BLOCK_ROUNDED: with the HIP head and with torch's head they agree with each other far inside the
    bar (the head's rounding barely reaches them), and both miss the reference by the same per-entry amount."""
    from conftest import elementwise_violations
    for name, key in _BLOCK_ROUNDED:
        case = next(c for c in CASES if c[0] == name)
        hip, grads = _model_grads(case, stack)
        ref, _ = _model_grads(case, stack, monkeypatch)
        monkeypatch.undo()
        a, b = hip[key].grad.cpu(), ref[key].grad.cpu()
        assert rel_err(a, b) < 1e-5, key
        assert abs(elementwise_violations(a, grads[key], 1e-4, 1e-5) - elementwise_violations(b, grads[key], 1e-4, 1e-5)) < 2e-3


@pytest.mark.parametrize("stack", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[c[0][:-4] for c in CASES])
def test_long_horizon_model_matches_the_reference(case, stack):
    from ms_gat_amd import engine
    g, net, grads = _net(case)
    net.stack_components = stack
    X, H, D, Y = (torch.from_numpy(g[k]).to(_dev()) for k in ("X", "H", "D", "Y"))
    pred = net(X, H, D)
    loss = engine.HuberLoss(50.0)(pred, Y)
    loss.backward()
    what = f"{case[0][:-4]}{'' if stack else '_loop'}"
    assert_parity(pred.detach().cpu(), g["pred"], what, "pred")
    assert abs(float(loss.detach()) - float(g["loss"])) < TOL * abs(float(g["loss"]))
    checked = 0
    for name, p in net.named_parameters():
        if p.grad is None:
            continue
        if (case[0], name) in _BLOCK_ROUNDED:   # see _BLOCK_ROUNDED: the head's share is checked tightly below
            assert_parity(p.grad.cpu(), grads[name], what, name, floor_eps=1e-4)
        else:
            assert_parity(p.grad.cpu(), grads[name], what, name)
        checked += 1
    assert checked == len(grads)


def test_trainer_hip_graph_replay_matches_eager_at_24_outputs(tmp_path):
    from ms_gat_amd import data, engine, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], out_timesteps=24, batch_size=8, days=2)
    net = model.msgat72(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=24, use_te=True, adj=ds.adj)
    net.to(_dev())
    twin = copy.deepcopy(net)
    batches = [b for _, b in zip(range(4), ds.training)]
    assert batches[0][-1].shape[-1] == 24
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True)
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        assert np.isfinite(le) and abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    graphed.save(str(tmp_path / "ck.pkl"))
    ev = engine.Evaluator(copy.deepcopy(twin), 50.0, str(tmp_path / "ev"), str(tmp_path / "ck.pkl"))
    first = ev.eval(batches[:2], gpu_id=0)
    assert np.isfinite(first)
    assert abs(ev.eval(batches[:2], gpu_id=0) - first) < 1e-5 * abs(first)
