"""CPU: the long-horizon fixtures (T_out > 16, tests/golden/make_golden_horizon.py) reproduce through the dense
restatement of the model in float64, and the data module makes targets of any horizon.

The head (msgat.py:153,159) is Conv2d(T_in -> T_out, [1, C]); the time embedding (msgat.py:187) gates [R,N,T_out]."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from horizon_fixtures import CASES, DILATIONS, load
from oracle import dense_torch


def _dense_model(state, X, H, D, R, T, To):
    """msgat.py:202-205 restated op by op: per component two MEAM blocks, LayerNorm over T, the head, the gate."""
    B, N = X.shape[0], X.shape[3]
    gate = (state["te.h_ebd.weight"][H] + state["te.d_ebd.weight"][D]).view(B, R, N, To)
    out = 0
    for r in range(R):
        x = X[:, r]
        for layer, dil in enumerate(DILATIONS):
            pre = f"tpcs.{r}.tgacns.{layer}."
            x = dense_torch.meam_dense(x, state["adj"], {k[len(pre):]: v for k, v in state.items() if k.startswith(pre)},
                                       dil)
        x = F.layer_norm(x, [T], state[f"tpcs.{r}.ln.weight"], state[f"tpcs.{r}.ln.bias"], 1e-5)
        y = F.conv2d(x.transpose(1, 3), state[f"tpcs.{r}.fc.weight"], state[f"tpcs.{r}.fc.bias"])
        out = out + y[..., 0].transpose(1, 2) * gate[:, r]
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0][:-4] for c in CASES])
def test_long_horizon_fixture_reproduces_in_float64(case):
    name, _, R, _, T, To, _ = case
    g, state, grads = load(name)
    state = {k: v.double().requires_grad_(k != "adj") for k, v in state.items()}
    X, Y = torch.from_numpy(g["X"]).double(), torch.from_numpy(g["Y"]).double()
    H, D = torch.from_numpy(g["H"]), torch.from_numpy(g["D"])
    pred = _dense_model(state, X, H, D, R, T, To)
    assert pred.shape == (X.shape[0], X.shape[3], To)
    assert rel_err(pred.detach(), g["pred"]) < 2e-5
    loss = dense_torch.huber(pred, Y, 50.0)
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    loss.backward()
    assert set(grads) == {k for k in state if k != "adj"}
    for k, want in grads.items():
        assert rel_err(state[k].grad, want) < 1e-4, k


def test_make_loaders_yields_targets_of_a_long_horizon():
    from ms_gat_amd import data
    ds = data.SyntheticPEMS(n_nodes=7, n_edges=8, n_channels=2, in_hours=[1, 2], out_timesteps=24, batch_size=4, days=3)
    for loader in (ds.training, ds.validation, ds.evaluation):
        batch = next(iter(loader))
        X, Y = batch[0], batch[-1]
        assert X.shape[1:] == (2, 2, 7, 12)
        assert Y.shape == (4, 7, 24)
