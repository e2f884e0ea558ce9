"""GPU: the kernels that re-create the softmax map with a score chain of their own (the adjacency's gradient, dense,
per edge and per sample; the map read-out; the gradient at the map) at the numerical edges the attention core is held
to in test_gpu_parity.py: large scores, saturated scores, magnitudes far from one, and lse formed by the split-operand
dense passes.  Their S comes from one kernel and their lse from another (the forward's dense pass); large scores are
where a mismatch between the two would show.

Through ops.gacn, N = 90 (100 for the magnitudes), B = 2, T = 12, widths 3 -> 24 (aggregate first, Cu = 3) and 72 -> 24
(project first, Cu = 24), against the float64 run of oracle/dense_torch.py's op sequence with the adjacency as a leaf
and `att` kept.  The map's gradient is taken from a loss on the map alone, so that nothing but these kernels feeds it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_parity, record_err, rel_err
from oracle import dense_torch

import ms_gat_amd
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "score_edges"
TOL = 1e-4
T = 12
WIDTHS = [(3, 24), (72, 24)]
FORMS = ["dense", "values", "sets", "softmax", "softmax_grad"]


def _problem(C, Co, N, B, seed, x_scale=1.0, cq=1.0, cg=1.0):
    """test_gpu_parity.random_problem's distributions, with a learned adjacency per sample and a cotangent for the map.
    Signals of magnitude x_scale * cq with Wg scaled by 1 / cq^2 (the scores stay what they are), cotangents of cg."""
    rng = np.random.default_rng(seed)
    p = dict(x=rng.standard_normal((B, C, N, T)) * (x_scale * cq), Wg=rng.standard_normal((T, T)) * (1.0 / T) ** 0.5 / (cq * cq),
             alpha=rng.uniform(-C ** -0.5, C ** -0.5, C), W=rng.standard_normal((Co, C)) * (2.0 / (Co + C)) ** 0.5,
             dz=rng.standard_normal((B, Co, N, T)) * cg, dP=rng.standard_normal((B, N, N)) * cg)
    p["adj"] = np.stack([ms_gat_amd.synthetic_adjacency(N, N + 6 + 3 * b, seed + b).numpy() * rng.uniform(0.25, 1.5, (N, N))
                         for b in range(B)])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


def _dense_ops(x, adj, Wg, alpha, W):
    """dense_torch.gacn_dense, op for op, with `att` kept (the reference forms it at attention.py:34)"""
    q = torch.einsum("bcnt,c->bnt", x, alpha)
    att = torch.softmax(torch.matmul(torch.matmul(q, Wg), q.transpose(1, 2)), dim=-1)
    y = torch.einsum("bnm,bcmt->bcnt", att * adj, x)
    return torch.matmul(y.transpose(1, -1), W.t()).transpose(1, -1), att, q


def _reference(p, form, dtype):
    """The tensors `_ours` returns for `form`, by autograd on the CPU in `dtype` (fp32: the reference's own op sequence)."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in p.items()}
    adj = (t["adj"] if form == "sets" else t["adj"][0]).requires_grad_(True)
    x, Wg, alpha = (t[k].requires_grad_(True) for k in ("x", "Wg", "alpha"))
    z, att, _ = _dense_ops(x, adj, Wg, alpha, t["W"])
    if dtype == torch.float32:
        assert torch.equal(z, dense_torch.gacn_dense(x, adj, Wg, alpha, t["W"]))
    if form == "softmax":
        return {"att": att.detach()}
    if form == "softmax_grad":
        (att * t["dP"]).sum().backward()
        return {"att": att.detach(), "dx": x.grad, "dWg": Wg.grad, "dalpha": alpha.grad}
    z.backward(t["dz"])
    return {"dadj": adj.grad} if form == "dense" else {"dval": adj.grad[_stored(p, form)]}


def _stored(p, form):
    """index of the stored entries, in the order of the values: the non-zeros, row-major"""
    return np.nonzero(p["adj"] if form == "sets" else p["adj"][0])


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _ours(p, form):
    x = _dev(p["x"]).requires_grad_(True)
    alpha, Wg, W = (_dev(p[k]).requires_grad_(True) for k in ("alpha", "Wg", "W"))
    N = p["adj"].shape[-1]
    if form == "softmax":
        with torch.no_grad():
            _, w = ops.gacn(x, alpha, Wg, W, _dev(p["adj"][0]), need_weights=True, weights="softmax")
        return {"att": w}
    if form == "softmax_grad":
        _, w = ops.gacn(x, alpha, Wg, W, _dev(p["adj"][0]), need_weights=True, weights="softmax_grad")
        (w * _dev(p["dP"])).sum().backward()
        return {"att": w.detach(), "dx": x.grad, "dWg": Wg.grad, "dalpha": alpha.grad}
    if form == "dense":
        leaf = a = _dev(p["adj"][0]).requires_grad_(True)
    elif form == "values":
        r, c = _stored(p, form)
        leaf = torch.nn.Parameter(_dev(p["adj"][0][r, c]))
        crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))])
        a = torch.sparse_csr_tensor(_dev(crow, torch.int64), _dev(c, torch.int64), leaf, (N, N))
    else:
        v, i, j = _stored(p, form)
        leaf = torch.nn.Parameter(_dev(p["adj"][v, i, j]))
        a = torch.sparse_coo_tensor(_dev(np.stack([v, i, j]), torch.int64), leaf, p["adj"].shape, is_coalesced=True)
    ops.gacn(x, alpha, Wg, W, a).backward(_dev(p["dz"]))
    return {"dadj" if form == "dense" else "dval": leaf.grad}


def _finite(got):
    torch.cuda.synchronize()
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k


# ---- large scores --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,Co", WIDTHS)
def test_large_scores_against_the_fp32_op_sequence(C, Co, form):
    """Scores up to ~1e2, rows partly saturated.  The rule of test_large_scores_need_the_running_max: no tensor may be
    further from float64 than 3x the distance of the reference's own fp32 op sequence (or the usual 1e-4)."""
    p = _problem(C, Co, 90, 2, seed=5 + C, x_scale=6.0)
    got, want, ref32 = _ours(p, form), _reference(p, form, torch.float64), _reference(p, form, torch.float32)
    _finite(got)
    for k in want:
        bar = max(TOL, 3.0 * rel_err(ref32[k], want[k]))
        e = rel_err(got[k], want[k])
        record_err(WHAT, f"large C{C}_Co{Co} {form}:{k}", e, bar)
        assert e < bar, (k, e, bar)


# ---- saturated scores ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,Co", WIDTHS)
def test_saturated_scores_stay_finite_and_accurate(C, Co, form):
    """Scores ~1e3: every softmax row is one-hot in fp32.  dadj, dval and the map are O(1) and meet the usual bar.  The
    outputs of the map's gradient are differences of terms that cancel, dS = P dP - r P; they are held to 1e-5 of the
    magnitude of those terms, |P dP| + |r| P, carried through the products that follow (the float64 oracle supplies
    it), as test_fully_saturated_softmax_stays_finite_and_accurate holds dWg and dalpha."""
    p = _problem(C, Co, 90, 2, seed=5 + C, x_scale=25.0)
    got, want = _ours(p, form), _reference(p, form, torch.float64)
    _finite(got)
    key = f"saturated C{C}_Co{Co} {form}"
    for k in ("dadj", "dval", "att"):
        if k in want:
            assert_parity(got[k], want[k], WHAT, f"{key}:{k}")
    if form != "softmax_grad":
        return
    t = {k: torch.from_numpy(v).double() for k, v in p.items()}
    _, P, q = _dense_ops(t["x"], t["adj"][0], t["Wg"], t["alpha"], t["W"])
    X = P * t["dP"]
    dS = X.abs() + X.sum(-1, keepdim=True).abs() * P
    kW, Wa = (q @ t["Wg"]).abs(), t["Wg"].abs()
    dkW = dS @ q.abs()
    dq = dS.transpose(1, 2) @ kW + dkW @ Wa.T
    scale = dict(dWg=torch.einsum("bnt,bns->ts", q.abs(), dkW).max(), dalpha=torch.einsum("bnt,bcnt->c", dq, t["x"].abs()).max(),
                 dx=(t["alpha"].abs()[None, :, None, None] * dq[:, None]).max())
    for k, s in scale.items():
        err = float((got[k].detach().cpu().double() - want[k]).abs().max())
        record_err(WHAT, f"{key}:{k} / cancelling terms", err / float(s), 1e-5)
        assert err < 1e-5 * float(s), (k, err, float(s))


# ---- magnitudes far from one ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cq,cg", [(1e-6, 1e-8), (1e3, 1e5), (3e7, 1e-3)])
@pytest.mark.parametrize("C,Co", WIDTHS)
def test_magnitudes_far_from_one(C, Co, cq, cg, form):
    """The (cq, cg) pairs of test_payload_magnitudes_far_from_one at N = 100: signals of magnitude cq with Wg / cq^2, so
    that scores and attention stay what they are, cotangents of magnitude cg; against float64 at the usual bar."""
    p = _problem(C, Co, 100, 2, seed=4100 + C, cq=cq, cg=cg)
    got, want = _ours(p, form), _reference(p, form, torch.float64)
    _finite(got)
    for k in want:
        assert_parity(got[k], want[k], WHAT, f"magnitudes C{C}_Co{Co} q~{cq:g} g~{cg:g} {form}:{k}")


# ---- lse from the split-operand dense passes ---------------------------------------------------------------------------

def test_split_operand_dense_passes_child_run():
    """MSGAT_DENSE_SPLIT=1 (read once per process) makes the dense passes of every T = 12 shape form lse from operands
    split into bf16 / fp16 terms; the kernels here keep their fp32 score chain.  One fresh child process repeats the
    large-score cases that way: the two must still agree where the scores are large."""
    env = dict(os.environ, MSGAT_DENSE_SPLIT="1")
    env.pop("MSGAT_PARITY_LOG", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "large_scores"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout
