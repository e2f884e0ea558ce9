"""GPU: an adjacency whose values change between calls is read at its CURRENT values (graph.graph_of / batched_graph_of).

Whoever uses the adjacency's gradient writes the adjacency, and the next forward has to see what was written.  Every cell
runs the op on the adjacency object, applies a writer to it, runs forward and backward again on the same object and
compares z, dx, the parameter gradients and dadj with the float64 autograd of oracle/dense_torch.py at the values the
tensor holds NOW (conftest.assert_parity: 1e-4, per entry).

Forms: dense [N,N], [1,N,N], [B,N,N], [R*B,N,N]; sparse CSR and an `edge_adjacency` weight as controls (their values are
read where they sit).  Writers: an in-place op under no_grad; torch.optim.Adam; FlatAdam (its plain, guarded and
averaged update kernels, which write through the parameters' addresses); swap_averaged / averaged_parameters;
`.data`; replays of a captured forward + backward with a write between them; a captured step with the optimizer inside.

Teeth, a condition on the inputs checked against the reference alone: the float64 results at the old and at the new
values differ by rel_err > 1e-2 in z and in dadj, so a stale read misses the 1e-4 bar by two orders of magnitude.
The loss is 0.5 |z - target|^2 (target: the `dz` of `_case`), not a fixed output gradient: z is linear in the adjacency,
so with a fixed dz the gradient dadj = softmax * (dz . x) would not depend on the adjacency's values at all and a stale
read could never show in it; with dz = z - target it does.

Shapes: N = 64, T = 12, B = 2, the smallest at which the three modes still differ: AGG_FIRST with the in-kernel tail
(3 -> 24), PROJ_FIRST (72 -> 24), plain attention (3 -> 0); the stacked forms with R = 3 relations of 72 -> 24.
"""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_parity, rel_err
from oracle import dense_torch
from test_gpu_adjacency_grad import _case, _learned_adjacency, _oracle_dadj

import ms_gat_amd
from ms_gat_amd import _lib, engine, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

N, T, B, R_STACKED = 64, 12, 2, 3
MODES = {"agg_first": (3, 24), "proj_first": (72, 24), "attention": (3, 0)}
DENSE = [(mode, form) for form in ("nn", "1nn") for mode in MODES] + [("proj_first", "bnn"), ("proj_first", "rbnn")]
CONTROLS = [(mode, form) for form in ("csr", "edge") for mode in MODES]
KEYS = ("z", "dx", "dalpha", "dWg", "dW", "dadj")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _factors(shape, seed):
    """a factor per entry, none inside [0.8, 1.25]"""
    rng = np.random.default_rng(seed)
    f = np.where(rng.random(shape) < 0.5, rng.uniform(0.3, 0.8, shape), rng.uniform(1.25, 3.0, shape)).astype(np.float32)
    assert not ((f > 0.8) & (f < 1.25)).any()
    return _dev(f)


class _Cell:
    """One (mode, form): inputs, parameters and the adjacency as ONE leaf on the device -- the dense tensor, or the stored
    values of the sparse controls -- plus the float64 reference at any values of it."""

    def __init__(self, mode, form, seed=0, full=False):
        C, O = MODES[mode]
        self.what = f"coherence {mode} {form}"
        self.form, self.R = form, R_STACKED if form in ("bnn", "rbnn") else 1
        self.case = _case(B, C, O, N, T, seed=seed + C + O, R=self.R)
        V = {"1nn": 1, "bnn": B, "rbnn": self.R * B}.get(form)
        adj = _learned_adjacency(N, seed=seed + 17, V=V)
        if full:        # no zero entry: an optimizer step cannot grow the pattern
            adj = adj + np.random.default_rng(seed + 3).uniform(0.02, 0.1, adj.shape).astype(np.float32)
        x, dz, Wg, alpha, W = self.case
        self.x, self.dz = _dev(x).requires_grad_(True), _dev(dz)
        self.alpha, self.Wg = _dev(alpha).requires_grad_(True), _dev(Wg).requires_grad_(True)
        self.W = None if W is None else _dev(W).requires_grad_(True)
        self.out = torch.empty((self.R * B, O or C, N, T), device=DEV)
        if form in ("csr", "edge"):
            self.rows, self.cols = np.nonzero(adj)
            crow = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=N))])
            self.crow, self.col = _dev(crow, torch.int64), _dev(self.cols, torch.int64)
            self.leaf = torch.nn.Parameter(_dev(adj[self.rows, self.cols]))
        else:
            self.leaf = torch.nn.Parameter(_dev(adj))

    def adjacency(self):
        """what the op is handed: the dense leaf itself, every time the same object; the sparse controls on the leaf"""
        if self.form == "csr":
            return torch.sparse_csr_tensor(self.crow, self.col, self.leaf, (N, N))
        if self.form == "edge":
            return ops.edge_adjacency(self.crow, self.col, self.leaf)
        return self.leaf

    def values(self):
        """the dense adjacency the leaf holds now (float32 host array in the shape the reference takes)"""
        v = self.leaf.detach().cpu().numpy()
        if self.form in ("csr", "edge"):
            a = np.zeros((N, N), dtype=np.float32)
            a[self.rows, self.cols] = v
            return a
        return v.copy()

    def leaves(self):
        return [t for t in (self.x, self.alpha, self.Wg, self.W, self.leaf) if t is not None]

    def step(self):
        """forward + backward of the loss 0.5 |z - target|^2 on the adjacency object; z goes to `out`, the gradients to
        the leaves' .grad (zeroed in place first, so that a captured step keeps writing the same tensors)"""
        for t in self.leaves():
            if t.grad is not None:
                t.grad.zero_()
        z = ops.gacn(self.x, self.alpha, self.Wg, self.W, self.adjacency())
        self.out.copy_(z.detach())
        (0.5 * (z - self.dz).square().sum()).backward()

    def outputs(self):
        torch.cuda.synchronize()
        got = dict(z=self.out, dx=self.x.grad, dalpha=self.alpha.grad, dWg=self.Wg.grad, dadj=self.leaf.grad)
        if self.W is not None:
            got["dW"] = self.W.grad
        return {k: v.detach().clone() for k, v in got.items()}

    def run(self):
        self.step()
        return self.outputs()

    def oracle(self, adj):
        """float64 autograd of gacn_dense / graph_attention_dense at the dense adjacency `adj`, relation by relation"""
        x, dz, Wg, alpha, W = self.case
        f = lambda t: torch.from_numpy(t).to(DEV, torch.float64).requires_grad_(True)  # noqa: E731
        a, xt, Wgt, alt = f(adj), f(x), f(Wg), f(alpha)
        Wt = None if W is None else f(W)
        outs = []
        for r in range(self.R):
            xr = xt[r * B:(r + 1) * B]
            ar = a[r * B:(r + 1) * B] if self.form == "rbnn" else a
            if Wt is None:
                outs.append(dense_torch.graph_attention_dense(xr, ar, Wgt[r], alt[r]))
            else:
                outs.append(dense_torch.gacn_dense(xr, ar, Wgt[r], alt[r], Wt[r]))
        z = torch.cat(outs)
        (0.5 * (z - torch.from_numpy(dz).to(DEV, torch.float64)).square().sum()).backward()
        want = dict(z=z.detach(), dx=xt.grad, dalpha=alt.grad, dWg=Wgt.grad, dadj=a.grad)
        if Wt is not None:
            want["dW"] = Wt.grad
        want = {k: v.cpu().numpy() for k, v in want.items()}
        if self.form in ("csr", "edge"):
            want["dadj"] = want["dadj"][self.rows, self.cols]
        return want

    def check(self, got, want, writer):
        for k in KEYS:
            if k in want:
                assert_parity(got[k], want[k], f"{self.what} {writer}", k)


def _assert_teeth(old, new, what):
    """the reference at the old values against the reference at the new ones: a stale read is 100x over the bar"""
    for k in ("z", "dadj"):
        e = rel_err(old[k], new[k])
        print(f"teeth {what} {k}: {e:.3e}")
        assert e > 1e-2, f"{what}: the write moves {k} by {e:.3e} only, a stale read would pass"


def test_the_reference_here_is_the_one_of_the_adjacency_gradient_tests():
    """`_oracle_dadj` of test_gpu_adjacency_grad.py, handed the output gradient z - target of this file's loss (rounded
    to float32 on the way in, hence 1e-6 and not equality)"""
    cell = _Cell("proj_first", "rbnn")
    adj = cell.values()
    want = cell.oracle(adj)
    x, target, Wg, alpha, W = cell.case
    dz = (want["z"] - target).astype(np.float32)
    assert rel_err(_oracle_dadj(x, dz, Wg, alpha, W, adj, R=cell.R).cpu().numpy(), want["dadj"]) < 1e-6


# ---- eager writers ---------------------------------------------------------------------------------------------------

def _write(cell, writer):
    leaf = cell.leaf
    if writer == "inplace":
        with torch.no_grad():
            leaf.mul_(_factors(tuple(leaf.shape), 5))
    elif writer == "data":
        version = leaf._version
        leaf.data.mul_(_factors(tuple(leaf.shape), 6))
        assert leaf._version == version
    elif writer == "adam":
        torch.optim.Adam([leaf], lr=0.05).step()
    else:
        raise AssertionError(writer)


@pytest.mark.parametrize("writer", ["inplace", "adam", "data"])
@pytest.mark.parametrize("mode,form", DENSE + CONTROLS)
def test_eager_writer_is_seen_by_the_next_call(mode, form, writer):
    """torch.optim.Adam on a sparse-start dense adjacency turns every zero into an edge (the gradient is dense off the
    edges): the pattern grows, and the next call must carry the N^2 edges."""
    cell = _Cell(mode, form)
    cell.run()
    old = cell.oracle(cell.values())
    zeros = int((cell.values() == 0).sum())
    _write(cell, writer)
    if writer == "adam" and form not in ("csr", "edge"):
        assert zeros > 0 and int((cell.values() == 0).sum()) == 0
    got = cell.run()
    new = cell.oracle(cell.values())
    _assert_teeth(old, new, f"{cell.what} {writer}")
    cell.check(got, new, writer)


FLAT_ADAM = {"plain": {}, "guarded": {"max_grad_norm": 1.0}, "averaged": {"ema_decay": 0.9}}


@pytest.mark.parametrize("variant", list(FLAT_ADAM))
@pytest.mark.parametrize("mode,form", DENSE + CONTROLS)
def test_flat_adam_steps_are_seen_by_the_next_call(mode, form, variant):
    """FlatAdam's three update kernels (msgat_adam_step, _guarded, _averaged) write the parameter through its address:
    no version counter moves.  Three steps on the gradients of a real backward, every one checked."""
    cell = _Cell(mode, form)
    opt = engine.FlatAdam([cell.leaf], lr=0.05, **FLAT_ADAM[variant])
    cell.run()
    for k in range(3):
        old = cell.oracle(cell.values())
        version = cell.leaf._version
        opt.step()
        assert cell.leaf._version == version
        got = cell.run()
        new = cell.oracle(cell.values())
        _assert_teeth(old, new, f"{cell.what} flat_adam {variant} step {k}")
        cell.check(got, new, f"flat_adam_{variant}_{k}")


@pytest.mark.parametrize("mode,form", DENSE + CONTROLS)
def test_swapped_in_average_is_the_adjacency_read(mode, form):
    """swap_averaged() (msgat_param_swap) exchanges the parameter and its average in place: inside
    `averaged_parameters()` the averaged adjacency is the one read, after it the trained one."""
    cell = _Cell(mode, form)
    opt = engine.FlatAdam([cell.leaf], lr=0.05, ema_decay=0.9)
    cell.run()
    for _ in range(3):
        opt.step()
        cell.run()
    trained = cell.values()
    at_trained = cell.oracle(trained)
    with opt.averaged_parameters():
        averaged = cell.values()
        assert not np.array_equal(averaged, trained)
        got = cell.run()
        at_averaged = cell.oracle(averaged)
        _assert_teeth(at_trained, at_averaged, f"{cell.what} swap in")
        cell.check(got, at_averaged, "averaged_in")
    assert np.array_equal(cell.values(), trained)
    cell.check(cell.run(), at_trained, "averaged_out")
    opt.swap_averaged()                      # the bare call, and back
    assert np.array_equal(cell.values(), averaged)
    cell.check(cell.run(), at_averaged, "swap_averaged")
    opt.swap_averaged()
    cell.check(cell.run(), at_trained, "swap_averaged_back")


# ---- captured steps --------------------------------------------------------------------------------------------------

def _capture(cell, body):
    """PyTorch's recipe: warm-up on a side stream, then the capture of `body`"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


@pytest.mark.parametrize("mode,form", DENSE)
def test_replays_of_a_captured_step_reread_the_dense_adjacency(mode, form):
    """test_hip_graph_capture_rereads_the_weights for the dense forms: a replay runs no Python, so the refill of the
    graph's values has to be part of what was captured."""
    cell = _Cell(mode, form)
    cell.run()
    graph = _capture(cell, cell.step)
    for k in range(2):
        old = cell.oracle(cell.values())
        with torch.no_grad():
            cell.leaf.mul_(_factors(tuple(cell.leaf.shape), 30 + k))      # multiplicative: the pattern stays
        graph.replay()
        got = cell.outputs()
        new = cell.oracle(cell.values())
        _assert_teeth(old, new, f"{cell.what} replay {k}")
        cell.check(got, new, f"replay_{k}")


@pytest.mark.parametrize("mode,form", DENSE)
def test_captured_step_with_the_optimizer_inside(mode, form):
    """forward, backward and FlatAdam.step() in one captured step, on an adjacency without a zero entry (the pattern
    cannot grow): every replay reads what the replay before it wrote."""
    cell = _Cell(mode, form, full=True)
    opt = engine.FlatAdam([cell.leaf], lr=0.05)
    seen = []

    def body():
        if not torch.cuda.is_current_stream_capturing():
            seen.append(cell.values())
        cell.step()
        opt.step()

    cell.run()
    graph = _capture(cell, body)
    before = cell.oracle(seen[-1])           # the values of the last forward that ran any Python
    for k in range(3):
        values = cell.values()
        assert (values != 0).all()
        graph.replay()
        got = cell.outputs()
        want = cell.oracle(values)
        _assert_teeth(before, want, f"{cell.what} captured optimizer replay {k}")
        cell.check(got, want, f"captured_optimizer_{k}")
        before = want
    assert not np.array_equal(cell.values(), values)


def test_pattern_growth_under_capture_is_computed_or_refused_never_dropped():
    """A captured step with the optimizer inside, on a sparse-start dense [N,N] parameter.  The step makes every entry
    non-zero, and a captured step cannot rebuild the pattern.

    The outcome chosen: both, each where it is the truth.  The replay's own forward read the sparse values the pattern
    was built for, so its results are right; the next EAGER call finds the tensor outside the pattern, rebuilds it and
    matches float64 at the current values.  A further replay of the old capture then does drop edges (its pattern is the
    captured one), counts them on the device, and the next eager call on the tensor raises an MsgatError that names
    the adjacency's pattern.  Nothing is dropped silently."""
    cell = _Cell("proj_first", "nn")
    opt = engine.FlatAdam([cell.leaf], lr=0.05)
    start = cell.leaf.detach().clone()

    def body():
        cell.step()
        opt.step()

    cell.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                               # the optimizer's buffers exist; the adjacency is full now
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        cell.leaf.copy_(start)               # sparse again, and no eager forward before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    sparse = cell.values()
    assert (sparse == 0).sum() > N * N // 2
    graph.replay()
    cell.check(cell.outputs(), cell.oracle(sparse), "growth_replay")
    grown = cell.values()
    assert (grown != 0).all()
    at_grown = cell.oracle(grown)
    _assert_teeth(cell.oracle(sparse), at_grown, f"{cell.what} growth")
    cell.check(cell.run(), at_grown, "growth_next_eager")      # outcome 1: computed, on the rebuilt pattern
    graph.replay()                           # the old capture: its pattern lacks the new edges
    torch.cuda.synchronize()
    with pytest.raises(_lib.MsgatError, match="pattern"):      # outcome 2: refused at the next eager call
        cell.step()


# ---- the Trainer -----------------------------------------------------------------------------------------------------

class _LearnedGraphNet(torch.nn.Module):
    """GACN on a learned dense adjacency [N,N] with the MSGAT call signature; `full`: without a zero entry."""

    def __init__(self, n_nodes, full=True):
        super().__init__()
        torch.manual_seed(0)
        self.gacn = ms_gat_amd.GACN(1, 4, 12)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():                # GACN leaves its parameters uninitialised, like the reference's
            self.gacn.gatt.Wg.copy_(torch.randn(12, 12, generator=g) * 12 ** -0.5)
            self.gacn.gatt.alpha.copy_(torch.rand(1, generator=g) + 0.5)
            self.gacn.W.copy_(torch.randn(4, 1, generator=g))
        # small entries: the Trainer's Adam moves every entry by about its rate, 1e-3, per step, and a handful of steps
        # has to move the output by far more than the parity bar (asserted where the output is checked)
        adj = 0.05 * ms_gat_amd.synthetic_adjacency(n_nodes, 40, 0)
        if full:
            adj = adj + 0.002 + 0.008 * torch.rand(n_nodes, n_nodes, generator=g)
        self.adj = torch.nn.Parameter(adj)

    def forward(self, X, H, D, adj=None):
        z = self.gacn(X[:, 0], self.adj if adj is None else adj)      # [B,4,N,12]
        return 50.0 * z.mean(1)


def _assert_reads_the_trained_adjacency(m, a0, inputs, what):
    """the module's output on its adjacency object equals its output on a fresh copy of it (a fresh tensor: a fresh
    build), and -- teeth -- differs from its output at the start values `a0` by far more than the bar"""
    with torch.no_grad():
        got, want, stale = m(*inputs), m(*inputs, adj=m.adj.detach().clone()), m(*inputs, adj=a0.clone())
    moved = rel_err(stale.cpu(), want.cpu())
    print(f"teeth {what}: {moved:.3e}")
    assert moved > 1e-2, f"{what}: training moved the output by {moved:.3e} only, a stale read would pass"
    assert_parity(got, want.cpu().numpy(), what, "pred")


def _train_twins(tmp_path, full, **trainer):
    from ms_gat_amd import data
    ds = data.SyntheticPEMS(n_nodes=32, n_edges=40, n_channels=1, in_hours=[1], batch_size=8, days=2)
    net = _LearnedGraphNet(32, full).to(DEV)
    twin = copy.deepcopy(net)
    batches = [b for _, b in zip(range(4), ds.training)]
    inputs = tuple(t.to(DEV) for t in batches[0][:3])
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, **trainer)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True, **trainer)
    return net, twin, eager, graphed, batches, inputs


def _assert_twins_agree(net, twin, a0):
    """the bounds test_learned_edge_weights_train_captured_and_eager holds its twins to"""
    assert rel_err(twin.adj.detach().cpu(), net.adj.detach().cpu()) < 2e-2
    assert (net.adj.detach() - a0).abs().max() > 1e-4                          # the adjacency moves
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name


def test_learned_dense_adjacency_trains_captured_and_eager(tmp_path):
    """test_learned_edge_weights_train_captured_and_eager for a dense learned graph, held to its bounds; after each epoch
    the module's output equals its output on a fresh copy of the adjacency."""
    net, twin, eager, graphed, batches, inputs = _train_twins(tmp_path, full=True)
    assert (net.adj != 0).all()
    a0 = net.adj.detach().clone()
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
        for name, m in (("eager", net), ("captured", twin)):
            _assert_reads_the_trained_adjacency(m, a0, inputs, f"coherence trainer {name} epoch {epoch}")
    assert len(graphed._graphs) == 1
    _assert_twins_agree(net, twin, a0)


def test_sparse_start_adjacency_trains_captured_with_the_update_outside_the_step(tmp_path):
    """Gradient accumulation keeps the optimizer out of the captured step (as several ranks do), so the warm-up of the
    capture takes no update and a sparse-start graph is captured on its sparse pattern.  The first update fills every
    zero; the Trainer rebuilds the pattern right after it and captures anew, and nothing is dropped: same bounds, and
    the end of every epoch (which reads the captured steps' counters) raises nothing."""
    net, twin, eager, graphed, batches, inputs = _train_twins(tmp_path, full=False, accumulate_steps=2)
    a0 = net.adj.detach().clone()
    assert int((a0 == 0).sum()) > a0.numel() // 2
    for epoch in (1, 2):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
        assert graphed.last_stats["optimizer_steps"] == 2
        assert (twin.adj != 0).all() and (net.adj != 0).all()                  # one update: every entry an edge
        for name, m in (("eager", net), ("captured", twin)):
            _assert_reads_the_trained_adjacency(m, a0, inputs, f"coherence trainer accumulate {name} epoch {epoch}")
    assert len(graphed._graphs) == 1
    _assert_twins_agree(net, twin, a0)


def test_a_step_captured_before_the_pattern_grew_is_refused_at_the_end_of_its_epoch(tmp_path):
    """A validation step captured on the sparse pattern, then training (whose warm-up grows the pattern), then the old
    validation step again: its replays drop the new edges and no eager call on the tensor follows, so the end of
    run_epoch raises the MsgatError that names the pattern.  The Trainer drops its captured steps with it: the next
    epoch captures anew and is right."""
    net, twin, eager, graphed, batches, inputs = _train_twins(tmp_path, full=False)
    a0 = twin.adj.detach().clone()
    graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="validate")
    graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    assert (twin.adj != 0).all()
    with pytest.raises(_lib.MsgatError, match="pattern"):
        graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="validate")
    assert not graphed._graphs
    captured = graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="validate")
    eager.run_epoch(batches, gpu_id=0, epoch=1, mode="train")           # the eager twin: the same epoch, never captured
    assert abs(captured - eager.run_epoch(batches, gpu_id=0, epoch=1, mode="validate")) < 1e-4 * abs(captured)
    _assert_reads_the_trained_adjacency(twin, a0, inputs, "coherence trainer recaptured validation")
