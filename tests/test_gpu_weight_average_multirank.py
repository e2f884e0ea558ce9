"""GPU: the averaged weights with TWO ranks on one MI355X (fresh child processes sharing cuda:0 over gloo, as in
tests/test_gpu_multirank.py).  The average comes out of the same launch as the update, after the one all-reduce, so both
ranks hold the same shadow bits -- and each rank's shadow is the float32 restatement driven by the parameters that rank
observed.  Shards are uneven: 7 = 4 + 3 samples."""
import os

import pytest
import torch

import weight_average_ref as ref
from test_gpu_guarded_multirank import _spawn
from test_gpu_multirank import _free_port, _join, _leave, _model_and_batches

pytestmark = pytest.mark.gpu

STEPS = 4
DECAY = 0.5


def _worker(rank, world, port, out_dir):
    from ms_gat_amd import engine
    net, batches = _model_and_batches((7,) * STEPS)
    _join(rank, world, port)
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"r{rank}"), hip_graph=False, ema_decay=DECAY)
    opt = tr.optimizer
    opt._build()
    start = [p.detach().cpu().numpy().copy() for p in opt._params]
    first_shadow = [e.cpu().numpy().copy() for e in opt._shadow_views()]
    observed, active = [], []
    for k, batch in enumerate(batches):                     # one data-parallel step per call: read the parameters after it
        tr.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
        observed.append([p.detach().cpu().numpy().copy() for p in opt._params])
        active.append(tuple(opt._last_active))
    torch.save(dict(start=start, first_shadow=first_shadow, observed=observed, active=active,
                    shadow=[e.cpu().numpy().copy() for e in opt._shadow_views()], steps=opt._dev_steps.tolist()),
               os.path.join(out_dir, f"rank{rank}.pt"))
    _leave(world)


def test_two_ranks_hold_the_same_shadow_bits_and_each_the_restatement_of_what_it_observed(tmp_path):
    out = str(tmp_path)
    _spawn(_worker, (2, _free_port(), out), 2)
    ranks = [torch.load(os.path.join(out, f"rank{r}.pt"), weights_only=False) for r in (0, 1)]
    for r in ranks:
        assert all(ref.same_bits(a, b) for a, b in zip(r["first_shadow"], r["start"]))        # it starts at the parameters
        assert len(r["observed"]) == STEPS and set(r["steps"]) == {float(STEPS)}
        want = [s.copy() for s in r["start"]]
        for k, (params, active) in enumerate(zip(r["observed"], r["active"])):
            assert all(active)
            want = [ref.average_f32(e, w, DECAY, k + 1) for e, w in zip(want, params)]
        for i, (got, w) in enumerate(zip(r["shadow"], want)):
            assert ref.same_bits(got, w), i
        assert not all(ref.same_bits(e, w) for e, w in zip(r["shadow"], r["observed"][-1]))   # the average lags the weights
    assert all(ref.same_bits(a, b) for a, b in zip(ranks[0]["shadow"], ranks[1]["shadow"]))
    assert all(ref.same_bits(a, b) for a, b in zip(ranks[0]["observed"][-1], ranks[1]["observed"][-1]))
