"""An engine outlives the trainer bound to it: ``DataParallelTrainer`` keeps a zero-copy view of the engine's flat gradient buffer
and launches on the engine, so ``Engine.close()`` while a trainer is bound takes effect when the trainer is released -- the
view never dangles and a micro-step the trainer still owes (an unfinished accumulation window) runs instead of failing on a
destroyed handle."""
import gc

import numpy as np
import pytest

from densereg_amd.engine import Engine
from densereg_amd.parallel import DataParallelTrainer


class _Handle:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


class _HostEngine(Engine):
    """The lifetime logic of Engine on the host: no device, no library."""

    def __init__(self):
        self.h = _Handle()
        self.calls = []

    def flat_view(self, which):
        return np.zeros(4, np.float32)

    def zero_grad(self):
        self.calls.append('zero')


def test_close_waits_for_the_bound_trainer():
    eng = _HostEngine()
    eng.close()
    assert eng.h.closed == 1                                    # nobody bound: closes at once
    eng = _HostEngine()
    a, b = DataParallelTrainer(eng, sub_batch=5), DataParallelTrainer(eng, sub_batch=5)
    eng.close()
    assert eng.h.closed == 0                                    # two trainers alias its gradient buffer
    del a
    gc.collect()
    assert eng.h.closed == 0
    del b
    gc.collect()
    assert eng.h.closed == 1                                    # the last one let go
    # a trainer released before close() leaves nothing pending
    eng = _HostEngine()
    t = DataParallelTrainer(eng, sub_batch=5)
    del t
    gc.collect()
    assert eng.h.closed == 0
    eng.close()
    assert eng.h.closed == 1


@pytest.mark.gpu
def test_micro_step_owed_after_close_runs_on_the_gpu(gpu):
    """A window left unfinished when the engine's owner closes it (the benchmark's profiled pass with step counts that are no
    multiple of the window does this): the owed micro-step runs, the gradient view stays valid, and the handle is destroyed when the
    trainer goes."""
    import torch
    from densereg_amd.data.synthetic import make_crops
    from densereg_amd.model.hourglass_um_crop_tiny import _random_params
    B, J = 8, 14
    eng = Engine(1, 32, J, 128, 3, B, 0, True, pipeline=1)          # one slot: the flat view is the gradient sum itself
    eng.load_params(_random_params(eng))
    dm, poses, cfgs, coms, _ = make_crops(B, 'nyu', seed=5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(eng.device)
    d_pose, d_cfg, d_com = t(poses), t(cfgs), t(coms)
    d_dm = eng.norm_dm(t(dm), d_com)
    tr = DataParallelTrainer(eng, dataset='nyu', sub_batch=3)
    l0 = tr.micro_step(d_dm, d_pose, d_cfg, d_com, seed=0, dropout_mode=0)
    g1 = tr.flat_grad.clone()
    eng.close()
    l1 = tr.micro_step(d_dm, d_pose, d_cfg, d_com, seed=1, dropout_mode=0)
    g2 = tr.flat_grad.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(l0).all() and torch.isfinite(l1).all() and torch.isfinite(g2).all()
    assert float((g2 - g1).abs().max()) > 0                     # the second micro-step accumulated into the live buffer
    h = eng.h
    assert h._h
    del tr
    gc.collect()
    assert not h._h                                             # destroyed with the last holder
