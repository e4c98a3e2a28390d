"""CPU-side checks (no GPU) of activation checkpointing for unrolled training steps: `unrolled_training_step` and
`DataParallelTrainer.step_unrolled` carry ``checkpoint`` (default None) and refuse anything but None or a bool with TypeError before they
touch a tensor; ops.nested_backward exists, and a normaliser records the statistics a step normalised with and replays them without accumulating."""
import inspect

import pytest
import torch


def _bare(cls):
    """A system model with nothing in it: a refused call never reads it."""
    model = cls.__new__(cls)
    torch.nn.Module.__init__(model)
    return model


def test_both_signatures_carry_checkpoint_with_default_none():
    from hgn_amd import parallel, system_model
    for fn in (system_model.AbstractSystemModel.unrolled_training_step, parallel.DataParallelTrainer.step_unrolled):
        p = inspect.signature(fn).parameters
        assert 'checkpoint' in p and p['checkpoint'].default is None, fn
        assert list(p)[-1] == 'checkpoint'                               # behind the arguments of before: positional callers are untouched
    for cls in (system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel):
        assert 'unrolled_training_step' not in cls.__dict__ and '_unroll_step' not in cls.__dict__      # one body, in the base class


@pytest.mark.parametrize('bad', [3, 'yes', 1.0, 0, (True,)])
def test_anything_but_none_or_a_bool_is_a_type_error_before_any_work(bad):
    from hgn_amd import parallel, system_model

    class Untouchable(dict):
        def __getitem__(self, key):
            raise AssertionError('the windows were read')

    model = _bare(system_model.FlagModel)
    with pytest.raises(TypeError, match='checkpoint must be None, False or True'):
        model.unrolled_training_step(Untouchable(), 2, checkpoint=bad)
    net = torch.nn.Linear(3, 2)
    tr = parallel.DataParallelTrainer(net, lr=1e-3, adam_fn=parallel._torch_adam)
    before = tr.fp.flat.clone()
    tr.fp.grad.fill_(1.0)
    with pytest.raises(TypeError, match='checkpoint must be None, False or True'):
        tr.step_unrolled(model, Untouchable(), 2, checkpoint=bad)
    assert torch.equal(tr.fp.flat, before) and bool((tr.fp.grad == 1).all()) and tr.t == 0 and tr.overlap is True


def test_a_normaliser_records_what_it_normalised_with_and_replays_it_without_accumulating(monkeypatch):
    """The arithmetic is device kernels: stand-ins here.  `_accumulate` adds the batch's column sums, `normalize` returns the
    statistics it was handed."""
    from hgn_amd import features
    from hgn_amd.normalizer import Normalizer
    assert Normalizer.record is None and Normalizer.replay is None
    nz = Normalizer(3, 'n')
    assert 'record' not in nz.__dict__ and 'replay' not in nz.__dict__

    def accumulate(data):
        nz._acc_sum += data.sum(0)
        nz._acc_count += data.shape[0]
        nz._host_num_acc += 1
    nz._accumulate = accumulate
    monkeypatch.setattr(features, 'normalize', lambda x, s, q, n, eps, **kw: (s, q, n))
    x = torch.ones(4, 3)
    nz.record = []
    first = [nz(x)[0].clone(), nz(x)[0].clone()]                         # twice in one step, as the intra-cluster normaliser is
    nz(x, False)                                                         # a call that does not accumulate records nothing
    seen = nz.__dict__.pop('record')
    assert len(seen) == 2 and float(first[0][0]) == 4 and float(first[1][0]) == 8 and nz._host_num_acc == 2
    assert all(torch.equal(s[0], f) for s, f in zip(seen, first)) and seen[0][0] is not nz._acc_sum      # copies
    nz(x)                                                                # a later step accumulates again (the flag's node dynamics)
    assert float(nz._acc_sum[0]) == 12
    nz.replay = iter(seen)
    again = [nz(x)[0], nz(x)[0]]
    assert nz(x, False)[0] is nz._acc_sum                                # not accumulating: the statistics as they are
    assert nz(x)[0] is nz._acc_sum                                       # nothing recorded for a further call: as they are
    del nz.replay
    assert all(torch.equal(a, f) for a, f in zip(again, first))
    assert float(nz._acc_sum[0]) == 12 and nz._host_num_acc == 3         # the replay accumulated nothing


def test_nested_backward_is_public_in_ops():
    from hgn_amd import ops
    assert inspect.isclass(ops.nested_backward)
    c = ops.Context()
    assert ops.nested_backward(c).ctx is c and ops.nested_backward().ctx is ops.current()
