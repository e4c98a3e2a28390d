"""Learning-rate schedule, decoupled weight decay and the resumable trainer, without a GPU: hgn_lr_at (the host side of the ONE
inline function the device kernel compiles) against parallel.LRSchedule.at, the refusals of hgn_lr_at / hgn_adam_step_sched
(status codes before any launch), ops.adam_step_sched's layout checks, and the trainer's host logic on CPU tensors
(parallel.DataParallelTrainer with adam_fn=_torch_adam: the same arithmetic in torch at lr = schedule.at(step)), single process
and gloo world 2, and state_dict() / load_state_dict().

Yardsticks.
* Formula: both sides are double arithmetic on the same formula, operation for operation, and differ by pow's last bits: 4 * 2^-52
  relative.  The C ABI holds lr, lr_min and decay_rate as float, so the schedules compared with it are given float32 numbers
  (LRSchedule.as_float32), as the Adam comparisons give both sides the float32 neighbours of the betas.
* Trainer: torch.optim.AdamW on a copy of the model, weight_decay per group (0 for the tensors the filter leaves out), lr set to
  schedule.at(t) before every step; tolerances of test_grad_clip_cpu.py's Adam comparison (1e-6 on m and v, rtol 2e-5 / atol 2e-6
  on the weights).
* Resume: the uninterrupted run, torch.equal."""
import ctypes as C
import os
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mgn_oracle as O
from tests import helpers as H
from tests.test_grad_clip_cpu import _batch, _flat_of, _small_problem
from tests.test_host_cpu import _OracleNet

INVALID = -1
EPS64 = 2.0 ** -52
BETAS = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in (0.9, 0.999))
WD = 0.01
WARMUP, DECAY = 100, 1000


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _schedules():
    from hgn_amd.parallel import LRSchedule
    return {'constant': LRSchedule(1e-3).as_float32(),
            'warm-up only': LRSchedule(1e-3, warmup_steps=WARMUP).as_float32(),
            'decay only': LRSchedule(1e-3, decay_steps=DECAY, decay_rate=0.1, lr_min=1e-5).as_float32(),
            'both': LRSchedule(1e-3, warmup_steps=WARMUP, decay_steps=DECAY, decay_rate=0.5, lr_min=1e-5).as_float32()}


def _lr_at(struct, t):
    from hgn_amd import _lib
    out = C.c_double(-1.0)
    assert _lib.lib().hgn_lr_at(C.byref(struct), t, C.byref(out)) == 0, _lib.lib().hgn_last_error()
    return out.value


# ---------------------------------------------------------------------------------------------------------------
# 1. the formula
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['constant', 'warm-up only', 'decay only', 'both'])
def test_hgn_lr_at_is_lrschedule_at(kind):
    s = _schedules()[kind]
    st = s.as_struct(0.0)
    assert (st.lr, st.lr_min, st.decay_rate) == (s.lr, s.lr_min, s.decay_rate)          # float32 numbers: nothing is lost in the struct
    for t in (1, 2, WARMUP - 1, WARMUP, WARMUP + 1, WARMUP + DECAY, 10 ** 6, 2 ** 31 - 1):
        got, want = _lr_at(st, t), s.at(t)
        print(f'{kind} t={t}: hgn_lr_at {got!r}  LRSchedule.at {want!r}  err / 2^-52 = {abs(got - want) / (EPS64 * want):.2f}')
        assert abs(got - want) <= 4 * EPS64 * want
        assert s.lr_min <= want <= s.lr or (s.warmup_steps and t < s.warmup_steps)


def test_known_answers():
    from hgn_amd.parallel import LRSchedule
    sch = _schedules()
    const = sch['constant']
    for t in (1, 2, 99, 10 ** 6, 2 ** 31 - 1):
        assert const.at(t) == const.lr and _lr_at(const.as_struct(), t) == const.lr          # exactly
    # a constant schedule above a floor is still the constant: no (lr_min + (lr - lr_min)) on the way
    assert LRSchedule(const.lr, lr_min=_f32(3e-4)).at(7) == const.lr
    # the warm-up ends AT warmup_steps: the undamped value there, a linear ramp before
    both, decay_only = sch['both'], LRSchedule(sch['both'].lr, 0, DECAY, sch['both'].decay_rate, sch['both'].lr_min)
    assert both.at(WARMUP) == both.lr                                   # no decay yet: max(0, t - warmup) = 0
    assert sch['warm-up only'].at(WARMUP) == const.lr and sch['warm-up only'].at(WARMUP + 5) == const.lr
    assert sch['warm-up only'].at(WARMUP // 4) == (WARMUP // 4 / WARMUP) * const.lr
    assert both.at(WARMUP + DECAY) == decay_only.at(DECAY)              # the decay counts from the end of the warm-up
    half = both.lr_min + (both.lr - both.lr_min) * 0.5
    assert abs(both.at(WARMUP + DECAY) - half) <= 4 * EPS64 * half      # one decay period: the rate (0.5) once
    assert abs(both.at(2 ** 31 - 1) - both.lr_min) <= 4 * EPS64 * both.lr_min
    # the MeshGraphNets setting, in the doubles as given
    mgn = LRSchedule(1e-4 + 1e-6, decay_steps=5 * 10 ** 6, decay_rate=0.1, lr_min=1e-6)
    assert abs(mgn.at(5 * 10 ** 6) - 1.1e-5) <= 1e-12 * 1.1e-5
    assert abs(mgn.at(1) - (1e-4 + 1e-6)) <= 1e-6 * 1e-4 and mgn.at(10 ** 9) < 1.0000001e-6


def test_lrschedule_is_an_immutable_value_that_pickles_and_validates():
    import pickle
    from hgn_amd.parallel import LRSchedule
    s = LRSchedule(1e-3, 10, 20, 0.5, 1e-5)
    again = pickle.loads(pickle.dumps(s))
    assert again == s and hash(again) == hash(s) and again is not s and again.at(17) == s.at(17)
    assert s != LRSchedule(1e-3, 10, 20, 0.5, 1e-6)
    with pytest.raises(AttributeError):
        s.lr = 1.0
    with pytest.raises(AttributeError):
        del s.lr
    for bad in (dict(lr=-1e-3), dict(lr=float('nan')), dict(lr=float('inf')), dict(lr=1e-3, lr_min=-1e-9), dict(lr=1e-3, lr_min=2e-3),
                dict(lr=1e-3, lr_min=float('nan')), dict(lr=1e-3, warmup_steps=-1), dict(lr=1e-3, decay_steps=-1),
                dict(lr=1e-3, warmup_steps=1.5), dict(lr=1e-3, decay_steps=2 ** 31), dict(lr=1e-3, decay_rate=0.0),
                dict(lr=1e-3, decay_rate=1.5), dict(lr=1e-3, decay_rate=float('nan'))):
        with pytest.raises(ValueError):
            LRSchedule(**bad)
    for bad_wd in (-0.1, float('nan'), float('inf'), 1000.0):          # 1e-3 * 1000 >= 1
        with pytest.raises(ValueError):
            LRSchedule(1e-3).as_struct(bad_wd)
    with pytest.raises(ValueError):
        s.at(0)
    st = s.as_struct(0.25)
    assert (st.warmup_steps, st.decay_steps, st.weight_decay) == (10, 20, 0.25)


# ---------------------------------------------------------------------------------------------------------------
# 2. the ABI's refusals
# ---------------------------------------------------------------------------------------------------------------
def test_abi_refusals_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    assert 'hgn_lr_at' in _lib.EXPORTS and 'hgn_adam_step_sched' in _lib.EXPORTS
    nan, inf = float('nan'), float('inf')
    good = dict(lr=1e-3, lr_min=1e-5, warmup_steps=10, decay_steps=100, decay_rate=0.5, weight_decay=0.01)
    bad_schedules = {'negative lr': dict(lr=-1e-3, lr_min=0.0), 'nan lr': dict(lr=nan), 'inf lr': dict(lr=inf),
                     'lr_min < 0': dict(lr_min=-1e-9), 'lr_min > lr': dict(lr_min=2e-3), 'nan lr_min': dict(lr_min=nan),
                     'warmup < 0': dict(warmup_steps=-1), 'decay_steps < 0': dict(decay_steps=-1),
                     'decay_rate 0': dict(decay_rate=0.0), 'decay_rate < 0': dict(decay_rate=-0.5), 'decay_rate > 1': dict(decay_rate=1.0001),
                     'nan decay_rate': dict(decay_rate=nan), 'weight_decay < 0': dict(weight_decay=-0.01), 'nan weight_decay': dict(weight_decay=nan),
                     'inf weight_decay': dict(weight_decay=inf), 'lr * weight_decay = 1': dict(lr=0.5, weight_decay=2.0),
                     'lr * weight_decay > 1': dict(lr=0.5, weight_decay=4.0)}
    # pointers are never dereferenced by a refused call: any aligned non-null value stands for a device buffer
    p, g, m, v, cnt, coef, mask, lr_out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000

    def step(sched, n=100, **kw):
        a = dict(p=p, g=g, m=m, v=v, step=cnt, count=1)
        a.update(kw)
        s = C.byref(sched) if sched is not None else None
        return lib.hgn_adam_step_sched(a['p'], a['g'], a['m'], a['v'], n, s, 0.9, 0.999, 1e-8, a['step'], a['count'], 1.0, coef, mask,
                                       lr_out, None)
    out = C.c_double(0.0)
    for what, kw in bad_schedules.items():
        st = _lib.AdamSched(**dict(good, **kw))
        for count in (0, 1):
            assert step(st, count=count) == INVALID, what
            assert b'hgn_adam_step_sched' in lib.hgn_last_error(), what
        assert lib.hgn_lr_at(C.byref(st), 5, C.byref(out)) == INVALID, what
        assert b'hgn_lr_at' in lib.hgn_last_error(), what
    ok = _lib.AdamSched(**good)
    for what, kw in {'null p': dict(p=None), 'null g': dict(g=None), 'null m': dict(m=None), 'null v': dict(v=None),
                     'null step_dev': dict(step=None)}.items():
        assert step(ok, **kw) == INVALID, what
        assert b'hgn_adam_step_sched' in lib.hgn_last_error(), what
    assert step(None) == INVALID and b'hgn_adam_step_sched' in lib.hgn_last_error()
    assert step(ok, n=-1) == INVALID and b'hgn_adam_step_sched' in lib.hgn_last_error()
    # n == 0 is valid; without count_step nothing is launched at all (so this runs without a GPU)
    assert step(ok, n=0, count=0) == 0
    assert step(ok, n=0, count=0, p=None, g=None, m=None, v=None) == 0
    # hgn_lr_at: null pointers, steps before the first
    assert lib.hgn_lr_at(None, 5, C.byref(out)) == INVALID and b'hgn_lr_at' in lib.hgn_last_error()
    assert lib.hgn_lr_at(C.byref(ok), 5, None) == INVALID and b'hgn_lr_at' in lib.hgn_last_error()
    for t in (0, -1, -2 ** 31):
        assert lib.hgn_lr_at(C.byref(ok), t, C.byref(out)) == INVALID and b'hgn_lr_at' in lib.hgn_last_error()
    assert lib.hgn_lr_at(C.byref(ok), 1, C.byref(out)) == 0 and out.value > 0


def test_ops_adam_step_sched_refuses_cpu_tensors_and_wrong_layouts():
    from hgn_amd import _lib, ops, parallel
    st = parallel.LRSchedule(1e-3).as_struct(0.0)
    z, cnt = torch.zeros(8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.HgnError):
        ops.adam_step_sched(z, z, z, z, st, 0.9, 0.999, 1e-8, cnt, count_step=True)
    with pytest.raises(_lib.HgnError):
        ops.adam_step_sched(z.double(), z, z, z, st, 0.9, 0.999, 1e-8, cnt, count_step=True)
    with pytest.raises(_lib.HgnError):
        ops.adam_step_sched(torch.zeros(8, 2)[:, 0], z, z, z, st, 0.9, 0.999, 1e-8, cnt, count_step=True)
    with pytest.raises(TypeError):
        ops.adam_step_sched(z, z, z, z, st, 0.9, 0.999, 1e-8, cnt)          # count_step has no default: the caller says who counts


# ---------------------------------------------------------------------------------------------------------------
# 3. the trainer on CPU tensors
# ---------------------------------------------------------------------------------------------------------------
LR = 1e-2
STEPS = 5


def _schedule():
    from hgn_amd.parallel import LRSchedule
    return LRSchedule(LR, warmup_steps=2, decay_steps=2, decay_rate=0.5, lr_min=1e-3)      # warm-up, peak, then two decay periods in 5 steps


def _reference(order, steps=STEPS, weight_decay=WD, seed=3):
    """torch.optim.AdamW, decay on the tensors with dim() >= 2 only, lr = schedule.at(t) before every step -> flat p, m, v."""
    graphs, shapes, targets, masks = _small_problem()
    model = _OracleNet(O.init_state_dict_like(shapes, seed))
    ps = list(model.parameters())
    opt = torch.optim.AdamW([{'params': [p for p in ps if p.dim() >= 2], 'weight_decay': weight_decay},
                             {'params': [p for p in ps if p.dim() < 2], 'weight_decay': 0.0}], lr=LR, betas=BETAS)
    g, target, mask = _batch(graphs, targets, masks, order)
    sched = _schedule()
    for t in range(1, steps + 1):
        for group in opt.param_groups:
            group['lr'] = sched.at(t)
        opt.zero_grad()
        O.masked_mse(model(g), target, mask).backward()
        opt.step()
    return _flat_of(ps), _flat_of([opt.state[p]['exp_avg'] for p in ps]), _flat_of([opt.state[p]['exp_avg_sq'] for p in ps])


def _trainer(seed=3, shapes=None, **kw):
    from hgn_amd import parallel
    if shapes is None:
        shapes = _small_problem()[1]
    model = _OracleNet(O.init_state_dict_like(shapes, seed))
    kw.setdefault('lr_schedule', _schedule())
    kw.setdefault('weight_decay', WD)
    return parallel.DataParallelTrainer(model, lr=LR, betas=BETAS, adam_fn=parallel._torch_adam, **kw)


def test_cpu_trainer_follows_the_schedule_and_decays_like_adamw():
    graphs, shapes, targets, masks = _small_problem()
    order = [0, 1, 2, 3]
    want_p, want_m, want_v = _reference(order)
    tr = _trainer()
    assert tr.t_dev is not None and tr.lr_dev.shape == (1,) and tr.lr_dev.dtype == torch.float32 and tr.grad_stats is None
    mask8 = tr.decay_mask
    assert mask8 is not None and mask8.dtype == torch.uint8 and mask8.numel() == tr.fp.numel
    for p, off in zip(tr.fp.params, tr.fp.offsets):                      # the default filter: weights, not biases / LayerNorm vectors
        assert bool((mask8[off:off + p.numel()] == (1 if p.dim() >= 2 else 0)).all())
    assert 0 < int(mask8.sum()) < tr.fp.numel
    g, target, mask = _batch(graphs, targets, masks, order)
    sched = _schedule()
    for t in range(1, STEPS + 1):
        tr.step(g, target, mask)
        assert int(tr.t_dev) == t == tr.t and float(tr.lr_dev) == _f32(sched.at(t))
    errs = {'m': H.rel_err(tr.m, want_m), 'v': H.rel_err(tr.v, want_v)}
    print('cpu schedule + decay after 5 steps: rel_err', errs, 'max |dp|', float((tr.fp.flat - want_p).abs().max()))
    assert errs['m'] <= 1e-6 and errs['v'] <= 1e-6
    torch.testing.assert_close(tr.fp.flat, want_p, rtol=2e-5, atol=2e-6)
    # and both did something: without the decay, and at the constant rate, the weights are elsewhere
    free_p, _, _ = _reference(order, weight_decay=0.0)
    assert float((free_p - want_p).abs().max()) > 1e-4
    const = _trainer(lr_schedule=None)
    for _ in range(STEPS):
        const.step(g, target, mask)
    assert float(const.lr_dev) == _f32(LR) and float((const.fp.flat - want_p).abs().max()) > 1e-3


def test_cpu_trainer_arguments():
    from hgn_amd import parallel
    shapes = _small_problem()[1]
    plain = parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), lr=LR, adam_fn=parallel._torch_adam)
    assert plain.t_dev is None and plain.lr_dev is None and plain.decay_mask is None and plain.sched is None
    every = _trainer(decay_filter=lambda name, p: True)
    assert every.decay_mask is None and every.weight_decay == WD           # every tensor decays: no mask is passed
    names = []
    one = _trainer(decay_filter=lambda name, p: (names.append(name), name == 'ps.0')[1])
    assert names == [n for n, _ in one.model.named_parameters()]
    assert int(one.decay_mask.sum()) == one.fp.params[0].numel() and bool(one.decay_mask[:one.fp.params[0].numel()].all())
    only_schedule = _trainer(weight_decay=0.0)
    assert only_schedule.decay_mask is None and only_schedule.lr_dev is not None
    with pytest.raises(ValueError, match='weight_decay'):
        parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), adam_fn=lambda *a, **k: None, weight_decay=WD)
    with pytest.raises(ValueError):
        _trainer(weight_decay=-1.0)
    with pytest.raises(ValueError):
        _trainer(weight_decay=1.0 / LR)                                     # lr * weight_decay >= 1
    with pytest.raises(ValueError):
        _trainer(lr_schedule=0.5)


def test_cpu_trainer_skipped_step_neither_decays_nor_moves_the_rate():
    graphs, shapes, targets, masks = _small_problem()
    g, target, mask = _batch(graphs, targets, masks, [0, 1, 2, 3])
    tr = _trainer(skip_nonfinite=True)
    tr.step(g, target, mask)
    before = [x.clone() for x in (tr.fp.flat, tr.m, tr.v, tr.t_dev, tr.lr_dev)]
    tr.fp.zero_grad()
    tr.fp.grad.fill_(0.25)
    tr.fp.grad[7] = float('nan')
    tr.fp.count.fill_(1.0)
    tr.reduce_and_update(torch.zeros(1), 1)
    for a, b in zip(before, (tr.fp.flat, tr.m, tr.v, tr.t_dev, tr.lr_dev)):
        assert torch.equal(a, b)
    assert int(tr.skipped_dev) == 1
    tr.step(g, target, mask)
    assert int(tr.t_dev) == 2 and float(tr.lr_dev) == _f32(_schedule().at(2))


def _dp_worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hgn_amd import parallel
    torch.set_num_threads(1)
    graphs, shapes, targets, masks = _small_problem()
    tr = _trainer(seed=3 + rank)                                        # different per rank: the broadcast fixes it
    g, target, mask = _batch(graphs, targets, masks, parallel.shard_indices(4, rank, world))
    rates = []
    for _ in range(STEPS):
        tr.step(g, target, mask)
        rates.append(tr.lr_dev.clone())
    mine = torch.cat([tr.fp.flat, tr.m, tr.v] + rates)
    theirs = mine.clone()
    dist.broadcast(theirs, src=0)
    assert torch.equal(mine, theirs), 'replicas diverged'
    if rank == 0:
        torch.save({'flat': tr.fp.flat.clone(), 'm': tr.m.clone(), 'v': tr.v.clone(), 'rates': torch.cat(rates)}, out)
    dist.destroy_process_group()


def test_two_ranks_follow_the_schedule_alike_and_like_adamw(tmp_path):
    from hgn_amd import parallel
    order = parallel.shard_indices(4, 0, 2) + parallel.shard_indices(4, 1, 2)
    port = 23500 + (os.getpid() % 2000)
    out = str(tmp_path / 'sched.pt')
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    res = torch.load(out)
    want_p, want_m, want_v = _reference(order)
    sched = _schedule()
    assert res['rates'].tolist() == [_f32(sched.at(t)) for t in range(1, STEPS + 1)]
    torch.testing.assert_close(res['flat'], want_p, rtol=2e-5, atol=2e-6)
    assert H.rel_err(res['m'], want_m) <= 2e-5 and H.rel_err(res['v'], want_v) <= 2e-5      # (the bound of the two-rank clip test)


# ---------------------------------------------------------------------------------------------------------------
# 4. resume
# ---------------------------------------------------------------------------------------------------------------
def test_cpu_resume_continues_bit_for_bit(tmp_path):
    graphs, shapes, targets, masks = _small_problem()
    g, target, mask = _batch(graphs, targets, masks, [0, 1, 2, 3])
    kw = dict(max_grad_norm=0.05, skip_nonfinite=True)
    straight = _trainer(**kw)
    for _ in range(6):
        straight.step(g, target, mask)
    first = _trainer(**kw)
    for _ in range(3):
        first.step(g, target, mask)
    state = first.state_dict()
    assert set(state) == {'m', 'v', 't', 't_dev', 'skipped_dev', 'grad_stats', 'lr_dev', 'hyper_parameters', 'layout'}
    assert all(not x.is_cuda for x in state.values() if isinstance(x, torch.Tensor)) and state['t'] == 3
    assert state['layout']['names'] == [n for n, _ in first.model.named_parameters()]
    assert state['layout']['offsets'] == first.fp.offsets and state['layout']['sizes'] == [p.numel() for p in first.fp.params]
    hp = state['hyper_parameters']
    assert hp['lr'] == LR and hp['betas'] == list(BETAS) and hp['weight_decay'] == WD and hp['max_grad_norm'] == 0.05
    assert hp['skip_nonfinite'] is True and hp['lr_schedule'] == _schedule().fields() and hp['eps'] == 1e-8
    path = str(tmp_path / 'ckpt.pt')
    torch.save({'model': first.model.state_dict(), 'trainer': state}, path)
    first.step(g, target, mask)                                      # the saved state is a copy: the run it came from goes on
    assert state['t'] == 3 and int(state['t_dev']) == 3
    ckpt = torch.load(path, weights_only=True)
    second = _trainer(seed=99, **kw)                                 # a fresh model (other weights) and trainer
    m_addr, flat_addr = second.m.data_ptr(), second.fp.flat.data_ptr()
    second.model.load_state_dict(ckpt['model'])
    with warnings.catch_warnings():
        warnings.simplefilter('error')                               # the same hyper-parameters: nothing to warn about
        second.load_state_dict(ckpt['trainer'])
    assert second.m.data_ptr() == m_addr and second.fp.flat.data_ptr() == flat_addr          # copied in place
    assert second.t == 3 and int(second.t_dev) == 3
    for _ in range(3):
        second.step(g, target, mask)
    for name in ('m', 'v', 't_dev', 'skipped_dev', 'grad_stats', 'lr_dev'):
        assert torch.equal(getattr(second, name), getattr(straight, name)), name
    assert torch.equal(second.fp.flat, straight.fp.flat) and second.t == straight.t == 6
    assert 0.0 < float(straight.grad_stats[1]) < 1.0                 # clipping was active in the run


def test_load_state_dict_refuses_another_layout_and_warns_about_hyper_parameters():
    graphs, shapes, targets, masks = _small_problem()
    g, target, mask = _batch(graphs, targets, masks, [0, 1, 2, 3])
    tr = _trainer()
    tr.step(g, target, mask)
    state = tr.state_dict()
    deeper = O.param_shapes('none', 'sum', 2, ['mesh_edges'], 5, {'mesh_edges': 7}, 0, 3, 16)      # one more block
    other = _trainer(shapes=deeper)
    m0 = other.m.clone()
    with pytest.raises(ValueError, match='laid out differently'):
        other.load_state_dict(state)
    assert torch.equal(other.m, m0) and other.t == 0                 # refused before anything was copied
    with pytest.raises(ValueError, match='laid out differently'):
        tr.load_state_dict(other.state_dict())
    changed = _trainer(weight_decay=0.02)
    flat0 = changed.fp.flat.clone()
    with pytest.warns(UserWarning, match='weight_decay'):
        changed.load_state_dict(state)
    assert changed.weight_decay == 0.02 and torch.equal(changed.m, tr.m) and changed.t == 1 and int(changed.t_dev) == 1
    assert torch.equal(changed.fp.flat, flat0)                       # the parameters are the model's business
    # a state saved by a trainer that counted on the host seeds the device counter of one that counts there
    from hgn_amd import parallel
    host = parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), lr=LR, betas=BETAS, adam_fn=parallel._torch_adam)
    host.step(g, target, mask)
    host.step(g, target, mask)
    assert 't_dev' not in host.state_dict()
    with pytest.warns(UserWarning):
        tr.load_state_dict(host.state_dict())
    assert tr.t == 2 and int(tr.t_dev) == 2
