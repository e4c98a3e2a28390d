"""Learning-rate schedule, decoupled weight decay and resume on the GPU: hgn_adam_step_sched through ops.adam_step_sched,
parallel.DataParallelTrainer(lr_schedule=..., weight_decay=..., decay_filter=...) eagerly, captured, unrolled and on two ranks, and
state_dict() / load_state_dict() into a captured step.

Yardsticks.
* Constant schedule, no decay: ops.adam_step_dev / ops.adam_step_clip on copies, torch.equal (p, m, v, the counter).
* The rate: float32(LRSchedule.at(t)) on float32 fields.  The device's double differs from the host's by pow's last bits and is
  rounded to fp32 once: the same float or its neighbour, 2^-23 relative (ULP, as in test_gpu_grad_clip.py).
* AdamW: the update formula of include/hgn_mp.h evaluated in float64 on the same fp32 inputs, with an elementwise bound counted
  from the roundings (test_adamw_step_vs_fp64_statement's docstring).
* Trainer: autograd + clip_grad_norm_ + torch.optim.AdamW at lr = schedule.at(t), the tolerances of test_gpu_grad_clip.py's trainer
  test; captured steps and the resumed run: the eager / uninterrupted trainer, torch.equal; two ranks against one process:
  test_gpu_dp.py's figures."""
import functools
import os
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests.test_gpu_grad_clip import ULP, _check_moments, _gradient, _launches

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 3, 255, 256, 257, 65_541]
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8)
BETAS = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in (0.9, 0.999))      # (test_gpu_grad_clip.py: BETAS)
LR, WD = 1e-3, 0.01
GUARD = 3.0e7                                                    # what lies around the views: a store out of bounds would show


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _schedule(warmup=2, decay=4):
    """Warm-up, then decay by a half per `decay` steps towards a tenth of the base rate; float32 fields (what the device holds)."""
    from hgn_amd.parallel import LRSchedule
    return LRSchedule(LR, warmup_steps=warmup, decay_steps=decay, decay_rate=0.5, lr_min=0.1 * LR).as_float32()


def _view(host):
    """A device copy of `host` as a view 16 bytes into a larger buffer (the trainer's `grad_ext[4:]`) -> (view, buffer)."""
    n = host.numel()
    buf = torch.full((n + 8,), GUARD, dtype=torch.float32).cuda()
    buf[4:4 + n].copy_(host)
    return buf[4:4 + n], buf


def _guards_intact(*bufs):
    return all(bool((b[:4] == GUARD).all()) and bool((b[-4:] == GUARD).all()) for b in bufs)


@functools.lru_cache(maxsize=None)
def _state_host(n):
    """p with magnitudes log-uniform in 1e-6 .. 1e2 and random signs, non-zero m and v >= 0, on the host.  Never written."""
    gen = torch.Generator().manual_seed(500 + n)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)
    sign = torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0
    p = (mag * sign).to(torch.float32)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.randn(n, generator=gen) ** 2 * 0.01 + 1e-6
    return p, m, v


def _fresh_state(n):
    """-> ([p, m, v] as views 16 bytes into their buffers, the buffers)."""
    views, bufs = zip(*(_view(x) for x in _state_host(n)))
    return list(views), list(bufs)


def _counter(t):
    return torch.tensor([t], dtype=torch.int32, device='cuda')


# ---------------------------------------------------------------------------------------------------------------
# 1. constant schedule, no decay: the bits of the existing kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_constant_schedule_counting_the_step_has_the_bits_of_adam_step_dev(n):
    from hgn_amd import ops, parallel
    g = _gradient(n)[0]
    st = parallel.LRSchedule(_f32(LR)).as_struct(0.0)
    (pa, ma, va), bufs_a = _fresh_state(n)
    (pb, mb, vb), bufs_b = _fresh_state(n)
    assert n == 0 or pa.data_ptr() == bufs_a[0].data_ptr() + 16
    ta, tb = _counter(4), _counter(4)
    lr_out = torch.full((1,), -7.0, device='cuda')
    for k in range(3):
        ops.adam_step_sched(pa, g, ma, va, st, ADAM['b1'], ADAM['b2'], ADAM['eps'], ta, count_step=True, grad_scale=0.37, lr_out=lr_out)
        ops.adam_step_dev(pb, g, mb, vb, _f32(LR), ADAM['b1'], ADAM['b2'], ADAM['eps'], tb, grad_scale=0.37)
        assert int(ta) == int(tb) == 5 + k
        for x, y, name in zip((pa, ma, va), (pb, mb, vb), 'pmv'):
            assert torch.equal(x, y), (name, k)
    assert _guards_intact(*bufs_a)
    if n:
        assert float(lr_out) == _f32(LR) and not torch.equal(pa, _state_host(n)[0].cuda())
    else:
        assert float(lr_out) == -7.0                           # n == 0 launches the counter's increment and nothing else


@pytest.mark.parametrize('coef', [1.0, 0.37])
@pytest.mark.parametrize('n', SIZES)
def test_constant_schedule_with_a_coefficient_has_the_bits_of_adam_step_clip(n, coef):
    from hgn_amd import ops, parallel
    g = _gradient(n)[0]
    st = parallel.LRSchedule(_f32(LR)).as_struct(0.0)
    (pa, ma, va), bufs_a = _fresh_state(n)
    (pb, mb, vb), bufs_b = _fresh_state(n)
    ta, tb = _counter(4), _counter(4)
    c = torch.tensor([coef], dtype=torch.float32, device='cuda')
    for k in range(3):
        ta += 1; tb += 1                                       # what hgn_grad_clip_coef does in front of either kernel
        ops.adam_step_sched(pa, g, ma, va, st, ADAM['b1'], ADAM['b2'], ADAM['eps'], ta, count_step=False, grad_scale=0.81, coef=c)
        ops.adam_step_clip(pb, g, mb, vb, _f32(LR), ADAM['b1'], ADAM['b2'], ADAM['eps'], tb, c, grad_scale=0.81)
        assert int(ta) == int(tb) == 5 + k                     # read, not counted
        for x, y, name in zip((pa, ma, va), (pb, mb, vb), 'pmv'):
            assert torch.equal(x, y), (name, k)
    assert _guards_intact(*bufs_a)
    assert n == 0 or not torch.equal(ma, _state_host(n)[1].cuda())


@pytest.mark.parametrize('n', SIZES)
def test_a_zero_coefficient_stores_nothing(n):
    """A skipped step: p, m, v and lr_out keep their bits -- also with a moving schedule and weight decay, which would both show."""
    from hgn_amd import ops
    g = _gradient(n)[0]
    st = _schedule().as_struct(WD)
    (p, m, v), bufs = _fresh_state(n)
    t = _counter(5)
    lr_out = torch.full((1,), -7.0, device='cuda')
    zero = torch.zeros(1, device='cuda')
    mask = (torch.arange(n) % 3 == 0).to(torch.uint8).cuda()
    for dm in (None, mask):
        ops.adam_step_sched(p, g, m, v, st, ADAM['b1'], ADAM['b2'], ADAM['eps'], t, count_step=False, coef=zero, decay_mask=dm, lr_out=lr_out)
    for x, host in zip((p, m, v), _state_host(n)):
        assert torch.equal(x.cpu(), host)
    assert float(lr_out) == -7.0 and int(t) == 5 and _guards_intact(*bufs)


# ---------------------------------------------------------------------------------------------------------------
# 2. the rate on the device
# ---------------------------------------------------------------------------------------------------------------
def test_the_rate_on_the_device_follows_the_schedule():
    from hgn_amd import ops
    warmup, decay = 100, 1000
    sched = _schedule(warmup, decay)
    st = sched.as_struct(0.0)
    g = _gradient(3)[0]
    (p, m, v), _ = _fresh_state(3)
    lr_out = torch.zeros(1, device='cuda')
    seen = []
    for c in (0, 1, warmup - 1, warmup, warmup + decay, 10 ** 6):
        t = _counter(c)
        ops.adam_step_sched(p, g, m, v, st, ADAM['b1'], ADAM['b2'], ADAM['eps'], t, count_step=True, lr_out=lr_out)      # counts first: t = c + 1
        got, want = float(lr_out), _f32(sched.at(c + 1))
        print(f'counter {c} -> step {c + 1}: lr_out {got!r}  float32(LRSchedule.at) {want!r}  err / ulp {abs(got - want) / (ULP * want):.3f}')
        assert int(t) == c + 1 and abs(got - want) <= ULP * want
        seen.append(got)
        if c >= 1:                                             # and read as it is: the rate of step c
            t = _counter(c)
            ops.adam_step_sched(p, g, m, v, st, ADAM['b1'], ADAM['b2'], ADAM['eps'], t, count_step=False, lr_out=lr_out)
            assert int(t) == c and abs(float(lr_out) - _f32(sched.at(c))) <= ULP * _f32(sched.at(c))
    assert seen[0] == _f32((1.0 / warmup) * sched.lr) and seen[2] == sched.lr             # the ramp's first step; the peak at its end
    assert seen[2] > seen[3] > seen[4] > seen[5] >= sched.lr_min and abs(seen[5] - sched.lr_min) <= ULP * sched.lr_min


# ---------------------------------------------------------------------------------------------------------------
# 3. AdamW against its fp64 statement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True], ids=['no-mask', 'every-third'])
def test_adamw_step_vs_fp64_statement(masked):
    """One step at t = 7 from non-zero m, v under a schedule with warm-up and decay, weight_decay 0.01, against

        g' = g,  m' = b1 m + (1 - b1) g',  v' = b2 v + (1 - b2) g'^2,
        p' = p * dk - (lr_t / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps),    dk = 1 - lr_t * wd where the element decays, else 1

    in float64 on the same fp32 inputs (b1, b2, eps the floats the ABI receives; 1 - b is exact in fp32 for both betas; grad_scale 1).
    The bound, with u = 2^-24 (one fp32 rounding, relative to the rounded result, which is at most the sum of the operands'
    magnitudes) and every term kept to first order -- the factor (1 + 2^-10) covers the products of two errors:
      m': fl(b1 m), fl((1 - b1) g), fl(sum): each summand carries u of its own magnitude, the sum u of at most their total:
          |dm| <= 2u A_m,  A_m = |b1 m| + |(1 - b1) g|.
      v': fl(b2 v) u, fl(fl((1 - b2) g) g) 2u, fl(sum) u, all terms positive so the total IS v':  |dv| <= 3u v'.
      p': sqrt halves v's 3u and rounds (2.5u); bc2's own rounding to fp32 and the division: 4.5u; adding eps (positive): 5.5u on the
          denominator D.  The quotient q = m' / D: |dq| <= (|dm| + 6.5u |m'|) / D.  The step s = fl(lr_t) / fl(bc1), rounded: 3u.
          The decayed parameter fl(p fl(dk)): 2u |p dk| (none where the element does not decay, counted all the same).  The last
          operation is one fused multiply-add, rounded once: u |p'|.
          |dp| <= u (2 |p dk| + |p'| + s ((2 A_m + 6.5 |m'|) / D + 3 |q|)).
    No intermediate is subnormal (|g| >= 1e-12 gives (1 - b2) g^2 >= 1e-27; m, v, p are far above).
    lr_t itself is the host's double: the device's differs by pow's last bits (~2^-52), far inside the 3u granted to s.
    Masked-out elements equal the weight_decay = 0 result bit for bit."""
    from hgn_amd import ops
    n, t = 65_541, 7
    u = 2.0 ** -24
    slack = 1.0 + 2.0 ** -10
    g = _gradient(n)[0]
    sched = _schedule(warmup=3, decay=8)                        # t = 7: past the warm-up, four steps into the decay
    p0, m0, v0 = _state_host(n)
    mask_host = (torch.arange(n) % 3 == 0)
    mask = mask_host.to(torch.uint8).cuda() if masked else None
    b1, b2, eps = (_f32(ADAM[k]) for k in ('b1', 'b2', 'eps'))

    def run(weight_decay, decay_mask):
        (p, m, v), bufs = _fresh_state(n)
        step = _counter(t - 1)
        ops.adam_step_sched(p, g, m, v, sched.as_struct(weight_decay), ADAM['b1'], ADAM['b2'], ADAM['eps'], step, count_step=True,
                            decay_mask=decay_mask)
        assert int(step) == t and _guards_intact(*bufs)
        return p.cpu(), m.cpu(), v.cpu()
    p1, m1, v1 = run(WD, mask)
    lr_t = sched.at(t)
    assert sched.lr_min < lr_t < sched.lr
    g64, p64, m64, v64 = (x.double().cpu() for x in (g, p0, m0, v0))
    a_m = (b1 * m64).abs() + ((1.0 - b1) * g64).abs()
    m_ref = b1 * m64 + (1.0 - b1) * g64
    v_ref = b2 * v64 + (1.0 - b2) * g64 * g64
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    dk = torch.full_like(p64, 1.0 - lr_t * WD)
    if masked:
        dk[~mask_host] = 1.0
    denom = v_ref.sqrt() / bc2 ** 0.5 + eps
    q, s = m_ref / denom, lr_t / bc1
    p_ref = p64 * dk - s * q
    bounds = {'m': 2 * u * a_m * slack, 'v': 3 * u * v_ref * slack,
              'p': u * (2 * (p64 * dk).abs() + p_ref.abs() + s * ((2 * a_m + 6.5 * m_ref.abs()) / denom + 3 * q.abs())) * slack}
    misses = []
    for name, got, ref in (('m', m1, m_ref), ('v', v1, v_ref), ('p', p1, p_ref)):
        ratio = ((got.double() - ref).abs() / bounds[name]).max()
        print(f'adamw[{"mask" if masked else "all"}] {name}: worst error / bound {float(ratio):.3f}')
        if not float(ratio) <= 1.0:
            misses.append((name, float(ratio)))
    assert not misses, misses
    # the decay is there (an error of lr_t * wd |p| would be ~60 roundings of p), and only where the mask says
    p_free, m_free, v_free = run(0.0, None)
    assert torch.equal(m1, m_free) and torch.equal(v1, v_free)
    decays = mask_host if masked else torch.ones(n, dtype=torch.bool)
    big = p0.abs() > 1e-2                                       # (where the Adam step does not drown the parameter)
    assert bool((p1[decays & big] != p_free[decays & big]).all())
    assert torch.equal(p1[~decays], p_free[~decays]) and (not masked or int((~decays).sum()) == n - (n + 2) // 3)


def test_argument_checks_on_device_tensors():
    from hgn_amd import _lib, ops
    st = _schedule().as_struct(WD)
    z, t = torch.zeros(16, device='cuda'), _counter(1)
    one = torch.ones(1, device='cuda')
    args = (ADAM['b1'], ADAM['b2'], ADAM['eps'])
    for bad in (dict(p=z[:8]), dict(step=None), dict(step=torch.zeros(1, dtype=torch.int64, device='cuda')), dict(coef=torch.ones(2, device='cuda')),
                dict(coef=one.double()), dict(lr_out=torch.ones(2, device='cuda')), dict(lr_out=torch.ones(1)),
                dict(decay_mask=torch.ones(16, dtype=torch.bool, device='cuda')), dict(decay_mask=torch.ones(15, dtype=torch.uint8, device='cuda')),
                dict(decay_mask=torch.ones(32, dtype=torch.uint8, device='cuda')[::2]), dict(sched=(LR, 0.0))):
        a = dict(p=z, step=t, coef=one, lr_out=one.clone(), decay_mask=None, sched=st)
        a.update(bad)
        with pytest.raises(_lib.HgnError):
            ops.adam_step_sched(a['p'], z, z, z, a['sched'], *args, a['step'], count_step=True, coef=a['coef'], decay_mask=a['decay_mask'],
                                lr_out=a['lr_out'])
    bad_st = _lib.AdamSched(LR, 2 * LR, 0, 0, 1.0, 0.0)                  # the library's own refusal reaches the caller
    with pytest.raises(_lib.HgnError, match='hgn_adam_step_sched'):
        ops.adam_step_sched(z, z, z, z, bad_st, *args, t, count_step=True)
    assert int(t) == 1 and float(z.abs().max()) == 0.0                   # refused before any launch: nothing was counted


# ---------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_problem():
    """A 'none' / 'sum' model of two blocks on a 10 x 9 grid (the sizes of test_trainer_flat_gradients_and_adam_match_torch)."""
    import hgn_amd
    graph = synth.grid_graph(seed=7, nx=10, ny=9)
    sets = [e.name for e in graph.edge_sets]
    shapes = O.param_shapes('none', 'sum', 2, sets, 5, {n: 7 for n in sets}, 0, 3, 128)
    target = torch.randn(90, 3, generator=torch.Generator().manual_seed(2)).cuda()
    mask = torch.ones(90, dtype=torch.bool); mask[:3] = False
    g = hgn_amd.MultiGraph([x.cuda() for x in graph.node_features],
                           [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in graph.edge_sets])
    return g, target, mask.cuda(), (lambda seed=5: H.hip_model('none', 'sum', 2, sets, O.init_state_dict_like(shapes, seed=seed)))


@functools.lru_cache(maxsize=None)
def _first_norm():
    """The norm of the first step's gradient: max_grad_norm = half of it clips every early step."""
    from hgn_amd import parallel
    g, target, mask, make = _trainer_problem()
    probe = parallel.DataParallelTrainer(make(), lr=LR, max_grad_norm=0.0)
    probe.step(g, target, mask)
    return float(probe.grad_stats[0])


def _adamw(model, weight_decay=WD):
    ps = list(model.parameters())
    return torch.optim.AdamW([{'params': [p for p in ps if p.dim() >= 2], 'weight_decay': weight_decay},
                              {'params': [p for p in ps if p.dim() < 2], 'weight_decay': 0.0}], lr=LR, betas=BETAS)


def test_trainer_follows_the_schedule_clips_and_decays_like_torch_adamw():
    from hgn_amd import parallel
    g, target, mask, make = _trainer_problem()
    max_norm = 0.5 * _first_norm()
    sched = _schedule()
    ref = make()
    opt = _adamw(ref)
    flat = make()
    tr = parallel.DataParallelTrainer(flat, lr=LR, betas=BETAS, max_grad_norm=max_norm, lr_schedule=sched, weight_decay=WD)
    # a second trainer without decay, fed the first one's gradients: what the filter leaves out must not notice the decay
    other = parallel.DataParallelTrainer(make(), lr=LR, betas=BETAS, max_grad_norm=max_norm, lr_schedule=sched)
    assert tr.lr_dev.shape == (1,) and tr.lr_dev.is_cuda and tr.decay_mask is not None and other.decay_mask is None
    misses = []
    for step in range(3):
        for group in opt.param_groups:
            group['lr'] = sched.at(step + 1)
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(target[mask], ref(g)[mask])
        loss.backward()
        g_ref = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in ref.named_parameters()}
        norm_ref = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        coef_ref = min(1.0, max_norm / (norm_ref + 1e-6))
        opt.step()
        l2 = tr.step(g, target, mask)
        other.fp.zero_grad()
        other.fp.grad.copy_(tr.fp.grad)                                   # the gradient of the global mean, before the coefficient
        other.fp.count.fill_(1.0)
        other.reduce_and_update(torch.zeros(1, device='cuda'), 1)
        norm, coef = (float(x) for x in tr.grad_stats.cpu())
        print(f'trainer step {step}: lr {float(tr.lr_dev)!r} (schedule {sched.at(step + 1)!r})  norm {norm:.9g} (torch {norm_ref:.9g})  '
              f'coef {coef:.9g} (torch {coef_ref:.9g})')
        if step == 0:
            for k, p in flat.named_parameters():
                assert H.rel_err(p.grad, g_ref[k]) <= 2e-6 or float(g_ref[k].abs().max()) == 0, k
            assert 0.49 < coef < 0.51
        assert abs(float(l2) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
        assert abs(float(tr.lr_dev) - _f32(sched.at(step + 1))) <= ULP * sched.at(step + 1)
        if abs(coef - coef_ref) > 1e-5 * coef_ref:
            misses.append((f'coef at step {step}', coef, coef_ref))
        misses += _check_moments(f'trainer schedule + decay step {step}', tr, list(ref.named_parameters()), opt)
    assert not misses, misses
    assert int(tr.t_dev) == 3 == int(other.t_dev) and int(tr.skipped_dev) == 0
    assert abs(float(tr.lr_dev) - _f32(sched.at(3))) <= ULP * sched.at(3) and sched.at(3) < sched.at(2) == sched.lr
    for (k, p), (_, q) in zip(ref.named_parameters(), flat.named_parameters()):
        d = (q - p).detach().abs()
        assert int((d > 0.005 * 3 * LR).sum()) <= max(4, d.numel() // 50), k
        assert float(d.max()) <= 2 * 3 * LR, k
    # the filter: same gradients, same moments; vectors bit-equal with and without decay, matrices not
    assert torch.equal(tr.m, other.m) and torch.equal(tr.v, other.v) and torch.equal(tr.grad_stats, other.grad_stats)
    kinds = set()
    for (k, p), (_, q) in zip(flat.named_parameters(), other.model.named_parameters()):
        kinds.add(p.dim() >= 2)
        assert torch.equal(p, q) == (p.dim() < 2), k
    assert kinds == {True, False}


def test_unset_arguments_change_nothing(monkeypatch):
    """Without lr_schedule / weight_decay the step issues the calls and launches it issued before they existed (the counts
    test_gpu_grad_clip.py records: one Adam scope per step, two with clipping), and ops.adam_step_sched is never reached; with them
    ops.adam_step_sched stands where adam_step_dev / adam_step_clip stood and nothing else moves."""
    from hgn_amd import ops, parallel
    g, target, mask, make = _trainer_problem()
    calls = []
    for name in ('adam_step', 'adam_step_dev', 'grad_norm_clip', 'adam_step_clip', 'adam_step_sched'):
        monkeypatch.setattr(ops, name, (lambda *a, _f=getattr(ops, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1]))
    counts, flats = {}, {}
    forms = (('plain', {}), ('plain again', {}), ('device', dict(device_step=True)), ('clip', dict(max_grad_norm=1.0)),
             ('sched', dict(lr_schedule=_schedule())), ('decay', dict(weight_decay=WD)),
             ('clip + sched', dict(max_grad_norm=1.0, lr_schedule=_schedule(), weight_decay=WD)))
    for key, kw in forms:
        tr = parallel.DataParallelTrainer(make(), lr=LR, **kw)
        tr.step(g, target, mask)                                           # (the first step records the pack plan: count the second)
        del calls[:]
        _, counts[key] = _launches(lambda: tr.step(g, target, mask))
        counts[key]['calls'] = list(calls)
        flats[key] = tr.fp.flat.clone()
        assert (tr.lr_dev is None) == (key in ('plain', 'plain again', 'device', 'clip')) and (tr.t_dev is None) == key.startswith('plain')
    print('launch counts per step:', counts)
    assert counts['plain']['calls'] == ['adam_step'] == counts['plain again']['calls'] and counts['device']['calls'] == ['adam_step_dev']
    assert counts['clip']['calls'] == ['grad_norm_clip', 'adam_step_clip']
    assert counts['sched']['calls'] == ['adam_step_sched'] == counts['decay']['calls']
    assert counts['clip + sched']['calls'] == ['grad_norm_clip', 'adam_step_sched']
    assert [counts[k]['adam'] for k, _ in forms] == [1, 1, 1, 2, 1, 1, 2]
    rest = lambda c: {k: v for k, v in c.items() if k not in ('adam', 'calls')}
    assert all(rest(counts[k]) == rest(counts['plain']) for k, _ in forms)
    assert torch.equal(flats['plain'], flats['plain again'])
    # the constant schedule that weight_decay alone implies, with nothing to decay, is the device-step trainer bit for bit
    nothing = parallel.DataParallelTrainer(make(), lr=LR, weight_decay=WD, decay_filter=lambda name, p: False)
    for _ in range(2):
        nothing.step(g, target, mask)
    assert torch.equal(nothing.fp.flat, flats['device']) and not torch.equal(flats['decay'], flats['device'])


def _poison_once(model):
    """A forward hook that puts one inf into the gradient of the model's output, once -> the handle."""
    state = {'armed': True}

    def spoil(grad):
        if not state['armed']:
            return None
        state['armed'] = False
        grad = grad.clone()
        grad[5, 1] = float('inf')
        return grad

    def hook(module, inputs, output):
        if state['armed'] and output.requires_grad:
            output.register_hook(spoil)
        return None
    return model.register_forward_hook(hook)


def test_a_skipped_step_neither_decays_nor_moves_the_rate():
    from hgn_amd import parallel
    g, target, mask, make = _trainer_problem()
    sched = _schedule()
    tr = parallel.DataParallelTrainer(make(), lr=LR, skip_nonfinite=True, lr_schedule=sched, weight_decay=WD)
    tr.step(g, target, mask)
    tr.step(g, target, mask)
    before = [x.clone() for x in (tr.t_dev, tr.lr_dev, tr.fp.flat, tr.m, tr.v)]
    assert int(tr.t_dev) == 2 and int(tr.skipped_dev) == 0
    handle = _poison_once(tr.model)
    tr.step(g, target, mask)
    handle.remove()
    assert not bool(torch.isfinite(tr.fp.grad).all())                     # the poison reached the flat gradient
    for a, b, name in zip(before, (tr.t_dev, tr.lr_dev, tr.fp.flat, tr.m, tr.v), ('t_dev', 'lr_dev', 'p', 'm', 'v')):
        assert torch.equal(a, b), name
    assert int(tr.skipped_dev) == 1 and float(tr.grad_stats[1]) == 0.0 and tr.t == 3
    tr.step(g, target, mask)                                              # the next clean step is step 3 of the schedule
    assert int(tr.t_dev) == 3 and int(tr.skipped_dev) == 1 and not torch.equal(before[2], tr.fp.flat)
    assert abs(float(tr.lr_dev) - _f32(sched.at(3))) <= ULP * sched.at(3) and float(tr.lr_dev) != float(before[1])


# ---------------------------------------------------------------------------------------------------------------
# 5. captured steps
# ---------------------------------------------------------------------------------------------------------------
def _same_state(a, b):
    return {name: torch.equal(getattr(a, name), getattr(b, name)) for name in ('m', 'v', 't_dev', 'lr_dev')} | \
        {'flat': torch.equal(a.fp.flat, b.fp.flat)}


def test_captured_step_replays_a_rate_that_moves():
    from hgn_amd import graphs as hg, parallel
    g, target, mask, make = _trainer_problem()
    kw = dict(lr=LR, lr_schedule=_schedule(), weight_decay=WD)
    eager = parallel.DataParallelTrainer(make(), **kw)
    for _ in range(1 + 4):                                                  # the constructor's one warm-up step, then four replays
        eager.step(g, target, mask)
    tr = parallel.DataParallelTrainer(make(), **kw)
    step = hg.GraphedTrainStep(tr, g, target, mask, warmup=1)
    rates = []
    for _ in range(4):
        step()
        rates.append(float(tr.lr_dev))
    torch.cuda.synchronize()
    same = _same_state(tr, eager)
    print('captured step: lr_dev per replay', rates, same)
    assert step.captures == 1 and int(tr.t_dev) == 5 and all(same.values()), same
    sched = _schedule()
    assert rates[0] != rates[-1] and all(abs(r - _f32(sched.at(t))) <= ULP * sched.at(t) for r, t in zip(rates, (2, 3, 4, 5)))


def test_captured_shard_step_keeps_the_scheduled_update_behind_its_graph():
    from hgn_amd import graphs as hg, parallel
    g, target, mask, make = _trainer_problem()
    kw = dict(lr=LR, lr_schedule=_schedule(), weight_decay=WD, max_grad_norm=0.5 * _first_norm())
    eager = parallel.DataParallelTrainer(make(), **kw)
    for _ in range(4):
        eager.step(g, target, mask)
    tr = parallel.DataParallelTrainer(make(), **kw)
    step = hg.GraphedShardStep(tr, g, target, mask, warmup=1)               # (its warm-up runs forward + backward only)
    for _ in range(4):
        step()
    torch.cuda.synchronize()
    same = _same_state(tr, eager)
    assert int(tr.t_dev) == 4 and all(same.values()) and torch.equal(tr.grad_stats, eager.grad_stats), same


def test_step_unrolled_follows_the_schedule():
    """FlagModel (the warm model of test_gpu_unrolled_training.py) on a 6 x 5 mesh, W = 2 windows, n_steps = 2."""
    from hgn_amd import parallel
    from tests import test_gpu_unrolled_training as UT
    frames = [[synth.flag_frame(seed=300 + 10 * w + t, nx=6, ny=5) for t in range(2)] for w in range(2)]
    names = UT._state_names('flag') + UT.PER_STEP['flag'] + ('node_type',)
    win = {name: torch.stack([torch.stack([f[name] for f in row]) for row in frames]).cuda() for name in names}
    win['cells'], win['mesh_pos'] = frames[0][0]['cells'].cuda(), frames[0][0]['mesh_pos'].cuda()
    assert win['mesh_pos'].shape[0] == 30
    model = UT._model('flag')
    sched = _schedule()
    tr = parallel.DataParallelTrainer(model.learned_model, lr=LR, lr_schedule=sched, weight_decay=WD)
    before = tr.fp.flat.clone()
    for call in range(3):
        tr.step_unrolled(model, win, 2, through_state=True)
        got = float(tr.lr_dev)
        assert int(tr.t_dev) == call + 1 and abs(got - _f32(sched.at(call + 1))) <= ULP * sched.at(call + 1)
        assert not torch.equal(before, tr.fp.flat)
        before = tr.fp.flat.clone()
    assert bool(torch.isfinite(tr.fp.flat).all())


# ---------------------------------------------------------------------------------------------------------------
# 6. two ranks
# ---------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out, max_norm):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hgn_amd import parallel
    from tests import test_gpu_dp as DP
    gs, shapes, targets, masks = DP._problem()
    model = H.hip_model('none', 'sum', DP.LAYERS, ['mesh_edges'], O.init_state_dict_like(shapes, 11 + rank))      # the broadcast fixes it
    mine = parallel.shard_indices(DP.N_GRAPHS, rank, world)
    g = DP._to_dev(synth.batch([gs[i] for i in mine]))
    target = torch.cat([targets[i] for i in mine]).cuda()
    mask = torch.cat([masks[i] for i in mine]).cuda()
    with torch.no_grad():
        model(g)
    tr = parallel.DataParallelTrainer(model, lr=DP.LR, max_grad_norm=max_norm, lr_schedule=_schedule(), weight_decay=WD)
    losses, stats, grad1 = [], [], None
    for i in range(DP.STEPS):
        losses.append(tr.step(g, target, mask))
        stats.append(torch.cat([tr.grad_stats, tr.lr_dev]))
        if i == 0:
            grad1 = tr.fp.grad.clone()
    torch.cuda.synchronize()
    total = torch.stack(losses).cpu()
    dist.all_reduce(total)
    state = torch.cat([tr.fp.flat, tr.m, tr.v] + stats).cpu()
    theirs = state.clone()
    dist.broadcast(theirs, src=0)
    assert torch.equal(state, theirs), 'replicas (or their rates) differ'
    if rank == 0:
        torch.save({'flat': tr.fp.flat.cpu(), 'grad1': grad1.cpu(), 'losses': total, 'stats': torch.stack(stats).cpu()}, out)
    dist.destroy_process_group()


def test_two_ranks_stay_bit_equal_and_match_one_process(tmp_path):
    from hgn_amd import parallel
    from tests import test_gpu_dp as DP
    gs, shapes, targets, masks = DP._problem()
    order = parallel.shard_indices(DP.N_GRAPHS, 0, 2) + parallel.shard_indices(DP.N_GRAPHS, 1, 2)
    g = DP._to_dev(synth.batch([gs[i] for i in order]))
    target = torch.cat([targets[i] for i in order]).cuda()
    mask = torch.cat([masks[i] for i in order]).cuda()
    sd = O.init_state_dict_like(shapes, 11)

    def single(max_norm):
        tr = parallel.DataParallelTrainer(H.hip_model('none', 'sum', DP.LAYERS, ['mesh_edges'], sd), lr=DP.LR, max_grad_norm=max_norm,
                                          lr_schedule=_schedule(), weight_decay=WD)
        losses, grad1, norm1 = [], None, None
        for i in range(DP.STEPS):
            losses.append(float(tr.step(g, target, mask)))
            if i == 0:
                grad1, norm1 = tr.fp.grad.clone().cpu(), float(tr.grad_stats[0])
        return tr, losses, grad1, norm1
    max_norm = 0.5 * single(0.0)[3]
    one, losses, grad1, _ = single(max_norm)
    port = 26500 + (os.getpid() % 2000)
    out = str(tmp_path / 'dp_sched.pt')
    ctx = mp.spawn(_dp_worker, args=(2, port, out, max_norm), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0                                   # the test's own limit for the two ranks
    try:
        while not ctx.join(timeout=2.0):                                  # raises as soon as a rank has failed, and ends the other
            assert time.monotonic() < deadline, 'the two ranks did not finish in time'
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    res = torch.load(out)
    sched = _schedule()
    print('two ranks: losses', res['losses'].tolist(), 'one process', losses, '[norm, coef, lr]', res['stats'].tolist())
    assert 0.49 < float(res['stats'][0, 1]) < 0.51                        # clipping was active
    for k in range(DP.STEPS):
        assert abs(float(res['stats'][k, 2]) - _f32(sched.at(k + 1))) <= ULP * sched.at(k + 1)
    for a, b in zip(res['losses'].tolist(), losses):
        assert abs(a - b) <= 5e-5 * abs(b), (a, b)
    for (k, p), off in zip(one.model.named_parameters(), one.fp.offsets):
        want = grad1[off:off + p.numel()]
        if float(want.abs().max()) > 0:
            assert H.rel_err(res['grad1'][off:off + p.numel()], want) <= 1e-5, k
    d = (res['flat'] - one.fp.flat.cpu()).abs()
    assert int((d > 0.005 * DP.STEPS * DP.LR).sum()) <= max(2, d.numel() // 100)
    assert float(d.max()) <= 2 * DP.STEPS * DP.LR


# ---------------------------------------------------------------------------------------------------------------
# 7. resume
# ---------------------------------------------------------------------------------------------------------------
def test_resume_into_a_captured_step_continues_bit_for_bit(tmp_path):
    import warnings
    from hgn_amd import graphs as hg, parallel
    g, target, mask, make = _trainer_problem()
    kw = dict(lr=LR, device_step=True, max_grad_norm=0.5 * _first_norm(), skip_nonfinite=True, lr_schedule=_schedule(), weight_decay=WD)
    straight = parallel.DataParallelTrainer(make(), **kw)
    coefs = []
    for _ in range(6):
        straight.step(g, target, mask)
        coefs.append(float(straight.grad_stats[1]))
    assert 0.49 < coefs[0] < 0.51 and all(0.0 < c <= 1.0 for c in coefs)    # clipping was active
    first = parallel.DataParallelTrainer(make(), **kw)
    for _ in range(3):
        first.step(g, target, mask)
    path = str(tmp_path / 'ckpt.pt')
    torch.save({'model': first.model.state_dict(), 'trainer': first.state_dict()}, path)
    ckpt = torch.load(path, weights_only=True)
    assert all(not x.is_cuda for x in ckpt['trainer'].values() if isinstance(x, torch.Tensor)) and ckpt['trainer']['t'] == 3
    second = parallel.DataParallelTrainer(make(seed=6), **kw)               # a fresh model with other weights, a fresh trainer
    assert not torch.equal(second.fp.flat, first.fp.flat)
    addresses = [x.data_ptr() for x in (second.fp.flat, second.m, second.v, second.t_dev, second.lr_dev, second.grad_stats)]
    second.model.load_state_dict(ckpt['model'])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        second.load_state_dict(ckpt['trainer'])
    assert addresses == [x.data_ptr() for x in (second.fp.flat, second.m, second.v, second.t_dev, second.lr_dev, second.grad_stats)]
    assert torch.equal(second.fp.flat, first.fp.flat) and torch.equal(second.m, first.m) and int(second.t_dev) == 3
    step = hg.GraphedTrainStep(second, g, target, mask, warmup=1)           # captured AFTER the load; its warm-up step is step 4
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    same = _same_state(second, straight)
    same['grad_stats'] = torch.equal(second.grad_stats, straight.grad_stats)
    same['skipped_dev'] = torch.equal(second.skipped_dev, straight.skipped_dev)
    assert all(same.values()) and int(second.t_dev) == 6, same
    deeper = H.hip_model('none', 'sum', 3, ['mesh_edges'], O.init_state_dict_like(
        O.param_shapes('none', 'sum', 3, ['mesh_edges'], 5, {'mesh_edges': 7}, 0, 3, 128), seed=5))
    with torch.no_grad():
        deeper(g)
    with pytest.raises(ValueError, match='laid out differently'):
        parallel.DataParallelTrainer(deeper, **kw).load_state_dict(ckpt['trainer'])
