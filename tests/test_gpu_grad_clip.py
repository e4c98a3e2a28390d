"""Clipping by the global norm and the non-finite-step guard on the GPU: hgn_grad_clip_coef / hgn_adam_step_clip through
ops.grad_norm_clip / ops.adam_step_clip, parallel.DataParallelTrainer(max_grad_norm=..., skip_nonfinite=...) eagerly and captured,
and DataParallelTrainer.step_unrolled on one rank and on two.

Yardsticks.
* Norm: sqrt of the fp64 sum of squares (torch, on the host), rounded to fp32.  The kernel accumulates every square and every
  partial sum in double, so its double sum differs from any other fp64 summation by ~n * 2^-53 relative; after sqrt and ONE rounding
  to fp32 that is the reference's fp32 value or its neighbour: 1 ulp = 2^-23 relative.  The coefficient is the same formula on that
  double: the same bound.
* Adam: hgn_adam_step_dev on copies, torch.equal -- the same update with the two scalars multiplied first.
* Trainer: the same model under autograd + torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, with the tolerances
  test_gpu_parity.py::test_trainer_flat_gradients_and_adam_match_torch holds (2e-6 on gradients, its rule on weights), 1e-5 on the
  coefficient and the moments: Adam's update is nearly invariant under a scaling of the gradient, the moments are not.
* Captured: the eager trainer, torch.equal.
* Unrolled: AbstractSystemModel.unrolled_training_step + backward + clip_grad_norm_ + torch.optim.Adam on a copy (1e-6 on the
  losses, 2e-6 on the flat gradient); two ranks against one process with test_gpu_dp.py's figures (5e-5 losses, 1e-5 gradient)."""
import functools
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
SIZES = [0, 1, 3, 255, 256, 257, 65_541, 2_400_003]
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# The C ABI takes beta1 / beta2 as float: a trainer built with the default betas runs Adam with float32(0.999) = 0.99900001287...,
# hgn_adam_step_dev and hgn_adam_step_clip alike, and its v then sits 1.29e-5 (relative) away from that of a torch.optim.Adam that
# is given the double 0.999 (measured on an MI355X with the defaults: 1.32e-5 .. 1.48e-5 after one step, with m at 1.4e-6 and the
# gradients bit-equal).  The comparisons with torch.optim.Adam therefore hand BOTH sides the same numbers, the float32 neighbours
# of the defaults; 1 - beta is then exact in either arithmetic.
BETAS = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in (0.9, 0.999))


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def _launches(fn):
    """-> (fn(), the library's launch counts by kernel family while it ran)."""
    from hgn_amd import ops
    ops.prof_reset(); ops.prof_enable(True)
    try:
        res = fn()
        counts = {k: v['count'] for k, v in ops.prof_collect().items()}
    finally:
        ops.prof_enable(False)
    return res, counts


# ---------------------------------------------------------------------------------------------------------------
# 1. the norm and the coefficient
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient(n):
    """n values with magnitudes log-uniform in 1e-12 .. 1e6 and random signs, as a view 16 bytes into a larger device buffer (the
    trainer's `grad_ext[4:]`) -> (view, the buffer, fp64 norm on the host).  Shared by the tests, never written."""
    gen = torch.Generator().manual_seed(1000 + n)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 18.0 - 12.0)
    sign = torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0
    host = (mag * sign).to(torch.float32)
    buf = torch.full((n + 8,), 3.0e7, dtype=torch.float32).cuda()      # what lies around the view would show in the norm
    buf[4:4 + n].copy_(host)
    return buf[4:4 + n], buf, float(host.double().square().sum().sqrt())


def _coef64(max_norm, norm64):
    if max_norm <= 0:
        return 1.0
    c = max_norm / (norm64 + 1e-6)
    return float(torch.tensor(c, dtype=torch.float64).to(torch.float32)) if c < 1.0 else 1.0


@pytest.mark.parametrize('n', SIZES)
def test_norm_and_coefficient_vs_fp64_and_bit_reproducible(n):
    from hgn_amd import ops
    g, buf, norm64 = _gradient(n)
    assert g.numel() == n and (n == 0 or g.data_ptr() == buf.data_ptr() + 16)
    want_norm = float(torch.tensor(norm64, dtype=torch.float64).to(torch.float32))
    for max_norm in (0.5 * norm64 if n else 1.0, 2.0 * norm64 + 1.0, 0.0, -1.0, None):
        stats = ops.grad_norm_clip(g, max_norm)
        again = ops.grad_norm_clip(g, max_norm, torch.full((2,), -7.0, device='cuda'))
        assert stats.shape == (2,) and stats.dtype == torch.float32 and torch.equal(stats, again)
        got_norm, got_coef = (float(x) for x in stats.cpu())
        want_coef = _coef64(0.0 if max_norm is None else max_norm, norm64)
        print(f'grad_norm_clip n={n} max_norm={max_norm}: norm {got_norm:.9g} (fp64 {norm64:.17g}) err/ulp '
              f'{abs(got_norm - want_norm) / (ULP * want_norm) if want_norm else 0.0:.3f}  coef {got_coef:.9g} (fp64 formula {want_coef:.9g})')
        assert abs(got_norm - want_norm) <= ULP * want_norm
        assert abs(got_coef - want_coef) <= ULP * want_coef
        if max_norm is None or max_norm <= 0 or max_norm > norm64:
            assert got_coef == 1.0
        else:
            assert got_coef < 1.0
    if n == 0:
        assert got_norm == 0.0
        return
    # the assignment of elements to threads does not depend on where the buffer starts: another alignment, the same bits
    shifted = torch.empty(n + 8, dtype=torch.float32, device='cuda')
    for off in (1, 2, 3):
        shifted[off:off + n].copy_(g)
        assert torch.equal(ops.grad_norm_clip(shifted[off:off + n], 0.5 * norm64), ops.grad_norm_clip(g, 0.5 * norm64)), off


def test_counters_and_argument_checks():
    from hgn_amd import _lib, ops
    g, _, norm64 = _gradient(257)
    step, skipped = torch.tensor([4], dtype=torch.int32, device='cuda'), torch.tensor([2], dtype=torch.int32, device='cuda')
    ops.grad_norm_clip(g, 1.0, step_dev=step, skipped_dev=skipped, skip_nonfinite=True)
    assert int(step) == 5 and int(skipped) == 2
    ops.grad_norm_clip(g, 1.0, step_dev=step)                            # either counter may be absent
    ops.grad_norm_clip(g, 1.0, skipped_dev=skipped)
    assert int(step) == 6 and int(skipped) == 2
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(g.double(), 1.0)
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(torch.zeros(10, 2, device='cuda')[:, 0], 1.0)
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(g, 1.0, stats=torch.zeros(3, device='cuda'))
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(g, 1.0, step_dev=torch.zeros(1, dtype=torch.int64, device='cuda'))
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(g, float('nan'))
    z = torch.zeros(16, device='cuda')
    with pytest.raises(_lib.HgnError):
        ops.adam_step_clip(z, z[:8], z, z, 1e-3, 0.9, 0.999, 1e-8, step, torch.ones(1, device='cuda'))
    with pytest.raises(_lib.HgnError):
        ops.adam_step_clip(z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, None, torch.ones(1, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------
# 2. the update
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adam_state(n=65_541):
    gen = torch.Generator().manual_seed(77)
    p, g, m = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    return p, g * 0.3, m * 0.1, (torch.randn(n, generator=gen) ** 2 * 0.01).cuda()


@pytest.mark.parametrize('clipping', [False, True], ids=['coef-1', 'clipping'])
def test_adam_step_clip_has_the_bits_of_adam_step_dev(clipping):
    from hgn_amd import ops
    p0, g, m0, v0 = _adam_state()
    norm = float(g.double().square().sum().sqrt())
    scale = 0.37
    a = [t.clone() for t in (p0, m0, v0)]
    b = [t.clone() for t in (p0, m0, v0)]
    ta, tb = torch.tensor([4], dtype=torch.int32, device='cuda'), torch.tensor([4], dtype=torch.int32, device='cuda')
    stats = ops.grad_norm_clip(g, 0.25 * norm if clipping else 2.0 * norm, step_dev=ta)
    assert int(ta) == 5
    ops.adam_step_clip(a[0], g, a[1], a[2], ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], ta, stats[1:2], grad_scale=scale)
    coef = stats[1].cpu()
    assert (0.24 < float(coef) < 0.26) if clipping else float(coef) == 1.0
    both = float(torch.tensor(scale, dtype=torch.float32) * coef)         # the two scalars first, in fp32
    ops.adam_step_dev(b[0], g, b[1], b[2], ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], tb, grad_scale=both)
    assert int(ta) == 5 and int(tb) == 5
    for x, y, name in zip(a, b, 'pmv'):
        assert torch.equal(x, y), name
    assert not torch.equal(a[0], p0) and not torch.equal(a[1], m0) and not torch.equal(a[2], v0)


def test_a_non_finite_gradient_is_skipped():
    """One inf, then one NaN, in an ordinary buffer of floats: p, m, v and the step counter keep their bits, the skips are counted."""
    from hgn_amd import ops
    p0, g0, m0, v0 = _adam_state()
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    step, skipped = torch.tensor([4], dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    stats = torch.zeros(2, device='cuda')
    for k, bad in enumerate((float('inf'), float('nan'))):
        g = g0.clone()
        g[40_000 + k] = bad
        ops.grad_norm_clip(g, 1.0, stats, step, skipped, skip_nonfinite=True)
        ops.adam_step_clip(p, g, m, v, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], step, stats[1:2])
        assert int(skipped) == k + 1 and int(step) == 4 and float(stats[1]) == 0.0
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
    ops.grad_norm_clip(g0, 1.0, stats, step, skipped, skip_nonfinite=True)          # a finite gradient again: the step is taken
    ops.adam_step_clip(p, g0, m, v, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], step, stats[1:2])
    assert int(skipped) == 2 and int(step) == 5 and 0.0 < float(stats[1]) <= 1.0 and not torch.equal(p, p0)


# ---------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_problem():
    """The problem of test_gpu_parity.py::test_trainer_flat_gradients_and_adam_match_torch."""
    import hgn_amd
    graph = synth.grid_graph(seed=7, nx=10, ny=9, clusters=4)
    sets = [e.name for e in graph.edge_sets]
    shapes = O.param_shapes('multiscale', 'pna', 2, sets, 5, {n: 7 for n in sets}, 8, 3, 128)
    sd = O.init_state_dict_like(shapes, seed=5)
    target = torch.randn(90, 3, generator=torch.Generator().manual_seed(2)).cuda()
    mask = torch.ones(90, dtype=torch.bool); mask[:3] = False
    g = hgn_amd.MultiGraph([x.cuda() for x in graph.node_features],
                           [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in graph.edge_sets])
    return g, target, mask.cuda(), (lambda: H.hip_model('multiscale', 'pna', 2, sets, sd))


def _check_moments(what, trainer, named, opt, tol=1e-5):
    """trainer.m / trainer.v against torch.optim.Adam's exp_avg / exp_avg_sq, per parameter, where the reference is not zero
    -> the misses (every step's figures are printed before the caller asserts that there are none)."""
    worst = {'m': 0.0, 'v': 0.0}
    offset_of = {id(p): off for p, off in zip(trainer.fp.params, trainer.fp.offsets)}
    offsets = {k: offset_of[id(p)] for k, p in trainer.model.named_parameters() if id(p) in offset_of}
    checked = 0
    for k, p in named:
        st = opt.state.get(p)
        if not st or k not in offsets:
            continue
        off = offsets[k]
        checked += 1
        for name, flat, ref in (('m', trainer.m, st['exp_avg']), ('v', trainer.v, st['exp_avg_sq'])):
            if float(ref.abs().max()) == 0:
                continue
            worst[name] = max(worst[name], H.rel_err(flat[off:off + p.numel()].view(p.shape), ref))
    print(f'{what}: worst rel_err of m {worst["m"]:.3e}, of v {worst["v"]:.3e} over {checked} parameters (bound {tol:g})')
    assert checked >= 2
    return [] if worst['m'] <= tol and worst['v'] <= tol else [(what, worst)]


def test_trainer_clips_like_clip_grad_norm_and_torch_adam():
    from hgn_amd import parallel
    g, target, mask, make = _trainer_problem()
    probe = parallel.DataParallelTrainer(make(), lr=1e-3, skip_nonfinite=True)      # unclipped: reports the norm
    probe.step(g, target, mask)
    norm0, coef0 = (float(x) for x in probe.grad_stats.cpu())
    assert norm0 > 0 and coef0 == 1.0 and int(probe.t_dev) == 1 and int(probe.skipped_dev) == 0
    max_norm = 0.5 * norm0
    ref = make()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=BETAS)
    flat = make()
    tr = parallel.DataParallelTrainer(flat, lr=1e-3, betas=BETAS, wgrad_stream=True, max_grad_norm=max_norm)
    misses = []
    for step in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(target[mask], ref(g)[mask])
        loss.backward()
        g_ref = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in ref.named_parameters()}
        norm_ref = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        coef_ref = min(1.0, max_norm / (norm_ref + 1e-6))
        opt.step()
        l2 = tr.step(g, target, mask)
        norm, coef = (float(x) for x in tr.grad_stats.cpu())
        print(f'trainer clip step {step}: norm {norm:.9g} (torch {norm_ref:.9g})  coef {coef:.9g} (torch {coef_ref:.9g})')
        if step == 0:
            for k, p in flat.named_parameters():
                assert H.rel_err(p.grad, g_ref[k]) <= 2e-6 or float(g_ref[k].abs().max()) == 0, k
            assert 0.49 < coef < 0.51
        assert abs(float(l2) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
        if abs(coef - coef_ref) > 1e-5 * coef_ref:
            misses.append((f'coef at step {step}', coef, coef_ref))
        misses += _check_moments(f'trainer clip step {step}', tr, list(ref.named_parameters()), opt)
    assert not misses, misses
    assert int(tr.t_dev) == 3 and int(tr.skipped_dev) == 0
    for (k, p), (_, q) in zip(ref.named_parameters(), flat.named_parameters()):
        d = (q - p).detach().abs()
        assert int((d > 0.005 * 3 * 1e-3).sum()) <= max(4, d.numel() // 50), k
        assert float(d.max()) <= 2 * 3 * 1e-3, k


def test_a_trainer_without_the_arguments_issues_the_launches_of_before(monkeypatch):
    """No max_grad_norm, no skip_nonfinite: one Adam launch per step through ops.adam_step (ops.adam_step_dev with device_step), none of
    the new entry points; with clipping the step differs by exactly the norm's launch scope, and the Adam goes through adam_step_clip."""
    from hgn_amd import ops, parallel
    g, target, mask, make = _trainer_problem()
    calls = []
    for name in ('adam_step', 'adam_step_dev', 'grad_norm_clip', 'adam_step_clip'):
        monkeypatch.setattr(ops, name, (lambda *a, _f=getattr(ops, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1]))
    counts = {}
    for key, kw in (('plain', {}), ('device', dict(device_step=True)), ('clip', dict(max_grad_norm=1.0)),
                    ('skip', dict(skip_nonfinite=True, device_step=True))):
        tr = parallel.DataParallelTrainer(make(), lr=1e-3, **kw)
        tr.step(g, target, mask)                                           # (the first step records the pack plan: count the second)
        del calls[:]
        _, counts[key] = _launches(lambda: tr.step(g, target, mask))
        counts[key]['calls'] = list(calls)
        assert (tr.grad_stats is None) == (key in ('plain', 'device'))
    print('launch counts per step:', counts)
    assert counts['plain']['calls'] == ['adam_step'] and counts['device']['calls'] == ['adam_step_dev']
    assert counts['clip']['calls'] == ['grad_norm_clip', 'adam_step_clip'] == counts['skip']['calls']
    assert counts['plain']['adam'] == 1 and counts['device']['adam'] == 1 and counts['clip']['adam'] == 2
    rest = lambda c: {k: v for k, v in c.items() if k not in ('adam', 'calls')}
    assert rest(counts['plain']) == rest(counts['device']) == rest(counts['clip']) == rest(counts['skip'])


def test_captured_step_with_clipping_replays_the_eager_steps():
    from hgn_amd import graphs as hg, parallel
    g, target, mask, make = _trainer_problem()
    probe = parallel.DataParallelTrainer(make(), lr=1e-3, max_grad_norm=0.0)
    probe.step(g, target, mask)
    max_norm = 0.1 * float(probe.grad_stats[0])                           # far below the norm: active at every step
    eager = parallel.DataParallelTrainer(make(), lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=True)
    for _ in range(1 + 3):                                                  # the captured step's one warm-up step, then three
        eager.step(g, target, mask)
    tr = parallel.DataParallelTrainer(make(), lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=True)
    step = hg.GraphedTrainStep(tr, g, target, mask, warmup=1)
    seen = []
    for _ in range(3):
        step()
        seen.append(tr.grad_stats.clone())
    torch.cuda.synchronize()
    assert step.captures == 1 and int(tr.t_dev) == 4 == int(eager.t_dev) and int(tr.skipped_dev) == 0
    assert torch.equal(tr.fp.flat, eager.fp.flat) and torch.equal(tr.m, eager.m) and torch.equal(tr.v, eager.v)
    assert torch.equal(seen[2], eager.grad_stats)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])       # the replays compute it anew
    assert all(0.0 < float(s[1]) <= 1.0 for s in seen) and float(seen[0][1]) < 1.0


# ---------------------------------------------------------------------------------------------------------------
# 4. unrolled steps in the trainer
# ---------------------------------------------------------------------------------------------------------------
LR_U = 1e-3


def _noisy_model(kind):
    from tests import test_gpu_noise as TN
    from tests import test_gpu_unrolled_training as UT
    model = UT._model(kind)
    model._params = dict(model._params, **TN.NOISE[kind])
    model.noise_seed = 77
    return model


def _pick(win, idx):
    """The windows `idx` of a set of windows (the mesh is shared)."""
    return {k: (v if k in ('cells', 'mesh_pos') else v[idx]) for k, v in win.items()}


@pytest.mark.parametrize('kind,through_state', [('flag', True), ('cylinder', False)])
def test_step_unrolled_vs_unrolled_training_step_clip_grad_norm_and_torch_adam(kind, through_state):
    from hgn_amd import parallel
    from tests import test_gpu_unrolled_training as UT
    W, n_steps = 2, 3
    win = UT._windows(kind, W, n_steps)
    probe = _noisy_model(kind)
    probe.unrolled_training_step(win, n_steps, through_state=through_state, noise_draw=0)[0].backward()
    max_norm = 0.5 * float(torch.nn.utils.clip_grad_norm_(probe.learned_model.parameters(), float('inf')))
    ref, mine = _noisy_model(kind), _noisy_model(kind)
    opt = torch.optim.Adam(ref.learned_model.parameters(), lr=LR_U, betas=BETAS)
    tr = parallel.DataParallelTrainer(mine.learned_model, lr=LR_U, betas=BETAS, max_grad_norm=max_norm)
    misses = []
    with pytest.raises(ValueError, match='learned_model'):
        tr.step_unrolled(ref, win, n_steps)
    for draw in range(2):                                  # the second step refreshes the packed weights through the recorded plan
        opt.zero_grad()
        loss, per = ref.unrolled_training_step(win, n_steps, through_state=through_state, is_training=True, noise_draw=draw)
        loss.backward()
        named = list(ref.learned_model.named_parameters())
        g_ref = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in named}
        norm_ref = float(torch.nn.utils.clip_grad_norm_(ref.learned_model.parameters(), max_norm))
        coef_ref = min(1.0, max_norm / (norm_ref + 1e-6))
        opt.step()
        share, per_t = tr.step_unrolled(mine, win, n_steps, through_state=through_state, is_training=True, noise_draw=draw)
        norm, coef = (float(x) for x in tr.grad_stats.cpu())
        errs = {'loss': H.rel_err(share, loss), 'per-step': H.rel_err(per_t, per)}
        worst = max(H.rel_err(p.grad, g_ref[k]) for k, p in mine.learned_model.named_parameters() if float(g_ref[k].abs().max()) > 0)
        print(f'step_unrolled[{kind}] step {draw}: {errs}  worst gradient rel_err {worst:.3e}  norm {norm:.9g} (torch {norm_ref:.9g})  '
              f'coef {coef:.9g} (torch {coef_ref:.9g})')
        assert per_t.shape == (n_steps,) and not share.requires_grad and share.dim() == 0
        assert errs['loss'] <= 1e-6 and errs['per-step'] <= 1e-6
        assert worst <= 2e-6
        assert draw > 0 or 0.49 < coef < 0.51
        if abs(coef - coef_ref) > 1e-5 * coef_ref:
            misses.append((f'coef at step {draw}', coef, coef_ref))
        misses += _check_moments(f'step_unrolled[{kind}] step {draw}', tr, named, opt)
    assert not misses, misses
    assert tr.overlap is True and tr.ctx.pack_plan is not None and int(tr.t_dev) == 2


def _unrolled_worker(rank, world, port, out, max_norm):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hgn_amd import parallel
    from hgn_amd.normalizer import Normalizer
    from tests import test_gpu_unrolled_training as UT
    model = _noisy_model('flag')
    parallel.attach_normalizer_sync([m for m in model.modules() if isinstance(m, Normalizer)])
    mine = parallel.shard_indices(4, rank, world)                  # windows r, r + 2, under their global ids
    win = _pick(UT._windows('flag', 4, 3), mine)
    tr = parallel.DataParallelTrainer(model.learned_model, lr=LR_U, max_grad_norm=max_norm)
    losses, stats, grad1 = [], [], None
    for draw in range(3):
        losses.append(tr.step_unrolled(model, win, 3, through_state=True, noise_draw=draw, frame_ids=mine)[0])
        stats.append(tr.grad_stats.clone())
        if draw == 0:
            grad1 = tr.fp.grad.clone()
    torch.cuda.synchronize()
    total = torch.stack(losses).cpu()
    dist.all_reduce(total)                                         # the shares of the global mean add up to it
    state = torch.cat([tr.fp.flat, tr.m, tr.v] + stats).cpu()
    theirs = state.clone()
    dist.broadcast(theirs, src=0)
    assert torch.equal(state, theirs), 'replicas (or their grad_stats) differ'
    if rank == 0:
        torch.save({'grad1': grad1.cpu(), 'losses': total, 'stats': torch.stack(stats).cpu()}, out)
    dist.destroy_process_group()


def test_step_unrolled_on_two_ranks_equals_one_process(tmp_path):
    from hgn_amd import parallel
    from tests import test_gpu_unrolled_training as UT
    order = parallel.shard_indices(4, 0, 2) + parallel.shard_indices(4, 1, 2)
    win = _pick(UT._windows('flag', 4, 3), order)

    def single(max_norm):
        model = _noisy_model('flag')
        tr = parallel.DataParallelTrainer(model.learned_model, lr=LR_U, max_grad_norm=max_norm)
        losses, grad1 = [], None
        for draw in range(3):
            losses.append(float(tr.step_unrolled(model, win, 3, through_state=True, noise_draw=draw, frame_ids=order)[0]))
            if draw == 0:
                grad1, norm1 = tr.fp.grad.clone().cpu(), float(tr.grad_stats[0])
        return tr, losses, grad1, norm1
    max_norm = 0.5 * single(0.0)[3]
    tr, losses, grad1, _ = single(max_norm)
    port = 27500 + (os.getpid() % 2000)
    out = str(tmp_path / 'unrolled.pt')
    mp.spawn(_unrolled_worker, args=(2, port, out, max_norm), nprocs=2, join=True)
    res = torch.load(out)
    print('two ranks: losses', res['losses'].tolist(), 'one process', losses, 'stats', res['stats'].tolist())
    assert 0.49 < float(res['stats'][0, 1]) < 0.51                  # clipping was active
    for a, b in zip(res['losses'].tolist(), losses):
        assert abs(a - b) <= 5e-5 * abs(b), (a, b)
    for (k, p), off in zip(tr.model.named_parameters(), tr.fp.offsets):
        want = grad1[off:off + p.numel()]
        if float(want.abs().max()) > 0:
            assert H.rel_err(res['grad1'][off:off + p.numel()], want) <= 1e-5, k
