"""Activation checkpointing for unrolled training steps, on the GPU: `unrolled_training_step(..., checkpoint=True)`,
`DataParallelTrainer.step_unrolled(..., checkpoint=True)`, ops.nested_backward.

Yardstick, in every comparison: the plain call (checkpoint=None) on another deep copy of the same warm model.  `loss` and
`per_step_losses` must be torch.equal -- a step's forward is the same launches on the same bits, with or without z saves.  State-leaf
gradients and ALL parameter gradients must agree within helpers.rel_err <= TOL_GRAD (the 1e-5 of tests/test_gpu_unrolled_training.py),
and every parameter gradient must be non-zero.  Whether the gradients are bit-equal as well is printed, not asserted.
Shapes are those of tests/test_gpu_unrolled_training.py: the 5 x 4 synthetic meshes, W = 2 windows, 2 message-passing layers (the memory
test alone takes more windows, for the reason it gives)."""
import random

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import synth
from tests import test_gpu_unrolled_training as UT

pytestmark = pytest.mark.gpu
TOL_GRAD = UT.TOL_GRAD


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def _noisy(model, kind):
    from tests import test_gpu_noise as TN
    model._params = dict(model._params, **TN.NOISE[kind])
    model.noise_seed = 77
    return model


def _seed(seed):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _route(model, kind, win, n_steps, checkpoint, leaves=True, seed=None, **kw):
    """One forward + backward of a route on fresh leaves -> what the comparisons read."""
    model.zero_grad(set_to_none=True)
    held = {}
    if leaves:
        win, held = UT._with_leaves(win, kind)
    if seed is not None:
        _seed(seed)
    loss, per = model.unrolled_training_step(win, n_steps, checkpoint=checkpoint, **kw)
    assert loss.dim() == 0 and loss.grad_fn is not None and per.shape == (n_steps,) and not per.requires_grad
    loss.backward()
    return {'loss': loss.detach(), 'per': per, 'leaves': {n: x.grad for n, x in held.items()},
            'grads': {n: p.grad for n, p in model.learned_model.named_parameters()}, 'stats': UT._stats(model),
            'rng': (torch.get_rng_state(), torch.cuda.get_rng_state())}


def _same(tag, plain, ckpt, parameters=True):
    assert torch.equal(plain['loss'], ckpt['loss']) and torch.equal(plain['per'], ckpt['per']), tag
    worst, equal, total = 0.0, 0, 0
    assert plain['leaves'].keys() == ckpt['leaves'].keys()
    for n, want in plain['leaves'].items():
        got = ckpt['leaves'][n]
        assert (want is None) == (got is None), n                       # (a noised series hands its leaf no gradient on either route)
        if want is None:
            continue
        assert float(got.abs().max()) > 0, n
        err = H.rel_err(got, want)
        worst, equal, total = max(worst, err), equal + int(torch.equal(got, want)), total + 1
        assert err <= TOL_GRAD, (tag, n, err)
    if parameters:
        assert plain['grads'].keys() == ckpt['grads'].keys() and len(plain['grads']) > 2
        for n, want in plain['grads'].items():
            got = ckpt['grads'][n]
            assert want is not None and got is not None, n
            assert float(got.abs().max()) > 0, (tag, n)
            err = H.rel_err(got, want)
            worst, equal, total = max(worst, err), equal + int(torch.equal(got, want)), total + 1
            assert err <= TOL_GRAD, (tag, n, err)
    print(f'checkpoint[{tag}]: worst gradient rel_err {worst:.3e}; bit-equal gradients {equal} of {total}')


def _same_stats(tag, plain, ckpt, before=None):
    a, b = plain['stats'], ckpt['stats']
    assert a.keys() == b.keys()
    for n in a:
        assert all(torch.equal(x, y) for x, y in zip(a[n][:4], b[n][:4])) and a[n][4] == b[n][4], (tag, n)
    if before is not None:                                              # and the call did accumulate
        assert a['_output_normalizer'][4] == before['_output_normalizer'][4] + 1


# ---------------------------------------------------------------------------------------------------------------
# 1. / 2. through the state
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n_steps', [('flag', 3), ('cylinder', 2)])
def test_through_state_with_frozen_statistics(kind, n_steps):
    win = UT._windows(kind, 2, n_steps)
    a, b = UT._model(kind), UT._model(kind)
    before = UT._stats(a)
    plain = _route(a, kind, win, n_steps, None, through_state=True, is_training=False)
    ckpt = _route(b, kind, win, n_steps, True, through_state=True, is_training=False)
    _same(f'{kind}-{n_steps}', plain, ckpt)
    _same_stats(kind, plain, ckpt)
    if kind == 'cylinder':                                              # (the flag's node-dynamic normaliser accumulates on every build)
        assert all(before[n][4] == ckpt['stats'][n][4] for n in before)
    # checkpoint=False is the plain step as well
    off = _route(UT._model(kind), kind, win, n_steps, False, through_state=True, is_training=False)
    assert torch.equal(off['loss'], plain['loss']) and all(torch.equal(off['grads'][n], plain['grads'][n]) for n in plain['grads'])


@pytest.mark.parametrize('loss_kernel', [False, True], ids=['torch-loss', 'loss-kernel'])
@pytest.mark.parametrize('kind,n_steps', [('flag', 3), ('cylinder', 2)])
def test_training_mode_with_noise_leaves_the_statistics_of_the_plain_call(kind, n_steps, loss_kernel):
    win = UT._windows(kind, 2, n_steps)
    a, b = _noisy(UT._model(kind), kind), _noisy(UT._model(kind), kind)
    a.loss_kernel = b.loss_kernel = loss_kernel
    before = UT._stats(a)
    plain = _route(a, kind, win, n_steps, None, through_state=True, is_training=True, noise_draw=5)
    ckpt = _route(b, kind, win, n_steps, True, through_state=True, is_training=True, noise_draw=5)
    _same(f'{kind}-{n_steps}-noise-{loss_kernel}', plain, ckpt)
    _same_stats(kind, plain, ckpt, before)
    assert not any('replay' in m.__dict__ or 'record' in m.__dict__ for m in b.modules())


# ---------------------------------------------------------------------------------------------------------------
# 3. push-forward: draws and clusters
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,connector,frequency', [('plate', 'none', 1), ('flag', 'hyper', 1), ('flag', 'hyper', 3)],
                         ids=['plate', 'flag-hyper', 'flag-hyper-clusters-every-step'])
def test_push_forward_replays_the_draws_and_keeps_the_clusters(kind, connector, frequency, monkeypatch):
    n_steps = 3
    win = UT._windows(kind, 2, n_steps)
    res, calls, last = {}, {}, {}
    for route, checkpoint in (('plain', None), ('ckpt', True)):
        model = UT._model(kind, connector)
        calls[route] = []
        if connector != 'none':
            model._remote_graph._node_connector._noise_scale = 0.003       # `hyper_noise` on: one torch.normal per call
            model._rmp_frequency = frequency
            algo = model._remote_graph._clustering_algorithm

            def run(*args, _real=algo.run, _log=calls[route], **kw):
                out = _real(*args, **kw)
                _log.append(out)
                return out
            monkeypatch.setattr(algo, 'run', run)
        res[route] = _route(model, kind, win, n_steps, checkpoint, leaves=False, seed=11, through_state=False, is_training=True)
        last[route] = model._remote_graph._clusters if connector != 'none' else None
    _same(f'{kind}-{connector}-f{frequency}', res['plain'], res['ckpt'])
    _same_stats(kind, res['plain'], res['ckpt'])
    assert torch.equal(res['plain']['rng'][0], res['ckpt']['rng'][0]) and torch.equal(res['plain']['rng'][1], res['ckpt']['rng'][1])
    if connector != 'none':
        assert len(calls['plain']) == len(calls['ckpt']) == frequency
        got, want = last['ckpt'], calls['ckpt'][-1]                       # the clusters of the first pass, not of a rebuild
        assert got is want or (len(got) == len(want) and all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(got, want)))
        assert len(got) == len(last['plain']) and all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(got, last['plain']))
        # the draw matters: another seed gives another loss, so the rebuild did replay it
        model = UT._model(kind, connector)
        model._remote_graph._node_connector._noise_scale = 0.003
        model._rmp_frequency = frequency
        other = _route(model, kind, win, n_steps, None, leaves=False, seed=12, through_state=False, is_training=True)
        assert not torch.equal(other['per'][0], res['plain']['per'][0])


# ---------------------------------------------------------------------------------------------------------------
# 4. / 5. connector with position gradients; frozen network; torch.autograd.grad
# ---------------------------------------------------------------------------------------------------------------
def test_connector_with_position_gradients():
    win = UT._windows('flag', 2, 2)
    a, b = UT._model('flag', 'hyper'), UT._model('flag', 'hyper')
    a.position_gradients = b.position_gradients = True
    plain = _route(a, 'flag', win, 2, None, through_state=True, is_training=False)
    ckpt = _route(b, 'flag', win, 2, True, through_state=True, is_training=False)
    _same('flag-hyper-position-gradients', plain, ckpt)
    # without the switch the refusals are those of the plain call: through the state at once, a graph that carries grad at step 0
    from hgn_amd import _lib
    c = UT._model('flag', 'hyper')
    with pytest.raises(_lib.HgnError, match='through_state'):
        c.unrolled_training_step(win, 2, through_state=True, is_training=False, checkpoint=True)
    leafy, _ = UT._with_leaves(win, 'flag')
    for checkpoint in (None, True):
        with pytest.raises(_lib.HgnError):
            c.unrolled_training_step(leafy, 2, through_state=False, is_training=False, checkpoint=checkpoint)
    with pytest.raises(ValueError, match='unrolled_training_step'):
        c.unrolled_training_step(win, 3, through_state=False, checkpoint=True)


def test_frozen_network_gives_state_gradients_only():
    win = UT._windows('flag', 2, 3)
    a, b = UT._model('flag'), UT._model('flag')
    for m in (a, b):
        m.learned_model.requires_grad_(False)
    plain = _route(a, 'flag', win, 3, None, through_state=True, is_training=False)
    ckpt = _route(b, 'flag', win, 3, True, through_state=True, is_training=False)
    _same('flag-frozen', plain, ckpt, parameters=False)
    assert all(g is None for g in ckpt['grads'].values()) and all(g is not None for g in ckpt['leaves'].values())


def test_autograd_grad_with_respect_to_the_leaves():
    win = UT._windows('flag', 2, 3)
    grads = {}
    for route, checkpoint in (('plain', None), ('ckpt', True)):
        model = UT._model('flag')
        w, leaves = UT._with_leaves(win, 'flag')
        loss, _ = model.unrolled_training_step(w, 3, through_state=True, is_training=False, checkpoint=checkpoint)
        grads[route] = torch.autograd.grad(loss, list(leaves.values()))
        assert all(p.grad is None for p in model.learned_model.parameters()) and all(x.grad is None for x in leaves.values())
    for want, got in zip(grads['plain'], grads['ckpt']):
        assert float(got.abs().max()) > 0 and H.rel_err(got, want) <= TOL_GRAD


# ---------------------------------------------------------------------------------------------------------------
# 6. one step is the plain step; how often the network runs
# ---------------------------------------------------------------------------------------------------------------
def test_one_step_is_the_plain_step_and_n_steps_cost_n_minus_one_more_forwards():
    counts = {}
    for n_steps in (1, 3):
        win = UT._windows('flag', 2, n_steps)
        res = {}
        for route, checkpoint in (('plain', None), ('ckpt', True)):
            model = UT._model('flag')
            seen = []
            handle = model.learned_model.register_forward_hook(lambda *a: seen.append(1))
            res[route] = _route(model, 'flag', win, n_steps, checkpoint, through_state=True, is_training=True)
            handle.remove()
            counts[n_steps, route] = len(seen)
        if n_steps == 1:
            assert torch.equal(res['plain']['loss'], res['ckpt']['loss']) and torch.equal(res['plain']['per'], res['ckpt']['per'])
            for group in ('leaves', 'grads'):
                assert all(torch.equal(res['plain'][group][n], res['ckpt'][group][n]) for n in res['plain'][group])
            _same_stats('one step', res['plain'], res['ckpt'])
    assert counts == {(1, 'plain'): 1, (1, 'ckpt'): 1, (3, 'plain'): 3, (3, 'ckpt'): 3 + 2}


# ---------------------------------------------------------------------------------------------------------------
# 7. the trainer: weight gradients deferred into the flat buffer, nested engine runs
# ---------------------------------------------------------------------------------------------------------------
def _trainer(kind, connector, side=False):
    """A trainer on a deep copy of the warm model, at rate 0 -- the weights stay what they are, so every step of every trainer
    differentiates the same function -- with ``max_grad_norm`` set and an ``adam_fn`` that clones the gradient it is handed and
    changes nothing.  (On the device the clipped update is the trainer's own kernel pair, which does not go through ``adam_fn`` and
    leaves the gradient buffer as it is: `_flat_grad` reads the clone when there is one, the buffer otherwise.)"""
    from hgn_amd import parallel
    model = UT._model(kind, connector)
    handed = []

    def adam_fn(p, g, m, v, lr, b1, b2, eps, step, **kw):
        handed.append(g.clone())
    tr = parallel.DataParallelTrainer(model.learned_model, lr=0.0, max_grad_norm=1.0, adam_fn=adam_fn, wgrad_stream=side)
    return model, tr, handed


def _flat_grad(tr, handed):
    torch.cuda.synchronize()
    return handed.pop() if handed else tr.fp.grad.clone()


@pytest.mark.parametrize('kind,connector,through_state,side', [('flag', 'none', True, False), ('flag', 'hyper', False, False),
                                                               ('flag', 'none', True, True)],
                         ids=['flag-through-state', 'flag-hyper-push-forward', 'flag-through-state-side-stream'])
def test_trainer_loses_no_deferred_weight_gradient(kind, connector, through_state, side):
    from hgn_amd import ops
    n_steps = 3
    win = UT._windows(kind, 2, n_steps)
    kw = dict(through_state=through_state, is_training=False)

    def step(trainer, checkpoint):
        model, tr, handed = trainer
        weights = tr.fp.flat.clone()
        share, per = tr.step_unrolled(model, win, n_steps, checkpoint=checkpoint, **kw)
        g = _flat_grad(tr, handed)
        assert ops.discard_stale_wgrad(tr.ctx) == 0 and tr.ctx.wq_graph_task == -1 and not tr.ctx.redq and not tr.ctx.lnq
        assert tr.overlap is True and tr.ctx.wgrad_stream is None and torch.equal(weights, tr.fp.flat)
        return share, per, g

    a, b = _trainer(kind, connector, side), _trainer(kind, connector, side)
    share_p, per_p, g_plain = step(a, None)
    share_c, per_c, g_ckpt = step(b, True)
    assert torch.equal(share_p, share_c) and torch.equal(per_p, per_c)
    err = H.rel_err(g_ckpt, g_plain)
    print(f'trainer[{kind}-{connector}-side={side}]: flat gradient rel_err {err:.3e} bit_equal={bool(torch.equal(g_ckpt, g_plain))}')
    assert err <= TOL_GRAD
    for g in (g_plain, g_ckpt):
        for p, off in zip(a[1].fp.params, a[1].fp.offsets):
            assert float(g[off:off + p.numel()].abs().max()) > 0, off
    # the other kind of step directly afterwards: the pack plan one kind recorded serves the other, and the queue is as a fresh one
    assert a[1].ctx.pack_plan is not None and b[1].ctx.pack_plan is not None
    _, _, g_ckpt_after_plain = step(a, True)
    _, _, g_plain_after_ckpt = step(b, None)
    for what, got, want in (('checkpointed after plain', g_ckpt_after_plain, g_ckpt), ('plain after checkpointed', g_plain_after_ckpt, g_plain)):
        err = H.rel_err(got, want)
        print(f'trainer[{kind}-{connector}-side={side}] {what}: rel_err vs a fresh trainer {err:.3e} bit_equal={bool(torch.equal(got, want))}')
        assert err <= TOL_GRAD, what


def test_a_backward_pass_that_raises_leaves_nothing_queued():
    from hgn_amd import ops
    model, tr, handed = _trainer('flag', 'none')
    win = UT._windows('flag', 2, 3)
    _, _, want = (*tr.step_unrolled(model, win, 3, is_training=False, checkpoint=True), _flat_grad(tr, handed))
    real, seen = model._unroll_step, []

    def failing(frame, W, t, *args, **kw):
        seen.append((t, torch.is_grad_enabled()))
        if torch.is_grad_enabled() and t == 0:                           # the rebuild of step 0: steps 2 and 1 have queued and flushed
            raise RuntimeError('rebuild failed')
        return real(frame, W, t, *args, **kw)
    model._unroll_step = failing
    with pytest.raises(RuntimeError, match='rebuild failed'):
        tr.step_unrolled(model, win, 3, is_training=False, checkpoint=True)
    del model._unroll_step
    assert (0, True) in seen and tr.overlap is True and tr.ctx.wgrad_stream is None
    assert not any('replay' in m.__dict__ or 'record' in m.__dict__ for m in model.modules())
    assert sum(len(q[0]) for q in tr.ctx.wq.values()) + len(tr.ctx.redq) + len(tr.ctx.lnq) == 0
    tr.step_unrolled(model, win, 3, is_training=False, checkpoint=True)   # and the next step is a whole one
    got = _flat_grad(tr, handed)
    assert H.rel_err(got, want) <= TOL_GRAD


class _NestedRun(torch.autograd.Function):
    """x -> x; its backward runs ``fn`` (a forward + backward of its own: an engine run nested in the outer one)."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


@pytest.mark.parametrize('supported', [True, False], ids=['nested_backward', 'bare-nested-run'])
def test_an_outer_run_with_queued_tasks_keeps_them_across_a_nested_run_only_under_nested_backward(supported):
    """The rule itself, without the checkpointed step (whose steps are all nested runs, so that its outer run queues nothing): the
    network's backward pass in the OUTER run defers node-level weight gradients, LayerNorm slabs and slab sums into a flat buffer; then
    a node's backward runs the same forward + backward again as a nested run.  Under ops.nested_backward the buffer ends with twice the
    gradient of one pass; a bare nested run makes `_arm_flush` drop what the outer run had queued, and the buffer misses it."""
    import contextlib
    from hgn_amd import ops, parallel
    model = UT._model('flag')
    win = UT._windows('flag', 2, 1)
    frame = {k: (v if k in ('cells', 'mesh_pos') else v[:, 0]) for k, v in win.items()}
    graph = model.expand_graph_batch(model.build_graph_batch(frame, False), 2, 0, 1, False)
    net = model.learned_model
    fp = parallel.FlatParams(net)
    ctx = net._hgn_ctx
    queued = []

    def one_pass():
        net(graph).square().sum().backward()

    def nested():
        queued.append(sum(len(q[0]) for q in ctx.wq.values()) + len(ctx.redq) + len(ctx.lnq))
        with (ops.nested_backward(ctx) if supported else contextlib.nullcontext()), torch.enable_grad():
            one_pass()
    fp.zero_grad()
    one_pass()
    torch.cuda.synchronize()
    once = fp.grad.clone()
    assert float(once.abs().max()) > 0
    fp.zero_grad()
    ops.discard_stale_wgrad(ctx)
    anchor = torch.zeros(1, device='cuda', requires_grad=True)
    tail = _NestedRun.apply(anchor, nested)                             # made first: its backward runs last in the outer run
    (net(graph).square().sum() + tail.sum()).backward()
    torch.cuda.synchronize()
    assert queued and queued[0] > 0, 'the outer run had nothing queued when the nested run began: the case shows nothing'
    err = H.rel_err(fp.grad, 2 * once)
    print(f'nested run, supported={supported}: {queued[0]} entries queued by the outer run; flat gradient vs twice one pass rel_err {err:.3e}')
    assert ops.discard_stale_wgrad(ctx) == 0
    if supported:
        assert err <= TOL_GRAD
    else:
        assert err > 1e-3                                               # the outer run's queued gradients are gone


def test_a_second_backward_is_refused_in_words_and_no_grad_takes_the_plain_route():
    win = UT._windows('flag', 2, 3)
    model = UT._model('flag')
    loss, _ = model.unrolled_training_step(win, 3, is_training=False, checkpoint=True)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    seen = []
    model.replay_rollout = False                                          # (every launch eager: no capture inside this test)
    real = model._unroll_step
    model._unroll_step = lambda *a, **kw: seen.append(torch.is_grad_enabled()) or real(*a, **kw)
    with torch.no_grad():
        quiet, per = model.unrolled_training_step(win, 3, is_training=False, checkpoint=True)
        plain, per_plain = model.unrolled_training_step(win, 3, is_training=False)
    del model._unroll_step
    assert seen == [False] * 6 and not quiet.requires_grad                # no step was built with gradients
    assert torch.equal(quiet, plain) and torch.equal(per, per_plain) and torch.equal(quiet, loss.detach())


# ---------------------------------------------------------------------------------------------------------------
# 8. memory
# ---------------------------------------------------------------------------------------------------------------
def test_a_checkpointed_unroll_keeps_one_step_of_activations():
    """A = P2 - P1 is what one more plain step retains; a checkpointed unroll of four steps must stay below P1 + A / 2 and below P2.
    The mesh is the suite's 5 x 4 one, the smallest: a row keeps 2-3 KB per layer against the 24 B of its two states, so A >= 64 *
    the bytes of the states holds there for any W (asserted).  W is sized by what no mesh changes: a rebuilt step holds one set of
    parameter gradients (about 1.6 MB for the two-layer model) until it hands them to the outer backward pass.  W = 96 windows (1 920
    node rows) make a step's activations dwarf those too; A >= 8 * the parameters' bytes is asserted so that the choice shows."""
    nx, ny = 5, 4
    W, T = 96, 4
    frames = [[synth.flag_frame(seed=300 + 10 * w + t, nx=nx, ny=ny) for t in range(T)] for w in range(W)]
    names = ('world_pos', 'prev|world_pos', 'target|world_pos', 'node_type')
    win = {n: torch.stack([torch.stack([f[n] for f in row]) for row in frames]).cuda() for n in names}
    win['cells'], win['mesh_pos'] = frames[0][0]['cells'].cuda(), frames[0][0]['mesh_pos'].cuda()
    model = UT._model('flag')

    def peak(n_steps, checkpoint):
        model.zero_grad(set_to_none=True)
        w, leaves = UT._with_leaves(win, 'flag')
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, _ = model.unrolled_training_step(w, n_steps, through_state=True, is_training=False, checkpoint=checkpoint)
        loss.backward()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        assert all(x.grad is not None for x in leaves.values())
        del loss, w, leaves
        return rise
    peak(2, None), peak(2, True)                                         # warm: workspaces, topology caches, lazy state
    p1, p2, c4 = peak(1, None), peak(2, None), peak(4, True)
    a = p2 - p1
    state_bytes = 2 * win['world_pos'][:, 0].numel() * 4
    param_bytes = sum(p.numel() * 4 for p in model.learned_model.parameters())
    print(f'memory: P1={p1} P2={p2} A={a} C4={c4} bytes; states {state_bytes}, parameters {param_bytes}; C4 - P1 = {c4 - p1}')
    assert a > 0 and a >= 64 * state_bytes and a >= 8 * param_bytes
    assert c4 <= p1 + a / 2
    assert c4 < p2
