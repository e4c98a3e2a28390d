"""Training on unrolled multi-step rollouts in lock step, on the GPU: features.advance_state (the one-launch state update as a
differentiable function; backward = hgn_rollout_advance_bwd) and AbstractSystemModel.unrolled_training_step.

Yardsticks.
* advance_state forward: features.rollout_advance into caller buffers and Normalizer.inverse -> lincomb3 -> torch.where, torch.equal.
* advance_state backward: the derivative table of include/hgn_features.h evaluated in fp64 on the fp32 inputs and the fp32 scale
  s_c = normalizer._std_with_epsilon().  d_net = s_c * (g + h) takes two roundings of at most 2^-24 each: |got - exact| <=
  2^-23 * s_c * (|g| + |h|).  d_cur / d_prev / d_fallback take one: <= 2^-24 * |exact| (exact when the coefficient is a power of
  two).  What a row that is not free passes on is a copy or a zero: exact.
* unrolled_training_step: `training_step` on the batched graph for one step (torch.equal); for more steps the same loop written
  per window with build_graph, batching.batch_graphs, update and torch.where (loss torch.equal: the same arithmetic row by row;
  gradients within the project's 1e-5, helpers.rel_err: autograd sums a leaf's contributions in another order); the fp64 oracle
  with the HIP forward's ReLU gates transferred (1e-5, as test_gpu_feature_grad.py holds the two-step unroll); `rollout_batch`
  for the states of the push-forward mode (torch.equal).
Meshes are the 5 x 4 synthetic ones (20 nodes; the plate frame of tests/synth.py has 158), message_passing_steps = 2.  Statistics are
frozen where two routes are compared: the normalisers are warmed once without gradients and the routes run with is_training=False."""
import copy
import functools

import pytest
import torch

from oracle import features_oracle as FO
from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests import test_gpu_feature_grad as FG

pytestmark = pytest.mark.gpu
TOL_GRAD = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


# ---------------------------------------------------------------------------------------------------------------
# 1. / 2. the operator
# ---------------------------------------------------------------------------------------------------------------
CASES = {'flag': dict(F=3, d=3, prev=True, ca=2.0, cp=-1.0, inv_from=None, fallback=False, free=(0,)),
         'cylinder': dict(F=3, d=2, prev=False, ca=1.0, cp=0.0, inv_from=2, fallback=False, free=(0, 5)),
         'plate': dict(F=3, d=3, prev=False, ca=1.0, cp=0.0, inv_from=0, fallback=True, free=(0,)),
         'general': dict(F=5, d=2, prev=True, ca=1.7, cp=-0.3, inv_from=1, fallback=False, free=(0, 3))}
ROWS = [1, 85, 86, 300]          # F = 3: 85 / 86 rows put the last thread on either side of a 256-thread block boundary
KINDS = torch.tensor([0, 1, 3, 5, 40, -1], dtype=torch.int64)     # 40, -1: outside the bit mask, never free


@functools.lru_cache(maxsize=None)
def _normalizer(F):
    from hgn_amd.normalizer import Normalizer
    gen = torch.Generator().manual_seed(F)
    nz = Normalizer(F, 'output_normalizer')
    scale, shift = torch.tensor([0.3, 2.0, 11.0, 0.7, 5.0][:F]), torch.tensor([0.1, -1.5, 4.0, 0.0, -2.0][:F])
    nz((torch.randn(257, F, generator=gen) * scale + shift).cuda())
    return nz


@functools.lru_cache(maxsize=None)
def _inputs(name, rows):
    """The inputs of one case on the device (shared by the tests, never written): the network output is a column slice of a wider
    tensor; w_next / w_inv are the gradients that arrive at the two outputs."""
    c = CASES[name]
    F, d = c['F'], c['d']
    gen = torch.Generator().manual_seed(1000 * rows + 10 * F + d)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()
    width_inv = F - c['inv_from'] if c['inv_from'] is not None else 0
    node_type = KINDS[torch.randint(0, len(KINDS), (rows, 1), generator=gen)].cuda()
    return dict(c, wide=rnd(rows, F + 4), cur=rnd(rows, d), prev=rnd(rows, d) if c['prev'] else None,
                fb=rnd(rows, d) if c['fallback'] else None, node_type=node_type, w_next=rnd(rows, d),
                w_inv=rnd(rows, width_inv) if width_inv else None, nz=_normalizer(F))


def _leaf(t, grad=True):
    return None if t is None else t.detach().clone().requires_grad_(grad)


def _advance(x, grads=('net', 'cur', 'prev', 'fb')):
    """advance_state on fresh leaves of the case -> (leaves, next, inv)."""
    from hgn_amd import features
    leaves = {'wide': _leaf(x['wide'], 'net' in grads), 'cur': _leaf(x['cur'], 'cur' in grads), 'prev': _leaf(x['prev'], 'prev' in grads),
              'fb': _leaf(x['fb'], 'fb' in grads)}
    net = leaves['wide'][:, 2:2 + x['F']]
    nxt, inv = features.advance_state(net, x['nz'], leaves['cur'], x['d'], x['ca'], leaves['prev'], x['cp'], x['node_type'], x['free'],
                                      leaves['fb'], x['inv_from'])
    return leaves, nxt, inv


def _backward(x, nxt, inv, g, h):
    outs, grads = [nxt] + ([inv] if inv is not None else []), [g] + ([h] if inv is not None else [])
    torch.autograd.backward(outs, grads)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('name', list(CASES))
def test_advance_state_forward_has_the_bits_of_rollout_advance_and_of_the_three_launches(name, rows):
    from hgn_amd import features
    x = _inputs(name, rows)
    F, d, inv_from = x['F'], x['d'], x['inv_from']
    net = x['wide'][:, 2:2 + F]
    assert not net.is_contiguous() or rows == 1
    nxt, inv = features.advance_state(net, x['nz'], x['cur'], d, x['ca'], x['prev'], x['cp'], x['node_type'], x['free'], x['fb'], inv_from)
    assert nxt.grad_fn is None and not nxt.requires_grad and (inv is None) == (inv_from is None)     # no autograd node
    assert nxt.shape == (rows, d) and (inv is None or inv.shape == (rows, F - inv_from))
    # rollout_advance into caller buffers
    buf = torch.empty(rows, d, device='cuda')
    ibuf = torch.empty(rows, F - inv_from, device='cuda') if inv_from is not None else None
    features.rollout_advance(net, x['nz'], x['cur'], d, x['ca'], x['prev'], x['cp'], x['node_type'], x['free'], x['fb'], buf,
                             inv_out=ibuf, inv_from=inv_from or 0)
    assert torch.equal(nxt, buf) and (inv is None or torch.equal(inv, ibuf))
    # Normalizer.inverse -> lincomb3 -> torch.where
    full = x['nz'].inverse(net)
    integrated = (features.lincomb3(x['cur'], x['ca'], full[:, :d], 1.0, x['prev'], x['cp']) if x['prev'] is not None
                  else features.lincomb3(x['cur'], x['ca'], full[:, :d], 1.0))
    free = torch.isin(x['node_type'][:, 0], torch.tensor(list(x['free']), dtype=torch.int64, device='cuda'))
    want = torch.where(free.unsqueeze(1).expand(-1, d), integrated, x['cur'] if x['fb'] is None else x['fb'])
    assert torch.equal(nxt, want) and (inv is None or torch.equal(inv, full[:, inv_from:]))
    # with a grad-requiring input: an autograd node, the same bits
    _, gn, gi = _advance(x)
    assert gn.grad_fn is not None and torch.equal(gn.detach(), nxt) and (inv is None or (gi.grad_fn is not None and torch.equal(gi.detach(), inv)))
    with torch.no_grad():
        _, nn_, _ = _advance(x)
    assert nn_.grad_fn is None and torch.equal(nn_, nxt)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('name', list(CASES))
def test_advance_state_backward_vs_the_derivative_table_in_fp64(name, rows):
    x = _inputs(name, rows)
    F, d, inv_from = x['F'], x['d'], x['inv_from']
    leaves, nxt, inv = _advance(x)
    _backward(x, nxt, inv, x['w_next'], x['w_inv'])
    s = x['nz']._std_with_epsilon().double().cpu()                     # the fp32 scale, as a fp64 number
    g = torch.zeros(rows, F, dtype=torch.float64)
    h = torch.zeros(rows, F, dtype=torch.float64)
    g[:, :d] = x['w_next'].double().cpu()
    if inv_from is not None:
        h[:, inv_from:] = x['w_inv'].double().cpu()
    t = x['node_type'][:, 0].cpu()
    free = torch.isin(t, torch.tensor(list(x['free']), dtype=torch.int64))
    assert bool(((t < 0) | (t >= 32)).any()) or rows == 1
    fr = free.unsqueeze(1)
    gd = g[:, :d]
    # d_net
    got = leaves['wide'].grad.cpu()
    assert float(got[:, :2].abs().max()) == 0 and float(got[:, 2 + F:].abs().max()) == 0      # the columns outside the slice
    exact = s * torch.where(fr, g + h, h)
    err = (got[:, 2:2 + F].double() - exact).abs()
    bound = 2.0 ** -23 * s * (g.abs() + h.abs())
    print(f'advance_state backward [{name}-{rows}] d_net: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all())
    # d_cur, d_prev, d_fallback (the coefficients are fp32 numbers in the kernel)
    ca, cp = (float(torch.tensor(x[k], dtype=torch.float32).double()) for k in ('ca', 'cp'))
    want = {'cur': torch.where(fr, ca * gd, torch.zeros_like(gd) if x['fallback'] else gd),
            'prev': torch.where(fr, cp * gd, torch.zeros_like(gd)) if x['prev'] is not None else None,
            'fb': torch.where(fr, torch.zeros_like(gd), gd) if x['fallback'] else None}
    for key, exact in want.items():
        if exact is None:
            assert leaves[key] is None
            continue
        got = leaves[key].grad.cpu()
        assert got.shape == (rows, d) and got.dtype == torch.float32
        assert bool(((got.double() - exact).abs() <= 2.0 ** -24 * exact.abs()).all()), key
        rest = ~free
        if key == 'prev' or (key == 'cur' and x['fallback']):
            assert bool((got[rest] == 0).all()), key
        else:                                                           # cur without a fallback, or the fallback: a copy of g
            assert torch.equal(got[rest], x['w_next'].cpu()[rest]), key
        if key == 'fb':
            assert bool((got[free] == 0).all())
    # an incoming gradient that is a transposed view gives the bits of its contiguous copy; a second run gives the same bits
    transposed = lambda w: None if w is None else w.t().contiguous().t()
    assert rows == 1 or not transposed(x['w_next']).is_contiguous()
    for g_in, h_in in ((transposed(x['w_next']), transposed(x['w_inv'])), (x['w_next'], x['w_inv'])):
        again, n2, i2 = _advance(x)
        _backward(x, n2, i2, g_in, h_in)
        for key in leaves:
            assert (leaves[key] is None) == (again[key] is None)
            assert leaves[key] is None or torch.equal(leaves[key].grad, again[key].grad), key
    # only some inputs require grad: the others get none, the wanted ones the same bits
    some = ('cur', 'fb') if x['fallback'] else ('cur',)
    part, n3, i3 = _advance(x, grads=some)
    _backward(x, n3, i3, x['w_next'], x['w_inv'])
    assert part['wide'].grad is None and (part['prev'] is None or part['prev'].grad is None)
    for key in some:
        assert torch.equal(part[key].grad, leaves[key].grad), key
    only_net, n4, i4 = _advance(x, grads=('net',))
    _backward(x, n4, i4, x['w_next'], x['w_inv'])
    assert only_net['cur'].grad is None and torch.equal(only_net['wide'].grad, leaves['wide'].grad)


# ---------------------------------------------------------------------------------------------------------------
# 3. - 7. the models
# ---------------------------------------------------------------------------------------------------------------
STATE = {'flag': 'world_pos', 'cylinder': 'velocity', 'plate': 'world_pos'}
OLD = {'flag': 'prev|world_pos'}
PER_STEP = {'flag': ('target|world_pos',), 'cylinder': ('target|velocity', 'pressure'), 'plate': ('target|world_pos',)}
MAKE = {'flag': lambda seed: synth.flag_frame(seed=seed, nx=5, ny=4), 'cylinder': lambda seed: synth.cylinder_frame(seed=seed, nx=5, ny=4),
        'plate': lambda seed: synth.plate_frame(seed=seed)}


def _state_names(kind):
    return (STATE[kind],) + ((OLD[kind],) if kind in OLD else ())


@functools.lru_cache(maxsize=None)
def _windows(kind, W, T):
    """W windows of T frames of one mesh on the device, in the layout rollout_batch takes (shared by the tests, never written)."""
    frames = [[MAKE[kind](100 + 10 * w + t) for t in range(T)] for w in range(W)]
    names = _state_names(kind) + PER_STEP[kind] + ('node_type',)
    win = {name: torch.stack([torch.stack([f[name] for f in row]) for row in frames]).cuda() for name in dict.fromkeys(names)}
    win['cells'], win['mesh_pos'] = frames[0][0]['cells'].cuda(), frames[0][0]['mesh_pos'].cuda()
    return win


@functools.lru_cache(maxsize=None)
def _warm_model(kind, connector='none'):
    """A model whose normalisers have seen one frame (without gradients), whose clusters and lazy layers exist.  Tests take a copy."""
    from hgn_amd import system_model
    cls = {'flag': system_model.FlagModel, 'cylinder': system_model.CylinderModel, 'plate': system_model.PlateModel}[kind]
    torch.manual_seed(7)
    model = cls(FG._params('sum', steps=2, connector=connector))
    frame = FG._cuda(MAKE[kind](1))
    with torch.no_grad():
        g = model.build_graph(frame, True)
        model.get_target(frame, True)
        model.learned_model(model.expand_graph(g, 0, 10 ** 9, True))
    return model


def _model(kind, connector='none'):
    base = _warm_model(kind, connector)
    model = copy.deepcopy(base)
    if connector != 'none':
        model._remote_graph._clusters, model._remote_graph._neighbors = base._remote_graph._clusters, base._remote_graph._neighbors
    return model


def _with_leaves(win, kind):
    """The windows with frame 0 of the state series replaced by fresh leaves -> (windows, {series: leaf [W, N, .]})."""
    leaves = {n: win[n][:, 0].detach().clone().requires_grad_(True) for n in _state_names(kind)}
    out = dict(win)
    for n, leaf in leaves.items():
        out[n] = torch.cat([leaf.unsqueeze(1), win[n][:, 1:]], dim=1)
    return out, leaves


def _two_grads(model):
    grads = {n: p.grad for n, p in model.learned_model.named_parameters() if p.grad is not None}
    names = sorted(grads)
    assert len(names) >= 2
    return {n: grads[n].clone() for n in (names[0], names[-1])}         # one parameter of the decoder, one of the processor


def _stats(model):
    from hgn_amd.normalizer import Normalizer
    return {n: (m._acc_sum.clone(), m._acc_sum_squared.clone(), m._acc_count.clone(), m._num_accumulations.clone(), m._host_num_acc)
            for n, m in model.named_modules() if isinstance(m, Normalizer)}


def _loop_form(model, kind, win, n_steps, start, detach=False):
    """The unroll written with what the package had before unrolled_training_step: per step and per window build_graph (+
    expand_graph, at steps that do not refresh the clusters), batching.batch_graphs, the model, get_target, _masked_mse, update and
    torch.where with the loss mask, then the next per-window frames.  ``start``: {state series: [W, N, .]}.
    -> (loss, per-step losses, the states after every step but the last [W*N, d])."""
    from hgn_amd import batching
    from hgn_amd.system_model import _masked_mse
    W = win['node_type'].shape[0]
    shared = {'cells': win['cells'], 'mesh_pos': win['mesh_pos']}
    state = [{k: v[w] for k, v in start.items()} for w in range(W)]
    losses, states = [], []
    for t in range(n_steps):
        frames = [dict(shared, node_type=win['node_type'][w, 0], **state[w], **{k: win[k][w, t] for k in PER_STEP[kind]}) for w in range(W)]
        graphs = [model.expand_graph(model.build_graph(f, False), 1 + t, 10 ** 9, False) for f in frames]
        cat = dict(shared, **{k: torch.cat([f[k] for f in frames]) for k in frames[0] if k not in shared})
        out = model(batching.batch_graphs(graphs))
        losses.append(_masked_mse(model.get_target(cat, False), out, model._loss_mask(cat)))
        if t + 1 == n_steps:
            break
        cur = cat[STATE[kind]]
        predicted = FG._first(model.update(cat, out))
        keep = cat['target|world_pos'] if kind == 'plate' else cur      # plate: the scripted motion
        nxt = torch.where(model._loss_mask(cat).unsqueeze(1).expand(-1, cur.shape[1]), predicted, keep)
        if detach:
            nxt, cur = nxt.detach(), cur.detach()
        states.append(nxt.detach())
        N = nxt.shape[0] // W
        state = [{STATE[kind]: nxt[w * N:(w + 1) * N], **({OLD[kind]: cur[w * N:(w + 1) * N]} if kind in OLD else {})} for w in range(W)]
    per = torch.stack(losses)
    return per.mean(), per.detach(), states


@pytest.mark.parametrize('kind', ['flag', 'cylinder'])
def test_one_unrolled_step_is_training_step_on_the_batched_graph(kind):
    """3. Loss, two parameter gradients and the normaliser states afterwards, bit for bit (is_training=True on both routes)."""
    a, b = _model(kind), _model(kind)
    win = _windows(kind, 2, 2)
    loss_a, per = a.unrolled_training_step(win, 1)
    frames = {k: (v if k in ('cells', 'mesh_pos') else v[:, 0]) for k, v in win.items()}
    loss_b = b.training_step(b.expand_graph_batch(b.build_graph_batch(frames, True), 2, 0, 1, True), b.flatten_frames(frames))
    assert bool(torch.isfinite(loss_a)) and float(loss_a.detach()) > 0 and loss_a.requires_grad
    assert torch.equal(loss_a, loss_b) and per.shape == (1,) and not per.requires_grad and torch.equal(per[0], loss_b.detach())
    loss_a.backward()
    loss_b.backward()
    ga, gb = _two_grads(a), _two_grads(b)
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert float(ga[n].abs().max()) > 0 and torch.equal(ga[n], gb[n]), n
    sa, sb, before = _stats(a), _stats(b), _stats(_warm_model(kind))
    assert sa.keys() == sb.keys()
    for n in sa:
        assert all(torch.equal(x, y) for x, y in zip(sa[n][:4], sb[n][:4])) and sa[n][4] == sb[n][4], n
    assert sa['_output_normalizer'][4] == before['_output_normalizer'][4] + 1          # and the step did accumulate


@pytest.mark.parametrize('kind,n_steps', [('flag', 3), ('cylinder', 2)])
def test_lockstep_unroll_equals_the_loop_written_per_window(kind, n_steps):
    """4. through_state=True, W = 2, frozen statistics."""
    model = _model(kind)
    win = _windows(kind, 2, n_steps)
    wa, la = _with_leaves(win, kind)
    loss_a, per_a = model.unrolled_training_step(wa, n_steps, through_state=True, is_training=False)
    loss_a.backward()
    ga = _two_grads(model)
    model.zero_grad(set_to_none=True)
    _, lb = _with_leaves(win, kind)
    loss_b, per_b, _ = _loop_form(model, kind, win, n_steps, lb)
    loss_b.backward()
    gb = _two_grads(model)
    assert per_a.shape == (n_steps,) and not per_a.requires_grad
    assert torch.equal(loss_a, loss_b) and torch.equal(per_a, per_b)
    assert torch.equal(loss_a.detach(), per_a.mean())
    for n in la:
        assert la[n].grad is not None and float(la[n].grad.abs().max()) > 0, n
        err = H.rel_err(la[n].grad, lb[n].grad)
        print(f'unroll[{kind}] d loss / d {n}: lock step vs loop rel_err={err:.3e} bit_equal={bool(torch.equal(la[n].grad, lb[n].grad))}')
        assert err <= TOL_GRAD, n
    for n in ga:
        err = H.rel_err(ga[n], gb[n])
        print(f'unroll[{kind}] d loss / d {n}: lock step vs loop rel_err={err:.3e} bit_equal={bool(torch.equal(ga[n], gb[n]))}')
        assert float(gb[n].abs().max()) > 0 and err <= TOL_GRAD, n


def test_two_step_unroll_vs_fp64_oracle():
    """5. Flag, W = 1, n_steps = 2, through_state=True: the two-term mean loss and its gradients against the fp64 oracle with the
    HIP forward's ReLU gates."""
    frame, base = FG._system('flag', 'sum')
    model = copy.deepcopy(base)
    model.zero_grad(set_to_none=True)
    target2 = synth.flag_frame(seed=9, nx=5, ny=4)['target|world_pos']
    leaves = {n: frame[n].cuda().clone().requires_grad_(True) for n in FG.STATE['flag']}
    two = lambda first, second: torch.stack([first, second]).unsqueeze(0)
    win = {'world_pos': two(leaves['world_pos'], leaves['world_pos'].detach()),
           'prev|world_pos': two(leaves['prev|world_pos'], leaves['prev|world_pos'].detach()),
           'target|world_pos': two(frame['target|world_pos'], target2).cuda(),
           'node_type': two(frame['node_type'], frame['node_type']).cuda(), 'cells': frame['cells'].cuda(), 'mesh_pos': frame['mesh_pos'].cuda()}
    (loss, per), gates, winners = FG._logged(model, lambda: model.unrolled_training_step(win, 2, through_state=True, is_training=False))
    loss.backward()

    ff = FG._oracle_features('flag', model)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = FG._leaves(frame, FG.STATE['flag'], dict(dtype=torch.float64))
    free = (frame['node_type'][:, 0] == 0).unsqueeze(1)

    def mse(target, out):
        m = free.to(out.dtype)
        return (((out - target) ** 2) * m).sum() / (m.sum() * out.shape[1])

    def step(fr):
        out = O.mesh_graph_net(sd, FO._as_multigraph(ff.build_graph(fr, False)), 'none', 'sum')
        return out, mse(ff.get_target(fr, False), out)
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners):
        out1, l1 = step(fo)
        nxt = torch.where(free, ff.update(fo, out1), fo['world_pos'])
        _, l2 = step({**fo, 'world_pos': nxt, 'prev|world_pos': fo['world_pos'], 'target|world_pos': target2.double()})
        loss64 = (l1 + l2) / 2
    assert all(len(v) == 0 for v in gt.gates.values()), 'decisions left over'
    loss64.backward()
    tid = 'test_two_step_unroll_vs_fp64_oracle'
    assert H.report(tid, 'loss', loss, loss64)['norm'] <= TOL_GRAD
    assert H.report(tid, 'per-step losses', per, torch.stack([l1, l2]))['norm'] <= TOL_GRAD
    for n in FG.STATE['flag']:
        assert leaves[n].grad is not None, n
        assert H.report(tid, f'd loss / d {n}', leaves[n].grad, fo[n].grad)['norm'] <= TOL_GRAD, n
    k = FG._two_params(sd)[0]
    assert H.report(tid, f'd loss / d {k}', dict(model.learned_model.named_parameters())[k].grad, sd[k].grad)['norm'] <= TOL_GRAD


def test_push_forward_states_are_the_rollouts_and_every_step_trains_alone(monkeypatch):
    """6. through_state=False on flag, W = 2, n_steps = 3."""
    from hgn_amd import features
    from hgn_amd.system_model import _masked_mse
    model = _model('flag')
    W, n_steps = 2, 3
    win = _windows('flag', W, n_steps)
    N = win['node_type'].shape[2]
    wa, leaves = _with_leaves(win, 'flag')
    real, states = features.advance_state, []

    def spy(*args, **kw):
        res = real(*args, **kw)
        states.append(res[0].detach().clone())
        return res
    monkeypatch.setattr(features, 'advance_state', spy)
    loss, per = model.unrolled_training_step(wa, n_steps, through_state=False, is_training=False)
    monkeypatch.setattr(features, 'advance_state', real)
    loss.backward()
    got = _two_grads(model)
    model.zero_grad(set_to_none=True)
    # the intermediate states are those of the rollout (which records the state BEFORE every step)
    assert len(states) == n_steps - 1
    pred = model.rollout_batch(win, n_steps)[0]['pred_pos']
    for t, s in enumerate(states):
        assert torch.equal(s.view(W, N, 3), pred[:, t + 1]), t
    # every step alone, at those detached states
    cur, prev = [win['world_pos'][:, 0]] + [s.view(W, N, 3) for s in states], [win['prev|world_pos'][:, 0], win['world_pos'][:, 0]] + [s.view(W, N, 3) for s in states[:-1]]
    first = {n: win[n][:, 0].detach().clone().requires_grad_(True) for n in leaves}
    for t in range(n_steps):
        frame = {'cells': win['cells'], 'mesh_pos': win['mesh_pos'], 'node_type': win['node_type'][:, 0],
                 'world_pos': first['world_pos'] if t == 0 else cur[t], 'prev|world_pos': first['prev|world_pos'] if t == 0 else prev[t],
                 'target|world_pos': win['target|world_pos'][:, t]}
        flat = model.flatten_frames(frame)
        out = model(model.expand_graph_batch(model.build_graph_batch(frame, False), W, 1 + t, 10 ** 9, False))
        single = _masked_mse(model.get_target(flat, False), out, model._loss_mask(flat))
        assert H.rel_err(per[t], single) <= 1e-6, t
        (single / n_steps).backward()
    want = _two_grads(model)
    for n in got:
        assert float(want[n].abs().max()) > 0 and H.rel_err(got[n], want[n]) <= TOL_GRAD, n
    for n in leaves:                                                    # the initial state sees step 0 alone
        assert float(first[n].grad.abs().max()) > 0 and H.rel_err(leaves[n].grad, first[n].grad) <= TOL_GRAD, n
    # through the state, the later steps reach the initial state as well
    model.zero_grad(set_to_none=True)
    wb, through = _with_leaves(win, 'flag')
    model.unrolled_training_step(wb, n_steps, through_state=True, is_training=False)[0].backward()
    assert H.rel_err(through['world_pos'].grad, first['world_pos'].grad) > 1e-3


@pytest.mark.parametrize('kind,connector', [('plate', 'none'), ('flag', 'hyper')], ids=['plate', 'flag-hyper'])
def test_push_forward_works_where_the_graph_is_not_differentiable(kind, connector):
    """6. PlateModel and a model with a connector: through_state=False trains, through_state=True is refused before any launch."""
    from hgn_amd import _lib
    model = _model(kind, connector)
    W, n_steps = 2, 2
    win = _windows(kind, W, n_steps)
    before = _stats(model)
    with pytest.raises(_lib.HgnError, match='through_state'):
        model.unrolled_training_step(win, n_steps, through_state=True, is_training=False)
    after = _stats(model)
    assert all(before[n][4] == after[n][4] for n in before)            # refused before anything ran
    loss, per = model.unrolled_training_step(win, n_steps, through_state=False, is_training=False)
    assert bool(torch.isfinite(loss)) and per.shape == (n_steps,)
    loss.backward()
    grads = _two_grads(model)
    assert all(float(g.abs().max()) > 0 for g in grads.values())
    model.zero_grad(set_to_none=True)
    start = {n: win[n][:, 0] for n in _state_names(kind)}
    loop_loss, loop_per, _ = _loop_form(model, kind, win, n_steps, start, detach=True)
    assert torch.equal(loss, loop_loss) and torch.equal(per, loop_per)
    # one step has no state to differentiate through: allowed in either mode
    one, _ = model.unrolled_training_step(win, 1, through_state=True, is_training=False)
    assert bool(torch.isfinite(one))


def test_unrolled_step_refuses_windows_that_are_too_short_and_a_balancer():
    from hgn_amd import _lib, system_model
    model = _model('flag')
    win = _windows('flag', 2, 2)
    with pytest.raises(ValueError, match='unrolled_training_step'):
        model.unrolled_training_step(win, 3)
    with pytest.raises(ValueError, match='unrolled_training_step'):
        model.unrolled_training_step(win, 0)
    params = FG._params('sum', steps=1)
    params['graph_balancer'] = {'algorithm': 'random', 'frequency': 1, 'remove_edges': False, 'random': {'edge_amount': 4}}
    with pytest.raises(_lib.HgnError, match='expand_graph_batch.*balancer'):
        system_model.FlagModel(params).unrolled_training_step(win, 2, through_state=False)


@pytest.mark.parametrize('kind', ['flag', 'cylinder'])
def test_an_unrolled_step_leaves_the_rollout_alone(kind):
    """7."""
    model = _model(kind)
    win = _windows(kind, 2, 3)
    key = 'pred_pos' if kind == 'flag' else 'pred_velocity'
    ops, errors = model.rollout_batch(win, 3)
    before, before_errors = ops[key].clone(), errors.clone()
    wa, _ = _with_leaves(win, kind)
    model.unrolled_training_step(wa, 3, through_state=True, is_training=False)[0].backward()
    ops, errors = model.rollout_batch(win, 3)
    assert torch.equal(ops[key], before) and torch.equal(errors, before_errors)
