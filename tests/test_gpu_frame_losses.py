"""Per-frame losses on the GPU: features.frame_losses (hgn_frame_losses / hgn_frame_losses_bwd) and what the system models build
on it -- `loss_kernel`, training_step_batch, validation_step_batch, one_step_errors.

Yardsticks.
* tests/loss_statement.py: the header's definition in numpy fp64 on the fp32 inputs; the updated state is taken as the fp32 bits of
  features.advance_state.  Forward entries: relative error <= 2^-23 (one fp32 rounding of a double quotient is 2^-24, the double sums
  add about n 2^-53; the bound is twice that).  `count` is exact.  d_net: element-wise relative <= 4 * 2^-24 (three fp32 roundings: the
  difference, w, the product); d_target is its bit-wise negation; rows that are not free are exactly zero.
* Position independence and repeatability: torch.equal.
* The torch path of the parent (`_masked_mse` and its autograd gradient) as a sanity check: value 1e-5, gradient 1e-6 of the fp64
  value (the two sides together make about eight fp32 roundings, 5e-7).
* Models: 20-node synthetic frames as in tests/test_gpu_unrolled_training.py (the plate frame has 158 nodes), B = 3; the project's parity
  tolerance 1e-5 where two routes differ in the order of fp32 operations."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import loss_statement as LS
from tests import test_gpu_unrolled_training as UT

pytestmark = pytest.mark.gpu
TOL_FWD = 2.0 ** -23
TOL_BWD = 4 * 2.0 ** -24
TOL_PARITY = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


# ---------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 5), (63, 3), (64, 2), (65, 3), (257, 2), (3000, 2)]          # (rows_per_frame, B); 3000 rows: 11 full chunks + 184
CONFIGS = {'flag': dict(F=3, d=3, prev=True, ca=2.0, cp=-1.0, free=(0,)),
           'cylinder': dict(F=3, d=2, prev=False, ca=1.0, cp=0.0, free=(0, 5)),
           'plate': dict(F=3, d=3, prev=False, ca=1.0, cp=0.0, free=(0,)),
           'one': dict(F=1, d=1, prev=False, ca=1.0, cp=0.0, free=(0, 3)),
           'wide': dict(F=32, d=32, prev=True, ca=2.0, cp=-1.0, free=(0,))}
KINDS = torch.tensor([0, 0, 0, 1, 3, 5, 40, -1], dtype=torch.int64)               # 40, -1: outside the bit mask, never free
CASES = [(name, rpf, B) for name in CONFIGS for rpf, B in SHAPES]
IDS = [f'{name}-{rpf}x{B}' for name, rpf, B in CASES]


@functools.lru_cache(maxsize=None)
def _normalizer(F):
    """A warmed output normaliser with statistics that differ from column to column."""
    from hgn_amd.normalizer import Normalizer
    gen = torch.Generator().manual_seed(F)
    nz = Normalizer(F, 'output_normalizer')
    scale, shift = 0.3 + 0.37 * torch.arange(F), torch.linspace(-2.0, 4.0, F)
    nz((torch.randn(257, F, generator=gen) * scale + shift).cuda())
    return nz


@functools.lru_cache(maxsize=None)
def _inputs(name, rpf, B, seed=0):
    """The inputs of one case on the device (shared by the tests, never written).  The network output is a column slice of a wider
    slab and the node types are column 0 of a two-column matrix (ldt = 2)."""
    c = CONFIGS[name]
    F, d, rows = c['F'], c['d'], rpf * B
    gen = torch.Generator().manual_seed(100000 * seed + 1000 * rpf + 10 * B + F + d)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()
    types = torch.full((rows, 2), 7, dtype=torch.int64)
    types[:, 0] = KINDS[torch.randint(0, len(KINDS), (rows,), generator=gen)]
    types[0, 0] = 0                                                         # at least one free row in the batch
    return dict(c, name=name, rpf=rpf, B=B, wide=rnd(rows, F + 4), target=rnd(rows, F), cur=rnd(rows, d),
                prev=rnd(rows, d) if c['prev'] else None, state_target=rnd(rows, d), types=types.cuda(), nz=_normalizer(F))


def _net(x, wide=None):
    return (x['wide'] if wide is None else wide)[:, 2:2 + x['F']]


def _state(x, rows=slice(None)):
    return (x['nz'], x['cur'][rows], x['d'], x['ca'], x['prev'][rows] if x['prev'] is not None else None, x['cp'], x['state_target'][rows])


def _call(x, with_state=True, rows=slice(None), frames=True, wide=None, target=None):
    """frame_losses on the case (or on the rows of one frame, as a single frame)."""
    from hgn_amd import features
    return features.frame_losses(_net(x, wide)[rows], (x['target'] if target is None else target)[rows], x['types'][rows, :1], x['free'],
                                 x['rpf'] if frames else None, _state(x, rows) if with_state else None)


def _statement(x):
    from hgn_amd import features
    v, _ = features.advance_state(_net(x), x['nz'], x['cur'], x['d'], x['ca'], x['prev'], x['cp'], x['types'][:, :1], x['free'])
    return LS.losses(_net(x), x['target'], x['types'][:, 0], x['free'], x['rpf'], v, x['state_target'])


def _assert_close(got, want, rel, what):
    """|got - want| <= rel * |want| element-wise; NaN exactly where the statement has NaN.  -> the worst error / bound."""
    got = got.detach().double().cpu().numpy().reshape(np.shape(want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    err, bound = np.abs(got - want)[~nan], rel * np.abs(want)[~nan]
    assert bool((err <= bound).all()), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def _same(a, b):
    """Equal bits (NaN entries compare by their place)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0)) \
        and torch.equal(torch.isnan(a.float()), torch.isnan(b.float()))


@pytest.mark.parametrize('name,rpf,B', CASES, ids=IDS)
def test_forward_vs_the_statement(name, rpf, B):
    from hgn_amd.system_model import _masked_mse
    x = _inputs(name, rpf, B)
    assert rpf * B == 1 or not _net(x).is_contiguous()
    assert x['types'][:, :1].stride(0) == 2 and bool((x['types'][:, 0] < 0).any() or rpf * B < 20) and bool((x['types'][:, 0] >= 32).any() or rpf * B < 20)
    res = _call(x)
    loss, state_err, count = _statement(x)
    assert res.loss.shape == () and res.per_frame.shape == (B,) and res.state_error.shape == () and res.state_per_frame.shape == (B,)
    assert res.count.shape == (B + 1,) and res.count.dtype == torch.int64 and res.loss.dtype == torch.float32
    assert res.loss.grad_fn is None and not res.loss.requires_grad                   # no autograd node without a grad-requiring input
    assert np.array_equal(res.count.cpu().numpy(), count)
    worst = max(_assert_close(res.per_frame, loss[:B], TOL_FWD, 'per_frame'), _assert_close(res.loss, loss[B], TOL_FWD, 'loss'),
                _assert_close(res.state_per_frame, state_err[:B], TOL_FWD, 'state_per_frame'),
                _assert_close(res.state_error, state_err[B], TOL_FWD, 'state_error'))
    print(f'frame_losses forward [{name}-{rpf}x{B}]: worst error / bound = {worst:.3f}; frames without a free row: {int((count[:B] == 0).sum())}')
    # without the state part: the same loss bits, no state outputs; a second run: the same bits
    bare = _call(x, with_state=False)
    assert bare.state_error is None and bare.state_per_frame is None
    again = _call(x)
    for a, b in ((bare.loss, res.loss), (bare.per_frame, res.per_frame), (again.loss, res.loss), (again.per_frame, res.per_frame),
                 (again.state_error, res.state_error), (again.state_per_frame, res.state_per_frame)):
        assert _same(a, b)
    assert torch.equal(bare.count, res.count) and torch.equal(again.count, res.count)
    # sanity: the torch path of the parent
    t = x['types'][:, 0]
    mask = torch.isin(t, torch.tensor(list(x['free']), device='cuda'))
    torch_loss = _masked_mse(x['target'], _net(x), mask)
    assert abs(float(torch_loss) - loss[B]) <= 1e-5 * abs(loss[B])


def _backward(x, g_loss, frame, g_frame, rows=slice(None), frames=True):
    """-> (d_net [rows, F], d_target, the gradient of the slab outside the slice) for upstream g_loss on `loss` and g_frame on
    per_frame[frame] (None: absent)."""
    wide, target = x['wide'].detach().clone().requires_grad_(True), x['target'].detach().clone().requires_grad_(True)
    res = _call(x, rows=rows, frames=frames, wide=wide, target=target)
    assert res.loss.requires_grad and res.per_frame.requires_grad
    assert not res.state_error.requires_grad and not res.state_per_frame.requires_grad and not res.count.requires_grad
    total = 0
    if g_loss is not None:
        total = total + g_loss * res.loss
    if g_frame is not None:
        total = total + g_frame * res.per_frame[frame]
    total.backward()
    F = x['F']
    outside = torch.cat([wide.grad[:, :2], wide.grad[:, 2 + F:]], dim=1)
    return wide.grad[:, 2:2 + F][rows], target.grad[rows], outside


@pytest.mark.parametrize('name,rpf,B', CASES, ids=IDS)
def test_backward_vs_the_statement(name, rpf, B):
    from hgn_amd.system_model import _masked_mse
    x = _inputs(name, rpf, B)
    F = x['F']
    _, _, count = _statement(x)
    live = [f for f in range(B) if count[f] > 0]
    frame = live[-1]
    free = LS.free_rows(x['types'][:, 0], x['free'])
    for what, g_loss, g_frame in (('all rows', 0.7, None), ('one frame', None, 1.3), ('both', 0.7, 1.3)):
        g = np.zeros(B + 1)
        g[B], g[frame] = g_loss or 0.0, g_frame or 0.0
        want = LS.d_net(_net(x), x['target'], x['types'][:, 0], x['free'], rpf, g)
        d_net, d_target, outside = _backward(x, g_loss, frame, g_frame)
        worst = _assert_close(d_net, want, TOL_BWD, what)
        print(f'frame_losses backward [{name}-{rpf}x{B}, upstream on {what}]: worst error / bound = {worst:.3f}')
        assert d_net.dtype == torch.float32 and float(outside.abs().max()) == 0
        assert torch.equal(d_target.view(torch.int32), d_net.view(torch.int32) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device='cuda'))
        rest = torch.from_numpy(~free).cuda()
        assert bool((d_net[rest] == 0).all()) and bool((d_target[rest] == 0).all())
        if g_frame is not None and g_loss is None:                       # and nothing reaches the other frames
            other = torch.ones(rpf * B, dtype=torch.bool, device='cuda')
            other[frame * rpf:(frame + 1) * rpf] = False
            assert bool((d_net[other] == 0).all())
        again = _backward(x, g_loss, frame, g_frame)
        assert torch.equal(again[0], d_net) and torch.equal(again[1], d_target)
    # sanity: the autograd gradient of the torch path of the parent, upstream 1 on the loss over all rows
    want = LS.d_net(_net(x), x['target'], x['types'][:, 0], x['free'], rpf, np.append(np.zeros(B), 1.0))
    d_net, _, _ = _backward(x, 1.0, frame, None)
    wide = x['wide'].detach().clone().requires_grad_(True)
    mask = torch.isin(x['types'][:, 0], torch.tensor(list(x['free']), device='cuda'))
    _masked_mse(x['target'], _net(x, wide), mask).backward()
    gap = (d_net.double() - wide.grad[:, 2:2 + F].double()).abs().cpu().numpy()
    assert bool((gap[want != 0] <= 1e-6 * np.abs(want[want != 0])).all())


def test_only_the_gradients_asked_for_and_no_launch_for_unused_outputs(monkeypatch):
    from hgn_amd import _lib
    x = _inputs('flag', 65, 3)
    calls = []
    real = _lib.lib().hgn_frame_losses_bwd
    monkeypatch.setattr(_lib.lib(), 'hgn_frame_losses_bwd', lambda *a: calls.append(a) or real(*a))
    full, _, _ = _backward(x, 0.7, 0, None)
    assert len(calls) == 1                                               # one launch for both gradients
    wide = x['wide'].detach().clone().requires_grad_(True)
    res = _call(x, wide=wide)                                            # the target needs no gradient: d_target is not formed
    (0.7 * res.loss).backward()
    assert len(calls) == 2 and calls[1][14] is None and calls[1][12] is not None
    assert torch.equal(wide.grad[:, 2:5], full)
    target = x['target'].detach().clone().requires_grad_(True)
    res = _call(x, target=target)
    (0.7 * res.loss).backward()
    assert len(calls) == 3 and calls[2][12] is None and torch.equal(target.grad.view(torch.int32) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device='cuda'),
                                                                    full.view(torch.int32))
    # a graph that uses no differentiable output of the node launches nothing in the backward pass
    wide = x['wide'].detach().clone().requires_grad_(True)
    res = _call(x, wide=wide)
    (wide.sum() + res.state_error + res.count[0]).backward()
    assert len(calls) == 3 and bool((wide.grad == 1).all())
    with torch.no_grad():
        res = _call(x, wide=wide)
    assert res.loss.grad_fn is None


def test_a_frame_without_a_free_row_is_nan_and_leaves_the_others_alone():
    from hgn_amd import features
    x = dict(_inputs('flag', 65, 3))
    res = _call(x)
    types = x['types'].clone()
    types[65:130, 0] = 1                                                # frame 1: no free row
    x['types'] = types
    got = _call(x)
    loss, state_err, count = _statement(x)
    assert count[1] == 0 and np.isnan(loss[1]) and np.isnan(state_err[1]) and not np.isnan(loss[[0, 2, 3]]).any()
    assert np.array_equal(got.count.cpu().numpy(), count)
    for g, w in ((got.per_frame, loss[:3]), (got.loss, loss[3]), (got.state_per_frame, state_err[:3]), (got.state_error, state_err[3])):
        _assert_close(g, w, TOL_FWD, 'frame without a free row')
    for f in (0, 2):                                                    # the other frames: the bits they had
        assert torch.equal(got.per_frame[f], res.per_frame[f]) and torch.equal(got.state_per_frame[f], res.state_per_frame[f])
        assert torch.equal(got.count[f], res.count[f])
    d_net, d_target, _ = _backward(x, 0.7, 2, 1.3)
    assert bool((d_net[65:130] == 0).all()) and bool(torch.isfinite(d_net).all()) and float(d_net.abs().max()) > 0
    # a batch without any free row: every entry NaN, zero gradients
    none = features.frame_losses(_net(x)[65:130], x['target'][65:130], types[65:130, :1], x['free'], 13)
    assert bool(torch.isnan(none.per_frame).all()) and bool(torch.isnan(none.loss)) and int(none.count.abs().max()) == 0


@pytest.mark.parametrize('name', list(CONFIGS))
@pytest.mark.parametrize('rpf,B', [(65, 3), (3000, 2)])
def test_a_frame_gets_the_same_bits_alone_and_inside_the_batch(name, rpf, B):
    x = _inputs(name, rpf, B)
    batch = _call(x)
    for f in range(B):
        rows = slice(f * rpf, (f + 1) * rpf)
        alone = _call(x, rows=rows, frames=False)
        assert alone.per_frame.shape == (1,) and alone.count.shape == (2,)
        for a, b in ((alone.per_frame[0], batch.per_frame[f]), (alone.state_per_frame[0], batch.state_per_frame[f]),
                     (alone.loss, batch.per_frame[f]), (alone.state_error, batch.state_per_frame[f])):
            assert torch.equal(a, b) and bool(torch.isfinite(a)), f
        assert torch.equal(alone.count[0], batch.count[f]) and torch.equal(alone.count[1], batch.count[f])
        in_batch = _backward(x, None, f, 1.3)
        on_its_own = _backward(x, None, 0, 1.3, rows=rows, frames=False)
        assert float(in_batch[0][rows].abs().max()) > 0
        assert torch.equal(in_batch[0][rows], on_its_own[0]) and torch.equal(in_batch[1][rows], on_its_own[1]), f


def test_the_forward_is_capturable_and_replays_on_new_inputs():
    x = dict(_inputs('flag', 65, 3))
    fresh = _inputs('flag', 65, 3, seed=1)
    names = ('wide', 'target', 'cur', 'prev', 'state_target', 'types')
    for n in names:
        x[n] = x[n].clone()                                             # static buffers of the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _call(x)
    for n in names:
        x[n].copy_(fresh[n])
    graph.replay()
    torch.cuda.synchronize()
    eager = _call(fresh)
    first = _call(_inputs('flag', 65, 3))
    assert not torch.equal(eager.per_frame, first.per_frame)
    for a, b in zip(captured, eager):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
SERIES = {kind: UT._state_names(kind) + UT.PER_STEP[kind] + ('node_type',) for kind in ('flag', 'cylinder', 'plate')}


@functools.lru_cache(maxsize=None)
def _frames(kind, count, seed=200):
    """-> (the frames one by one, on the device; the same stacked [B, N, .] with `cells` and `mesh_pos` given once)."""
    singles = [UT.FG._cuda(UT.MAKE[kind](seed + b)) for b in range(count)]
    shared = {'cells': singles[0]['cells'], 'mesh_pos': singles[0]['mesh_pos']}
    singles = [dict(f, **shared) for f in singles]
    stacked = dict(shared, **{name: torch.stack([f[name] for f in singles]) for name in dict.fromkeys(SERIES[kind])})
    return singles, stacked


def _trajectory(kind, count):
    singles, _ = _frames(kind, count)
    return {name: torch.stack([f[name] for f in singles]) for name in singles[0]}


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize('kind', ['flag', 'cylinder', 'plate'])
def test_validation_step_batch_vs_the_statement_and_validation_step(kind):
    from hgn_amd import features
    B = 3
    singles, stacked = _frames(kind, B)
    model = UT._model(kind)
    ls = model._LOCKSTEP
    graph = model.expand_graph_batch(model.build_graph_batch(stacked, False), B, 0, B, False)
    flat = model.flatten_frames(stacked)
    loss, state_error = model.validation_step_batch(graph, flat, B)
    assert loss.shape == (B,) and state_error.shape == (B,) and loss.dtype == state_error.dtype == torch.float32 and loss.is_cuda
    with torch.no_grad():
        out = model(graph)
        target = model.get_target(flat, False)
        v, _ = features.advance_state(out, model._output_normalizer, flat[ls.state], ls.d, ls.ca, flat[ls.prev] if ls.prev else None, ls.cp,
                                      flat['node_type'], ls.free_types)
    want_loss, want_err, count = LS.losses(out, target, flat['node_type'], ls.free_types, out.shape[0] // B, v, flat[ls.target])
    assert (count[:B] > 0).all() and count[B] < out.shape[0]
    _assert_close(loss, want_loss[:B], TOL_FWD, 'loss')
    _assert_close(state_error, want_err[:B], TOL_FWD, 'state_error')
    # against validation_step on every frame's own graph.  The flag's node-dynamic normaliser accumulates on every build, so there
    # the two routes run on twin models, one frame per chunk: equal statistics at every frame, only the loss differs.
    if kind == 'flag':
        a, b = UT._model(kind), UT._model(kind)
        pairs = []
        for frame in singles:
            one = {name: (t if name in ('cells', 'mesh_pos') else t.unsqueeze(0)) for name, t in frame.items()}
            got = a.validation_step_batch(a.expand_graph_batch(a.build_graph_batch(one, False), 1, 0, B, False), a.flatten_frames(one), 1)
            pairs.append(((got[0][0], got[1][0]), b.validation_step(b.expand_graph(b.build_graph(frame, False), 0, B, False), frame)))
    else:
        pairs = [((loss[i], state_error[i]), model.validation_step(model.expand_graph(model.build_graph(frame, False), 0, B, False), frame))
                 for i, frame in enumerate(singles)]
    for i, (got, want) in enumerate(pairs):
        gaps = (_rel(got[0], want[0]), _rel(got[1], want[1]))
        print(f'validation_step_batch [{kind}, frame {i}] vs validation_step: loss rel {gaps[0]:.2e}, state error rel {gaps[1]:.2e}')
        assert want[0] > 0 and want[1] > 0 and max(gaps) <= TOL_PARITY, (i, gaps)


def test_one_step_errors_equals_its_chunks_and_the_loop():
    kind, T, M = 'flag', 5, 2
    trajectory = _trajectory(kind, T)
    a, b = UT._model(kind), UT._model(kind)
    got = a.one_step_errors(trajectory, batch=M)
    assert got.shape == (T, 2) and got.dtype == torch.float32 and got.device.type == 'cpu' and bool((got > 0).all())
    chunks = []
    for first in range(0, T, M):
        chunk = {name: (t[0] if name == 'cells' else t[first:first + M]) for name, t in trajectory.items()}
        count = chunk['node_type'].shape[0]
        graph = b.expand_graph_batch(b.build_graph_batch(chunk, False), count, first, T, False)
        chunks.append(torch.stack(b.validation_step_batch(graph, b.flatten_frames(chunk), count), dim=1))
    assert [c.shape[0] for c in chunks] == [2, 2, 1] and torch.equal(got, torch.cat(chunks).cpu())
    # num_timesteps: the first frames only
    c = UT._model(kind)
    assert torch.equal(c.one_step_errors(trajectory, batch=M, num_timesteps=4), torch.cat(chunks[:2]).cpu())
    # batch=None: the reference's loop over validation_step, exactly
    a, b = UT._model(kind), UT._model(kind)
    loop = a.one_step_errors(trajectory)
    want = []
    for t in range(T):
        frame = {name: series[t] for name, series in trajectory.items()}
        want.append(list(b.validation_step(b.expand_graph(b.build_graph(frame, False), t, T, False), frame)))
    assert torch.equal(loop, torch.tensor(want, dtype=torch.float32))
    gap = float(((got - loop).abs() / loop.abs()).max())
    print(f'one_step_errors [flag, T = {T}]: batch = {M} against the per-frame loop, worst relative gap {gap:.2e} '
          '(the node-dynamic normaliser accumulates once per chunk on the batched route)')


def test_one_step_errors_ignores_batch_for_a_model_with_a_connector(monkeypatch):
    model = UT._model('flag', 'hyper')
    trajectory = _trajectory('flag', 3)
    calls = {'frame': 0}
    real = model.validation_step

    def spy(graph, frame):
        calls['frame'] += 1
        return real(graph, frame)

    def refuse(*args, **kw):
        raise AssertionError('the batched route was taken')
    monkeypatch.setattr(model, 'validation_step', spy)
    monkeypatch.setattr(model, 'build_graph_batch', refuse)
    monkeypatch.setattr(model, 'validation_step_batch', refuse)
    got = model.one_step_errors(trajectory, batch=2)
    assert calls['frame'] == 3 and got.shape == (3, 2) and bool(torch.isfinite(got).all()) and bool((got > 0).all())


@pytest.mark.parametrize('kind', ['flag', 'cylinder'])
def test_training_step_batch_is_training_step_with_the_kernel_and_reports_every_frame(kind, monkeypatch):
    from hgn_amd import features
    B = 3
    _, stacked = _frames(kind, B)
    a, b = UT._model(kind), UT._model(kind)
    seen = []
    real = features.frame_losses
    monkeypatch.setattr(features, 'frame_losses', lambda *args, **kw: seen.append((args, real(*args, **kw))) or seen[-1][1])
    loss_a, per_frame = a.training_step_batch(a.expand_graph_batch(a.build_graph_batch(stacked, True), B, 0, 1, True), a.flatten_frames(stacked), B)
    b.loss_kernel = True
    loss_b = b.training_step(b.expand_graph_batch(b.build_graph_batch(stacked, True), B, 0, 1, True), b.flatten_frames(stacked))
    assert len(seen) == 2 and seen[0][0][4] == stacked['node_type'].shape[1] and len(seen[1][0]) == 4      # B frames; one frame
    assert loss_a.requires_grad and loss_b.requires_grad and torch.equal(loss_a, loss_b) and float(loss_a.detach()) > 0
    assert per_frame.shape == (B,) and not per_frame.requires_grad
    (out, target, node_type, free), res = seen[0][0][:4], seen[0][1]
    want, _, count = LS.losses(out, target, node_type, free, out.shape[0] // B)
    _assert_close(per_frame, want[:B], TOL_FWD, 'per_frame')
    _assert_close(loss_a, want[B], TOL_FWD, 'loss')
    assert np.array_equal(res.count.cpu().numpy(), count)
    loss_a.backward()
    loss_b.backward()
    ga, gb = UT._two_grads(a), UT._two_grads(b)
    for n in ga:
        assert float(ga[n].abs().max()) > 0 and torch.equal(ga[n], gb[n]), n


def _all_grads(model):
    return {n: p.grad.clone() for n, p in model.learned_model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', ['flag', 'cylinder'])
def test_loss_kernel_off_is_the_path_of_before_and_on_agrees_with_it(kind):
    B = 3
    _, stacked = _frames(kind, B)
    win = UT._windows(kind, 2, 2)

    def single(model):
        return model.training_step(model.expand_graph_batch(model.build_graph_batch(stacked, True), B, 0, 1, True), model.flatten_frames(stacked))

    def unrolled(model):
        return model.unrolled_training_step(win, 2, through_state=True, is_training=False)[0]
    for what, step in (('training_step', single), ('unrolled_training_step(W = 2, n_steps = 2)', unrolled)):
        runs = {}
        for key, setting in (('untouched', None), ('off', False), ('on', True), ('on again', True)):
            model = UT._model(kind)
            if setting is not None:
                model.loss_kernel = setting
            assert ('loss_kernel' in model.__dict__) == (setting is not None)
            loss = step(model)
            loss.backward()
            runs[key] = (loss.detach().clone(), _all_grads(model), UT._two_grads(model))
        # off: the bits of a model on which the attribute was never touched
        assert torch.equal(runs['off'][0], runs['untouched'][0]) and runs['off'][1].keys() == runs['untouched'][1].keys()
        assert len(runs['off'][1]) >= 2 and all(torch.equal(g, runs['untouched'][1][n]) for n, g in runs['off'][1].items())
        # on: the same loss and gradients up to the order of the sums; repeatable to the bit
        gap = _rel(runs['on'][0], runs['off'][0])
        grad_gaps = {n: H.rel_err(g, runs['off'][2][n]) for n, g in runs['on'][2].items()}
        print(f'loss_kernel [{kind}, {what}]: loss rel gap on / off {gap:.2e}; two parameter gradients '
              + ', '.join(f'{n} {v:.2e}' for n, v in grad_gaps.items()))
        assert gap <= TOL_PARITY and all(float(runs['off'][2][n].abs().max()) > 0 and v <= TOL_PARITY for n, v in grad_gaps.items())
        assert torch.equal(runs['on'][0], runs['on again'][0])
        assert all(torch.equal(g, runs['on again'][1][n]) for n, g in runs['on'][1].items())


def test_unrolled_step_through_the_state_with_the_kernel_reaches_the_state_leaves(monkeypatch):
    """The later steps' targets depend on the state (get_target), so this drives d_target."""
    from hgn_amd import _lib, features
    kind = 'flag'
    win = UT._windows(kind, 2, 3)
    grads, forward, backward = {}, [], []
    real, real_bwd = features.frame_losses, _lib.lib().hgn_frame_losses_bwd
    monkeypatch.setattr(features, 'frame_losses', lambda *a, **kw: forward.append(1) or real(*a, **kw))
    monkeypatch.setattr(_lib.lib(), 'hgn_frame_losses_bwd', lambda *a: backward.append(a[14] is not None) or real_bwd(*a))
    for setting in (False, True):
        model = UT._model(kind)
        model.loss_kernel = setting
        wa, leaves = UT._with_leaves(win, kind)
        model.unrolled_training_step(wa, 3, through_state=True, is_training=False)[0].backward()
        grads[setting] = {n: leaf.grad.clone() for n, leaf in leaves.items()}
        # off: no call; on: one per step, and one backward launch per step -- all three with d_target: the targets depend on the leaves
        assert (len(forward), backward) == ((3, [True, True, True]) if setting else (0, []))
    for n in grads[True]:
        gap = H.rel_err(grads[True][n], grads[False][n])
        print(f'loss_kernel [flag, unrolled through the state] d loss / d {n}: rel gap on / off {gap:.2e}')
        assert float(grads[True][n].abs().max()) > 0 and float(grads[False][n].abs().max()) > 0 and gap <= TOL_PARITY, n
