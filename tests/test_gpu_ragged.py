"""Ragged batches on the GPU -- frames of different meshes in one batch (not in the reference, which builds, expands and evaluates
every frame on its own, MeshSimulator.py:159-234,292-297): the kernels hgn_frame_losses_ragged / _bwd, hgn_training_noise_ragged and
hgn_radius_edges_ragged_count/_fill, and on top of them build_graph_frames, the batched steps with per-frame row counts and
rollout_frames of the three system models.

Yardsticks.  The kernels: the uniform or single-graph entries on every frame alone (torch.equal: the header promises those bits), with
equal frames the uniform batch entries (torch.equal), and the fp64 statement of tests/loss_statement.py, cut into frames by slicing,
at the bounds of tests/test_gpu_frame_losses.py (forward 2^-23, backward 4 * 2^-24 relative).  The models: the per-frame route
(build_graph / validation_step / rollout per frame or trajectory) on a deep copy taken before any call, so both routes start from the
same statistics and weights; ids and features torch.equal, running normaliser sums at rtol 1e-5 / atol 1e-4 (the bound of
tests/test_gpu_batch_build.py), losses and gradients at 1e-5 relative (TOL_PARITY), rollouts at the bounds of
tests/test_gpu_rollout_lockstep.py (errors rtol 1e-5, predictions step-relative 2e-5 doubling per step)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import loss_statement as LS
from tests import synth
from tests import test_gpu_unrolled_training as UT
from tests.test_gpu_batch_build import lifted

pytestmark = pytest.mark.gpu
TOL_FWD = 2.0 ** -23
TOL_BWD = 4 * 2.0 ** -24
TOL_PARITY = 1e-5
RADIUS = 0.03
OBSTACLE, NORMAL = 1, 0


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def cuda(frame):
    return {k: v.cuda() for k, v in frame.items()}


def starts(frame_rows):
    return [sum(frame_rows[:b]) for b in range(len(frame_rows) + 1)]


def slices(frame_rows):
    p = starts(frame_rows)
    return [slice(p[b], p[b + 1]) for b in range(len(frame_rows))]


def _same(a, b):
    """Equal bits (NaN entries compare by their place)."""
    a, b = a.reshape(-1), b.reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a.float()), torch.isnan(b.float())) \
        and torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))


def _within(got, want, rel, what):
    """|got - want| <= rel * |want| element-wise; NaN exactly where the statement has NaN.  -> the worst error / bound."""
    got = got.detach().double().cpu().numpy().reshape(np.shape(want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    err, bound = np.abs(got - want)[~nan], rel * np.abs(want)[~nan]
    assert bool((err <= bound).all()), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# the kernels: losses
# ---------------------------------------------------------------------------------------------------------------
LOSS_ROWS = (257, 1, 256, 255, 70)      # a frame of one row, frames either side of a chunk boundary, starts off every multiple of 64
NO_FREE = 4                             # the frame without a free row
LOSS_CONFIGS = {'flag-state': dict(F=3, d=3, ca=2.0, cp=-1.0, free=(0,), state=True), 'no-state': dict(F=2, free=(0, 5), state=False)}
KINDS = torch.tensor([0, 0, 0, 1, 3, 5, 40, -1], dtype=torch.int64)               # 40, -1: outside the bit mask, never free


@functools.lru_cache(maxsize=None)
def _loss_inputs(name, frame_rows=LOSS_ROWS, no_free=NO_FREE):
    """The inputs of one case on the device (shared by the tests, never written): the network output is a column slice of a wider slab,
    the node types are column 0 of a two-column matrix."""
    from hgn_amd.normalizer import Normalizer
    c = LOSS_CONFIGS[name]
    F, rows = c['F'], sum(frame_rows)
    gen = torch.Generator().manual_seed(1000 * F + rows)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()
    types = torch.full((rows, 2), 7, dtype=torch.int64)
    types[:, 0] = KINDS[torch.randint(0, len(KINDS), (rows,), generator=gen)]
    for b, own in enumerate(slices(frame_rows)):
        types[own.start, 0] = 0                                          # every frame has a free row (the frame of one row too) ...
        if b == no_free:
            types[own, 0] = 1                                            # ... but one
    x = dict(c, frame_rows=frame_rows, wide=rnd(rows, F + 4), target=rnd(rows, F), types=types.cuda())
    if c['state']:
        nz = Normalizer(F, 'output_normalizer')
        nz((torch.randn(257, F, generator=gen) * (0.3 + 0.37 * torch.arange(F)) + torch.linspace(-2.0, 4.0, F)).cuda())
        x.update(nz=nz, cur=rnd(rows, c['d']), prev=rnd(rows, c['d']), state_target=rnd(rows, c['d']))
    return x


def _net(x, wide=None):
    return (x['wide'] if wide is None else wide)[:, 2:2 + x['F']]


def _state(x, rows=slice(None)):
    return (x['nz'], x['cur'][rows], x['d'], x['ca'], x['prev'][rows], x['cp'], x['state_target'][rows]) if x['state'] else None


def _losses(x, rows=slice(None), wide=None, target=None, **split):
    from hgn_amd import features
    return features.frame_losses(_net(x, wide)[rows], (x['target'] if target is None else target)[rows], x['types'][rows, :1], x['free'],
                                 state=_state(x, rows), **split)


@pytest.mark.parametrize('name', list(LOSS_CONFIGS))
def test_ragged_losses_per_frame_bits_and_the_statement(name):
    from hgn_amd import features
    x = _loss_inputs(name)
    frame_rows, B = x['frame_rows'], len(x['frame_rows'])
    assert not _net(x).is_contiguous() and x['types'][:, :1].stride(0) == 2 and any(p % 64 for p in starts(frame_rows)[1:-1])
    res = _losses(x, frame_rows=frame_rows)
    assert res.loss.shape == () and res.per_frame.shape == (B,) and res.count.shape == (B + 1,) and res.count.dtype == torch.int64
    assert res.loss.grad_fn is None and (res.state_error is None) == (not x['state'])
    # every frame: the bits of the uniform entry on that frame alone; the frame without a free row is NaN and leaves the others alone
    for b, own in enumerate(slices(frame_rows)):
        alone = _losses(x, rows=own)
        assert _same(res.per_frame[b], alone.per_frame[0]) and _same(res.per_frame[b], alone.loss), b
        assert int(res.count[b]) == int(alone.count[0]) == int(alone.count[1]), b
        if x['state']:
            assert _same(res.state_per_frame[b], alone.state_per_frame[0]), b
        assert bool(torch.isnan(res.per_frame[b])) == (b == NO_FREE) and (int(res.count[b]) == 0) == (b == NO_FREE)
    assert int(res.count[1]) == 1 and frame_rows[1] == 1
    # all rows: the statement with every row in one frame
    v = None
    if x['state']:
        v, _ = features.advance_state(_net(x), x['nz'], x['cur'], x['d'], x['ca'], x['prev'], x['cp'], x['types'][:, :1], x['free'])
    loss, state_err, count = LS.losses(_net(x), x['target'], x['types'][:, 0], x['free'], None, v, x.get('state_target'))
    assert int(res.count[B]) == int(count[1]) == int(res.count[:B].sum()) and 0 < int(count[1]) < sum(frame_rows)
    worst = _within(res.loss, loss[1], TOL_FWD, 'loss')
    if x['state']:
        worst = max(worst, _within(res.state_error, state_err[1], TOL_FWD, 'state_error'))
    # ... and per frame, the statement on the frame's slice
    for b, own in enumerate(slices(frame_rows)):
        want, want_err, _ = LS.losses(_net(x)[own], x['target'][own], x['types'][own, 0], x['free'], None, v[own] if x['state'] else None,
                                      x['state_target'][own] if x['state'] else None)
        worst = max(worst, _within(res.per_frame[b], want[0], TOL_FWD, f'per_frame[{b}]'))
        if x['state']:
            worst = max(worst, _within(res.state_per_frame[b], want_err[0], TOL_FWD, f'state_per_frame[{b}]'))
    print(f'ragged frame_losses forward [{name}]: worst error / bound = {worst:.3f}')
    again = _losses(x, frame_rows=frame_rows)
    assert _same(again.loss, res.loss) and _same(again.per_frame, res.per_frame) and torch.equal(again.count, res.count)


def _backward(x, g_loss, frame, g_frame, **split):
    wide, target = x['wide'].detach().clone().requires_grad_(True), x['target'].detach().clone().requires_grad_(True)
    res = _losses(x, wide=wide, target=target, **split)
    assert res.loss.requires_grad and res.per_frame.requires_grad and not res.count.requires_grad
    assert res.state_error is None or not (res.state_error.requires_grad or res.state_per_frame.requires_grad)
    (g_loss * res.loss + g_frame * res.per_frame[frame]).backward()
    F = x['F']
    outside = torch.cat([wide.grad[:, :2], wide.grad[:, 2 + F:]], dim=1)
    return res, wide.grad[:, 2:2 + F], target.grad, outside


@pytest.mark.parametrize('name', list(LOSS_CONFIGS))
def test_ragged_losses_backward_vs_the_statement(name, monkeypatch):
    """Upstream gradients on `loss` and on one `per_frame` entry: the statement's d_net over all rows plus, on the frame's rows, the
    statement's d_net of the frame's slice.  One backward launch."""
    from hgn_amd import _lib
    x = _loss_inputs(name)
    frame_rows = x['frame_rows']
    real, calls = _lib.lib(), []

    class Spy:
        def __getattr__(self, entry):
            if entry.startswith('hgn_frame_losses'):
                calls.append(entry)
            return getattr(real, entry)
    monkeypatch.setattr(_lib, 'lib', lambda: Spy())
    for frame in (0, 1, 3):
        own = slices(frame_rows)[frame]
        del calls[:]
        _, d_net, d_target, outside = _backward(x, 0.7, frame, 1.3, frame_rows=frame_rows)
        assert calls == ['hgn_frame_losses_ragged_workspace_bytes', 'hgn_frame_losses_ragged', 'hgn_frame_losses_ragged_bwd']
        want = LS.d_net(_net(x), x['target'], x['types'][:, 0], x['free'], None, [0.0, 0.7])
        want[own] += LS.d_net(_net(x)[own], x['target'][own], x['types'][own, 0], x['free'], None, [1.3, 0.0])
        worst = _within(d_net, want, TOL_BWD, f'frame {frame}')
        print(f'ragged frame_losses backward [{name}, upstream on loss and per_frame[{frame}]]: worst error / bound = {worst:.3f}')
        assert float(outside.abs().max()) == 0 and float(d_net[own].abs().max()) > 0
        assert torch.equal(d_target.view(torch.int32), d_net.view(torch.int32) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device='cuda'))
        rest = torch.from_numpy(~LS.free_rows(x['types'][:, 0], x['free'])).cuda()
        assert bool((d_net[rest] == 0).all()) and bool(rest[slices(frame_rows)[NO_FREE]].all())


@pytest.mark.parametrize('name', list(LOSS_CONFIGS))
def test_ragged_losses_with_equal_frames_have_the_bits_of_the_uniform_entries(name):
    x = _loss_inputs(name, (96, 96, 96), -1)
    a, da, ta, _ = _backward(x, 0.7, 1, 1.3, frame_rows=(96, 96, 96))
    b, db, tb, _ = _backward(x, 0.7, 1, 1.3, rows_per_frame=96)
    for got, want in zip(a, b):
        assert (got is None and want is None) or (_same(got, want) and got.dtype == want.dtype)
    assert torch.equal(da, db) and torch.equal(ta, tb) and float(da.abs().max()) > 0
    with pytest.raises(ValueError, match='frame_rows'):
        _losses(x, frame_rows=(96, 96, 95))


# ---------------------------------------------------------------------------------------------------------------
# the kernels: noise
# ---------------------------------------------------------------------------------------------------------------
NOISE_ROWS = (5, 300, 1)
NOISE_IDS = (7, 2 ** 32 + 3, 0)


@pytest.mark.parametrize('d', [3, 2])
def test_ragged_noise_gives_every_frame_the_samples_it_gets_alone(d, monkeypatch):
    from hgn_amd import _lib, features
    rows = sum(NOISE_ROWS)
    gen = torch.Generator().manual_seed(50 + d)
    slab, target = torch.randn(rows, d + 2, generator=gen).cuda(), torch.randn(rows, d, generator=gen).cuda()
    x = slab[:, 1:1 + d]                                                 # a column slice of a wider slab
    types = KINDS[torch.randint(0, len(KINDS), (rows, 1), generator=gen)]
    types[0], types[5], types[304], types[305] = 1, 0, 0, 0             # a copied row; free rows at a frame start, a frame end and alone
    types = types.cuda()
    free = types[:, 0] == 0
    std, seed, draw, scale = 0.02, 0x1234567890ab, 3, 0.1
    for ids in (NOISE_IDS, None):
        out_x, out_t = features.add_noise(x, types, (0,), std, seed, draw, target, scale, frame_ids=ids, frame_rows=NOISE_ROWS)
        assert out_x.shape == x.shape and out_t.shape == target.shape and out_x.dtype == torch.float32
        for b, own in enumerate(slices(NOISE_ROWS)):
            alone_x, alone_t = features.add_noise(x[own], types[own], (0,), std, seed, draw, target[own], scale,
                                                  frame_ids=[ids[b] if ids else b])
            assert torch.equal(out_x[own], alone_x) and torch.equal(out_t[own], alone_t), (ids, b)
        bits = lambda t: t.contiguous().view(torch.int32)
        assert torch.equal(bits(out_x)[~free], bits(x)[~free]) and torch.equal(bits(out_t)[~free], bits(target)[~free])
        assert bool((out_x[free] != x[free]).any(dim=1).all()) and int(free.sum()) > 50
    only_x, none = features.add_noise(x, types, (0,), std, seed, draw, frame_ids=NOISE_IDS, frame_rows=NOISE_ROWS)
    assert none is None and torch.equal(only_x, features.add_noise(x, types, (0,), std, seed, draw, target, scale, frame_ids=NOISE_IDS,
                                                                   frame_rows=NOISE_ROWS)[0])
    # an autograd node whose backward launches nothing
    leaf = x.detach().clone().requires_grad_(True)
    noisy, _ = features.add_noise(leaf, types, (0,), std, seed, draw, frame_ids=NOISE_IDS, frame_rows=NOISE_ROWS)
    real, calls = _lib.lib(), []

    class Spy:
        def __getattr__(self, entry):
            calls.append(entry)
            return getattr(real, entry)
    monkeypatch.setattr(_lib, 'lib', lambda: Spy())
    (noisy * 2.0).sum().backward()
    assert calls == [] and torch.equal(leaf.grad, torch.full_like(leaf, 2.0)) and torch.equal(noisy.detach(), only_x)
    with pytest.raises(ValueError, match='frame ids'):
        features.add_noise(x, types, (0,), std, seed, draw, frame_ids=[1, 2], frame_rows=NOISE_ROWS)


# ---------------------------------------------------------------------------------------------------------------
# the kernels: radius
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plate_frames():
    """Four plate frames of three meshes, N = 58, 158, 32, 58; the last is the first with its obstacle lifted out of reach: it has no
    pair of its own, and its plate lies under the obstacle of the frame before it."""
    first = synth.plate_frame(seed=21, nx=5, ny=4, nz=2, obstacle=(3, 3, 2))
    return [first, synth.plate_frame(seed=20), synth.plate_frame(seed=23, nx=4, ny=3, nz=2, obstacle=(2, 2, 2)), lifted(first)]


PLATE_ROWS, PLATE_PAIRS = (58, 158, 32, 58), (33, 62, 12, 0)


def mesh_csr(senders, receivers, rows):
    """Neighbour CSR as PlateModel builds it."""
    from hgn_amd import topology
    csr = topology.segment_csr(receivers, rows, senders.device)
    return csr.rowptr, senders[csr.perm.long()].to(torch.int32).contiguous()


@pytest.mark.parametrize('with_csr', [True, False], ids=['union_nbr_csr', 'no_csr'])
def test_radius_edges_ragged_equals_shifted_per_graph_results(with_csr):
    from hgn_amd import features
    frames = plate_frames()
    B = len(frames)
    assert tuple(f['node_type'].shape[0] for f in frames) == PLATE_ROWS
    for f in frames:                    # no pair within 1e-6 of the radius (fp64): the result does not hang on fp32 rounding
        raw, w = f['node_type'][:, 0].long(), f['world_pos'].double()
        dist = torch.sqrt((w[:, None, :] - w[None, :, :]).pow(2).sum(-1))[raw == OBSTACLE][:, raw == NORMAL]
        assert float((dist - RADIUS).abs().min()) > 1e-6
    # a pair across the last two frames lies inside the radius: only the graph boundary keeps it out
    obstacle = frames[2]['world_pos'][frames[2]['node_type'][:, 0] == OBSTACLE].double()
    plate = frames[3]['world_pos'][frames[3]['node_type'][:, 0] == NORMAL].double()
    assert float(torch.cdist(obstacle, plate).min()) < RADIUS - 1e-3
    pos = torch.cat([f['world_pos'] for f in frames]).cuda()
    types = torch.cat([f['node_type'] for f in frames]).cuda()
    first = starts(PLATE_ROWS)
    meshes = [features.cells_to_edges(f['cells'].cuda(), True)[:2] for f in frames]
    per_frame_csr = [mesh_csr(s.contiguous(), r.contiguous(), n) if with_csr else (None, None) for (s, r), n in zip(meshes, PLATE_ROWS)]
    union_csr = (None, None)
    if with_csr:
        union_csr = mesh_csr(torch.cat([s + p for (s, _), p in zip(meshes, first)]).contiguous(),
                             torch.cat([r + p for (_, r), p in zip(meshes, first)]).contiguous(), sum(PLATE_ROWS))
    S, R, counts = [], [], [0]
    for b, own in enumerate(slices(PLATE_ROWS)):
        s, r = features.radius_edges(pos[own], types[own], RADIUS, OBSTACLE, NORMAL, *per_frame_csr[b])
        assert s.shape[0] == PLATE_PAIRS[b], b
        S.append(s + first[b])
        R.append(r + first[b])
        counts.append(counts[-1] + s.shape[0])
    s, r, off = features.radius_edges_ragged(pos, types, PLATE_ROWS, RADIUS, OBSTACLE, NORMAL, *union_csr)
    assert s.dtype == torch.int64 and r.dtype == torch.int64 and off.dtype == torch.int32 and off.shape == (B + 1,)
    assert torch.equal(s, torch.cat(S)) and torch.equal(r, torch.cat(R)) and off.tolist() == counts
    graph_of = lambda ids: torch.bucketize(ids, torch.tensor(first[1:], device='cuda'), right=True)
    assert bool((graph_of(s) == graph_of(r)).all())
    # any type on either end, the mesh edges excluded or not: many more pairs, the same statement
    S, R = [], []
    for b, own in enumerate(slices(PLATE_ROWS)):
        sb, rb = features.radius_edges(pos[own], types[own], RADIUS, -1, -1, *per_frame_csr[b])
        S.append(sb + first[b])
        R.append(rb + first[b])
    s, r, off = features.radius_edges_ragged(pos, types, PLATE_ROWS, RADIUS, -1, -1, *union_csr)
    assert s.shape[0] > sum(PLATE_PAIRS) and torch.equal(s, torch.cat(S)) and torch.equal(r, torch.cat(R)) and int(off[-1]) == s.shape[0]
    with pytest.raises(ValueError, match='frame_rows'):
        features.radius_edges_ragged(pos, types, PLATE_ROWS[:-1], RADIUS, OBSTACLE, NORMAL)


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_frames(kind):
    """Three frames of different meshes per model, on the device (shared, never written)."""
    if kind == 'flag':
        frames = [synth.flag_frame(seed=300 + i, nx=nx, ny=ny) for i, (nx, ny) in enumerate(((3, 3), (17, 17), (5, 4)))]
        assert [f['node_type'].shape[0] for f in frames] == [9, 289, 20]
    elif kind == 'cylinder':
        frames = [synth.cylinder_frame(seed=300 + i, nx=nx, ny=ny) for i, (nx, ny) in enumerate(((4, 3), (18, 15), (6, 5)))]
        assert [f['node_type'].shape[0] for f in frames] == [12, 270, 30]
    else:
        frames = plate_frames()[:3]
    return [cuda(f) for f in frames]


def twins(kind):
    """A warm model and its deep copy, taken before either is called."""
    model = UT._model(kind)
    return model, copy.deepcopy(model)


def union_of(graphs):
    """The test's own disjoint union of per-frame build_graph results: ids of frame b shifted by the rows before it, every set and
    every per-node field concatenated frame by frame."""
    rows = [g.node_features[0].shape[0] for g in graphs]
    first = starts(rows)
    sets = []
    for k, e in enumerate(graphs[0].edge_sets):
        sets.append((e.name, torch.cat([g.edge_sets[k].features for g in graphs]),
                     torch.cat([g.edge_sets[k].senders + p for g, p in zip(graphs, first)]),
                     torch.cat([g.edge_sets[k].receivers + p for g, p in zip(graphs, first)])))
    return dict(nodes=torch.cat([g.node_features[0] for g in graphs]), sets=sets,
                target=torch.cat([g.target_feature for g in graphs]), mesh=torch.cat([g.mesh_features for g in graphs]),
                raw=torch.cat([g.unnormalized_edges.features for g in graphs]),
                obstacle=None if graphs[0].obstacle_nodes is None else torch.cat([g.obstacle_nodes for g in graphs]))


def assert_is_union(got, want, node_dynamic=None):
    assert len(got.node_features) == 1 and torch.equal(got.node_features[0], want['nodes'])
    assert [e.name for e in got.edge_sets] == [s[0] for s in want['sets']]
    for e, (name, feat, s, r) in zip(got.edge_sets, want['sets']):
        assert e.senders.dtype == torch.int64 and torch.equal(e.senders, s) and torch.equal(e.receivers, r), name
        assert e.features.shape == feat.shape and torch.equal(e.features, feat), name
    assert torch.equal(got.target_feature, want['target']) and torch.equal(got.mesh_features, want['mesh'])
    un = got.unnormalized_edges
    assert un.name == 'mesh_edges' and torch.equal(un.features, want['raw'])
    assert torch.equal(un.senders, want['sets'][0][2]) and torch.equal(un.receivers, want['sets'][0][3])
    assert (got.obstacle_nodes is None) == (want['obstacle'] is None)
    if want['obstacle'] is not None:
        assert torch.equal(got.obstacle_nodes, want['obstacle'])


KINDS3 = ['flag', 'cylinder', 'plate']


@pytest.mark.parametrize('kind', KINDS3)
def test_build_graph_frames_is_the_union_of_the_per_frame_graphs(kind):
    frames = model_frames(kind)
    a, b = twins(kind)
    with torch.no_grad():
        per = [b.build_graph(f, False) for f in frames]
        got = a.build_graph_frames(frames, False)
    assert_is_union(got, union_of(per))
    assert got.model_type == per[0].model_type and got.node_features[0].shape[0] == sum(f['node_type'].shape[0] for f in frames)
    if kind == 'plate':
        assert [e.senders.shape[0] for e in (g.edge_sets[1] for g in per)] == list(PLATE_PAIRS[:3]) and got.node_dynamic is None
    elif kind == 'cylinder':
        assert got.node_dynamic == []
    else:
        assert got.node_dynamic.shape[0] == sum(f['node_type'].shape[0] for f in frames)
    # the same composition again: the same index tensors (one topology for the caches behind the network), also from the pair form
    flat, frame_rows = a.concat_frames(frames)
    with torch.no_grad():
        again, pair = a.build_graph_frames(frames, False), a.build_graph_frames((flat, frame_rows), False)
    for other in (again, pair):
        assert all(x.senders is y.senders and x.receivers is y.receivers for x, y in zip(other.edge_sets[:1], got.edge_sets[:1]))
        assert all(torch.equal(x.features, y.features) and torch.equal(x.senders, y.senders) for x, y in zip(other.edge_sets, got.edge_sets))
    # another order of the frames is another composition
    with torch.no_grad():
        swapped = a.build_graph_frames(frames[::-1], False)
    assert_is_union(swapped, union_of(per[::-1]))


@pytest.mark.parametrize('kind', KINDS3)
def test_build_graph_frames_accumulates_the_statistics_of_the_whole_batch(kind):
    frames = model_frames(kind)
    a, b = twins(kind)
    with torch.no_grad():
        for f in frames:
            b.build_graph(f, True)
        a.build_graph_frames(frames, True)
    names = ['_node_normalizer', '_mesh_edge_normalizer'] + (['_world_edge_normalizer'] if kind == 'plate' else [])
    for name in names:
        na, nb = getattr(a, name), getattr(b, name)
        assert float(na._acc_count) > 0 and torch.equal(na._acc_count, nb._acc_count), name
        torch.testing.assert_close(na._acc_sum, nb._acc_sum, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(na._acc_sum_squared, nb._acc_sum_squared, rtol=1e-5, atol=1e-4)
        assert float(na._num_accumulations) == float(nb._num_accumulations) - (len(frames) - 1), name


def assert_same_graph(got, want):
    assert_is_union(got, union_of([want]))
    if torch.is_tensor(want.node_dynamic):
        assert torch.equal(got.node_dynamic, want.node_dynamic)
    else:
        assert got.node_dynamic == want.node_dynamic


@pytest.mark.parametrize('kind', KINDS3)
def test_build_graph_frames_of_one_frame_and_of_equal_meshes(kind):
    """A batch of one frame is build_graph, bit for bit; frames of one mesh (equal `cells` in tensors of their own) are
    build_graph_batch, bit for bit."""
    frames = model_frames(kind)
    for f in (frames[0], frames[1]):
        a, b = twins(kind)
        with torch.no_grad():
            assert_same_graph(a.build_graph_frames([f], False), b.build_graph(f, False))
    make = {'flag': lambda i: synth.flag_frame(seed=i, nx=5, ny=4), 'cylinder': lambda i: synth.cylinder_frame(seed=i, nx=5, ny=4),
            'plate': lambda i: synth.plate_frame(seed=i)}[kind]
    same_mesh = [cuda(make(310 + i)) for i in range(3)]
    assert same_mesh[0]['cells'] is not same_mesh[1]['cells'] and torch.equal(same_mesh[0]['cells'], same_mesh[1]['cells'])
    stacked = {k: (same_mesh[0][k] if k in ('cells', 'mesh_pos') else torch.stack([f[k] for f in same_mesh])) for k in same_mesh[0]}
    a, b = twins(kind)
    with torch.no_grad():
        assert_same_graph(a.build_graph_frames(same_mesh, False), b.build_graph_batch(stacked, False))
    assert len(a._meshes) == 1                                          # one distinct mesh: one cells_to_edges


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize('kind', KINDS3)
def test_validation_step_batch_with_frame_rows_vs_validation_step(kind):
    frames = model_frames(kind)
    a, b = twins(kind)
    flat, frame_rows = a.concat_frames(frames)
    B = len(frames)
    graph = a.expand_graph_frames(a.build_graph_frames(frames, False), frame_rows, 0, B, False)
    loss, state_error = a.validation_step_batch(graph, flat, frame_rows)
    assert loss.shape == (B,) and state_error.shape == (B,) and loss.dtype == state_error.dtype == torch.float32 and loss.is_cuda
    for i, frame in enumerate(frames):
        want = b.validation_step(b.expand_graph(b.build_graph(frame, False), 0, B, False), frame)
        gaps = (_rel(loss[i], want[0]), _rel(state_error[i], want[1]))
        print(f'validation_step_batch [{kind}, ragged, frame {i}] vs validation_step: loss rel {gaps[0]:.2e}, state error rel {gaps[1]:.2e}')
        assert want[0] > 0 and want[1] > 0 and max(gaps) <= TOL_PARITY, (i, gaps)
    with pytest.raises(ValueError, match='frame_rows'):
        a.validation_step_batch(graph, flat, frame_rows[:-1])


@pytest.mark.parametrize('kind', KINDS3)
def test_training_step_batch_with_frame_rows_vs_the_per_frame_route(kind):
    """`per_frame` against the masked MSE of every frame, and the parameter gradients of `loss` against those of the all-rows masked
    MSE, both over the union the test forms from the per-frame build_graph results on the copy."""
    from hgn_amd import system_model, util
    frames = model_frames(kind)
    a, b = twins(kind)
    flat, frame_rows = a.concat_frames(frames)
    B = len(frames)
    with torch.no_grad():
        graph = a.expand_graph_frames(a.build_graph_frames(frames, False), frame_rows, 0, 1, True)
        u = union_of([b.build_graph(f, False) for f in frames])
    loss, per_frame = a.training_step_batch(graph, flat, frame_rows)
    assert loss.requires_grad and per_frame.shape == (B,) and not per_frame.requires_grad and float(loss.detach()) > 0
    loss.backward()
    union = util.MultiGraph(node_features=[u['nodes']], edge_sets=[util.EdgeSet(name=n, features=f, senders=s, receivers=r)
                                                                   for n, f, s, r in u['sets']])
    out = b(union)
    target = b.get_target(flat)                                          # accumulates once, as training_step_batch does
    mask = b._loss_mask(flat)
    want = system_model._masked_mse(target, out, mask)
    want.backward()
    gap = _rel(loss.detach(), want.detach())
    frame_gaps = [_rel(per_frame[i], system_model._masked_mse(target[own], out[own], mask[own]).detach())
                  for i, own in enumerate(slices(frame_rows))]
    ga = {n: p.grad for n, p in a.learned_model.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in b.learned_model.named_parameters() if p.grad is not None}
    assert ga.keys() == gb.keys() and len(ga) >= 2
    grad_gaps = {n: H.rel_err(ga[n], gb[n]) for n in ga}
    print(f'training_step_batch [{kind}, ragged]: loss rel gap {gap:.2e}, per frame {[f"{g:.2e}" for g in frame_gaps]}, worst parameter '
          f'gradient gap {max(grad_gaps.values()):.2e}')
    assert gap <= TOL_PARITY and max(frame_gaps) <= TOL_PARITY
    assert all(float(gb[n].abs().max()) > 0 and v <= TOL_PARITY for n, v in grad_gaps.items()), grad_gaps


def test_model_add_noise_with_frame_rows_is_the_per_frame_noise():
    frames = model_frames('cylinder')
    model = UT._model('cylinder')
    model._params = dict(model._params, noise=0.02, gamma=0.1, field='velocity')
    flat, frame_rows = model.concat_frames(frames)
    ids = (11, 5, 2 ** 32 + 1)
    noisy = model.add_noise(flat, 9, ids, seed=77, frame_rows=frame_rows)
    assert noisy['cells'] is flat['cells'] and noisy['mesh_pos'] is flat['mesh_pos'] and noisy['velocity'] is not flat['velocity']
    for i, (frame, own) in enumerate(zip(frames, slices(frame_rows))):
        alone = model.add_noise(frame, 9, [ids[i]], seed=77)
        for name in ('velocity', 'target|velocity'):
            assert torch.equal(noisy[name][own], alone[name]) and not torch.equal(alone[name], frame[name]), (i, name)


# ---------------------------------------------------------------------------------------------------------------
# rollout of several trajectories in lock step
# ---------------------------------------------------------------------------------------------------------------
def trajectory_of(make, seeds):
    """T frames of one mesh stacked into the [T, ...] series `rollout` takes (`cells` and `mesh_pos` per frame)."""
    frames = [make(seed) for seed in seeds]
    shared = {'cells': frames[0]['cells'], 'mesh_pos': frames[0]['mesh_pos']}
    return {name: torch.stack([dict(f, **shared)[name] for f in frames]).cuda() for name in frames[0]}


ROLLOUTS = {'flag': [lambda s: synth.flag_frame(seed=s, nx=3, ny=3), lambda s: synth.flag_frame(seed=s, nx=17, ny=17)],
            'plate': [lambda s: synth.plate_frame(seed=s, nx=5, ny=4, nz=2, obstacle=(3, 3, 2)),
                      lambda s: synth.plate_frame(seed=s, nx=4, ny=3, nz=2, obstacle=(2, 2, 2))]}


def step_bound(kind, steps):
    first = 1 if kind == 'flag' else 0                         # flag records the input state first (exact)
    return torch.tensor([2e-5 * 2.0 ** max(t - first, 0) for t in range(steps)], dtype=torch.float64)


def per_step_err(got, want, scale):
    return (got.double() - want.double()).abs().flatten(1).max(1).values.cpu() / scale


@pytest.mark.parametrize('kind', list(ROLLOUTS))
def test_rollout_frames_vs_rollout_per_trajectory(kind):
    T = 4
    trajectories = [trajectory_of(make, range(400 + 10 * i, 400 + 10 * i + T)) for i, make in enumerate(ROLLOUTS[kind])]
    before = [{name: t.clone() for name, t in trajectory.items()} for trajectory in trajectories]
    a, b = twins(kind)
    results = a.rollout_frames(trajectories, T)
    assert len(results) == 2
    for i, (trajectory, (got, errors)) in enumerate(zip(trajectories, results)):
        want, want_errors = b.rollout(trajectory, T)
        assert errors.shape == (T,) and set(got) == set(want)
        torch.testing.assert_close(errors, want_errors, rtol=1e-5, atol=0)
        for key in want:
            assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (i, key)
            if key in ('pred_pos', 'cur_positions', 'cur_velocities'):
                p = want['pred_pos'].double()
                scale = float((p[1:] - p[:-1]).abs().max()) if key != 'cur_velocities' else float(want[key].abs().max())
                err = per_step_err(got[key], want[key], scale)
                print(f'rollout_frames [{kind}, trajectory {i}] {key}: step-relative difference to rollout', err.tolist())
                assert bool((err <= step_bound(kind, T)).all()), (i, key, err.tolist())
                assert float((want[key][-1] - want[key][0]).abs().max()) > 0
            else:
                assert torch.equal(got[key], want[key]), (i, key)
    for trajectory, kept in zip(trajectories, before):                  # inputs are not written
        assert all(torch.equal(trajectory[name], kept[name]) for name in kept)
    with pytest.raises(ValueError, match='rollout_frames'):
        a.rollout_frames(trajectories, T + 1)


@pytest.mark.parametrize('stage', ['connector', 'balancer'])
def test_expand_graph_frames_refuses_a_connector_and_a_balancer(stage):
    from hgn_amd import _lib, system_model
    from tests.test_gpu_batch_build import params
    balancer = {'algorithm': 'random', 'frequency': 1, 'remove_edges': False, 'random': {'edge_amount': 4}}
    model = system_model.FlagModel(params('hyper') if stage == 'connector' else params(balancer=balancer))
    frames = model_frames('flag')
    with torch.no_grad():
        graph = model.build_graph_frames(frames, False)
        with pytest.raises(_lib.HgnError, match='expand_graph_frames.*per-frame route'):
            model.expand_graph_frames(graph, tuple(f['node_type'].shape[0] for f in frames), 0, 1, False)
