"""Whole batches of frames built into one graph (not in the reference, which builds and expands every frame on its own and
concatenates, MeshSimulator.py:159-234): the radius query over a batch of graphs (hgn_radius_edges_batch_count/_fill),
CylinderModel / PlateModel.build_graph_batch, expand_graph_batch and flatten_frames.

Yardsticks.  The kernel: the single-graph entry features.radius_edges (pinned by the reference's goldens), called per graph,
shifted and concatenated -- integer outputs, torch.equal.  The models: batching.batch_graphs over the per-frame build_graph /
expand_graph results on a second model that holds the same statistics, clusters and weights.  Both routes run the same kernels over
the same rows in the same order, so ids AND features are compared with torch.equal; running normaliser sums within
rtol 1e-5 / atol 1e-4 (one accumulate over the batch against B accumulates: fp32 summation order, the bound of
test_flag_build_graph_batch_equals_per_frame_graphs).  Cylinder input gradients: torch.equal (every term is formed row by row)."""
import copy

import pytest
import torch

from oracle import features_oracle as FO
from tests import synth
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
TOL_GRAD = 1e-5
RADIUS = 0.03
OBSTACLE, NORMAL = 1, 0
SHARED = ('cells', 'mesh_pos')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def cuda_frame(fr):
    return {k: v.cuda() for k, v in fr.items()}


def params(connector='none', K=4, balancer=None):
    return {'size': 3, 'aggregation': 'sum', 'message_passing_steps': 1,
            'rmp': {'clustering': 'kmeans' if connector != 'none' else 'none', 'connector': connector, 'num_clusters': K,
                    'hyper_noise': 'none', 'hyper_node_features': True, 'frequency': 1, 'fully_connect': False,
                    'intra_cluster_sampling': {'enabled': False, 'alpha': 0.1, 'spotter_threshold': 0}},
            'graph_balancer': balancer or {'algorithm': 'none', 'frequency': 1}}


def stack(frames):
    """B frames of one mesh as one stacked frame on the device: per-node series [B, N, .], `cells` / `mesh_pos` once."""
    return {k: (frames[0][k] if k in SHARED else torch.stack([f[k] for f in frames])).cuda() for k in frames[0]}


def lifted(frame, dz=1.0):
    """The frame with its obstacle block moved up by ``dz``: no obstacle -> plate pair is inside the radius any more."""
    out = dict(frame)
    obst = frame['node_type'][:, 0] == OBSTACLE
    for k in ('world_pos', 'target|world_pos'):
        out[k] = frame[k].clone()
        out[k][obst, 2] += dz
    return out


def plate_frames(n, seed0=20, empty=1):
    frames = [synth.plate_frame(seed=seed0 + i) for i in range(n)]
    frames[empty] = lifted(frames[empty])
    return frames


def mesh_csr(frame):
    """Neighbour CSR of one frame's mesh as PlateModel builds it."""
    from hgn_amd import features, topology
    s, r, _ = features.cells_to_edges(frame['cells'].cuda(), True)
    s, r = s.contiguous(), r.contiguous()
    csr = topology.segment_csr(r, frame['node_type'].shape[0], s.device)
    return csr.rowptr, s[csr.perm.long()].to(torch.int32).contiguous()


def per_graph(pos, types, B, radius, st, rt, rowptr=None, nbr=None):
    """The yardstick: features.radius_edges on every graph, shifted by b*N and concatenated; + the cumulative counts."""
    from hgn_amd import features
    N = pos.shape[0] // B
    S, R, counts = [], [], [0]
    for b in range(B):
        s, r = features.radius_edges(pos[b * N:(b + 1) * N], types[b * N:(b + 1) * N], radius, st, rt, rowptr, nbr)
        S.append(s + b * N)
        R.append(r + b * N)
        counts.append(counts[-1] + s.shape[0])
    return torch.cat(S), torch.cat(R), torch.tensor(counts, dtype=torch.int32), counts


# ----------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_csr', [True, False], ids=['nbr_csr', 'no_csr'])
def test_radius_edges_batch_equals_concatenated_per_graph_results(with_csr):
    """1. B = 3 plate frames (N = 158: no multiple of 64, B*N no multiple of the 4 waves of a workgroup), the middle one without
    world edges."""
    from hgn_amd import features
    B = 3
    frames = plate_frames(B, seed0=20, empty=1)
    N = frames[0]['node_type'].shape[0]
    assert N == 158 and (B * N) % 4 != 0
    # no pair within 1e-6 of the radius (fp64): the result does not hang on fp32 rounding of a distance
    raw = frames[0]['node_type'][:, 0].long()
    for f in frames:
        w = f['world_pos'].double()
        dist = torch.sqrt((w[:, None, :] - w[None, :, :]).pow(2).sum(-1))[raw == OBSTACLE][:, raw == NORMAL]
        assert float((dist - FO.PlateFeatures.RADIUS).abs().min()) > 1e-6
    o64 = [FO.PlateFeatures(dtype=torch.float64).build_graph(f, False)['edge_sets'][1] for f in frames]
    assert o64[0].senders.shape[0] >= 1 and o64[2].senders.shape[0] >= 1 and o64[1].senders.shape[0] == 0
    pos = torch.cat([f['world_pos'] for f in frames]).cuda()
    types = torch.cat([f['node_type'] for f in frames]).cuda()
    rowptr, nbr = mesh_csr(frames[0]) if with_csr else (None, None)
    want_s, want_r, want_off, counts = per_graph(pos, types, B, RADIUS, OBSTACLE, NORMAL, rowptr, nbr)
    assert counts[1] - counts[0] >= 1 and counts[2] == counts[1] and counts[3] - counts[2] >= 1
    s, r, off = features.radius_edges_batch(pos, types, B, RADIUS, OBSTACLE, NORMAL, rowptr, nbr)
    assert s.dtype == torch.int64 and r.dtype == torch.int64 and off.dtype == torch.int32 and off.shape == (B + 1,)
    assert torch.equal(s, want_s) and torch.equal(r, want_r)
    assert torch.equal(off.cpu(), want_off)
    if with_csr:                                            # and the fp64 oracle's pairs (mesh edges excluded there too)
        assert torch.equal(s.cpu(), torch.cat([e.senders + b * N for b, e in enumerate(o64)]))
        assert torch.equal(r.cpu(), torch.cat([e.receivers + b * N for b, e in enumerate(o64)]))


def test_radius_edges_batch_reports_no_pair_across_graphs():
    """2. Two graphs with IDENTICAL positions: every cross-graph twin pair is at distance 0 and must not appear."""
    from hgn_amd import features
    f = synth.plate_frame(seed=31)
    N = f['node_type'].shape[0]
    pos = torch.cat([f['world_pos'], f['world_pos']]).cuda()
    types = torch.cat([f['node_type'], f['node_type']]).cuda()
    rowptr, nbr = mesh_csr(f)
    for st, rt, csr in ((OBSTACLE, NORMAL, (rowptr, nbr)), (-1, -1, (None, None))):
        s1, r1 = features.radius_edges(pos[:N], types[:N], RADIUS, st, rt, *csr)
        assert s1.shape[0] >= 1
        s, r, off = features.radius_edges_batch(pos, types, 2, RADIUS, st, rt, *csr)
        assert torch.equal(s, torch.cat([s1, s1 + N])) and torch.equal(r, torch.cat([r1, r1 + N]))
        assert bool((torch.div(s, N, rounding_mode='floor') == torch.div(r, N, rounding_mode='floor')).all())
        assert off.tolist() == [0, s1.shape[0], 2 * s1.shape[0]]


@pytest.mark.parametrize('N', [5, 64, 65])
def test_radius_edges_batch_chunk_and_graph_boundaries(N):
    """3. One partial chunk, a graph boundary on a chunk boundary, one node more; any-type senders / receivers."""
    from hgn_amd import features, topology
    B = 2
    g = torch.Generator().manual_seed(100 + N)
    pos = torch.rand(B * N, 3, generator=g)                 # unit cube: radius 0.35 catches a good share of the pairs
    pos[N - 1] = pos[0] + 0.01                              # last row of graph 0 next to its first row ...
    pos[N] = pos[N - 1]                                     # ... and on top of the first row of graph 1
    types = torch.randint(0, 2, (B * N, 1), generator=g)
    types[0], types[N - 1], types[N], types[-1] = 1, 0, 0, 1
    # a ring as the shared mesh: i <-> i + 1 (local ids)
    a = torch.arange(N)
    ms, mr = torch.cat([a, (a + 1) % N]).cuda(), torch.cat([(a + 1) % N, a]).cuda()
    csr = topology.segment_csr(mr, N, ms.device)
    nbr = ms[csr.perm.long()].to(torch.int32).contiguous()
    pos, types = pos.cuda(), types.cuda()
    seen = 0
    for st, rt in ((1, 0), (-1, 0), (1, -1), (-1, -1)):
        for rowptr, nb in ((None, None), (csr.rowptr, nbr)):
            want_s, want_r, want_off, counts = per_graph(pos, types, B, 0.35, st, rt, rowptr, nb)
            s, r, off = features.radius_edges_batch(pos, types, B, 0.35, st, rt, rowptr, nb)
            assert torch.equal(s, want_s) and torch.equal(r, want_r), (st, rt, rowptr is None)
            assert torch.equal(off.cpu(), want_off)
            seen += counts[-1]
            if st < 0 and rt < 0 and rowptr is None:
                pairs = set(zip(s.tolist(), r.tolist()))
                assert (0, N - 1) in pairs and (N - 1, 0) in pairs            # inside graph 0, across the whole sweep
                assert (N - 1, N) not in pairs and (N, N - 1) not in pairs    # distance 0, but two graphs
    assert seen > 0


def test_radius_edges_batch_of_one_graph_equals_the_single_graph_entry():
    """4. B = 1."""
    from hgn_amd import features
    f = synth.plate_frame(seed=33)
    pos, types = f['world_pos'].cuda(), f['node_type'].cuda()
    rowptr, nbr = mesh_csr(f)
    s1, r1 = features.radius_edges(pos, types, RADIUS, OBSTACLE, NORMAL, rowptr, nbr)
    s, r, off = features.radius_edges_batch(pos, types, 1, RADIUS, OBSTACLE, NORMAL, rowptr, nbr)
    assert s1.shape[0] >= 1 and torch.equal(s, s1) and torch.equal(r, r1) and off.tolist() == [0, s1.shape[0]]


def test_radius_edges_batch_refuses_rows_that_do_not_split_into_equal_graphs():
    from hgn_amd import features
    pos = torch.rand(7, 3).cuda()
    types = torch.zeros(7, 1, dtype=torch.int64).cuda()
    for B in (2, 3, 0, -1):
        with pytest.raises(ValueError, match='radius_edges_batch'):
            features.radius_edges_batch(pos, types, B, RADIUS, -1, -1)
    with pytest.raises(ValueError, match='radius_edges_batch'):                  # node types of another length
        features.radius_edges_batch(pos[:6], types, 2, RADIUS, -1, -1)
    s, r, off = features.radius_edges_batch(pos, types, 7, 10.0, -1, -1)         # seven graphs of one node: nothing to pair
    assert s.shape == (0,) and off.tolist() == [0] * 8


def test_radius_edges_batch_without_any_pair_returns_empty_tensors(monkeypatch):
    """5. Total 0: empty tensors, the fill entry is not launched."""
    from hgn_amd import _lib, features
    frames = [lifted(synth.plate_frame(seed=34 + i)) for i in range(2)]
    pos = torch.cat([f['world_pos'] for f in frames]).cuda()
    types = torch.cat([f['node_type'] for f in frames]).cuda()
    real = _lib.lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name == 'hgn_radius_edges_batch_fill':
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, 'lib', lambda: Spy())
    s, r, off = features.radius_edges_batch(pos, types, 2, RADIUS, OBSTACLE, NORMAL)
    assert s.shape == (0,) and r.shape == (0,) and s.dtype == torch.int64 and s.is_cuda and off.tolist() == [0, 0, 0]
    assert calls == []
    s, r, off = features.radius_edges_batch(pos, types, 2, 0.05, -1, -1)        # the spy does see a fill that happens
    assert s.shape[0] > 0 and calls == ['hgn_radius_edges_batch_fill']


# ----------------------------------------------------------------------------------------------------------------
# the models
# ----------------------------------------------------------------------------------------------------------------
def model_pair(kind, connector='none', network=False):
    """Two models of one kind with the same warm statistics (and, through the copy, the same clusters and -- ``network`` -- the
    same weights), and the B frames of the case."""
    from hgn_amd import system_model
    if kind == 'cylinder':
        frames = [synth.cylinder_frame(seed=70 + i, nx=9, ny=7) for i in range(4)]
        warm, cls = synth.cylinder_frame(seed=1, nx=9, ny=7), system_model.CylinderModel
    elif kind == 'plate':
        frames = plate_frames(4, seed0=40, empty=2)
        warm, cls = synth.plate_frame(seed=1), system_model.PlateModel
    else:
        frames = [synth.flag_frame(seed=80 + i, nx=9, ny=7) for i in range(4)]
        warm, cls = synth.flag_frame(seed=1, nx=9, ny=7), system_model.FlagModel
    a = cls(params(connector))
    w = cuda_frame(warm)
    with torch.no_grad():
        g = a.build_graph(w, True)
        a.get_target(w, True)
        g = a.expand_graph(g, 0, 10 ** 9, True)             # step 0: clusters (scikit-learn, once)
        if network:
            a(g)                                            # the lazy first layers take their shape
    b = copy.deepcopy(a)
    if connector != 'none':                                 # both routes use the very same cluster lists
        b._remote_graph._clusters, b._remote_graph._neighbors = a._remote_graph._clusters, a._remote_graph._neighbors
    return a, b, frames


def assert_same_sets(got, ref):
    assert [e.name for e in got.edge_sets] == [e.name for e in ref.edge_sets]
    for e, f in zip(got.edge_sets, ref.edge_sets):
        assert torch.equal(e.senders, f.senders) and torch.equal(e.receivers, f.receivers), e.name
        assert e.features.shape == f.features.shape and torch.equal(e.features, f.features), e.name
    assert len(got.node_features) == len(ref.node_features)
    for k, (x, y) in enumerate(zip(got.node_features, ref.node_features)):
        assert x.shape == y.shape and torch.equal(x, y), f'node part {k}'


@pytest.mark.parametrize('kind', ['cylinder', 'plate'])
def test_build_graph_batch_equals_per_frame_graphs_with_frozen_normalisers(kind):
    """6."""
    from hgn_amd import batching
    a, b, frames = model_pair(kind)
    B, N = len(frames), frames[0]['node_type'].shape[0]
    per = [a.build_graph(cuda_frame(f), False) for f in frames]
    ref = batching.batch_graphs(per)
    got = b.build_graph_batch(stack(frames), False)
    assert_same_sets(got, ref)
    assert got.node_features[0].shape[0] == B * N
    assert torch.equal(got.target_feature, torch.cat([g.target_feature for g in per]))
    assert torch.equal(got.mesh_features, torch.cat([g.mesh_features for g in per]))
    un = got.unnormalized_edges
    assert un.name == 'mesh_edges' and torch.equal(un.features, torch.cat([g.unnormalized_edges.features for g in per]))
    assert torch.equal(un.senders, ref.edge_sets[0].senders) and torch.equal(un.receivers, ref.edge_sets[0].receivers)
    assert got.model_type == per[0].model_type
    if kind == 'plate':
        assert [e.name for e in got.edge_sets] == ['mesh_edges', 'world_edges']
        counts = [g.edge_sets[1].senders.shape[0] for g in per]
        assert counts[2] == 0 and min(counts[0], counts[1], counts[3]) >= 1
        assert got.obstacle_nodes.shape == (B * N,)
        assert torch.equal(got.obstacle_nodes, torch.cat([g.obstacle_nodes for g in per]))
        assert got.node_dynamic is None
    else:
        assert got.obstacle_nodes is None and got.node_dynamic == []
    # a mesh_pos handed in per frame gives the same graph
    st = stack(frames)
    st['mesh_pos'] = torch.stack([f['mesh_pos'] for f in frames]).cuda()
    assert_same_sets(b.build_graph_batch(st, False), ref)


@pytest.mark.parametrize('kind', ['cylinder', 'plate'])
def test_build_graph_batch_accumulates_the_statistics_of_the_whole_batch(kind):
    """7. One accumulate over the batch == B accumulates over the frames."""
    a, b, frames = model_pair(kind)
    for f in frames:
        a.build_graph(cuda_frame(f), True)
    b.build_graph_batch(stack(frames), True)
    names = ['_node_normalizer', '_mesh_edge_normalizer'] + (['_world_edge_normalizer'] if kind == 'plate' else [])
    for name in names:
        na, nb = getattr(a, name), getattr(b, name)
        assert float(nb._acc_count) > 0 and torch.equal(na._acc_count, nb._acc_count), name
        torch.testing.assert_close(na._acc_sum, nb._acc_sum, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(na._acc_sum_squared, nb._acc_sum_squared, rtol=1e-5, atol=1e-4)
        assert float(nb._num_accumulations) == float(na._num_accumulations) - (len(frames) - 1), name


RMP_CASES = [('plate', 'hetero'), ('flag', 'hyper'), ('flag', 'multi'), ('plate', 'multi')]


@pytest.mark.parametrize('kind,connector', RMP_CASES, ids=[f'{k}-{c}' for k, c in RMP_CASES])
def test_expand_graph_batch_equals_per_frame_expansion(kind, connector):
    """8. Remote message passing over the union == batch_graphs of the per-frame expansions: ids of every set and both node parts,
    and the features, bit for bit (hyper node k of graph b = B*N + b*K + k; every remote set graph-major)."""
    from hgn_amd import batching
    a, b, frames = model_pair(kind, connector)
    B, K = 3, 4
    frames = frames[1:]                                     # plate: the frame without world edges is now the middle one
    N = frames[0]['node_type'].shape[0]
    with torch.no_grad():
        per = [a.expand_graph(a.build_graph(cuda_frame(f), False), 1 + i, 10 ** 9, False) for i, f in enumerate(frames)]
        ref = batching.batch_graphs(per)
        got = b.expand_graph_batch(b.build_graph_batch(stack(frames), False), B, 1, 10 ** 9, False)
    assert b._remote_graph._clusters is a._remote_graph._clusters
    assert_same_sets(got, ref)
    assert got.node_features[0].shape[0] == B * N and got.node_features[1].shape[0] == B * K
    if connector != 'multi':
        inter = [e for e in got.edge_sets if e.name == 'inter_cluster'][0]
        assert int(inter.senders.min()) >= B * N and int(inter.senders.max()) < B * N + B * K
        up = [e for e in got.edge_sets if e.name == 'intra_cluster_to_cluster'][0]
        assert bool((torch.div(up.receivers - B * N, K, rounding_mode='floor') == torch.div(up.senders, N, rounding_mode='floor')).all())


@pytest.mark.parametrize('kind', ['plate', 'flag'])
def test_multi_connector_with_a_balancer_keeps_only_mesh_and_world_edges(kind):
    """The `multi` connector folds the remote sets into 'mesh_edges' and hands on 'world_edges' alone, where the model has them: the
    'balance' set a configured balancer appended in front of it is dropped, as in the reference (multigraph_connector.py:83)."""
    import numpy as np
    from hgn_amd import system_model
    balancer = {'algorithm': 'random', 'frequency': 1, 'remove_edges': False, 'random': {'edge_amount': 4}}
    if kind == 'plate':
        frame, cls, want = synth.plate_frame(seed=3), system_model.PlateModel, ['mesh_edges', 'world_edges']
    else:
        frame, cls, want = synth.flag_frame(seed=3, nx=7, ny=6), system_model.FlagModel, ['mesh_edges']
    model = cls(params('multi', balancer=balancer))
    assert 'balance' in model._edge_sets
    np.random.seed(0)
    with torch.no_grad():
        g = model.build_graph(cuda_frame(frame), True)
        n_mesh, width = g.edge_sets[0].senders.shape[0], g.edge_sets[0].features.shape[1]
        world = g.edge_sets[1] if kind == 'plate' else None
        mg = model.expand_graph(g, 0, 5, True)
    assert [e.name for e in mg.edge_sets] == want
    N, K = frame['node_type'].shape[0], 4
    M = sum(int(c.numel()) for c in model._remote_graph._clusters)
    P = mg.edge_sets[0].senders.shape[0] - n_mesh - 2 * M          # inter-cluster edges: what is left after mesh + up + down
    assert P >= 2 and P % 2 == 0                                    # no room for the 4 balance edges: 4 is not added on top
    assert mg.edge_sets[0].features.shape[1] == width + 4
    assert int(mg.edge_sets[0].features[:, width:].sum()) == mg.edge_sets[0].senders.shape[0]      # one tag per row
    assert int(mg.edge_sets[0].features[:, width + 1].sum()) == 2 * len(model._remote_graph._neighbors) == P
    assert mg.node_features[0].shape[0] == N and mg.node_features[1].shape[0] == K
    if kind == 'plate':
        assert mg.edge_sets[1] is world


def test_expand_graph_batch_clusters_the_first_frame_of_the_batch():
    """Step 0 of a trajectory: the clusters come from rows [0, N) of the union with its mesh edges, through remove_obstacles for
    the plate -- the lists expand_graph computes from the first frame."""
    from hgn_amd import system_model
    frames = plate_frames(3, seed0=50, empty=1)
    a, b = system_model.PlateModel(params('hetero')), system_model.PlateModel(params('hetero'))
    with torch.no_grad():
        a.expand_graph(a.build_graph(cuda_frame(frames[0]), True), 0, 5, True)
        got = b.expand_graph_batch(b.build_graph_batch(stack(frames), True), 3, 0, 5, True)
    ca, cb = a._remote_graph._clusters, b._remote_graph._clusters
    assert len(ca) == len(cb) == 4 and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(ca, cb))
    assert [tuple(t.tolist()) for t in a._remote_graph._neighbors] == [tuple(t.tolist()) for t in b._remote_graph._neighbors]
    N = frames[0]['node_type'].shape[0]
    obstacle = set(torch.nonzero(frames[0]['node_type'][:, 0] == OBSTACLE).flatten().tolist())
    assert not obstacle & set(torch.cat([c.cpu() for c in cb]).tolist())
    assert got.node_features[1].shape[0] == 3 * 4 and got.node_features[0].shape[0] == 3 * N
    # without a connector the union comes back as a plain MultiGraph
    c = system_model.PlateModel(params('none'))
    g = c.build_graph_batch(stack(frames), True)
    mg = c.expand_graph_batch(g, 3, 0, 5, True)
    assert type(mg).__name__ == 'MultiGraph' and mg._fields == ('node_features', 'edge_sets')
    assert mg.node_features is g.node_features and mg.edge_sets is g.edge_sets


@pytest.mark.parametrize('kind,connector', [('cylinder', 'none'), ('plate', 'hetero')], ids=['cylinder', 'plate-hetero'])
def test_network_and_training_step_on_a_batched_graph(kind, connector):
    """9. The network's output, the loss of a training step and parameter gradients: equal on both routes."""
    from hgn_amd import batching
    a, b, frames = model_pair(kind, connector, network=True)
    B = len(frames)
    per = [a.expand_graph(a.build_graph(cuda_frame(f), False), 1 + i, 10 ** 9, False) for i, f in enumerate(frames)]
    ref = batching.batch_graphs(per)
    stacked = stack(frames)
    got = b.expand_graph_batch(b.build_graph_batch(stacked, False), B, 1, 10 ** 9, False)
    out_a, out_b = a(ref), b(got)
    assert out_b.shape == (B * frames[0]['node_type'].shape[0], 3) and bool(torch.isfinite(out_b).all())
    assert torch.equal(out_a, out_b)
    cat = {k: (frames[0][k] if k in SHARED else torch.cat([f[k] for f in frames])).cuda() for k in frames[0]}
    loss_a = a.training_step(ref, cat)
    flat = b.flatten_frames(stacked)
    assert flat['cells'] is stacked['cells'] and flat['node_type'].shape == cat['node_type'].shape
    loss_b = b.training_step(got, flat)
    assert bool(torch.isfinite(loss_b)) and torch.equal(loss_a, loss_b)
    loss_a.backward()
    loss_b.backward()
    ga = {n: p.grad for n, p in a.learned_model.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in b.learned_model.named_parameters() if p.grad is not None}
    assert sorted(ga) == sorted(gb) and len(ga) >= 2
    names = sorted(ga)
    for n in (names[0], names[-1]):                         # one parameter of the decoder, one of the processor
        assert float(ga[n].abs().max()) > 0, n
        assert torch.equal(ga[n], gb[n]), n
    # validation_step / update work on the flattened frames as well
    with torch.no_grad():
        assert b.validation_step(got, flat) == a.validation_step(ref, cat)


def test_cylinder_build_graph_batch_carries_velocity_gradients():
    """10. d loss / d velocity through build_graph_batch and the network == the stacked per-frame gradients."""
    from hgn_amd import batching
    a, b, frames = model_pair('cylinder', network=True)
    B = len(frames)
    vel = [f['velocity'].cuda().requires_grad_(True) for f in frames]
    per_frames = [dict(cuda_frame(f), velocity=v) for f, v in zip(frames, vel)]
    per = [a.build_graph(f, False) for f in per_frames]
    assert all(g.node_features[0].requires_grad for g in per)
    cat = {k: (per_frames[0][k] if k in SHARED else torch.cat([f[k] for f in per_frames])) for k in per_frames[0]}
    a.training_step(batching.batch_graphs(per), cat).backward()
    want = torch.stack([v.grad for v in vel])
    stacked = stack(frames)
    stacked['velocity'].requires_grad_(True)
    g = b.build_graph_batch(stacked, False)
    assert g.node_features[0].requires_grad and g.target_feature.requires_grad
    assert not g.unnormalized_edges.features.requires_grad
    b.training_step(b.expand_graph_batch(g, B, 1, 10 ** 9, False), b.flatten_frames(stacked)).backward()
    got = stacked['velocity'].grad
    assert got is not None and got.shape == want.shape and float(want.abs().max()) > 0
    err = rel_err(got, want)
    print(f'cylinder velocity gradient, batched vs per frame: rel_err={err:.3e} bit_equal={bool(torch.equal(got, want))}')
    assert err <= TOL_GRAD
    # every term of this gradient is formed row by row (the encoder's input gradient, the normaliser's and the node-feature
    # backward are element-wise over rows; nothing is summed across frames): the same bits on both routes
    assert torch.equal(got, want)


def test_batched_calls_refuse_what_they_cannot_do():
    """11."""
    from hgn_amd import _lib, system_model
    frames = plate_frames(2, seed0=60, empty=1)
    st = stack(frames)
    st['world_pos'].requires_grad_(True)
    with pytest.raises(_lib.HgnError, match='build_graph_batch'):
        system_model.PlateModel(params('none')).build_graph_batch(st, False)
    flag = [synth.flag_frame(seed=90 + i, nx=6, ny=5) for i in range(2)]
    balanced = system_model.FlagModel(params('none', balancer={'algorithm': 'random', 'frequency': 1, 'remove_edges': False,
                                                                'random': {'edge_amount': 4}}))
    g = balanced.build_graph_batch(stack(flag), False)
    with pytest.raises(_lib.HgnError, match='expand_graph_batch.*balancer'):
        balanced.expand_graph_batch(g, 2, 0, 5, False)
    hyper = system_model.FlagModel(params('hyper'))
    st = stack(flag)
    st['world_pos'].requires_grad_(True)
    g = hyper.build_graph_batch(st, False)
    assert g.node_features[0].requires_grad
    with pytest.raises(_lib.HgnError, match='expand_graph_batch.*not differentiable'):
        hyper.expand_graph_batch(g, 2, 0, 5, False)
    assert hyper._remote_graph._clusters is None             # refused before any clustering


# ----------------------------------------------------------------------------------------------------------------
# one body behind build_graph and build_graph_batch; run-time caches
# ----------------------------------------------------------------------------------------------------------------
ACCUMULATORS = ('_acc_sum', '_acc_sum_squared', '_acc_count', '_num_accumulations')


def same(x, y):
    """Two graph fields: tensors by torch.equal, EdgeSets field by field, lists element by element, the rest by ==."""
    if torch.is_tensor(x) or torch.is_tensor(y):
        return torch.is_tensor(x) and torch.is_tensor(y) and x.shape == y.shape and torch.equal(x, y)
    if isinstance(x, (list, tuple)) and not hasattr(x, '_fields'):
        return type(x) is type(y) and len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
    if hasattr(x, '_fields'):
        return type(x) is type(y) and all(same(getattr(x, f), getattr(y, f)) for f in x._fields)
    return x == y


def assert_same_graph(got, ref):
    assert_same_sets(got, ref)
    for field in ('target_feature', 'mesh_features', 'unnormalized_edges', 'node_dynamic', 'obstacle_nodes', 'model_type'):
        assert same(getattr(got, field), getattr(ref, field)), field


def leading_one(frame):
    return {k: (v if k == 'cells' else v.unsqueeze(0)) for k, v in cuda_frame(frame).items()}


ONE_FRAME_CASES = [('flag', 0, None), ('cylinder', 0, None), ('plate', 0, True), ('plate', 2, False)]


@pytest.mark.parametrize('kind,index,world', ONE_FRAME_CASES, ids=['flag', 'cylinder', 'plate-world-edges', 'plate-no-world-edge'])
def test_a_batch_of_one_frame_is_that_frame(kind, index, world):
    """12. build_graph_batch of one frame with a leading dimension of 1 == build_graph of that frame: every field, and after an
    accumulating build every accumulator of every normaliser, bit for bit (the same kernels over the same rows)."""
    from hgn_amd.normalizer import Normalizer
    a, b, frames = model_pair(kind)
    frame = frames[index]
    for is_training in (False, True):
        one = a.build_graph(cuda_frame(frame), is_training)
        got = b.build_graph_batch(leading_one(frame), is_training)
        assert_same_graph(got, one)
        if world is not None:
            count = one.edge_sets[1].senders.shape[0]
            assert count >= 1 if world else count == 0
    na = {n: m for n, m in a.named_modules() if isinstance(m, Normalizer)}
    nb = {n: m for n, m in b.named_modules() if isinstance(m, Normalizer)}
    assert sorted(na) == sorted(nb) and len(na) >= 7
    for name in na:
        for acc in ACCUMULATORS:
            assert torch.equal(getattr(na[name], acc), getattr(nb[name], acc)), (name, acc)
    assert float(a._node_normalizer._num_accumulations) == 2.0          # the warm-up frame and the accumulating build


def test_run_time_caches_do_not_travel_in_copies_and_pickles():
    """13. After a build_graph and a build_graph_batch a PlateModel holds every topology cache; a deep copy, a pickle round trip
    and a checkpoint from before the caches existed start without them, hold the same weights and build the same graphs."""
    import pickle
    from hgn_amd import system_model
    model, _, frames = model_pair('plate', network=True)
    caches = system_model.AbstractSystemModel._RUNTIME_CACHES
    assert set(caches) == {'_fwd_cache', '_cells_key', '_cells_edges', '_batch_edges_key', '_batch_edges', '_nbr_key', '_nbr'}
    frame, stacked = cuda_frame(frames[0]), stack(frames[:2])
    with torch.no_grad():
        one, union = model.build_graph(frame, False), model.build_graph_batch(stacked, False)
    assert all(getattr(model, name) is not None for name in caches if name != '_fwd_cache')
    old_state = copy.deepcopy(model.__getstate__())
    for name in caches:
        old_state.pop(name, None)
    old = system_model.PlateModel.__new__(system_model.PlateModel)
    old.__setstate__(old_state)
    assert not any(name in old.__dict__ for name in caches)
    for twin in (copy.deepcopy(model), pickle.loads(pickle.dumps(model)), old):
        assert all(getattr(twin, name) is None for name in caches)
        sd, ref = twin.state_dict(), model.state_dict()
        assert list(sd) == list(ref) and len(sd) >= 2 and all(torch.equal(sd[k], ref[k]) for k in ref)
        with torch.no_grad():
            assert_same_graph(twin.build_graph(frame, False), one)
            assert_same_graph(twin.build_graph_batch(stacked, False), union)
        assert all(getattr(twin, name) is not None for name in caches if name != '_fwd_cache')
    assert all(getattr(model, name) is not None for name in caches if name != '_fwd_cache')      # the live model keeps its own
