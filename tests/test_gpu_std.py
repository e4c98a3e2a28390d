"""`message_passing_aggregator='std'` on the HIP path (graphnet.py:50-70 -> src/util.py:129-130 -> torch_scatter.scatter_std): the
five-operation streaming segment reduce (include/hgn_mp.h: hgn_segment_reduce5_*) as an operator, in mixed op lists, in its two backward
forms, and inside the models -- plain blocks, node parts, the public stage API, a captured training step.

Tolerances are the project's (helpers.rel_err, norm-wise): operators 2e-6 on values and 2e-5 on gradients (test_g1_segment_std_golden),
models 1e-5 on outputs and 2e-5 on gradients, 2e-5 on outputs against the reference's own fp32 numbers."""
import ctypes as C
import os

import pytest
import torch

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD = 1e-5, 2e-5
FIXTURE = os.path.join(H.GOLDEN, 'stdagg_none_L2_lat128.pt')
HYPER_SETS = ['mesh_edges', 'intra_cluster_to_mesh', 'intra_cluster_to_cluster', 'inter_cluster']


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


# ---------------------------------------------------------------------------------------------------------------
# 3. the operator against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
def _ids_with_lengths(lengths, gen):
    """Segment ids (in random row order) of segments with exactly these lengths, segment numbers shuffled."""
    order = torch.randperm(len(lengths), generator=gen)                       # segment order[i] gets lengths[i] rows
    ids = torch.repeat_interleave(order, torch.tensor(lengths))
    return ids[torch.randperm(ids.numel(), generator=gen)]


def _case(name):
    """-> (ids [E], N, offset of the rows): every populated segment holds >= 2 rows (random, hence distinct)."""
    gen = torch.Generator().manual_seed(31)
    if name in ('random', 'offset100'):
        ids, N = torch.randint(0, 40, (600,), generator=gen), 40
    elif name == 'lengths':             # empty segments, every number of rows in flight, more rows than the registers keep, > one 64-row tile
        ids, N = _ids_with_lengths([0, 2, 3, 4, 5, 9, 70], gen), 7
        assert sorted(torch.bincount(ids, minlength=N).tolist()) == [0, 2, 3, 4, 5, 9, 70]
    elif name == 'one_segment':
        ids, N = torch.zeros(5, dtype=torch.long), 1
    else:
        ids, N = torch.zeros(0, dtype=torch.long), 5
    cnt = torch.bincount(ids, minlength=N)
    assert not bool((cnt == 1).any())
    return ids, N, (100.0 if name == 'offset100' else 0.0)


def _hip_aggregate(data, ids, N, ops, path, w):
    """ops.aggregate on the device: `sorted` = rows put into segment order first (perm = None: the layout of the model path),
    `perm` = rows in the caller's order, read through the CSR permutation.  -> (out, gradient in the caller's row order)."""
    from hgn_amd import ops as hops, topology
    csr = topology.segment_csr(ids.cuda(), N, torch.device('cuda'))
    x = data.clone().cuda().requires_grad_(True)
    if path == 'sorted':
        y = hops.aggregate([x.index_select(0, csr.perm.long())], [(None, csr.rowptr, csr.seg)], ops)
    else:
        y = hops.aggregate([x], [(csr.perm, csr.rowptr, csr.seg)], ops)
    (y * w.float().cuda()).sum().backward()
    return y.detach(), x.grad


def _oracle_aggregate(data, ids, N, ops, gen):
    xo = data.clone().double().requires_grad_(True)
    yo = torch.cat([O.segment_reduce(xo, ids, N, op) for op in ops], dim=1)
    w = torch.randn(yo.shape, generator=gen, dtype=torch.float64)
    (yo * w).sum().backward()
    return yo.detach(), xo.grad, w


@pytest.mark.parametrize('path,D', [('sorted', 128), ('perm', 128), ('perm', 3), ('perm', 1)], ids=['sorted128', 'perm128', 'generic3', 'generic1'])
@pytest.mark.parametrize('case', ['random', 'lengths', 'one_segment', 'no_rows', 'offset100'])
def test_std_operator_vs_oracle_fp64(case, path, D):
    """Values to 2e-6, gradients (random upstream weights) to 2e-5 of the fp64 oracle's segment_reduce; an empty segment is exactly 0.
    `offset100` (rows = 100 + N(0, 1)) is where a running sum and sum of squares is 2e-3 ... 4e-3 off: the kernels take two sweeps."""
    ids, N, off = _case(case)
    gen = torch.Generator().manual_seed(7)
    data = off + torch.randn(ids.numel(), D, generator=gen)
    yo, go, w = _oracle_aggregate(data, ids, N, ('std',), gen)
    y, g = _hip_aggregate(data, ids, N, ('std',), path, w)
    ev, eg = H.rel_err(y, yo), H.rel_err(g, go)
    print(f'std operator {case}/{path}/D={D}: values {ev:.2e} gradients {eg:.2e}')
    assert tuple(y.shape) == (N, D) and ev <= 2e-6
    assert bool(torch.isfinite(g).all()) and eg <= 2e-5
    empty = (torch.bincount(ids, minlength=N) == 0).nonzero().flatten()
    assert empty.numel() == 0 or float(y[empty.cuda()].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# 4. segments without variance: NaN exactly where the reference has it
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path,D', [('sorted', 128), ('perm', 128), ('perm', 3)], ids=['sorted128', 'perm128', 'generic3'])
def test_std_nan_parity_for_segments_without_variance(path, D):
    """One segment of ONE row and one of three IDENTICAL rows among ordinary ones: both values are 0, their rows' gradients are NaN
    (0 / 0: the wheel's sqrt'(0) * 0) and nothing else is -- the oracle's mask; the finite rows agree to 2e-5."""
    gen = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randint(0, 6, (60,), generator=gen), torch.tensor([6, 7, 7, 7])])
    ids[ids == 2] = 3                                                         # (segment 2 is empty)
    data = torch.randn(64, D, generator=gen)
    data[61:] = (torch.randn(1, D, generator=gen) * 4).round() / 2            # halves: three of them sum exactly, in fp32 and in fp64
    shuffle = torch.randperm(64, generator=gen)
    ids, data = ids[shuffle], data[shuffle]
    yo, go, w = _oracle_aggregate(data, ids, 8, ('std',), gen)
    y, g = _hip_aggregate(data, ids, 8, ('std',), path, w)
    special = (ids == 6) | (ids == 7)
    assert torch.equal(torch.isnan(go), special.unsqueeze(1).expand_as(go))    # what the oracle does
    assert H.rel_err(y, yo) <= 2e-6 and float(y[6:8].abs().max()) == 0.0 and float(y[2].abs().max()) == 0.0
    assert torch.equal(torch.isnan(g).cpu(), torch.isnan(go))
    assert H.rel_err(g.cpu()[~special], go[~special]) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 5. 'std' in any slot of a list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path,D', [('sorted', 128), ('perm', 128), ('perm', 3)], ids=['sorted128', 'perm128', 'generic3'])
@pytest.mark.parametrize('ops', [('std', 'sum'), ('sum', 'mean', 'max', 'std'), ('std',), ('min', 'std', 'std')], ids='-'.join)
def test_std_in_mixed_lists(ops, path, D):
    """Every sum / mean / max / min slot is the single-op result of the four-operation entries bit for bit, every `std` slot the
    ('std',) result bit for bit; the gradient of the whole list against the fp64 oracle."""
    ids, N, _ = _case('lengths')
    gen = torch.Generator().manual_seed(11)
    data = torch.randn(ids.numel(), D, generator=gen)
    yo, go, w = _oracle_aggregate(data, ids, N, ops, gen)
    y, g = _hip_aggregate(data, ids, N, ops, path, w)
    for s, op in enumerate(ops):
        single, _ = _hip_aggregate(data, ids, N, (op,), path, w[:, s * D:(s + 1) * D])
        assert torch.equal(y[:, s * D:(s + 1) * D], single), (s, op)
    assert H.rel_err(y, yo) <= 2e-6
    assert H.rel_err(g, go) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 6. the two backward forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_base', [True, False])
@pytest.mark.parametrize('codes', [(4,), (4, 2), (0, 1, 3, 4)], ids=['std', 'std_max', 'sum_mean_min_std'])
@pytest.mark.parametrize('N,max_deg,seed', [(60, 70, 0), (1237, 9, 1)])
def test_std_backward_sorted_equals_edge_parallel_bit_for_bit(N, max_deg, seed, codes, with_base):
    """hgn_segment_reduce5_bwd_sorted (one half-wave per segment: what the edge block's backward runs) gives the bits of
    hgn_segment_reduce5_bwd (one per row) on rows in segment order, with and without the d(e') base, ragged and empty segments."""
    from hgn_amd import _lib, topology
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(1, max_deg + 1, (N,), generator=gen)
    deg[deg == 1] = 0                                                         # empty segments, none without variance
    receivers = torch.repeat_interleave(torch.arange(N), deg)
    E, k = receivers.shape[0], len(codes)
    topo = topology.EdgeTopology(torch.randint(0, N, (E,), generator=gen), receivers, N, torch.device('cuda'))
    data = torch.randn(E, 128, generator=gen).cuda()
    L, st = _lib.lib(), _lib.stream_ptr()
    ops = (C.c_int32 * k)(*codes)
    agg = torch.empty(N, k * 128, device='cuda'); mean = torch.empty(N, 256, device='cuda')      # two fp32 words per column
    amax = torch.empty(N, 128, dtype=torch.int32, device='cuda'); amin = torch.empty_like(amax)
    _lib.check(L.hgn_segment_reduce5_fwd(data.data_ptr(), 128, 128, None, topo.r.rowptr.data_ptr(), N, ops, k, agg.data_ptr(), k * 128,
                                         amax.data_ptr(), amin.data_ptr(), mean.data_ptr(), 256, st), 'fwd')
    d_agg = torch.randn(N, k * 128, generator=gen).cuda()
    base = torch.randn(E, 128, generator=gen).cuda() if with_base else None
    bp = base.data_ptr() if base is not None else None
    ref = torch.full((E, 128), float('nan'), device='cuda'); got = torch.full((E, 128), float('nan'), device='cuda')
    tail = (data.data_ptr(), 128, agg.data_ptr(), k * 128, mean.data_ptr(), 256, st)
    _lib.check(L.hgn_segment_reduce5_bwd(d_agg.data_ptr(), k * 128, 128, None, topo.rcv.data_ptr(), topo.r.rowptr.data_ptr(), E, ops, k,
                                         amax.data_ptr(), amin.data_ptr(), bp, ref.data_ptr(), 128, *tail), 'edge-parallel')
    _lib.check(L.hgn_segment_reduce5_bwd_sorted(d_agg.data_ptr(), k * 128, topo.r.rowptr.data_ptr(), N, ops, k, amax.data_ptr(), amin.data_ptr(),
                                                bp, got.data_ptr(), 128, *tail), 'segment-parallel')
    assert bool(torch.isfinite(ref).all()) and torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------
# 7. plain blocks: the model against the fp64 oracle and against the reference's fixture
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [2, 15], ids=['L2', 'L15'])
def test_std_model_plain_blocks_vs_oracle_and_reference_fixture(steps):
    """MeshGraphNet('none', 'std') on the fixture's 8 x 6 triangulated grid (every node receives >= 2 edges: nothing is NaN):
    outputs to 1e-5 of the fp64 oracle, parameter and input gradients to 2e-5 (L = 15: 5e-5) of the fp64 oracle evaluated with the HIP
    forward's ReLU gates (helpers.GateTransfer, as the `sum` tests do); at L = 2 with the fixture's own weights the outputs and the loss
    to 2e-5 of the REFERENCE's fp32 numbers.  An instance with a ReLU input within fp32 rounding of its kink (fp64 margin <= 3e-7) is
    passed over, at most four seeds are tried (test_flag_L15_sum_vs_oracle_fp64); how many were rejected goes into the parity report.
    Fails on a build without the feature with `Invalid operation type!`."""
    fx = torch.load(FIXTURE)
    graph = H.graph_from_fixture(fx)
    target, mask = fx['target'], fx['mask']
    shapes = fx['shapes'] if steps == 2 else O.param_shapes('none', 'std', steps, ['mesh_edges'], 5, {'mesh_edges': 7}, 0, 3, 128)
    first = fx['seed'] if steps == 2 else 3
    chosen = None
    for wseed in range(first, first + 4):
        sd = O.init_state_dict_like(shapes, seed=wseed)
        with H.KinkMargin() as km:
            out_o, loss_o, _, _ = H.oracle_run(sd, graph, 'none', 'std', target, mask)
        if km.worst > 3e-7:
            chosen = wseed
            break
    tid = f'test_std_model_plain_blocks_vs_oracle_and_reference_fixture[L{steps}]'
    H._REPORT.append({'test': tid, 'what': 'instance selection', 'first_seed_tried': first, 'seed_used': chosen,
                      'seeds_rejected': (chosen if chosen is not None else first + 4) - first,
                      'criterion': 'smallest |ReLU input| of the fp64 oracle run > 3e-7', 'margin_of_seed_used': km.worst})
    assert chosen is not None, 'four seeds in a row with a ReLU gate at rounding level'
    model = H.hip_model('none', 'std', steps, ['mesh_edges'], sd)
    out, loss, grads, ing, gates, _ = H.hip_run_logged(model, graph, target, mask)
    assert H.report(tid, 'output', out, out_o)['norm'] <= TOL_OUT
    assert H.rel_err(loss, loss_o) <= TOL_OUT
    with H.GateTransfer(gates) as gt:
        _, _, grads_g, ing_g = H.oracle_run(sd, graph, 'none', 'std', target, mask)
    assert all(len(v) == 0 for v in gt.gates.values())
    # One parameter has NO gradient with this aggregator: the LayerNorm bias of the LAST block's edge model.  Those edge latents are read
    # by the aggregation only, and a constant added to a column of every row moves no standard deviation.  The exact value is 0; fp64 gives
    # rounding noise (~1e-17), fp32 too (~1e-8), and a ratio of the two says nothing.  It is held against the scale of its sibling, the
    # same LayerNorm's weight gradient (a column sum over the same rows of d(e')); every other tensor on its own scale, as everywhere.
    dead = f'processor.graphnet_blocks.{steps - 1}.edge_models.mesh_edges.1.bias'
    sibling = float(grads_g[dead[:-4] + 'weight'].abs().max())
    assert float(grads_g[dead].abs().max()) <= 1e-10 * sibling
    e_dead = float(grads[dead].abs().max()) / sibling
    live = {k: v for k, v in grads_g.items() if k != dead and float(v.abs().max()) > 0}
    assert len(live) == len(grads_g) - 1
    gn, ge = H.worst_grad(grads, live)
    e_node = H.rel_err(ing['node'][0], ing_g['node'][0])
    e_edge = H.rel_err(ing['edge']['mesh_edges'], ing_g['edge']['mesh_edges'])
    H._REPORT.append({'test': tid, 'what': 'gradients vs the fp64 oracle with the HIP gates', 'param_norm': gn, 'param_elem': ge,
                      'zero_gradient_vs_sibling_scale': e_dead, 'node_input': e_node, 'edge_input': e_edge, 'gates_differing_from_fp64': gt.flipped})
    print(tid, 'param grads', gn, 'zero gradient / sibling scale', e_dead, 'input grads', e_node, e_edge, 'gates flipped', gt.flipped)
    bound = TOL_GRAD if steps == 2 else 5e-5
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert gn <= bound and e_dead <= bound and e_node <= bound and e_edge <= bound
    if steps == 2:
        if chosen != fx['seed']:                  # the fixture's numbers belong to the fixture's weights
            model = H.hip_model('none', 'std', 2, ['mesh_edges'], O.init_state_dict_like(fx['shapes'], fx['seed']))
            out, loss, _, _ = H.hip_run(model, graph, target, mask)
        assert H.report(tid, 'output vs the reference fixture', out, fx['out'])['norm'] <= 2e-5
        assert H.rel_err(loss, fx['loss']) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 8. node parts: mesh rows and hyper rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arch', ['hyper', 'hetero'])
def test_std_model_with_node_parts_forward_vs_oracle(arch):
    """`hyper` and `hetero` with `std` on a small clustered grid, forward only: `intra_cluster_to_mesh` hands every mesh node ONE row, so
    that aggregate is 0 everywhere (the one-row case, through parts = (off_s, off_r)) -- and its gradient is NaN in the reference itself,
    which is why there is NO gradient assertion for these schedules.  Outputs to 1e-5 of the fp64 oracle under torch.no_grad(); the
    training-mode forward (which also writes the means and the saves) gives the same bits."""
    graph = synth.grid_graph(seed=5, nx=8, ny=6, clusters=4)
    assert [e.name for e in graph.edge_sets if e.name in HYPER_SETS] and len(graph.node_features) == 2
    sets = [e.name for e in graph.edge_sets]
    down = next(e for e in graph.edge_sets if e.name == 'intra_cluster_to_mesh')
    assert torch.equal(torch.bincount(down.receivers, minlength=48)[:48], torch.ones(48, dtype=torch.long))
    edge_in = {e.name: e.features.shape[1] for e in graph.edge_sets}
    nsn = {'node_model_cross': len(sets), 'hyper_node_model_cross': len(sets)} if arch == 'hetero' else None
    shapes = O.param_shapes(arch, 'std', 2, sets, graph.node_features[0].shape[1], edge_in, graph.node_features[1].shape[1], 3, 128, nsn)
    sd = O.init_state_dict_like(shapes, seed=12)
    order = ['mesh_edges', 'world_edges', 'inter_cluster', 'inter_cluster_world']
    with torch.no_grad():
        out_o = O.mesh_graph_net({k: v.double() for k, v in sd.items()},
                                 O.MultiGraph([x.double() for x in graph.node_features],
                                              [e._replace(features=e.features.double()) for e in graph.edge_sets]), arch, 'std', set_order=order)
    model = H.hip_model(arch, 'std', 2, sets, sd, set_order=order)
    G = H.hip_graph(graph.node_features, graph.edge_sets)
    with torch.no_grad():
        out = model(G)
    assert bool(torch.isfinite(out).all())
    assert H.report(f'test_std_model_with_node_parts_forward_vs_oracle[{arch}]', 'output', out, out_o)['norm'] <= TOL_OUT
    out_train = model(G)
    assert out_train.requires_grad and torch.equal(out_train.detach(), out)


# ---------------------------------------------------------------------------------------------------------------
# 9. the public stage API and a captured training step
# ---------------------------------------------------------------------------------------------------------------
def test_std_graphnet_block_on_a_public_multigraph_vs_oracle():
    """GraphNet(..., 'std', ...) called with a MultiGraph (rows in the caller's order, receivers unsorted) against helpers.oracle_block:
    node latents, edge latents in the caller's row order, parameter and input gradients of a random linear functional."""
    fx = torch.load(FIXTURE)
    graph = H.with_unsorted_receivers(H.graph_from_fixture(fx), seed=1)
    assert H.receivers_unsorted(graph)
    sd = O.init_state_dict_like(fx['shapes'], seed=21)
    gen = torch.Generator().manual_seed(2)
    es = graph.edge_sets[0]
    h, e = torch.randn(48, 128, generator=gen), torch.randn(es.senders.numel(), 128, generator=gen)
    ch, ce = torch.randn(48, 128, generator=gen, dtype=torch.float64), torch.randn(e.shape, generator=gen, dtype=torch.float64)
    sd64 = H.oracle_params(sd)
    g64 = H.oracle_graph([h], [('mesh_edges', e, es.senders, es.receivers)])
    r64 = H.oracle_block(sd64, 0, g64, 'none', 'std')
    ((r64.node_features[0] * ch).sum() + (r64.edge_sets[0].features * ce).sum()).backward()
    import hgn_amd
    model = H.hip_model('none', 'std', 2, ['mesh_edges'], sd)
    block = model.processor.graphnet_blocks[0]
    assert type(block) is hgn_amd.modules.GraphNet and block.message_passing_aggregator == 'std'
    G = H.hip_graph([h], [('mesh_edges', e, es.senders, es.receivers)])
    model.zero_grad(set_to_none=True)
    r = block(G)
    ((r.node_features[0] * ch.float().cuda()).sum() + (r.edge_sets[0].features * ce.float().cuda()).sum()).backward()
    assert H.rel_err(r.node_features[0], r64.node_features[0]) <= TOL_OUT
    assert H.rel_err(r.edge_sets[0].features, r64.edge_sets[0].features) <= TOL_OUT
    assert H.rel_err(G.node_features[0].grad, g64.node_features[0].grad) <= TOL_GRAD
    assert H.rel_err(G.edge_sets[0].features.grad, g64.edge_sets[0].features.grad) <= TOL_GRAD
    pre = 'processor.graphnet_blocks.0.'
    got = {k: p.grad for k, p in model.named_parameters() if k.startswith(pre)}
    assert got and all(g is not None for g in got.values())
    worst = max((H.rel_err(g, sd64[k].grad), k) for k, g in got.items())
    assert worst[0] <= TOL_GRAD, worst


def test_std_captured_train_step_equals_the_eager_step_bit_for_bit():
    """graphs.GraphedTrainStep of the two-block none / std model on the 8 x 6 graph, replayed twice: loss and flat gradient of every
    replay are the bits of the eager trainer's step on the same weights (same kernels, same order: the reduce, its mean, the pre-pass)."""
    import hgn_amd
    from hgn_amd import graphs, parallel
    fx = torch.load(FIXTURE)
    g = H.graph_from_fixture(fx)
    sd = O.init_state_dict_like(fx['shapes'], fx['seed'])
    G = hgn_amd.MultiGraph([x.cuda() for x in g.node_features],
                           [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in g.edge_sets])
    target, mask = fx['target'].cuda(), fx['mask'].cuda()
    eager = parallel.DataParallelTrainer(H.hip_model('none', 'std', 2, ['mesh_edges'], sd), lr=1e-3, device_step=True)
    captured = parallel.DataParallelTrainer(H.hip_model('none', 'std', 2, ['mesh_edges'], sd), lr=1e-3, device_step=True)
    gs = graphs.GraphedTrainStep(captured, G, target, mask, warmup=1)
    eager.step(G, target, mask)                                        # the warm-up step; the capture itself executes nothing
    for replay in range(2):
        l_e = eager.step(G, target, mask).clone()
        l_g = gs().clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(captured.fp.grad).all()) and float(captured.fp.grad.abs().max()) > 0
        assert torch.equal(l_g, l_e), (replay, float(l_g), float(l_e))
        assert torch.equal(captured.fp.grad, eager.fp.grad), (replay, H.rel_err(captured.fp.grad, eager.fp.grad))
    assert torch.equal(captured.fp.flat, eager.fp.flat) and int(captured.t_dev) == 3
