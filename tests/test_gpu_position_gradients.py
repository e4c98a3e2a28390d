"""Position gradients through the connector and the PlateModel graph (`model.position_gradients = True`), on the GPU: the backward of
the cluster mean (include/hgn_features.h: hgn_member_mean_bwd), HierarchicalConnector / MultigraphConnector and PlateModel.build_graph
under autograd, and unrolled_training_step(through_state=True) for both.

Yardsticks and bounds.
* hgn_member_mean_bwd: a row with one membership is ONE fp32 division, compared exactly; a row in no cluster is exactly 0 in a buffer
  that held NaN; where the members are a partition of the rows the result has the bits ops.aggregate(('mean',)) differentiates to
  (hgn_segment_reduce_bwd, same expression); a row with up to three memberships is a sum of correctly rounded quotients added one by
  one: |got - exact| <= 2^-23 * sum |terms| (each quotient and each partial sum is rounded once, 2^-24 each, the partial sums are
  bounded by the sum of the magnitudes).
* connector and plate graph: torch autograd through oracle/features_oracle.py in fp64 on the CPU.  Bound as for
  hgn_rel_edge_features_bwd in test_gpu_feature_grad.py: the oracle's own fp32 autograd is run on the same inputs and the HIP result
  may be at most FACTOR = 4 times as far from fp64 (helpers.rel_err) as that.  The normaliser statistics are constants on both sides
  (the oracle's normalisers are given the mean / std the HIP normalisers hold, in the dtype the oracle runs in).  Labels, world-edge
  membership and spread winners are constants on the HIP side and decided by the values on the oracle's: the inputs are checked (fp64,
  CPU) to keep every decision away from its threshold by 1e-4 relative, so that fp32 and fp64 decide alike.
* end to end: the fp64 oracle unroll with the HIP forward's ReLU gates transferred, 1e-5 (test_gpu_unrolled_training.py, test 5);
  the per-window loop form, losses torch.equal and gradients within 1e-5 (that file, test 4); frozen against trainable 2e-6
  (test_gpu_frozen.py)."""
import pytest
import torch

from oracle import features_oracle as FO
from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests import test_gpu_feature_grad as FG
from tests import test_gpu_frozen as FZ
from tests import test_gpu_unrolled_training as UT

pytestmark = pytest.mark.gpu
FACTOR = FG.FACTOR
TOL_GRAD = UT.TOL_GRAD
GAP = 1e-4


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


# ---------------------------------------------------------------------------------------------------------------
# 1. - 3. the kernel
# ---------------------------------------------------------------------------------------------------------------
def _layout(clusters, rows):
    """Cluster lists (ids < rows; a list may be empty) -> the five index arrays of the entry, built on the CPU."""
    assert all(0 <= n < rows for c in clusters for n in c)
    sizes = torch.tensor([len(c) for c in clusters], dtype=torch.int64)
    members = torch.tensor([n for c in clusters for n in c], dtype=torch.int64)
    item_seg = torch.repeat_interleave(torch.arange(len(clusters)), sizes)
    seg_rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    node_items = torch.argsort(members, stable=True)
    node_rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(members, minlength=rows).cumsum(0)])
    i32 = lambda t: t.to(torch.int32).cuda().contiguous()
    return dict(seg_rowptr=i32(seg_rowptr), item_seg_dev=i32(item_seg),
                node_rowptr=i32(node_rowptr), node_items=i32(node_items), S=len(clusters), M=int(members.numel()), rows=rows)


def _member_mean_bwd(lay, d_mean, D, pad_out=0):
    """One call of the entry into a buffer that holds NaN.  ``d_mean`` may be a column view of a wider matrix; ``pad_out`` more
    columns make the output one."""
    from hgn_amd import _lib
    rows = lay['rows']
    slab = torch.full((rows, D + pad_out), float('nan'), device='cuda')
    out = slab[:, :D]
    ld_mean = d_mean.stride(0) if d_mean.shape[0] > 1 else D
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _lib.check(_lib.lib().hgn_member_mean_bwd(d_mean.data_ptr(), ld_mean, D, ptr(lay['seg_rowptr']), lay['S'], ptr(lay['item_seg_dev']),
                                              ptr(lay['node_rowptr']), ptr(lay['node_items']), rows, lay['M'], out.data_ptr(),
                                              D + pad_out, _lib.stream_ptr()), 'hgn_member_mean_bwd')
    if pad_out:
        assert bool(torch.isnan(slab[:, D:]).all()), 'the call wrote outside its D columns'
    return out


def _shape_clusters(shape, rows):
    """Disjoint clusters over ``rows`` rows; the rows outside every cluster are what the shape is named after."""
    ids = list(range(rows))
    if shape == 'one_segment':                       # S = 1, every row a member
        return [ids]
    if shape == 'single_and_empty':                  # a one-member cluster, an empty segment, the rest in a third
        return [ids[:1], [], ids[1:]]
    cut = max(1, rows // 4)
    if shape == 'outside_first':
        keep = ids[cut:]
    elif shape == 'outside_last':
        keep = ids[:rows - cut]
    else:                                            # 'outside_scattered': every third row belongs to no cluster
        keep = [n for n in ids if n % 3 != 1]
    keep = keep[::-1]                                # member lists need not ascend
    return [keep[0::3], keep[1::3], keep[2::3]]


SHAPES = ['one_segment', 'single_and_empty', 'outside_first', 'outside_last', 'outside_scattered']


@pytest.mark.parametrize('pad', [0, 3], ids=['packed', 'views'])
@pytest.mark.parametrize('D', [1, 10, 12])
@pytest.mark.parametrize('rows', [1, 63, 64, 65, 300])
def test_member_mean_bwd_is_one_exact_division_per_member_row_and_zero_elsewhere(rows, D, pad):
    """1. Every cluster shape at every size and width; `views`: d_mean and d_data are column slices of matrices 3 columns wider."""
    gen = torch.Generator().manual_seed(rows * 100 + D)
    for shape in SHAPES:
        clusters = _shape_clusters(shape, rows)                             # one row: some shapes leave it outside, M = 0
        lay = _layout(clusters, rows)
        S = lay['S']
        wide = torch.randn(S, D + pad, generator=gen).cuda()
        d_mean = wide[:, :D]
        got = _member_mean_bwd(lay, d_mean, D, pad_out=pad).cpu()
        assert bool(torch.isfinite(got).all()), shape
        want = torch.zeros(rows, D)
        dm = d_mean.cpu()
        for s, c in enumerate(clusters):
            if c:
                want[torch.tensor(c)] = dm[s] / torch.tensor(float(len(c)), dtype=torch.float32)     # one fp32 division
        assert torch.equal(got, want), (shape, float((got - want).abs().max()))
        outside = sorted(set(range(rows)) - {n for c in clusters for n in c})
        if outside:
            assert float(got[torch.tensor(outside)].abs().max()) == 0, shape
        if shape.startswith('outside') and rows >= 4:
            assert outside, 'the shape was meant to leave rows outside'


def test_member_mean_bwd_without_members_writes_zeros():
    lay = _layout([[], []], 65)
    got = _member_mean_bwd(lay, torch.randn(2, 10).cuda(), 10)
    assert float(got.abs().max()) == 0 and bool(torch.isfinite(got).all())


@pytest.mark.parametrize('D', [1, 10, 12])
@pytest.mark.parametrize('rows', [65, 300])
def test_member_mean_bwd_on_a_partition_has_the_bits_of_the_segment_reduce_backward(rows, D):
    """2. M = rows: the case in which ops.aggregate's own backward is valid."""
    from hgn_amd import ops, topology
    gen = torch.Generator().manual_seed(rows + D)
    S = 7
    label = torch.randint(0, S, (rows,), generator=gen)
    label[:S] = torch.arange(S)                                             # no empty segment
    csr = topology.CSR(label.cuda(), S)
    x = torch.randn(rows, D, generator=gen).cuda().requires_grad_(True)
    w = torch.randn(S, D, generator=gen).cuda()
    (ops.aggregate([x], [(csr.perm, csr.rowptr, csr.seg)], ('mean',)) * w).sum().backward()
    clusters = [torch.nonzero(label == s).flatten().tolist() for s in range(S)]
    got = _member_mean_bwd(_layout(clusters, rows), w, D)
    assert float(x.grad.abs().max()) > 0 and torch.equal(got, x.grad)


@pytest.mark.parametrize('D', [1, 10, 12])
def test_member_mean_bwd_with_rows_in_up_to_three_clusters(D):
    """3. Overlapping clusters (what intra-cluster sampling can produce): against fp64 within 2^-23 * sum |terms| per element; two runs
    give the same bits."""
    rows, S = 300, 5
    gen = torch.Generator().manual_seed(40 + D)
    clusters = [[] for _ in range(S)]
    count = torch.zeros(rows, dtype=torch.int64)
    for n in range(rows):
        k = n % 4                                                           # 0 .. 3 memberships
        for s in torch.randperm(S, generator=gen)[:k].tolist():
            clusters[s].append(n)
        count[n] = k
    lay = _layout(clusters, rows)
    d_mean = torch.randn(S, D, generator=gen).cuda()
    first, second = _member_mean_bwd(lay, d_mean, D), _member_mean_bwd(lay, d_mean, D)
    assert torch.equal(first, second) and bool(torch.isfinite(first).all())
    dm = d_mean.cpu().double()
    exact, mags = torch.zeros(rows, D, dtype=torch.float64), torch.zeros(rows, D, dtype=torch.float64)
    for s, c in enumerate(clusters):
        idx = torch.tensor(c)
        exact[idx] += dm[s] / len(c)
        mags[idx] += dm[s].abs() / len(c)
    err = (first.cpu().double() - exact).abs()
    assert int(count.max()) == 3 and bool((err <= 2.0 ** -23 * mags).all()), float((err / mags.clamp(min=1e-300)).max())
    assert float(first.cpu()[count == 0].abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------
# 4. the connector against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
def _params(connector, K, hnf=True):
    p = FG._params('sum', steps=1, connector=connector)
    p['rmp']['num_clusters'] = K
    p['rmp']['hyper_node_features'] = hnf
    return p


def _pin(oracle_norm, hip_norm, dtype):
    """FG._pin in the dtype the oracle runs in (a float64 constant would lift an fp32 oracle run to fp64)."""
    m, s = hip_norm._mean().double().cpu().to(dtype), hip_norm._std_with_epsilon().double().cpu().to(dtype)
    oracle_norm.mean, oracle_norm.std = (lambda: m), (lambda: s)


def _assert_spread_gaps(world, mesh, clusters):
    """In every cluster the two largest member distances differ by more than GAP relative, for both spreads (fp64)."""
    cf = torch.cat((world, mesh), 1).double()
    for c in clusters:
        rowsc = cf[c.long()]
        if rowsc.shape[0] < 2:
            continue
        mean = rowsc.mean(0)
        for cols in (slice(-3, None), slice(0, 3)):
            d = torch.sqrt((mean[cols] - rowsc[:, cols]).pow(2).sum(1)).sort(descending=True).values
            assert float(d[0] - d[1]) > GAP * float(d[0]), 'two members tie for a spread: choose other inputs'


def _strips(nx, ny, K):
    """K clusters of whole mesh columns (node id = i * ny + j), of unequal sizes."""
    label = [(i * K) // nx for i in range(nx) for _ in range(ny)]
    return [torch.tensor([n for n, l in enumerate(label) if l == k]) for k in range(K)], label


def _connector_case(name):
    """-> dict(model, frames (CPU), clusters, nb (list of tuples), kind, multi, hnf): a warmed model with injected clusters."""
    from hgn_amd import system_model
    torch.manual_seed(3)
    kind, multi, hnf, B = 'flag', False, True, 1
    if name in ('flag5x4_k3', 'flag5x4_k3_plain', 'flag5x4_k3_batch3'):
        nx, ny, K = 5, 4, 3
        hnf = name != 'flag5x4_k3_plain'
        B = 3 if name.endswith('batch3') else 1
    elif name == 'flag8x6_k2':
        nx, ny, K = 8, 6, 2
    elif name == 'flag8x6_k5':
        nx, ny, K = 8, 6, 5
    else:
        kind, K = 'plate', 3
        multi = name == 'plate_multi'
    if kind == 'flag':
        frames = [synth.flag_frame(seed=21 + b, nx=nx, ny=ny) for b in range(B)]
        clusters, label = _strips(nx, ny, K)
        s, r = FO.triangles_to_edges(frames[0]['cells'])
        nb = FO.neighboring_clusters(s, r, label)
        model = system_model.FlagModel(_params('hyper', K, hnf))
    else:
        first = name != 'plate_obstacle_last'
        frames = [synth.plate_frame(seed=4, obstacle_first=first)]
        free = torch.nonzero(frames[0]['node_type'][:, 0] != 1).flatten()
        lab = torch.randint(0, K, (free.numel(),), generator=torch.Generator().manual_seed(8))
        clusters, nb = [free[lab == k] for k in range(K)], []
        assert int(free[0]) == (32 if first else 0) and free.numel() < frames[0]['node_type'].shape[0]
        model = system_model.PlateModel(_params('multi' if multi else 'hetero', K, hnf))
    for f in frames:
        _assert_spread_gaps(f['world_pos'], f['mesh_pos'], clusters)
    rmp = model._remote_graph
    rmp._clusters, rmp._neighbors = clusters, [torch.tensor(p) for p in nb]
    with torch.no_grad():
        for f in frames:                                                   # the normalisers see the frames, without gradients
            model.expand_graph(model.build_graph(FG._cuda(f), True), 1, 10 ** 9, True)
    assert rmp._clusters is clusters
    model.position_gradients = True
    return dict(model=model, frames=frames, clusters=clusters, nb=nb, kind=kind, multi=multi, hnf=hnf)


def _outputs(mg):
    return list(mg.node_features) + [e.features for e in mg.edge_sets]


def _weights(outputs, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(t.shape), generator=gen) for t in outputs]


def _oracle_connect(case, base, world, nodes, weights, dtype):
    """The oracle connector on one frame's graph (``base``: the HIP graph's pass-through parts on the CPU) in ``dtype`` under
    autograd -> (d world, d nodes)."""
    model = case['model']
    ff = (FO.FlagFeatures if case['kind'] == 'flag' else FO.PlateFeatures)(dtype=dtype)
    _pin(ff.intra_edge, model._intra_edge_normalizer, dtype)
    _pin(ff.inter_edge, model._inter_edge_normalizer, dtype)
    _pin(ff.hyper_node, model._hyper_node_normalizer, dtype)
    w = world.detach().clone().to(dtype).requires_grad_(True)
    nf = nodes.detach().clone().to(dtype).requires_grad_(True)
    g = {'node_features': [nf], 'target_feature': w, 'mesh_features': base['mesh'].to(dtype),
         'edge_sets': [O.EdgeSet(n, f.to(dtype), s, r) for n, f, s, r in base['sets']]}
    args = (g, case['clusters'], case['nb'], ff.intra_edge, ff.inter_edge, ff.hyper_node, False, case['hnf'])
    mg = FO.multigraph_connect(*args) if case['multi'] else FO.hierarchical_connect(*args)
    outs = _outputs(mg)
    assert [tuple(t.shape) for t in outs] == [tuple(t.shape) for t in weights]
    sum((t * c.to(dtype)).sum() for t, c in zip(outs, weights)).backward()
    return w.grad, nf.grad


def _base(graph):
    """What the connector hands through or reads as constants, on the CPU."""
    return {'mesh': graph.mesh_features.detach().cpu(),
            'sets': [(e.name, e.features.detach().cpu(), e.senders.cpu(), e.receivers.cpu()) for e in graph.edge_sets]}


def _leaf_graph(graph):
    w = graph.target_feature.detach().clone().requires_grad_(True)
    nf = graph.node_features[0].detach().clone().requires_grad_(True)
    return graph._replace(target_feature=w, node_features=[nf]), w, nf


def _check_against_oracle(tid, got, g64, g32):
    for name, a, exact, ref32 in zip(('d target_feature', 'd node_features'), got, g64, g32):
        assert a is not None and bool(torch.isfinite(a).all()) and float(exact.abs().max()) > 0, name
        rec = H.report(tid, name, a, exact, ref32)
        assert rec['norm'] <= FACTOR * rec['ref_fp32_norm'], (name, rec)


CONNECTOR_CASES = ['flag5x4_k3', 'flag5x4_k3_plain', 'flag8x6_k2', 'flag8x6_k5', 'plate_obstacle_first', 'plate_obstacle_last',
                   'plate_multi']


@pytest.mark.parametrize('name', CONNECTOR_CASES)
def test_connector_gradient_vs_fp64_oracle(name):
    """4. Random weights on every tensor of the expanded graph; gradients with respect to target_feature and the node features."""
    case = _connector_case(name)
    model, frame = case['model'], case['frames'][0]
    with torch.no_grad():
        graph = model.build_graph(FG._cuda(frame), False)
    leafy, w, nf = _leaf_graph(graph)
    mg = model.expand_graph(leafy, 1, 10 ** 9, False)
    outs = _outputs(mg)
    weights = _weights(outs, 5)
    sum((t * c.cuda()).sum() for t, c in zip(outs, weights)).backward()
    base = _base(graph)
    g64 = _oracle_connect(case, base, w.cpu(), nf.cpu(), weights, torch.float64)
    g32 = _oracle_connect(case, base, w.cpu(), nf.cpu(), weights, torch.float32)
    _check_against_oracle(f'test_connector_gradient_vs_fp64_oracle[{name}]', (w.grad, nf.grad), g64, g32)
    if case['kind'] == 'plate':                                            # obstacle rows belong to no cluster and feed no remote edge
        obstacle = torch.nonzero(frame['node_type'][:, 0] == 1).flatten()
        assert float(g64[0][obstacle].abs().max()) == 0 and float(w.grad.cpu()[obstacle].abs().max()) == 0


def test_batched_connector_gradient_is_the_sum_of_the_per_frame_gradients():
    """4, n_graphs = 3: the union graph has the bits of batch_graphs over the per-frame expansions (as in test_gpu_batch_build.py);
    its gradient and the sum of the three per-frame gradients (one leaf, sliced per frame) are both held against the fp64 oracle."""
    from hgn_amd import batching
    case = _connector_case('flag5x4_k3_batch3')
    model, frames = case['model'], case['frames']
    B, N = len(frames), frames[0]['node_type'].shape[0]
    stacked = {k: (frames[0][k] if k == 'cells' else torch.stack([f[k] for f in frames])).cuda() for k in frames[0]}
    stacked['mesh_pos'] = frames[0]['mesh_pos'].cuda()
    with torch.no_grad():
        union = model.build_graph_batch(stacked, False)
        singles = [model.build_graph(FG._cuda(f), False) for f in frames]
    leafy, w, nf = _leaf_graph(union)
    got = model.expand_graph_batch(leafy, B, 1, 10 ** 9, False)
    # per frame, on slices of one leaf pair
    w2, nf2 = w.detach().clone().requires_grad_(True), nf.detach().clone().requires_grad_(True)
    per = [model.expand_graph(g._replace(target_feature=w2[b * N:(b + 1) * N], node_features=[nf2[b * N:(b + 1) * N]]), 1, 10 ** 9, False)
           for b, g in enumerate(singles)]
    ref = batching.batch_graphs(per)
    assert [e.name for e in got.edge_sets] == [e.name for e in ref.edge_sets]
    for e, f in zip(got.edge_sets, ref.edge_sets):
        assert torch.equal(e.senders, f.senders) and torch.equal(e.receivers, f.receivers) and torch.equal(e.features, f.features), e.name
    for x, y in zip(got.node_features, ref.node_features):
        assert torch.equal(x, y)
    per_weights = [_weights(_outputs(g), 30 + b) for b, g in enumerate(per)]
    union_weights = [torch.cat([pw[k] for pw in per_weights]) for k in range(len(per_weights[0]))]
    sum((t * c.cuda()).sum() for t, c in zip(_outputs(got), union_weights)).backward()
    sum((t * c.cuda()).sum() for t, c in zip(_outputs(ref), union_weights)).backward()
    g64, g32 = [], []
    for b, g in enumerate(singles):
        rows = slice(b * N, (b + 1) * N)
        for store, dtype in ((g64, torch.float64), (g32, torch.float32)):
            store.append(_oracle_connect(case, _base(g), w[rows].detach().cpu(), nf[rows].detach().cpu(), per_weights[b], dtype))
    cat = lambda parts: tuple(torch.cat([p[i] for p in parts]) for i in range(2))
    tid = 'test_batched_connector_gradient_is_the_sum_of_the_per_frame_gradients'
    _check_against_oracle(tid + '[union]', (w.grad, nf.grad), cat(g64), cat(g32))
    _check_against_oracle(tid + '[per frame]', (w2.grad, nf2.grad), cat(g64), cat(g32))


# ---------------------------------------------------------------------------------------------------------------
# 5. the plate graph against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
def _plate_model():
    from hgn_amd import system_model
    torch.manual_seed(5)
    model = system_model.PlateModel(FG._params('sum', steps=2))
    frame = FG._cuda(synth.plate_frame(seed=1))
    with torch.no_grad():
        g = model.build_graph(frame, True)
        model.get_target(frame, True)
        model.learned_model(model.expand_graph(g, 0, 10 ** 9, True))
    model.position_gradients = True
    return model


def _plate_oracle(model, dtype):
    ff = FO.PlateFeatures(dtype=dtype)
    for o, h in ((ff.output, model._output_normalizer), (ff.node, model._node_normalizer), (ff.mesh_edge, model._mesh_edge_normalizer),
                 (ff.world_edge, model._world_edge_normalizer)):
        _pin(o, h, dtype)
    return ff


def _assert_world_edges_are_clear(frame, hip_edges, oracle_edges, n_min=4):
    """The three preconditions of the plate comparisons, for one frame: enough world edges, the same pairs on both sides, and no
    pair that the radius decides about (obstacle -> normal, not a mesh edge) has an fp64 distance within GAP relative of it."""
    hip = set(zip(hip_edges.senders.cpu().tolist(), hip_edges.receivers.cpu().tolist()))
    ora = set(zip(oracle_edges.senders.tolist(), oracle_edges.receivers.tolist()))
    assert len(ora) >= n_min and hip == ora
    world = frame['world_pos'].detach().double().cpu()
    kind = frame['node_type'][:, 0].cpu()
    dist = torch.sqrt((world[:, None, :] - world[None, :, :]).pow(2).sum(-1))
    decided = (kind == 1).unsqueeze(1) & (kind == 0).unsqueeze(0)
    s, r = FO.triangles_to_edges(frame['cells'].cpu(), deform=True)
    decided[s, r] = False
    radius = FO.PlateFeatures.RADIUS
    assert not bool((((dist - radius).abs() <= GAP * radius) & decided).any()), 'a pair sits on the radius: choose other inputs'


def _plate_outputs(g):
    nodes = g['node_features'] if isinstance(g, dict) else g.node_features
    sets = g['edge_sets'] if isinstance(g, dict) else g.edge_sets
    return list(nodes) + [e.features for e in sets]


def test_plate_graph_gradient_vs_fp64_oracle():
    """5. build_graph on one frame and build_graph_batch on two: d / d world_pos and d / d target|world_pos of randomly weighted
    node, mesh-edge and world-edge features."""
    model = _plate_model()
    frames = [synth.plate_frame(seed=11), synth.plate_frame(seed=12)]
    names = ('world_pos', 'target|world_pos')
    tid = 'test_plate_graph_gradient_vs_fp64_oracle'
    per_weights, g64, g32, union_grads = [], [], [], None
    for b, frame in enumerate(frames):
        fr = FG._leaves(FG._cuda(frame), names, dict(device='cuda', dtype=torch.float32))
        graph = model.build_graph(fr, False)
        assert not graph.unnormalized_edges.features.requires_grad
        outs = _plate_outputs(graph)
        weights = _weights(outs, 60 + b)
        per_weights.append(weights)
        sum((t * c.cuda()).sum() for t, c in zip(outs, weights)).backward()
        for store, dtype in ((g64, torch.float64), (g32, torch.float32)):
            fo = FG._leaves(frame, names, dict(dtype=dtype))
            og = _plate_oracle(model, dtype).build_graph(fo, False)
            if dtype == torch.float64:
                _assert_world_edges_are_clear(frame, graph.edge_sets[1], og['edge_sets'][1])
            oo = _plate_outputs(og)
            assert [tuple(t.shape) for t in oo] == [tuple(t.shape) for t in weights]
            sum((t * c.to(dtype)).sum() for t, c in zip(oo, weights)).backward()
            store.append(tuple(fo[n].grad for n in names))
        for i, n in enumerate(names):
            rec = H.report(f'{tid}[frame {b}]', f'd {n}', fr[n].grad, g64[b][i], g32[b][i])
            assert float(g64[b][i].abs().max()) > 0 and rec['norm'] <= FACTOR * rec['ref_fp32_norm'], (n, rec)
    # the batch of two: the union's tensors are the per-frame ones behind one another (test_gpu_batch_build.py), so are the weights
    stacked = {k: (frames[0][k] if k in ('cells', 'mesh_pos') else torch.stack([f[k] for f in frames])).cuda() for k in frames[0]}
    st = FG._leaves(stacked, names, dict(device='cuda', dtype=torch.float32))
    union = model.build_graph_batch(st, False)
    outs = _plate_outputs(union)
    weights = [torch.cat([pw[k] for pw in per_weights]) for k in range(len(outs))]
    sum((t * c.cuda()).sum() for t, c in zip(outs, weights)).backward()
    for i, n in enumerate(names):
        exact, ref32 = torch.stack([g[i] for g in g64]), torch.stack([g[i] for g in g32])
        rec = H.report(f'{tid}[batch of 2]', f'd {n}', st[n].grad, exact, ref32)
        assert rec['norm'] <= FACTOR * rec['ref_fp32_norm'], (n, rec)


# ---------------------------------------------------------------------------------------------------------------
# 6. the forward is unchanged
# ---------------------------------------------------------------------------------------------------------------
def _same_graph(a, b):
    assert [e.name for e in a.edge_sets] == [e.name for e in b.edge_sets] and len(a.node_features) == len(b.node_features)
    for e, f in zip(a.edge_sets, b.edge_sets):
        assert torch.equal(e.senders, f.senders) and torch.equal(e.receivers, f.receivers), e.name
        assert torch.equal(e.features.detach(), f.features.detach()), e.name
    for x, y in zip(a.node_features, b.node_features):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize('kind,connector', [('plate', 'none'), ('plate', 'hetero'), ('flag', 'hyper'), ('flag', 'multi')],
                         ids=['plate', 'plate-hetero', 'flag-hyper', 'flag-multi'])
def test_with_the_switch_on_the_forward_has_the_bits_of_the_call_without_gradients(kind, connector):
    """6. build_graph / expand_graph and their batched forms: leaves that require grad against the same call under torch.no_grad().
    With a connector the clusters come from the model's own clustering (k-means; for the plate through remove_obstacles), run at
    step 0 on a graph that carries gradients."""
    from hgn_amd import system_model
    torch.manual_seed(9)
    cls = system_model.PlateModel if kind == 'plate' else system_model.FlagModel
    model = cls(_params(connector, 3))
    make = (lambda s: synth.plate_frame(seed=s)) if kind == 'plate' else (lambda s: synth.flag_frame(seed=s, nx=5, ny=4))
    frames = [make(31), make(32)]
    names = ('world_pos', 'target|world_pos') if kind == 'plate' else ('world_pos', 'prev|world_pos')
    with torch.no_grad():
        model.expand_graph(model.build_graph(FG._cuda(frames[0]), True), 1, 10 ** 9, True)      # statistics
    model.position_gradients = True
    rmp = model._remote_graph if connector != 'none' else None

    def single(fr, step):
        return model.expand_graph(model.build_graph(fr, False), step, 10 ** 9, False)

    def union(st, step):
        return model.expand_graph_batch(model.build_graph_batch(st, False), 2, step, 10 ** 9, False)
    stacked = {k: (frames[0][k] if k in ('cells', 'mesh_pos') else torch.stack([f[k] for f in frames])).cuda() for k in frames[0]}
    for route, inputs in ((single, FG._cuda(frames[0])), (union, stacked)):
        if rmp is not None:
            rmp.reset_clusters()
        leaves = FG._leaves(inputs, names, dict(device='cuda', dtype=torch.float32))
        with_grad = route(leaves, 0)                                        # step 0 clusters, from tensors that require grad
        assert any(t.requires_grad for t in _outputs(with_grad))
        with torch.no_grad():
            plain = route(leaves, 1)
        assert not any(t.requires_grad for t in _outputs(plain))
        _same_graph(with_grad, plain)
        if rmp is not None:
            assert sum(len(c) for c in rmp._clusters) == (126 if kind == 'plate' else 20)


def test_with_the_switch_on_a_balancer_still_refuses():
    from hgn_amd import _lib, system_model
    params = _params('hyper', 3)
    params['graph_balancer'] = {'algorithm': 'random', 'frequency': 1, 'remove_edges': False, 'random': {'edge_amount': 4}}
    model = system_model.FlagModel(params)
    model.position_gradients = True
    frame = synth.flag_frame(seed=5, nx=5, ny=4)
    fr = FG._leaves(FG._cuda(frame), ('world_pos',), dict(device='cuda', dtype=torch.float32))
    with pytest.raises(_lib.HgnError, match='not differentiable'):
        model.expand_graph(model.build_graph(fr, False), 0, 10, False)
    with pytest.raises(_lib.HgnError, match='expand_graph_batch.*balancer'):
        model.unrolled_training_step(UT._windows('flag', 2, 2), 2, through_state=True, is_training=False)


# ---------------------------------------------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------------------------------------------
def _two(first, second):
    return torch.stack([first, second]).unsqueeze(0)


def test_two_step_unroll_of_a_hyper_model_vs_fp64_oracle():
    """7. Flag + `hyper`, W = 1, two steps through the state: loss, per-step losses, d / d world_pos, d / d prev|world_pos and two
    weight gradients against the fp64 oracle unroll with the HIP forward's ReLU gates."""
    from hgn_amd import system_model
    torch.manual_seed(2)
    frame = synth.flag_frame(seed=5, nx=5, ny=4)
    model = system_model.FlagModel(FG._params('sum', steps=2, connector='hyper'))
    with torch.no_grad():
        g = model.build_graph(FG._cuda(frame), True)
        model.get_target(FG._cuda(frame), True)
        model.learned_model(model.expand_graph(g, 0, 10 ** 9, True))
    model.position_gradients = True
    target2 = synth.flag_frame(seed=9, nx=5, ny=4)['target|world_pos']
    leaves = {n: frame[n].cuda().clone().requires_grad_(True) for n in FG.STATE['flag']}
    win = {'world_pos': _two(leaves['world_pos'], leaves['world_pos'].detach()),
           'prev|world_pos': _two(leaves['prev|world_pos'], leaves['prev|world_pos'].detach()),
           'target|world_pos': _two(frame['target|world_pos'], target2).cuda(),
           'node_type': _two(frame['node_type'], frame['node_type']).cuda(), 'cells': frame['cells'].cuda(), 'mesh_pos': frame['mesh_pos'].cuda()}
    (loss, per), gates, winners = FG._logged(model, lambda: model.unrolled_training_step(win, 2, through_state=True, is_training=False))
    loss.backward()

    rmp = model._remote_graph
    clusters, nb = rmp._clusters, [tuple(t.tolist()) for t in rmp._neighbors]
    ff = FG._oracle_features('flag', model)
    for o, h in ((ff.intra_edge, model._intra_edge_normalizer), (ff.inter_edge, model._inter_edge_normalizer),
                 (ff.hyper_node, model._hyper_node_normalizer)):
        FG._pin(o, h)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = FG._leaves(frame, FG.STATE['flag'], dict(dtype=torch.float64))
    free = (frame['node_type'][:, 0] == 0).unsqueeze(1)

    def mse(target, out):
        m = free.to(out.dtype)
        return (((out - target) ** 2) * m).sum() / (m.sum() * out.shape[1])

    def step(fr):
        mg = FO.hierarchical_connect(ff.build_graph(fr, False), clusters, nb, ff.intra_edge, ff.inter_edge, ff.hyper_node, False)
        out = O.mesh_graph_net(sd, mg, 'hyper', 'sum')
        return out, mse(ff.get_target(fr, False), out)
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners):
        out1, l1 = step(fo)
        nxt = torch.where(free, ff.update(fo, out1), fo['world_pos'])
        _, l2 = step({**fo, 'world_pos': nxt, 'prev|world_pos': fo['world_pos'], 'target|world_pos': target2.double()})
        loss64 = (l1 + l2) / 2
    assert all(len(v) == 0 for v in gt.gates.values()), 'decisions left over'
    loss64.backward()
    tid = 'test_two_step_unroll_of_a_hyper_model_vs_fp64_oracle'
    assert H.report(tid, 'loss', loss, loss64)['norm'] <= TOL_GRAD
    assert H.report(tid, 'per-step losses', per, torch.stack([l1, l2]))['norm'] <= TOL_GRAD
    for n in FG.STATE['flag']:
        assert leaves[n].grad is not None, n
        assert H.report(tid, f'd loss / d {n}', leaves[n].grad, fo[n].grad)['norm'] <= TOL_GRAD, n
    named = dict(model.learned_model.named_parameters())
    for k in FG._two_params(sd):
        assert H.report(tid, f'd loss / d {k}', named[k].grad, sd[k].grad)['norm'] <= TOL_GRAD, k


def test_two_step_unroll_of_the_plate_model_vs_fp64_oracle(monkeypatch):
    """7. Plate, W = 1, two steps through the state; the world edges of both steps are checked to be the oracle's."""
    from hgn_amd import features
    model = _plate_model()
    frame = synth.plate_frame(seed=11)
    target2 = synth.plate_frame(seed=12)['target|world_pos']
    leaf = frame['world_pos'].cuda().clone().requires_grad_(True)
    win = {'world_pos': _two(leaf, leaf.detach()), 'target|world_pos': _two(frame['target|world_pos'], target2).cuda(),
           'node_type': _two(frame['node_type'], frame['node_type']).cuda(), 'cells': frame['cells'].cuda(), 'mesh_pos': frame['mesh_pos'].cuda()}
    real, queries = features.radius_edges_batch, []

    def spy(pos, *args, **kw):
        assert not pos.requires_grad                                        # the query reads values
        res = real(pos, *args, **kw)
        queries.append((pos.detach().cpu(), O.EdgeSet('world_edges', None, res[0].cpu(), res[1].cpu())))
        return res
    monkeypatch.setattr(features, 'radius_edges_batch', spy)
    (loss, per), gates, winners = FG._logged(model, lambda: model.unrolled_training_step(win, 2, through_state=True, is_training=False))
    monkeypatch.setattr(features, 'radius_edges_batch', real)
    loss.backward()
    assert len(queries) == 2

    ff = _plate_oracle(model, torch.float64)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = FG._leaves(frame, ('world_pos',), dict(dtype=torch.float64))
    free = (frame['node_type'][:, 0] == 0).unsqueeze(1)
    seen = []

    def mse(target, out):
        m = free.to(out.dtype)
        return (((out - target) ** 2) * m).sum() / (m.sum() * out.shape[1])

    def step(fr):
        g = ff.build_graph(fr, False)
        seen.append((fr, g['edge_sets'][1]))
        out = O.mesh_graph_net(sd, FO._as_multigraph(g), 'none', 'sum')
        return out, mse(ff.get_target(fr, False), out)
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners):
        out1, l1 = step(fo)
        nxt = torch.where(free, ff.update(fo, out1), fo['target|world_pos'].double())
        _, l2 = step({**fo, 'world_pos': nxt, 'target|world_pos': target2.double()})
        loss64 = (l1 + l2) / 2
    assert all(len(v) == 0 for v in gt.gates.values()), 'decisions left over'
    for (fr, oracle_edges), (_, hip_edges) in zip(seen, queries):
        _assert_world_edges_are_clear(fr, hip_edges, oracle_edges)
    loss64.backward()
    tid = 'test_two_step_unroll_of_the_plate_model_vs_fp64_oracle'
    assert H.report(tid, 'loss', loss, loss64)['norm'] <= TOL_GRAD
    assert H.report(tid, 'per-step losses', per, torch.stack([l1, l2]))['norm'] <= TOL_GRAD
    assert leaf.grad is not None
    assert H.report(tid, 'd loss / d world_pos', leaf.grad, fo['world_pos'].grad)['norm'] <= TOL_GRAD
    named = dict(model.learned_model.named_parameters())
    for k in FG._two_params(sd):
        assert H.report(tid, f'd loss / d {k}', named[k].grad, sd[k].grad)['norm'] <= TOL_GRAD, k


@pytest.mark.parametrize('kind,connector', [('flag', 'hyper'), ('plate', 'none')], ids=['flag-hyper', 'plate'])
def test_lockstep_unroll_through_the_state_equals_the_loop_written_per_window(kind, connector):
    """7, W = 2: k-means reads `mesh_pos` alone, so the clusters the lock-step call makes at step 0 are those every window of the loop
    form uses.  Losses torch.equal, gradients within 1e-5; and the later step does reach the initial state."""
    model = UT._model(kind, connector)
    model.position_gradients = True
    win = UT._windows(kind, 2, 2)
    wa, la = UT._with_leaves(win, kind)
    loss_a, per_a = model.unrolled_training_step(wa, 2, through_state=True, is_training=False)
    loss_a.backward()
    ga = UT._two_grads(model)
    model.zero_grad(set_to_none=True)
    _, lb = UT._with_leaves(win, kind)
    loss_b, per_b, _ = UT._loop_form(model, kind, win, 2, lb)
    loss_b.backward()
    gb = UT._two_grads(model)
    model.zero_grad(set_to_none=True)
    assert torch.equal(loss_a, loss_b) and torch.equal(per_a, per_b)
    for n in la:
        assert la[n].grad is not None and float(la[n].grad.abs().max()) > 0, n
        err = H.rel_err(la[n].grad, lb[n].grad)
        print(f'unroll[{kind}-{connector}] d loss / d {n}: lock step vs loop rel_err={err:.3e}')
        assert err <= TOL_GRAD, n
    for n in ga:
        err = H.rel_err(ga[n], gb[n])
        print(f'unroll[{kind}-{connector}] d loss / d {n}: lock step vs loop rel_err={err:.3e}')
        assert float(gb[n].abs().max()) > 0 and err <= TOL_GRAD, n
    # push-forward shows the initial state step 0 alone: what through_state adds is the second step's loss, and it is not zero
    wc, lc = UT._with_leaves(win, kind)
    model.unrolled_training_step(wc, 2, through_state=False, is_training=False)[0].backward()
    state = UT.STATE[kind]
    later = la[state].grad - lc[state].grad
    assert float(later.abs().max()) > 1e-3 * float(lc[state].grad.abs().max())


# ---------------------------------------------------------------------------------------------------------------
# 8. frozen network
# ---------------------------------------------------------------------------------------------------------------
def test_unrolled_step_through_the_state_of_a_frozen_hyper_model():
    """8. Flag + `hyper`, W = 2, two steps: the loss torch.equal to the trainable run, the state gradients within 2e-6."""
    win = UT._windows('flag', 2, 2)
    out = {}
    for frozen in (False, True):
        model = UT._model('flag', 'hyper')
        model.position_gradients = True
        model.learned_model.requires_grad_(not frozen)
        wa, la = UT._with_leaves(win, 'flag')
        loss, _ = model.unrolled_training_step(wa, 2, through_state=True, is_training=False)
        loss.backward()
        out[frozen] = (loss.detach(), {n: t.grad for n, t in la.items()})
        assert all(p.grad is None for p in model.learned_model.parameters()) == frozen
    assert torch.equal(out[True][0], out[False][0])
    for n in out[True][1]:
        assert float(out[True][1][n].abs().max()) > 0 and H.rel_err(out[True][1][n], out[False][1][n]) <= FZ.TOL_SUM, n
