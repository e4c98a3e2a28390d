"""Position gradients of the frame -> graph step on the GPU: the backward kernels of include/hgn_features.h behind the autograd
wrappers of hgn_amd/features.py, and FlagModel / CylinderModel differentiated from the loss back to the input frame.

Yardstick: torch autograd through oracle/features_oracle.py and oracle/mgn_oracle.py in fp64 on the CPU.

Bounds.
* rel_edge_features backward: not a fixed number.  The oracle's own fp32 autograd is run on the same inputs; the HIP result may
  be at most 4x as far from fp64 (helpers.rel_err) as that: the per-node summation order differs from index_add's edge order, and
  the 70-term sums of the star case lose about two bits more than a 12-term sum.
* node_features and normalize backward are one multiply (or a copy) per element: 2 ulp of the fp64 result rounded to fp32.  The
  normaliser statistics of that test are dyadic numbers, so that mean, E[x^2] - mean^2 and (for most columns) its root are exact in
  fp32 and in fp64 alike: what is measured is the backward multiply / divide, not the cancellation of the fp32 variance formula.
* end to end and the two-step unroll: the project's 1e-5 (helpers.rel_err) for gradients with the HIP forward's discrete decisions
  (ReLU gates, max / min winners) transferred to the oracle, as in test_gpu_parity.py.

Statistics are constants.  The reference's Normalizer would let a gradient flow into the running sums when it accumulates from
a tensor that requires grad; hgn_amd accumulates from detached values.  The end-to-end cases therefore accumulate first (no grad)
and differentiate with ``is_training=False`` on both sides, and the oracle's normalisers are given the very mean / std tensors the
HIP normalisers hold, so that both sides differentiate the same function.

Zero-length edge.  The oracle writes the length as sqrt(sum(u^2)), whose autograd value at u = 0 is NaN (0 * inf); the kernel
takes the subgradient 0 there (what torch.linalg.vector_norm does).  For that one case the yardstick is the oracle's expression
with vector_norm in place of sqrt(sum(.^2)) -- checked, on a graph without such an edge, to have the oracle's fp64 gradient.
"""
import pytest
import torch

from oracle import features_oracle as FO
from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-5          # transferred gradients (test_gpu_parity.py)
FACTOR = 4.0             # HIP error allowed over the oracle's own fp32 error, rel_edge_features backward


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import hgn_amd  # noqa: F401
    from hgn_amd import _lib
    _lib.lib()
    yield


# ---------------------------------------------------------------------------------------------------------------
# operator gradients: rel_edge_features
# ---------------------------------------------------------------------------------------------------------------
def _two_way(pairs):
    s = torch.tensor([p[0] for p in pairs], dtype=torch.int64)
    r = torch.tensor([p[1] for p in pairs], dtype=torch.int64)
    return torch.cat([s, r]), torch.cat([r, s])


def _graph(kind):
    """-> (N, senders, receivers, {node: node whose position it duplicates})."""
    if kind == 'two_triangles':                       # 4 nodes, 5 undirected = 10 directed edges
        s, r = _two_way([(1, 0), (2, 0), (2, 1), (3, 1), (3, 2)])
        return 4, s, r, {}
    if kind == 'grid5x4':
        s, r = synth.two_way_edges(synth.grid_triangles(5, 4))
        return 20, s, r, {}
    if kind == 'star70':                              # 67 nodes; node 0 has 70 outgoing and 70 incoming edges (4 of them doubled)
        s, r = _two_way([(0, j) for j in range(1, 67)] + [(0, j) for j in (3, 17, 40, 66)] + [(5, 6), (7, 9)])
        return 67, s, r, {}
    if kind == 'isolated':                            # node 20 has no edge
        s, r = synth.two_way_edges(synth.grid_triangles(5, 4))
        return 21, s, r, {}
    if kind == 'zero_length':                         # node 3 sits on node 1: edge (3, 1) has length 0
        s, r = _two_way([(1, 0), (2, 0), (2, 1), (3, 1), (3, 2)])
        return 4, s, r, {3: 1}
    if kind == 'no_edges':
        e = torch.zeros(0, dtype=torch.int64)
        return 3, e, e.clone(), {}
    raise KeyError(kind)


GRAPHS = ['two_triangles', 'grid5x4', 'star70', 'isolated', 'zero_length', 'no_edges']
WIDTHS = [(3, 2), (2, 0)]
MODES = ['feat_and_len', 'feat_only', 'len_only', 'len_unused']     # which of d_feat / d_len reach the kernel
_CASES = {}


def _case(kind, da, db, mode):
    """Inputs (fp32, CPU), the fp64 gradient and the oracle's own fp32 gradient -- computed once per case."""
    key = (kind, da, db, mode)
    if key in _CASES:
        return _CASES[key]
    N, s, r, dup = _graph(kind)
    gen = torch.Generator().manual_seed(11 + 7 * GRAPHS.index(kind) + da)
    a = torch.randn(N, da, generator=gen)
    b = torch.randn(N, db, generator=gen) if db else None
    for k, v in dup.items():
        a[k] = a[v]
        if b is not None:
            b[k] = b[v]
    E = s.shape[0]
    W = da + 1 + (db + 1 if db else 0)
    cf = torch.randn(E, W, generator=gen)
    cl = torch.randn(E, generator=gen)

    def rel(world, mesh):
        if not dup:
            return FO.rel_features(world, mesh, s, r)
        rw = world[s] - world[r]                     # FO.rel_features with the norm's subgradient 0 at 0 (module docstring)
        cols = [rw, torch.linalg.vector_norm(rw, dim=-1, keepdim=True)]
        if mesh is not None:
            rm = mesh[s] - mesh[r]
            cols += [rm, torch.linalg.vector_norm(rm, dim=-1, keepdim=True)]
        return torch.cat(cols, -1)

    def oracle(dtype):
        aa = a.detach().clone().to(dtype).requires_grad_(True)
        bb = b.detach().clone().to(dtype).requires_grad_(True) if b is not None else None
        feat = rel(aa, bb)
        loss = feat.sum() * 0
        if mode in ('feat_and_len', 'feat_only', 'len_unused'):
            loss = loss + (feat * cf.to(dtype)).sum()
        if mode in ('feat_and_len', 'len_only'):
            loss = loss + (feat[:, da] * cl.to(dtype)).sum()
        loss.backward()
        return aa.grad, (bb.grad if bb is not None else None)
    _CASES[key] = dict(N=N, s=s, r=r, a=a, b=b, cf=cf, cl=cl, dup=dup, g64=oracle(torch.float64), g32=oracle(torch.float32))
    return _CASES[key]


def _hip_rel_grads(c, da, mode):
    from hgn_amd import features
    a = c['a'].cuda().requires_grad_(True)
    b = c['b'].cuda().requires_grad_(True) if c['b'] is not None else None
    s, r = c['s'].cuda(), c['r'].cuda()
    feat, ln = features.rel_edge_features(a, b, s, r, want_feat=True, want_len=mode != 'feat_only')
    assert (ln is None) == (mode == 'feat_only')
    loss = 0
    if mode in ('feat_and_len', 'feat_only', 'len_unused'):
        loss = loss + (feat * c['cf'].cuda()).sum()
    if mode in ('feat_and_len', 'len_only'):
        loss = loss + (ln * c['cl'].cuda()).sum()
    loss.backward()
    return a.grad, (b.grad if b is not None else None), (feat, ln)


def test_the_norm_form_of_the_zero_length_yardstick_has_the_oracles_gradient():
    """(CPU arithmetic only.)  Where no edge has length 0, the vector_norm form used for the zero-length case and the oracle's
    sqrt(sum(u^2)) have the same fp64 gradient."""
    N, s, r, _ = _graph('two_triangles')
    gen = torch.Generator().manual_seed(3)
    a0, b0, cf = torch.randn(N, 3, generator=gen).double(), torch.randn(N, 2, generator=gen).double(), torch.randn(s.shape[0], 7, generator=gen).double()
    grads = []
    for norm_form in (False, True):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        if norm_form:
            rw, rm = a[s] - a[r], b[s] - b[r]
            feat = torch.cat([rw, torch.linalg.vector_norm(rw, dim=-1, keepdim=True), rm, torch.linalg.vector_norm(rm, dim=-1, keepdim=True)], -1)
        else:
            feat = FO.rel_features(a, b, s, r)
        (feat * cf).sum().backward()
        grads.append((a.grad, b.grad))
    assert H.rel_err(grads[1][0], grads[0][0]) <= 1e-14 and H.rel_err(grads[1][1], grads[0][1]) <= 1e-14


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('da,db', WIDTHS, ids=['a3b2', 'a2'])
@pytest.mark.parametrize('kind', GRAPHS)
def test_rel_edge_features_backward_vs_fp64_oracle(kind, da, db, mode):
    """d_a and d_b of every graph / width / arriving-gradient combination: at most FACTOR x the oracle's own fp32 error; finite at a
    zero-length edge; exactly zero on a node without edges and for E = 0."""
    c = _case(kind, da, db, mode)
    ga, gb, (feat, ln) = _hip_rel_grads(c, da, mode)
    tid = f'test_rel_edge_features_backward_vs_fp64_oracle[{kind}-a{da}b{db}-{mode}]'
    for name, got, exact, ref32 in (('d_a', ga, c['g64'][0], c['g32'][0]), ('d_b', gb, c['g64'][1], c['g32'][1])):
        if exact is None:
            assert got is None
            continue
        assert got is not None and got.shape == exact.shape and got.dtype == torch.float32
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(exact).all()), name
        rec = H.report(tid, name, got, exact, ref32)
        if float(exact.abs().max()) == 0:                       # no gradient arrives (d_b with only the length) or no edge
            assert float(got.abs().max()) == 0, name
            continue
        assert rec['norm'] <= FACTOR * rec['ref_fp32_norm'], (name, rec)
    if kind == 'isolated':
        assert float(ga[20].abs().max()) == 0 and (gb is None or float(gb[20].abs().max()) == 0)
    if kind == 'no_edges':
        assert feat.shape[0] == 0 and float(ga.abs().max()) == 0


def test_rel_edge_features_backward_kernel_with_either_gradient_absent_and_outputs_nullable():
    """The C entry called through features.rel_edge_features_bwd: d_feat alone, d_len alone, d_a alone and d_b alone each give the
    bits of the matching part of the full call."""
    from hgn_amd import features
    c = _case('star70', 3, 2, 'feat_and_len')
    a, b, s, r = c['a'].cuda(), c['b'].cuda(), c['s'].cuda(), c['r'].cuda()
    cf, cl = c['cf'].cuda(), c['cl'].cuda()
    da_full, db_full = features.rel_edge_features_bwd(cf, cl, a, b, s, r)
    da_only, none_b = features.rel_edge_features_bwd(cf, cl, a, b, s, r, want_b=False)
    none_a, db_only = features.rel_edge_features_bwd(cf, cl, a, b, s, r, want_a=False)
    assert none_a is None and none_b is None
    assert torch.equal(da_only, da_full) and torch.equal(db_only, db_full)
    da_f, db_f = features.rel_edge_features_bwd(cf, None, a, b, s, r)
    da_l, db_l = features.rel_edge_features_bwd(None, cl, a, b, s, r)
    assert torch.equal(db_f, db_full) and float(db_l.abs().max()) == 0          # the length carries nothing for b
    assert H.rel_err(da_f, _case('star70', 3, 2, 'len_unused')['g64'][0]) <= 1e-5
    assert H.rel_err(da_l, _case('star70', 3, 2, 'len_only')['g64'][0]) <= 1e-5
    z_a, z_b = features.rel_edge_features_bwd(None, None, a, b, s, r)
    assert float(z_a.abs().max()) == 0 and float(z_b.abs().max()) == 0


def test_rel_edge_features_backward_is_bit_identical_from_run_to_run():
    """The degree-70 node is summed by a wavefront, its neighbours by a thread each: no atomics, so two runs give the same bits."""
    c = _case('star70', 3, 2, 'feat_and_len')
    first = _hip_rel_grads(c, 3, 'feat_and_len')
    second = _hip_rel_grads(c, 3, 'feat_and_len')
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert float(first[0][0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------
# operator gradients: node_features, normalize, lincomb3
# ---------------------------------------------------------------------------------------------------------------
def _within_ulps(got, exact64, n):
    ref = exact64.float()
    ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float('inf'))) - ref.abs()
    return bool(((got.cpu().double() - exact64).abs() <= n * ulp.double()).all())


@pytest.mark.parametrize('with_prev', [True, False], ids=['prev', 'no_prev'])
@pytest.mark.parametrize('vel_mask_type', [-1, 1], ids=['unmasked', 'masked'])
@pytest.mark.parametrize('vel_first', [True, False], ids=['vel_first', 'onehot_first'])
def test_node_features_backward_vs_fp64(vel_first, vel_mask_type, with_prev):
    from hgn_amd import features
    N, d, n_classes = 23, 3, 3
    gen = torch.Generator().manual_seed(5)
    cur, prev = torch.randn(N, d, generator=gen), torch.randn(N, d, generator=gen)
    node_type = torch.randint(0, 3, (N, 1), generator=gen)
    w = torch.randn(N, d + n_classes, generator=gen)

    c64 = cur.double().requires_grad_(True)
    p64 = prev.double().requires_grad_(True) if with_prev else None
    v = c64 - p64 if with_prev else c64
    if vel_mask_type >= 0:
        v = v * (node_type == vel_mask_type).double()
    one_hot = torch.nn.functional.one_hot(node_type[:, 0], n_classes).double()
    out64 = torch.cat((v, one_hot) if vel_first else (one_hot, v), -1)
    (out64 * w.double()).sum().backward()

    cg = cur.cuda().requires_grad_(True)
    pg = prev.cuda().requires_grad_(True) if with_prev else None
    out = features.node_features(cg, pg, node_type.cuda(), None, n_classes, vel_first=vel_first, vel_mask_type=vel_mask_type)
    assert H.rel_err(out, out64) <= 1e-6
    (out * w.cuda()).sum().backward()
    assert _within_ulps(cg.grad, c64.grad, 2)
    if with_prev:
        assert _within_ulps(pg.grad, p64.grad, 2)
    if vel_mask_type >= 0:
        masked = (node_type[:, 0] != vel_mask_type)
        assert float(cg.grad.cpu()[masked].abs().max()) == 0


@pytest.mark.parametrize('inverse', [False, True], ids=['forward', 'inverse'])
@pytest.mark.parametrize('F', [1, 3, 12])
def test_normalize_backward_vs_fp64_oracle(F, inverse):
    """Dyadic statistics (module docstring): count 64, means k/8, standard deviations from {1/2, 2, 3, 5/4} -- and, for F >= 3, one
    column of zero variance that sits on the epsilon floor."""
    from hgn_amd import features
    gen = torch.Generator().manual_seed(F)
    count = 64.0
    mean = torch.tensor([(k % 5 - 2) / 8.0 for k in range(F)], dtype=torch.float64)
    std = torch.tensor([(0.5, 2.0, 3.0, 1.25)[k % 4] for k in range(F)], dtype=torch.float64)
    if F >= 3:
        std[2] = 0.0
    acc_sum, acc_sq = count * mean, count * (std * std + mean * mean)
    on = O.Normalizer(F, dtype=torch.float64)
    on.acc_sum, on.acc_sum_sq, on.acc_count = acc_sum, acc_sq, torch.tensor([count], dtype=torch.float64)
    x = torch.randn(37, F, generator=gen)
    w = torch.randn(37, F, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = on.inverse(x64) if inverse else on(x64, accumulate=False)
    (y64 * w.double()).sum().backward()

    xg = x.cuda().requires_grad_(True)
    stats = [t.float().cuda() for t in (acc_sum, acc_sq, on.acc_count)]
    before = [t.clone() for t in stats]
    y = features.normalize(xg, *stats, 1e-8, inverse=inverse)
    assert all(not t.requires_grad for t in stats)
    (y * w.cuda()).sum().backward()
    assert all(torch.equal(a, b) for a, b in zip(stats, before))
    assert _within_ulps(xg.grad, x64.grad, 2), H.rel_err(xg.grad, x64.grad)


def test_normalizer_accumulates_detached_values_and_backward_uses_the_statistics_of_its_forward():
    """Accumulating from a tensor that requires grad works, leaves the statistics without a graph, and a later accumulation (in
    place) does not change the gradient of an earlier call."""
    from hgn_amd.normalizer import Normalizer
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(50, 3, generator=gen).cuda().requires_grad_(True)
    nz = Normalizer(3, 'test')
    y = nz(x, True)
    std_then = nz._std_with_epsilon().clone()
    assert y.requires_grad and not nz._acc_sum.requires_grad and nz._host_num_acc == 1
    nz(10 * torch.randn(80, 3, generator=gen).cuda(), True)          # statistics move on
    assert not torch.equal(nz._std_with_epsilon(), std_then)
    y.sum().backward()
    assert H.rel_err(x.grad, (1.0 / std_then).expand(50, 3)) <= 2e-7


def test_lincomb3_backward_scales_the_three_inputs():
    from hgn_amd import features
    gen = torch.Generator().manual_seed(4)
    a, b, c = (torch.randn(9, 3, generator=gen).cuda().requires_grad_(True) for _ in range(3))
    w = torch.randn(9, 3, generator=gen).cuda()
    (features.lincomb3(a, 2.0, b, 1.0, c, -1.0) * w).sum().backward()
    assert torch.equal(a.grad, 2.0 * w) and torch.equal(b.grad, w) and torch.equal(c.grad, -w)


# ---------------------------------------------------------------------------------------------------------------
# system models
# ---------------------------------------------------------------------------------------------------------------
def _params(agg, steps=2, connector='none'):
    return {'size': 3, 'aggregation': agg, 'message_passing_steps': steps,
            'rmp': {'clustering': 'kmeans' if connector != 'none' else 'none', 'connector': connector, 'num_clusters': 3,
                    'hyper_noise': 'none', 'hyper_node_features': True, 'frequency': 1, 'fully_connect': False,
                    'intra_cluster_sampling': {'enabled': False, 'alpha': 0.1, 'spotter_threshold': 0}},
            'graph_balancer': {'algorithm': 'none', 'frequency': 1}}


def _cuda(frame):
    return {k: v.cuda() for k, v in frame.items()}


_MODELS = {}


def _system(kind, agg):
    """A model on a 5 x 4 mesh whose normalisers have seen the frame (without gradients) and whose lazy layers exist."""
    key = (kind, agg)
    if key not in _MODELS:
        from hgn_amd import system_model
        torch.manual_seed(1 + len(_MODELS))
        if kind == 'flag':
            frame, model = synth.flag_frame(seed=5, nx=5, ny=4), system_model.FlagModel(_params(agg))
        else:
            frame, model = synth.cylinder_frame(seed=6, nx=5, ny=4), system_model.CylinderModel(_params(agg))
        with torch.no_grad():
            g = model.build_graph(_cuda(frame), True)
            model.get_target(_cuda(frame), True)
            model.learned_model(g)
        _MODELS[key] = (frame, model)
    return _MODELS[key]


def _pin(oracle_norm, hip_norm):
    """The oracle normaliser with the HIP normaliser's mean / std (constants on both sides: module docstring)."""
    m, s = hip_norm._mean().double().cpu(), hip_norm._std_with_epsilon().double().cpu()
    oracle_norm.mean, oracle_norm.std = (lambda: m), (lambda: s)


def _oracle_features(kind, model):
    ff = (FO.FlagFeatures if kind == 'flag' else FO.CylinderFeatures)(dtype=torch.float64)
    _pin(ff.output, model._output_normalizer)
    _pin(ff.node, model._node_normalizer)
    _pin(ff.mesh_edge, model._mesh_edge_normalizer)
    if kind == 'flag':
        _pin(ff.node_dynamic, model._node_dynamic_normalizer)
    return ff


def _logged(model, fn):
    """fn() with the HIP forward's ReLU gates and max / min winners recorded: -> (result, gates, winners)."""
    from hgn_amd import ops
    ops._GATE_LOG, ops._ARG_LOG = [], []
    try:
        res = fn()
        gates, winners = H.hip_gates(model.learned_model, ops._GATE_LOG), H.hip_winners(model.learned_model, ops._ARG_LOG)
    finally:
        ops._GATE_LOG, ops._ARG_LOG = None, None
    return res, gates, winners


def _leaves(frame, names, dev_dtype):
    out = dict(frame)
    for n in names:
        out[n] = frame[n].to(**dev_dtype).detach().clone().requires_grad_(True)
    return out


STATE = {'flag': ('world_pos', 'prev|world_pos'), 'cylinder': ('velocity',)}
TARGET = {'flag': 'target|world_pos', 'cylinder': 'target|velocity'}


def _first(x):
    return x[0] if isinstance(x, tuple) else x


def _two_params(sd):
    ks = [k for k in sd if k.endswith('linear_0.weight')]
    return ks[0], [k for k in sd if k.endswith('.weight')][-1]


@pytest.mark.parametrize('agg', ['sum', 'pna'])
@pytest.mark.parametrize('kind', ['flag', 'cylinder'])
def test_loss_gradient_reaches_the_input_frame_vs_fp64_oracle(kind, agg):
    """loss = mse(update(frame, model(build_graph(frame))), target): d loss / d world_pos, d prev|world_pos (flag), d velocity
    (cylinder) and two parameter gradients against the fp64 oracle with the HIP forward's decisions."""
    frame, model = _system(kind, agg)
    model.zero_grad(set_to_none=True)
    fr = _leaves(_cuda(frame), STATE[kind], dict(device='cuda', dtype=torch.float32))

    def run():
        graph = model.build_graph(fr, False)
        assert graph.node_features[0].requires_grad
        assert not graph.unnormalized_edges.features.requires_grad
        assert kind != 'flag' or not graph.node_dynamic.requires_grad
        pred = _first(model.update(fr, model(graph)))
        return torch.nn.functional.mse_loss(pred, fr[TARGET[kind]])
    loss, gates, winners = _logged(model, run)
    loss.backward()
    for n in STATE[kind]:
        assert fr[n].grad is not None, f'no gradient reached {n}'

    ff = _oracle_features(kind, model)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = _leaves(frame, STATE[kind], dict(dtype=torch.float64))
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners) as wt:
        g = ff.build_graph(fo, False)
        pred = _first(ff.update(fo, O.mesh_graph_net(sd, FO._as_multigraph(g), 'none', agg)))
        loss64 = torch.nn.functional.mse_loss(pred, fo[TARGET[kind]].double())
    assert all(len(v) == 0 for v in gt.gates.values()) and all(len(v) == 0 for v in wt.winners.values()), 'decisions left over'
    loss64.backward()
    tid = f'test_loss_gradient_reaches_the_input_frame_vs_fp64_oracle[{kind}-{agg}]'
    assert H.rel_err(loss, loss64) <= TOL_GRAD
    for n in STATE[kind]:
        assert H.report(tid, f'd loss / d {n}', fr[n].grad, fo[n].grad)['norm'] <= TOL_GRAD, n
    named = dict(model.learned_model.named_parameters())
    for k in _two_params(sd):
        assert H.report(tid, f'd loss / d {k}', named[k].grad, sd[k].grad)['norm'] <= TOL_GRAD, k


def test_two_step_unroll_gradient_vs_fp64_oracle():
    """Flag: the first step's prediction becomes world_pos (and the old world_pos prev|world_pos) of a second build_graph; the loss is
    taken on the second prediction.  One backward pass runs twice through the one model."""
    frame, model = _system('flag', 'sum')
    model.zero_grad(set_to_none=True)

    def unroll(build, update, net, fr):
        p1 = update(fr, net(build(fr)))
        fr2 = {**fr, 'world_pos': p1, 'prev|world_pos': fr['world_pos']}
        p2 = update(fr2, net(build(fr2)))
        return torch.nn.functional.mse_loss(p2, fr['target|world_pos'].to(p2.dtype))
    fr = _leaves(_cuda(frame), STATE['flag'], dict(device='cuda', dtype=torch.float32))
    loss, gates, winners = _logged(model, lambda: unroll(lambda f: model.build_graph(f, False), model.update, model, fr))
    loss.backward()

    ff = _oracle_features('flag', model)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = _leaves(frame, STATE['flag'], dict(dtype=torch.float64))
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners):
        loss64 = unroll(lambda f: FO._as_multigraph(ff.build_graph(f, False)), ff.update,
                        lambda g: O.mesh_graph_net(sd, g, 'none', 'sum'), fo)
    assert all(len(v) == 0 for v in gt.gates.values()), 'decisions left over'
    loss64.backward()
    tid = 'test_two_step_unroll_gradient_vs_fp64_oracle'
    assert H.rel_err(loss, loss64) <= TOL_GRAD
    for n in STATE['flag']:
        assert fr[n].grad is not None, n
        assert H.report(tid, f'd loss / d {n}', fr[n].grad, fo[n].grad)['norm'] <= TOL_GRAD, n
    k = _two_params(sd)[0]
    assert H.report(tid, f'd loss / d {k}', dict(model.learned_model.named_parameters())[k].grad, sd[k].grad)['norm'] <= TOL_GRAD


def test_graph_without_gradients_is_bit_equal_and_the_rollout_still_captures():
    """build_graph of a frame that does not require grad gives the bits of the differentiable call, and -- after a backward pass
    through the model -- a rollout still captures its forward into a HIP graph at the second sight of the topology and replays the
    eager launches bit for bit (as in test_gpu_rollout.py)."""
    frame, model = _system('flag', 'sum')
    # the node_dynamic normaliser accumulates on EVERY build_graph call (flag.py:115 passes no `accumulate`): both calls start from
    # the same statistics
    nd = model._node_dynamic_normalizer
    names = ('_acc_sum', '_acc_sum_squared', '_acc_count', '_num_accumulations')
    kept = {n: getattr(nd, n).clone() for n in names}
    plain = model.build_graph(_cuda(frame), False)
    assert not plain.node_features[0].requires_grad and not plain.edge_sets[0].features.requires_grad
    for n in names:
        getattr(nd, n).copy_(kept[n])
    fr = _leaves(_cuda(frame), STATE['flag'], dict(device='cuda', dtype=torch.float32))
    diff = model.build_graph(fr, False)
    assert diff.node_features[0].requires_grad and diff.edge_sets[0].features.requires_grad
    for a, b in ((plain.node_features[0], diff.node_features[0]), (plain.edge_sets[0].features, diff.edge_sets[0].features),
                 (plain.node_dynamic, diff.node_dynamic), (plain.unnormalized_edges.features, diff.unnormalized_edges.features)):
        assert torch.equal(a, b.detach())
    model.update(fr, model(diff)).sum().backward()
    T = 4
    traj = {k: torch.stack([v] * T).cuda() for k, v in frame.items()}
    model._fwd_cache = None
    model.replay_rollout = True
    replayed, mse = model.rollout(traj, T)
    assert model._fwd_cache is not None and model._fwd_cache.captures == 1
    model.replay_rollout = False
    eager, eager_mse = model.rollout(traj, T)
    model.replay_rollout = True
    assert torch.equal(eager['pred_pos'], replayed['pred_pos']) and torch.equal(eager_mse, mse)


def test_plate_model_and_connector_stages_refuse_position_gradients():
    from hgn_amd import _lib, system_model
    plate = system_model.PlateModel(_params('sum', steps=1))
    pf = _cuda(synth.plate_frame(seed=1))
    plate.build_graph(pf, False)                                                # values: fine
    pf['world_pos'] = pf['world_pos'].clone().requires_grad_(True)
    with pytest.raises(_lib.HgnError, match='not differentiable'):
        plate.build_graph(pf, False)
    with torch.no_grad():
        plate.build_graph(pf, False)                                            # no graph is recorded: fine
    flag = system_model.FlagModel(_params('sum', steps=1, connector='hyper'))
    frame = synth.flag_frame(seed=5, nx=5, ny=4)
    fr = _leaves(_cuda(frame), ('world_pos',), dict(device='cuda', dtype=torch.float32))
    graph = flag.build_graph(fr, False)
    with pytest.raises(_lib.HgnError, match='not differentiable'):
        flag.expand_graph(graph, 0, 10, False)
    flag.expand_graph(flag.build_graph(_cuda(frame), False), 0, 10, False)      # values: fine
