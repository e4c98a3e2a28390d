"""The plain fp32-MFMA kernel path (hgn_mlp_fwd_t.flags: HGN_F_FP32_MFMA -- ops.Context(fp32_mfma=True), model.set_fp32_mfma(True)) at
the 128-wide shapes it exists for, against fp64: mlp_fwd_kernel with two gathered addends behind hgn_linear_fwd, mlp_bwd_kernel with the
aggregation backward folded into its d_out load, hgn_linear_bwd, wgrad_dma_kernel, and the route ops.EdgeBlockFn takes without packs.

The path is selected through the public host API only.  Every case is compared with an fp64 evaluation of the same operation (the
oracle's functions under torch autograd), within the bounds the default path is held to (TOL_OUT / TOL_GRAD of test_gpu_parity.py), and
every operator-level case also runs the default context on the same inputs: at least one tensor must differ bitwise -- other products
and another summation order cannot reproduce the split kernels' bits, so equality would mean the flag was ignored.

Measured on an MI355X, worst tensor over all cases, plain path / default path on the same inputs (norm-wise, against fp64):
fused MLP 4.5e-7 / 4.1e-7 forward and 6.4e-7 / 6.4e-7 gradients; edge block + node update 5.3e-7 / 4.0e-7 and 7.6e-7 / 5.8e-7; whole
models 1.8e-6 / 1.4e-6 and 1.3e-6 / 1.2e-6.  (Figures only: the bounds are the project's TOL_OUT = 1e-5 and TOL_GRAD = 2e-5.)"""
import pytest
import torch

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests.test_gpu_parity import TOL_GRAD, TOL_OUT, _mlp_sd, _weights

pytestmark = pytest.mark.gpu

MLP_NAMES = [f'm.0.layers.linear_{i}.{p}' for i in range(3) for p in ('weight', 'bias')] + ['m.1.weight', 'm.1.bias']
# Conditioning of an instance with max / min aggregates: all of d(max) goes to ONE edge, so where the two best candidates of a segment
# are closer than the rounding of the fp32 forward, which one wins is the arithmetic's choice and says nothing about parity.  An
# instance is used only when, in the fp64 forward, every winner leads its runner-up by more than TIE_REL of its own magnitude AND
# by more than TIE_SCALE of the largest magnitude among the aggregated rows (the criterion of test_model_vs_oracle: rows are sums
# of terms of that size, so that, not the winner's own size, is what their fp32 rounding scales with).
TIE_REL = 1e-5
TIE_SCALE = 2e-6
# ... and the same for ReLU: a hidden unit whose fp64 input lies within fp32 rounding of zero may be gated the other way by ANY fp32
# evaluation (tests/helpers.py: gate transfer), which moves the gradients upstream of it by 1e-3..1e-2.  Instances are used only when
# the smallest |ReLU input| of the fp64 run exceeds KINK, the criterion of test_flag_L15_sum_vs_oracle_fp64.
KINK = 3e-7


class _Leads:
    """Over every max / min aggregation of an fp64 oracle run: the smallest lead of a winner over its runner-up, relative to the
    winner (`rel`) and relative to the largest magnitude of that aggregation's input (`scale`); an exact tie counts as 0."""

    def __enter__(self):
        self.rel = self.scale = self.kink = float('inf')
        self._orig = O.segment_reduce

        def probe(data, segment_ids, num_segments, operation, return_arg=False):
            if operation in ('max', 'min') and data.dim() == 2 and data.shape[0] > 0:
                d = (data if operation == 'max' else -data).detach().double()
                ids = segment_ids.long()
                idx = ids.unsqueeze(1).expand_as(d)
                m1 = torch.full((num_segments, d.shape[1]), float('-inf'), dtype=d.dtype).scatter_reduce(0, idx, d, 'amax')
                top = d == m1[ids]
                ties = torch.zeros(num_segments, d.shape[1], dtype=d.dtype).scatter_add(0, idx, top.double())
                m2 = torch.full_like(m1, float('-inf')).scatter_reduce(0, idx, d.masked_fill(top, float('-inf')), 'amax')
                gap = torch.where(ties > 1, torch.zeros_like(m1), m1 - m2)
                ok = torch.isfinite(gap)                          # (segments with one row, or none, have no runner-up)
                if ok.any():
                    self.rel = min(self.rel, float((gap / m1.abs().clamp(min=1e-300))[ok].min()))
                    self.scale = min(self.scale, float(gap[ok].min() / d.abs().max().clamp(min=1e-30)))
            return self._orig(data, segment_ids, num_segments, operation, return_arg)
        O.segment_reduce = probe
        return self

    def __exit__(self, *exc):
        O.segment_reduce = self._orig
        return False

    def ok(self):
        return self.rel > TIE_REL and self.scale > TIE_SCALE

    def record(self, tid, first, used, what):
        H._REPORT.append({'test': tid, 'what': 'instance selection', 'first_seed_tried': first, 'seed_used': used, 'seeds_rejected': used - first,
                          'criterion': f'fp64 {what}: every max / min winner leads its runner-up by > {TIE_REL} of itself and > {TIE_SCALE} of '
                                       f'the largest aggregated magnitude; smallest |ReLU input| > {KINK}',
                          'lead_rel_to_winner': self.rel, 'lead_rel_to_scale': self.scale, 'smallest_relu_input': self.kink})


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()          # the HIP extension must be the thing that runs: fail loudly if it is not built
    yield


def _report_pair(tid, plain, split, exact, n_fwd):
    """Worst forward and worst gradient tensor of the plain path and of the default path on the same inputs -> parity report;
    tensors whose exact value is identically zero carry no relative error.  -> {name: error of the plain path}."""
    errs = {}
    for path, got in (('fp32-MFMA', plain), ('default', split)):
        e = {k: H.rel_err(got[k], exact[k]) for k in exact if float(exact[k].abs().max()) > 0}
        names = list(exact)
        for what, ks in (('forward', names[:n_fwd]), ('gradient', names[n_fwd:])):
            k = max((k for k in ks if k in e), key=lambda k_: e[k_])
            H.report(tid, f'{path}: worst {what} tensor ({k})', got[k], exact[k])
        if path == 'fp32-MFMA':
            errs = e
    return errs


# ---------------------------------------------------------------------------------------------------------------
# a. fused MLP, forward and backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 17, 64, 65, 333])
@pytest.mark.parametrize('case', ['latent_res', 'node2src', 'node_pna', 'encoder_idx'])
def test_fused_mlp_fp32_mfma_vs_fp64(M, case):
    """mlp_fwd_kernel / mlp_bwd_kernel / wgrad_dma_kernel behind ops.fused_mlp: one 128-wide source with residual, two 128-wide
    sources, 128 + 512 columns (several 128-blocks per source) and a narrow gathered source (the generic weight-gradient kernel beside
    the DMA ring).  Rows: one, a partial 16-row wave, exactly one 64-row tile, one row into a second tile (the tile's other 63 rows are
    clamped to row M - 1: a missing mask shows in the LayerNorm-gradient and weight-gradient sums), several tiles with a ragged end.
    Bounds: those of test_fused_mlp_vs_oracle."""
    from hgn_amd import ops
    residual = -1
    if case == 'encoder_idx':
        widths = [8]
    elif case == 'node2src':
        widths, residual = [128, 128], 0
    elif case == 'node_pna':
        widths, residual = [128, 512], 0
    else:
        widths, residual = [128], 0
    sd = _mlp_sd(sum(widths), 128, True, seed=M)
    first = M * 7 + len(case)
    for seed in range(first, first + 50):                      # the first input seed whose fp64 forward stays clear of every ReLU kink
        gen = torch.Generator().manual_seed(seed)
        idx = torch.randperm(M, generator=gen) if case == 'encoder_idx' else None
        srcs = [torch.randn(M, wd, generator=gen) for wd in widths]
        w_out = torch.randn(M, 128, generator=gen, dtype=torch.float64)
        sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        so = [s.double().requires_grad_(True) for s in srcs]
        with H.KinkMargin() as km:
            yo = O.mlp(sdo, 'm', torch.cat([so[0][idx] if idx is not None else so[0]] + so[1:], -1), layer_norm=True)
        if km.worst > KINK:
            break
    assert km.worst > KINK, 'no input seed without a ReLU input at fp32 rounding distance from zero'
    tid = f'test_fused_mlp_fp32_mfma_vs_fp64[{case}-{M}]'
    H._REPORT.append({'test': tid, 'what': 'instance selection', 'first_seed_tried': first, 'seed_used': seed, 'seeds_rejected': seed - first,
                      'criterion': f'smallest |ReLU input| of the fp64 run > {KINK}', 'margin_of_seed_used': km.worst})
    if residual >= 0:
        yo = yo + so[residual]
    (yo * w_out).sum().backward()
    exact = {'out': yo.detach()}
    exact.update({f'dx{i}': s.grad for i, s in enumerate(so)})
    exact.update({'d ' + n: sdo[n].grad for n in MLP_NAMES})

    def run():
        w, wts = _weights(sd, True)
        sh = [s.cuda().requires_grad_(True) for s in srcs]
        idxs = [idx.cuda().int() if idx is not None else None] + [None] * (len(sh) - 1)
        y = ops.fused_mlp(sh, w, idxs, residual)
        (y * w_out.float().cuda()).sum().backward()
        got = {'out': y.detach()}
        got.update({f'dx{i}': s.grad for i, s in enumerate(sh)})
        got.update({'d ' + n: t.grad for n, t in zip(MLP_NAMES, wts)})
        return got

    with ops.using(ops.Context(fp32_mfma=True)):
        plain = run()
    split = run()
    errs = _report_pair(tid, plain, split, exact, 1)
    print({k: f'{v:.2e}' for k, v in errs.items()})
    assert all(bool(torch.isfinite(t).all()) for t in plain.values())
    assert errs['out'] <= TOL_OUT, errs['out']
    bad = {k: v for k, v in errs.items() if k != 'out' and v > TOL_GRAD}
    assert not bad, bad
    assert any(not torch.equal(plain[k], split[k]) for k in plain), 'the flag changed nothing: the default kernels ran'


# ---------------------------------------------------------------------------------------------------------------
# b. edge block + node update, forward and backward
# ---------------------------------------------------------------------------------------------------------------
def _edge_node_instance(nx, ny, aggs):
    """Graph, weights, inputs (ORIGINAL edge order) and cotangents of one edge block + node update.
    The input seed is the first of 0, 1, 2, ... whose fp64 forward has no tie and no near-tie inside a segment (_Leads.ok: only with
    max / min among the aggregates) and no ReLU input within KINK of zero.  CPU only."""
    g = synth.grid_graph(seed=3, nx=nx, ny=ny)
    es = g.edge_sets[0]
    N, E = nx * ny, es.senders.shape[0]
    sd_e = _mlp_sd(384, 128, True, seed=nx)
    sd_n = _mlp_sd(128 + 128 * len(aggs), 128, True, seed=100 + ny)

    def inputs(seed):
        gen = torch.Generator().manual_seed(seed)
        return torch.randn(N, 128, generator=gen), torch.randn(E, 128, generator=gen)

    def ref(h0, e0, r_y=None, r_hn=None):
        pe = {k: v.double().requires_grad_(True) for k, v in sd_e.items()}
        pn = {k: v.double().requires_grad_(True) for k, v in sd_n.items()}
        h, e = h0.double().requires_grad_(True), e0.double().requires_grad_(True)
        y = O.update_edge_features(pe, 'm', [h], O.EdgeSet('x', e, es.senders, es.receivers))
        agg = torch.cat([O.segment_reduce(y, es.receivers, N, op) for op in aggs], -1)
        hn = h + O.mlp(pn, 'm', torch.cat([h, agg], -1))
        if r_y is None:
            return None
        ((hn * r_hn).sum() + (y * r_y).sum()).backward()
        exact = {'y': y.detach(), 'hn': hn.detach(), 'dh': h.grad, 'de': e.grad}
        exact.update({'d edge ' + n: pe[n].grad for n in MLP_NAMES})
        exact.update({'d node ' + n: pn[n].grad for n in MLP_NAMES})
        return exact

    for seed in range(200):                                     # (about one seed in five passes at 2 242 edges with max / min)
        with torch.no_grad(), _Leads() as leads, H.KinkMargin() as km:
            ref(*inputs(seed))
        if leads.ok() and km.worst > KINK:
            break
    assert leads.ok() and km.worst > KINK, 'no input seed below 200 without a near-tie or a ReLU input at rounding distance from zero'
    leads.kink = km.worst
    h0, e0 = inputs(seed)
    gen = torch.Generator().manual_seed(12345)
    # the loss is LINEAR in the outputs (fixed random cotangents): see test_split_products_cover_the_fp32_range for why not |out|^2
    r_y = torch.randn(E, 128, generator=gen, dtype=torch.float64)
    r_hn = torch.randn(N, 128, generator=gen, dtype=torch.float64)
    return es, N, E, sd_e, sd_n, h0, e0, r_y, r_hn, ref(h0, e0, r_y, r_hn), seed, leads


def _edge_node_run(es, N, sd_e, sd_n, h0, e0, r_y, r_hn, aggs):
    """The same on the HIP path, in the current context -> tensors in ORIGINAL edge order, named as in _edge_node_instance."""
    from hgn_amd import ops, topology
    topo = topology.EdgeTopology(es.senders.cuda(), es.receivers.cuda(), N, torch.device('cuda'))
    perm = topo.r.perm.long()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel(), device='cuda')
    we, wte = _weights(sd_e, True)
    wn, wtn = _weights(sd_n, True)
    h = h0.cuda().requires_grad_(True)
    e = e0.cuda()[perm].requires_grad_(True)                    # rows in receiver order, as the processor keeps them
    y, agg = ops.edge_block(h, e, topo, we, aggs)
    hn = ops.fused_mlp([h, agg], wn, None, 0)
    ((hn * r_hn.float().cuda()).sum() + (y * r_y.float().cuda()[perm]).sum()).backward()
    got = {'y': y.detach()[inv], 'hn': hn.detach(), 'dh': h.grad, 'de': e.grad[inv]}
    got.update({'d edge ' + n: t.grad for n, t in zip(MLP_NAMES, wte)})
    got.update({'d node ' + n: t.grad for n, t in zip(MLP_NAMES, wtn)})
    return got


AGGS = [('sum',), ('sum', 'mean', 'max', 'min'), ('max',)]


@pytest.mark.parametrize('aggs', AGGS, ids=['sum', 'pna', 'max'])
@pytest.mark.parametrize('nx,ny', [(2, 2), (7, 5), (20, 20)])
def test_edge_block_and_node_update_fp32_mfma_vs_fp64(nx, ny, aggs):
    """ops.edge_block + the node update under the flag: hgn_linear_fwd, mlp_fwd_kernel with n_add = 2, a separate aggregation launch,
    mlp_bwd_kernel with agg_dout (max / min through the saved arg rows), wgrad_dma_kernel, hgn_linear_bwd.  10 edges (less than a
    tile), 164 (a ragged third tile), 2 242 (36 tiles; weight-gradient chunks of 16-row multiples, the last one short)."""
    from hgn_amd import ops
    es, N, E, sd_e, sd_n, h0, e0, r_y, r_hn, exact, seed, leads = _edge_node_instance(nx, ny, aggs)
    with ops.using(ops.Context(fp32_mfma=True)):
        plain = _edge_node_run(es, N, sd_e, sd_n, h0, e0, r_y, r_hn, aggs)
    split = _edge_node_run(es, N, sd_e, sd_n, h0, e0, r_y, r_hn, aggs)
    tid = f"test_edge_block_and_node_update_fp32_mfma_vs_fp64[{nx}x{ny}-{'+'.join(aggs)}]"
    leads.record(tid, 0, seed, 'forward of the edge block and the node update')
    errs = _report_pair(tid, plain, split, exact, 2)
    print({k: f'{v:.2e}' for k, v in errs.items()})
    assert all(bool(torch.isfinite(t).all()) for t in plain.values())
    assert errs['y'] <= TOL_OUT and errs['hn'] <= TOL_OUT, (errs['y'], errs['hn'])
    bad = {k: v for k, v in errs.items() if k not in ('y', 'hn') and v > TOL_GRAD}
    assert not bad, bad
    assert any(not torch.equal(plain[k], split[k]) for k in plain), 'the flag changed nothing: the default kernels ran'


def test_edge_block_launches_the_kernels_its_context_names():
    """The library's own launch counters (ops.prof_collect) for one edge block, forward and backward: under the flag the plain
    backward kernel and the plain pre-projection pair, no fused backward; by default the fused backward and no launch of the
    two-launch backward.  (`linear_fwd` / `linear_bwd` count the pre-projection in either form, so they are only required, never
    forbidden.)"""
    from hgn_amd import ops
    aggs = ('sum',)
    es, N, E, sd_e, sd_n, h0, e0, r_y, r_hn, _, _, _ = _edge_node_instance(7, 5, aggs)
    seen = {}
    for name, ctx in (('plain', ops.Context(fp32_mfma=True)), ('default', ops.Context())):
        ops.prof_reset(); ops.prof_enable(True)
        try:
            with ops.using(ctx):
                _edge_node_run(es, N, sd_e, sd_n, h0, e0, r_y, r_hn, aggs)
            seen[name] = ops.prof_collect()
        finally:
            ops.prof_enable(False)
    for k in ('mlp_fwd_edge', 'mlp_bwd_edge', 'linear_fwd', 'linear_bwd', 'wgrad'):
        assert k in seen['plain'], (k, sorted(seen['plain']))
    assert 'edge_bwd_fused' not in seen['plain'], sorted(seen['plain'])
    assert 'edge_bwd_fused' in seen['default'] and 'mlp_bwd_edge' not in seen['default'], sorted(seen['default'])


# ---------------------------------------------------------------------------------------------------------------
# c. whole models
# ---------------------------------------------------------------------------------------------------------------
HIER = ['mesh_edges', 'intra_cluster_to_mesh', 'intra_cluster_to_cluster', 'inter_cluster']
MODELS = [
    ('none', 'sum', ['mesh_edges'], dict(seed=5, nx=9, ny=7), False),
    ('hetero', 'pna', HIER + ['world_edges'], dict(seed=5, nx=12, ny=8, clusters=5, world=19), False),
    ('hyper', 'sum', HIER, dict(seed=9, nx=20, ny=15, clusters=4), True),
]


@pytest.mark.parametrize('arch,agg,sets,gkw,flat', MODELS, ids=[f'{c[0]}-{c[1]}' for c in MODELS])
def test_model_fp32_mfma_vs_oracle(arch, agg, sets, gkw, flat):
    """Two message-passing steps of a whole model with its own context in fp32-MFMA mode against the fp64 oracle: outputs, loss,
    every parameter gradient, the gradients of the inputs.  The `hyper` case also trains through parallel.DataParallelTrainer with
    lr = 0 (gradients accumulate into the flat buffer: node-level weight-gradient tasks queued and launched 16 at a time,
    hgn_mlp_wgrad_partial + hgn_slab_reduce_batch, deferred LayerNorm sums): the flat gradient, slice by slice, against the oracle."""
    import hgn_amd
    from hgn_amd import parallel
    graph = synth.grid_graph(**gkw)
    assert sorted(e.name for e in graph.edge_sets) == sorted(sets)
    hyper_in = graph.node_features[1].shape[1] if len(graph.node_features) > 1 else 0
    nsn = {'node_model_cross': len(sets), 'hyper_node_model_cross': len(sets)} if arch == 'hetero' else None
    shapes = O.param_shapes(arch, agg, 2, sets, graph.node_features[0].shape[1], {e.name: e.features.shape[1] for e in graph.edge_sets},
                            hyper_in, 3, 128, nsn)
    N = graph.node_features[0].shape[0]
    target = torch.randn(N, 3, generator=torch.Generator().manual_seed(1))
    mask = torch.ones(N, dtype=torch.bool); mask[:3] = False
    order = ['mesh_edges', 'world_edges', 'inter_cluster', 'inter_cluster_world']
    # the first weight seed whose fp64 forward has no near-tie inside a segment (_Leads.ok) and no ReLU input within KINK of zero
    g64 = O.MultiGraph([x.double() for x in graph.node_features],
                       [O.EdgeSet(e.name, e.features.double(), e.senders, e.receivers) for e in graph.edge_sets])
    for wseed in range(11, 211):
        with torch.no_grad(), _Leads() as leads, H.KinkMargin() as km:
            O.mesh_graph_net({k: v.double() for k, v in O.init_state_dict_like(shapes, seed=wseed).items()}, g64, arch, agg, set_order=order)
        if leads.ok() and km.worst > KINK:
            break
    assert leads.ok() and km.worst > KINK, 'no weight seed in 11..210 without a near-tie or a ReLU input at rounding distance from zero'
    leads.kink = km.worst
    sd = O.init_state_dict_like(shapes, seed=wseed)
    out_o, loss_o, grads_o, ing_o = H.oracle_run(sd, graph, arch, agg, target, mask, set_order=order)
    tid = f'test_model_fp32_mfma_vs_oracle[{arch}-{agg}]'
    leads.record(tid, 11, wseed, 'forward of the model')

    def model(fp32_mfma):
        m = H.hip_model(arch, agg, 2, sets, sd, set_order=order)
        m.set_fp32_mfma(fp32_mfma)                              # before the first forward: the model enters its own context
        return m
    out, loss, grads, ing = H.hip_run(model(True), graph, target, mask)
    out_d, _, grads_d, _ = H.hip_run(model(None), graph, target, mask)
    H.report(tid, 'fp32-MFMA: output', out, out_o)
    H.report(tid, 'default: output', out_d, out_o)
    for path, g_ in (('fp32-MFMA', grads), ('default', grads_d)):
        wn, we = H.worst_grad(g_, grads_o)
        H._REPORT.append({'test': tid, 'what': f'{path}: param grads (worst tensor)', 'norm': wn, 'elem': we})
    assert H.rel_err(out, out_o) <= TOL_OUT and H.rel_err(loss, loss_o) <= TOL_OUT
    assert H.worst_grad(grads, grads_o)[0] <= TOL_GRAD, max((H.rel_err(grads[k], grads_o[k]), k) for k in grads_o if float(grads_o[k].abs().max()) > 0)
    for k in grads_o:
        if float(grads_o[k].abs().max()) == 0:
            assert float(grads[k].abs().max()) == 0, k
    for a, b in zip(ing['node'], ing_o['node']):
        assert H.rel_err(a, b) <= TOL_GRAD
    for name, b in ing_o['edge'].items():
        if b is not None and ing['edge'][name] is not None:
            assert H.rel_err(ing['edge'][name], b) <= TOL_GRAD, name
    assert not torch.equal(out, out_d)                          # the model's own context carried the flag into its launches
    if flat:
        G = hgn_amd.MultiGraph([x.cuda() for x in graph.node_features],
                               [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in graph.edge_sets])
        tr = parallel.DataParallelTrainer(model(True), lr=0.0)
        assert tr.ctx.fp32_only()
        tr.step(G, target.cuda(), mask.cuda())                  # lr = 0: parameters stay, the flat gradient is what we look at
        tr.step(G, target.cuda(), mask.cuda())
        assert not tr.ctx.wq and not tr.ctx.redq and not tr.ctx.lnq      # nothing left behind after backward()
        flat_g = {k: tr.fp.grad[off:off + p.numel()].view(p.shape) for (k, p), off in zip(tr.model.named_parameters(), tr.fp.offsets)}
        wn, we = H.worst_grad(flat_g, grads_o)
        H._REPORT.append({'test': tid, 'what': 'fp32-MFMA: flat gradient through the trainer (worst tensor)', 'norm': wn, 'elem': we})
        for k in grads_o:
            if float(grads_o[k].abs().max()) > 0:
                assert H.rel_err(flat_g[k], grads_o[k]) <= TOL_GRAD, k


# ---------------------------------------------------------------------------------------------------------------
# e. the flag travels per call
# ---------------------------------------------------------------------------------------------------------------
def test_fp32_mfma_model_and_default_model_interleaved_equal_their_solo_runs():
    """Two models in one process, one on the plain fp32-MFMA kernels and one on the default ones, trained step by step IN TURN: the flag
    travels in every argument struct and each model's ops.Context holds its own deferred queues, so each model's losses and parameters
    equal, bit for bit, those of the same model trained alone."""
    import hgn_amd
    from hgn_amd import ops, parallel
    graph = synth.grid_graph(seed=5, nx=14, ny=11, clusters=3)
    sets = [e.name for e in graph.edge_sets]
    shapes = O.param_shapes('hyper', 'pna', 2, sets, 5, {n: 7 for n in sets}, 8, 3, 128)
    G = hgn_amd.MultiGraph([x.cuda() for x in graph.node_features],
                           [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in graph.edge_sets])
    N = graph.node_features[0].shape[0]
    target = torch.randn(N, 3, generator=torch.Generator().manual_seed(2)).cuda()
    mask = torch.ones(N, dtype=torch.bool).cuda()

    def make(seed, plain):
        m = H.hip_model('hyper', 'pna', 2, sets, O.init_state_dict_like(shapes, seed=seed))
        m.set_fp32_mfma(plain)
        return parallel.DataParallelTrainer(m, lr=1e-3)

    def solo(seed, plain, steps=3):
        tr = make(seed, plain)
        losses = [tr.step(G, target, mask).clone() for _ in range(steps)]
        return losses, tr.fp.flat.clone()

    solo_a, solo_b = solo(1, None), solo(2, True)
    ta, tb = make(1, None), make(2, True)
    la, lb = [], []
    for _ in range(3):
        la.append(ta.step(G, target, mask).clone())
        lb.append(tb.step(G, target, mask).clone())
    assert all(torch.equal(x, y) for x, y in zip(la, solo_a[0])) and torch.equal(ta.fp.flat, solo_a[1])
    assert all(torch.equal(x, y) for x, y in zip(lb, solo_b[0])) and torch.equal(tb.fp.flat, solo_b[1])
    assert not ops.default_context().fp32_only() and not ta.ctx.fp32_only() and tb.ctx.fp32_only()
    # ... and the flag really was in effect for model b only: the default kernels on b's weights end at other parameters
    # (a one-element loss may agree by chance; a million parameters after three steps do not)
    tc = make(2, None)
    for _ in range(3):
        tc.step(G, target, mask)
    assert not torch.equal(tc.fp.flat, solo_b[1])
