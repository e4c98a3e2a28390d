"""Operand layout as a tested dimension (tests/view_layouts.py): every operator of hgn_amd.ops on views -- row slices, column offsets,
wider rows, every second row, transposes, expanded and fp64 tensors, and upstream gradients housed the way torch.cat's backward leaves
them -- against the same call on contiguous clones, BIT FOR BIT (ops._rowmajor: an operand's layout never changes which kernels run, nor
a bit of the result), the contiguous result against the fp64 oracle (helpers.rel_err: 1e-5 on outputs, 2e-5 on gradients), and the
NaN padding of the wider buffers: never read (the results are finite and equal), never written, gradient exactly zero.

No test hands a misaligned address to the C ABI: everything goes through hgn_amd.ops; the refusals are in tests/test_views_cpu.py."""
import pytest
import torch

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests import view_layouts as V
from tests.test_gpu_parity import _mlp_sd, _weights

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-5
TOL_GRAD = 2e-5
KINK_MIN = 3e-7          # smallest |ReLU input| of the fp64 run (test_split_bf16_products_are_fp32_accurate)
IN_PLACE_WIDE = ('row_slice', 'every_second_row', 'col0_of_wider4')      # the layouts a 128-wide operand keeps: also at the larger M


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _first_well_conditioned(tid, make):
    """make(seed) -> whatever an fp64 oracle run of the instance of that seed returns: the first seed 1, 2, ... whose run keeps every ReLU
    input farther than KINK_MIN from zero (the rule of test_split_bf16_products_are_fp32_accurate), recorded in the parity report."""
    for seed in range(1, 41):
        with H.KinkMargin() as km:
            got = make(seed)
        if km.worst > KINK_MIN:
            break
    assert km.worst > KINK_MIN, km.worst
    H._REPORT.append({'test': tid, 'what': 'instance selection', 'first_seed_tried': 1, 'seed_used': seed, 'seeds_rejected': seed - 1,
                      'criterion': 'smallest |ReLU input| of the fp64 run > 3e-7', 'margin_of_seed_used': km.worst})
    return got


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), what
        assert torch.equal(a, b), (what, H.rel_err(a, b))


# ---------------------------------------------------------------------------------------------------------------
# ops.fused_mlp
# ---------------------------------------------------------------------------------------------------------------
MLP_CASES = ['latent_res', 'node2src', 'node_pna', 'encoder7', 'encoder_idx', 'decoder3']
_MLP_NAMES = [f'linear_{i}.{p}' for i in range(3) for p in ('weight', 'bias')]


def _mlp_spec(case):
    """-> (source widths, LayerNorm, output width, residual source, gathered) of the cases of test_fused_mlp_vs_oracle"""
    return {'latent_res': ([128], True, 128, 0, False), 'node2src': ([128, 128], True, 128, 0, False),
            'node_pna': ([128, 1024], True, 128, 0, False), 'encoder7': ([7], True, 128, -1, False),
            'encoder_idx': ([8], True, 128, -1, True), 'decoder3': ([128], False, 3, -1, False)}[case]


def _mlp_instance(case, M, seed, device='cpu'):
    widths, ln, out_w, residual, gathered = _mlp_spec(case)
    gen = torch.Generator(device=device).manual_seed(1000 * seed + M)
    srcs = [torch.randn(M, wd, generator=gen, device=device) for wd in widths]
    w_out = torch.randn(M, out_w, generator=gen, device=device)
    idx = torch.randperm(M, generator=gen, device=device) if gathered else None
    return _mlp_sd(sum(widths), out_w, ln, seed=seed), srcs, w_out, idx


def _mlp_oracle(case, M):
    widths, ln, out_w, residual, gathered = _mlp_spec(case)

    def make(seed):
        sd, srcs, w_out, idx = _mlp_instance(case, M, seed)
        sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        so = [s.double().requires_grad_(True) for s in srcs]
        yo = O.mlp(sdo, 'm', torch.cat([so[0][idx] if idx is not None else so[0]] + so[1:], -1), layer_norm=ln)
        if residual >= 0:
            yo = yo + so[residual]
        (yo * w_out.double()).sum().backward()
        base = 'm.0.layers.' if ln else 'm.layers.'
        pg = [sdo[base + n].grad for n in _MLP_NAMES] + ([sdo['m.1.weight'].grad, sdo['m.1.bias'].grad] if ln else [])
        return seed, yo.detach(), [s.grad for s in so], pg
    return _cached(('mlp_oracle', case, M), lambda: _first_well_conditioned(f'test_fused_mlp_contiguous_vs_oracle[{case}]', make))


def _mlp_run(case, inst, layouts=None, grad_layout='contiguous'):
    """One forward + backward of ops.fused_mlp; layouts: {source index: layout}.  -> (out, source gradients, parameter gradients,
    the housed operands, the re-housed upstream gradients)"""
    from hgn_amd import ops
    widths, ln, out_w, residual, gathered = _mlp_spec(case)
    sd, srcs, w_out, idx = inst
    w, wts = _weights(sd, ln)
    housed = [V.Housed(s.cuda(), (layouts or {}).get(i, 'contiguous'), requires_grad=True) for i, s in enumerate(srcs)]
    idxs = [idx.cuda().int() if idx is not None else None] + [None] * (len(srcs) - 1)
    y = ops.fused_mlp([h.view for h in housed], w, idxs, residual)
    log = []
    (V.rehouse(y, grad_layout, log) * w_out.cuda()).sum().backward()
    return y.detach(), [h.grad() for h in housed], [t.grad for t in wts], housed, log


def _mlp_values_of(inst, housed):
    """The instance with the values the housed operands really hold (`expanded` repeats the first row)."""
    sd, srcs, w_out, idx = inst
    return sd, [h.values() for h in housed], w_out, idx


def _mlp_compare(case, inst, layouts, grad_layout, base=None):
    y, gs, gw, housed, log = _mlp_run(case, inst, layouts, grad_layout)
    if base is None or any(h.layout == 'expanded' for h in housed):
        base = _mlp_run(case, _mlp_values_of(inst, housed))[:3]
    y0, gs0, gw0 = base
    what = (case, layouts, grad_layout)
    _same(y, y0, what + ('out',))
    for i, (a, b) in enumerate(zip(gs, gs0)):
        if housed[i].layout == 'expanded':          # one row read M times: its gradient is the column sum of the M rows' (torch's sum)
            assert H.rel_err(a, b.double().sum(0, keepdim=True)) <= 1e-6, what
        else:
            _same(a, b, what + (f'd(source {i})',))
    for n, (a, b) in enumerate(zip(gw, gw0)):
        _same(a, b, what + (f'parameter gradient {n}',))
    assert all(h.padding_untouched() for h in housed), what
    assert V.gradients_left_alone(log), what


@pytest.mark.parametrize('case', MLP_CASES)
def test_fused_mlp_contiguous_vs_oracle(case):
    """(b) the contiguous run of the instance every view below is compared with, against fp64.  M = 70: two 64-row tiles, or five
    16-row workgroups with the last one partial."""
    M = 70
    widths, ln, out_w, residual, gathered = _mlp_spec(case)
    seed, yo, go, pgo = _mlp_oracle(case, M)
    y, gs, gw, _, _ = _mlp_run(case, _mlp_instance(case, M, seed))
    tid = f'test_fused_mlp_contiguous_vs_oracle[{case}]'
    assert H.report(tid, 'out', y, yo)['norm'] <= TOL_OUT
    for i, (a, b) in enumerate(zip(gs, go)):
        assert H.report(tid, f'd(source {i})', a, b)['norm'] <= TOL_GRAD
    for n, (a, b) in enumerate(zip(gw, pgo)):
        assert H.report(tid, f'parameter gradient {n}', a, b)['norm'] <= TOL_GRAD


@pytest.mark.parametrize('layout', V.LAYOUTS[1:])
@pytest.mark.parametrize('case', MLP_CASES)
def test_fused_mlp_sources_as_views(case, layout):
    """(a), (c): every source in turn (source 0 is the residual source of the cases that have one) in the layout."""
    M = 70
    seed = _mlp_oracle(case, M)[0]
    inst = _mlp_instance(case, M, seed)
    base = _cached(('mlp_base', case, M), lambda: _mlp_run(case, inst)[:3])
    for i in range(len(_mlp_spec(case)[0])):
        _mlp_compare(case, inst, {i: layout}, 'contiguous', base)
    if len(_mlp_spec(case)[0]) > 1:
        _mlp_compare(case, inst, {0: layout, 1: layout}, 'contiguous', base)


@pytest.mark.parametrize('grad_layout', V.GRAD_LAYOUTS[1:])
@pytest.mark.parametrize('case', MLP_CASES)
def test_fused_mlp_upstream_gradient_as_view(case, grad_layout):
    """(a), (c): the gradient of the output where torch.cat's backward (or any slicing consumer) leaves it -- for the 128-wide outputs
    the layouts hgn_mlp_bwd refuses (include/hgn_mp.h: hgn_mlp_bwd_t.d_out) and ops.MLPFn.backward therefore copies; the 3-wide
    decoder gradient stays where it is and is read element by element.  Alone, and with the residual source a view as well."""
    M = 70
    seed = _mlp_oracle(case, M)[0]
    inst = _mlp_instance(case, M, seed)
    base = _cached(('mlp_base', case, M), lambda: _mlp_run(case, inst)[:3])
    _mlp_compare(case, inst, None, grad_layout, base)
    _mlp_compare(case, inst, {0: 'col_offset1'}, grad_layout, base)


@pytest.mark.parametrize('M', [4100, 16400])
@pytest.mark.parametrize('case', MLP_CASES)
def test_fused_mlp_in_place_views_in_the_row_per_wave_forms(case, M):
    """launch_mlp6_fwd / launch_mlp6_bwd leave the column-split form above 4096 rows and the latency form above 16384: the layouts that
    stay in place, in both row-per-wave forms, bit for bit against the contiguous run of the same M."""
    inst = _mlp_instance(case, M, 1, device='cuda')
    base = _mlp_run(case, inst)[:3]
    n_src = len(_mlp_spec(case)[0])
    for layout in IN_PLACE_WIDE:
        _mlp_compare(case, inst, {i: layout for i in range(n_src)}, 'contiguous', base)


# ---------------------------------------------------------------------------------------------------------------
# ops.edge_block on the 7 x 5 grid of test_edge_block_vs_oracle
# ---------------------------------------------------------------------------------------------------------------
PNA = ('sum', 'mean', 'max', 'min')
_EDGE_NAMES = [f'm.0.layers.linear_{i}.{p}' for i in range(3) for p in ('weight', 'bias')] + ['m.1.weight', 'm.1.bias']


def _edge_topology():
    def make():
        from hgn_amd import topology
        g = synth.grid_graph(seed=7, nx=7, ny=5)
        es = g.edge_sets[0]
        N = 35
        return es, N, topology.EdgeTopology(es.senders, es.receivers, N, torch.device('cuda'))
    return _cached('edge_topology', make)


def _edge_instance(seed):
    es, N, topo = _edge_topology()
    E = es.senders.shape[0]
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return _mlp_sd(384, 128, True, seed=seed), rn(N, 128), rn(E, 128), rn(E, 128), rn(N, 4 * 128)


def _edge_oracle(agg, two):
    """fp64: e' and the aggregate over receivers; `two`: senders and receivers read two tensors (equal values, gradients of their own)."""
    es, N, topo = _edge_topology()

    def make(seed):
        sd, h, e, w_y, w_a = _edge_instance(seed)
        sdo = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        hs, hr, eo = h.double().requires_grad_(True), h.double().requires_grad_(True), e.double().requires_grad_(True)
        snd, rcv = es.senders.long(), es.receivers.long()
        x = torch.cat([hs[snd], (hr if two else hs)[rcv], eo], -1)
        yo = eo + O.mlp(sdo, 'm', x, layer_norm=True)
        ao = torch.cat([O.segment_reduce(yo, es.receivers, N, op) for op in agg], 1)
        ((yo * w_y.double()).sum() + (ao * w_a[:, :ao.shape[1]].double()).sum()).backward()
        return seed, yo.detach(), ao.detach(), hs.grad, hr.grad if two else None, eo.grad, [sdo[n].grad for n in _EDGE_NAMES]
    tid = f'test_edge_block_contiguous_vs_oracle[{"-".join(agg)}-{"two" if two else "one"}]'
    return _cached(('edge_oracle', agg, two), lambda: _first_well_conditioned(tid, make))


def _edge_run(agg, two, seed, layouts=None, grad_layouts=None, values=None):
    """layouts: {'h' / 'h_r' / 'e': layout}; grad_layouts: {'y' / 'agg': layout}; values: {operand: tensor} instead of the instance's.
    Edge rows in receiver-sorted order, as the model keeps them.  -> (e', aggregate, d(h), d(h_r), d(e), parameter gradients, ...)"""
    from hgn_amd import ops
    es, N, topo = _edge_topology()
    sd, h, e, w_y, w_a = _edge_instance(seed)
    perm = topo.r.perm.long()
    vals = {'h': h.cuda(), 'h_r': h.cuda(), 'e': e.cuda()[perm]}
    vals.update(values or {})
    layouts, grad_layouts = layouts or {}, grad_layouts or {}
    w, wts = _weights(sd, True)
    hd = {k: V.Housed(v, layouts.get(k, 'contiguous'), requires_grad=True) for k, v in vals.items() if two or k != 'h_r'}
    if two:
        y, a = ops.edge_block(hd['h'].view, hd['e'].view, topo, w, agg, parts=(0, 0), h_r=hd['h_r'].view)
    else:
        y, a = ops.edge_block(hd['h'].view, hd['e'].view, topo, w, agg)
    log = []
    loss = (V.rehouse(y, grad_layouts.get('y', 'contiguous'), log) * w_y.cuda()[perm]).sum()
    loss = loss + (V.rehouse(a, grad_layouts.get('agg', 'contiguous'), log) * w_a[:, :a.shape[1]].cuda()).sum()
    loss.backward()
    return (y.detach(), a.detach(), hd['h'].grad(), hd['h_r'].grad() if two else None, hd['e'].grad(), [t.grad for t in wts]), hd, log


def _edge_compare(agg, two, seed, layouts, grad_layouts, base):
    got, hd, log = _edge_run(agg, two, seed, layouts, grad_layouts)
    exp = [k for k, h in hd.items() if h.layout == 'expanded']
    if exp:
        base = _edge_run(agg, two, seed, values={k: hd[k].values() for k in exp})[0]
    what = (agg, two, layouts, grad_layouts)
    for name, a, b in zip(('out', 'aggregate', 'h', 'h_r', 'e'), got[:5], base[:5]):
        if name in exp:
            assert H.rel_err(a, b.double().sum(0, keepdim=True)) <= 1e-6, what
        else:
            _same(a, b, what + (name,))
    for n, (a, b) in enumerate(zip(got[5], base[5])):
        _same(a, b, what + (f'parameter gradient {n}',))
    assert all(h.padding_untouched() for h in hd.values()), what
    assert V.gradients_left_alone(log), what


@pytest.mark.parametrize('two', [False, True], ids=['one_node_tensor', 'two_node_tensors'])
@pytest.mark.parametrize('agg', [('sum',), PNA], ids=['sum', 'pna'])
def test_edge_block_contiguous_vs_oracle(agg, two):
    es, N, topo = _edge_topology()
    perm = topo.r.perm.long().cpu()
    seed, yo, ao, ghs, ghr, geo, pgo = _edge_oracle(agg, two)
    (y, a, gh, ghr_, ge, gw), _, _ = _edge_run(agg, two, seed)
    tid = f'test_edge_block_contiguous_vs_oracle[{"-".join(agg)}-{"two" if two else "one"}]'
    assert H.report(tid, 'out', y, yo[perm])['norm'] <= TOL_OUT
    assert H.report(tid, 'aggregate', a, ao)['norm'] <= TOL_OUT
    assert H.report(tid, 'd(h)', gh, ghs)['norm'] <= TOL_GRAD
    if two:
        assert H.report(tid, 'd(h_r)', ghr_, ghr)['norm'] <= TOL_GRAD
    assert H.report(tid, 'd(e)', ge, geo[perm])['norm'] <= TOL_GRAD
    for n, (g, go) in enumerate(zip(gw, pgo)):
        assert H.report(tid, f'parameter gradient {n}', g, go)['norm'] <= TOL_GRAD


@pytest.mark.parametrize('layout', V.LAYOUTS[1:])
@pytest.mark.parametrize('two', [False, True], ids=['one_node_tensor', 'two_node_tensors'])
@pytest.mark.parametrize('agg', [('sum',), PNA], ids=['sum', 'pna'])
def test_edge_block_operands_as_views(agg, two, layout):
    seed = _edge_oracle(agg, two)[0]
    base = _cached(('edge_base', agg, two), lambda: _edge_run(agg, two, seed)[0])
    for k in ('h', 'e') + (('h_r',) if two else ()):
        _edge_compare(agg, two, seed, {k: layout}, None, base)
    _edge_compare(agg, two, seed, {k: layout for k in ('h', 'h_r', 'e')}, None, base)


@pytest.mark.parametrize('grad_layout', V.GRAD_LAYOUTS[1:])
@pytest.mark.parametrize('two', [False, True], ids=['one_node_tensor', 'two_node_tensors'])
@pytest.mark.parametrize('agg', [('sum',), PNA], ids=['sum', 'pna'])
def test_edge_block_upstream_gradients_as_views(agg, two, grad_layout):
    """The gradient of e', the gradient of the aggregate, both -- and both with every operand a column-offset view as well."""
    seed = _edge_oracle(agg, two)[0]
    base = _cached(('edge_base', agg, two), lambda: _edge_run(agg, two, seed)[0])
    for gl in ({'y': grad_layout}, {'agg': grad_layout}, {'y': grad_layout, 'agg': grad_layout}):
        _edge_compare(agg, two, seed, None, gl, base)
    _edge_compare(agg, two, seed, {k: 'col_offset1' for k in ('h', 'h_r', 'e')}, {'y': grad_layout, 'agg': grad_layout}, base)


# ---------------------------------------------------------------------------------------------------------------
# the plain fp32-MFMA kernels (ops.Context(fp32_mfma=True)): mlp_fwd_kernel / mlp_bwd_kernel / linear_*_kernel, whose loads of the
# residual, of d_out (csrc/mlp_common.h: load_dout) and of the pre-projection rows are 16-byte loads without a test of their own
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['latent_res', 'node_pna', 'encoder7', 'decoder3'])
def test_plain_fp32_mlp_kernels_on_views(case):
    """Bit for bit against the contiguous run of the same kernels (their accuracy against fp64: tests/test_gpu_fp32_mfma.py)."""
    from hgn_amd import ops
    M = 70
    inst = _mlp_instance(case, M, _mlp_oracle(case, M)[0])
    split = _cached(('mlp_base', case, M), lambda: _mlp_run(case, inst)[:3])
    with ops.using(ops.Context(fp32_mfma=True)):
        base = _mlp_run(case, inst)[:3]
        # other kernels ran (the 3-wide decoder has no other)
        assert case == 'decoder3' or any(not torch.equal(a, b) for a, b in zip([base[0]] + base[1] + base[2], [split[0]] + split[1] + split[2]))
        for layout in V.LAYOUTS[1:]:
            _mlp_compare(case, inst, {i: layout for i in range(len(inst[1]))}, 'contiguous', base)
        for grad_layout in V.GRAD_LAYOUTS[1:]:
            _mlp_compare(case, inst, {0: 'col_offset1'}, grad_layout, base)


@pytest.mark.parametrize('two', [False, True], ids=['one_node_tensor', 'two_node_tensors'])
@pytest.mark.parametrize('agg', [('sum',), PNA], ids=['sum', 'pna'])
def test_plain_fp32_edge_block_kernels_on_views(agg, two):
    from hgn_amd import ops
    seed = _edge_oracle(agg, two)[0]
    with ops.using(ops.Context(fp32_mfma=True)):
        base = _edge_run(agg, two, seed)[0]
        for layout in V.LAYOUTS[1:]:
            _edge_compare(agg, two, seed, {k: layout for k in ('h', 'h_r', 'e')}, None, base)
        for grad_layout in V.GRAD_LAYOUTS[1:]:
            _edge_compare(agg, two, seed, {k: 'col_offset1' for k in ('h', 'h_r', 'e')}, {'y': grad_layout, 'agg': grad_layout}, base)


# ---------------------------------------------------------------------------------------------------------------
# ops.aggregate / hgn_amd.unsorted_segment_operation
# ---------------------------------------------------------------------------------------------------------------
SEG_OPS = ('sum', 'mean', 'max', 'min', 'std')
# how -> ops.  'public': hgn_amd.unsorted_segment_operation once per op (rows in the caller's order); 'std_list': ops.aggregate with 'std'
# in a list of four (hgn_segment_reduce5_*); 'pna': ops.aggregate with the four ops of the four-operation kernels
SEG_LISTS = {'public': SEG_OPS, 'std_list': ('std', 'mean', 'max', 'min'), 'pna': ('sum', 'mean', 'max', 'min')}


def _segments():
    from tests.test_gpu_std import _case
    ids, N, _ = _case('lengths')                     # segment lengths [0, 2, 3, 4, 5, 9, 70], rows in random order
    return ids, N


def _segment_oracle(D, how):
    def make():
        ids, N = _segments()
        gen = torch.Generator().manual_seed(D)
        data = torch.randn(ids.numel(), D, generator=gen)
        w = torch.randn(N, len(SEG_LISTS[how]) * D, generator=gen)
        xo = data.double().requires_grad_(True)
        yo = torch.cat([O.segment_reduce(xo, ids, N, op) for op in SEG_LISTS[how]], 1)
        (yo * w.double()).sum().backward()
        return data, w, yo.detach(), xo.grad
    return _cached(('segment_oracle', D, how), make)


def _segment_run(D, how, layout='contiguous', grad_layout='contiguous', values=None):
    import hgn_amd
    from hgn_amd import ops, topology
    ids, N = _segments()
    data, w, _, _ = _segment_oracle(D, how)
    x = V.Housed(values if values is not None else data.cuda(), layout, requires_grad=True)
    log = []
    if how == 'public':
        # one backward pass per op, gradients side by side [E, 5 D]: the engine's own sum of five contributions (in the precision of
        # the leaf, fp64 for the fp64 layout) is no part of what is compared bit for bit
        ys, gs = [], []
        for i, op in enumerate(SEG_OPS):
            yi = hgn_amd.unsorted_segment_operation(x.view, ids.cuda(), N, op)
            (gi,) = torch.autograd.grad((V.rehouse(yi, grad_layout, log) * w.cuda()[:, i * D:(i + 1) * D]).sum(), x.leaf)
            assert x.pad is None or not bool(gi[x.pad].any())
            ys.append(yi.detach().float())
            gs.append(x.of_leaf(gi))
        return torch.cat(ys, 1), torch.cat(gs, 1), x, log
    else:
        csr = topology.segment_csr(ids.cuda(), N, torch.device('cuda'))
        y = V.rehouse(ops.aggregate([x.view], [(csr.perm, csr.rowptr, csr.seg)], SEG_LISTS[how]), grad_layout, log)
    (y * w.cuda()).sum().backward()
    return y.detach().float(), x.grad(), x, log      # (the public function answers in the dtype it was asked in: fp32 values either way)


@pytest.mark.parametrize('D', [128, 3])
@pytest.mark.parametrize('how', list(SEG_LISTS))
def test_segment_operations_contiguous_vs_oracle(how, D):
    data, w, yo, go = _segment_oracle(D, how)
    y, g, _, _ = _segment_run(D, how)
    tid = f'test_segment_operations_contiguous_vs_oracle[{how}-{D}]'
    assert H.report(tid, 'out', y, yo)['norm'] <= TOL_OUT
    if how == 'public':                                   # (one gradient per op, side by side: the oracle has their sum)
        g = g.double().view(g.shape[0], len(SEG_OPS), D).sum(1)
    assert H.report(tid, 'd(data)', g, go)['norm'] <= TOL_GRAD


@pytest.mark.parametrize('layout', V.LAYOUTS[1:])
@pytest.mark.parametrize('D', [128, 3])
@pytest.mark.parametrize('how', list(SEG_LISTS))
def test_segment_operations_on_views(how, D, layout):
    y, g, x, _ = _segment_run(D, how, layout)
    y0, g0, _, _ = _segment_run(D, how, values=x.values()) if layout == 'expanded' else _cached(('segment_base', how, D), lambda: _segment_run(D, how))
    _same(y, y0, (how, D, layout, 'out'))
    if layout == 'expanded':
        # equal rows: a segment without variance, whose 'std' gradient is NaN in the reference as well (test_gpu_std) -- on the view as
        # on the clone; without 'std' the one row's gradient is the column sum of the rows' gradients
        want = g0.double().sum(0, keepdim=True)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(g), nan) and ('std' in SEG_LISTS[how] or not bool(nan.any()))
        assert bool(nan.all()) or H.rel_err(g[~nan], want[~nan]) <= 1e-6
    else:
        _same(g, g0, (how, D, layout, 'd(data)'))
    assert x.padding_untouched()


@pytest.mark.parametrize('grad_layout', V.GRAD_LAYOUTS[1:])
@pytest.mark.parametrize('D', [128, 3])
@pytest.mark.parametrize('how', list(SEG_LISTS))
def test_segment_operations_upstream_gradient_as_view(how, D, grad_layout):
    y, g, x, log = _segment_run(D, how, 'col_offset1', grad_layout)
    y0, g0, _, _ = _cached(('segment_base', how, D), lambda: _segment_run(D, how))
    _same(y, y0, (how, D, grad_layout, 'out'))
    _same(g, g0, (how, D, grad_layout, 'd(data)'))
    assert x.padding_untouched() and V.gradients_left_alone(log) and len(log) == (len(SEG_OPS) if how == 'public' else 1)


# ---------------------------------------------------------------------------------------------------------------
# the public API: GraphNet blocks and the whole MeshGraphNet on a MultiGraph of views, the latent read through torch.cat
# ---------------------------------------------------------------------------------------------------------------
def _offset_view(x, lead=3):
    """x's rows as a column-offset view (address 12 bytes past a 16-byte boundary, row stride W + 3) of a NaN-padded tensor made by
    torch.cat: differentiable, and its backward hands x's producer a gradient in the same layout."""
    pad = torch.full((x.shape[0], lead), float('nan'), device=x.device)
    return torch.cat([pad, x], 1)[:, lead:]


def _staged_on_views(model, graph, target, mask, views):
    """helpers.hip_staged with every tensor that crosses the public API a view: the raw node and edge features column-offset views of
    NaN-padded buffers, the latents between the blocks re-housed by torch.cat, and the output latent read by the decoder THROUGH
    torch.cat([latent, extra], 1) -- an outside consumer whose backward hands the last block a [N, 131]-strided gradient."""
    import hgn_amd
    layout = 'col_offset1' if views else 'contiguous'
    nodes = [V.Housed(x.cuda(), layout, requires_grad=True) for x in graph.node_features]
    edges = [V.Housed(e.features.cuda(), layout, requires_grad=True) for e in graph.edge_sets]
    G = hgn_amd.MultiGraph([h.view for h in nodes],
                           [hgn_amd.EdgeSet(e.name, h.view, e.senders.cuda(), e.receivers.cuda()) for e, h in zip(graph.edge_sets, edges)])
    re = _offset_view if views else (lambda x: x)
    model.zero_grad(set_to_none=True)
    g = model.encoder(G)
    blocks = []
    for blk in model.processor.graphnet_blocks:
        g = blk(g._replace(node_features=[re(x) for x in g.node_features],
                           edge_sets=[e._replace(features=re(e.features)) for e in g.edge_sets]))
        blocks.append(g)
    latent = g.node_features[0]
    if views:
        extra = torch.full((latent.shape[0], 3), float('nan'), device=latent.device)
        latent = torch.cat([latent, extra], 1)[:, :128]
    out = model.decoder(g._replace(node_features=latent))
    loss = torch.nn.functional.mse_loss(target.cuda()[mask.cuda()], out[mask.cuda()])
    loss.backward()
    return {'blocks': blocks, 'out': out.detach(), 'loss': loss.detach(), 'grads': H.param_grads(model.named_parameters()),
            'in_grads': [h.grad() for h in nodes + edges], 'housed': nodes + edges}


@pytest.mark.parametrize('share', [True, False], ids=['shared', 'not_shared'])
@pytest.mark.parametrize('arch,agg', [('none', 'sum'), ('hyper', 'pna')], ids=['none-sum', 'hyper-pna'])
def test_public_api_on_views_vs_oracle(arch, agg, share, monkeypatch):
    """The gradient-sharing case.  ops.share_grad / shared_grad key on the address of the node latent a block was handed: a latent that
    is a misaligned view is copied, and a copy made inside ONE of its consumers would never meet the other in that table.  The join
    copies once for both (ops._JoinFn), so the staged run on views gives the bits of the staged run on contiguous tensors, with the
    sharing on and off; and every output and gradient agrees with helpers.oracle_staged."""
    from hgn_amd import ops
    from tests import test_gpu_public_api as P
    ref, km, tm = P.oracle_staged(arch, agg)
    P._well_conditioned(km, tm, agg, 'staged')
    seed = P.SEED_A[f'{arch}-{agg}']
    g, sets, sd, target, mask = P._instance(arch, agg, seed)
    model = P._model(arch, agg, seed)
    tid = f'test_public_api_on_views_vs_oracle[{arch}-{agg}-{"shared" if share else "not_shared"}]'
    H._REPORT.append({'test': tid, 'what': 'instance', 'seed_used': seed, 'smallest_relu_input_of_the_fp64_run': km.worst})
    if not share:
        monkeypatch.setattr(ops, '_SHARE_GRADS', False)
    before = dict(ops.share_stats)
    got = _staged_on_views(model, g, target, mask, True)
    acc_views = ops.share_stats['accumulated'] - before['accumulated']
    before = dict(ops.share_stats)
    flat = _staged_on_views(model, g, target, mask, False)
    acc_flat = ops.share_stats['accumulated'] - before['accumulated']
    H._REPORT.append({'test': tid, 'what': 'edge-block gradients accumulated into the node update\'s tensor', 'views': acc_views, 'contiguous': acc_flat})
    assert acc_views == acc_flat, (acc_views, acc_flat)               # the layout does not decide how d(h) is summed
    assert acc_flat == 0 if not share else (acc_flat > 0 or arch != 'none'), acc_flat
    # (b) the contiguous run against fp64, (a) the run on views against the contiguous run
    for run, name in ((flat, 'contiguous'), (got, 'views')):
        for i, (a, b) in enumerate(zip(run['blocks'], ref['blocks'])):
            P._check_graph(tid, f'{name}: block {i}', a, b)
        assert H.report(tid, f'{name}: decoder output', run['out'], ref['out'])['norm'] <= TOL_OUT
        assert H.rel_err(run['loss'], ref['loss']) <= TOL_OUT
        live = [k for k in ref['grads'] if float(ref['grads'][k].abs().max()) > 0]
        assert P._worst(tid, f'{name}: parameter gradients', [(k, run['grads'][k], ref['grads'][k]) for k in live]) <= TOL_GRAD
        for k in ref['grads']:
            assert k in live or float(run['grads'][k].abs().max()) == 0, k
        refs = list(ref['in_grads']['node']) + [ref['in_grads']['edge'][e.name] for e in g.edge_sets]
        assert P._worst(tid, f'{name}: input gradients', [(str(i), a, b) for i, (a, b) in enumerate(zip(run['in_grads'], refs))]) <= TOL_GRAD
        assert all(h.padding_untouched() for h in run['housed'])
    _same(got['out'], flat['out'], 'decoder output')
    for a, b in zip(got['blocks'], flat['blocks']):
        for x, y in zip(list(a.node_features) + [e.features for e in a.edge_sets], list(b.node_features) + [e.features for e in b.edge_sets]):
            _same(x.detach(), y.detach(), 'latents')
    for k in flat['grads']:
        _same(got['grads'][k], flat['grads'][k], k)
    for i, (a, b) in enumerate(zip(got['in_grads'], flat['in_grads'])):
        _same(a, b, f'input gradient {i}')


@pytest.mark.parametrize('arch,agg', [('none', 'sum'), ('hyper', 'pna')], ids=['none-sum', 'hyper-pna'])
def test_whole_model_on_views_equals_contiguous_bit_for_bit(arch, agg):
    """MeshGraphNet.forward + backward on a MultiGraph whose node and edge features are column-offset views (narrow encoder inputs:
    they stay in place and are read on the masked path at whatever address they have)."""
    import hgn_amd
    from tests import test_gpu_public_api as P
    seed = P.SEED_A[f'{arch}-{agg}']
    g, sets, sd, target, mask = P._instance(arch, agg, seed)
    model = P._model(arch, agg, seed)

    def run(layout):
        nodes = [V.Housed(x.cuda(), layout, requires_grad=True) for x in g.node_features]
        edges = [V.Housed(e.features.cuda(), layout, requires_grad=True) for e in g.edge_sets]
        G = hgn_amd.MultiGraph([h.view for h in nodes],
                               [hgn_amd.EdgeSet(e.name, h.view, e.senders.cuda(), e.receivers.cuda()) for e, h in zip(g.edge_sets, edges)])
        model.zero_grad(set_to_none=True)
        out = model(G)
        torch.nn.functional.mse_loss(target.cuda()[mask.cuda()], out[mask.cuda()]).backward()
        assert all(h.padding_untouched() for h in nodes + edges)
        return out.detach(), [h.grad() for h in nodes + edges], H.param_grads(model.named_parameters())
    out0, gi0, gp0 = run('contiguous')
    for layout in ('col_offset1', 'lead_of_wider1', 'every_second_row'):
        out, gi, gp = run(layout)
        _same(out, out0, (layout, 'out'))
        for i, (a, b) in enumerate(zip(gi, gi0)):
            _same(a, b, (layout, f'input gradient {i}'))
        for k in gp0:
            _same(gp[k], gp0[k], (layout, k))
