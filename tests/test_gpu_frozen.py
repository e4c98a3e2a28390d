"""Frozen MLPs on the GPU: a model (or any subset of its MLPs) whose parameters do not require grad, differentiated with respect to
its inputs.  Such an MLP saves no z1 / z2 in its forward (ops.is_frozen; csrc/mlp6.hip: mlp6_fwd_edge_kernel<NP, false> for edge
launches of >= 98 304 rows, the null-z paths of the general kernels below), stores no dz3 / dz2 in its backward and launches no
weight-gradient or LayerNorm-affine sum (hgn_mlp_bwd with HGN_F_DATA_ONLY).

Yardstick, unless a test says otherwise: the SAME call with the weights trainable under ops.Context(fused_edge_bwd=False) -- both runs
then go through the same data kernels, rows are independent, so outputs, saves and data gradients are equal BIT FOR BIT.  Against the
default fused edge backward: 2e-6, the project's figure for fused against two-launch (tests/test_gpu_product_modes.py: TOL_SUM)."""
import copy
import functools

import pytest
import torch

from oracle import features_oracle as FO
from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth
from tests import test_gpu_feature_grad as FG
from tests import test_gpu_parity as P
from tests import test_gpu_product_modes as PM
from tests import test_gpu_unrolled_training as UT

pytestmark = pytest.mark.gpu
MODES = ['fp32', 'fp32-bf16x3']
TOL_SUM = PM.TOL_SUM
EDGE_ROWS = 98304


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()
    yield


def _randn(*shape, seed):
    return torch.randn(*shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


def _freeze(wts, frozen=True):
    for t in wts:
        t.requires_grad_(not frozen)
        t.grad = None


# ---------------------------------------------------------------------------------------------------------------
# 1. the edge forward without z saves
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_set(E):
    """A receiver-sorted edge set of exactly E rows: 8 rows per receiver (the last one fewer), random senders."""
    from hgn_amd import topology
    N = (E + 7) // 8
    rcv = torch.arange(E, dtype=torch.int64) // 8
    snd = torch.randint(0, N, (E,), generator=torch.Generator().manual_seed(E))
    topo = topology.EdgeTopology(snd.cuda(), rcv.cuda(), N, torch.device('cuda'))
    assert topo.num_edges == E and topo.r.max_rows <= 12
    return topo, N


def _edge_forward(E, mode, frozen, wts, w):
    from hgn_amd import ops
    topo, N = _edge_set(E)
    _freeze(wts, frozen)
    h, e = _randn(N, 128, seed=1).requires_grad_(True), _randn(E, 128, seed=2).requires_grad_(True)
    with ops.using(ops.Context(precision=mode, fused_edge_bwd=False)):
        ops.prof_reset(); ops.prof_enable(True)
        try:
            y, agg = ops.edge_block(h, e, topo, w, ('sum',))
            kern = ops.prof_collect()
        finally:
            ops.prof_enable(False)
    return y, agg, kern


@pytest.mark.parametrize('E', [EDGE_ROWS, EDGE_ROWS + 19, 99019, EDGE_ROWS - 1])
@pytest.mark.parametrize('mode', MODES)
def test_edge_forward_without_z_saves_has_the_bits_of_the_saving_form(mode, E):
    """98 304 rows: the smallest launch of the edge kernel, 768 full tiles (the path with the static wait count only); 98 323: the last
    workgroup has a partial first and an empty second sub-tile; 99 019: a full first and a partial second; 98 303: the 64-row general
    form with null z1 / z2.  out, the in-kernel `sum` aggregate, x-hat, 1/sigma and the sign words: torch.equal over all rows."""
    sd = P._mlp_sd(384, 128, True, seed=4)
    w, wts = P._weights(sd, True)
    y_t, agg_t, kern_t = _edge_forward(E, mode, False, wts, w)
    saves_t = list(y_t.grad_fn.saves)
    assert all(torch.is_tensor(t) for t in saves_t)
    y_f, agg_f, kern_f = _edge_forward(E, mode, True, wts, w)
    saves_f = list(y_f.grad_fn.saves)
    _freeze(wts, False)
    assert 'mlp_fwd_edge' in kern_t and 'mlp_fwd_edge' in kern_f
    assert len(saves_f) == 5 and saves_f[0] is None and saves_f[1] is None
    assert torch.equal(y_f, y_t), 'out'
    assert torch.equal(agg_f, agg_t), 'aggregate'
    for name, a_, b_ in zip(PM.SAVES[2:], saves_f[2:], saves_t[2:]):
        assert a_.shape == b_.shape and torch.equal(a_, b_), name
    assert float(agg_f.detach().abs().max()) > 0 and float(y_f.detach().abs().max()) > 0


def test_edge_forward_form_as_the_library_reports_it(monkeypatch):
    """The launches the test above makes: at 98 304 rows the edge kernel without saves (2) frozen and with them (1) trainable, at
    98 303 the general kernel (0) -- asked of the library with the very argument struct ops hands to hgn_mlp_fwd."""
    from hgn_amd import _lib
    handle, seen = _lib.lib(), []

    class Spy:
        def __getattr__(self, name):
            if name != 'hgn_mlp_fwd':
                return getattr(handle, name)

            def fwd(a, st):
                seen.append(int(handle.hgn_mlp_fwd_edge_form(a)))
                return handle.hgn_mlp_fwd(a, st)
            return fwd
    sd = P._mlp_sd(384, 128, True, seed=4)
    w, wts = P._weights(sd, True)
    for E in (EDGE_ROWS, EDGE_ROWS - 1):
        _edge_set(E)
    spy = Spy()
    monkeypatch.setattr(_lib, 'lib', lambda: spy)
    for E, frozen in ((EDGE_ROWS, True), (EDGE_ROWS, False), (EDGE_ROWS - 1, True)):
        _edge_forward(E, 'fp32', frozen, wts, w)
    _freeze(wts, False)
    assert seen == [2, 1, 0], seen


# ---------------------------------------------------------------------------------------------------------------
# 2. the small forms with null z
# ---------------------------------------------------------------------------------------------------------------
SMALL_CASES = dict(PM.CASES, decoder3=([128], -1))


def _fused_mlp_run(case, M, mode, frozen):
    from hgn_amd import ops
    widths, residual = SMALL_CASES[case]
    ln = case != 'decoder3'
    sd = P._mlp_sd(sum(widths), 128 if ln else 3, ln, seed=5)
    w, wts = P._weights(sd, ln)
    _freeze(wts, frozen)
    xs = [_randn(M, wd, seed=11 + i).requires_grad_(True) for i, wd in enumerate(widths)]
    with ops.using(ops.Context(precision=mode, fused_edge_bwd=False)):
        y = ops.fused_mlp(xs, w, [None] * len(xs), residual)
        saves = list(y.grad_fn.saves)
        y.backward(_randn(M, y.shape[1], seed=7))
    return y.detach(), saves, [x.grad for x in xs], [t.grad for t in wts]


@pytest.mark.parametrize('case', list(SMALL_CASES))
@pytest.mark.parametrize('mode,M', [(m, M) for m in MODES for M in (1, 63, 64, 65, 300, 20011)] + [('bf16', 300), ('fp16', 300)])
def test_fused_mlp_frozen_equals_trainable_bit_for_bit(mode, M, case):
    """Column-split (<= 4 096 rows), latency (<= 16 384) and 64-row forms of forward and backward with null z1 / z2 / dz3 / dz2 / dz1,
    and the plain fp32 kernels of the 3-wide decoder: output, x-hat, 1/sigma, sign words and every source gradient torch.equal."""
    y_t, s_t, dx_t, gw_t = _fused_mlp_run(case, M, mode, False)
    y_f, s_f, dx_f, gw_f = _fused_mlp_run(case, M, mode, True)
    assert all(g is not None for g in gw_t) and all(g is None for g in gw_f)
    assert s_f[0] is None and s_f[1] is None and torch.is_tensor(s_t[0])
    assert torch.equal(y_f, y_t)
    for a_, b_ in zip(s_f[2:], s_t[2:]):
        assert (a_ is None) == (b_ is None) and (a_ is None or torch.equal(a_, b_))
    for i, (a_, b_) in enumerate(zip(dx_f, dx_t)):
        assert a_ is not None and float(a_.abs().max()) > 0 and torch.equal(a_, b_), f'd source {i}'


# ---------------------------------------------------------------------------------------------------------------
# 3. edge block backward
# ---------------------------------------------------------------------------------------------------------------
def _edge_graph(which):
    if which == 'small':
        g = synth.grid_graph(seed=3, nx=5, ny=4)
        es = g.edge_sets[0]
        return es, g.node_features[0].shape[0]
    _, es, N, _, _ = PM._batch()
    return es, N


def _edge_block_run(which, agg_ops, two_parts, mode, frozen, fused, wts, w):
    from hgn_amd import ops, topology
    es, N = _edge_graph(which)
    E = es.senders.shape[0]
    topo = topology.EdgeTopology(es.senders.cuda(), es.receivers.cuda(), N, torch.device('cuda'))
    _freeze(wts, frozen)
    h = _randn(N, 128, seed=1).requires_grad_(True)
    h2 = _randn(N, 128, seed=6).requires_grad_(True) if two_parts else None
    e = _randn(E, 128, seed=2).requires_grad_(True)
    with ops.using(ops.Context(precision=mode, fused_edge_bwd=fused)):
        if two_parts:
            y, agg = ops.edge_block(h, e, topo, w, agg_ops, parts=(0, 0), h_r=h2)
        else:
            y, agg = ops.edge_block(h, e, topo, w, agg_ops)
        torch.autograd.backward([y, agg], [_randn(E, 128, seed=3), _randn(N, len(agg_ops) * 128, seed=5)])
    return {'y': y.detach(), 'agg': agg.detach(), 'de': e.grad, 'dh': h.grad, **({'dh_r': h2.grad} if two_parts else {})}


AGGS = {'sum': ('sum',), 'pna': ('sum', 'mean', 'max', 'min'), 'std': ('sum', 'std', 'max')}


@pytest.mark.parametrize('two_parts', [False, True], ids=['one_tensor', 'two_parts'])
@pytest.mark.parametrize('agg', list(AGGS))
@pytest.mark.parametrize('which', ['small', 'batch'])
@pytest.mark.parametrize('mode', MODES)
def test_edge_block_backward_frozen_equals_trainable(mode, which, agg, two_parts):
    """de and dh (one node tensor for both sides; sender and receiver parts in tensors of their own) on a 5 x 4 mesh and on the
    11 x (40 x 40) batch of test_gpu_product_modes, for `sum`, the four pna aggregates (the kernel form that parks d(e') + the scattered
    aggregation backward) and a list with 'std' (streaming pre-pass): torch.equal against the trainable two-launch run; within 2e-6 of
    the trainable run on the default fused path."""
    sd = P._mlp_sd(384, 128, True, seed=4)
    w, wts = P._weights(sd, True)
    try:
        ref = _edge_block_run(which, AGGS[agg], two_parts, mode, False, False, wts, w)
        fus = _edge_block_run(which, AGGS[agg], two_parts, mode, False, True, wts, w)
        got = _edge_block_run(which, AGGS[agg], two_parts, mode, True, None, wts, w)
        assert all(t.grad is None for t in wts)
    finally:
        _freeze(wts, False)
    for k in ref:
        assert got[k] is not None and float(got[k].abs().max()) > 0, k
        assert torch.equal(got[k], ref[k]), (k, H.rel_err(got[k], ref[k]))
        err = H.rel_err(got[k], fus[k])
        print(mode, which, agg, two_parts, k, f'frozen vs fused trainable {err:.2e}')
        assert err <= TOL_SUM, (k, err)


# ---------------------------------------------------------------------------------------------------------------
# 4. launch census, 7. no residue
# ---------------------------------------------------------------------------------------------------------------
W_IDS = ('wgrad', 'wgrad_node', 'edge_bwd_fused')            # kernel ids 4, 11, 14 (hgn_amd/_lib.py: KERNEL_NAMES)


def _flag_model(data_only=None):
    from hgn_amd import ops
    frame, base = FG._system('flag', 'sum')
    model = copy.deepcopy(base)
    model.zero_grad(set_to_none=True)
    model.learned_model._hgn_ctx = ops.Context(data_only=data_only)
    return frame, model


def _flag_backward(frame, model):
    """loss = mse(update(frame, model(build_graph(frame))), target).backward() under the profiler -> (loss, leaves, census)."""
    from hgn_amd import ops
    fr = FG._leaves(FG._cuda(frame), FG.STATE['flag'], dict(device='cuda', dtype=torch.float32))
    ops.prof_reset(); ops.prof_enable(True)
    try:
        pred = FG._first(model.update(fr, model(model.build_graph(fr, False))))
        loss = torch.nn.functional.mse_loss(pred, fr[FG.TARGET['flag']])
        loss.backward()
        kern = ops.prof_collect()
    finally:
        ops.prof_enable(False)
    c = model.learned_model._hgn_ctx
    assert not any(q[0] for q in c.wq.values()) and not c.redq and not c.lnq, 'queues not empty after backward()'
    return loss.detach(), fr, {k: v['count'] for k, v in kern.items()}


def _n_edge_blocks(model):
    return sum(len(b.edge_models) for b in model.learned_model.processor.graphnet_blocks)


def test_launch_census_of_a_frozen_a_trainable_and_a_partly_frozen_model():
    from hgn_amd import ops
    frame, model = _flag_model()
    params = dict(model.learned_model.named_parameters())
    # trainable control
    ops.bwd_stats.update(data_only=0, full=0)
    loss_t, fr_t, kern_t = _flag_backward(frame, model)
    grads_t = {k: p.grad.clone() for k, p in params.items()}
    assert all(kern_t.get(k, 0) > 0 for k in W_IDS), kern_t
    assert ops.bwd_stats['data_only'] == 0 and ops.bwd_stats['full'] > 0
    # everything frozen
    model.zero_grad(set_to_none=True)
    model.learned_model.requires_grad_(False)
    ops.bwd_stats.update(data_only=0, full=0)
    loss_f, fr_f, kern_f = _flag_backward(frame, model)
    assert all(kern_f.get(k, 0) == 0 for k in W_IDS), kern_f
    assert kern_f.get('mlp_bwd_edge', 0) == _n_edge_blocks(model) == 2, kern_f
    # (an MLP none of whose inputs requires grad -- the edge encoder -- has no backward node at all when it is frozen)
    n_nodes = ops.bwd_stats['data_only']
    assert n_nodes >= 2 + 2 + 2 and ops.bwd_stats['full'] == 0, ops.bwd_stats      # two blocks (edge + node), node encoder, decoder
    assert all(p.grad is None for p in params.values())
    assert torch.equal(loss_f, loss_t)
    for n in FG.STATE['flag']:
        assert H.rel_err(fr_f[n].grad, fr_t[n].grad) <= TOL_SUM, n
    # the same model with the switch off: the trainable census (and still no parameter gradient: nothing requires one)
    model.learned_model._hgn_ctx = ops.Context(data_only=False)
    ops.bwd_stats.update(data_only=0, full=0)
    _, fr_o, kern_o = _flag_backward(frame, model)
    assert all(kern_o.get(k, 0) > 0 for k in W_IDS) and kern_o['edge_bwd_fused'] == kern_t['edge_bwd_fused'], (kern_o, kern_t)
    assert kern_o.get('mlp_bwd_edge', 0) == kern_t.get('mlp_bwd_edge', 0)
    assert ops.bwd_stats == {'data_only': 0, 'full': n_nodes}
    for n in FG.STATE['flag']:
        assert torch.equal(fr_o[n].grad, fr_t[n].grad), n
    # the decoder alone trainable
    model.learned_model._hgn_ctx = ops.Context()
    dec = [k for k in params if k.startswith('decoder')]
    assert len(dec) == 6
    for k in dec:
        params[k].requires_grad_(True)
    ops.bwd_stats.update(data_only=0, full=0)
    _, fr_d, kern_d = _flag_backward(frame, model)
    assert ops.bwd_stats == {'data_only': n_nodes - 1, 'full': 1}, ops.bwd_stats
    assert kern_d.get('edge_bwd_fused', 0) == 0 and kern_d.get('wgrad', 0) + kern_d.get('wgrad_node', 0) >= 1, kern_d
    assert kern_d.get('wgrad', 0) + kern_d.get('wgrad_node', 0) < kern_t['wgrad'] + kern_t['wgrad_node']
    for k, p in params.items():
        assert (p.grad is not None) == (k in dec), k
    for k in dec:
        assert H.rel_err(params[k].grad, grads_t[k]) <= TOL_SUM, k
    for n in FG.STATE['flag']:
        assert H.rel_err(fr_d[n].grad, fr_t[n].grad) <= TOL_SUM, n


def test_frozen_backward_leaves_nothing_behind_for_a_trainable_one():
    """frozen, trainable, frozen on one model and context: the trainable weight gradients are those of a run on a fresh copy of the
    model with a fresh context, bit for bit; the queues are empty after each backward() (_flag_backward asserts it)."""
    frame, fresh = _flag_model()
    _flag_backward(frame, fresh)
    want = {k: p.grad.clone() for k, p in fresh.learned_model.named_parameters()}
    frame, model = _flag_model()
    params = dict(model.learned_model.named_parameters())
    for frozen in (True, False, True):
        model.zero_grad(set_to_none=True)
        model.learned_model.requires_grad_(not frozen)
        _, fr, _ = _flag_backward(frame, model)
        assert all(float(fr[n].grad.abs().max()) > 0 for n in FG.STATE['flag'])
        if frozen:
            assert all(p.grad is None for p in params.values())
        else:
            for k, p in params.items():
                assert torch.equal(p.grad, want[k]), k


# ---------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,agg', [('flag', 'sum'), ('flag', 'pna'), ('cylinder', 'sum')])
def test_input_gradients_of_a_frozen_model_vs_fp64_oracle_and_vs_the_trainable_run(kind, agg):
    """d loss / d world_pos and d prev|world_pos (flag), d velocity (cylinder) of a model whose learned_model is frozen: against the
    fp64 oracle with the HIP forward's gates / winners transferred (test_gpu_feature_grad's bound and helpers), and within 2e-6 of the
    trainable run."""
    frame, base = FG._system(kind, agg)
    grads = {}
    for frozen in (False, True):
        model = copy.deepcopy(base)
        model.zero_grad(set_to_none=True)
        model.learned_model.requires_grad_(not frozen)
        fr = FG._leaves(FG._cuda(frame), FG.STATE[kind], dict(device='cuda', dtype=torch.float32))

        def run():
            pred = FG._first(model.update(fr, model(model.build_graph(fr, False))))
            return torch.nn.functional.mse_loss(pred, fr[FG.TARGET[kind]])
        # (the decisions the oracle takes over are logged on the trainable run: an MLP none of whose inputs requires grad -- the
        #  cylinder's edge encoder -- is no training forward when it is frozen and logs none; the forward bits are the same)
        loss, g_, w_ = FG._logged(model, run)
        if not frozen:
            gates, winners = g_, w_
        loss.backward()
        grads[frozen] = (loss.detach(), {n: fr[n].grad for n in FG.STATE[kind]})
        assert all(p.grad is None for p in model.learned_model.parameters()) == frozen
    ff = FG._oracle_features(kind, model)
    sd = H.oracle_params({k: v.detach().cpu() for k, v in model.learned_model.state_dict().items()})
    fo = FG._leaves(frame, FG.STATE[kind], dict(dtype=torch.float64))
    with H.GateTransfer(gates) as gt, H.WinnerTransfer(winners) as wt:
        g = ff.build_graph(fo, False)
        pred = FG._first(ff.update(fo, O.mesh_graph_net(sd, FO._as_multigraph(g), 'none', agg)))
        loss64 = torch.nn.functional.mse_loss(pred, fo[FG.TARGET[kind]].double())
    assert all(len(v) == 0 for v in gt.gates.values()) and all(len(v) == 0 for v in wt.winners.values()), 'decisions left over'
    loss64.backward()
    assert torch.equal(grads[True][0], grads[False][0]) and H.rel_err(grads[True][0], loss64) <= FG.TOL_GRAD
    for n in FG.STATE[kind]:
        e64, et = H.rel_err(grads[True][1][n], fo[n].grad), H.rel_err(grads[True][1][n], grads[False][1][n])
        print(kind, agg, n, f'frozen vs fp64 {e64:.2e}  vs trainable {et:.2e}')
        assert e64 <= FG.TOL_GRAD and et <= TOL_SUM, (n, e64, et)


def test_unrolled_step_through_the_state_of_a_frozen_model():
    """unrolled_training_step(W = 2, n_steps = 2, through_state=True): loss torch.equal to the trainable run, the gradients of the
    initial state within 2e-6."""
    win = UT._windows('flag', 2, 2)
    out = {}
    for frozen in (False, True):
        model = UT._model('flag')
        model.learned_model.requires_grad_(not frozen)
        wa, la = UT._with_leaves(win, 'flag')
        loss, _ = model.unrolled_training_step(wa, 2, through_state=True, is_training=False)
        loss.backward()
        out[frozen] = (loss.detach(), {n: t.grad for n, t in la.items()})
        assert all(p.grad is None for p in model.learned_model.parameters()) == frozen
    assert torch.equal(out[True][0], out[False][0])
    for n in out[True][1]:
        assert float(out[True][1][n].abs().max()) > 0 and H.rel_err(out[True][1][n], out[False][1][n]) <= TOL_SUM, n


# ---------------------------------------------------------------------------------------------------------------
# 6. memory
# ---------------------------------------------------------------------------------------------------------------
def test_a_frozen_edge_block_holds_two_activation_arrays_less():
    """One edge block at 98 304 rows: while its output is alive, torch.cuda.memory_allocated() is at least 2 x E x 512 bytes lower
    frozen than trainable (z1 and z2)."""
    sd = P._mlp_sd(384, 128, True, seed=4)
    w, wts = P._weights(sd, True)
    held = {}
    _edge_forward(EDGE_ROWS, 'fp32', False, wts, w)           # (packed weight images, topology: allocated once, before the counts)
    for frozen in (False, True):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y, agg, _ = _edge_forward(EDGE_ROWS, 'fp32', frozen, wts, w)
        torch.cuda.synchronize()
        held[frozen] = torch.cuda.memory_allocated() - before
        del y, agg
    _freeze(wts, False)
    print('held while the output is alive: trainable', held[False], 'frozen', held[True])
    assert held[False] - held[True] >= 2 * EDGE_ROWS * 512, held
