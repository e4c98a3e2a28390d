"""The public stage API on the GPU: Encoder / the processor's blocks / Decoder called one at a time on public MultiGraphs, as the
reference composes them (meshgraphnet.py:46-51), and node latents that have consumers outside the block that reads them.

Checker: the fp64 oracle's stage functions (oracle/mgn_oracle.py) on the same state dict.  Metric and bounds are the project's:
helpers.rel_err, outputs <= 1e-5, gradients <= 2e-5.  Every instance (graph, weights, latents) is fixed in this file and was chosen
once from the ORACLE's own conditioning: no ReLU input within 3e-7 of zero, no max / min winner leading by less than 2e-6 -- both are
asserted on the oracle run, before anything is compared.
"""
import pytest
import torch

from oracle import mgn_oracle as O
from tests import helpers as H
from tests import synth

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-5
TOL_GRAD = 2e-5
KINK_MIN = 3e-7          # smallest |ReLU input| of the fp64 run (test_flag_L15_sum_vs_oracle_fp64)
TIE_MIN = 2e-6           # smallest lead of a max / min winner (test_model_vs_oracle)
SHARE_MIN = 0.1          # what the edge blocks, and the outside consumer, each contribute to d(h), of max |d(h)|

ORDER = ['mesh_edges', 'world_edges', 'inter_cluster', 'inter_cluster_world']
ARCHS = [('none', 'sum'), ('none', 'pna'), ('multi', 'sum'), ('repeated', 'sum'), ('hetero', 'pna'), ('hyper', 'pna'), ('multiscale', 'sum')]
ARCH_IDS = [f'{a}-{g}' for a, g in ARCHS]
# weights seed of (a) / weights + latents seed of (b), per architecture: the first that passes the conditioning asserts for every case
SEED_A = {'none-sum': 1, 'none-pna': 2, 'multi-sum': 1, 'repeated-sum': 1, 'hetero-pna': 2, 'hyper-pna': 2, 'multiscale-sum': 2}
SEED_B = {'none-sum': 1, 'none-pna': 2, 'multi-sum': 1, 'repeated-sum': 1, 'hetero-pna': 29, 'hyper-pna': 3, 'multiscale-sum': 2}
R_SCALE = 1.0            # of the outside consumer's weights r in (b): both shares of d(h) >= SHARE_MIN (asserted on the oracle)
R_SCALE_HOOK = 1e-4      # the same for the whole-model case, whose loss is a mean over the outputs


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import hgn_amd
    from hgn_amd import _lib
    _lib.lib()          # the HIP extension must be the thing that runs: fail loudly if it is not built
    yield


# ---------------------------------------------------------------------------------------------------------------
# instances (CPU only: shared by the oracle and the HIP side)
# ---------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _instance(arch, agg, seed):
    """Graph (receivers NOT sorted), weights of a two-block model, target and mask."""
    def make():
        two_part = arch in ('hetero', 'hyper', 'multiscale')
        g = H.with_unsorted_receivers(synth.grid_graph(seed=9, nx=8, ny=7, clusters=4 if two_part else 0), seed=3)
        assert H.receivers_unsorted(g), 'the receiver-sort permutation of some edge set is the identity'
        sets = [e.name for e in g.edge_sets]
        shapes = O.param_shapes(arch, agg, 2, sets, 5, {e.name: e.features.shape[1] for e in g.edge_sets},
                                g.node_features[1].shape[1] if two_part else 0, 3, 128)
        sd = O.init_state_dict_like(shapes, seed=seed)
        N = g.node_features[0].shape[0]
        target = torch.randn(N, 3, generator=torch.Generator().manual_seed(2))
        mask = torch.ones(N, dtype=torch.bool); mask[:3] = False
        return g, sets, sd, target, mask
    return _cached(('instance', arch, agg, seed), make)


def _well_conditioned(km, tm, agg, what):
    assert km.worst > KINK_MIN, (what, 'a ReLU input of the fp64 run within rounding of zero', km.worst)
    assert agg != 'pna' or tm.worst > TIE_MIN, (what, 'a max / min winner of the fp64 run within rounding of its runner-up', tm.worst)


def _model(arch, agg, seed):
    g, sets, sd, _, _ = _instance(arch, agg, seed)
    return _cached(('model', arch, agg, seed), lambda: H.hip_model(arch, agg, 2, sets, sd, set_order=ORDER))


# ---------------------------------------------------------------------------------------------------------------
# (a) the three stages in public, forward and backward
# ---------------------------------------------------------------------------------------------------------------
def oracle_staged(arch, agg):
    seed = SEED_A[f'{arch}-{agg}']
    g, sets, sd, target, mask = _instance(arch, agg, seed)

    def make():
        with H.KinkMargin() as km, H.TieMargin() as tm:
            ref = H.oracle_staged(sd, g, arch, agg, 2, target, mask, set_order=ORDER)
        return ref, km, tm
    return _cached(('staged', arch, agg), make)


def _worst(tid, what, pairs):
    """One report line for the worst of (name, got, exact): -> its norm-wise error."""
    err, name, a, b = max(((H.rel_err(a, b), name, a, b) for name, a, b in pairs), key=lambda t: t[0])
    H.report(tid, f'{what} (worst: {name})', a, b)
    return err


def _check_graph(tid, what, got, exact):
    assert len(got.node_features) == len(exact.node_features)
    assert [e.name for e in got.edge_sets] == [e.name for e in exact.edge_sets]
    for a, b in zip(got.edge_sets, exact.edge_sets):       # rows in the CALLER's order, as the oracle keeps them
        assert torch.equal(a.senders.cpu(), b.senders) and torch.equal(a.receivers.cpu(), b.receivers), (what, a.name)
    pairs = [(f'nodes[{p}]', a, b) for p, (a, b) in enumerate(zip(got.node_features, exact.node_features))]
    pairs += [(a.name, a.features, b.features) for a, b in zip(got.edge_sets, exact.edge_sets)]
    for name, a, b in pairs:
        assert H.rel_err(a, b) <= TOL_OUT, (what, name, H.rel_err(a, b))
    _worst(tid, what, pairs)


@pytest.mark.parametrize('own_context', [True, False], ids=['model_context', 'default_context'])
@pytest.mark.parametrize('arch,agg', ARCHS, ids=ARCH_IDS)
def test_staged_public_forward_backward_vs_oracle(arch, agg, own_context):
    """encoder(graph) -> processor(latent) -> decoder(latent._replace(node_features=latent.node_features[0])), and every block of the
    processor on its own on the public output of the one before: node latents and the edge latents of every set IN THE CALLER'S ROW
    ORDER after every stage, the decoder output, and after the backward pass every parameter and input gradient."""
    import contextlib
    from hgn_amd import ops
    ref, km, tm = oracle_staged(arch, agg)
    _well_conditioned(km, tm, agg, 'staged')
    g, sets, sd, target, mask = _instance(arch, agg, SEED_A[f'{arch}-{agg}'])
    model = _model(arch, agg, SEED_A[f'{arch}-{agg}'])
    tid = f'test_staged_public_forward_backward_vs_oracle[{arch}-{agg}-{"model_context" if own_context else "default_context"}]'
    with (ops.using(model._hgn_ctx) if own_context else contextlib.nullcontext()):
        got = H.hip_staged(model, g, target, mask)
    _check_graph(tid, 'encoder', got['enc'], ref['enc'])
    for i, (a, b) in enumerate(zip(got['blocks'], ref['blocks'])):
        _check_graph(tid, f'block {i}', a, b)
    _check_graph(tid, 'processor', got['blocks_via_processor'], ref['blocks'][-1])
    assert H.report(tid, 'decoder output', got['out'], ref['out'])['norm'] <= TOL_OUT
    assert H.rel_err(got['loss'], ref['loss']) <= TOL_OUT
    live = [k for k in ref['grads'] if float(ref['grads'][k].abs().max()) > 0]
    assert _worst(tid, 'parameter gradients', [(k, got['grads'][k], ref['grads'][k]) for k in live]) <= TOL_GRAD
    for k in ref['grads']:
        if k not in live:
            assert float(got['grads'][k].abs().max()) == 0, k
    ins = [(f'node_features[{p}]', a, b) for p, (a, b) in enumerate(zip(got['in_grads']['node'], ref['in_grads']['node']))]
    ins += [(f'{name}.features', got['in_grads']['edge'][name], b) for name, b in ref['in_grads']['edge'].items()]
    assert all(a is not None for _, a, _ in ins)
    for name, a, b in ins:
        assert H.rel_err(a, b) <= TOL_GRAD, (name, H.rel_err(a, b))
    _worst(tid, 'input gradients', ins)
    # (not asserted: whether the staged path gives the very bits of MeshGraphNet.forward, whose edge latents stay receiver-sorted)
    with (ops.using(model._hgn_ctx) if own_context else contextlib.nullcontext()):
        whole = model(got['graph']).detach()
    H._REPORT.append({'test': tid, 'what': 'staged output bit-equal to model(G)', 'bit_equal': bool(torch.equal(whole, got['out']))})


# ---------------------------------------------------------------------------------------------------------------
# (b), (c) node latents with consumers outside the block
# ---------------------------------------------------------------------------------------------------------------
PATTERNS = ['none', 'before', 'after', 'skip', 'nonleaf', 'two_blocks_same_graph', 'alias', 'chain_tap', 'grad_wrt_intermediate',
            'backward_twice', 'hook_tap']


def _latents(arch, agg):
    """Random 128-wide node and edge latents on the instance's topology, the weights C of f, r and A -- fp32, CPU."""
    seed = SEED_B[f'{arch}-{agg}']
    g, sets, sd, target, mask = _instance(arch, agg, seed)

    def make():
        gen = torch.Generator().manual_seed(100 + seed)
        rn = lambda *s: torch.randn(*s, generator=gen)
        h = [rn(x.shape[0], 128) for x in g.node_features]
        e = [(es.name, rn(es.features.shape[0], 128), es.senders, es.receivers) for es in g.edge_sets]
        C = {'nodes': [rn(x.shape[0], 128) for x in g.node_features], 'edges': {es.name: rn(es.features.shape[0], 128) for es in g.edge_sets}}
        r = [R_SCALE * rn(x.shape[0], 128) for x in g.node_features]
        A = rn(128, 128) / 128 ** 0.5
        return h, e, C, r, A
    return _cached(('latents', arch, agg), make)


def _f(graph, C):
    """A fixed random linear functional plus a square of every row of the graph's node and edge latents."""
    tot = 0
    for x, c in zip(graph.node_features, C['nodes']):
        tot = tot + (x * c).sum() + 0.5 * (x * x).sum()
    for es in graph.edge_sets:
        tot = tot + (es.features * C['edges'][es.name]).sum() + 0.5 * (es.features * es.features).sum()
    return tot


def _expression(pattern, block, g, C, r, A):
    """One expression, evaluated alike by the oracle and by the HIP blocks.  block(i, graph) -> graph; g: leaf latents.
    -> (loss without the outside consumer's term, that term or None, {name: tensor whose gradient is compared}, the tensors an
    outside consumer reads)."""
    h = list(g.node_features)
    leaves = {f'h[{p}]': x for p, x in enumerate(h)}
    leaves.update({f'e[{es.name}]': es.features for es in g.edge_sets})
    dot = lambda xs: sum((x * w).sum() for x, w in zip(xs, r))
    if pattern == 'none':
        return _f(block(0, g), C), None, leaves, h
    if pattern == 'before':
        aux = dot(h)
        return _f(block(0, g), C), aux, leaves, h
    if pattern in ('after', 'backward_twice'):
        out = block(0, g)
        return _f(out, C), dot(h), leaves, h
    if pattern == 'skip':
        out = block(0, g)
        return _f(out._replace(node_features=[o + x for o, x in zip(out.node_features, h)]), C), None, leaves, h
    if pattern == 'nonleaf':
        hs = [x @ A for x in h]                                    # (the leaves are x; the block reads a user's own torch result)
        out = block(0, g._replace(node_features=hs))
        return _f(out, C), dot(hs), leaves, hs
    if pattern == 'two_blocks_same_graph':
        return _f(block(0, g), C) + _f(block(1, g), C), None, leaves, h
    if pattern == 'alias':
        h2 = [x.detach().requires_grad_() for x in h]              # same address, same shape, another autograd tensor
        leaves.update({f'h2[{p}]': x for p, x in enumerate(h2)})
        return _f(block(0, g), C) + _f(block(1, g._replace(node_features=h2)), C), None, leaves, h + h2
    if pattern in ('chain_tap', 'grad_wrt_intermediate'):
        g1 = block(0, g)
        g2 = block(1, g1)
        main = _f(g2, C)
        mid = list(g1.node_features)
        leaves.update({f'g1.nodes[{p}]': x for p, x in enumerate(mid)})
        return main, dot(mid), leaves, mid
    raise KeyError(pattern)


def _block_param_names(sd):
    return [k for k in sd if k.startswith('processor.graphnet_blocks.')]


def oracle_consumers(arch, agg, pattern):
    """fp64 value of every gradient the case compares, and the conditioning of the case: ReLU / tie margins, and how much of d(h)
    comes through the edge blocks and from the outside consumer (each differentiated on its own)."""
    def make():
        seed = SEED_B[f'{arch}-{agg}']
        g, sets, sd, target, mask = _instance(arch, agg, seed)
        h, e, C, r, A = _latents(arch, agg)
        d = lambda t: t.double()
        C64 = {'nodes': [d(c) for c in C['nodes']], 'edges': {k: d(v) for k, v in C['edges'].items()}}
        sd64 = H.oracle_params(sd)
        og = H.oracle_graph(h, e)
        block = lambda i, gr: H.oracle_block(sd64, i, gr, arch, agg, ORDER)
        with H.KinkMargin() as km, H.TieMargin() as tm, H.EdgeShare() as es:
            main, aux, leaves, read = _expression(pattern, block, og, C64, [d(x) for x in r], d(A))
            for t in list(leaves.values()) + read:
                if not t.is_leaf:
                    t.retain_grad()
            loss = main if aux is None else main + aux
            loss.backward(retain_graph=aux is not None)
            total = {id(t): t.grad.detach().clone() for t in list(leaves.values()) + read}
            through_edges = [es.of(t) for t in read]
            # (afterwards, on copies: a second pass would add to the retained gradients of the non-leaf tensors)
            aux_share = torch.autograd.grad(aux, read) if aux is not None else None
        shares = []
        for i, t in enumerate(read):
            top = float(total[id(t)].abs().max())
            shares.append({'edge': float(through_edges[i].abs().max()) / top if through_edges[i] is not None else 0.0,
                           'aux': float(aux_share[i].abs().max()) / top if aux is not None else None})
        times = 2.0 if pattern == 'backward_twice' else 1.0
        grads = {k: times * total[id(t)] for k, t in leaves.items()}
        pg = {k: times * (sd64[k].grad if sd64[k].grad is not None else torch.zeros_like(sd64[k])) for k in _block_param_names(sd)}
        return grads, pg, km, tm, shares
    return _cached(('consumers', arch, agg, pattern), make)


def oracle_hook_tap(arch, agg):
    def make():
        seed = SEED_B[f'{arch}-{agg}']
        g, sets, sd, target, mask = _instance(arch, agg, seed)
        r = R_SCALE_HOOK * torch.randn(g.node_features[0].shape[0], 128, generator=torch.Generator().manual_seed(7)).double()
        sd64 = H.oracle_params(sd)
        g0 = H.oracle_graph(g.node_features, g.edge_sets)
        with H.KinkMargin() as km, H.TieMargin() as tm, H.EdgeShare() as es:
            g1 = H.oracle_block(sd64, 0, O.encoder(sd64, g0, O.BLOCKS.get(arch, (None, False))[1]), arch, agg, ORDER)
            tap = g1.node_features[0]
            tap.retain_grad()
            g2 = H.oracle_block(sd64, 1, g1, arch, agg, ORDER)
            out = O.mlp(sd64, 'decoder.model', g2.node_features[0], layer_norm=False)
            aux = (tap * r).sum()
            loss = O.masked_mse(out, target.double(), mask) + aux
            loss.backward()
        top = float(tap.grad.abs().max())
        shares = [{'edge': float(es.of(tap).abs().max()) / top, 'aux': float(r.abs().max()) / top}]
        return H.param_grads(sd64.items()), km, tm, shares, r
    return _cached(('hook_tap', arch, agg), make)


def _hip_consumers(arch, agg, pattern):
    """The same expression through the model's own blocks, called in public: -> (gradients of the compared tensors, of the blocks' parameters)."""
    seed = SEED_B[f'{arch}-{agg}']
    g, sets, sd, target, mask = _instance(arch, agg, seed)
    h, e, C, r, A = _latents(arch, agg)
    model = _model(arch, agg, seed)
    model.zero_grad(set_to_none=True)
    cu = lambda t: t.cuda()
    Cc = {'nodes': [cu(c) for c in C['nodes']], 'edges': {k: cu(v) for k, v in C['edges'].items()}}
    G = H.hip_graph(h, e)
    blocks = model.processor.graphnet_blocks
    main, aux, leaves, read = _expression(pattern, lambda i, gr: blocks[i](gr), G, Cc, [cu(x) for x in r], cu(A))
    loss = main if aux is None else main + aux
    if pattern == 'grad_wrt_intermediate':
        names = list(leaves)
        got = torch.autograd.grad(loss, [leaves[k] for k in names])
        return dict(zip(names, got)), None
    if pattern == 'backward_twice':
        loss.backward(retain_graph=True)
    loss.backward()
    grads = {k: t.grad for k, t in leaves.items() if t.is_leaf}
    return grads, H.param_grads((k, p) for k, p in model.named_parameters() if k.startswith('processor.graphnet_blocks.'))


def _hip_hook_tap(arch, agg, r):
    seed = SEED_B[f'{arch}-{agg}']
    g, sets, sd, target, mask = _instance(arch, agg, seed)
    model = _model(arch, agg, seed)
    model.zero_grad(set_to_none=True)
    G = H.hip_graph(g.node_features, g.edge_sets)
    kept = {}
    handle = model.processor.graphnet_blocks[0].register_forward_hook(lambda mod, inp, out: kept.__setitem__('tap', out.nodes[0]))
    try:
        out = model(G)
    finally:
        handle.remove()
    aux = (kept['tap'] * r.float().cuda()).sum()                      # formed after the model call
    loss = torch.nn.functional.mse_loss(target.cuda()[mask.cuda()], out[mask.cuda()]) + aux
    loss.backward()
    return H.param_grads(model.named_parameters())


def _assert_shares(shares, what):
    for s in shares:
        assert s['edge'] >= SHARE_MIN, (what, 'the edge blocks contribute too little to d(h) for their loss to show', shares)
        assert s['aux'] is None or s['aux'] >= SHARE_MIN, (what, 'the outside consumer contributes too little to d(h)', shares)


@pytest.mark.parametrize('share', [True, False], ids=['shared', 'not_shared'])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('arch,agg', ARCHS, ids=ARCH_IDS)
def test_node_latent_with_outside_consumers_vs_oracle(arch, agg, pattern, share, monkeypatch):
    """A node latent h that a block reads may be read by anybody else as well -- before or after the block call, by a skip
    connection, by a second block, through an alias of the same address, as an intermediate of a chain that is tapped or
    differentiated with respect to, twice in a row, or by a forward hook inside the whole model.  ops.share_grad lets the edge blocks
    add their share of d(h) into the node update's gradient tensor: with an outside consumer that reports first, an engine that
    sums into a buffer of its own would leave that tensor a dead copy and every edge-block contribution would be lost, silently.
    d(h) of every node part, d(e) of every set and every block parameter gradient against the fp64 oracle evaluating the same
    expression -- with the in-place accumulation on and (ops._SHARE_GRADS = False) off.  On the oracle alone: the edge blocks'
    share and the outside consumer's share of d(h) are each >= 10 % of max |d(h)|, four orders of magnitude above the bound."""
    from hgn_amd import ops
    tid = f'test_node_latent_with_outside_consumers_vs_oracle[{arch}-{agg}-{pattern}-{"shared" if share else "not_shared"}]'
    if pattern == 'hook_tap':
        pg_o, km, tm, shares, r = oracle_hook_tap(arch, agg)
        grads_o = {}
    else:
        grads_o, pg_o, km, tm, shares = oracle_consumers(arch, agg, pattern)
    _well_conditioned(km, tm, agg, pattern)
    _assert_shares(shares, pattern)
    if not share:
        monkeypatch.setattr(ops, '_SHARE_GRADS', False)
    before = dict(ops.share_stats)
    if pattern == 'hook_tap':
        grads, pg = {}, _hip_hook_tap(arch, agg, r)
    else:
        grads, pg = _hip_consumers(arch, agg, pattern)
    acc, own = ops.share_stats['accumulated'] - before['accumulated'], ops.share_stats['own'] - before['own']
    H._REPORT.append({'test': tid, 'what': 'edge-block gradients for node latents', 'accumulated': acc, 'own_tensor': own,
                      'edge_share_of_dh': min(s['edge'] for s in shares),
                      'outside_share_of_dh': min([s['aux'] for s in shares if s['aux'] is not None], default=None)})
    if not share:
        assert acc == 0, acc
    pairs = []
    for k, b in grads_o.items():
        if k in grads:                          # (leaves of the HIP side; the oracle also keeps the non-leaf ones for the shares)
            assert grads[k] is not None, k
            pairs.append((k, grads[k], b))
    if pattern != 'hook_tap':
        assert any(k.startswith('h') for k in grads) and any(k.startswith('e[') for k in grads)
        err = _worst(tid, 'latent gradients', pairs)
        assert err <= TOL_GRAD, [(k, H.rel_err(a, b)) for k, a, b in pairs]
    if pg is not None:
        live = [k for k, b in pg_o.items() if float(b.abs().max()) > 0]
        for k in pg_o:
            if k not in live:
                assert float(pg[k].abs().max()) == 0, k
        err = _worst(tid, 'parameter gradients', [(k, pg[k], pg_o[k]) for k in live])
        assert err <= TOL_GRAD, err


# ---------------------------------------------------------------------------------------------------------------
# (d) the in-place accumulation is still what a captured training step records
# ---------------------------------------------------------------------------------------------------------------
def test_captured_train_step_accumulates_in_place_and_equals_the_eager_step():
    """graphs.GraphedTrainStep on the two-block none / sum model: the edge blocks accumulate into the node updates' gradient tensors
    while the step is captured (ops.share_stats), and the gradients a replay leaves in the flat buffer are those of the eager step
    on the same weights."""
    import hgn_amd
    from hgn_amd import graphs, ops, parallel
    g, sets, sd, target, mask = _instance('none', 'sum', SEED_A['none-sum'])
    G = hgn_amd.MultiGraph([x.cuda() for x in g.node_features],
                           [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in g.edge_sets])
    target, mask = target.cuda(), mask.cuda()
    eager = parallel.DataParallelTrainer(H.hip_model('none', 'sum', 2, sets, sd), lr=1e-3)
    captured = parallel.DataParallelTrainer(H.hip_model('none', 'sum', 2, sets, sd), lr=1e-3, device_step=True)
    seen = []                                                      # (stream capturing?, accumulations) of every step the trainer runs
    step = captured.step

    def counted(*args):
        capturing, n = torch.cuda.is_current_stream_capturing(), ops.share_stats['accumulated']
        res = step(*args)
        seen.append((capturing, ops.share_stats['accumulated'] - n))
        return res
    captured.step = counted
    gs = graphs.GraphedTrainStep(captured, G, target, mask, warmup=1)
    assert [c for c, _ in seen] == [False, True], seen
    assert seen[1][1] > 0 and seen[1][1] == seen[0][1], seen          # accumulated > 0 during capture, as in the eager warm-up
    eager.step(G, target, mask)                                        # the warm-up step; capture itself executes nothing
    before = dict(ops.share_stats)
    l_e = float(eager.step(G, target, mask))
    assert ops.share_stats['accumulated'] - before['accumulated'] == seen[1][1]
    l_g = float(gs())
    torch.cuda.synchronize()
    bit_equal = bool(torch.equal(captured.fp.grad, eager.fp.grad))
    H._REPORT.append({'test': 'test_captured_train_step_accumulates_in_place_and_equals_the_eager_step', 'what': 'replayed flat gradient',
                      'norm': H.rel_err(captured.fp.grad, eager.fp.grad), 'bit_equal': bit_equal, 'accumulated_during_capture': seen[1][1]})
    assert abs(l_e - l_g) <= 1e-6 * abs(l_e)
    assert H.rel_err(captured.fp.grad, eager.fp.grad) <= 1e-6           # (the bound of test_hip_graph_forward_and_train_step_replay)
