"""The four shipped product modes at the THROUGHPUT forms of the matrix-product kernels.

Every product kernel is a template over the product mode and has several forms by row count (csrc/mlp6.hip: launch_mlp6_fwd /
launch_mlp6_bwd and the hgn_linear_*6* entries, csrc/wgrad.hip: wgrad_impl, csrc/fused_bwd.hip: fused_grid): column-split (<= 4 096 rows),
row-per-wave latency form (<= 256 tiles of 64 rows), 64-row throughput form, 128-row form / mlp6_fwd_edge_kernel (>= 98 304 rows, products
3 and 6), the persistent fused edge backward (several tiles per workgroup above 16 384 rows) and the weight-gradient kernel whose
register buffers are refilled inside its loop once a workgroup gets more than two 32-row blocks.  tests/test_gpu_parity.py covers all of
them in the default mode; the other modes ('fp32-bf16x3', 'bf16', 'fp16') ran on graphs of a few thousand rows only.  Here, through
ops.fused_mlp / ops.edge_block / ops.Context / ops.using / ops.set_fused_edge_backward alone and with the mode set per call:

  rows are independent           -> forms agree BIT FOR BIT on the head and on the tail of a launch (outputs, saves, data gradients)
  weight gradients are row sums  -> additive over a row partition within the project's bound for "same products, other summation
                                    order over rows" (2e-6: test_fused_edge_backward_equals_two_launch_backward)
  member graphs of a batch are independent -> an edge block on the batch equals the block on a member alone

and, so that these carry a statement about VALUES, anchors in the small forms: 'fp32-bf16x3' at the default mode's oracle tolerances,
'fp16' against the rounded-operand model of its forward."""
import functools

import pytest
import torch

from tests import helpers as H
from tests import synth
from tests import test_gpu_parity as P      # _mlp_sd / _weights and the test bodies that run again in another mode

pytestmark = pytest.mark.gpu

MODES = ['fp32', 'fp32-bf16x3', 'bf16', 'fp16']
SMALL, MID, BIGS = 1000, 20011, (99000, 99019)      # 20 011: ragged last 64-row tile and 32-row block; 99 019 mod 128 = 75
TOL_SUM = 2e-6                                      # same products, other fp32 summation order over rows
CASES = {'latent_res': ([128], 0), 'node2src': ([128, 128], 0), 'node_pna': ([128, 512], 0), 'encoder7': ([7], -1)}
SAVES = ('z1', 'z2', 'xhat', 'rstd', 'relu bits')
W_NAMES = ('dW1', 'db1', 'dW2', 'db2', 'dW3', 'db3', 'd gamma', 'd beta')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from hgn_amd import _lib
    _lib.lib()          # the HIP extension must be the thing that runs: fail loudly if it is not built
    yield


def _randn(*shape, seed):
    return torch.randn(*shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))


class _RelErrs:
    """Context manager: every figure H.rel_err hands out inside it (the bodies borrowed from test_gpu_parity assert on them
    without returning them) -> .worst, for the parity report."""

    def __enter__(self):
        self.worst, self.n, self._orig = 0.0, 0, H.rel_err

        def rel_err(a, b):
            v = self._orig(a, b)
            self.worst, self.n = max(self.worst, v), self.n + 1
            return v
        H.rel_err = rel_err
        return self

    def __exit__(self, *exc):
        H.rel_err = self._orig
        return False


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2: forms agree on the head and on the tail of a launch, forward and backward data path
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_and_tail(mode, case):
    """ops.fused_mlp forward + backward on M rows for M in (MID, *BIGS), and on rows [0, SMALL) and [M - SMALL, M) as launches
    of their own (column-split form).  -> (names of what differs in the forward, names of what differs in the data gradients);
    only the names are kept, the tensors are released."""
    from hgn_amd import ops
    widths, residual = CASES[case]
    sd = P._mlp_sd(sum(widths), 128, True, seed=5)
    w, _ = P._weights(sd, True)
    top = max(BIGS)
    srcs = [_randn(top, wd, seed=11 + i + len(case)) for i, wd in enumerate(widths)]
    d = _randn(top, 128, seed=7)

    def run(lo, hi):
        xs = [x[lo:hi].clone().requires_grad_(True) for x in srcs]
        y = ops.fused_mlp(xs, w, [None] * len(xs), residual)
        saves = list(y.grad_fn.saves)
        assert len(saves) == len(SAVES) and all(torch.is_tensor(t) and t.shape[0] == hi - lo for t in saves)
        y.backward(d[lo:hi].clone())
        return [y.detach()] + saves, [x.grad for x in xs]

    bad_fwd, bad_bwd = [], []
    with ops.using(ops.Context(precision=mode)):
        head = run(0, SMALL)
        for M in (MID,) + BIGS:
            whole = run(0, M)
            for where, lo, alone in (('head', 0, head), ('tail', M - SMALL, run(M - SMALL, M))):
                for name, a_, b_ in zip(('out',) + SAVES, whole[0], alone[0]):
                    if not torch.equal(a_[lo:lo + SMALL], b_):
                        bad_fwd.append((M, where, name))
                for i, (a_, b_) in enumerate(zip(whole[1], alone[1])):
                    if not torch.equal(a_[lo:lo + SMALL], b_):
                        bad_bwd.append((M, where, f'd source {i}'))
            del whole
    return bad_fwd, bad_bwd


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('mode', MODES)
def test_forward_forms_agree_on_head_and_tail_bit_for_bit(mode, case):
    """The first and the last 1 000 rows of a launch of 20 011 rows (64-row throughput form, ragged last tile), of 99 000 and of 99 019
    rows (products 3 and 6: 128-row workgroups for one-source launches, and for every launch in the six-product mode; the last
    workgroup has a partial first and an empty second sub-tile at 99 000, a full first and a partial second at 99 019; products 1
    and 2: 64-row form) against the same rows as launches of their own (column-split form): output and every saved array -- z1, z2,
    x-hat, 1/sigma, ReLU sign words -- BIT FOR BIT, in every product mode."""
    bad_fwd, _ = _head_and_tail(mode, case)
    assert not bad_fwd, (mode, case, bad_fwd)


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('mode', MODES)
def test_backward_data_path_forms_agree_on_head_and_tail_bit_for_bit(mode, case):
    """The same launches with an upstream gradient: the source gradients of the two slices (64-row throughput form of the backward
    chain above 256 tiles; 'fp16' runs its backward products as the default mode does) equal those of the stand-alone 1 000-row
    launches (column-split form) BIT FOR BIT."""
    _, bad_bwd = _head_and_tail(mode, case)
    assert not bad_bwd, (mode, case, bad_bwd)


# ---------------------------------------------------------------------------------------------------------------
# 3: weight gradients are additive over a row partition
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [MID, BIGS[1]])
@pytest.mark.parametrize('case', ['latent_res', 'node2src'])
@pytest.mark.parametrize('mode', MODES)
def test_weight_gradients_are_additive_over_a_row_partition(mode, case, M):
    """dW1, db1, dW2, db2, dW3, db3 and the LayerNorm d gamma / d beta of ONE launch over M rows (the weight-gradient workgroups take
    more than two 32-row blocks each: the register buffers are refilled inside the loop) against the fp64 sum of the same gradients
    from launches over consecutive parts of 4 096 rows (column-split forward / backward, one or two blocks per weight-gradient
    workgroup; 4 096 is a multiple of 32: the 32-row blocks, and with them the block scales of the scaled modes, are the same in both
    runs).  Saved activations and per-row gradients are equal bit for bit (the two tests above), the operand roundings therefore the
    same: only the fp32 order of the row sum differs -> 2e-6, in every product mode."""
    from hgn_amd import ops
    widths, residual = CASES[case]
    sd = P._mlp_sd(sum(widths), 128, True, seed=5)
    w, wts = P._weights(sd, True)
    srcs = [_randn(M, wd, seed=21 + i) for i, wd in enumerate(widths)]
    d = _randn(M, 128, seed=9)

    def run(lo, hi):
        for t in wts:
            t.grad = None
        xs = [x[lo:hi].clone().requires_grad_(True) for x in srcs]
        ops.fused_mlp(xs, w, [None] * len(xs), residual).backward(d[lo:hi].clone())
        return [t.grad.clone() for t in wts]

    with ops.using(ops.Context(precision=mode)):
        whole = run(0, M)
        parts = [torch.zeros_like(t, dtype=torch.float64) for t in wts]
        for lo in range(0, M, 4096):
            for acc, g in zip(parts, run(lo, min(M, lo + 4096))):
                acc += g.double()
    errs = {n: H.rel_err(a_, b_) for n, a_, b_ in zip(W_NAMES, whole, parts)}
    print(mode, case, M, {n: f'{v:.2e}' for n, v in errs.items()})
    H._REPORT.append({'test': f'test_weight_gradients_are_additive_over_a_row_partition[{mode}-{case}-{M}]',
                      'what': 'one launch against the fp64 sum over parts of 4 096 rows (worst tensor)', 'norm': max(errs.values())})
    assert max(errs.values()) <= TOL_SUM, (mode, case, M, errs)


# ---------------------------------------------------------------------------------------------------------------
# 4: an edge block on a batch of graphs against the block on a member graph alone
# ---------------------------------------------------------------------------------------------------------------
MEMBERS = 11


@functools.lru_cache(maxsize=None)
def _batch():
    """The 11 x (40 x 40) batch of test_training_edge_forward_kernel_equals_the_general_kernel_bit_for_bit: >= 98 304 edge rows, not
    a multiple of 128; 17 600 node rows.  -> (members, batched edge set, N, E, first original edge row of every member)."""
    members = [synth.grid_graph(seed=i % 3, nx=40, ny=40) for i in range(MEMBERS)]
    g = synth.batch(members)
    es = g.edge_sets[0]
    N, E = g.node_features[0].shape[0], es.senders.shape[0]
    assert E >= 98304 and E % 128 != 0 and N > 16384
    first = [0]
    for m in members:
        first.append(first[-1] + m.edge_sets[0].senders.shape[0])
    assert first[-1] == E
    return members, es, N, E, first


def _edge_block_on_batch_and_members(mode, fused, agg_ops):
    """ops.edge_block forward + backward (fixed random cotangents for e' and for the aggregate) on the batch and on every member graph
    alone -- own EdgeTopology, own node rows, own edge rows: about 9 k edges and 1 600 nodes, i.e. the latency and column-split forms --;
    the assertions of item 4 on the first and on the last member, weight gradients over all of them.  -> worst figures."""
    from hgn_amd import ops, topology
    members, es, N, E, first = _batch()
    n1 = N // MEMBERS
    k = len(agg_ops)
    dev = torch.device('cuda')
    sd = P._mlp_sd(384, 128, True, seed=4)
    w, wts = P._weights(sd, True)
    h0 = _randn(N, 128, seed=1)
    e0, r_y = _randn(E, 128, seed=2), _randn(E, 128, seed=3)          # rows in the ORIGINAL edge order of the batch
    r_agg = _randn(N, k * 128, seed=5)

    def run(topo, rows, node_lo, node_hi):
        """`rows`: original edge row of every receiver-sorted row of this launch."""
        for t in wts:
            t.grad = None
        h, e = h0[node_lo:node_hi].clone().requires_grad_(True), e0[rows].requires_grad_(True)
        y, agg = ops.edge_block(h, e, topo, w, agg_ops)
        torch.autograd.backward([y, agg], [r_y[rows], r_agg[node_lo:node_hi].clone()])
        return y.detach(), agg.detach(), h.grad, e.grad, [t.grad.clone() for t in wts]

    ops.set_fused_edge_backward(fused)
    try:
        with ops.using(ops.Context(precision=mode)):
            topo = topology.EdgeTopology(es.senders, es.receivers, N, dev)
            perm = topo.r.perm.long()
            ops.prof_reset(); ops.prof_enable(True)
            try:
                y_b, agg_b, dh_b, de_b, gw_b = run(topo, perm, 0, N)
                kern = ops.prof_collect()
            finally:
                ops.prof_enable(False)
            # the kernels the big launch went through
            assert 'mlp_fwd_edge' in kern and ('edge_bwd_fused' in kern) == fused and ('mlp_bwd_edge' in kern) == (not fused), sorted(kern)
            y_o, de_o = torch.empty_like(y_b), torch.empty_like(de_b)      # back to the original edge order
            y_o[perm] = y_b
            de_o[perm] = de_b
            gw_sum = [torch.zeros_like(t, dtype=torch.float64) for t in wts]
            worst = {'agg': 0.0, 'dh': 0.0}
            for i, m in enumerate(members):
                ms = m.edge_sets[0]
                topo_i = topology.EdgeTopology(ms.senders, ms.receivers, n1, dev)
                rows = first[i] + topo_i.r.perm.long()
                y_i, agg_i, dh_i, de_i, gw_i = run(topo_i, rows, i * n1, (i + 1) * n1)
                for acc, g_ in zip(gw_sum, gw_i):
                    acc += g_.double()
                if i in (0, MEMBERS - 1):
                    assert torch.equal(y_o[rows], y_i), (mode, fused, i, "e'")
                    assert torch.equal(de_o[rows], de_i), (mode, fused, i, 'de')
                    worst['agg'] = max(worst['agg'], H.rel_err(agg_b[i * n1:(i + 1) * n1], agg_i))
                    worst['dh'] = max(worst['dh'], H.rel_err(dh_b[i * n1:(i + 1) * n1], dh_i))
    finally:
        ops.set_fused_edge_backward(None)
    worst['dW'] = max(H.rel_err(a_, b_) for a_, b_ in zip(gw_b, gw_sum))
    per = {n: f'{H.rel_err(a_, b_):.2e}' for n, a_, b_ in zip(W_NAMES, gw_b, gw_sum)}
    print(mode, 'fused' if fused else 'two-launch', agg_ops, worst, per)
    return worst


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two_launch'])
@pytest.mark.parametrize('mode', MODES)
def test_edge_block_on_a_batch_equals_the_block_on_its_member_graphs(mode, fused):
    """Member graphs of a batch share no row: ops.edge_block(..., ('sum',)) on 11 x (40 x 40) (staged pre-projection forms; 128-row edge
    forward kernel for products 3 and 6, 64-row throughput kernel for 1 and 2; about 6 tiles per persistent workgroup of the fused
    backward, the 64-row throughput form of the two-launch one) against the block on the first and on the last member alone (latency and
    column-split forms): e' and de of the member's rows BIT FOR BIT; the aggregate and dh of its nodes within 2e-6 (segment sums may be
    formed elsewhere by form: test_edge_block_fused_segment_sums); every weight gradient additive over the 11 members within 2e-6.

    [bf16-two_launch] is the case that found something.  The two-launch path used to form the receiver sums of dz1 inside the backward
    kernel in every mode (ops.EdgeBlockFn.backward: fuse_seg; csrc/mlp_common.h: a segment that crosses the end of a 64-row tile is
    summed in two parts), and where a tile ends depends on the row offset of the member inside the batch: in 'fp32' these sums differ
    in the last bit in ~380 node rows per member (dh 1.3e-7).  dh and dW1's node columns take them as an OPERAND, which 'bf16' rounds
    to 8 bits; where a last bit moved a rounding -- one node row each in 4 of the 11 members -- dh of that row was off by up to 2.7e-5
    and dW1's receiver columns by 5.04e-6.  In 'bf16' the sums now come from the streaming kernel, which adds in one order wherever
    the tiles end (as the fused path always did)."""
    worst = _edge_block_on_batch_and_members(mode, fused, ('sum',))
    H._REPORT.append({'test': f"test_edge_block_on_a_batch_equals_the_block_on_its_member_graphs[{mode}-{'fused' if fused else 'two_launch'}]",
                      'what': 'batch against member graphs: aggregate, dh, weight gradients (worst tensor)', **worst})
    assert max(worst.values()) <= TOL_SUM, (mode, fused, worst)


def test_pna_edge_block_on_a_batch_equals_the_block_on_its_member_graphs_in_the_six_product_mode():
    """The same with the four pna aggregates in 'fp32-bf16x3' on the two-launch path: the backward kernel that parks d(e') + the
    scattered aggregation backward for the residual gradient (mlp6_bwd_kernel<1, 6, true>), above 256 tiles."""
    worst = _edge_block_on_batch_and_members('fp32-bf16x3', False, ('sum', 'mean', 'max', 'min'))
    H._REPORT.append({'test': 'test_pna_edge_block_on_a_batch_equals_the_block_on_its_member_graphs_in_the_six_product_mode',
                      'what': 'batch against member graphs: aggregate, dh, weight gradients (worst tensor)', **worst})
    assert max(worst.values()) <= TOL_SUM, worst


# ---------------------------------------------------------------------------------------------------------------
# 5: fused against two-launch edge backward in the six-product mode
# ---------------------------------------------------------------------------------------------------------------
class _ModelsIn:
    """Context manager: the models H.hip_model builds launch in an ops.Context of their own with the given precision (a model enters
    its own context for every call, so an ops.using around the call would not reach its launches)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from hgn_amd import ops
        self._orig = H.hip_model

        def hip_model(*a, **kw):
            model = self._orig(*a, **kw)
            model._hgn_ctx = ops.Context(precision=self.mode)
            return model
        H.hip_model = hip_model
        return self

    def __exit__(self, *exc):
        H.hip_model = self._orig
        return False


def test_fused_edge_backward_equals_two_launch_backward_in_the_six_product_mode():
    """The body of test_fused_edge_backward_equals_two_launch_backward[sum-120-100] (71 k edge rows: several tiles per persistent
    workgroup of edge_bwd_fused_kernel<6>) with the model in 'fp32-bf16x3': outputs equal, every gradient within 2e-6, a second run
    bit-identical.  Not asserted for 'bf16': there a last-bit difference between the two paths' fp32 intermediates may move a bf16
    rounding of an operand."""
    with _ModelsIn('fp32-bf16x3'), _RelErrs() as errs:
        P.test_fused_edge_backward_equals_two_launch_backward('sum', 120, 100)
    assert errs.n >= 10
    H._REPORT.append({'test': 'test_fused_edge_backward_equals_two_launch_backward_in_the_six_product_mode',
                      'what': 'fused against two-launch (worst gradient tensor)', 'norm': errs.worst})


# ---------------------------------------------------------------------------------------------------------------
# 6: anchors in the small forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 31, 128, 333])
@pytest.mark.parametrize('case', ['encoder7', 'encoder_idx', 'node2src', 'node_pna', 'decoder3', 'latent_res'])
def test_fused_mlp_vs_oracle_in_the_six_product_mode(M, case):
    """test_fused_mlp_vs_oracle's body, same cases and tolerances (1e-5 outputs, 2e-5 gradients against fp64), in 'fp32-bf16x3'."""
    from hgn_amd import ops
    with ops.using(ops.Context(precision='fp32-bf16x3')), _RelErrs() as errs:
        P.test_fused_mlp_vs_oracle(M, case)
    assert errs.n >= 8
    H._REPORT.append({'test': f'test_fused_mlp_vs_oracle_in_the_six_product_mode[{case}-{M}]', 'what': 'worst tensor against fp64', 'norm': errs.worst})


@pytest.mark.parametrize('nx,ny', [(2, 2), (7, 5), (40, 40)])
def test_edge_block_vs_oracle_in_the_six_product_mode(nx, ny):
    """test_edge_block_vs_oracle's body, same cases and tolerances, in 'fp32-bf16x3'."""
    from hgn_amd import ops
    with ops.using(ops.Context(precision='fp32-bf16x3')), _RelErrs() as errs:
        P.test_edge_block_vs_oracle(nx, ny)
    assert errs.n >= 11
    H._REPORT.append({'test': f'test_edge_block_vs_oracle_in_the_six_product_mode[{nx}-{ny}]', 'what': 'worst tensor against fp64', 'norm': errs.worst})


def round_significant(x: torch.Tensor, bits: int) -> torch.Tensor:
    """x (fp64) rounded to `bits` significant bits, to nearest even, whatever its exponent (through frexp, not through .half(): the
    kernels scale rows and blocks by powers of two before they convert, so fp16's exponent range does not apply)."""
    m, _ = torch.frexp(x)                                      # x = m 2^e, 0.5 <= |m| < 1
    # (every step exact but the rounding: products with a power of two, and x / m = 2^e -- no 2^e from a device's pow())
    scale = float(2 ** bits)
    return torch.where(x == 0, x, torch.round(m * scale) / scale * (x / torch.where(x == 0, torch.ones_like(m), m)))


def rounded_operand_block(P_, topo, h, e, agg, rnd):
    """fp64 evaluation of an edge block + node update (graphnet.py:22-48) whose matrix-product operands -- activations and weights --
    go through `rnd`; bias, LayerNorm and residual exact.  `agg`: the aggregate the node update reads (None: the sum of this
    evaluation's own e').  -> (e', h')"""
    def mlp(x, pre):
        z = torch.relu(rnd(x) @ rnd(P_[pre + '.0.layers.linear_0.weight']).T + P_[pre + '.0.layers.linear_0.bias'])
        z = torch.relu(rnd(z) @ rnd(P_[pre + '.0.layers.linear_1.weight']).T + P_[pre + '.0.layers.linear_1.bias'])
        z = rnd(z) @ rnd(P_[pre + '.0.layers.linear_2.weight']).T + P_[pre + '.0.layers.linear_2.bias']
        return torch.nn.functional.layer_norm(z, (128,), P_[pre + '.1.weight'], P_[pre + '.1.bias'], 1e-5)
    snd, rcv = topo.snd.long(), topo.rcv.long()
    y = e + mlp(torch.cat([h[snd], h[rcv], e], 1), 'edge_models.mesh_edges')
    if agg is None:
        agg = torch.zeros(h.shape[0], 128, dtype=torch.float64, device=h.device).index_add_(0, rcv, y)
    return y, h + mlp(torch.cat([h, agg], 1), 'node_model_cross')


def test_fp16_forward_computes_the_rounded_operand_model():
    """'fp16' runs every forward product as ONE fp16 MFMA on operands scaled by powers of two: 11 significant bits per operand, fp32
    accumulation.  The "computes what it claims" check test_split_bf16_products_are_fp32_accurate (i) makes for 'bf16', on the same
    20 x 20 edge block + node update: the forward against an fp64 evaluation with every matrix-product operand rounded to 11
    significant bits -- mean error <= 2e-5 and max-norm error <= 3e-3 (that test's bounds: a value on a rounding boundary may round
    the other way under fp32 than under fp64 accumulation).  They discriminate: a kernel that rounded to bf16's 8 bits would sit
    near 1e-3 mean against this reference, one that did not round at all near 1e-4.  And against UNROUNDED fp64 the error is at
    least 2e-5: it really is the reduced mode.  (Unlike the scaled two-term mode, this one converts without a scale -- csrc/mlp6_device.h:
    split_np<2>, csrc/mlp6.hip: pack_block --, so an operand below 2^-14, one weight in a thousand here, keeps fewer than 11 bits: part
    of what is measured, 1.6e-6 / 3.2e-6 mean, 1.0e-4 / 2.1e-4 max-norm; 3.3e-4 / 4.2e-4 away from unrounded fp64.)"""
    from hgn_amd import ops, topology, modules
    import hgn_amd
    g = synth.grid_graph(seed=3, nx=20, ny=20)
    es = g.edge_sets[0]
    N, E = g.node_features[0].shape[0], es.senders.shape[0]
    topo = topology.EdgeTopology(es.senders.cuda(), es.receivers.cuda(), N, torch.device('cuda'))
    torch.manual_seed(0)
    m = hgn_amd.MeshGraphNet(3, 128, 2, 'sum', 1, 'none', ['mesh_edges']).cuda()
    with torch.no_grad():
        m(hgn_amd.MultiGraph([g.node_features[0].cuda()], [hgn_amd.EdgeSet(es.name, es.features.cuda(), es.senders.cuda(), es.receivers.cuda())]))
        blk = m.processor.graphnet_blocks[0]
        we = modules.weights_of(blk.edge_models['mesh_edges'], 384)
        wn = modules.weights_of(blk.node_model_cross, 256)
    h0 = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    e0 = torch.randn(E, 128, generator=torch.Generator().manual_seed(2)).cuda()
    with ops.using(ops.Context(precision='fp16')):                 # the training forward, as in that test
        h = h0.clone().requires_grad_(True)
        y, agg = ops.edge_block(h, e0.clone().requires_grad_(True), topo, we, ('sum',))
        hn = ops.fused_mlp([h, agg], wn, None, 0)
    y, hn = y.detach(), hn.detach()
    with torch.no_grad():
        P_ = {n: p.detach().double() for n, p in blk.named_parameters()}
        agg_k = torch.zeros(N, 128, dtype=torch.float64, device='cuda').index_add_(0, topo.rcv.long(), y.double())
        model = rounded_operand_block(P_, topo, h0.double(), e0.double(), agg_k, lambda x: round_significant(x, 11))
        exact = rounded_operand_block(P_, topo, h0.double(), e0.double(), None, lambda x: x)
    rec = {'test': 'test_fp16_forward_computes_the_rounded_operand_model'}
    for name, got, ref, ref_exact in (("e'", y, model[0], exact[0]), ("h'", hn, model[1], exact[1])):
        mean_err = float((got.double() - ref).abs().mean() / ref.abs().mean())
        worst, away = H.rel_err(got, ref), H.rel_err(got, ref_exact)
        rec[name] = {'mean_vs_model': mean_err, 'norm_vs_model': worst, 'norm_vs_unrounded_fp64': away}
        print(name, rec[name])
    H._REPORT.append(rec)
    for name in ("e'", "h'"):
        r = rec[name]
        assert r['mean_vs_model'] <= 2e-5 and r['norm_vs_model'] <= 3e-3, (name, r)
        assert r['norm_vs_unrounded_fp64'] >= 2e-5, (name, r)
