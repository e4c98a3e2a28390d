"""`message_passing_aggregator='std'` (graphnet.py:50-70 -> src/util.py:129-130), the parts that need no GPU: the fp32 oracle against
the reference-generated model fixture (tests/golden/gen_golden_std_model.py), and the C ABI of the five-operation segment reduce
(include/hgn_mp.h: hgn_segment_reduce5_*): exports, op codes, argument validation."""
import ctypes as C
import os
import re

import torch

from oracle import mgn_oracle as O
from tests import test_oracle_golden as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'stdagg_none_L2_lat128.pt')
NEW = ('hgn_segment_reduce5_fwd', 'hgn_segment_reduce5_bwd', 'hgn_segment_reduce5_bwd_sorted')


def test_std_model_fixture_is_what_the_issue_names_and_the_oracle_reproduces_it():
    """Architecture `none`, aggregator `std`, 2 steps, `mesh_edges` on an 8 x 6 grid, latent 128; data only; nothing NaN.  The fp32 oracle
    gives the reference's outputs, loss and gradient digests to the bounds of the sibling latent-128 fixtures
    (test_oracle_golden.test_model_matches_reference: outputs rtol 2e-5 / atol 2e-6, loss rtol 1e-5, digests 5e-5 l2 sqrt(n))."""
    fx = torch.load(FIXTURE)
    assert (fx['arch'], fx['agg'], fx['steps'], fx['edge_sets'], fx['latent']) == ('none', 'std', 2, ['mesh_edges'], 128)
    assert fx['graph_kwargs'] == dict(nx=8, ny=6) and fx['weights'] == 'seeded' and 'state_dict' not in fx
    assert os.path.getsize(FIXTURE) < 1 << 20
    name, feats, snd, rcv = fx['graph']['edge_sets'][0]
    assert name == 'mesh_edges' and int(torch.bincount(rcv, minlength=48).min()) >= 2       # every node: a segment with variance
    assert bool(torch.isfinite(fx['out']).all()) and bool(torch.isfinite(fx['loss']))
    assert all(bool(torch.isfinite(g).all()) for g in fx['in_grads']['node'])
    sd = {k: v.requires_grad_(True) for k, v in TG.state_dict_of(fx).items()}
    g = TG.load_graph(fx, requires_grad=True)
    out = O.mesh_graph_net(sd, g, 'none', 'std', set_order=list(fx['set_order']) + list(fx['set_order_hyper']))
    torch.testing.assert_close(out, fx['out'], rtol=2e-5, atol=2e-6)
    loss = O.masked_mse(out, fx['target'], fx['mask'])
    torch.testing.assert_close(loss, fx['loss'], rtol=1e-5, atol=1e-7)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    dg = TG.digest(grads, fx['seed'])
    assert set(dg) == set(fx['grad_digest'])
    # (the LayerNorm bias of the last block's edge model has NO gradient with `std`: a constant added to a column of every edge row moves
    #  no standard deviation.  Reference and oracle both hold rounding noise there: it is held against its sibling's scale instead)
    dead = 'processor.graphnet_blocks.1.edge_models.mesh_edges.1.bias'
    sibling = float(fx['grad_digest'][dead[:-4] + 'weight']['l2'])
    assert float(fx['grad_digest'][dead]['l2']) <= 5e-5 * sibling and float(dg[dead]['l2']) <= 5e-5 * sibling
    for k, ref in fx['grad_digest'].items():
        if k == dead:
            continue
        tol = 5e-5 * float(ref['l2']) * (grads[k].numel() ** 0.5) + 1e-9
        assert float((dg[k]['proj'] - ref['proj']).abs().max()) <= tol, k
        assert abs(float(dg[k]['l2'] - ref['l2'])) <= 1e-4 * float(ref['l2']) + 1e-9, k
    for x, gref in zip(g.node_features, fx['in_grads']['node']):
        torch.testing.assert_close(x.grad, gref, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(g.edge_sets[0].features.grad, fx['in_grads']['edge']['mesh_edges'], rtol=1e-4, atol=1e-6)


def test_std_abi_entries_load_and_op_code():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_mp.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib._SIGS[name][1])
    assert _lib.OP_CODES == {'sum': 0, 'mean': 1, 'max': 2, 'min': 3, 'std': 4}
    assert re.search(r'#define\s+HGN_OP_STD\s+4\b', header)
    # every entry cites the reference lines it replaces
    doc = header[header.index("'std' (src/util.py:129-130"):header.index('int hgn_segment_reduce5_fwd(')]
    assert 'graphnet.py:50-70' in doc and 'src/util.py:116-130' in doc and 'NaN' in doc


def test_std_abi_argument_validation_without_gpu():
    """Nothing here reaches a launch: every call is refused (or is an empty no-op) on the host."""
    from hgn_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 96)()
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)        # an aligned host address: looked at, never dereferenced
    err = lambda: lib.hgn_last_error()

    def fwd5(ops, n=1, N=4):
        return lib.hgn_segment_reduce5_fwd(p, 128, 128, None, p, N, ops, n, p, 128 * n, None, None, None, 256, None)

    def bwd5(ops, n, data, out, mean, E=4):
        return lib.hgn_segment_reduce5_bwd(p, 128 * n, 128, None, p, p, E, ops, n, p, p, None, p, 128, data, 128, out, 128 * n, mean, 256, None)

    def bwd5s(ops, n, data, out, mean, N=4):
        return lib.hgn_segment_reduce5_bwd_sorted(p, 128 * n, p, N, ops, n, p, p, None, p, 128, data, 128, out, 128 * n, mean, 256, None)
    # an unknown op code: old and new entries alike
    bad = (C.c_int32 * 1)(7)
    neg = (C.c_int32 * 2)(4, -1)
    for rc in (lib.hgn_segment_reduce_fwd(None, 128, 128, None, None, 4, bad, 1, None, 128, None, None, None),
               lib.hgn_segment_reduce_bwd(p, 128, 128, None, p, p, 4, bad, 1, None, None, None, p, 128, None),
               lib.hgn_segment_reduce_bwd_sorted(p, 128, p, 4, bad, 1, None, None, None, p, 128, None),
               fwd5(bad), bwd5(bad, 1, p, p, p), bwd5s(bad, 1, p, p, p), fwd5(neg, 2), bwd5(neg, 2, p, p, p)):
        assert rc == -1 and b'Invalid operation type' in err()
    assert fwd5((C.c_int32 * 5)(4, 0, 1, 2, 3), 5) == -1 and b'1..4 ops' in err()
    # code 4 on the four-operation entries: refused, and the message names the entries that serve it
    std, mixed = (C.c_int32 * 1)(4), (C.c_int32 * 2)(0, 4)
    for rc in (lib.hgn_segment_reduce_fwd(p, 128, 128, None, p, 4, std, 1, p, 128, None, None, None),
               lib.hgn_segment_reduce_fwd(p, 128, 128, None, p, 4, mixed, 2, p, 256, None, None, None),
               lib.hgn_segment_reduce_bwd(p, 128, 128, None, p, p, 4, std, 1, None, None, None, p, 128, None),
               lib.hgn_segment_reduce_bwd_sorted(p, 256, p, 4, mixed, 2, None, None, None, p, 128, None)):
        assert rc == -1
        assert b'hgn_segment_reduce5_fwd' in err() and b'hgn_segment_reduce5_bwd' in err() and b'hgn_segment_reduce5_bwd_sorted' in err()
    # a list with 'std' needs data, out and mean in both backward forms
    for ops, n in ((std, 1), (mixed, 2)):
        for miss in range(3):
            args = [p, p, p]
            args[miss] = None
            assert bwd5(ops, n, *args) == -1 and b'data, out and mean' in err() and b'hgn_segment_reduce5_bwd:' in err()
            assert bwd5s(ops, n, *args) == -1 and b'data, out and mean' in err() and b'hgn_segment_reduce5_bwd_sorted:' in err()
    # ... and other bad arguments are refused before that
    assert lib.hgn_segment_reduce5_fwd(p, 128, 128, None, None, 4, std, 1, p, 128, None, None, None, 256, None) == -1 and b'bad argument' in err()
    assert lib.hgn_segment_reduce5_fwd(p, 128, 128, None, p, 4, std, 1, p, 64, None, None, None, 256, None) == -1
    assert lib.hgn_segment_reduce5_fwd(p, 128, 128, None, p, 4, std, 1, p, 128, None, None, p, 128, None) == -1      # mean: two words per column
    assert lib.hgn_segment_reduce5_bwd_sorted(p, 128, p, 4, std, 1, None, None, None, p, 128, p, 128, p, 128, p, 128, None) == -1 and b'leading dimension' in err()
    assert lib.hgn_segment_reduce5_bwd_sorted(p, 128, p, 4, std, 1, None, None, None, p, 130, p, 128, p, 128, p, 256, None) == -1
    assert lib.hgn_segment_reduce5_bwd_sorted(p, 128, p, 4, std, 1, None, None, None, p, 128, p, 130, p, 128, p, 256, None) == -1
    mx = (C.c_int32 * 2)(4, 2)
    assert lib.hgn_segment_reduce5_bwd(p, 256, 128, None, p, p, 4, mx, 2, None, None, None, p, 128, p, 128, p, 256, p, 256, None) == -1
    assert b'arg index' in err()
    # empty problems are no-ops, with or without 'std'
    assert fwd5(std, 1, N=0) == 0 and bwd5(std, 1, None, None, None, E=0) == 0 and bwd5s(mixed, 2, None, None, None, N=0) == 0
    # the struct-driven backward entries take op codes too: they have no room for data / out / mean and say where to go
    b = _lib.MlpBwd()
    b.M = 64; b.out_w = 128; b.ld_dout = 128
    b.agg_dout = p; b.ld_agg = 128; b.n_agg_ops = 1; b.agg_ops[0] = 4; b.agg_seg = p; b.agg_rowptr = p
    b.relu_bits = p; b.W2 = p; b.W3 = p
    assert lib.hgn_mlp_bwd(C.byref(b), None) == -1 and b'hgn_segment_reduce5_bwd_sorted' in err()
    assert lib.hgn_edge_bwd_fused_eligible(C.byref(b)) == 0
    b.agg_ops[0] = 9
    assert lib.hgn_mlp_bwd(C.byref(b), None) == -1 and b'Invalid operation type' in err()
