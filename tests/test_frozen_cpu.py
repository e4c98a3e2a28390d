"""Frozen MLPs (no weight tensor requires grad), the host side: the decision rule, the kernel hgn_mlp_fwd picks for an edge-shaped
launch with and without z1 / z2 (hgn_mlp_fwd_edge_form: shapes and pointers only, nothing is launched), the refusals that go with
HGN_F_DATA_ONLY, and the Context switch.  No GPU."""
import ctypes as C
import pickle

import torch

EDGE_ROWS = 98304          # the smallest launch that takes the 128-row forms (csrc/mlp6.hip: FWD128_MIN_ROWS)


def _w(n_ln=2, grad=False):
    shapes = [(128, 128), (128,), (128, 128), (128,), (128, 128), (128,)] + [(128,)] * n_ln
    return [torch.zeros(*s).requires_grad_(grad) for s in shapes]


def test_decision_rule_on_lists_of_tensors():
    from hgn_amd import ops
    x, y = torch.zeros(2, 128).requires_grad_(True), torch.zeros(2, 128)
    for n_ln in (2, 0):
        assert ops.is_frozen([x, y], _w(n_ln))                          # all six / eight frozen, one source requires grad
        assert ops.is_frozen([y, None, x], _w(n_ln))                    # (an edge block without a second node part passes None)
        for i in range(6 + n_ln):                                       # any one trainable tensor -- a bias, a LayerNorm vector --: not frozen
            wt = _w(n_ln)
            wt[i].requires_grad_(True)
            assert not ops.is_frozen([x, y], wt), i
        assert not ops.is_frozen([y, y], _w(n_ln))                      # no source requires grad
        assert not ops.is_frozen([x], _w(n_ln, grad=True))
        with torch.no_grad():
            assert not ops.is_frozen([x, y], _w(n_ln))                  # grad mode off
    assert ops.bwd_stats.keys() == {'data_only', 'full'}


def _edge_args(M, z=(True, True), products=0, flags=0):
    """An edge-shaped hgn_mlp_fwd_t on fabricated 16-byte aligned addresses (nothing reads them)."""
    from hgn_amd import _lib
    a = _lib.MlpFwd()
    p = iter(range(0x10000, 0x100000, 0x1000))
    a.M = M
    a.n_src = 1
    a.src[0].x = next(p); a.src[0].ld = 128; a.src[0].K = 128; a.src[0].W = next(p); a.src[0].Wpk = next(p)
    a.n_add = 2
    for i in range(2):
        a.add[i].P = next(p); a.add[i].ld = 256; a.add[i].idx = next(p)
    a.ldw1 = 384
    a.b1 = next(p); a.W2 = next(p); a.b2 = next(p); a.W3 = next(p); a.b3 = next(p)
    a.W2pk = next(p); a.W3pk = next(p)
    a.out_w = 128
    a.ln_g = next(p); a.ln_b = next(p)
    a.res = next(p); a.ld_res = 128
    a.out = next(p); a.ld_out = 128
    if z[0]:
        a.z1 = next(p)
    if z[1]:
        a.z2 = next(p)
    a.xhat = next(p); a.rstd = next(p); a.relu_bits = next(p)
    a.products, a.flags = products, flags
    return a


def test_edge_form_of_a_forward_launch():
    from hgn_amd import _lib
    form = lambda *a_, **kw: _lib.lib().hgn_mlp_fwd_edge_form(C.byref(_edge_args(*a_, **kw)))
    assert _lib.lib().hgn_get_matmul_products() == 3
    for products in (0, 3, 6):
        assert form(EDGE_ROWS, products=products) == 1                  # both z present: the saving form ...
        assert form(EDGE_ROWS - 1, products=products) == 0              # ... from 98 304 rows on
        assert form(EDGE_ROWS, z=(False, False), products=products) == 2
        assert form(EDGE_ROWS + 19, z=(False, False), products=products) == 2
        assert form(EDGE_ROWS - 1, z=(False, False), products=products) == 0
        assert form(EDGE_ROWS, z=(True, False), products=products) == 0   # exactly one: the general kernel, as before
        assert form(EDGE_ROWS, z=(False, True), products=products) == 0
        for z in ((True, True), (False, False)):
            assert form(EDGE_ROWS, z=z, products=products, flags=_lib.F_GENERAL_FWD) == 0
            assert form(EDGE_ROWS, z=z, products=products, flags=_lib.F_FP32_MFMA) == 0
    for products in (1, 2):                                            # the reduced modes have no edge kernel
        assert form(EDGE_ROWS, products=products) == 0 and form(EDGE_ROWS, z=(False, False), products=products) == 0
    assert form(EDGE_ROWS, products=5) == 0
    assert _lib.lib().hgn_mlp_fwd_edge_form(None) == 0
    # a misaligned z1 only matters when it is there
    a = _edge_args(EDGE_ROWS)
    a.z1 = a.z1 + 4
    assert _lib.lib().hgn_mlp_fwd_edge_form(C.byref(a)) == 0
    a = _edge_args(EDGE_ROWS, z=(False, False))
    a.n_src = 2
    assert _lib.lib().hgn_mlp_fwd_edge_form(C.byref(a)) == 0


def test_data_only_flag_is_refused_where_weight_gradients_are_formed():
    from hgn_amd import _lib
    lib = _lib.lib()
    b = _lib.MlpBwd()
    b.M = 64
    b.flags = _lib.F_DATA_ONLY
    wf = _lib.WFuse()
    assert lib.hgn_edge_bwd_fused_eligible(C.byref(b)) == 0
    assert lib.hgn_edge_bwd_fused(C.byref(b), C.byref(wf), None, 0, None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()
    red = (_lib.WRed * 2)()
    assert lib.hgn_edge_bwd_fused_partial(C.byref(b), C.byref(wf), None, 0, red, None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()
    t = (_lib.WTask * 2)()
    t[1].flags = _lib.F_DATA_ONLY
    assert lib.hgn_mlp_wgrad(t, 2, 64, None, 0, None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()
    assert lib.hgn_mlp_wgrad_partial(t, 2, 64, None, 0, red, None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()
    # hgn_mlp_bwd: dz3 / dz2 must be null with the flag (refused before any launch)
    b.out_w = 128
    b.d_out = 0x1000; b.ld_dout = 128; b.relu_bits = 0x2000; b.W2 = 0x3000; b.W3 = 0x4000
    b.dz3 = 0x5000
    assert lib.hgn_mlp_bwd(C.byref(b), None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()
    b.dz3 = None; b.dz2 = 0x5000
    assert lib.hgn_mlp_bwd(C.byref(b), None) == -1 and b'DATA_ONLY' in lib.hgn_last_error()


def test_context_data_only_switch_travels_in_pickles_and_old_states_load():
    from hgn_amd import ops
    assert ops.Context().data_only is None and ops.Context().skips_frozen() is ops._DEFAULTS['data_only']
    assert ops.Context(data_only=False).skips_frozen() is False and ops.Context(data_only=True).skips_frozen() is True
    for v in (None, False, True):
        c = pickle.loads(pickle.dumps(ops.Context(precision='fp32-bf16x3', data_only=v)))
        assert c.data_only is v and c.precision == 'fp32-bf16x3' and c.wq == {} and c.redq == [] and c.lnq == []
    old = ops.Context.__new__(ops.Context)                              # a state written before the switch existed
    old.__setstate__({'precision': 'bf16', 'fused_edge_bwd': False, 'fp32_mfma': None, 'general_fwd': None})
    assert old.data_only is None and old.skips_frozen() is ops._DEFAULTS['data_only'] and old.precision == 'bf16' and old.fused() is False
