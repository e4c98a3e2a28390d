"""Operand layouts, the part that needs no GPU: what ops._rowmajor takes in place and what it copies (CPU tensors), and the entry
points of the C ABI that read an operand with 16-byte loads refusing a misaligned one before any launch (made-up addresses)."""
import ctypes as C

import pytest
import torch

from tests import view_layouts as V

WIDTHS = (128, 256, 8, 7, 12)


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('layout', V.LAYOUTS)
def test_rowmajor_copies_exactly_what_the_vector_paths_cannot_take(layout, W):
    from hgn_amd import ops
    M = 6
    x = torch.randn(M, W, generator=torch.Generator().manual_seed(W))
    v, buf, pad = V.house(x, layout)
    want = v.detach().float().clone()
    before = buf.clone() if buf is not None else None
    out = ops._rowmajor(v)
    assert out.dtype == torch.float32 and tuple(out.shape) == (M, W)
    assert torch.equal(out, want)                                     # the values, whatever happened to the layout
    assert out.stride(1) == 1 and out.stride(0) >= W                  # what every kernel assumes of every operand
    in_place = out.data_ptr() == v.data_ptr() and out.stride() == v.stride()
    assert in_place == (not V.copied(layout, W)), (layout, W, v.stride(), v.data_ptr() % 16)
    if in_place and v.dtype == torch.float32:
        assert out is v
    if W % 4 == 0:
        assert V.meets_contract(out), (layout, W, out.stride(), out.data_ptr() % 16)
    if buf is not None:                                               # the caller's buffer is never written
        assert torch.equal(torch.isnan(buf), pad) and torch.equal(buf[~pad], before[~pad])


def test_rowmajor_layout_facts_the_table_rests_on():
    """The two layouts of the table that break the contract really do (so that a copy is what makes them safe), and the one-row and
    flat-offset views that torch calls contiguous are copied too."""
    from hgn_amd import ops
    a = torch.zeros(6, 132)[:, 1:129]
    b = torch.zeros(6, 129)[:, :128]
    assert a.data_ptr() % 16 == 4 and a.stride() == (132, 1)
    assert b.data_ptr() % 16 == 0 and ops._ld(b) == 129
    for t in (a, b):
        assert not V.meets_contract(t) and V.meets_contract(ops._rowmajor(t))
    # what autograd makes by itself: the gradient that torch.cat's backward hands the producer of its second input
    g = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 1.0

        @staticmethod
        def backward(ctx, d):
            g['stride'], g['mod'] = d.stride(), d.data_ptr() % 16
            g['fixed'] = V.meets_contract(ops._rowmajor(d))
            return d
    x = torch.zeros(5, 128, requires_grad=True)
    (torch.cat([torch.zeros(5, 3), Probe.apply(x)], 1) * torch.randn(5, 131)).sum().backward()
    assert g == {'stride': (131, 1), 'mod': 12, 'fixed': True}, g
    # torch calls these contiguous: .contiguous() would hand them back as they are
    one_row = torch.zeros(3, 132)[1:2, 1:129]
    flat = torch.zeros(1 + 4 * 128)[1:].view(4, 128)
    for t in (one_row, flat):
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        r = ops._rowmajor(t)
        assert V.meets_contract(r) and torch.equal(r, t)
    # empty operands pass through
    assert ops._rowmajor(torch.zeros(0, 128)).shape == (0, 128)
    with pytest.raises(ValueError):
        ops._rowmajor(torch.zeros(4))


def test_join_hands_both_consumers_of_a_latent_one_aligned_tensor():
    """ops.share_grad / shared_grad key on the address of the latent a block's node update and edge blocks were handed (ops.join):
    a misaligned view is copied ONCE, in the join, so the two still meet in that table; a tensor the kernels can take passes through."""
    from hgn_amd import ops
    buf = torch.randn(6, 132).requires_grad_(True)
    h = buf[:, 1:129]
    a, b = ops.join(h)
    assert a.data_ptr() == b.data_ptr() != h.data_ptr() and V.meets_contract(a) and torch.equal(a, h)
    assert ops._rowmajor(a) is a and ops._rowmajor(b) is b               # neither consumer copies again
    (2 * a + 3 * b).sum().backward()
    assert torch.equal(buf.grad[:, 1:129], torch.full((6, 128), 5.0)) and not bool(buf.grad[:, :1].any()) and not bool(buf.grad[:, 129:].any())
    for h in (torch.randn(6, 128).requires_grad_(True), torch.randn(12, 128).requires_grad_(True)[::2], torch.randn(9, 132).requires_grad_(True)[:6, :128]):
        a, b = ops.join(h)
        assert a.data_ptr() == b.data_ptr() == h.data_ptr() and a.stride() == h.stride()


def test_abi_refuses_misaligned_operands_before_any_launch():
    from hgn_amd import _lib
    lib = _lib.lib()
    host = (C.c_char * 4096)()
    base = (C.addressof(host) + 63) // 64 * 64

    def _fake(nbytes_off=0):
        """A made-up operand address (a host buffer: looked at, never dereferenced -- every call below is refused before a launch)."""
        return C.c_void_p(base + nbytes_off)
    p, odd = _fake(), _fake(4)

    def err():
        return lib.hgn_last_error()
    # ---- hgn_mlp_fwd: the residual is added with 16-byte loads
    def fwd(res, ld_res):
        a = _lib.MlpFwd()
        a.M = 5; a.n_src = 1; a.out_w = 128; a.ldw1 = 128
        a.src[0].x = p; a.src[0].ld = 128; a.src[0].K = 128; a.src[0].W = p
        a.b1 = p; a.W2 = p; a.b2 = p; a.W3 = p; a.b3 = p; a.out = p; a.ld_out = 128
        a.res = res; a.ld_res = ld_res
        return lib.hgn_mlp_fwd(C.byref(a), None)
    assert fwd(odd, 128) == -1 and b'residual must be 16-byte aligned' in err()
    assert fwd(p, 129) == -1 and b'residual must be 16-byte aligned' in err()
    assert fwd(p, 130) == -1 and fwd(_fake(8), 132) == -1
    # ---- hgn_mlp_bwd: a 128-wide d_out is read (and, for a residual source gradient, added) with 16-byte loads: refused, not masked
    def bwd(d_out, ld, residual, packed=False):
        b = _lib.MlpBwd()
        b.M = 5; b.out_w = 128; b.d_out = d_out; b.ld_dout = ld
        b.relu_bits = p; b.W2 = p; b.W3 = p; b.ldw1 = 128; b.dz1 = p
        b.n_dx = 1; b.dx[0].W = p; b.dx[0].K = 128; b.dx[0].dx = p; b.dx[0].ld = 128; b.dx[0].residual = residual
        if packed:              # everything the split-product kernels ask for: the refusal does not depend on which kernel would run
            b.ln_g = p; b.xhat = p; b.rstd = p; b.ln_ws = p; b.d_gamma = p; b.d_beta = p
            b.W3pk_t = p; b.W2pk_t = p; b.dx[0].Wpk_t = p
        if d_out.value % 16 == 0 and ld % 4 == 0:                       # (nothing to refuse: only asked which kernels would take it)
            return None, bool(lib.hgn_mlp_bwd6_eligible(C.byref(b)))
        return lib.hgn_mlp_bwd(C.byref(b), None), bool(lib.hgn_mlp_bwd6_eligible(C.byref(b)))
    for packed in (False, True):
        for residual in (0, 1):
            for d_out, ld in ((odd, 128), (p, 129), (p, 130), (_fake(12), 131), (_fake(8), 128)):
                rc, elig = bwd(d_out, ld, residual, packed)
                assert rc == -1 and b'd_out must be 16-byte aligned' in err(), (packed, residual, ld)
                assert not elig
    assert bwd(p, 128, 1, True)[1] and bwd(p, 132, 1, True)[1]          # (the aligned forms are what the split-product kernels take)
    # ---- the pre-projection of an edge block: hgn_linear_fwd / hgn_linear_fwd6z (and their data gradients)
    wb = (C.c_void_p * 2)(p.value, p.value)
    for x, ldx, out, ld_out in ((odd, 128, p, 256), (p, 129, p, 256), (p, 128, odd, 256), (p, 128, p, 258)):
        assert lib.hgn_linear_fwd(x, ldx, 5, wb, 2, 384, out, ld_out, None) == -1 and b'hgn_linear: bad argument' in err()
        assert lib.hgn_linear_bwd(x, ldx, 5, wb, 2, 384, out, ld_out, None) == -1 and b'hgn_linear: bad argument' in err()
        assert lib.hgn_linear_fwd6z(x, ldx, 5, wb, 2, out, ld_out, None, 0, 0, None) == -1 and b'hgn_linear_fwd6: bad argument' in err()
        assert lib.hgn_linear_bwd6a(x, ldx, 5, wb, 2, out, ld_out, 1, 0, None) == -1 and b'hgn_linear_bwd6: bad argument' in err()
    for zero, ld_zero in ((odd, 128), (p, 130), (p, 64)):
        assert lib.hgn_linear_fwd6z(p, 128, 5, wb, 2, p, 256, zero, ld_zero, 0, None) == -1 and b'hgn_linear_fwd6: bad argument' in err()
    # ---- hgn_segment_reduce_bwd_sorted: gradient rows, base and result rows as float4
    ops1 = (C.c_int32 * 1)(0)
    for d_out, ld_out, base, d_data, ld in ((odd, 128, None, p, 128), (p, 130, None, p, 128), (p, 128, odd, p, 128), (p, 128, None, odd, 128),
                                            (p, 128, p, p, 130), (p, 128, p, p, 64)):
        assert lib.hgn_segment_reduce_bwd_sorted(d_out, ld_out, p, 4, ops1, 1, None, None, base, d_data, ld, None) == -1
        assert b'16-byte aligned' in err()
