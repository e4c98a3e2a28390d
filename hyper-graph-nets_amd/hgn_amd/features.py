"""Host wrappers of include/hgn_features.h: the frame -> graph-feature step in front of the message-passing path
(SURVEY.md section 8 rows f2 / f3).  Device tensors in, device tensors out; nothing here falls back to torch math.
"""
import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib, topology
from .ops import _workspace


def _f32_rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 2-D view whose rows are unit-stride (a column slice of a wider row-major tensor is fine)."""
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _ld(t) -> int:
    """Row stride of a 2-D tensor in elements; 0 for an absent (None) one."""
    if t is None:
        return 0
    return t.stride(0) if t.shape[0] > 1 else max(int(t.shape[1]), 1)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ids(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.int64).contiguous()


def _type_column(node_type: torch.Tensor, dev, rows: int):
    """The reference's ``node_type`` ([rows, 1] or [rows]) as int64 on ``dev`` -> (column 0, its stride in elements)."""
    nt = node_type.to(device=dev, dtype=torch.int64)
    if nt.dim() == 2:
        nt = nt[:, 0]
    return nt, (nt.stride(0) if rows > 1 else 1)


def _free_mask(free_types, what: str) -> int:
    """The node types whose rows are free as the bit mask the kernels take (the convention of hgn_rollout_advance)."""
    free_mask = 0
    for t in free_types:
        if not 0 <= int(t) < 32:
            raise ValueError(f'{what}: free node types must lie in [0, 32)')
        free_mask |= 1 << int(t)
    return free_mask


def cells_to_edges(cells: torch.Tensor, deform: bool = False):
    """src/util.py:50-89: -> (senders_two_way, receivers_two_way, n_undirected); int64 device tensors."""
    _lib.require_gpu(cells)
    verts = 4 if deform else 3
    if cells.dim() != 2 or cells.shape[1] < verts:
        raise ValueError(f'cells must be [n_cells, {verts}]')
    cells = cells[:, :verts].to(torch.int64).contiguous()
    F = cells.shape[0]
    dev = cells.device
    L = _lib.lib()
    nb = C.c_size_t(0)
    _lib.check(L.hgn_cells_to_edges_workspace_bytes(F, verts, C.byref(nb)), 'hgn_cells_to_edges_workspace_bytes')
    ws = _workspace(dev, nb.value, 'cells')
    s = torch.empty(2 * verts * F, dtype=torch.int64, device=dev)
    r = torch.empty(2 * verts * F, dtype=torch.int64, device=dev)
    n = C.c_int64(0)
    _lib.check(L.hgn_cells_to_edges(cells.data_ptr(), F, verts, s.data_ptr(), r.data_ptr(), C.byref(n), ws.data_ptr(),
                                    ws.numel(), _lib.stream_ptr()), 'hgn_cells_to_edges')
    return s[:2 * n.value], r[:2 * n.value], n.value


def _needs_grad(*tensors) -> bool:
    """Whether a call has to become an autograd node: grad mode on and a floating input that requires grad.  Otherwise the
    wrappers below launch exactly what they launched before they could be differentiated."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.is_floating_point() and t.requires_grad for t in tensors)


def _like(grad, ref: torch.Tensor):
    """A gradient in the shape, dtype and place of the input it belongs to."""
    return None if grad is None else grad.reshape(ref.shape).to(device=ref.device, dtype=ref.dtype)


def rel_edge_features_bwd(d_feat, d_len, a: torch.Tensor, b, senders: torch.Tensor, receivers: torch.Tensor,
                          want_a: bool = True, want_b: bool = True):
    """Gradient of rel_edge_features with respect to ``a`` / ``b`` (hgn_rel_edge_features_bwd): node-parallel over the CSRs of
    the edges by sender and by receiver (topology.segment_csr: cached on the id tensors), no atomics, deterministic.
    ``d_feat`` [E, W] and ``d_len`` [E] may each be None.  -> (d_a or None, d_b or None)."""
    _lib.require_gpu(a)
    dev = a.device
    a = _f32_rows(a)
    N, da = a.shape
    db = 0
    if b is not None:
        b = _f32_rows(b.to(dev))
        db = b.shape[1]
        if b.shape[0] != N:
            raise ValueError('a and b must have the same number of rows')
    want_b = want_b and db > 0
    s, r = _ids(senders, dev), _ids(receivers, dev)
    E = s.shape[0]
    if r.shape[0] != E:
        raise ValueError('senders / receivers length mismatch')
    W = da + 1 + (db + 1 if db else 0)
    if d_feat is not None:
        d_feat = _f32_rows(d_feat.to(dev))
        if tuple(d_feat.shape) != (E, W):
            raise ValueError(f'd_feat must be [{E}, {W}]')
    if d_len is not None:
        d_len = d_len.to(dev).float().reshape(-1).contiguous()
        if d_len.shape[0] != E:
            raise ValueError(f'd_len must be [{E}]')
    d_a = torch.empty(N, da, dtype=torch.float32, device=dev) if want_a else None
    d_b = torch.empty(N, db, dtype=torch.float32, device=dev) if want_b else None
    cs = cr = None
    if E > 0:
        cs, cr = topology.segment_csr(s, N, dev), topology.segment_csr(r, N, dev)
    _lib.check(_lib.lib().hgn_rel_edge_features_bwd(
        _ptr(d_feat), _ld(d_feat), _ptr(d_len), a.data_ptr(), _ld(a), da,
        b.data_ptr() if db else None, _ld(b) if db else 0, db, N, s.data_ptr(), r.data_ptr(), E,
        _ptr(cs.rowptr) if cs else None, _ptr(cs.perm) if cs else None, _ptr(cr.rowptr) if cr else None,
        _ptr(cr.perm) if cr else None, cs.max_rows + cr.max_rows if cs else 0, _ptr(d_a), _ptr(d_b), _lib.stream_ptr()),
        'hgn_rel_edge_features_bwd')
    return d_a, d_b


class _RelEdgeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, senders, receivers, want_feat, want_len):
        ctx.set_materialize_grads(False)
        feat, ln = rel_edge_features(a.detach(), b.detach() if b is not None else None, senders, receivers, want_feat, want_len)
        ctx.ids = (senders, receivers)
        ctx.has_b = b is not None
        ctx.save_for_backward(a, *([b] if b is not None else []))
        return feat, ln

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_feat, d_len):
        a = ctx.saved_tensors[0]
        b = ctx.saved_tensors[1] if ctx.has_b else None
        want_a, want_b = ctx.needs_input_grad[0], ctx.has_b and ctx.needs_input_grad[1]
        d_a, d_b = rel_edge_features_bwd(d_feat, d_len, a, b, *ctx.ids, want_a=want_a, want_b=want_b)
        return _like(d_a, a), (_like(d_b, b) if d_b is not None else None), None, None, None, None


def rel_edge_features(a: torch.Tensor, b, senders: torch.Tensor, receivers: torch.Tensor, want_feat: bool = True,
                      want_len: bool = False):
    """[a[s]-a[r], |.|, b[s]-b[r], |.|] per edge (b may be None) and/or the length |a[s]-a[r]|.  Differentiable with
    respect to ``a`` and ``b``."""
    _lib.require_gpu(a)
    if _needs_grad(a, b):
        return _RelEdgeFn.apply(a, b, senders, receivers, want_feat, want_len)
    dev = a.device
    a = _f32_rows(a)
    da = a.shape[1]
    db = 0
    if b is not None:
        b = _f32_rows(b.to(dev))
        db = b.shape[1]
        if b.shape[0] != a.shape[0]:
            raise ValueError('a and b must have the same number of rows')
    s, r = _ids(senders, dev), _ids(receivers, dev)
    E = s.shape[0]
    if r.shape[0] != E:
        raise ValueError('senders / receivers length mismatch')
    W = da + 1 + (db + 1 if db else 0)
    feat = torch.empty(E, W, dtype=torch.float32, device=dev) if want_feat else None
    ln = torch.empty(E, dtype=torch.float32, device=dev) if want_len else None
    _lib.check(_lib.lib().hgn_rel_edge_features(
        a.data_ptr(), _ld(a), da, b.data_ptr() if db else None, _ld(b) if db else 0, db, a.shape[0], s.data_ptr(),
        r.data_ptr(), E, feat.data_ptr() if want_feat else None, W, ln.data_ptr() if want_len else None,
        _lib.stream_ptr()), 'hgn_rel_edge_features')
    return feat, ln


_map_cache = {}


def _class_map(mapping, dev):
    if mapping is None:
        return None
    key = (tuple(mapping), dev.type, dev.index)
    t = _map_cache.get(key)
    if t is None:
        t = torch.tensor(list(mapping), dtype=torch.int32, device=dev)
        _map_cache[key] = t
    return t


class _NodeFeaturesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cur, prev, node_type, mapping, n_classes, vel_first, vel_mask_type, d):
        out = node_features(cur.detach() if cur is not None else None, prev.detach() if prev is not None else None, node_type,
                            mapping, n_classes, vel_first, vel_mask_type, d)
        ctx.cfg = (node_type, n_classes, vel_first, vel_mask_type, cur, prev)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        node_type, n_classes, vel_first, vel_mask_type, cur, prev = ctx.cfg
        dev = d_out.device
        d_out = _f32_rows(d_out)
        N = d_out.shape[0]
        d = d_out.shape[1] - n_classes
        nt, ldt = _type_column(node_type, dev, N)
        d_cur = torch.empty(N, d, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        d_prev = torch.empty(N, d, dtype=torch.float32, device=dev) if prev is not None and ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().hgn_node_features_bwd(
            d_out.data_ptr(), _ld(d_out), d, n_classes, 1 if vel_first else 0, nt.data_ptr(), ldt, vel_mask_type, N,
            d_cur.data_ptr() if d_cur is not None else None, d_prev.data_ptr() if d_prev is not None else None,
            _lib.stream_ptr()), 'hgn_node_features_bwd')
        return (_like(d_cur, cur) if d_cur is not None else None, _like(d_prev, prev) if d_prev is not None else None,
                None, None, None, None, None, None)


def node_features(cur, prev, node_type: torch.Tensor, mapping, n_classes: int, vel_first: bool = True,
                  vel_mask_type: int = -1, d: int = None) -> torch.Tensor:
    """[velocity | one-hot(class)] (or [one-hot | velocity]); ``node_type`` is the reference's [N, 1] (or [N]) tensor,
    ``mapping`` an optional tuple raw type -> class.  Differentiable with respect to ``cur`` and ``prev``."""
    _lib.require_gpu(node_type)
    if _needs_grad(cur, prev):
        return _NodeFeaturesFn.apply(cur, prev, node_type, mapping, n_classes, vel_first, vel_mask_type, d)
    dev = node_type.device
    N = node_type.shape[0]
    nt, ldt = _type_column(node_type, dev, N)
    if cur is not None:
        cur = _f32_rows(cur.to(dev))
        d = cur.shape[1]
        ld = _ld(cur)
        if prev is not None:
            prev = _f32_rows(prev.to(dev))
            if prev.shape != cur.shape:
                raise ValueError('cur / prev shape mismatch')
            if _ld(prev) != ld:
                cur, prev = cur.contiguous(), prev.contiguous()
                ld = _ld(cur)
    else:
        ld = d = int(d or 0)
    m = _class_map(mapping, dev)
    out = torch.empty(N, d + n_classes, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().hgn_node_features(
        cur.data_ptr() if cur is not None else None, prev.data_ptr() if prev is not None else None, ld, d,
        nt.data_ptr(), ldt, m.data_ptr() if m is not None else None, len(mapping) if mapping is not None else 0,
        n_classes, 1 if vel_first else 0, vel_mask_type, N, out.data_ptr(), d + n_classes, _lib.stream_ptr()),
        'hgn_node_features')
    return out


def col_stats(x: torch.Tensor) -> torch.Tensor:
    """-> device [2F]: column sums then column sums of squares (fp64 accumulation, deterministic)."""
    _lib.require_gpu(x)
    x = x.reshape(x.shape[0], -1) if x.dim() != 2 else x
    x = x.float().contiguous()
    rows, F = x.shape
    L = _lib.lib()
    nb = C.c_size_t(0)
    _lib.check(L.hgn_col_stats_workspace_bytes(rows, F, C.byref(nb)), 'hgn_col_stats_workspace_bytes')
    ws = _workspace(x.device, nb.value, 'stats')
    batch = torch.empty(2 * F, dtype=torch.float32, device=x.device)
    _lib.check(L.hgn_col_stats(x.data_ptr(), rows, F, batch.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'hgn_col_stats')
    return batch


def normalizer_update(acc_sum, acc_sumsq, acc_count, num_acc, batch, count, max_acc: float) -> None:
    _lib.require_gpu(acc_sum)
    F = acc_sum.numel()
    _lib.check(_lib.lib().hgn_normalizer_update(acc_sum.data_ptr(), acc_sumsq.data_ptr(), acc_count.data_ptr(),
                                                num_acc.data_ptr(), batch.data_ptr(), count.data_ptr(), F,
                                                float(max_acc), _lib.stream_ptr()), 'hgn_normalizer_update')


class _NormalizeFn(torch.autograd.Function):
    """The running statistics are constants: the gradient goes to ``x`` alone.  They are updated in place by later
    accumulations, so the backward pass uses the values this forward call normalised with (three tiny copies)."""

    @staticmethod
    def forward(ctx, x, acc_sum, acc_sumsq, acc_count, eps, inverse):
        out = normalize(x.detach(), acc_sum, acc_sumsq, acc_count, eps, inverse)
        ctx.cfg = (eps, inverse, x)
        ctx.save_for_backward(acc_sum.detach().clone(), acc_sumsq.detach().clone(), acc_count.detach().clone())
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        eps, inverse, x = ctx.cfg
        acc_sum, acc_sumsq, acc_count = ctx.saved_tensors
        F = acc_sum.numel()
        g = d_out.float().contiguous()
        d_x = torch.empty_like(g)
        _lib.check(_lib.lib().hgn_normalize_bwd(g.data_ptr(), g.numel() // F, F, acc_sum.data_ptr(), acc_sumsq.data_ptr(),
                                                acc_count.data_ptr(), float(eps), 1 if inverse else 0, d_x.data_ptr(),
                                                _lib.stream_ptr()), 'hgn_normalize_bwd')
        return _like(d_x, x), None, None, None, None, None


def normalize(x: torch.Tensor, acc_sum, acc_sumsq, acc_count, eps: float, inverse: bool = False) -> torch.Tensor:
    """(x - mean) / std, or x * std + mean (``inverse``).  Differentiable with respect to ``x``; the statistics are constants."""
    _lib.require_gpu(x)
    if _needs_grad(x):
        return _NormalizeFn.apply(x, acc_sum, acc_sumsq, acc_count, eps, inverse)
    shape = x.shape
    F = acc_sum.numel()
    if x.dim() == 0 or shape[-1] != F and not (F == 1):
        raise ValueError(f'last dimension {tuple(shape)} does not match the normaliser width {F}')
    xf = x.float().contiguous()
    rows = xf.numel() // F
    out = torch.empty_like(xf)
    _lib.check(_lib.lib().hgn_normalize(xf.data_ptr(), rows, F, acc_sum.data_ptr(), acc_sumsq.data_ptr(),
                                        acc_count.data_ptr(), float(eps), 1 if inverse else 0, out.data_ptr(),
                                        _lib.stream_ptr()), 'hgn_normalize')
    return out


class _Lincomb3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, ca, b, cb, c, cc):
        ctx.cfg = (ca, cb, cc, a, b, c)
        return lincomb3(a.detach(), ca, b.detach(), cb, c.detach() if c is not None else None, cc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ca, cb, cc, a, b, c = ctx.cfg
        scaled = lambda k, ref: _like(g if k == 1.0 else g * k, ref)          # three scalings, no kernel of its own
        return (scaled(ca, a) if ctx.needs_input_grad[0] else None, None, scaled(cb, b) if ctx.needs_input_grad[2] else None, None,
                scaled(cc, c) if c is not None and ctx.needs_input_grad[4] else None, None)


def lincomb3(a: torch.Tensor, ca: float, b: torch.Tensor, cb: float, c=None, cc: float = 0.0) -> torch.Tensor:
    """(ca*a + cb*b) + cc*c, every product / sum rounded on its own (the reference's left-to-right fp32 order).  Differentiable with
    respect to ``a``, ``b`` and ``c``."""
    _lib.require_gpu(a)
    if _needs_grad(a, b, c):
        return _Lincomb3Fn.apply(a, float(ca), b, float(cb), c, float(cc))
    dev = a.device
    a = a.float().contiguous()
    b = b.to(dev).float().contiguous()
    if b.shape != a.shape:
        raise ValueError('lincomb3: shape mismatch')
    if c is not None:
        c = c.to(dev).float().contiguous()
        if c.shape != a.shape:
            raise ValueError('lincomb3: shape mismatch')
    out = torch.empty_like(a)
    _lib.check(_lib.lib().hgn_lincomb3(a.data_ptr(), float(ca), b.data_ptr(), float(cb),
                                       c.data_ptr() if c is not None else None, float(cc), a.numel(), out.data_ptr(),
                                       _lib.stream_ptr()), 'hgn_lincomb3')
    return out


def _out_rows(t: torch.Tensor, rows: int, width: int, what: str) -> torch.Tensor:
    """An output of rollout_advance is written in place: fp32 [rows, width] on the device with unit-stride rows, or an error (a
    copy would swallow the result)."""
    if (t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (rows, width) or not t.is_cuda
            or (width > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < width)):
        raise ValueError(f'rollout_advance: {what} must be a float32 device tensor [{rows}, {width}] with unit-stride rows')
    return t


def rollout_advance(net_out: torch.Tensor, normalizer, cur: torch.Tensor, d: int, ca: float, prev, cp: float,
                    node_type: torch.Tensor, free_types, fallback, next_out: torch.Tensor, rec=None, rec_before: bool = False,
                    prev_out=None, inv_out=None, inv_from: int = 0) -> torch.Tensor:
    """One rollout step's state update in one launch (hgn_rollout_advance; flag.py:169-180,243, cylinder.py:155-165,
    plate.py:246-257,328): ``normalizer.inverse(net_out)``, the integration ``ca*cur + out[:, :d] + cp*prev`` (``prev`` may be
    None), and per row the choice between the integrated value (node types listed in ``free_types``) and ``fallback`` (None: ``cur``).
    Bit-identical to Normalizer.inverse -> lincomb3 -> torch.where.  Written in place: ``next_out`` [rows, d]; ``rec`` (the slice of
    the recorded trajectory: the state before the step if ``rec_before``, else the new one); ``prev_out`` (receives ``cur``);
    ``inv_out`` [rows, F - inv_from] (the inverse-normalised columns from ``inv_from`` on).  Outputs may be column slices of wider
    slabs; they must not overlap the inputs.  -> ``next_out``."""
    _lib.require_gpu(net_out)
    dev = net_out.device
    x = _f32_rows(net_out)
    rows, cols = x.shape
    F = normalizer._acc_sum.numel()
    d = int(d)
    cur = _f32_rows(cur.to(dev))
    if cur.shape[0] != rows or cur.shape[1] != d:
        raise ValueError(f'rollout_advance: cur must be [{rows}, {d}]')
    if prev is not None:
        prev = _f32_rows(prev.to(dev))
        if prev.shape != cur.shape:
            raise ValueError('rollout_advance: cur / prev shape mismatch')
    if fallback is not None:
        fallback = _f32_rows(fallback.to(dev))
        if fallback.shape != cur.shape:
            raise ValueError('rollout_advance: cur / fallback shape mismatch')
    nt, ldt = _type_column(node_type, dev, rows)
    if nt.shape[0] != rows:
        raise ValueError(f'rollout_advance: {nt.shape[0]} node types for {rows} rows')
    free_mask = _free_mask(free_types, 'rollout_advance')
    _out_rows(next_out, rows, d, 'next_out')
    if rec is not None:
        _out_rows(rec, rows, d, 'rec')
    if prev_out is not None:
        _out_rows(prev_out, rows, d, 'prev_out')
    if inv_out is not None:
        _out_rows(inv_out, rows, F - int(inv_from), 'inv_out')
    _lib.check(_lib.lib().hgn_rollout_advance(
        x.data_ptr(), _ld(x), cols, F, normalizer._acc_sum.data_ptr(), normalizer._acc_sum_squared.data_ptr(),
        normalizer._acc_count.data_ptr(), float(normalizer._eps), cur.data_ptr(), _ld(cur), d, float(ca), _ptr(prev), _ld(prev),
        float(cp), nt.data_ptr(), ldt, free_mask, _ptr(fallback), _ld(fallback), rows, next_out.data_ptr(), _ld(next_out),
        _ptr(rec), _ld(rec), 1 if rec_before else 0, _ptr(prev_out), _ld(prev_out), _ptr(inv_out), _ld(inv_out), int(inv_from),
        _lib.stream_ptr()), 'hgn_rollout_advance')
    return next_out


def _advance_into_fresh(net_out, normalizer, cur, d, ca, prev, cp, node_type, free_types, fallback, inv_from):
    rows, F = _f32_rows(net_out).shape[0], normalizer._acc_sum.numel()
    nxt = torch.empty(rows, d, dtype=torch.float32, device=net_out.device)
    inv = torch.empty(rows, F - int(inv_from), dtype=torch.float32, device=net_out.device) if inv_from is not None else None
    rollout_advance(net_out, normalizer, cur, d, ca, prev, cp, node_type, free_types, fallback, nxt, inv_out=inv,
                    inv_from=int(inv_from or 0))
    return nxt, inv


class _AdvanceStateFn(torch.autograd.Function):
    """The statistics are constants, and later accumulations update them in place: the backward pass uses the values this forward
    call normalised with (three tiny copies, as in _NormalizeFn)."""

    @staticmethod
    def forward(ctx, net_out, cur, prev, fallback, normalizer, d, ca, cp, node_type, free_types, inv_from):
        ctx.set_materialize_grads(False)
        det = lambda t: t.detach() if t is not None else None
        nxt, inv = _advance_into_fresh(net_out.detach(), normalizer, cur.detach(), d, ca, det(prev), cp, node_type, free_types,
                                       det(fallback), inv_from)
        ctx.cfg = (float(normalizer._eps), d, ca, cp, _type_column(node_type, net_out.device, nxt.shape[0]),
                   sum(1 << int(t) for t in set(free_types)), int(inv_from or 0), net_out, cur, prev, fallback)
        ctx.save_for_backward(normalizer._acc_sum.detach().clone(), normalizer._acc_sum_squared.detach().clone(),
                              normalizer._acc_count.detach().clone())
        return nxt, inv

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_next, d_inv):
        eps, d, ca, cp, (nt, ldt), free_mask, inv_from, net_out, cur, prev, fallback = ctx.cfg
        acc_sum, acc_sumsq, acc_count = ctx.saved_tensors
        dev, F, rows = acc_sum.device, acc_sum.numel(), nt.shape[0]
        g = _f32_rows(d_next.to(dev)) if d_next is not None else None         # an incoming gradient may have any stride
        h = _f32_rows(d_inv.to(dev)) if d_inv is not None else None
        want = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], prev is not None and ctx.needs_input_grad[2],
                fallback is not None and ctx.needs_input_grad[3]]
        outs = [torch.empty(rows, w, dtype=torch.float32, device=dev) if need else None for need, w in zip(want, (F, d, d, d))]
        if any(want):
            _lib.check(_lib.lib().hgn_rollout_advance_bwd(
                _ptr(g), _ld(g), _ptr(h), _ld(h), inv_from, F, acc_sum.data_ptr(), acc_sumsq.data_ptr(), acc_count.data_ptr(), eps, d,
                ca, cp, nt.data_ptr(), ldt, free_mask, 1 if fallback is not None else 0, rows,
                _ptr(outs[0]), _ld(outs[0]), _ptr(outs[1]), _ld(outs[1]), _ptr(outs[2]), _ld(outs[2]), _ptr(outs[3]), _ld(outs[3]),
                _lib.stream_ptr()), 'hgn_rollout_advance_bwd')
        refs = (net_out, cur, prev, fallback)
        return tuple(_like(o, r) if o is not None else None for o, r in zip(outs, refs)) + (None,) * 7


def advance_state(net_out: torch.Tensor, normalizer, cur: torch.Tensor, d: int, ca: float, prev, cp: float,
                  node_type: torch.Tensor, free_types, fallback=None, inv_from=None):
    """``rollout_advance`` as a function: the same one launch (hgn_rollout_advance, hence the bits of Normalizer.inverse -> lincomb3
    -> torch.where) written into fresh tensors.  -> (next [rows, d], the inverse-normalised columns from ``inv_from`` on
    [rows, F - inv_from], or None when ``inv_from`` is None).  Differentiable with respect to ``net_out``, ``cur``, ``prev`` and
    ``fallback`` in one launch of its own (hgn_rollout_advance_bwd); the normaliser's statistics are constants."""
    _lib.require_gpu(net_out)
    d, ca, cp = int(d), float(ca), float(cp)
    if _needs_grad(net_out, cur, prev, fallback):
        return _AdvanceStateFn.apply(net_out, cur, prev, fallback, normalizer, d, ca, cp, node_type, tuple(free_types), inv_from)
    return _advance_into_fresh(net_out, normalizer, cur, d, ca, prev, cp, node_type, free_types, fallback, inv_from)


_frame_ptr_cache = {}
_FRAME_PTR_CACHE_SIZE = 64


class _Ragged(NamedTuple):
    """A ragged batch as the C ABI takes it: B, the frame sizes as a host int64 array, their exclusive prefix as a device int32 [B+1]."""
    B: int
    host: object
    ptr: torch.Tensor


def _ragged(frame_rows, rows: int, dev, what: str) -> _Ragged:
    """``frame_rows`` (a sequence of ints, every one >= 1, summing to ``rows``) -> _Ragged; the device prefix is built once per distinct
    tuple and device and kept in a small cache (the oldest entry leaves when it is full)."""
    sizes = tuple(int(n) for n in frame_rows)
    if not sizes or min(sizes) < 1 or sum(sizes) != rows:
        raise ValueError(f'{what}: frame_rows must be a non-empty sequence of row counts >= 1 that sum to the {rows} rows given, '
                         f'got {len(sizes)} frames with {sum(sizes)} rows')
    if rows >= 1 << 31:
        raise ValueError(f'{what}: {rows} rows do not fit the int32 frame_ptr')
    key = (sizes, dev.type, dev.index)
    hit = _frame_ptr_cache.get(key)
    if hit is None:
        prefix = [0]
        for n in sizes:
            prefix.append(prefix[-1] + n)
        hit = _Ragged(len(sizes), (C.c_int64 * len(sizes))(*sizes), torch.tensor(prefix, dtype=torch.int32, device=dev))
        if len(_frame_ptr_cache) >= _FRAME_PTR_CACHE_SIZE:
            _frame_ptr_cache.pop(next(iter(_frame_ptr_cache)))
        _frame_ptr_cache[key] = hit
    return hit


def _one_split(what: str, rows_per_frame, frame_rows) -> None:
    if rows_per_frame is not None and frame_rows is not None:
        raise ValueError(f'{what}: give rows_per_frame (frames of equal size) or frame_rows (a ragged batch), not both')


def _frame_ids_tensor(frame_ids, n_frames: int, dev):
    """ids travel as int64 and are read modulo 2^32; a Python int up to 2^64 - 1 keeps its low 64 bits"""
    if not torch.is_tensor(frame_ids):
        frame_ids = torch.tensor([((int(i) + (1 << 63)) % (1 << 64)) - (1 << 63) for i in frame_ids], dtype=torch.int64)
    frame_ids = _ids(frame_ids.reshape(-1), dev)
    if frame_ids.shape[0] != n_frames:
        raise ValueError(f'add_noise: {frame_ids.shape[0]} frame ids for {n_frames} frames')
    return frame_ids


def _noise_into_fresh(x, node_type, free_types, std, seed, draw, target, target_scale, rows_per_frame, frame_ids,
                      frame_rows=None):
    dev = x.device
    shape, x = x.shape, _f32_rows(x)
    rows, d = x.shape
    if not 1 <= d <= 4:
        raise ValueError(f'add_noise: x must have 1..4 columns, got {d}')
    if target is not None:
        target = _f32_rows(target.to(dev))
        if target.shape != x.shape:
            raise ValueError('add_noise: x / target shape mismatch')
    nt, ldt = _type_column(node_type, dev, rows)
    if nt.shape[0] != rows:
        raise ValueError(f'add_noise: {nt.shape[0]} node types for {rows} rows')
    free_mask = _free_mask(free_types, 'add_noise')
    ragged = _ragged(frame_rows, rows, dev, 'add_noise') if frame_rows is not None else None
    per_frame = max(rows, 1) if rows_per_frame is None else int(rows_per_frame)
    if ragged is None and (per_frame < 1 or rows % per_frame):
        raise ValueError(f'add_noise: {rows} rows do not split into frames of {rows_per_frame} rows')
    if frame_ids is not None:
        frame_ids = _frame_ids_tensor(frame_ids, ragged.B if ragged else rows // per_frame, dev)
    seed, draw = int(seed), int(draw)
    if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 64):
        raise ValueError('add_noise: seed and draw must lie in [0, 2^64)')
    out_x = torch.empty(rows, d, dtype=torch.float32, device=dev)
    out_t = torch.empty(rows, d, dtype=torch.float32, device=dev) if target is not None else None
    tail = (_ptr(frame_ids), seed, draw, float(std), _ptr(target), _ld(target), float(target_scale), out_x.data_ptr(), _ld(out_x),
            _ptr(out_t), _ld(out_t), _lib.stream_ptr())
    if ragged is not None:
        _lib.check(_lib.lib().hgn_training_noise_ragged(x.data_ptr(), _ld(x), d, nt.data_ptr(), ldt, free_mask, rows, ragged.host,
                                                        ragged.ptr.data_ptr(), ragged.B, *tail), 'hgn_training_noise_ragged')
    else:
        _lib.check(_lib.lib().hgn_training_noise(x.data_ptr(), _ld(x), d, nt.data_ptr(), ldt, free_mask, rows, per_frame, *tail),
                   'hgn_training_noise')
    return out_x.reshape(shape), (out_t.reshape(shape) if out_t is not None else None)


class _AddNoiseFn(torch.autograd.Function):
    """The noise is additive and a masked row is a copy: both outputs have the identity as derivative.  The backward launches nothing."""

    @staticmethod
    def forward(ctx, x, target, args):
        ctx.set_materialize_grads(False)
        ctx.refs = (x, target)
        return _noise_into_fresh(x.detach(), *args[:5], target.detach() if target is not None else None, *args[5:])

    @staticmethod
    def backward(ctx, d_x, d_target):
        x, target = ctx.refs
        return (_like(d_x, x) if ctx.needs_input_grad[0] else None,
                _like(d_target, target) if target is not None and ctx.needs_input_grad[1] else None, None)


def add_noise(x: torch.Tensor, node_type: torch.Tensor, free_types, std: float, seed: int, draw: int, target=None,
              target_scale: float = 0.0, rows_per_frame=None, frame_ids=None, frame_rows=None):
    """Seeded training noise for a batch of frames in one launch (hgn_training_noise; src/data/preprocessing.py:84-98,
    Preprocessing._add_noise, which runs once per frame): on the rows whose node type is listed in ``free_types``,
    ``noisy_x = x + n`` and ``noisy_target = target + target_scale * n`` with ``n = std * z``, z standard normal; every other row is
    copied.  ``x`` [rows, d] (d = 1..4) holds rows / rows_per_frame frames of ``rows_per_frame`` rows each (None: one frame), or -- a
    ragged batch, frames of different meshes -- ``frame_rows`` = the row count of every frame in turn (hgn_training_noise_ragged, one
    launch as well; giving both raises ValueError).  A frame's rows get the samples this call gives that frame alone with its id.
    The generator is counter-based (Philox4x32-10, Box-Muller): the sample of a row is a function of ``seed``, ``draw`` (both in
    [0, 2^64); e.g. the training step), the frame's id (``frame_ids``: a sequence or an int64 tensor of one id per frame, read modulo
    2^32; None: 0, 1, ..) and the row's place in its frame -- not of the frame's place in the batch or of the rank that holds it.
    -> (noisy_x, noisy_target or None): fresh tensors in the shape of ``x``; nothing is written into the inputs, which may be views
    of a trajectory.  When ``x`` or ``target`` requires grad the call is an autograd node whose backward hands the two incoming
    gradients back unchanged and launches nothing.
    Out of scope: the connector's `hyper_noise` keeps torch.normal; the reference's own src/data/preprocessing.py path through the
    shim is unchanged; noise inside captured graphs."""
    _one_split('add_noise', rows_per_frame, frame_rows)
    _lib.require_gpu(x)
    args = (node_type, tuple(free_types), float(std), seed, draw, float(target_scale), rows_per_frame, frame_ids, frame_rows)
    if _needs_grad(x, target):
        return _AddNoiseFn.apply(x, target, args)
    return _noise_into_fresh(x, *args[:5], target, *args[5:])


class FrameLosses(NamedTuple):
    """What frame_losses returns.  ``loss`` (0-d) is over all rows, ``per_frame`` [B] per frame; ``state_error`` / ``state_per_frame``
    likewise for the updated state (None without a state part); ``count`` [B+1] int64: the free rows of every frame, then of all."""
    loss: torch.Tensor
    per_frame: torch.Tensor
    state_error: Optional[torch.Tensor]
    state_per_frame: Optional[torch.Tensor]
    count: torch.Tensor


def _frame_losses_launch(net_out, target, node_type, free_types, rows_per_frame, state, frame_rows=None):
    """-> (loss [B+1], state_err [B+1] or None, count [B+1], what the backward launch needs)."""
    dev = net_out.device
    x = _f32_rows(net_out)
    rows, F = x.shape
    tgt = _f32_rows(target.to(dev))
    if tgt.shape != x.shape:
        raise ValueError(f'frame_losses: net_out {tuple(x.shape)} / target {tuple(tgt.shape)} shape mismatch')
    nt, ldt = _type_column(node_type, dev, rows)
    if nt.shape[0] != rows:
        raise ValueError(f'frame_losses: {nt.shape[0]} node types for {rows} rows')
    free_mask = _free_mask(free_types, 'frame_losses')
    ragged = _ragged(frame_rows, rows, dev, 'frame_losses') if frame_rows is not None else None
    per_frame = max(rows, 1) if rows_per_frame is None else int(rows_per_frame)
    if ragged is None and (per_frame < 1 or rows % per_frame):
        raise ValueError(f'frame_losses: {rows} rows do not split into frames of {rows_per_frame} rows')
    B = ragged.B if ragged else rows // per_frame
    nz = cur = prev = state_target = None
    d, ca, cp, eps = 0, 0.0, 0.0, 0.0
    if state is not None:
        nz, cur, d, ca, prev, cp, state_target = state
        d, eps = int(d), float(nz._eps)
        if nz._acc_sum.numel() != F:
            raise ValueError(f'frame_losses: the normaliser has {nz._acc_sum.numel()} columns, net_out {F}')
        cur, state_target = _f32_rows(cur.to(dev)), _f32_rows(state_target.to(dev))
        prev = _f32_rows(prev.to(dev)) if prev is not None else None
        for name, t in (('cur', cur), ('prev', prev), ('state_target', state_target)):
            if t is not None and tuple(t.shape) != (rows, d):
                raise ValueError(f'frame_losses: {name} must be [{rows}, {d}]')
    L = _lib.lib()
    nb = C.c_size_t(0)
    if ragged is not None:
        _lib.check(L.hgn_frame_losses_ragged_workspace_bytes(rows, ragged.host, B, C.byref(nb)), 'hgn_frame_losses_ragged_workspace_bytes')
    else:
        _lib.check(L.hgn_frame_losses_workspace_bytes(rows, per_frame, C.byref(nb)), 'hgn_frame_losses_workspace_bytes')
    ws = torch.empty(max(nb.value // 8, 1), dtype=torch.float64, device=dev)        # a fresh buffer per call: capturable
    loss = torch.empty(B + 1, dtype=torch.float32, device=dev)
    state_err = torch.empty(B + 1, dtype=torch.float32, device=dev) if state is not None else None
    count = torch.empty(B + 1, dtype=torch.int64, device=dev)
    head = (x.data_ptr(), _ld(x), tgt.data_ptr(), _ld(tgt), F, nt.data_ptr(), ldt, free_mask, rows)
    tail = (_ptr(nz._acc_sum) if nz is not None else None, _ptr(nz._acc_sum_squared) if nz is not None else None,
            _ptr(nz._acc_count) if nz is not None else None, eps, _ptr(cur), _ld(cur), d, float(ca), _ptr(prev), _ld(prev), float(cp),
            _ptr(state_target), _ld(state_target), loss.data_ptr(), _ptr(state_err), count.data_ptr(), ws.data_ptr(), ws.numel() * 8,
            _lib.stream_ptr())
    if ragged is not None:
        _lib.check(L.hgn_frame_losses_ragged(*head, ragged.host, ragged.ptr.data_ptr(), B, *tail), 'hgn_frame_losses_ragged')
    else:
        _lib.check(L.hgn_frame_losses(*head, per_frame, *tail), 'hgn_frame_losses')
    return loss, state_err, count, (x, tgt, nt, ldt, free_mask, per_frame, ragged)


def _split_losses(loss, state_err, count) -> FrameLosses:
    B = loss.shape[0] - 1
    return FrameLosses(loss[B], loss[:B], state_err[B] if state_err is not None else None,
                       state_err[:B] if state_err is not None else None, count)


_zero_cache = {}


def _zeros(dev, n: int) -> torch.Tensor:
    """n fp32 zeros that are never written (the absent half of an upstream gradient); fresh ones while a stream is capturing."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(n, dtype=torch.float32, device=dev)
    key = (dev.type, dev.index, n)
    if key not in _zero_cache:
        _zero_cache[key] = torch.zeros(n, dtype=torch.float32, device=dev)
    return _zero_cache[key]


class _FrameLossesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net_out, target, node_type, free_types, rows_per_frame, state, frame_rows):
        ctx.set_materialize_grads(False)
        loss, state_err, count, saved = _frame_losses_launch(net_out.detach(), target.detach(), node_type, free_types, rows_per_frame,
                                                             state, frame_rows)
        ctx.cfg = saved + (count, net_out, target)
        out = _split_losses(loss, state_err, count)
        ctx.mark_non_differentiable(*(t for t in out[2:] if t is not None))
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_frames, *unused):
        x, tgt, nt, ldt, free_mask, per_frame, ragged, count, net_out, target = ctx.cfg
        want_net, want_tgt = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_loss is None and g_frames is None) or not (want_net or want_tgt):
            return (None,) * 7
        dev, (rows, F) = x.device, x.shape
        B = ragged.B if ragged else rows // per_frame
        g = torch.cat([g_frames.to(dev).float().reshape(B) if g_frames is not None else _zeros(dev, B),
                       g_loss.to(dev).float().reshape(1) if g_loss is not None else _zeros(dev, 1)])
        d_net = torch.empty(rows, F, dtype=torch.float32, device=dev) if want_net else None
        d_tgt = torch.empty(rows, F, dtype=torch.float32, device=dev) if want_tgt else None
        head = (x.data_ptr(), _ld(x), tgt.data_ptr(), _ld(tgt), F, nt.data_ptr(), ldt, free_mask, rows)
        tail = (count.data_ptr(), g.data_ptr(), _ptr(d_net), _ld(d_net), _ptr(d_tgt), _ld(d_tgt), _lib.stream_ptr())
        if ragged is not None:
            _lib.check(_lib.lib().hgn_frame_losses_ragged_bwd(*head, ragged.host, ragged.ptr.data_ptr(), B, *tail),
                       'hgn_frame_losses_ragged_bwd')
        else:
            _lib.check(_lib.lib().hgn_frame_losses_bwd(*head, per_frame, *tail), 'hgn_frame_losses_bwd')
        return _like(d_net, net_out), _like(d_tgt, target), None, None, None, None, None


def frame_losses(net_out: torch.Tensor, target: torch.Tensor, node_type: torch.Tensor, free_types, rows_per_frame=None,
                 state=None, frame_rows=None) -> FrameLosses:
    """The reference's masked MSE (flag.py:150-152: MSELoss()(target[mask], output[mask]), mask = the rows whose node type is listed
    in ``free_types``) per frame of a batch and over all rows, on the device, in two launches and without a host read
    (hgn_frame_losses).  ``net_out`` / ``target`` [rows, F] hold rows / rows_per_frame frames of ``rows_per_frame`` rows each (None:
    one frame), or -- a ragged batch, frames of different meshes -- ``frame_rows`` = the row count of every frame in turn
    (hgn_frame_losses_ragged: the same launches, order and bits per frame; giving both raises ValueError); views with a row stride are
    taken as they are.  ``state`` = (normalizer, cur, d, ca, prev, cp, state_target) adds the
    error of the updated state ``ca*cur + normalizer.inverse(net_out)[:, :d] + cp*prev`` (``prev`` may be None; the bits of
    rollout_advance / the model's `update`) against ``state_target`` [rows, d]: what validation_step reports beside the loss.
    Sums are doubles in a fixed order (include/hgn_features.h): runs are bit-equal, and a frame's entries depend on its own rows
    alone.  A frame without a free row has NaN entries, as the reference's mean over no element.
    -> FrameLosses(loss, per_frame [B], state_error, state_per_frame [B], count [B+1]).  When ``net_out`` or ``target`` requires grad
    the call is an autograd node: ``loss`` and ``per_frame`` are differentiable through ONE launch (hgn_frame_losses_bwd), the other
    outputs are not (the state error is an evaluation figure); an output nobody differentiates costs nothing in the backward pass."""
    _one_split('frame_losses', rows_per_frame, frame_rows)
    _lib.require_gpu(net_out)
    if _needs_grad(net_out, target):
        return FrameLosses(*_FrameLossesFn.apply(net_out, target, node_type, tuple(free_types), rows_per_frame, state, frame_rows))
    loss, state_err, count, _ = _frame_losses_launch(net_out.detach(), target.detach(), node_type, free_types, rows_per_frame, state,
                                                     frame_rows)
    return _split_losses(loss, state_err, count)


def radius_edges(pos: torch.Tensor, node_type: torch.Tensor, radius: float, sender_type: int, receiver_type: int,
                 nbr_rowptr=None, nbr=None):
    """plate.py:84-110: directed pairs closer than ``radius`` with the given endpoint types that are not mesh
    neighbours (CSR ``nbr_rowptr`` / ``nbr``); ascending (sender, receiver) order.  -> (senders, receivers) int64."""
    _lib.require_gpu(pos)
    dev = pos.device
    pos = _f32_rows(pos)
    N = pos.shape[0]
    nt, ldt = _type_column(node_type, dev, N)
    L = _lib.lib()
    nb = C.c_size_t(0)
    _lib.check(L.hgn_radius_edges_workspace_bytes(N, C.byref(nb)), 'hgn_radius_edges_workspace_bytes')
    ws = _workspace(dev, nb.value, 'radius')
    offsets = torch.empty(N + 1, dtype=torch.int32, device=dev)
    total = C.c_int64(0)
    args = (pos.data_ptr(), _ld(pos), pos.shape[1], nt.data_ptr(), ldt, N, float(radius), int(sender_type),
            int(receiver_type), _ptr(nbr_rowptr), _ptr(nbr))
    _lib.check(L.hgn_radius_edges_count(*args, offsets.data_ptr(), C.byref(total), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr()), 'hgn_radius_edges_count')
    s = torch.empty(total.value, dtype=torch.int64, device=dev)
    r = torch.empty(total.value, dtype=torch.int64, device=dev)
    if total.value:
        _lib.check(L.hgn_radius_edges_fill(*args, offsets.data_ptr(), s.data_ptr(), r.data_ptr(), _lib.stream_ptr()),
                   'hgn_radius_edges_fill')
    return s, r


def radius_edges_batch(pos: torch.Tensor, node_type: torch.Tensor, n_graphs: int, radius: float, sender_type: int,
                       receiver_type: int, nbr_rowptr=None, nbr=None):
    """``radius_edges`` over the disjoint union of ``n_graphs`` graphs of equal size in one query (not in the reference, which
    runs plate.py:84-110 per frame and concatenates, MeshSimulator.py:159-234): ``pos`` / ``node_type`` hold the B*N rows of the
    union, graph b owns rows [b*N, (b+1)*N); no pair crosses a graph; ``nbr_rowptr`` / ``nbr`` is the neighbour CSR of ONE mesh
    (local ids) shared by all graphs.  Union ids in ascending (sender, receiver) order = the per-graph results shifted by b*N and
    concatenated.  One host read-back for the whole batch.
    -> (senders, receivers) int64 and graph_offsets [B+1] int32 (edges before graph b; the last entry is the total)."""
    _lib.require_gpu(pos)
    dev = pos.device
    pos = _f32_rows(pos)
    rows, B = pos.shape[0], int(n_graphs)
    nt, ldt = _type_column(node_type, dev, rows)
    if B < 1 or rows % B or nt.shape[0] != rows:
        raise ValueError(f'radius_edges_batch: {rows} position rows / {nt.shape[0]} node types do not split into {B} graphs of equal size')
    N = rows // B
    L = _lib.lib()
    nb = C.c_size_t(0)
    _lib.check(L.hgn_radius_edges_batch_workspace_bytes(B, N, C.byref(nb)), 'hgn_radius_edges_batch_workspace_bytes')
    ws = _workspace(dev, nb.value, 'radius')
    offsets = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    graph_offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    total = C.c_int64(0)
    args = (pos.data_ptr(), _ld(pos), pos.shape[1], nt.data_ptr(), ldt, B, N, float(radius), int(sender_type),
            int(receiver_type), _ptr(nbr_rowptr), _ptr(nbr))
    _lib.check(L.hgn_radius_edges_batch_count(*args, offsets.data_ptr(), graph_offsets.data_ptr(), C.byref(total),
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'hgn_radius_edges_batch_count')
    s = torch.empty(total.value, dtype=torch.int64, device=dev)
    r = torch.empty(total.value, dtype=torch.int64, device=dev)
    if total.value:
        _lib.check(L.hgn_radius_edges_batch_fill(*args, offsets.data_ptr(), s.data_ptr(), r.data_ptr(), _lib.stream_ptr()),
                   'hgn_radius_edges_batch_fill')
    return s, r, graph_offsets


def radius_edges_ragged(pos: torch.Tensor, node_type: torch.Tensor, frame_rows, radius: float, sender_type: int,
                        receiver_type: int, nbr_rowptr=None, nbr=None):
    """``radius_edges_batch`` for graphs of different sizes (hgn_radius_edges_ragged_count/_fill): ``pos`` / ``node_type`` hold the
    rows of the disjoint union, graph b owns the ``frame_rows[b]`` rows after those of the graphs before it; no pair crosses a graph.
    Every graph has its own mesh, so ``nbr_rowptr`` [rows+1] / ``nbr`` is the neighbour CSR of the UNION, in union ids (both None: no
    exclusion).  Union ids in ascending (sender, receiver) order = the per-graph ``radius_edges`` results shifted by the rows before
    the graph and concatenated.  One host read-back for the whole batch.
    -> (senders, receivers) int64 and graph_offsets [B+1] int32 (edges before graph b; the last entry is the total)."""
    _lib.require_gpu(pos)
    dev = pos.device
    pos = _f32_rows(pos)
    rows = pos.shape[0]
    nt, ldt = _type_column(node_type, dev, rows)
    if nt.shape[0] != rows:
        raise ValueError(f'radius_edges_ragged: {nt.shape[0]} node types for {rows} position rows')
    ragged = _ragged(frame_rows, rows, dev, 'radius_edges_ragged')
    L = _lib.lib()
    nb = C.c_size_t(0)
    _lib.check(L.hgn_radius_edges_ragged_workspace_bytes(rows, ragged.host, ragged.B, C.byref(nb)),
               'hgn_radius_edges_ragged_workspace_bytes')
    ws = _workspace(dev, nb.value, 'radius')
    offsets = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    graph_offsets = torch.empty(ragged.B + 1, dtype=torch.int32, device=dev)
    total = C.c_int64(0)
    args = (pos.data_ptr(), _ld(pos), pos.shape[1], nt.data_ptr(), ldt, rows, ragged.host, ragged.ptr.data_ptr(), ragged.B,
            float(radius), int(sender_type), int(receiver_type), _ptr(nbr_rowptr), _ptr(nbr))
    _lib.check(L.hgn_radius_edges_ragged_count(*args, offsets.data_ptr(), graph_offsets.data_ptr(), C.byref(total),
                                               ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'hgn_radius_edges_ragged_count')
    s = torch.empty(total.value, dtype=torch.int64, device=dev)
    r = torch.empty(total.value, dtype=torch.int64, device=dev)
    if total.value:
        _lib.check(L.hgn_radius_edges_ragged_fill(*args, offsets.data_ptr(), s.data_ptr(), r.data_ptr(), _lib.stream_ptr()),
                   'hgn_radius_edges_ragged_fill')
    return s, r, graph_offsets
