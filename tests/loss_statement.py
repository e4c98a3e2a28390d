"""The per-frame losses of include/hgn_features.h (hgn_frame_losses, hgn_frame_losses_bwd) stated in numpy fp64: the yardstick of
tests/test_frame_losses_cpu.py and tests/test_gpu_frame_losses.py.  Everything is evaluated on the fp32 inputs promoted to double; the
updated state ``v`` is not recomputed here but taken as fp32 bits from features.advance_state (the header defines it as those bits)."""
import numpy as np


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def free_rows(node_type, free_types) -> np.ndarray:
    """[rows] bool: the type is listed in ``free_types`` and lies in [0, 32)."""
    t = np.asarray(node_type.detach().cpu().numpy() if hasattr(node_type, 'detach') else node_type).reshape(len(node_type), -1)[:, 0]
    listed = np.isin(t, np.asarray([int(k) for k in free_types if 0 <= int(k) < 32], dtype=np.int64))
    return listed & (t >= 0) & (t < 32)


def _entries(sq, free, rows_per_frame):
    """sq [rows, width] squared differences -> (mean over the free rows' elements per frame and over all [B+1], count [B+1])."""
    rows, width = sq.shape
    B = rows // rows_per_frame
    per_row = np.where(free, sq.sum(axis=1), 0.0)
    S = per_row.reshape(B, rows_per_frame).sum(axis=1)
    n = free.reshape(B, rows_per_frame).sum(axis=1).astype(np.int64)
    S, n = np.append(S, S.sum()), np.append(n, n.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        return S / (n.astype(np.float64) * width), n


def losses(net_out, target, node_type, free_types, rows_per_frame=None, v=None, state_target=None):
    """-> (loss [B+1] fp64, state_err [B+1] fp64 or None, count [B+1] int64); entry B covers all rows; a frame without a free row has
    NaN entries.  ``v`` [rows, d]: the updated state (fp32 bits), ``state_target`` [rows, d]."""
    o, g = _f64(net_out), _f64(target)
    rows = o.shape[0]
    rpf = rows if rows_per_frame is None else int(rows_per_frame)
    free = free_rows(node_type, free_types)
    loss, count = _entries((o - g) ** 2, free, rpf)
    state_err = None
    if v is not None:
        state_err, _ = _entries((_f64(v) - _f64(state_target)) ** 2, free, rpf)
    return loss, state_err, count


def d_net(net_out, target, node_type, free_types, rows_per_frame, g):
    """The derivative of sum_k g[k] * loss[k] with respect to net_out, fp64 [rows, F]; the one with respect to target is its negation.
    ``g`` [B+1]."""
    o, t = _f64(net_out), _f64(target)
    rows, F = o.shape
    rpf = rows if rows_per_frame is None else int(rows_per_frame)
    free = free_rows(node_type, free_types)
    _, count = _entries(np.zeros_like(o), free, rpf)
    g = np.asarray(g, dtype=np.float64)
    B = rows // rpf
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.repeat(g[:B] / (count[:B] * float(F)), rpf) + g[B] / (count[B] * float(F))
    return np.where(free[:, None], 2.0 * (o - t) * w[:, None], 0.0)
