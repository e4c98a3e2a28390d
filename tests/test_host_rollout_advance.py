"""CPU-side checks (no GPU) of the lock-step evaluation: the C ABI of the one-launch state update (include/hgn_features.h:
hgn_rollout_advance) is exported, declared, and answers bad arguments with HGN_E_INVALID and a message that names the entry before
any device work; the strided window views n_step_computation hands to rollout_batch index the frames its loop slices."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'hgn_rollout_advance'
INVALID = -1


def test_abi_rollout_advance_is_exported_and_declared():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    assert ENTRY in declared and ENTRY in _lib.EXPORTS
    assert hasattr(raw, ENTRY) and hasattr(lib, ENTRY)
    for cite in ('flag.py:169-180,243', 'cylinder.py:155-165', 'plate.py:246-257,328'):
        assert cite in header, cite
    # the ctypes signature has one entry per parameter of the declaration
    params = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', header, flags=re.S).group(1)
    assert len(_lib._SIGS[ENTRY][1]) == len(params.split(','))


def _call(lib, **kw):
    """Host memory stands in for device buffers: every call below must be refused before anything is dereferenced or launched."""
    p = lambda a: C.cast(a, C.c_void_p)
    buf = {name: p((C.c_float * 64)()) for name in ('net', 'sum', 'sq', 'cnt', 'cur', 'prev', 'fb', 'next', 'rec', 'po', 'inv')}
    buf['types'] = p((C.c_int64 * 16)())
    a = dict(net=buf['net'], ld_out=3, out_cols=3, F=3, acc_sum=buf['sum'], acc_sumsq=buf['sq'], acc_count=buf['cnt'], eps=1e-8,
             cur=buf['cur'], ld_cur=3, d=3, ca=2.0, prev=buf['prev'], ld_prev=3, cp=-1.0, types=buf['types'], ldt=1, free_mask=1,
             fb=buf['fb'], ld_fb=3, rows=10, next=buf['next'], ld_next=3, rec=buf['rec'], ld_rec=3, rec_before=1, po=buf['po'],
             ld_po=3, inv=buf['inv'], ld_inv=3, inv_from=0)
    a.update(kw)
    return lib.hgn_rollout_advance(
        a['net'], a['ld_out'], a['out_cols'], a['F'], a['acc_sum'], a['acc_sumsq'], a['acc_count'], a['eps'], a['cur'], a['ld_cur'],
        a['d'], a['ca'], a['prev'], a['ld_prev'], a['cp'], a['types'], a['ldt'], a['free_mask'], a['fb'], a['ld_fb'], a['rows'],
        a['next'], a['ld_next'], a['rec'], a['ld_rec'], a['rec_before'], a['po'], a['ld_po'], a['inv'], a['ld_inv'], a['inv_from'],
        None)


def test_abi_rollout_advance_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = {'null network output': dict(net=None), 'null cur': dict(cur=None), 'null node_type': dict(types=None),
           'null next': dict(next=None), 'null acc_sum': dict(acc_sum=None), 'null acc_sumsq': dict(acc_sumsq=None),
           'null acc_count': dict(acc_count=None),
           'zero ld_out': dict(ld_out=0), 'zero ld_cur': dict(ld_cur=0), 'zero ld_prev': dict(ld_prev=0), 'zero ldt': dict(ldt=0),
           'zero ld_fb': dict(ld_fb=0), 'zero ld_next': dict(ld_next=0), 'zero ld_rec': dict(ld_rec=0), 'zero ld_po': dict(ld_po=0),
           'zero ld_inv': dict(ld_inv=0), 'zero ld_inv, no column': dict(ld_inv=0, inv_from=3),
           'ld_out < F': dict(ld_out=2), 'ld_rec < d': dict(ld_rec=2), 'ld_inv < F - inv_from': dict(ld_inv=1, inv_from=1),
           'columns do not match the normaliser': dict(out_cols=2), 'more columns than the normaliser': dict(out_cols=4, ld_out=4),
           'F = 0': dict(F=0, out_cols=0), 'F too wide': dict(F=33, out_cols=33, ld_out=33),
           'd = 0': dict(d=0), 'd > F': dict(d=4, ld_cur=4, ld_next=4), 'negative rows': dict(rows=-1), 'rows >= 2^31': dict(rows=1 << 31),
           'inv_from < 0': dict(inv_from=-1), 'inv_from > F': dict(inv_from=4)}
    for what, kw in bad.items():
        assert _call(lib, **kw) == INVALID, what
        assert b'hgn_rollout_advance' in lib.hgn_last_error(), what
    assert _call(lib, out_cols=2) == INVALID and b'does not match the normaliser' in lib.hgn_last_error()
    # an unused (null) matrix carries no stride; no rows: nothing to do, nothing launched
    assert _call(lib, rows=0) == 0
    assert _call(lib, rows=0, prev=None, ld_prev=0, fb=None, ld_fb=0, rec=None, ld_rec=0, po=None, ld_po=0, inv=None, ld_inv=0) == 0


def test_rollout_advance_refuses_host_tensors():
    from hgn_amd import _lib, features
    from hgn_amd.normalizer import Normalizer
    with pytest.raises(_lib.HgnError):
        features.rollout_advance(torch.zeros(4, 3), Normalizer(3, 'n'), torch.zeros(4, 3), 3, 2.0, None, 0.0,
                                 torch.zeros(4, 1, dtype=torch.int64), (0,), None, torch.zeros(4, 3))


def test_window_views_index_the_frames_the_loop_slices():
    """Frame f, node n, component c of every series carries the code 10000 f + 10 n + c (+ an offset per series)."""
    from hgn_amd import system_model
    T, N, n_step = 9, 4, 3

    def coded(width, offset, dtype):
        f, n, c = torch.meshgrid(torch.arange(T), torch.arange(N), torch.arange(width), indexing='ij')
        return (10000 * f + 10 * n + c + offset).to(dtype)
    trajectory = {'world_pos': coded(3, 0, torch.float32), 'prev|world_pos': coded(3, 100000, torch.float32),
                  'node_type': coded(1, 200000, torch.int32), 'mesh_pos': coded(2, 300000, torch.float32),
                  'cells': coded(3, 400000, torch.int64)}
    for frames in (T, T - 2, n_step + 1):                       # the whole trajectory, `num_timesteps` frames of it, one window
        views = system_model.AbstractSystemModel.window_views(trajectory, n_step, frames)
        assert set(views) == set(trajectory)
        for name, series in trajectory.items():
            v = views[name]
            assert v.shape == (frames - n_step, n_step + 1) + tuple(series.shape[1:]) and v.dtype == series.dtype
            assert v.data_ptr() == series.data_ptr()            # a view of the trajectory: no copy
            for start in range(frames - n_step):                 # what n_step_computation's loop slices for this window
                assert torch.equal(v[start], series[start:start + n_step + 1]), (name, start)
            if frames - n_step > 1:                              # a chunk of windows is a view as well
                assert v[1:3].data_ptr() == series[1:].data_ptr()
    with pytest.raises(ValueError):
        system_model.AbstractSystemModel.window_views(trajectory, n_step, T + 1)
    # a series that is itself a view with strides of its own (every second frame of a longer recording)
    longer = torch.arange(2 * T * N * 3, dtype=torch.float32).reshape(2 * T, N, 3)
    sub = longer[::2]
    v = system_model.AbstractSystemModel.window_views({'world_pos': sub}, n_step, T)['world_pos']
    for start in range(T - n_step):
        assert torch.equal(v[start], sub[start:start + n_step + 1])


def test_nstep_batch_is_off_by_default_and_every_model_has_rollout_batch():
    from hgn_amd import system_model
    assert system_model.AbstractSystemModel.nstep_batch is None
    for cls in (system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel):
        assert callable(getattr(cls, 'rollout_batch'))
