"""CPU-side checks (no GPU) of the per-frame losses (include/hgn_features.h: hgn_frame_losses_workspace_bytes, hgn_frame_losses,
hgn_frame_losses_bwd; features.frame_losses; AbstractSystemModel.loss_kernel / one_step_errors): the entries are declared, exported
and bound and refuse bad arguments with HGN_E_INVALID and their name before any device work; the workspace size grows with its
arguments; the statement of tests/loss_statement.py is the reference's masked MSE; and one_step_errors cuts a trajectory into the
chunks it documents (the model calls are stubbed)."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import loss_statement as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'hgn_frame_losses_workspace_bytes': 3, 'hgn_frame_losses': 29, 'hgn_frame_losses_bwd': 17}
INVALID = -1


def test_abi_frame_losses_are_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for entry, n_args in ENTRIES.items():
        assert entry in declared and entry in _lib.EXPORTS, entry
        assert hasattr(raw, entry) and hasattr(lib, entry), entry
        params = re.search(r'int\s+' + entry + r'\s*\(([^;]*)\)\s*;', header, flags=re.S).group(1)
        assert len(_lib._SIGS[entry][1]) == len(params.split(',')) == n_args, entry
    chunk = int(re.search(r'#define\s+HGN_LOSS_CHUNK_ROWS\s+(\d+)', header).group(1))
    assert 1 <= chunk <= 1024
    flat = re.sub(r'\s*\n\s*\*\s*', ' ', header)
    for phrase in ('Nothing flows through state_err', 'two runs give equal bits', 'depend on the rows of frame f alone', 'No atomics'):
        assert phrase in flat, phrase


def _p(a):
    return C.cast(a, C.c_void_p)


def _fwd(lib, **kw):
    """Host memory stands in for device buffers: every call below must be refused before anything is dereferenced or launched."""
    f = lambda n=96: _p((C.c_float * n)())
    ws = (C.c_double * 64)()
    a = dict(net_out=f(), ld_out=3, target=f(), ld_tgt=3, F=3, types=_p((C.c_int64 * 32)()), ldt=1, free_mask=1, rows=12, rpf=4,
             acc_sum=f(), acc_sumsq=f(), acc_count=f(), eps=1e-8, cur=f(), ld_cur=3, d=3, ca=2.0, prev=f(), ld_prev=3, cp=-1.0,
             state_target=f(), ld_st=3, loss=f(), state_err=f(), count=_p((C.c_int64 * 8)()), ws=_p(ws), ws_bytes=C.sizeof(ws))
    a.update(kw)
    return lib.hgn_frame_losses(a['net_out'], a['ld_out'], a['target'], a['ld_tgt'], a['F'], a['types'], a['ldt'], a['free_mask'],
                                a['rows'], a['rpf'], a['acc_sum'], a['acc_sumsq'], a['acc_count'], a['eps'], a['cur'], a['ld_cur'],
                                a['d'], a['ca'], a['prev'], a['ld_prev'], a['cp'], a['state_target'], a['ld_st'], a['loss'],
                                a['state_err'], a['count'], a['ws'], a['ws_bytes'], None)


NO_STATE = dict(acc_sum=None, acc_sumsq=None, acc_count=None, cur=None, prev=None, state_target=None, state_err=None)


def test_abi_frame_losses_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    ws = (C.c_double * 64)()
    bad = {'F = 0': dict(F=0), 'F = 33': dict(F=33, ld_out=33, ld_tgt=33), 'd = 0': dict(d=0), 'd > F': dict(d=4, ld_cur=4, ld_st=4, ld_prev=4),
           'negative rows': dict(rows=-4), 'rows >= 2^31': dict(rows=1 << 31, rpf=1 << 31), 'rows_per_frame = 0': dict(rpf=0),
           'rows_per_frame < 0': dict(rpf=-4), 'rows_per_frame does not divide rows': dict(rpf=5),
           'ld_out < F': dict(ld_out=2), 'ld_tgt < F': dict(ld_tgt=2), 'ld_cur < d': dict(ld_cur=2), 'ld_prev < d': dict(ld_prev=0),
           'ld_st < d': dict(ld_st=2), 'ldt < 1': dict(ldt=0),
           'state part without acc_sum': dict(acc_sum=None), 'state part without acc_sumsq': dict(acc_sumsq=None),
           'state part without acc_count': dict(acc_count=None), 'state part without cur': dict(cur=None),
           'state part without state_target': dict(state_target=None), 'prev alone': dict(NO_STATE, prev=_p((C.c_float * 96)())),
           'state part without state_err': dict(state_err=None), 'state_err without a state part': dict(NO_STATE, state_err=_p((C.c_float * 8)())),
           'null net_out': dict(net_out=None), 'null target': dict(target=None), 'null node_type': dict(types=None),
           'null loss': dict(loss=None), 'null count': dict(count=None), 'null workspace': dict(ws=None),
           'workspace too small': dict(ws_bytes=3 * 3 * 8 - 1), 'workspace misaligned': dict(ws=C.c_void_p(C.addressof(ws) + 4))}
    for what, kw in bad.items():
        assert _fwd(lib, **kw) == INVALID, what
        assert b'hgn_frame_losses' in lib.hgn_last_error(), what
    # no rows: nothing to do, nothing launched -- with and without the state part, which then carries no stride
    assert _fwd(lib, rows=0) == 0
    assert _fwd(lib, rows=0, net_out=None, target=None, types=None, loss=None, count=None, ws=None, ws_bytes=0, d=0, ld_cur=0, ld_prev=0,
                ld_st=0, **NO_STATE) == 0
    assert _fwd(lib, rows=0, F=0) == INVALID and _fwd(lib, rows=0, rpf=0) == INVALID and _fwd(lib, rows=0, state_err=None) == INVALID


def _bwd(lib, **kw):
    f = lambda n=96: _p((C.c_float * n)())
    a = dict(net_out=f(), ld_out=3, target=f(), ld_tgt=3, F=3, types=_p((C.c_int64 * 32)()), ldt=1, free_mask=1, rows=12, rpf=4,
             count=_p((C.c_int64 * 8)()), g=f(8), d_net=f(), ld_dnet=3, d_target=f(), ld_dtgt=3)
    a.update(kw)
    return lib.hgn_frame_losses_bwd(a['net_out'], a['ld_out'], a['target'], a['ld_tgt'], a['F'], a['types'], a['ldt'], a['free_mask'],
                                    a['rows'], a['rpf'], a['count'], a['g'], a['d_net'], a['ld_dnet'], a['d_target'], a['ld_dtgt'], None)


def test_abi_frame_losses_bwd_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = {'F = 0': dict(F=0), 'F = 33': dict(F=33, ld_out=33, ld_tgt=33, ld_dnet=33, ld_dtgt=33), 'negative rows': dict(rows=-4),
           'rows >= 2^31': dict(rows=1 << 31, rpf=1 << 31), 'rows_per_frame = 0': dict(rpf=0), 'rows_per_frame < 0': dict(rpf=-4),
           'rows_per_frame does not divide rows': dict(rpf=5), 'ld_out < F': dict(ld_out=2), 'ld_tgt < F': dict(ld_tgt=2),
           'ld_dnet < F': dict(ld_dnet=2), 'ld_dtgt < F': dict(ld_dtgt=0), 'ldt < 1': dict(ldt=0),
           'no output': dict(d_net=None, d_target=None), 'null net_out': dict(net_out=None), 'null target': dict(target=None),
           'null node_type': dict(types=None), 'null count': dict(count=None)}
    for what, kw in bad.items():
        assert _bwd(lib, **kw) == INVALID, what
        assert b'hgn_frame_losses_bwd' in lib.hgn_last_error(), what
    assert _bwd(lib, rows=0) == 0 and _bwd(lib, rows=0, d_target=None, ld_dtgt=0, g=None) == 0
    assert _bwd(lib, rows=0, net_out=None, target=None, types=None, count=None, g=None) == 0
    assert _bwd(lib, rows=0, d_net=None, d_target=None) == INVALID and _bwd(lib, rows=0, F=0) == INVALID


def _ws(lib, rows, rpf):
    nb = C.c_size_t(0)
    rc = lib.hgn_frame_losses_workspace_bytes(rows, rpf, C.byref(nb))
    return rc, nb.value


def test_workspace_size_grows_with_frames_and_with_rows_per_frame():
    """Monotone in the number of frames at a fixed frame size and in the frame size at a fixed number of frames; a multiple of 8."""
    from hgn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    chunk = int(re.search(r'#define\s+HGN_LOSS_CHUNK_ROWS\s+(\d+)', header).group(1))
    sizes = [1, 2, chunk - 1, chunk, chunk + 1, 3000, 100000]
    for rpf in sizes:
        got = [_ws(lib, B * rpf, rpf) for B in (0, 1, 2, 3, 128)]
        assert all(rc == 0 and nb % 8 == 0 for rc, nb in got), rpf
        assert all(a[1] <= b[1] for a, b in zip(got, got[1:])) and got[1][1] > 0, rpf
    for B in (1, 3, 128):
        got = [_ws(lib, B * rpf, rpf)[1] for rpf in sizes]
        assert all(a <= b for a, b in zip(got, got[1:])), B
    assert _ws(lib, chunk + 1, chunk + 1)[1] > _ws(lib, chunk, chunk)[1]                 # a second chunk needs room
    for rows, rpf in ((-1, 1), (1 << 31, 1), (4, 0), (4, -2), (4, 3)):
        assert _ws(lib, rows, rpf)[0] == INVALID and b'hgn_frame_losses_workspace_bytes' in lib.hgn_last_error()
    assert lib.hgn_frame_losses_workspace_bytes(4, 2, None) == INVALID


@pytest.mark.parametrize('rpf,B,F,free', [(1, 5, 3, (0,)), (7, 3, 3, (0, 5)), (300, 2, 1, (0,)), (33, 4, 32, (0, 3))])
def test_statement_is_the_masked_mse_of_the_reference(rpf, B, F, free):
    """tests/loss_statement.py against `_masked_mse` (and against MSELoss on the boolean-indexed rows, flag.py:150-152) evaluated in
    fp64 by torch, per frame and over all rows; the derivative against autograd."""
    from hgn_amd.system_model import _masked_mse
    gen = torch.Generator().manual_seed(100 * rpf + B)
    rows = rpf * B
    out, tgt = torch.randn(rows, F, generator=gen), torch.randn(rows, F, generator=gen)
    kinds = torch.tensor([0, 1, 3, 5, 40, -1])
    types = kinds[torch.randint(0, len(kinds), (rows, 1), generator=gen)]
    types[0, 0] = 0
    loss, state_err, count = LS.losses(out, tgt, types, free, rpf)
    assert state_err is None and loss.shape == (B + 1,) and count.dtype == np.int64
    mask = torch.isin(types[:, 0], torch.tensor(free))
    assert np.array_equal(LS.free_rows(types, free + (40,)), mask.numpy())               # 40 is never free, listed or not
    o64, t64 = out.double().requires_grad_(True), tgt.double()
    whole = _masked_mse(t64, o64, mask)
    assert abs(float(whole.detach()) - loss[B]) <= 1e-14 * abs(loss[B]) and count[B] == int(mask.sum())
    assert abs(float(torch.nn.MSELoss()(t64[mask], o64[mask]).detach()) - loss[B]) <= 1e-14 * abs(loss[B])
    per = []
    for f in range(B):
        rows_f = slice(f * rpf, (f + 1) * rpf)
        per.append(_masked_mse(t64[rows_f], o64[rows_f], mask[rows_f]))
        assert count[f] == int(mask[rows_f].sum())
        if count[f] == 0:
            assert np.isnan(loss[f]) and bool(torch.isnan(per[-1]))
        else:
            assert abs(float(per[-1].detach()) - loss[f]) <= 1e-14 * abs(loss[f]), f
    g = np.zeros(B + 1)
    g[B], live = 0.7, [f for f in range(B) if count[f] > 0]
    g[live[0]] = 1.3
    (0.7 * whole + 1.3 * per[live[0]]).backward()
    want = LS.d_net(out, tgt, types, free, rpf, g)
    assert np.allclose(o64.grad.numpy(), want, rtol=1e-13, atol=0) and not want[~mask.numpy()].any()
    # the state part: any [rows, d] matrix of fp32 bits stands for the updated state
    v, st = torch.randn(rows, 2, generator=gen), torch.randn(rows, 2, generator=gen)
    _, err, _ = LS.losses(out, tgt, types, free, rpf, v, st)
    assert abs(float(_masked_mse(st.double(), v.double(), mask)) - err[B]) <= 1e-14 * abs(err[B])


def _bare(cls, connector=False, balancer=False):
    """A system model with the switches one_step_errors reads and nothing else; the model calls are stubbed by the tests."""
    model = cls.__new__(cls)
    torch.nn.Module.__init__(model)
    model._rmp, model._balancer = connector, balancer
    return model


def _trajectory(T, N=4):
    stamp = torch.arange(T, dtype=torch.float32).view(T, 1, 1)
    return {'cells': torch.zeros(T, 2, 3, dtype=torch.int64), 'mesh_pos': torch.zeros(T, N, 2), 'node_type': torch.zeros(T, N, 1, dtype=torch.int64),
            'world_pos': stamp.expand(T, N, 3).clone(), 'prev|world_pos': torch.zeros(T, N, 3), 'target|world_pos': torch.zeros(T, N, 3)}


def _stub(model, log):
    """Frames carry their index in `world_pos`; the stubs report [index, index + 0.5] and log how they were called."""
    def build_graph_batch(chunk, is_training):
        assert is_training is False and chunk['cells'].dim() == 2
        return ('union', chunk['world_pos'][:, 0, 0].tolist())

    def expand_graph_batch(graph, n_graphs, step, num_steps, is_training):
        assert is_training is False and len(graph[1]) == n_graphs
        log.append(('batch', step, n_graphs, num_steps))
        return graph

    def validation_step_batch(graph, flat, n_graphs):
        assert flat['world_pos'].dim() == 2 and flat['world_pos'].shape[0] == n_graphs * 4 and flat['cells'].dim() == 2
        ids = flat['world_pos'].view(n_graphs, 4, 3)[:, 0, 0]
        assert ids.tolist() == graph[1]
        return ids.clone(), ids + 0.5

    def build_graph(frame, is_training):
        assert is_training is False and frame['world_pos'].dim() == 2
        return ('single', float(frame['world_pos'][0, 0]))

    def expand_graph(graph, step, num_steps, is_training):
        assert is_training is False and graph[1] == step
        log.append(('frame', step, 1, num_steps))
        return graph

    def validation_step(graph, frame):
        return graph[1], graph[1] + 0.5
    for fn in (build_graph_batch, expand_graph_batch, validation_step_batch, build_graph, expand_graph, validation_step):
        setattr(model, fn.__name__, fn)


def test_one_step_errors_chunks_the_trajectory():
    from hgn_amd import system_model
    want = lambda T: torch.stack([torch.arange(T, dtype=torch.float32), torch.arange(T, dtype=torch.float32) + 0.5], dim=1)
    for T, M, chunks in ((5, 2, [(0, 2), (2, 2), (4, 1)]), (4, 2, [(0, 2), (2, 2)]), (3, 8, [(0, 3)]), (3, 1, [(0, 1), (1, 1), (2, 1)])):
        model, log = _bare(system_model.FlagModel), []
        _stub(model, log)
        got = model.one_step_errors(_trajectory(T), batch=M)
        assert log == [('batch', first, count, T) for first, count in chunks], (T, M)
        assert got.device.type == 'cpu' and got.dtype == torch.float32 and torch.equal(got, want(T)), (T, M)
    # num_timesteps: only the first frames, and the period of the stages is that many steps
    model, log = _bare(system_model.FlagModel), []
    _stub(model, log)
    got = model.one_step_errors(_trajectory(6), batch=4, num_timesteps=5)
    assert log == [('batch', 0, 4, 5), ('batch', 4, 1, 5)] and torch.equal(got, want(5))


def test_one_step_errors_takes_the_loop_without_a_batch_and_with_per_frame_stages():
    from hgn_amd import system_model
    want = torch.stack([torch.arange(5, dtype=torch.float32), torch.arange(5, dtype=torch.float32) + 0.5], dim=1)
    for cls, switches, batch in ((system_model.FlagModel, {}, None), (system_model.FlagModel, {}, 0),
                                 (system_model.CylinderModel, dict(connector=True), 2), (system_model.PlateModel, dict(balancer=True), 2)):
        model, log = _bare(cls, **switches), []
        _stub(model, log)
        got = model.one_step_errors(_trajectory(5), batch=batch)
        assert log == [('frame', t, 1, 5) for t in range(5)], (cls, switches, batch)
        assert got.shape == (5, 2) and got.dtype == torch.float32 and torch.equal(got, want)


def test_loss_kernel_is_a_class_default_and_travels_in_pickles():
    from hgn_amd import system_model
    for cls in (system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel):
        assert cls.loss_kernel is False and 'loss_kernel' not in cls.__dict__                  # the base class's one default
        for method in ('training_step_batch', 'validation_step_batch', 'one_step_errors'):
            assert callable(getattr(cls, method))
    model = _bare(system_model.FlagModel)
    old = pickle.loads(pickle.dumps(model))
    assert 'loss_kernel' not in old.__dict__ and old.loss_kernel is False                       # what an old checkpoint loads as
    model.loss_kernel = True
    assert pickle.loads(pickle.dumps(model)).loss_kernel is True and copy.deepcopy(model).loss_kernel is True
    assert system_model.FlagModel.loss_kernel is False


def test_frame_losses_refuses_host_tensors():
    from hgn_amd import _lib, features
    with pytest.raises(_lib.HgnError):
        features.frame_losses(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64), (0,))
    with pytest.raises(_lib.HgnError):
        features.frame_losses(torch.zeros(4, 3, requires_grad=True), torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64), (0,), 2)
    assert features.FrameLosses._fields == ('loss', 'per_frame', 'state_error', 'state_per_frame', 'count')
