"""CPU-side checks (no GPU) of ragged batches -- frames of different meshes in one batch (include/hgn_features.h:
hgn_radius_edges_ragged_*, hgn_training_noise_ragged, hgn_frame_losses_ragged_*; features.frame_losses / add_noise with
``frame_rows``, features.radius_edges_ragged; AbstractSystemModel.concat_frames and its neighbours): the entries are declared,
exported and bound with matching argument counts; each refuses a bad host ``frame_rows``, a null ``frame_ptr`` and everything its
uniform neighbour refuses with HGN_E_INVALID and its own name before any device work (host memory stands in for device buffers); the
loss workspace grows with the number of frames and with the largest frame; and the Python layer keeps the two ways to split rows
apart and lays the union out as documented."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'hgn_radius_edges_ragged_workspace_bytes': 4, 'hgn_radius_edges_ragged_count': 20, 'hgn_radius_edges_ragged_fill': 18,
           'hgn_training_noise_ragged': 22, 'hgn_frame_losses_ragged_workspace_bytes': 4, 'hgn_frame_losses_ragged': 31,
           'hgn_frame_losses_ragged_bwd': 19}
INVALID = -1


def _p(a):
    return C.cast(a, C.c_void_p)


def _sizes(*values):
    return (C.c_int64 * len(values))(*values)


def _f(n=96):
    return _p((C.c_float * n)())


PTR = _p((C.c_int32 * 8)())                 # stands for the device frame_ptr: never read by a call that is refused
# what every ragged entry refuses about the batch itself; rows = 12 in the callers below
BAD_BATCH = {'B = 0': dict(B=0), 'B < 0': dict(B=-2), 'a frame of 0 rows': dict(sizes=_sizes(4, 0, 8)),
             'a negative frame': dict(sizes=_sizes(16, -8, 4)), 'a sum below rows': dict(sizes=_sizes(4, 4, 3)),
             'a sum above rows': dict(sizes=_sizes(4, 4, 5)), 'fewer frames than the sum needs': dict(B=2),
             'rows = 0': dict(rows=0), 'negative rows': dict(rows=-12), 'rows >= 2^31': dict(rows=1 << 31, sizes=_sizes(1 << 31), B=1),
             'a frame that overflows the sum': dict(sizes=_sizes(1 << 62, 1 << 62, 12)), 'null frame_rows': dict(sizes=None),
             'null frame_ptr': dict(ptr=None)}


def test_abi_ragged_entries_are_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for entry, n_args in ENTRIES.items():
        assert entry in declared and entry in _lib.EXPORTS and entry in _lib._SIGS, entry
        assert hasattr(raw, entry) and hasattr(lib, entry), entry
        params = re.search(r'int\s+' + entry + r'\s*\(([^;]*)\)\s*;', header, flags=re.S).group(1)
        assert len(_lib._SIGS[entry][1]) == len(params.split(',')) == n_args, entry
        assert _lib._SIGS[entry][0] is C.c_int
        assert 'const int64_t* frame_rows' in params, entry                          # the host half of the batch
        assert ('const int32_t* frame_ptr' in params) == (not entry.endswith('workspace_bytes')), entry
    flat = re.sub(r'\s*\n\s*\*\s*', ' ', header)
    for phrase in ('entries f < B have the bits that hgn_frame_losses gives for that frame alone',
                   'with all N_b equal, all B+1 entries and the whole backward have the bits of the uniform entries',
                   'never a read or write outside the caller\'s buffers', 'no atomics',
                   "a row's sample stays a function of (seed, draw, frame id, node) alone", 'neighbour CSR of the UNION'):
        assert phrase in flat, phrase
    # the reference lines the uniform entries cite
    for cite in ('plate.py:84-110', 'MeshSimulator.py:159-234', 'data/preprocessing.py:84-98', 'flag.py:146-167', 'MeshSimulator.py:151-156'):
        assert header.count(cite) >= 2, cite


def _losses(lib, **kw):
    ws = (C.c_double * 64)()
    a = dict(net_out=_f(), ld_out=3, target=_f(), ld_tgt=3, F=3, types=_p((C.c_int64 * 32)()), ldt=1, free_mask=1, rows=12,
             sizes=_sizes(4, 4, 4), ptr=PTR, B=3, acc_sum=_f(), acc_sumsq=_f(), acc_count=_f(), eps=1e-8, cur=_f(), ld_cur=3, d=3, ca=2.0,
             prev=_f(), ld_prev=3, cp=-1.0, state_target=_f(), ld_st=3, loss=_f(), state_err=_f(), count=_p((C.c_int64 * 8)()), ws=_p(ws),
             ws_bytes=C.sizeof(ws), keep=ws)
    a.update(kw)
    return lib.hgn_frame_losses_ragged(a['net_out'], a['ld_out'], a['target'], a['ld_tgt'], a['F'], a['types'], a['ldt'], a['free_mask'],
                                       a['rows'], a['sizes'], a['ptr'], a['B'], a['acc_sum'], a['acc_sumsq'], a['acc_count'], a['eps'],
                                       a['cur'], a['ld_cur'], a['d'], a['ca'], a['prev'], a['ld_prev'], a['cp'], a['state_target'],
                                       a['ld_st'], a['loss'], a['state_err'], a['count'], a['ws'], a['ws_bytes'], None)


NO_STATE = dict(acc_sum=None, acc_sumsq=None, acc_count=None, cur=None, prev=None, state_target=None, state_err=None)


def test_abi_frame_losses_ragged_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    ws = (C.c_double * 64)()
    bad = dict(BAD_BATCH)
    bad.update({                                                              # every refusal of hgn_frame_losses
        'F = 0': dict(F=0), 'F = 33': dict(F=33, ld_out=33, ld_tgt=33), 'd = 0': dict(d=0), 'd > F': dict(d=4, ld_cur=4, ld_st=4, ld_prev=4),
        'ld_out < F': dict(ld_out=2), 'ld_tgt < F': dict(ld_tgt=2), 'ld_cur < d': dict(ld_cur=2), 'ld_prev < d': dict(ld_prev=0),
        'ld_st < d': dict(ld_st=2), 'ldt < 1': dict(ldt=0),
        'state part without acc_sum': dict(acc_sum=None), 'state part without acc_sumsq': dict(acc_sumsq=None),
        'state part without acc_count': dict(acc_count=None), 'state part without cur': dict(cur=None),
        'state part without state_target': dict(state_target=None), 'prev alone': dict(NO_STATE, prev=_f()),
        'state part without state_err': dict(state_err=None), 'state_err without a state part': dict(NO_STATE, state_err=_f(8)),
        'null net_out': dict(net_out=None), 'null target': dict(target=None), 'null node_type': dict(types=None),
        'null loss': dict(loss=None), 'null count': dict(count=None), 'null workspace': dict(ws=None),
        'workspace too small': dict(ws_bytes=3 * 3 * 8 - 1), 'workspace misaligned': dict(ws=C.c_void_p(C.addressof(ws) + 4))})
    for what, kw in bad.items():
        assert _losses(lib, **kw) == INVALID, what
        assert b'hgn_frame_losses_ragged' in lib.hgn_last_error(), what


def _losses_bwd(lib, **kw):
    a = dict(net_out=_f(), ld_out=3, target=_f(), ld_tgt=3, F=3, types=_p((C.c_int64 * 32)()), ldt=1, free_mask=1, rows=12,
             sizes=_sizes(4, 4, 4), ptr=PTR, B=3, count=_p((C.c_int64 * 8)()), g=_f(8), d_net=_f(), ld_dnet=3, d_target=_f(), ld_dtgt=3)
    a.update(kw)
    return lib.hgn_frame_losses_ragged_bwd(a['net_out'], a['ld_out'], a['target'], a['ld_tgt'], a['F'], a['types'], a['ldt'],
                                           a['free_mask'], a['rows'], a['sizes'], a['ptr'], a['B'], a['count'], a['g'], a['d_net'],
                                           a['ld_dnet'], a['d_target'], a['ld_dtgt'], None)


def test_abi_frame_losses_ragged_bwd_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = dict(BAD_BATCH)
    bad.update({'F = 0': dict(F=0), 'F = 33': dict(F=33, ld_out=33, ld_tgt=33, ld_dnet=33, ld_dtgt=33), 'ld_out < F': dict(ld_out=2),
                'ld_tgt < F': dict(ld_tgt=2), 'ld_dnet < F': dict(ld_dnet=2), 'ld_dtgt < F': dict(ld_dtgt=0), 'ldt < 1': dict(ldt=0),
                'no output': dict(d_net=None, d_target=None), 'null net_out': dict(net_out=None), 'null target': dict(target=None),
                'null node_type': dict(types=None), 'null count': dict(count=None)})
    for what, kw in bad.items():
        assert _losses_bwd(lib, **kw) == INVALID, what
        assert b'hgn_frame_losses_ragged_bwd' in lib.hgn_last_error(), what


def _noise(lib, **kw):
    buf = {name: _f(64) for name in ('x', 'target', 'out_x', 'out_target')}
    a = dict(x=buf['x'], ldx=3, d=3, types=_p((C.c_int64 * 16)()), ldt=1, free_mask=1, rows=12, sizes=_sizes(5, 6, 1), ptr=PTR, B=3,
             ids=_p((C.c_int64 * 16)()), seed=1, draw=2, std=0.003, target=buf['target'], ld_tgt=3, target_scale=0.1, out_x=buf['out_x'],
             ld_ox=3, out_target=buf['out_target'], ld_ot=3)
    a.update(kw)
    return lib.hgn_training_noise_ragged(a['x'], a['ldx'], a['d'], a['types'], a['ldt'], a['free_mask'], a['rows'], a['sizes'], a['ptr'],
                                         a['B'], a['ids'], a['seed'], a['draw'], a['std'], a['target'], a['ld_tgt'], a['target_scale'],
                                         a['out_x'], a['ld_ox'], a['out_target'], a['ld_ot'], None)


def test_abi_training_noise_ragged_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = dict(BAD_BATCH)
    bad.update({'d = 0': dict(d=0), 'd = 5': dict(d=5, ldx=5, ld_tgt=5, ld_ox=5, ld_ot=5), 'ldx < d': dict(ldx=2), 'ld_tgt < d': dict(ld_tgt=2),
                'ld_ox < d': dict(ld_ox=2), 'ld_ot < d': dict(ld_ot=0), 'ldt < 1': dict(ldt=0), 'negative std': dict(std=-0.003),
                'infinite std': dict(std=float('inf')), 'nan std': dict(std=float('nan')),
                'target without out_target': dict(out_target=None), 'out_target without target': dict(target=None),
                'null x': dict(x=None), 'null node_type': dict(types=None), 'null out_x': dict(out_x=None)})
    for what, kw in bad.items():
        assert _noise(lib, **kw) == INVALID, what
        assert b'hgn_training_noise_ragged' in lib.hgn_last_error(), what


def _radius_buffers():
    return dict(pos=_f(60), types=_p((C.c_int64 * 20)()), off=_p((C.c_int32 * 21)()), goff=_p((C.c_int32 * 4)()),
                ids=_p((C.c_int64 * 8)()), ws=_p((C.c_char * 64)()), rowptr=_p((C.c_int32 * 21)()))


def test_abi_radius_edges_ragged_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    b = _radius_buffers()
    tot = C.c_int64(7)

    def count(pos=b['pos'], ld=3, d=3, types=b['types'], ldt=1, rows=12, sizes=_sizes(7, 1, 4), ptr=PTR, B=3, radius=0.03, rowptr=None,
              nbr=None, off=b['off'], goff=b['goff'], tot=C.byref(tot), ws=b['ws'], ws_bytes=1 << 30):
        return lib.hgn_radius_edges_ragged_count(pos, ld, d, types, ldt, rows, sizes, ptr, B, radius, 1, 0, rowptr, nbr, off, goff, tot,
                                                 ws, ws_bytes, None)

    def fill(pos=b['pos'], ld=3, d=3, types=b['types'], ldt=1, rows=12, sizes=_sizes(7, 1, 4), ptr=PTR, B=3, radius=0.03, rowptr=None,
             nbr=None, off=b['off'], s=b['ids'], r=b['ids']):
        return lib.hgn_radius_edges_ragged_fill(pos, ld, d, types, ldt, rows, sizes, ptr, B, radius, 1, 0, rowptr, nbr, off, s, r, None)
    shared = dict(BAD_BATCH)
    shared['rows = 0x7fffffff'] = dict(rows=0x7fffffff, sizes=_sizes(0x7fffffff), B=1)         # the radius query stops one row earlier
    shared.update({'d = 0': dict(d=0), 'd = 4': dict(d=4, ld=4), 'ld < d': dict(ld=2), 'ldt < 1': dict(ldt=0),
                   'negative radius': dict(radius=-1.0), 'nan radius': dict(radius=float('nan')), 'null pos': dict(pos=None),
                   'null node_type': dict(types=None), 'rowptr without nbr': dict(rowptr=b['rowptr']),
                   'nbr without rowptr': dict(nbr=b['rowptr']), 'null offsets': dict(off=None)})
    for what, kw in dict(shared, **{'null total': dict(tot=None), 'null workspace': dict(ws=None),
                                    'workspace too small': dict(ws_bytes=64)}).items():
        assert count(**kw) == INVALID, what
        assert b'hgn_radius_edges_ragged_count' in lib.hgn_last_error(), what
    assert tot.value == 7                                   # nothing was written
    for what, kw in dict(shared, **{'null senders': dict(s=None), 'null receivers': dict(r=None)}).items():
        assert fill(**kw) == INVALID, what
        assert b'hgn_radius_edges_ragged_fill' in lib.hgn_last_error(), what


def _bytes(fn, rows, sizes):
    nb = C.c_size_t(0)
    rc = fn(rows, _sizes(*sizes) if sizes is not None else None, len(sizes) if sizes is not None else 1, C.byref(nb))
    return rc, nb.value


def test_loss_workspace_grows_with_frames_and_with_the_largest_frame():
    """One partial triple per workgroup of a grid of B x ceil(max N_b / chunk): monotone in B at a fixed largest frame and in the
    largest frame at a fixed B, whatever the other frames hold; with equal frames it is the uniform entry's size."""
    from hgn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    chunk = int(re.search(r'#define\s+HGN_LOSS_CHUNK_ROWS\s+(\d+)', header).group(1))
    ragged = lib.hgn_frame_losses_ragged_workspace_bytes
    largest = [1, 2, chunk - 1, chunk, chunk + 1, 3000, 100000]
    for big in largest:
        got = [_bytes(ragged, big + (B - 1), (big,) + (1,) * (B - 1)) for B in (1, 2, 3, 128)]
        assert all(rc == 0 and nb % 8 == 0 and nb > 0 for rc, nb in got), big
        assert all(a[1] < b[1] for a, b in zip(got, got[1:])), big
    for B in (1, 3, 128):
        got = [_bytes(ragged, big + (B - 1), (1,) * (B - 1) + (big,))[1] for big in largest]
        assert all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[0], B
    assert _bytes(ragged, chunk + 2, (chunk + 1, 1))[1] > _bytes(ragged, chunk + 1, (chunk, 1))[1]       # a second chunk needs room
    assert _bytes(ragged, 12, (4, 4, 4)) == (0, 3 * 3 * 8) == _bytes(ragged, 12, (1, 4, 7))               # 3 frames x 1 chunk x 3 doubles
    uniform = C.c_size_t(0)
    for rows, rpf in ((12, 4), (3 * 300, 300), (5 * 257, 257)):
        assert lib.hgn_frame_losses_workspace_bytes(rows, rpf, C.byref(uniform)) == 0
        assert _bytes(ragged, rows, (rpf,) * (rows // rpf)) == (0, uniform.value)
    for rows, sizes in ((12, ()), (12, (4, 0, 8)), (12, (4, 4, 3)), (1 << 31, (1 << 31,)), (12, None), (0, (1,)), (-3, (1, 2))):
        rc = ragged(rows, _sizes(*sizes) if sizes is not None else None, len(sizes) if sizes is not None else 1, C.byref(uniform))
        assert rc == INVALID and b'hgn_frame_losses_ragged_workspace_bytes' in lib.hgn_last_error(), (rows, sizes)
    assert ragged(12, _sizes(4, 8), 2, None) == INVALID


def test_radius_workspace_follows_the_rows_and_checks_the_batch():
    from hgn_amd import _lib
    lib = _lib.lib()
    ragged = lib.hgn_radius_edges_ragged_workspace_bytes
    batch = C.c_size_t(0)
    last = 0
    for sizes in ((1,), (158,), (58, 158, 32), (58, 158, 32, 58), (1600,) * 128):
        rc, nb = _bytes(ragged, sum(sizes), sizes)
        assert rc == 0 and nb >= (sum(sizes) + 1) * 4 and nb >= last, sizes
        last = nb
    assert lib.hgn_radius_edges_batch_workspace_bytes(3, 158, C.byref(batch)) == 0                   # the same rows: the same scratch
    assert _bytes(ragged, 3 * 158, (158, 158, 158)) == (0, batch.value) == _bytes(ragged, 3 * 158, (1, 472, 1))
    assert _bytes(ragged, 0x7ffffffe, (0x7ffffffe,))[0] == 0
    for rows, sizes in ((12, ()), (12, (4, 0, 8)), (12, (4, 4, 3)), (0x7fffffff, (0x7fffffff,)), (12, None), (0, (1,))):
        rc = ragged(rows, _sizes(*sizes) if sizes is not None else None, len(sizes) if sizes is not None else 1, C.byref(batch))
        assert rc == INVALID and b'hgn_radius_edges_ragged_workspace_bytes' in lib.hgn_last_error(), (rows, sizes)
    assert ragged(12, _sizes(4, 8), 2, None) == INVALID


def test_frame_rows_excludes_rows_per_frame_and_host_tensors_are_refused():
    from hgn_amd import _lib, features
    out, types = torch.zeros(6, 3), torch.zeros(6, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match='not both'):
        features.frame_losses(out, out, types, (0,), rows_per_frame=3, frame_rows=(2, 4))
    with pytest.raises(ValueError, match='not both'):
        features.add_noise(out, types, (0,), 0.003, 1, 0, rows_per_frame=3, frame_rows=(2, 4))
    with pytest.raises(_lib.HgnError):                                             # no CPU fallback for the ragged form either
        features.frame_losses(out, out, types, (0,), frame_rows=(2, 4))
    with pytest.raises(_lib.HgnError):
        features.add_noise(out, types, (0,), 0.003, 1, 0, frame_ids=[3, 4], frame_rows=(2, 4))
    with pytest.raises(_lib.HgnError):
        features.radius_edges_ragged(out, types, (2, 4), 0.03, 1, 0)
    for bad in ((), (2, 3), (2, 0, 4), (7, -1)):                                    # the Python layer checks the split before the C ABI
        with pytest.raises(ValueError, match='frame_rows'):
            features._ragged(bad, 6, torch.device('cpu'), 'test')


MAKE = {'flag': lambda seed, nx, ny: synth.flag_frame(seed=seed, nx=nx, ny=ny),
        'cylinder': lambda seed, nx, ny: synth.cylinder_frame(seed=seed, nx=nx, ny=ny),
        'plate': lambda seed, nx, ny: synth.plate_frame(seed=seed, nx=nx, ny=ny, nz=2, obstacle=(2, 2, 2))}


@pytest.mark.parametrize('kind', ['flag', 'cylinder', 'plate'])
def test_concat_frames_layout(kind):
    """Per-node series are concatenated in frame order, `cells` is the list of the frames' own tensors, frame_rows counts the rows."""
    from hgn_amd import system_model
    frames = [MAKE[kind](30 + i, nx, ny) for i, (nx, ny) in enumerate(((3, 3), (5, 4), (4, 3)))]
    cls = {'flag': system_model.FlagModel, 'cylinder': system_model.CylinderModel, 'plate': system_model.PlateModel}[kind]
    for concat in (system_model.AbstractSystemModel.concat_frames, cls.concat_frames):
        flat, frame_rows = concat(frames)
        assert frame_rows == tuple(f['node_type'].shape[0] for f in frames) and len(set(frame_rows)) == 3
        assert isinstance(frame_rows, tuple) and all(type(n) is int for n in frame_rows)
        assert set(flat) == set(frames[0])
        assert isinstance(flat['cells'], list) and all(a is f['cells'] for a, f in zip(flat['cells'], frames))
        first = 0
        for f, n in zip(frames, frame_rows):
            for name in f:
                if name != 'cells':
                    assert flat[name].shape == (sum(frame_rows),) + tuple(f[name].shape[1:]) and flat[name].dtype == f[name].dtype, name
                    assert torch.equal(flat[name][first:first + n], f[name]), name
            first += n
    with pytest.raises(ValueError):
        system_model.AbstractSystemModel.concat_frames([])


def test_ragged_methods_exist_on_every_model_and_caches_do_not_travel():
    import copy
    import pickle
    from hgn_amd import system_model
    for cls in (system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel):
        for method in ('concat_frames', 'build_graph_frames', 'expand_graph_frames', 'rollout_frames'):
            assert callable(getattr(cls, method)), (cls, method)
    model = system_model.FlagModel.__new__(system_model.FlagModel)
    torch.nn.Module.__init__(model)
    model._meshes, model._unions = [('mesh', 'edges')], [('rows', 'meshes', 'union')]
    for twin in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):
        assert twin._meshes is None and twin._unions is None


@pytest.mark.parametrize('switch', ['_rmp', '_balancer'])
def test_expand_graph_frames_refuses_per_mesh_stages(switch):
    """A connector or a balancer has no ragged form: HgnError that names the per-frame route, before the graph is looked at."""
    from hgn_amd import _lib, system_model
    model = system_model.CylinderModel.__new__(system_model.CylinderModel)
    torch.nn.Module.__init__(model)
    model._rmp = model._balancer = False
    setattr(model, switch, True)
    with pytest.raises(_lib.HgnError, match='per-frame route.*build_graph and expand_graph'):
        model.expand_graph_frames(None, (3, 4), 0, 1, False)
    model._rmp = model._balancer = False
    graph = system_model.MultiGraphWithPos(node_features=['n'], edge_sets=['e'], target_feature=None, mesh_features=None, model_type='x',
                                           node_dynamic=None, unnormalized_edges=None, obstacle_nodes=None)
    plain = model.expand_graph_frames(graph, (3, 4), 0, 1, False)
    assert isinstance(plain, system_model.MultiGraph) and plain.node_features == ['n'] and plain.edge_sets == ['e']
