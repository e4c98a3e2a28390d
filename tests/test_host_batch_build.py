"""CPU-side checks (no GPU) of the batched frame -> graph step: the C ABI of the radius query over a batch of graphs
(include/hgn_features.h: hgn_radius_edges_batch_*) answers bad arguments with HGN_E_INVALID and a message that names the entry,
before any device work; `flatten_frames` turns stacked frames into the rows of their disjoint union."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('hgn_radius_edges_batch_workspace_bytes', 'hgn_radius_edges_batch_count', 'hgn_radius_edges_batch_fill')
INVALID = -1


def test_abi_batch_entries_are_exported_and_declared():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(raw, name) and hasattr(lib, name), name
    assert 'plate.py:84-110' in header and 'MeshSimulator.py:159-234' in header


def test_abi_batch_workspace_bytes_is_monotone_and_checks_the_shape():
    from hgn_amd import _lib
    lib = _lib.lib()
    nb = C.c_size_t(0)
    last = 0
    for B, N in ((1, 0), (1, 1), (1, 158), (3, 158), (21, 158), (128, 158), (128, 1600), (1000, 100000)):
        assert lib.hgn_radius_edges_batch_workspace_bytes(B, N, C.byref(nb)) == 0, (B, N)
        assert nb.value >= (B * N + 1) * 4 and nb.value >= last, (B, N, nb.value, last)
        last = nb.value
    one = C.c_size_t(0)                                    # the same rows, split differently: the same scratch
    assert lib.hgn_radius_edges_batch_workspace_bytes(1, 3 * 158, C.byref(one)) == 0
    assert lib.hgn_radius_edges_batch_workspace_bytes(3, 158, C.byref(nb)) == 0 and nb.value == one.value
    assert lib.hgn_radius_edges_batch_workspace_bytes(1, 0x7ffffffe, C.byref(nb)) == 0
    for B, N in ((0, 10), (-1, 10), (2, -1), (1, 0x7fffffff), (2, 0x40000000), (1 << 40, 1 << 40)):
        assert lib.hgn_radius_edges_batch_workspace_bytes(B, N, C.byref(nb)) == INVALID, (B, N)
        assert b'hgn_radius_edges_batch_workspace_bytes' in lib.hgn_last_error()
    assert lib.hgn_radius_edges_batch_workspace_bytes(2, 10, None) == INVALID


def _buffers():
    """Host memory standing in for device buffers: every call below must be refused before anything is dereferenced."""
    pos = (C.c_float * 60)()
    types = (C.c_int64 * 20)()
    off = (C.c_int32 * 21)()
    goff = (C.c_int32 * 3)()
    ids = (C.c_int64 * 8)()
    ws = (C.c_char * 64)()
    rowptr = (C.c_int32 * 11)()
    p = lambda a: C.cast(a, C.c_void_p)
    return p(pos), p(types), p(off), p(goff), p(ids), p(ws), p(rowptr)


def test_abi_batch_count_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    pos, types, off, goff, ids, ws, rowptr = _buffers()
    tot = C.c_int64(7)
    big = 1 << 30

    def count(pos=pos, ld=3, d=3, types=types, ldt=1, B=2, N=10, radius=0.03, rowptr=None, nbr=None, off=off, goff=goff,
              tot=C.byref(tot), ws=ws, ws_bytes=big):
        return lib.hgn_radius_edges_batch_count(pos, ld, d, types, ldt, B, N, radius, 1, 0, rowptr, nbr, off, goff, tot, ws,
                                                ws_bytes, None)
    bad = {'n_graphs < 1': dict(B=0), 'n_graphs < 0': dict(B=-3), 'nodes_per_graph < 0': dict(N=-1),
           'too many rows': dict(B=2, N=0x40000000), 'rows overflow': dict(B=1 << 40, N=1 << 40),
           'd = 0': dict(d=0), 'd = 4': dict(d=4, ld=4), 'ld < d': dict(ld=2), 'ldt < 1': dict(ldt=0),
           'negative radius': dict(radius=-1.0), 'nan radius': dict(radius=float('nan')),
           'null pos': dict(pos=None), 'null node_type': dict(types=None),
           'rowptr without nbr': dict(rowptr=rowptr), 'nbr without rowptr': dict(nbr=rowptr),
           'null offsets': dict(off=None), 'null total': dict(tot=None),
           'null workspace': dict(ws=None), 'workspace too small': dict(ws_bytes=64)}
    for what, kw in bad.items():
        assert count(**kw) == INVALID, what
        assert b'hgn_radius_edges_batch_count' in lib.hgn_last_error(), what
    assert tot.value == 7                                   # nothing was written


def test_abi_batch_fill_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    pos, types, off, goff, ids, ws, rowptr = _buffers()

    def fill(pos=pos, ld=3, d=3, types=types, ldt=1, B=2, N=10, radius=0.03, rowptr=None, nbr=None, off=off, s=ids, r=ids):
        return lib.hgn_radius_edges_batch_fill(pos, ld, d, types, ldt, B, N, radius, 1, 0, rowptr, nbr, off, s, r, None)
    bad = {'n_graphs < 1': dict(B=0), 'nodes_per_graph < 0': dict(N=-1), 'too many rows': dict(B=2, N=0x40000000),
           'd = 4': dict(d=4, ld=4), 'ld < d': dict(ld=2), 'ldt < 1': dict(ldt=0), 'negative radius': dict(radius=-1.0),
           'null pos': dict(pos=None), 'null node_type': dict(types=None), 'rowptr without nbr': dict(rowptr=rowptr),
           'null offsets': dict(off=None), 'null senders': dict(s=None), 'null receivers': dict(r=None)}
    for what, kw in bad.items():
        assert fill(**kw) == INVALID, what
        assert b'hgn_radius_edges_batch_fill' in lib.hgn_last_error(), what
    assert fill(N=0) == 0                                   # an empty union: nothing to write, nothing launched


def test_radius_edges_batch_refuses_host_tensors():
    from hgn_amd import _lib, features
    with pytest.raises(_lib.HgnError):
        features.radius_edges_batch(torch.zeros(6, 3), torch.zeros(6, 1, dtype=torch.int64), 2, 0.03, 1, 0)


@pytest.mark.parametrize('kind', ['flag', 'cylinder', 'plate'])
def test_flatten_frames_shapes_identity_and_row_order(kind):
    from hgn_amd import system_model
    B = 3
    make = {'flag': lambda i: synth.flag_frame(seed=i, nx=5, ny=4), 'cylinder': lambda i: synth.cylinder_frame(seed=i, nx=5, ny=4),
            'plate': lambda i: synth.plate_frame(seed=i)}[kind]
    frames = [make(10 + i) for i in range(B)]
    N = frames[0]['node_type'].shape[0]
    shared = ('cells', 'mesh_pos')
    stacked = {k: (frames[0][k] if k in shared else torch.stack([f[k] for f in frames])) for k in frames[0]}
    cls = {'flag': system_model.FlagModel, 'cylinder': system_model.CylinderModel, 'plate': system_model.PlateModel}[kind]
    for flatten in (system_model.AbstractSystemModel.flatten_frames, cls.flatten_frames):
        flat = flatten(stacked)
        assert set(flat) == set(stacked)
        for k in stacked:
            if k in shared:
                assert flat[k] is stacked[k], k                              # shared entries: the same objects
            else:
                assert flat[k].shape == (B * N,) + tuple(frames[0][k].shape[1:]), k
                assert flat[k].dtype == frames[0][k].dtype
                assert torch.equal(flat[k], torch.cat([f[k] for f in frames])), k
    # a mesh_pos given per frame is a per-node series like the others
    stacked['mesh_pos'] = torch.stack([f['mesh_pos'] for f in frames])
    flat = system_model.AbstractSystemModel.flatten_frames(stacked)
    assert torch.equal(flat['mesh_pos'], torch.cat([f['mesh_pos'] for f in frames]))
    assert flat['cells'] is stacked['cells']
