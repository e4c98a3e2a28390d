"""CPU-side checks (no GPU) of the seeded training noise (include/hgn_features.h: hgn_training_noise; features.add_noise;
AbstractSystemModel.add_noise / noise_seed): the statement of tests/noise_statement.py reproduces Random123's known answers and the
sample rows worked out with it; the entry is declared, exported and bound, and refuses bad arguments with HGN_E_INVALID and its name
before any device work; the host functions refuse what they must and do without a launch where none is needed; and the statement's
samples have the moments of independent standard normals, so the cap the device test holds them to can be met."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import noise_statement as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'hgn_training_noise'
INVALID = -1


def test_statement_reproduces_the_known_answers():
    for counter, key, words in NS.KNOWN_ANSWERS:
        assert tuple(int(w) for w in NS.philox4x32_10(*counter, *key)) == words
    # counters broadcast: a column of counters gives the rows of the single calls
    got = NS.philox4x32_10(np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344]), 0, 0)
    assert tuple(int(w) for w in got[0]) == NS.KNOWN_ANSWERS[0][2]


def test_statement_sample_rows():
    z, w, rad = NS.normals(3, 3, 4, 0x1234, 0)
    assert tuple(int(x) for x in w[0]) == (0x4571334f, 0x3e0bdb6f, 0x588a14a7, 0x1acacde2)
    np.testing.assert_allclose(z[0], [0.0774283309, 1.6134964167, 1.1533440236, 0.8906500639], rtol=0, atol=1e-9)
    np.testing.assert_allclose(z[2], [-1.1126776508, -0.4367583304, -1.5904708721, -1.3720805102], rtol=0, atol=1e-9)
    assert rad.shape == (3, 2) and z.shape == (3, 4) and NS.normals(3, 3, 2, 0x1234, 0)[0].shape == (3, 2)
    z, _, _ = NS.normals(6, 3, 4, 0x1234, 0, frame_ids=[5, 2])
    np.testing.assert_allclose(z[4], [0.8611396837, -1.1897371907, 0.3679690188, 0.7190449880], rtol=0, atol=1e-9)
    # frame 2, node 1 wherever the frame sits; an id is read modulo 2^32
    again, _, _ = NS.normals(9, 3, 4, 0x1234, 0, frame_ids=[7, 2 + 2 ** 32, 2])
    assert np.array_equal(again[4], z[4]) and np.array_equal(again[7], z[4])


def test_abi_training_noise_is_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    assert ENTRY in declared and ENTRY in _lib.EXPORTS
    assert hasattr(raw, ENTRY) and hasattr(lib, ENTRY)
    assert 'data/preprocessing.py:84-98' in header
    params = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', header, flags=re.S).group(1)
    assert len(_lib._SIGS[ENTRY][1]) == len(params.split(',')) == 20


def _call(lib, **kw):
    """Host memory stands in for device buffers: every call below must be refused before anything is dereferenced or launched."""
    p = lambda a: C.cast(a, C.c_void_p)
    buf = {name: p((C.c_float * 64)()) for name in ('x', 'target', 'out_x', 'out_target')}
    buf['types'], buf['ids'] = p((C.c_int64 * 16)()), p((C.c_int64 * 16)())
    a = dict(x=buf['x'], ldx=3, d=3, types=buf['types'], ldt=1, free_mask=1, rows=12, rows_per_frame=4, ids=buf['ids'], seed=1, draw=2,
             std=0.003, target=buf['target'], ld_tgt=3, target_scale=0.1, out_x=buf['out_x'], ld_ox=3, out_target=buf['out_target'],
             ld_ot=3)
    a.update(kw)
    return lib.hgn_training_noise(a['x'], a['ldx'], a['d'], a['types'], a['ldt'], a['free_mask'], a['rows'], a['rows_per_frame'],
                                  a['ids'], a['seed'], a['draw'], a['std'], a['target'], a['ld_tgt'], a['target_scale'], a['out_x'],
                                  a['ld_ox'], a['out_target'], a['ld_ot'], None)


def test_abi_training_noise_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = {'d = 0': dict(d=0), 'd = 5': dict(d=5, ldx=5, ld_tgt=5, ld_ox=5, ld_ot=5), 'negative rows': dict(rows=-4),
           'rows >= 2^31': dict(rows=1 << 31, rows_per_frame=1 << 31), 'rows_per_frame = 0': dict(rows_per_frame=0),
           'rows_per_frame < 0': dict(rows_per_frame=-4), 'rows_per_frame does not divide rows': dict(rows_per_frame=5),
           'ldx < d': dict(ldx=2), 'ld_tgt < d': dict(ld_tgt=2), 'ld_ox < d': dict(ld_ox=2), 'ld_ot < d': dict(ld_ot=0),
           'ldt < 1': dict(ldt=0), 'negative std': dict(std=-0.003), 'infinite std': dict(std=float('inf')),
           'nan std': dict(std=float('nan')), 'target without out_target': dict(out_target=None),
           'out_target without target': dict(target=None), 'null x': dict(x=None), 'null node_type': dict(types=None),
           'null out_x': dict(out_x=None)}
    for what, kw in bad.items():
        assert _call(lib, **kw) == INVALID, what
        assert ENTRY.encode() in lib.hgn_last_error(), what
    # no rows: nothing to do, nothing launched; an absent target carries no stride
    assert _call(lib, rows=0) == 0
    assert _call(lib, rows=0, x=None, types=None, out_x=None, ids=None, target=None, out_target=None, ld_tgt=0, ld_ot=0) == 0
    assert _call(lib, rows=0, d=0) == INVALID and _call(lib, rows=0, rows_per_frame=0) == INVALID


def test_add_noise_refuses_host_tensors():
    from hgn_amd import _lib, features
    with pytest.raises(_lib.HgnError):
        features.add_noise(torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64), (0,), 0.003, 1, 0)
    with pytest.raises(_lib.HgnError):
        features.add_noise(torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64), (0,), 0.003, 1, 0, target=torch.zeros(4, 3),
                           target_scale=0.1, rows_per_frame=2, frame_ids=[3, 4])


def _bare(cls, params):
    """A system model with its parameters and nothing else: add_noise reads `_params` and `noise_seed` only."""
    model = cls.__new__(cls)
    torch.nn.Module.__init__(model)
    model._params = params
    return model


def test_noise_seed_is_a_class_default_and_travels_in_pickles():
    from hgn_amd import system_model
    for cls in (system_model.FlagModel, system_model.CylinderModel, system_model.PlateModel):
        assert cls.noise_seed is None and 'noise_seed' not in cls.__dict__             # the base class's one default
        assert callable(getattr(cls, 'add_noise'))
    assert system_model.AbstractSystemModel.__dict__['noise_seed'] is None
    model = _bare(system_model.FlagModel, {'field': 'world_pos', 'noise': 0.003, 'gamma': 0.9})
    assert 'noise_seed' not in model.__dict__ and model.noise_seed is None                # what an old checkpoint loads as
    old = pickle.loads(pickle.dumps(model))
    assert 'noise_seed' not in old.__dict__ and old.noise_seed is None
    model.noise_seed = 2 ** 63 + 5
    assert pickle.loads(pickle.dumps(model)).noise_seed == 2 ** 63 + 5 and copy.deepcopy(model).noise_seed == 2 ** 63 + 5
    assert system_model.FlagModel.noise_seed is None


def test_model_add_noise_without_a_launch_and_without_a_seed():
    from hgn_amd import system_model
    frames = {'world_pos': torch.randn(2, 5, 3), 'target|world_pos': torch.randn(2, 5, 3), 'prev|world_pos': torch.randn(2, 5, 3),
              'node_type': torch.zeros(2, 5, 1, dtype=torch.int64), 'cells': torch.zeros(4, 3, dtype=torch.int64)}
    kept = {k: v.clone() for k, v in frames.items()}
    for params in ({'field': 'world_pos', 'noise': 0, 'gamma': 0.9}, {'field': 'world_pos', 'noise': 0.0, 'gamma': 1},
                   {'field': 'world_pos', 'gamma': 0.9}, {}):
        model = _bare(system_model.FlagModel, params)
        for seed in (None, 3):                                   # a scale of 0 needs no seed: nothing is drawn
            out = model.add_noise(frames, 0, seed=seed)
            assert out is not frames and out.keys() == frames.keys()
            assert all(out[k] is frames[k] for k in frames)
    assert all(torch.equal(frames[k], kept[k]) for k in frames)
    model = _bare(system_model.CylinderModel, {'field': 'velocity', 'noise': 0.02, 'gamma': 0.9})
    with pytest.raises(ValueError, match='seed'):
        model.add_noise({'velocity': torch.zeros(5, 2), 'target|velocity': torch.zeros(5, 2),
                         'node_type': torch.zeros(5, 1, dtype=torch.int64)}, 0)
    model.noise_seed = 7                                        # with a seed the call goes on to the device path, which refuses host tensors
    if not torch.cuda.is_available():
        from hgn_amd import _lib
        with pytest.raises(_lib.HgnError):
            model.add_noise({'velocity': torch.zeros(5, 2), 'target|velocity': torch.zeros(5, 2),
                             'node_type': torch.zeros(5, 1, dtype=torch.int64)}, 0)


@pytest.mark.parametrize('B,N,d,seed,draw', NS.MOMENT_CASES)
def test_moments_of_the_statement(B, N, d, seed, draw):
    """Every standardised figure is at most 4 in magnitude (about 6e-5 per figure under the hypothesis); measured: at most 1.5."""
    z = NS.statement(B * N, N, d, seed, draw)[0]
    figures = NS.moment_figures(z, NS.statement(B * N, N, d, seed, draw + 1)[0], NS.statement(B * N, N, d, seed + 1, draw)[0], B, N)
    print(f'moments of the statement [{B} x {N} x {d}, seed {seed:#x}, draw {draw:#x}]: '
          + ', '.join(f'{k} {v:+.2f}' for k, v in figures.items()))
    expected = 7 + min(d - 1, 2)
    assert len(figures) == expected
    assert all(abs(v) <= NS.MOMENT_CAP for v in figures.values()), figures
