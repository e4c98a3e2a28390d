"""CPU-side checks (no GPU) of the backward of the one-launch state update (include/hgn_features.h: hgn_rollout_advance_bwd): the
entry is declared with the forward's citations, exported and bound with one ctypes slot per parameter, and it answers every bad
argument with HGN_E_INVALID and a message that names the entry before any device work."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'hgn_rollout_advance_bwd'
INVALID = -1


def test_abi_rollout_advance_bwd_is_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    assert ENTRY in declared and ENTRY in _lib.EXPORTS and ENTRY in _lib._SIGS
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY) and hasattr(_lib.lib(), ENTRY)
    # the comment block in front of the declaration cites what the forward cites
    decl = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', header, flags=re.S)
    comment = header[:decl.start()].rsplit('/*', 1)[1]
    assert comment.rstrip().endswith('*/')
    for cite in ('flag.py:169-180,243', 'cylinder.py:155-165', 'plate.py:246-257,328'):
        assert cite in comment, cite
    assert len(_lib._SIGS[ENTRY][1]) == len(decl.group(1).split(',')) == 27
    assert _lib._SIGS[ENTRY][0] is C.c_int


def _call(lib, **kw):
    """Host memory stands in for device buffers: every call below must be answered before anything is dereferenced or launched."""
    p = lambda a: C.cast(a, C.c_void_p)
    buf = {name: p((C.c_float * 64)()) for name in ('d_next', 'd_inv', 'sum', 'sq', 'cnt', 'd_net', 'd_cur', 'd_prev', 'd_fb')}
    buf['types'] = p((C.c_int64 * 16)())
    a = dict(d_next=buf['d_next'], ld_dnext=3, d_inv=buf['d_inv'], ld_dinv=3, inv_from=0, F=3, acc_sum=buf['sum'],
             acc_sumsq=buf['sq'], acc_count=buf['cnt'], eps=1e-8, d=3, ca=2.0, cp=-1.0, types=buf['types'], ldt=1, free_mask=1,
             has_fallback=1, rows=10, d_net=buf['d_net'], ld_dnet=3, d_cur=buf['d_cur'], ld_dcur=3, d_prev=buf['d_prev'],
             ld_dprev=3, d_fb=buf['d_fb'], ld_dfb=3)
    a.update(kw)
    return lib.hgn_rollout_advance_bwd(
        a['d_next'], a['ld_dnext'], a['d_inv'], a['ld_dinv'], a['inv_from'], a['F'], a['acc_sum'], a['acc_sumsq'], a['acc_count'],
        a['eps'], a['d'], a['ca'], a['cp'], a['types'], a['ldt'], a['free_mask'], a['has_fallback'], a['rows'], a['d_net'],
        a['ld_dnet'], a['d_cur'], a['ld_dcur'], a['d_prev'], a['ld_dprev'], a['d_fb'], a['ld_dfb'], None)


def test_abi_rollout_advance_bwd_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    no_output = dict(d_net=None, d_cur=None, d_prev=None, d_fb=None)
    bad = {'null acc_sum': dict(acc_sum=None), 'null acc_sumsq': dict(acc_sumsq=None), 'null acc_count': dict(acc_count=None),
           'null node_type': dict(types=None),
           'zero ld_dnext': dict(ld_dnext=0), 'zero ld_dinv': dict(ld_dinv=0), 'zero ld_dinv, no column': dict(ld_dinv=0, inv_from=3),
           'zero ldt': dict(ldt=0), 'zero ld_dnet': dict(ld_dnet=0), 'zero ld_dcur': dict(ld_dcur=0), 'zero ld_dprev': dict(ld_dprev=0),
           'zero ld_dfb': dict(ld_dfb=0),
           'ld_dnext < d': dict(ld_dnext=2), 'ld_dinv < F - inv_from': dict(ld_dinv=1, inv_from=1), 'ld_dnet < F': dict(ld_dnet=2),
           'ld_dcur < d': dict(ld_dcur=2), 'ld_dprev < d': dict(ld_dprev=2), 'ld_dfb < d': dict(ld_dfb=2),
           'd = 0': dict(d=0), 'd > F': dict(d=4, ld_dnext=4, ld_dcur=4, ld_dprev=4, ld_dfb=4),
           'inv_from < 0': dict(inv_from=-1), 'inv_from > F': dict(inv_from=4),
           'F = 0': dict(F=0, d=0), 'F too wide': dict(F=33, ld_dnet=33),
           'negative rows': dict(rows=-1), 'rows >= 2^31': dict(rows=1 << 31),
           'no output': no_output, 'no output and no rows': dict(no_output, rows=0)}
    for what, kw in bad.items():
        assert _call(lib, **kw) == INVALID, what
        assert ENTRY.encode() in lib.hgn_last_error(), what
    # no rows: nothing to do, nothing launched; a matrix that is not given carries no stride
    assert _call(lib, rows=0) == 0
    assert _call(lib, rows=0, d_next=None, ld_dnext=0, d_inv=None, ld_dinv=0, d_cur=None, ld_dcur=0, d_prev=None, ld_dprev=0,
                 d_fb=None, ld_dfb=0, types=None) == 0


def test_advance_state_refuses_host_tensors():
    import pytest
    import torch
    from hgn_amd import _lib, features
    from hgn_amd.normalizer import Normalizer
    with pytest.raises(_lib.HgnError):
        features.advance_state(torch.zeros(4, 3), Normalizer(3, 'n'), torch.zeros(4, 3), 3, 2.0, None, 0.0,
                               torch.zeros(4, 1, dtype=torch.int64), (0,))
