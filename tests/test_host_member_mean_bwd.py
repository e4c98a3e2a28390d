"""CPU-side checks (no GPU) of the backward of the connector's cluster mean (include/hgn_features.h: hgn_member_mean_bwd): the entry
is declared with the lines it differentiates, exported and bound with one ctypes slot per parameter, and it answers every bad
argument with HGN_E_INVALID and a message that names the entry before any device work."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'hgn_member_mean_bwd'
INVALID = -1


def test_abi_member_mean_bwd_is_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    assert ENTRY in declared and ENTRY in _lib.EXPORTS and ENTRY in _lib._SIGS
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY) and hasattr(_lib.lib(), ENTRY)
    decl = re.search(r'int\s+' + ENTRY + r'\s*\(([^;]*)\)\s*;', header, flags=re.S)
    comment = header[:decl.start()].rsplit('/*', 1)[1]
    assert comment.rstrip().endswith('*/')
    for cite in ('hierarchical_connector.py:39-45', 'rmp.py', 'means_all = ops.aggregate('):
        assert cite in comment, cite
    # the cited line is the one HierarchicalConnector.run still holds
    rmp = open(os.path.join(ROOT, 'hyper-graph-nets_amd', 'hgn_amd', 'rmp.py')).read()
    assert "means_all = ops.aggregate([both], [(t.node_perm, t.csr.rowptr, t.csr.seg)], ('mean',))" in rmp
    assert len(_lib._SIGS[ENTRY][1]) == len(decl.group(1).split(',')) == 13
    assert _lib._SIGS[ENTRY][0] is C.c_int


def _call(lib, **kw):
    """Host memory stands in for device buffers: every call below must be answered before anything is dereferenced or launched."""
    p = lambda a: C.cast(a, C.c_void_p)
    a = dict(d_mean=p((C.c_float * 64)()), ld_dmean=3, D=3, seg_rowptr=p((C.c_int32 * 8)()), S=4, item_seg=p((C.c_int32 * 16)()),
             node_rowptr=p((C.c_int32 * 16)()), node_items=p((C.c_int32 * 16)()), rows=10, M=8, d_data=p((C.c_float * 64)()), ld=3)
    a.update(kw)
    return lib.hgn_member_mean_bwd(a['d_mean'], a['ld_dmean'], a['D'], a['seg_rowptr'], a['S'], a['item_seg'], a['node_rowptr'],
                                   a['node_items'], a['rows'], a['M'], a['d_data'], a['ld'], None)


def test_abi_member_mean_bwd_refuses_bad_arguments_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    bad = {'null d_mean': dict(d_mean=None), 'null seg_rowptr': dict(seg_rowptr=None), 'null item_seg': dict(item_seg=None),
           'null node_rowptr': dict(node_rowptr=None), 'null node_items': dict(node_items=None), 'null d_data': dict(d_data=None),
           'null d_data, no members': dict(d_data=None, M=0),
           'D = 0': dict(D=0), 'D < 0': dict(D=-1), 'ld < D': dict(ld=2), 'ld = 0': dict(ld=0), 'ld_dmean < D': dict(ld_dmean=2),
           'ld_dmean = 0': dict(ld_dmean=0), 'ld < D, no rows': dict(ld=2, rows=0),
           'negative rows': dict(rows=-1), 'negative M': dict(M=-1), 'negative S': dict(S=-1),
           'rows >= 2^31': dict(rows=1 << 31), 'M >= 2^31': dict(M=1 << 31), 'members without a segment': dict(S=0)}
    for what, kw in bad.items():
        assert _call(lib, **kw) == INVALID, what
        assert ENTRY.encode() in lib.hgn_last_error(), what
    # no rows: nothing to do, nothing launched; empty tensors carry null pointers
    assert _call(lib, rows=0) == 0
    assert _call(lib, rows=0, M=0, S=0, d_mean=None, seg_rowptr=None, item_seg=None, node_rowptr=None, node_items=None, d_data=None) == 0
