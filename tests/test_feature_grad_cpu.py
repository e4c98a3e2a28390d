"""Backward of the frame -> graph feature kernels (include/hgn_features.h: hgn_rel_edge_features_bwd, hgn_node_features_bwd,
hgn_normalize_bwd), the parts that need no GPU: exports, argument validation on the host, and the rule that the autograd wrappers
of hgn_amd/features.py are entered only when grad mode is on and a floating input requires grad."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('hgn_rel_edge_features_bwd', 'hgn_node_features_bwd', 'hgn_normalize_bwd')


def test_backward_entries_are_declared_exported_and_bound():
    from hgn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'hgn_features.h')).read()
    declared = set(re.findall(r'^\s*int\s+(hgn_\w+)\s*\(', header, flags=re.M))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib._SIGS[name][1])
        # the ctypes signature has one slot per parameter of the declaration
        decl = header[header.index(f'int {name}('):]
        decl = decl[:decl.index(');')]
        assert len(fn.argtypes) == decl.count(',') + 1, name
    # the forward entries are still there, untouched
    for name in ('hgn_rel_edge_features', 'hgn_node_features', 'hgn_normalize', 'hgn_lincomb3'):
        assert name in declared and name in _lib.EXPORTS


def test_backward_entries_validate_their_arguments_without_gpu():
    """Nothing here reaches a launch: every call is refused, or is an empty no-op, on the host."""
    from hgn_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 96)()
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)        # an aligned host address: looked at, never dereferenced
    err = lambda: lib.hgn_last_error()

    def rel(da=3, db=2, lda=3, ldb=2, ldf=7, n_rows=4, E=5, d_a=p, d_b=p, csr=p, a=p):
        return lib.hgn_rel_edge_features_bwd(p, ldf, p, a, lda, da, p, ldb, db, n_rows, p, p, E, csr, csr, csr, csr, -1, d_a, d_b, None)
    for bad in (dict(da=0), dict(da=4), dict(db=4), dict(lda=2), dict(ldb=1), dict(E=-1), dict(n_rows=-1), dict(E=1 << 31)):
        assert rel(**bad) == -1 and b'hgn_rel_edge_features_bwd' in err(), bad
    assert rel(ldf=6) == -1 and b'ldf' in err()
    assert rel(db=0, ldb=0, ldf=4) == -1 and b'db = 0' in err()                 # d_b asked for, but there is no b
    assert rel(csr=None) == -1 and b'null pointer' in err()
    assert rel(a=None) == -1 and b'null pointer' in err()
    assert rel(n_rows=0) == 0 and rel(d_a=None, d_b=None) == 0                  # nothing to write

    def node(d=3, n_classes=2, ldo=5, ldt=1, N=4, d_out=p, nt=p, mask=-1, d_cur=p):
        return lib.hgn_node_features_bwd(d_out, ldo, d, n_classes, 1, nt, ldt, mask, N, d_cur, p, None)
    for bad in (dict(d=-1), dict(ldo=4), dict(ldt=0), dict(N=-1), dict(d=30, n_classes=3, ldo=33)):
        assert node(**bad) == -1 and b'hgn_node_features_bwd' in err(), bad
    assert node(d_out=None) == -1 and b'null pointer' in err()
    assert node(nt=None, mask=1) == -1 and b'null pointer' in err()
    assert node(N=0) == 0 and node(d=0, n_classes=2, ldo=2) == 0

    def norm(rows=4, F=3, stats=p, d_out=p, d_x=p):
        return lib.hgn_normalize_bwd(d_out, rows, F, stats, stats, stats, 1e-8, 0, d_x, None)
    for bad in (dict(F=0), dict(F=33), dict(rows=-1), dict(stats=None)):
        assert norm(**bad) == -1 and b'hgn_normalize_bwd' in err(), bad
    assert norm(d_out=None) == -1 and norm(d_x=None) == -1
    assert norm(rows=0) == 0


class _FakeLib:
    """Stands for the shared library: every entry succeeds without doing anything (the outputs stay uninitialised)."""

    def __getattr__(self, name):
        return lambda *args: 0


@pytest.fixture
def host_only(monkeypatch):
    """features.py with its launches stubbed out and every autograd wrapper counted: -> {wrapper name: times entered}."""
    from hgn_amd import features
    monkeypatch.setattr(features._lib, 'require_gpu', lambda t: None)
    monkeypatch.setattr(features._lib, 'lib', lambda: _FakeLib())
    monkeypatch.setattr(features._lib, 'stream_ptr', lambda: None)
    entered = {}
    for name in ('_RelEdgeFn', '_NodeFeaturesFn', '_NormalizeFn', '_Lincomb3Fn'):
        fn = getattr(features, name)
        assert issubclass(fn, torch.autograd.Function)

        def counted(*args, _name=name):
            entered[_name] = entered.get(_name, 0) + 1
            return 'entered'
        monkeypatch.setattr(fn, 'apply', counted)
    return entered


def _calls(features, a, b, x):
    s, r = torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])
    stats = [torch.ones(3), torch.ones(3), torch.ones(1)]
    node_type = torch.zeros(4, 1, dtype=torch.int64)
    return [features.rel_edge_features(a, b, s, r, want_len=True),
            features.node_features(a, x, node_type, None, 2),
            features.normalize(x, *stats, 1e-8),
            features.normalize(x, *stats, 1e-8, inverse=True),
            features.lincomb3(a, 2.0, x, 1.0, x, -1.0)]


def test_autograd_wrappers_are_entered_only_when_a_gradient_is_wanted(host_only):
    from hgn_amd import features
    a, b, x = torch.randn(4, 3), torch.randn(4, 2), torch.randn(4, 3)
    # nothing requires grad: the plain launches, no autograd node
    out = _calls(features, a, b, x)
    assert host_only == {} and all(not isinstance(o, str) for o in out)
    # integer tensors cannot require grad; a requirement under no_grad records nothing either
    ag, bg, xg = (t.clone().requires_grad_(True) for t in (a, b, x))
    with torch.no_grad():
        _calls(features, ag, bg, xg)
    assert host_only == {}
    # grad mode on and a floating input that requires grad: every wrapper is entered, once per call
    assert _calls(features, ag, bg, xg) == ['entered'] * 5
    assert host_only == {'_RelEdgeFn': 1, '_NodeFeaturesFn': 1, '_NormalizeFn': 2, '_Lincomb3Fn': 1}
    # one input is enough, whichever it is
    host_only.clear()
    features.rel_edge_features(a, bg, torch.tensor([0]), torch.tensor([1]))
    features.node_features(a, xg, torch.zeros(4, 1, dtype=torch.int64), None, 2)
    features.lincomb3(a, 1.0, x, 1.0, xg, 1.0)
    assert host_only == {'_RelEdgeFn': 1, '_NodeFeaturesFn': 1, '_Lincomb3Fn': 1}


def test_normalizer_accumulates_from_detached_values(host_only, monkeypatch):
    """Normalizer.forward hands _accumulate a tensor without a graph, and normalises the tensor it was given."""
    from hgn_amd import normalizer
    monkeypatch.setattr(normalizer, 'device', torch.device('cpu'))
    nz = normalizer.Normalizer(3, 'test')
    seen = []
    monkeypatch.setattr(nz, '_accumulate', lambda t, reduce_fn=None: seen.append(t))
    x = torch.randn(5, 3, requires_grad=True)
    assert nz(x, True) == 'entered' and host_only == {'_NormalizeFn': 1}
    assert len(seen) == 1 and not seen[0].requires_grad and seen[0].data_ptr() == x.data_ptr()
    y = torch.randn(5, 3)
    nz(y, True)
    assert seen[1] is y and host_only == {'_NormalizeFn': 1}
