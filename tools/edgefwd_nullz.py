"""One training edge forward launch (ops.edge_block, `sum` aggregate in the kernel) with and without the z1 / z2 saves: the
weights trainable against frozen, alternated in one process, device events around each forward.  Prints one JSON line.
Not part of the product or the tests."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'hyper-graph-nets_amd')):
    sys.path.insert(0, p)
import torch
from hgn_amd import ops, topology

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1188096)
ap.add_argument('--warm', type=int, default=3)
ap.add_argument('--iters', type=int, default=50)
ap.add_argument('--precision', default='fp32')
a = ap.parse_args()
E = a.rows
N = (E + 5) // 6
dev = torch.device('cuda')
gen = torch.Generator().manual_seed(0)
topo = topology.EdgeTopology(torch.randint(0, N, (E,), generator=gen).to(dev), (torch.arange(E) // 6).to(dev), N, dev)
shapes = [(128, 384), (128,), (128, 128), (128,), (128, 128), (128,), (128,), (128,)]
wts = [(torch.randn(*s, generator=gen) * (0.05 if len(s) == 2 else 0.1) + (1.0 if i == 6 else 0.0)).to(dev) for i, s in enumerate(shapes)]
w = ops.MLPWeights(*wts)
h = torch.randn(N, 128, device=dev, requires_grad=True)
e = torch.randn(E, 128, device=dev, requires_grad=True)
times = {False: [], True: []}
with ops.using(ops.Context(precision=a.precision)):
    for it in range(a.warm + a.iters):
        for frozen in (False, True):
            for t in wts:
                t.requires_grad_(not frozen)
            ops.prof_reset(); ops.prof_enable(True)
            y, agg = ops.edge_block(h, e, topo, w, ('sum',))
            ms = ops.prof_collect()['mlp_fwd_edge']['ms']          # device events around the hgn_mlp_fwd launch alone
            ops.prof_enable(False)
            assert (y.grad_fn.saves[0] is None) == frozen
            if it >= a.warm:
                times[frozen].append(ms)
            del y, agg
res = {'rows': E, 'precision': a.precision, 'iters': a.iters, 'bytes_written_per_row': {'saving': 2084, 'no_save': 1060}}
for frozen, name in ((False, 'saving_ms'), (True, 'no_save_ms')):
    v = sorted(times[frozen])
    res[name] = {'mean': sum(v) / len(v), 'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
print(json.dumps(res))
