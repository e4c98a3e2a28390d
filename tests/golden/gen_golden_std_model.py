"""Model-level golden for `message_passing_aggregator='std'` (graphnet.py:50-70 -> src/util.py:129-130), produced by running the
REFERENCE's own MeshGraphNet (through the import stand-ins of gen_golden.py, whose run_model / digest it uses).  Build container only, where
REF is the checkout of the reference and REPO this repository:

    cd $REF && PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 PYTHONPATH=$REPO/tools/oracle_shims:$REF \
      python $REPO/tests/golden/gen_golden_std_model.py --out $REPO/tests/golden

One latent-128 fixture in the format of gen_golden.py's seeded cases (data only: graph, target, mask, the reference's output, loss,
input gradients and gradient digests; the weights are the build-owned seeded init): architecture `none`, aggregator `std`, 2 steps,
`mesh_edges` on an 8 x 6 triangulated grid.  Every node of such a grid receives at least two edges, so no segment is without
variance and nothing is NaN (the generator checks it).  The file is NOT named mgn_*.pt: the tests that walk those fixtures compare every
parameter gradient on its own scale, and with `std` one of them is zero by construction (the LayerNorm bias of the last block's edge
model: a constant added to a column of every edge row leaves every standard deviation where it was) -- what the reference stores for
it is rounding noise.  tests/test_std_cpu.py and tests/test_gpu_std.py read this fixture.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                        # noqa: E402  (imports the reference; also puts the repository root on sys.path)
from tests import synth                       # noqa: E402

NAME, ARCH, AGG, STEPS, SETS, GKW, LATENT = 'none_std_L2_lat128', 'none', 'std', 2, ['mesh_edges'], dict(nx=8, ny=6), 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    torch.set_num_threads(4)
    seed = G.hash_name(NAME) % 1000
    graph = synth.grid_graph(seed=seed, **GKW)
    N = graph.node_features[0].shape[0]
    deg = torch.bincount(graph.edge_sets[0].receivers, minlength=N)
    assert int(deg.min()) >= 2, 'a node with fewer than two incoming edges: its std has no gradient'
    sd, out, target, mask, loss, grads, in_grads = G.run_model(ARCH, AGG, STEPS, SETS, graph, LATENT, seed, weights='seeded')
    finite = [out, loss, *grads.values(), *in_grads['node'], *[g for g in in_grads['edge'].values() if g is not None]]
    assert all(bool(torch.isfinite(t).all()) for t in finite), 'NaN / inf in the reference run'
    fx = {'arch': ARCH, 'agg': AGG, 'steps': STEPS, 'edge_sets': SETS, 'latent': LATENT, 'seed': seed, 'graph_kwargs': GKW,
          'set_order': list({'mesh_edges', 'world_edges'}), 'set_order_hyper': list({'inter_cluster', 'inter_cluster_world'}),
          'graph': {'node_features': graph.node_features,
                    'edge_sets': [(e.name, e.features, e.senders, e.receivers) for e in graph.edge_sets]},
          'out': out, 'target': target, 'mask': mask, 'loss': loss, 'weights': 'seeded',
          'shapes': {k: tuple(v.shape) for k, v in sd.items()}, 'grad_digest': G.digest(grads, seed), 'in_grads': in_grads}
    torch.save(fx, os.path.join(a.out, 'stdagg_none_L2_lat128.pt'))
    print(NAME, 'seed', seed, 'loss', float(loss), 'out', tuple(out.shape), 'min in-degree', int(deg.min()))


if __name__ == '__main__':
    main()
