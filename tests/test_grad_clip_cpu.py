"""Clipping by the global norm and the non-finite-step guard, without a GPU: argument validation of the C ABI
(hgn_grad_clip_coef / hgn_grad_clip_workspace_bytes / hgn_adam_step_clip answer with status codes before any launch) and the
trainer's host logic on CPU tensors (parallel.DataParallelTrainer with adam_fn=_torch_adam takes the torch form of the same
arithmetic: the norm in fp64, clip_grad_norm_'s coefficient, the skip), single process and gloo world 2.

Yardstick: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on a copy of the model.  Adam's update is nearly invariant under a
scaling of the gradient, so the moments m, v and the coefficient are compared, not only the weights."""
import ctypes as C
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mgn_oracle as O
from tests import helpers as H
from tests.test_host_cpu import _OracleNet

INVALID = -1
LR = 1e-2


def test_abi_validation_without_gpu():
    from hgn_amd import _lib
    lib = _lib.lib()
    nb = C.c_size_t(0)
    assert lib.hgn_grad_clip_workspace_bytes(2_400_003, C.byref(nb)) == 0 and nb.value > 0
    need = nb.value
    assert lib.hgn_grad_clip_workspace_bytes(0, C.byref(nb)) == 0 and nb.value == need        # a fixed grid: no dependence on n
    assert lib.hgn_grad_clip_workspace_bytes(-1, C.byref(nb)) == INVALID
    assert lib.hgn_grad_clip_workspace_bytes(10, None) == INVALID
    # pointers are never dereferenced by a refused call: any aligned non-null value stands for a buffer
    g, stats, ws, cnt = 0x1000, 0x2000, 0x3000, 0x4000
    bad = {'null g': dict(g=None), 'null stats': dict(stats=None), 'null ws': dict(ws=None), 'n < 0': dict(n=-1),
           'short workspace': dict(ws_bytes=need - 1), 'no workspace bytes': dict(ws_bytes=0), 'misaligned ws': dict(ws=0x3004),
           'nan max_norm': dict(max_norm=float('nan'))}
    for what, kw in bad.items():
        a = dict(g=g, n=100, max_norm=1.0, skip=1, stats=stats, step=cnt, skipped=cnt + 4, ws=ws, ws_bytes=need)
        a.update(kw)
        rc = lib.hgn_grad_clip_coef(a['g'], a['n'], a['max_norm'], a['skip'], a['stats'], a['step'], a['skipped'], a['ws'], a['ws_bytes'], None)
        assert rc == INVALID, what
        assert b'hgn_grad_clip_coef' in lib.hgn_last_error(), what
    p = 0x5000
    assert lib.hgn_adam_step_clip(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, None, 1.0, stats, None) == INVALID
    assert b'step counter' in lib.hgn_last_error()
    assert lib.hgn_adam_step_clip(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, cnt, 1.0, None, None) == INVALID
    assert b'coefficient' in lib.hgn_last_error()
    assert lib.hgn_adam_step_clip(None, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, cnt, 1.0, stats, None) == INVALID
    assert lib.hgn_adam_step_clip(p, p, p, p, -1, 1e-3, 0.9, 0.999, 1e-8, cnt, 1.0, stats, None) == INVALID
    assert lib.hgn_adam_step_clip(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, cnt, 1.0, stats, None) == 0      # nothing to update, nothing launched


def test_ops_refuse_cpu_tensors_and_wrong_layouts():
    from hgn_amd import _lib, ops
    import pytest
    with pytest.raises(_lib.HgnError):
        ops.grad_norm_clip(torch.zeros(8), 1.0)
    z = torch.zeros(8)
    with pytest.raises(_lib.HgnError):
        ops.adam_step_clip(z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, torch.zeros(1, dtype=torch.int32), torch.ones(1))


def _small_problem():
    """The small model and batch of test_host_cpu.py's data-parallel test: 4 graphs of 16 nodes, latent size 16."""
    from hgn_amd import synthetic
    graphs = [synthetic.grid_graph(seed=10 + i, nx=4, ny=4) for i in range(4)]
    shapes = O.param_shapes('none', 'sum', 1, ['mesh_edges'], 5, {'mesh_edges': 7}, 0, 3, 16)
    gen = torch.Generator().manual_seed(0)
    targets = torch.randn(4, 16, 3, generator=gen)
    masks = torch.ones(4, 16, dtype=torch.bool)
    masks[0, :5] = False
    return graphs, shapes, targets, masks


def _batch(graphs, targets, masks, order):
    from hgn_amd import synthetic
    g = synthetic.batch([graphs[i] for i in order])
    return (O.MultiGraph(g.node_features, [O.EdgeSet(*e) for e in g.edge_sets]), torch.cat([targets[i] for i in order]),
            torch.cat([masks[i] for i in order]))


def _flat_of(tensors):
    return torch.cat([torch.nn.functional.pad(t.detach().reshape(-1), (0, (-t.numel()) % 4)) for t in tensors])


def _reference(order, max_norm, steps=3, seed=3):
    """clip_grad_norm_ + torch.optim.Adam on the mean over all NORMAL nodes -> per step (norm, coef), then flat p, m, v."""
    graphs, shapes, targets, masks = _small_problem()
    model = _OracleNet(O.init_state_dict_like(shapes, seed))
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    g, target, mask = _batch(graphs, targets, masks, order)
    stats = []
    for _ in range(steps):
        opt.zero_grad()
        O.masked_mse(model(g), target, mask).backward()
        norm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm if max_norm is not None else float('inf')))
        stats.append((norm, min(1.0, max_norm / (norm + 1e-6)) if max_norm is not None else 1.0))
        opt.step()
    ps = list(model.parameters())
    return stats, _flat_of(ps), _flat_of([opt.state[p]['exp_avg'] for p in ps]), _flat_of([opt.state[p]['exp_avg_sq'] for p in ps])


def test_cpu_trainer_clips_like_clip_grad_norm_and_torch_adam():
    from hgn_amd import parallel
    graphs, shapes, targets, masks = _small_problem()
    order = [0, 1, 2, 3]
    unclipped, _, _, _ = _reference(order, None, steps=1)
    max_norm = 0.5 * unclipped[0][0]                       # active at the first step at least
    want_stats, want_p, want_m, want_v = _reference(order, max_norm)
    tr = parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), lr=LR, adam_fn=parallel._torch_adam,
                                      max_grad_norm=max_norm)
    assert tr.t_dev is not None and tr.grad_stats.shape == (2,) and int(tr.skipped_dev) == 0
    g, target, mask = _batch(graphs, targets, masks, order)
    for step in range(3):
        tr.step(g, target, mask)
        norm, coef = (float(x) for x in tr.grad_stats)
        print(f'cpu clip step {step}: norm {norm:.9g} (torch {want_stats[step][0]:.9g})  coef {coef:.9g} (torch {want_stats[step][1]:.9g})')
        assert abs(norm - want_stats[step][0]) <= 1e-6 * want_stats[step][0]
        assert abs(coef - want_stats[step][1]) <= 1e-6 * want_stats[step][1]
    assert want_stats[0][1] < 0.51 and int(tr.t_dev) == 3 and int(tr.skipped_dev) == 0
    errs = {'m': H.rel_err(tr.m, want_m), 'v': H.rel_err(tr.v, want_v)}
    print('cpu clip after 3 steps: rel_err', errs)
    assert errs['m'] <= 1e-6 and errs['v'] <= 1e-6
    torch.testing.assert_close(tr.fp.flat, want_p, rtol=2e-5, atol=2e-6)
    # and clipping did something: the unclipped moments are elsewhere
    _, _, free_m, _ = _reference(order, None)
    assert H.rel_err(free_m, want_m) > 0.1


def test_cpu_trainer_without_the_arguments_is_unchanged():
    from hgn_amd import parallel
    _, shapes, _, _ = _small_problem()
    tr = parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), lr=LR, adam_fn=parallel._torch_adam)
    assert tr.t_dev is None and tr.grad_stats is None and tr.skipped_dev is None and not tr.clip


def test_cpu_trainer_skips_a_non_finite_step():
    import pytest
    from hgn_amd import parallel
    graphs, shapes, targets, masks = _small_problem()
    g, target, mask = _batch(graphs, targets, masks, [0, 1, 2, 3])
    tr = parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), lr=LR, adam_fn=parallel._torch_adam,
                                      skip_nonfinite=True)
    assert tr.max_grad_norm is None and tr.t_dev is not None
    tr.step(g, target, mask)                               # a finite step first: m and v are not zero
    assert int(tr.t_dev) == 1 and int(tr.skipped_dev) == 0 and float(tr.grad_stats[1]) == 1.0
    before = [t.clone() for t in (tr.fp.flat, tr.m, tr.v, tr.t_dev)]
    for bad in (float('nan'), float('inf')):
        tr.fp.zero_grad()
        tr.fp.grad.fill_(0.25)
        tr.fp.grad[7] = bad                                # one entry of the reduced gradient
        tr.fp.count.fill_(1.0)
        tr.reduce_and_update(torch.zeros(1), 1)
    for a, b in zip(before, (tr.fp.flat, tr.m, tr.v, tr.t_dev)):
        assert torch.equal(a, b)
    assert int(tr.skipped_dev) == 2 and float(tr.grad_stats[1]) == 0.0
    tr.step(g, target, mask)                               # and training goes on
    assert int(tr.t_dev) == 2 and int(tr.skipped_dev) == 2 and not torch.equal(before[0], tr.fp.flat)
    with pytest.raises(ValueError, match='skip_nonfinite'):
        parallel.DataParallelTrainer(_OracleNet(O.init_state_dict_like(shapes, 3)), adam_fn=lambda *a, **k: None, skip_nonfinite=True)


def _dp_worker(rank, world, port, out, max_norm):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hgn_amd import parallel
    torch.set_num_threads(1)
    graphs, shapes, targets, masks = _small_problem()
    model = _OracleNet(O.init_state_dict_like(shapes, 3 + rank))        # different per rank: the broadcast fixes it
    tr = parallel.DataParallelTrainer(model, lr=LR, adam_fn=parallel._torch_adam, max_grad_norm=max_norm, skip_nonfinite=True)
    g, target, mask = _batch(graphs, targets, masks, parallel.shard_indices(4, rank, world))
    stats = []
    for _ in range(3):
        tr.step(g, target, mask)
        stats.append(tr.grad_stats.clone())
    mine = torch.cat([tr.fp.flat, tr.m, tr.v] + stats)
    theirs = mine.clone()
    dist.broadcast(theirs, src=0)
    assert torch.equal(mine, theirs), 'replicas diverged'
    if rank == 0:
        torch.save({'flat': tr.fp.flat.clone(), 'm': tr.m.clone(), 'v': tr.v.clone(), 'stats': torch.stack(stats)}, out)
    dist.destroy_process_group()


def test_two_ranks_clip_alike_and_like_one_process(tmp_path):
    from hgn_amd import parallel
    order = parallel.shard_indices(4, 0, 2) + parallel.shard_indices(4, 1, 2)
    unclipped, _, _, _ = _reference(order, None, steps=1)
    max_norm = 0.5 * unclipped[0][0]
    port = 25500 + (os.getpid() % 2000)
    out = str(tmp_path / 'clip.pt')
    mp.spawn(_dp_worker, args=(2, port, out, max_norm), nprocs=2, join=True)
    res = torch.load(out)
    want_stats, want_p, want_m, want_v = _reference(order, max_norm)
    assert float(res['stats'][0, 1]) < 0.51               # clipping was active
    torch.testing.assert_close(res['stats'], torch.tensor(want_stats, dtype=torch.float32), rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(res['flat'], want_p, rtol=2e-5, atol=2e-6)
    assert H.rel_err(res['m'], want_m) <= 2e-5 and H.rel_err(res['v'], want_v) <= 2e-5
