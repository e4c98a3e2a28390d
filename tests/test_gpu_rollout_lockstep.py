"""Lock-step evaluation on the GPU: the one-launch state update (features.rollout_advance / hgn_rollout_advance) against the three
launches it replaces, bit for bit; `rollout_batch` and `n_step_computation` with `nstep_batch` against the trajectories and n-step
figures the REFERENCE's own models produced (tests/golden/rollout_*.pt) and against the sequential path (`rollout` on every window
alone).

Tolerances are the project's own (tests/test_gpu_rollout.py): the two n-step figures and the per-step errors at rtol 1e-5; predictions
step-relative, max|a - b| / (largest change of state between two recorded steps) <= 2e-5 at the first predicted step, doubling per
further step (the state feeds back into the next frame's features)."""
import functools
import itertools

import pytest
import torch

from tests import rollout_cases as RC
from tests.test_gpu_rollout import cuda, hip_predictions, hip_system_model

pytestmark = pytest.mark.gpu

PLAIN = ['flag_none', 'cylinder_none', 'plate_none']


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
def _three_launches(out, nz, cur, d, ca, prev, cp, node_type, free_types, fallback):
    """Today's update: Normalizer.inverse -> lincomb3 -> torch.where."""
    from hgn_amd import features
    inv = nz.inverse(out)
    integrated = features.lincomb3(cur, ca, inv[:, :d], 1.0, prev, cp) if prev is not None else features.lincomb3(cur, ca, inv[:, :d], 1.0)
    free = torch.isin(node_type[:, 0], torch.tensor(list(free_types), dtype=torch.int64, device=out.device))
    return torch.where(free.unsqueeze(1).expand(-1, d), integrated, cur if fallback is None else fallback), inv


@pytest.mark.parametrize('F,d', [(3, 2), (3, 3)], ids=['width2+pressure', 'width3'])
@pytest.mark.parametrize('rows', [1, 63, 64, 65, 3 * 63])
def test_rollout_advance_equals_inverse_lincomb3_where_bit_for_bit(rows, F, d):
    from hgn_amd import features
    from hgn_amd.normalizer import Normalizer
    gen = torch.Generator().manual_seed(1000 * rows + d)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()
    nz = Normalizer(F, 'output_normalizer')
    nz(rnd(257, F) * torch.tensor([0.3, 2.0, 11.0][:F]).cuda() + torch.tensor([0.1, -1.5, 4.0][:F]).cuda())
    out, cur, prev, scripted = rnd(rows, F), rnd(rows, d), rnd(rows, d), rnd(rows, d)
    kinds = torch.tensor([0, 1, 3, 4, 5, 6, 2, 31, 32, 40, -1, 64], dtype=torch.int64)     # 32, 40, -1, 64: outside the bit mask
    mixed = kinds[torch.randint(0, len(kinds), (rows, 1), generator=gen)].cuda()
    SENTINEL = -7.0
    for use_prev, use_script, (node_type, free_types), rec_before in itertools.product(
            (True, False), (True, False),
            ((torch.zeros(rows, 1, dtype=torch.int64).cuda(), (0,)),                      # every row free
             (torch.full((rows, 1), 3, dtype=torch.int64).cuda(), (0, 5)),                 # no row free
             (mixed, (0, 5)), (mixed, (0,)), (mixed, (31,))), (True, False)):
        ca, cp = (2.0, -1.0) if use_prev else (1.0, 0.0)
        p, fb = (prev if use_prev else None), (scripted if use_script else None)
        want_next, want_inv = _three_launches(out, nz, cur, d, ca, p, cp, node_type, free_types, fb)
        inv_from = d if d < F else 0
        # every output is a non-contiguous column slice of a wider slab
        slabs = [torch.full((rows, 9), SENTINEL, device='cuda') for _ in range(4)]
        nxt, rec, po, inv = slabs[0][:, 1:1 + d], slabs[1][:, 4:4 + d], slabs[2][:, 0:d], slabs[3][:, 5:5 + F - inv_from]
        got = features.rollout_advance(out, nz, cur, d, ca, p, cp, node_type, free_types, fb, nxt, rec=rec, rec_before=rec_before,
                                       prev_out=po, inv_out=inv, inv_from=inv_from)
        what = (rows, F, d, use_prev, use_script, free_types, rec_before)
        assert got is nxt and torch.equal(nxt, want_next), what
        assert torch.equal(rec, cur if rec_before else want_next), what
        assert torch.equal(po, cur), what
        assert torch.equal(inv, want_inv[:, inv_from:]), what
        for slab, (c0, c1) in zip(slabs, ((1, 1 + d), (4, 4 + d), (0, d), (5, 5 + F - inv_from))):
            keep = torch.ones(9, dtype=torch.bool)
            keep[c0:c1] = False
            assert bool((slab[:, keep.cuda()] == SENTINEL).all()), what       # nothing outside the slice was written
        # the optional outputs left out, contiguous next
        alone = torch.empty(rows, d, device='cuda')
        features.rollout_advance(out, nz, cur, d, ca, p, cp, node_type, free_types, fb, alone)
        assert torch.equal(alone, want_next), what


def test_rollout_advance_refuses_outputs_it_would_have_to_copy():
    from hgn_amd import _lib, features
    from hgn_amd.normalizer import Normalizer
    nz = Normalizer(3, 'output_normalizer')
    out, cur = torch.zeros(4, 3, device='cuda'), torch.zeros(4, 3, device='cuda')
    types = torch.zeros(4, 1, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        features.rollout_advance(out, nz, cur, 3, 1.0, None, 0.0, types, (0,), None, torch.empty(3, 4, device='cuda').t())
    with pytest.raises(ValueError):
        features.rollout_advance(out, nz, cur, 3, 1.0, None, 0.0, types, (0,), None, torch.empty(4, 3, device='cuda'),
                                 rec=torch.empty(4, 3, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError):
        features.rollout_advance(out, nz, cur, 3, 1.0, None, 0.0, types, (32,), None, torch.empty(4, 3, device='cuda'))
    with pytest.raises(_lib.HgnError, match='does not match the normaliser'):
        features.rollout_advance(torch.zeros(4, 2, device='cuda'), nz, cur[:, :2], 2, 1.0, None, 0.0, types, (0,), None,
                                 torch.empty(4, 2, device='cuda'))


# ---- 2. - 6. the models -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(fixture, model, trajectory on the device), built once per case and shared by the tests below.  Tests set `nstep_batch`
    themselves and leave the model's parameters and statistics alone."""
    fx = RC.load(name)
    return fx, hip_system_model(name, fx), cuda(fx['trajectory'])


def windows_of(model, traj, n_step):
    views = model.window_views(traj, n_step, traj['cells'].shape[0])
    views['cells'] = views['cells'][0, 0]
    return views


def step_bound(name, steps):
    first = 1 if name.startswith('flag') else 0                # flag records the input state first (exact)
    return torch.tensor([2e-5 * 2.0 ** max(t - first, 0) for t in range(steps)], dtype=torch.float64)


@pytest.mark.parametrize('name', PLAIN)
def test_lockstep_matches_the_reference_figures_and_trajectory(name):
    fx, model, traj = case(name)
    model.nstep_batch = 8
    a, b = model.n_step_computation(traj, fx['n_step'])
    torch.testing.assert_close(a.cpu(), fx['n_step_result'][0], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(b.cpu(), fx['n_step_result'][1], rtol=1e-5, atol=1e-9)
    ops, errors = model.rollout_batch(windows_of(model, traj, fx['n_step']), fx['n_step'] + 1)
    W = traj['cells'].shape[0] - fx['n_step']
    assert errors.shape == (W, fx['n_step'] + 1)
    for key, got in hip_predictions(ops).items():
        want = fx['rollout'][key]
        assert got.shape[:2] == (W, fx['n_step'] + 1) and got.shape[2:] == want.shape[1:]
        shared = min(got.shape[1], want.shape[0])
        err = RC.per_step_err(got[0, :shared], want[:shared], RC.step_scale(fx, key))       # window 0 starts where the trajectory does
        print(f'lockstep[{name}] window 0 {key}: step-relative error vs the reference', err.tolist())
        assert bool((err <= step_bound(name, shared)).all()), (name, key, err.tolist())


@pytest.mark.parametrize('name', PLAIN)
def test_lockstep_matches_the_sequential_path_window_by_window(name):
    fx, model, traj = case(name)
    n_step = fx['n_step']
    horizon = n_step + 1
    ops, errors = model.rollout_batch(windows_of(model, traj, n_step), horizon)
    worst_rel, worst_abs, worst_mse = 0.0, 0.0, 0.0
    for w in range(traj['cells'].shape[0] - n_step):
        seq_ops, seq_errors = model.rollout({k: v[w:w + horizon] for k, v in traj.items()}, horizon)
        for key, want in hip_predictions(seq_ops).items():
            got = ops[key][w]
            assert got.shape == want.shape, (name, key, w)
            err = RC.per_step_err(got, want.cpu(), RC.step_scale(fx, key))
            worst_rel = max(worst_rel, float(err.max()))
            worst_abs = max(worst_abs, float((got - want).abs().max()))
            assert bool((err <= step_bound(name, horizon)).all()), (name, key, w, err.tolist())
        worst_mse = max(worst_mse, float(((errors[w] - seq_errors).abs() / seq_errors.abs().clamp_min(1e-30)).max()))
        torch.testing.assert_close(errors[w], seq_errors, rtol=1e-5, atol=0)
        for key in ('cur_positions', 'cur_velocities', 'mask'):
            if key in seq_ops:
                assert ops[key][w].shape == seq_ops[key].shape, (name, key, w)
    print(f'lockstep[{name}] vs sequential rollout, all windows: largest step-relative difference {worst_rel:.3e}, '
          f'largest absolute difference {worst_abs:.3e}, largest relative difference of a per-step error {worst_mse:.3e}')


@pytest.mark.parametrize('name', PLAIN)
def test_chunked_lockstep_and_the_loop(name):
    fx, model, traj = case(name)
    n_step = fx['n_step']
    model.nstep_batch = 8
    whole = model.n_step_computation(traj, n_step)
    model.nstep_batch = 2                                      # 3 windows: chunks of 2 and 1
    ragged = model.n_step_computation(traj, n_step)
    model.nstep_batch = 1
    singles = model.n_step_computation(traj, n_step)
    for got in (ragged, singles):
        torch.testing.assert_close(got[0], whole[0], rtol=1e-5, atol=0)
        torch.testing.assert_close(got[1], whole[1], rtol=1e-5, atol=0)
    # None: today's loop, to the bit
    model.nstep_batch = None
    loop = model.n_step_computation(traj, n_step)
    means, finals = [], []
    for start in range(traj['cells'].shape[0] - n_step):
        e = model.rollout({k: v[start:start + n_step + 1] for k, v in traj.items()}, n_step + 1)[1].cpu()
        means.append(e.mean())
        finals.append(e[-1])
    assert torch.equal(loop[0], torch.stack(means).mean()) and torch.equal(loop[1], torch.stack(finals).mean())
    torch.testing.assert_close(loop[0], fx['n_step_result'][0], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(loop[1], fx['n_step_result'][1], rtol=1e-5, atol=1e-9)
    # num_timesteps: fewer windows, the same ones in both paths
    frames = traj['cells'].shape[0] - 1
    model.nstep_batch = 8
    short = model.n_step_computation(traj, n_step, frames)
    model.nstep_batch = None
    short_loop = model.n_step_computation(traj, n_step, frames)
    torch.testing.assert_close(short[0], short_loop[0], rtol=1e-5, atol=0)
    torch.testing.assert_close(short[1], short_loop[1], rtol=1e-5, atol=0)


def test_a_model_with_a_connector_takes_the_loop():
    fx, model, traj = case('flag_hyper_k4')
    model.nstep_batch = None
    loop = model.n_step_computation(traj, fx['n_step'])
    model.nstep_batch = 8
    got = model.n_step_computation(traj, fx['n_step'])
    model.nstep_batch = None
    assert torch.equal(got[0], loop[0]) and torch.equal(got[1], loop[1])
    torch.testing.assert_close(got[0], fx['n_step_result'][0], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(got[1], fx['n_step_result'][1], rtol=1e-5, atol=1e-9)


def test_nstep_batch_travels_in_pickles_as_a_plain_value():
    import pickle
    fx, model, traj = case('cylinder_none')
    model.nstep_batch = 8
    copy = pickle.loads(pickle.dumps(model))
    model.nstep_batch = None
    assert copy.nstep_batch == 8
    state = copy.__getstate__()
    del state['nstep_batch']                                   # a checkpoint pickled before the attribute existed
    old = type(model).__new__(type(model))
    old.__setstate__(state)
    assert old.nstep_batch is None
    a = old.n_step_computation(traj, fx['n_step'])
    torch.testing.assert_close(a[0], fx['n_step_result'][0], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize('name', PLAIN)
def test_lockstep_evaluation_has_no_side_effects(name):
    from hgn_amd.normalizer import Normalizer
    fx, model, traj = case(name)
    before_ops, before_mse = model.rollout(traj, fx['T'])
    before_ops = {k: v.clone() for k, v in hip_predictions(before_ops).items()}
    normalisers = {n: m for n, m in model.named_modules() if isinstance(m, Normalizer)}
    assert '_output_normalizer' in normalisers and '_node_normalizer' in normalisers and '_mesh_edge_normalizer' in normalisers
    stats = lambda m: (m._acc_sum.clone(), m._acc_sum_squared.clone(), m._acc_count.clone(), m._num_accumulations.clone(), m._host_num_acc)
    before = {n: stats(m) for n, m in normalisers.items()}
    frames = {k: v.clone() for k, v in traj.items()}
    model.nstep_batch = 8
    model.n_step_computation(traj, fx['n_step'])
    model.nstep_batch = None
    for k, v in frames.items():                                 # the windows are views of the trajectory: it is read, never written
        assert torch.equal(traj[k], v), (name, k)
    W, N, steps = traj['cells'].shape[0] - fx['n_step'], traj['node_type'].shape[1], fx['n_step'] + 1
    for n, m in normalisers.items():
        was, now = before[n], stats(m)
        if name.startswith('flag') and n == '_node_dynamic_normalizer':
            # the one normaliser that accumulates in evaluation too, in `rollout` as in the reference (flag.py:115, no is_training):
            # lock step feeds it the same W * N values per step, in one accumulation
            assert float(now[2] - was[2]) == W * N * steps and float(now[3] - was[3]) == steps and now[4] - was[4] == steps
            continue
        assert all(torch.equal(a, b) for a, b in zip(was[:4], now[:4])) and was[4] == now[4], n
    after_ops, after_mse = model.rollout(traj, fx['T'])
    for key, want in before_ops.items():
        assert torch.equal(after_ops[key], want), (name, key)
    assert torch.equal(after_mse, before_mse)
