"""Row f4 through the reference's own API: FlagModel.rollout (flag.py:192-246) on a 40x40 flag mesh, per-step wall time with the
network replayed from a HIP graph (default: graphs.GraphedForwardCache behind AbstractSystemModel.forward) and with every launch
eager (`model.replay_rollout = False`).  Per step: build_graph (feature kernels, normalisers) + expand_graph + network + update.
    python tools/rolloutmodelbench.py [--steps 100]        prints one JSON object
With `--nstep-batch M` the object also holds the wall time of ONE n_step_computation (the reference's evaluation after every epoch,
flag.py:248-260) over `--nstep-frames` frames of the same mesh with windows of `--nstep` steps: the windows one by one (`nstep_batch = None`)
and in lock step, M windows per union graph (`model.nstep_batch = M`), and whether the two figures agree at rtol 1e-5.
With `--unroll N` the tool does one thing instead: it times ONE `unrolled_training_step` of N steps including `backward()`
(through_state=True, frozen statistics) on the 40x40 flag mesh (none/sum/L15), for `--unroll-windows` windows in lock step and for one
window, against the same loss written with the ops the package had before that method: per step build_graph_batch -> network ->
`update` -> torch.where.  The two forms alternate inside one process; the object holds the mean and the smallest time of each.
With `--frozen` the parameters of learned_model do not require grad and frame 0 of world_pos / prev|world_pos does: the backward pass
forms the gradients of the initial state only (data-only backward of frozen MLPs).
With `--connector <name>` (`hyper`, `hetero`, `multi`; k-means, `--clusters` hyper nodes) the model of `--unroll` has that connector.  What
is timed then is the method in its two modes, alternating in one process: `through_state=False` (push-forward) and, with
`--position-gradients` (which sets `model.position_gradients = True`; a connector refuses `through_state=True` without it),
`through_state=True`.  `--position-gradients` without a connector only sets the switch: the flag graph is differentiable either way.
With `--unroll N --checkpoint` the tool times that step plain and with `checkpoint=True` (activation checkpointing) for
`--unroll-windows` windows, alternating in one process, and prints ms per call, the peak of torch.cuda.max_memory_allocated() over the
start of the call and the device launches of both routes (`checkpoint_times`; profiles/unroll_checkpoint.md)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'hyper-graph-nets_amd')):
    sys.path.insert(0, p)
import torch


def params(connector, K, steps, agg):
    return {'size': 3, 'aggregation': agg, 'message_passing_steps': steps,
            'rmp': {'clustering': 'kmeans' if connector != 'none' else 'none', 'connector': connector, 'num_clusters': K,
                    'hyper_noise': 'none', 'hyper_node_features': True, 'frequency': 1, 'fully_connect': False,
                    'intra_cluster_sampling': {'enabled': False, 'alpha': 0.1, 'spotter_threshold': 0}},
            'graph_balancer': {'algorithm': 'none', 'frequency': 1}}


def nstep_times(model, frames, a):
    traj = {k: torch.stack([frames[i % 2][k] for i in range(a.nstep_frames)]).cuda() for k in frames[0]}
    model.replay_rollout = True
    out = {'frames': a.nstep_frames, 'n_step': a.nstep, 'windows': a.nstep_frames - a.nstep, 'nstep_batch': a.nstep_batch}
    figures = {}
    for label, batch in (('sequential', None), ('lock_step', a.nstep_batch)):
        model.nstep_batch = batch
        model.n_step_computation(traj, a.nstep, a.nstep + min(2 * a.nstep_batch, a.nstep_frames - a.nstep))   # warm: topology, capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        figures[label] = model.n_step_computation(traj, a.nstep)
        torch.cuda.synchronize()
        out[f'{label}_s'] = time.perf_counter() - t0
    model.nstep_batch = None
    out['speedup'] = out['sequential_s'] / out['lock_step_s']
    out['ms_per_window_step_sequential'] = out['sequential_s'] / (out['windows'] * (a.nstep + 1)) * 1e3
    out['ms_per_window_step_lock_step'] = out['lock_step_s'] / (out['windows'] * (a.nstep + 1)) * 1e3
    out['figures_agree_rtol_1e-5'] = all(bool(torch.isclose(x, y, rtol=1e-5, atol=0)) for x, y in zip(figures['sequential'], figures['lock_step']))
    out['figures'] = {k: [float(v[0]), float(v[1])] for k, v in figures.items()}
    return out


def loop_unroll(model, windows, n_steps):
    """The loss of unrolled_training_step(windows, n_steps, True, False) written with build_graph_batch, `update` and torch.where."""
    from hgn_amd.system_model import _masked_mse
    W, N = windows['node_type'].shape[0], windows['node_type'].shape[2]
    frame = {'cells': windows['cells'], 'mesh_pos': windows['mesh_pos'], 'node_type': windows['node_type'][:, 0],
             'world_pos': windows['world_pos'][:, 0], 'prev|world_pos': windows['prev|world_pos'][:, 0]}
    losses = []
    for t in range(n_steps):
        frame['target|world_pos'] = windows['target|world_pos'][:, t]
        graph = model.expand_graph_batch(model.build_graph_batch(frame, False), W, t, n_steps, False)
        flat = model.flatten_frames(frame)
        out = model(graph)
        mask = model._loss_mask(flat)
        losses.append(_masked_mse(model.get_target(flat, False), out, mask))
        if t + 1 < n_steps:
            nxt = torch.where(mask.unsqueeze(1).expand(-1, 3), model.update(flat, out), flat['world_pos'])
            frame['world_pos'], frame['prev|world_pos'] = nxt.reshape(W, N, 3), flat['world_pos'].reshape(W, N, 3)
    return torch.stack(losses).mean()


def unroll_times(a):
    from hgn_amd import synthetic, system_model
    torch.manual_seed(0)
    remote = a.connector != 'none'
    model = system_model.FlagModel(params(a.connector, a.clusters if remote else 0, 15, 'sum'))
    model.position_gradients = bool(a.position_gradients)
    warm = {k: v.cuda() for k, v in synthetic.flag_frame(seed=100, nx=40, ny=40).items()}
    with torch.no_grad():
        model.learned_model(model.expand_graph(model.build_graph(warm, True), 0, 10 ** 9, True))
        model.get_target(warm, True)
    res = {'n_steps': a.unroll, 'nodes': 1600, 'message_passing_steps': 15, 'repeats': a.unroll_repeats, 'connector': a.connector,
           'position_gradients': bool(a.position_gradients)}
    if remote:
        res['clusters'] = a.clusters
    for W in dict.fromkeys((a.unroll_windows, 1)):
        frames = [[synthetic.flag_frame(seed=200 + 10 * w + t, nx=40, ny=40) for t in range(a.unroll)] for w in range(W)]
        windows = {k: torch.stack([torch.stack([f[k] for f in row]) for row in frames]).cuda()
                   for k in ('world_pos', 'prev|world_pos', 'target|world_pos', 'node_type')}
        windows['cells'], windows['mesh_pos'] = warm['cells'], warm['mesh_pos']
        leaves = []
        if a.frozen:            # the network's parameters get no gradient; the loss is differentiated with respect to the initial state
            model.learned_model.requires_grad_(False)
            for k in ('world_pos', 'prev|world_pos'):
                leaf = windows[k][:, 0].clone().requires_grad_(True)
                windows[k] = torch.cat([leaf.unsqueeze(1), windows[k][:, 1:]], dim=1)
                leaves.append(leaf)
        if remote:              # the two modes of the method; through the state only where the switch lets the connector differentiate
            forms = {'push_forward': lambda: model.unrolled_training_step(windows, a.unroll, False, False)[0]}
            if a.position_gradients:
                forms = {'through_state': lambda: model.unrolled_training_step(windows, a.unroll, True, False)[0], **forms}
        else:
            forms = {'unrolled_training_step': lambda: model.unrolled_training_step(windows, a.unroll, True, False)[0],
                     'per_step_ops': lambda: loop_unroll(model, windows, a.unroll)}
        times, losses = {k: [] for k in forms}, {}
        for rep in range(2 + a.unroll_repeats):                # two warm rounds: lazy state, topology caches
            for name, fn in forms.items():
                model.zero_grad(set_to_none=True)
                for leaf in leaves:
                    leaf.grad = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = fn()
                loss.backward()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                losses[name] = float(loss.detach())
        res[f'W={W}'] = {f'{k}_ms': {'mean': sum(v) / len(v), 'min': min(v)} for k, v in times.items()}
        res[f'W={W}']['losses'] = losses
        if not remote:
            res[f'W={W}']['losses_equal'] = losses['unrolled_training_step'] == losses['per_step_ops']
            res[f'W={W}']['speedup_of_the_means'] = (res[f'W={W}']['per_step_ops_ms']['mean'] / res[f'W={W}']['unrolled_training_step_ms']['mean'])
    return res


def _device_launches(fn):
    """Kernel launches and device copies of one call of ``fn``, counted by torch's profiler (a profiler that fails raises)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))


def checkpoint_times(a):
    """`--unroll N --checkpoint`: ONE unrolled_training_step of N steps with backward() (through_state=True, frozen statistics; with a
    connector: push-forward, or through the state with --position-gradients) on the 40x40 flag mesh (sum/L15) for `--unroll-windows`
    windows, plain and with checkpoint=True, alternating in one process.  Per route: ms per call (mean, min), the rise of
    torch.cuda.max_memory_allocated() over memory_allocated() across forward + backward (the largest of the timed rounds), and the
    device launches of one call (torch's profiler, in a pass of their own after the timed rounds)."""
    from hgn_amd import synthetic, system_model
    torch.manual_seed(0)
    remote = a.connector != 'none'
    model = system_model.FlagModel(params(a.connector, a.clusters if remote else 0, 15, 'sum'))
    model.position_gradients = bool(a.position_gradients)
    warm = {k: v.cuda() for k, v in synthetic.flag_frame(seed=100, nx=40, ny=40).items()}
    with torch.no_grad():
        model.learned_model(model.expand_graph(model.build_graph(warm, True), 0, 10 ** 9, True))
        model.get_target(warm, True)
    W, through = a.unroll_windows, not remote or bool(a.position_gradients)
    frames = [[synthetic.flag_frame(seed=200 + 10 * w + t, nx=40, ny=40) for t in range(a.unroll)] for w in range(W)]
    windows = {k: torch.stack([torch.stack([f[k] for f in row]) for row in frames]).cuda()
               for k in ('world_pos', 'prev|world_pos', 'target|world_pos', 'node_type')}
    windows['cells'], windows['mesh_pos'] = warm['cells'], warm['mesh_pos']
    if a.frozen:
        model.learned_model.requires_grad_(False)
        for k in ('world_pos', 'prev|world_pos'):
            leaf = windows[k][:, 0].clone().requires_grad_(True)
            windows[k] = torch.cat([leaf.unsqueeze(1), windows[k][:, 1:]], dim=1)
    routes = {'plain': None, 'checkpoint': True}
    times, peaks, losses = {k: [] for k in routes}, {k: 0 for k in routes}, {}

    def call(checkpoint):
        model.zero_grad(set_to_none=True)
        loss = model.unrolled_training_step(windows, a.unroll, through, False, checkpoint=checkpoint)[0]
        loss.backward()
        return loss
    for rep in range(2 + a.unroll_repeats):                    # two warm rounds: lazy state, topology caches, workspaces
        for name, checkpoint in routes.items():
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            loss = call(checkpoint)
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - base)
            losses[name] = float(loss.detach())
            del loss
    res = {'n_steps': a.unroll, 'windows': W, 'nodes': 1600, 'message_passing_steps': 15, 'repeats': a.unroll_repeats,
           'connector': a.connector, 'through_state': through, 'frozen': bool(a.frozen), 'losses': losses,
           'losses_equal': losses['plain'] == losses['checkpoint']}
    for name, checkpoint in routes.items():
        res[name] = {'ms': {'mean': sum(times[name]) / len(times[name]), 'min': min(times[name])},
                     'peak_bytes_over_start': int(peaks[name])}
        try:
            res[name]['device_launches'] = _device_launches(lambda: call(checkpoint))
        except Exception as err:                                # the timings stand; the count is reported as not taken, with the reason
            res[name]['device_launches'] = None
            res[name]['device_launches_error'] = f'{type(err).__name__}: {err}'
    res['ms_ratio_of_the_means'] = res['checkpoint']['ms']['mean'] / res['plain']['ms']['mean']
    res['peak_ratio'] = res['checkpoint']['peak_bytes_over_start'] / max(1, res['plain']['peak_bytes_over_start'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--unroll', type=int, default=0, help='time one unrolled_training_step of N steps with backward() instead')
    ap.add_argument('--frozen', action='store_true', help='with --unroll: freeze learned_model, differentiate with respect to the initial state')
    ap.add_argument('--connector', default='none', help='with --unroll: the connector of the model (hyper, hetero, multi); times the two modes')
    ap.add_argument('--clusters', type=int, default=16, help='with --connector: the number of hyper nodes')
    ap.add_argument('--position-gradients', action='store_true', help='with --unroll: set model.position_gradients = True')
    ap.add_argument('--unroll-windows', type=int, default=8)
    ap.add_argument('--unroll-repeats', type=int, default=10)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--nstep-batch', type=int, default=0, help='also time one n_step_computation with model.nstep_batch = M and without')
    ap.add_argument('--nstep', type=int, default=60)
    ap.add_argument('--nstep-frames', type=int, default=120)
    ap.add_argument('--checkpoint', action='store_true',
                    help='with --unroll: time the step plain and with checkpoint=True; peak memory and device launches of both')
    a = ap.parse_args()
    if a.unroll > 0:
        print(json.dumps(checkpoint_times(a) if a.checkpoint else unroll_times(a)))
        return
    from hgn_amd import synthetic, system_model
    res = {}
    for name, connector, K, layers, agg in (('flag none/sum/L15', 'none', 0, 15, 'sum'), ('flag hyper/pna/L5/K16', 'hyper', 16, 5, 'pna')):
        frames = [synthetic.flag_frame(seed=100 + i, nx=40, ny=40) for i in range(2)]
        traj = {k: torch.stack([frames[i % 2][k] for i in range(a.steps)]).cuda() for k in frames[0]}
        torch.manual_seed(0)
        model = system_model.FlagModel(params(connector, K, layers, agg))
        f0 = {k: v.cuda() for k, v in frames[0].items()}
        model.build_graph(f0, True); model.get_target(f0, True)
        model.evaluate()
        out = {}
        for replay in (True, False):
            model.replay_rollout = replay
            model.rollout(traj, 8)                           # warm: lazy layers, topology, capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pred, _ = model.rollout(traj, a.steps)
            torch.cuda.synchronize()
            out['replayed' if replay else 'eager'] = (time.perf_counter() - t0) / a.steps * 1e3
            out.setdefault('pred', []).append(pred['pred_pos'])
        same = bool(torch.equal(out['pred'][0], out['pred'][1]))
        res[name] = {'ms_per_rollout_step_network_replayed': out['replayed'], 'ms_per_rollout_step_all_eager': out['eager'],
                     'predictions_bit_identical': same, 'steps': a.steps, 'nodes': 1600}
        if a.nstep_batch > 0 and connector == 'none':        # a model with a connector takes the loop whatever nstep_batch says
            res[name]['n_step_computation'] = nstep_times(model, frames, a)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
