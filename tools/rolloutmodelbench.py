"""Row f4 through the reference's own API: FlagModel.rollout (flag.py:192-246) on a 40x40 flag mesh, per-step wall time with the
network replayed from a HIP graph (default: graphs.GraphedForwardCache behind AbstractSystemModel.forward) and with every launch
eager (`model.replay_rollout = False`).  Per step: build_graph (feature kernels, normalisers) + expand_graph + network + update.
    python tools/rolloutmodelbench.py [--steps 100]        prints one JSON object
With `--nstep-batch M` the object also holds the wall time of ONE n_step_computation (the reference's evaluation after every epoch,
flag.py:248-260) over `--nstep-frames` frames of the same mesh with windows of `--nstep` steps: the windows one by one (`nstep_batch = None`)
and in lock step, M windows per union graph (`model.nstep_batch = M`), and whether the two figures agree at rtol 1e-5."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--nstep-batch', type=int, default=0, help='also time one n_step_computation with model.nstep_batch = M and without')
    ap.add_argument('--nstep', type=int, default=60)
    ap.add_argument('--nstep-frames', type=int, default=120)
    a = ap.parse_args()
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
