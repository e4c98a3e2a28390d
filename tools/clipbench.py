"""What gradient clipping costs a training step: bench.py's headline shape (its defaults: 128 flag graphs of 40x40, none/sum, 15 layers,
the whole step one captured HIP graph) with `max_grad_norm` / `skip_nonfinite` unset and set.
    python tools/clipbench.py [--batch 128] [--layers 15] [--rounds 9] [--steps 20]        prints one JSON object
Three trainers on copies of the same seeded model live in one process -- unset, set, and unset once more as a control for what two
instances of one form differ by; their captured steps alternate in rounds of `--steps` replays (the order rotates from round to
round), each round timed by a host clock around work that ends in a device synchronise.  The object holds the median, the smallest
and the largest round of each form in ms per step, and their difference.  The trainer with both arguments unset issues the launches of
a trainer built before the arguments existed (tests/test_gpu_grad_clip.py checks that), so its time is the step of the parent.
It also times the launches alone, eagerly, with device events over `--kernel-iters` calls on the trainer's own flat buffers:
ops.adam_step_dev against ops.grad_norm_clip + ops.adam_step_clip.
    python tools/clipbench.py --sched [--layers 15] [--rounds 9] [--kernel-iters 200]
times hgn_adam_step_sched against hgn_adam_step_dev, and nothing else: flat buffers of the `--layers`-block model's size (15 blocks:
2.3 M parameters), device events around `--kernel-iters` calls, the forms alternating in one process in `--rounds` rounds after two
warm rounds.  The forms: `adam_step_dev` twice (two instances on buffers of their own: what two instances of ONE kernel differ by),
`adam_step_sched` with a constant schedule, with warm-up + decay, with weight decay on every element, and with a decay mask.  The
kernel moves the 28 B per parameter hgn_adam_step_dev moves (+ 1 B with a mask), so its time should be that kernel's within the
spread of the two instances (+ 1 / 28 with a mask); the object holds the medians and that comparison."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'hyper-graph-nets_amd')):
    sys.path.insert(0, p)
import torch


def sched_kernels(own):
    assert torch.cuda.is_available(), 'clipbench.py needs an MI355X'
    import hgn_amd
    from hgn_amd import ops, parallel
    layers = own.layers if own.layers is not None else 15
    torch.manual_seed(0)
    model = hgn_amd.MeshGraphNet(output_size=3, latent_size=128, num_layers=2, message_passing_aggregator='sum',
                                 message_passing_steps=layers, architecture='none', edge_sets=['mesh_edges']).cuda()
    from hgn_amd import synthetic
    g = synthetic.grid_graph(seed=0, nx=8, ny=8)
    with torch.no_grad():                                                # materialise the lazy layers
        model(hgn_amd.MultiGraph([x.cuda() for x in g.node_features],
                                 [hgn_amd.EdgeSet(e.name, e.features.cuda(), e.senders.cuda(), e.receivers.cuda()) for e in g.edge_sets]))
    tr = parallel.DataParallelTrainer(model, lr=1e-4, weight_decay=0.01)     # its decay mask: the default filter on the real layout
    n, (b1, b2), eps = tr.fp.numel, tr.betas, tr.eps
    grad = torch.randn(n, device='cuda') * 1e-3

    def buffers():
        return tr.fp.flat.clone(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    moving = parallel.LRSchedule(1e-4, warmup_steps=1000, decay_steps=5_000_000, decay_rate=0.1, lr_min=1e-6)
    const = parallel.LRSchedule(1e-4)
    lr_out = torch.zeros(1, device='cuda')

    def dev():
        p, m, v, t = buffers()
        return lambda: ops.adam_step_dev(p, grad, m, v, 1e-4, b1, b2, eps, t)

    def sched(schedule, wd, mask):
        p, m, v, t = buffers()
        st = schedule.as_struct(wd)
        return lambda: ops.adam_step_sched(p, grad, m, v, st, b1, b2, eps, t, count_step=True, decay_mask=mask, lr_out=lr_out)
    forms = {'adam_step_dev': dev(), 'adam_step_dev_again': dev(), 'sched_constant': sched(const, 0.0, None),
             'sched_warmup_decay': sched(moving, 0.0, None), 'sched_decay_all': sched(moving, 0.01, None),
             'sched_decay_mask': sched(moving, 0.01, tr.decay_mask)}
    names, times = list(forms), {k: [] for k in forms}
    for r in range(2 + own.rounds):
        k = r % len(names)
        for name in names[k:] + names[:k]:                               # the order rotates
            fn = forms[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(own.kernel_iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= 2:                                                   # two warm rounds first
                times[name].append(a.elapsed_time(b) / own.kernel_iters * 1e3)
    res = {'mode': 'sched', 'layers': layers, 'params': n, 'masked_share': float(tr.decay_mask.float().mean()), 'rounds': own.rounds,
           'calls_per_round': own.kernel_iters, 'bytes_per_param': {'adam_step_dev': 28, 'sched': 28, 'sched_decay_mask': 29},
           'us_per_call': {k: {'median': statistics.median(ts), 'min': min(ts), 'max': max(ts)} for k, ts in times.items()}}
    med = {k: v['median'] for k, v in res['us_per_call'].items()}
    res['spread_of_two_adam_step_dev_instances_us'] = abs(med['adam_step_dev_again'] - med['adam_step_dev'])
    base = 0.5 * (med['adam_step_dev'] + med['adam_step_dev_again'])
    res['median_minus_adam_step_dev_us'] = {k: med[k] - base for k in names if k.startswith('sched')}
    res['expected_extra_with_mask_us'] = base / 28.0
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--layers', type=int, default=None)
    ap.add_argument('--nx', type=int, default=None)
    ap.add_argument('--ny', type=int, default=None)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--sched', action='store_true', help='time hgn_adam_step_sched against hgn_adam_step_dev (kernel level only)')
    own = ap.parse_args()
    if own.sched:
        return sched_kernels(own)
    import bench
    argv, sys.argv = sys.argv, ['bench.py']               # the shape is bench.py's: its defaults, unless overridden here
    try:
        args = bench.parse()
    finally:
        sys.argv = argv
    for k in ('batch', 'layers', 'nx', 'ny'):
        if getattr(own, k) is not None:
            setattr(args, k, getattr(own, k))
    assert torch.cuda.is_available(), 'clipbench.py needs an MI355X'
    dev = torch.device('cuda', 0)
    import hgn_amd
    from hgn_amd import graphs, ops, parallel
    ops.set_matmul_precision(args.precision)
    wk = bench.build_flag(args, parallel.shard_indices(args.batch, 0, 1), dev)
    graph, target, mask = wk['graph'], wk['target'], wk['mask']
    sets = [e.name for e in graph.edge_sets]

    def make(**kw):
        torch.manual_seed(0)
        model = hgn_amd.MeshGraphNet(output_size=3, latent_size=128, num_layers=2, message_passing_aggregator=args.agg,
                                     message_passing_steps=args.layers, architecture=args.arch, edge_sets=sets).to(dev)
        with torch.no_grad():
            model(graph)
        trainer = parallel.DataParallelTrainer(model, lr=1e-4, device_step=True, **kw)
        for _ in range(own.warmup):
            trainer.step(graph, target, mask)
        step = graphs.GraphedTrainStep(trainer, graph, target, mask, warmup=1)
        step()
        torch.cuda.synchronize()
        return trainer, step
    # (`unset_again`: a second trainer of the first form, built last -- what two instances of ONE form differ by in this process)
    forms = {'unset': make(), 'set': make(max_grad_norm=own.max_grad_norm, skip_nonfinite=True), 'unset_again': make()}
    times = {k: [] for k in forms}
    names = list(forms)
    for r in range(own.rounds):
        for name in names[r % 3:] + names[:r % 3]:            # the order rotates: no form always runs behind the same other one
            step = forms[name][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(own.steps):
                step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / own.steps * 1e3)
    res = {'shape': wk['workload'], 'graphs': args.batch, 'params': forms['set'][0].fp.numel, 'rounds': own.rounds, 'steps_per_round': own.steps,
           'max_grad_norm': own.max_grad_norm, 'grad_stats_of_the_last_step': [float(x) for x in forms['set'][0].grad_stats.cpu()],
           'skipped_steps': int(forms['set'][0].skipped_dev)}
    for name, ts in times.items():
        res[f'ms_per_step_{name}'] = {'median': statistics.median(ts), 'min': min(ts), 'max': max(ts)}
    res['median_difference_ms'] = res['ms_per_step_set']['median'] - res['ms_per_step_unset']['median']
    res['median_difference_of_the_two_unset_trainers_ms'] = res['ms_per_step_unset_again']['median'] - res['ms_per_step_unset']['median']
    res['max_memory_reserved_GB'] = torch.cuda.max_memory_reserved() / 2 ** 30
    res['median_difference_share_of_step'] = res['median_difference_ms'] / res['ms_per_step_unset']['median']

    # the launches alone, eager, device events
    tr = forms['set'][0]
    fp, (b1, b2) = tr.fp, tr.betas
    fp.grad.normal_(0.0, 1e-3)
    lone = {'adam_step_dev': lambda: ops.adam_step_dev(fp.flat, fp.grad, tr.m, tr.v, tr.lr, b1, b2, tr.eps, tr.t_dev),
            'grad_norm_clip': lambda: ops.grad_norm_clip(fp.grad, own.max_grad_norm, tr.grad_stats, tr.t_dev, tr.skipped_dev, True),
            'adam_step_clip': lambda: ops.adam_step_clip(fp.flat, fp.grad, tr.m, tr.v, tr.lr, b1, b2, tr.eps, tr.t_dev, tr.grad_stats[1:2])}
    res['us_per_call_eager'] = {}
    for name, fn in lone.items():
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(own.kernel_iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res['us_per_call_eager'][name] = a.elapsed_time(b) / own.kernel_iters * 1e3
    print(json.dumps(res))


if __name__ == '__main__':
    main()
