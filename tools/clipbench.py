"""What gradient clipping costs a training step: bench.py's headline shape (its defaults: 128 flag graphs of 40x40, none/sum, 15 layers,
the whole step one captured HIP graph) with `max_grad_norm` / `skip_nonfinite` unset and set.
    python tools/clipbench.py [--batch 128] [--layers 15] [--rounds 9] [--steps 20]        prints one JSON object
Three trainers on copies of the same seeded model live in one process -- unset, set, and unset once more as a control for what two
instances of one form differ by; their captured steps alternate in rounds of `--steps` replays (the order rotates from round to
round), each round timed by a host clock around work that ends in a device synchronise.  The object holds the median, the smallest
and the largest round of each form in ms per step, and their difference.  The trainer with both arguments unset issues the launches of
a trainer built before the arguments existed (tests/test_gpu_grad_clip.py checks that), so its time is the step of the parent.
It also times the launches alone, eagerly, with device events over `--kernel-iters` calls on the trainer's own flat buffers:
ops.adam_step_dev against ops.grad_norm_clip + ops.adam_step_clip."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'hyper-graph-nets_amd')):
    sys.path.insert(0, p)
import torch


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
    own = ap.parse_args()
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
