"""Measurement of the rows in front of the message-passing path on one MI355X:

  * per-frame latency of FlagModel.build_graph and of build_graph + expand_graph (hyper, K=16) -- what a training
    or rollout loop pays per frame -- next to the CPU oracle (the reference's op sequence) on the host cores;
  * kernel-level HBM rates of the feature kernels on a batch-sized input (64 x 9 282 edges), timed with HIP events.

  * whole batches of frames (B = 21, the reference's batch, and B = 128, the benchmark's): the per-frame path
    (build_graph x B + batching.batch_graphs) against build_graph_batch for the cylinder and the plate model, and for the plate
    with the hetero connector per-frame expand_graph + batch_graphs against expand_graph_batch -- both paths in this process, on
    the same inputs.

  * with --noise, the seeded training noise alone: one launch per batch of B = 21 / 128 flag frames against the reference's torch
    sequence per frame (noise_timing).

  * with --loss, the training loss (forward + backward) and one-step evaluation at 1 and at 128 flag frames: the torch sequence
    `_masked_mse` and the per-frame validation_step loop against features.frame_losses and one_step_errors(batch=B), with the
    device launches of both forms (loss_timing; profiles/frame_losses_time.md).

  * with --ragged, one batch of 8 frames of 8 different meshes (cylinder, plate): build and build + loss through the per-frame route
    against build_graph_frames / validation_step_batch (ragged_timing; profiles/ragged_batch_time.md).  `--ragged-route per-frame`
    runs the per-frame route alone, with calls the package had before the ragged ones: the form that also runs on an older commit.

    python tools/featbench.py [--frames 50] [--no-cpu] [--batched-only | --noise | --loss | --ragged [--ragged-route both|per-frame|ragged]]
Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'hyper-graph-nets_amd'))


def params(connector, K):
    return {'size': 3, 'aggregation': 'sum', 'message_passing_steps': 1,
            'rmp': {'clustering': 'kmeans' if connector != 'none' else 'none', 'connector': connector, 'num_clusters': K,
                    'hyper_noise': 'none', 'hyper_node_features': True, 'frequency': 1, 'fully_connect': False,
                    'intra_cluster_sampling': {'enabled': False, 'alpha': 0.1, 'spotter_threshold': 0}},
            'graph_balancer': {'algorithm': 'none', 'frequency': 1}}


def ev_time(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_time(fn, n=20, warm=3):
    """Mean wall-clock ms of ``fn`` over ``n`` repetitions, synchronised around the timed region (host work counts)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def batched_builds():
    """Per-frame path against the batched calls, cylinder and plate, B = 21 and 128 (ms per batch)."""
    from hgn_amd import batching, synthetic, system_model
    out = {}
    shared = ('cells', 'mesh_pos')
    cases = (('cylinder', system_model.CylinderModel, lambda i: synthetic.cylinder_frame(seed=i)),
             ('plate', system_model.PlateModel, lambda i: synthetic.plate_frame(seed=i)))
    for kind, cls, make in cases:
        host = [make(i) for i in range(8)]
        common = {k: host[0][k].cuda() for k in shared}
        dev = [{k: (common[k] if k in shared else v.cuda()) for k, v in f.items()} for f in host]
        for B in (21, 128):
            frames = [dev[i % 8] for i in range(B)]
            stacked = {k: (common[k] if k in shared else torch.stack([f[k] for f in frames])) for k in dev[0]}
            model = cls(params('none', 16))
            row = {'nodes per frame': int(host[0]['node_type'].shape[0]),
                   'build_graph x B + batch_graphs ms': wall_time(
                       lambda: batching.batch_graphs([model.build_graph(f, True) for f in frames])),
                   'build_graph_batch ms': wall_time(lambda: model.build_graph_batch(stacked, True))}
            if kind == 'plate':
                g = model.build_graph_batch(stacked, True)
                row['world edges in the batch'] = int(g.edge_sets[1].senders.shape[0])
                remote = cls(params('hetero', 8))
                remote.expand_graph(remote.build_graph(frames[0], True), 0, 10 ** 9, True)     # clustering: once, not timed
                graphs = [remote.build_graph(f, True) for f in frames]
                union = remote.build_graph_batch(stacked, True)
                row['hetero K=8: expand_graph x B + batch_graphs ms'] = wall_time(
                    lambda: batching.batch_graphs([remote.expand_graph(x, 1, 10 ** 9, True) for x in graphs]))
                row['hetero K=8: expand_graph_batch ms'] = wall_time(lambda: remote.expand_graph_batch(union, B, 1, 10 ** 9, True))
                row['hetero K=8: build + expand per frame + batch_graphs ms'] = wall_time(
                    lambda: batching.batch_graphs([remote.expand_graph(remote.build_graph(f, True), 1, 10 ** 9, True) for f in frames]))
                row['hetero K=8: build_graph_batch + expand_graph_batch ms'] = wall_time(
                    lambda: remote.expand_graph_batch(remote.build_graph_batch(stacked, True), B, 1, 10 ** 9, True))
            out[f'{kind} B={B}'] = row
    return out


def noise_timing(rounds=20, warm=3):
    """Training noise for B = 21 and B = 128 frames of the 1 600-node flag mesh: the one hgn_training_noise launch (FlagModel.add_noise
    on the stacked frames) against the torch sequence of the reference's Preprocessing._add_noise (src/data/preprocessing.py:84-98)
    run once per frame.  The two alternate in one process; every round of either is timed with device events of its own
    (ms per batch, mean and min over the timed rounds)."""
    from hgn_amd import synthetic, system_model
    from hgn_amd.util import NodeType
    cfg = dict(params('none', 16), field='world_pos', noise=0.003, gamma=0.9)
    model = system_model.FlagModel(cfg)
    model.noise_seed = 1
    field, scale, gamma = cfg['field'], cfg['noise'], cfg['gamma']
    host = [synthetic.flag_frame(seed=i, nx=40, ny=40) for i in range(4)]
    normal = torch.tensor([NodeType.NORMAL.value], device='cuda').int()

    def per_frame(frame):
        noise = torch.normal(torch.zeros(frame[field].size(), dtype=torch.float32, device='cuda'), std=scale)
        rows = torch.eq(frame['node_type'], normal)[:, 0]
        mask = torch.stack([rows for _ in range(noise.shape[1])], dim=1)
        noise = torch.where(mask, noise, torch.zeros_like(noise))
        frame[field] += noise
        frame['target|' + field] += (1.0 - gamma) * noise

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    out = {}
    for B in (21, 128):
        names = (field, 'target|' + field, 'node_type')
        frames = [{k: host[i % 4][k].cuda().clone() for k in names} for i in range(B)]          # written in place by the torch sequence
        stacked = {k: torch.stack([host[i % 4][k] for i in range(B)]).cuda() for k in names}
        draws = iter(range(10 ** 6))
        ms = {'one launch': [], 'torch sequence per frame': []}
        for r in range(warm + rounds):
            one = timed(lambda: model.add_noise(stacked, next(draws)))
            seq = timed(lambda: [per_frame(f) for f in frames])
            if r >= warm:
                ms['one launch'].append(one)
                ms['torch sequence per frame'].append(seq)
        out[f'B={B}'] = {'nodes per frame': int(stacked[field].shape[1]),
                         **{f'{k} ms {stat}': fn(v) for k, v in ms.items() for stat, fn in (('mean', lambda v: sum(v) / len(v)), ('min', min))}}
    return out


def _stats(ms):
    mean = sum(ms) / len(ms)
    return {'mean': mean, 'min': min(ms), 'max': max(ms), 'std': (sum((v - mean) ** 2 for v in ms) / len(ms)) ** 0.5}


def _device_launches(fn):
    """Kernel launches and device copies of one call of ``fn``, counted by torch's profiler; None where it records no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return count or None
    except Exception:
        return None


def loss_timing(rounds=20, warm=4, inner=20):
    """The training loss and one-step evaluation at 1 and at 128 frames of the 1 600-node flag mesh, the torch form of the parent
    against the kernel form, alternating round by round in one process (host clock around a synchronised window of ``inner`` calls;
    ms per call: mean, min, max and standard deviation over the timed rounds).
      * loss forward + backward: `_loss_mask` + `_masked_mse` + autograd against features.frame_losses(...).loss, on a network output
        that requires grad (the target does not: the single-step case);
      * one-step evaluation: the per-frame loop over build_graph / validation_step (one_step_errors(batch=None), two host reads per
        frame) against one_step_errors(batch=B): one union graph, one frame_losses call, one copy."""
    from functools import reduce
    from hgn_amd import features, synthetic, system_model
    from hgn_amd.system_model import _masked_mse
    host = [synthetic.flag_frame(seed=i, nx=40, ny=40) for i in range(4)]
    free = system_model.FlagModel._LOCKSTEP.free_types
    out = {}

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def alternate(forms, n):
        ms = {k: [] for k in forms}
        for r in range(warm + rounds):
            for k, fn in forms.items():
                t = window(fn, n)
                if r >= warm:
                    ms[k].append(t)
        return ms

    for B in (1, 128):
        rows = B * 1600
        gen = torch.Generator().manual_seed(B)
        net = torch.randn(rows, 3, generator=gen).cuda().requires_grad_(True)
        target = torch.randn(rows, 3, generator=gen).cuda()
        node_type = torch.cat([host[i % 4]['node_type'] for i in range(B)]).cuda()

        def torch_form():
            t = node_type[:, 0]
            mask = reduce(torch.logical_or, [torch.eq(t, value) for value in free])
            net.grad = None
            _masked_mse(target, net, mask).backward()
            return net.grad

        def kernel_form():
            net.grad = None
            features.frame_losses(net, target, node_type, free, 1600).loss.backward()
            return net.grad
        forms = {'torch sequence': torch_form, 'frame_losses': kernel_form}
        gap = float((torch_form() - kernel_form()).abs().max() / torch_form().abs().max())
        row = {'rows': rows, 'max gradient gap / max gradient': gap,
               'device launches per call': {k: _device_launches(fn) for k, fn in forms.items()}}
        row.update({f'{k} ms': _stats(v) for k, v in alternate(forms, inner).items()})
        out[f'loss forward + backward, B={B}'] = row

        model = system_model.FlagModel(dict(params('none', 16), message_passing_steps=15))
        trajectory = {k: torch.stack([host[i % 4][k] for i in range(B)]).cuda() for k in host[0]}
        with torch.no_grad():
            model.build_graph(_frame_of(trajectory, 0), True)               # the normalisers see data once
            model.get_target(_frame_of(trajectory, 0), True)
        forms = {'validation_step loop': lambda: model.one_step_errors(trajectory), 'one_step_errors(batch=B)': lambda: model.one_step_errors(trajectory, batch=B)}
        a, b = (fn() for fn in forms.values())
        row = {'frames': B, 'max relative gap of the figures': float(((a - b).abs() / a.abs()).max()),
               'device launches per call': {k: _device_launches(fn) for k, fn in forms.items()}}
        row.update({f'{k} ms': _stats(v) for k, v in alternate(forms, 1 if B > 1 else 5).items()})
        out[f'one-step evaluation, {B} frame(s), 15 message passing steps'] = row
    return out


def _frame_of(trajectory, t):
    return {k: v[t] for k, v in trajectory.items()}


RAGGED_MESHES = {'cylinder': ((40, 30), (52, 36), (36, 28), (60, 40), (44, 34), (56, 30), (38, 32), (48, 38)),
                 'plate': ((12, 10, 4), (16, 12, 4), (10, 10, 5), (18, 12, 4), (14, 12, 4), (12, 12, 5), (16, 10, 4), (14, 10, 5))}


def ragged_timing(routes=('per-frame', 'ragged'), rounds=20, warm=4):
    """Build and build + loss for ONE batch of 8 frames of 8 different meshes (cylinder: 1 008 .. 2 400 nodes; plate: 540 .. 972),
    15 message passing steps, evaluation mode:
      * per-frame (what the package offered for mixed meshes before the ragged calls; it runs on that commit too): build = build_graph
        per frame + a concatenation in the style of batching.batch_graphs, which itself takes graphs of one size only (ids shifted by
        the rows before the frame, one torch.cat per field); build + loss = build_graph, expand_graph and validation_step per frame,
        two host reads each;
      * ragged: build = build_graph_frames; build + loss = build_graph_frames, expand_graph_frames, validation_step_batch and one copy
        of the [B, 2] figures.
    The routes given alternate round by round in one process; the host clock runs around a synchronised call (ms per batch: mean,
    min, max and standard deviation over the timed rounds), and the device launches of one call are counted in a pass of their own."""
    from hgn_amd import synthetic, system_model
    from hgn_amd.util import EdgeSet, MultiGraph

    def concat_graphs(graphs):
        first = [0]
        for g in graphs:
            first.append(first[-1] + g.node_features[0].shape[0])
        sets = [EdgeSet(name=e.name, features=torch.cat([g.edge_sets[k].features for g in graphs]),
                        senders=torch.cat([g.edge_sets[k].senders + p for g, p in zip(graphs, first)]),
                        receivers=torch.cat([g.edge_sets[k].receivers + p for g, p in zip(graphs, first)]))
                for k, e in enumerate(graphs[0].edge_sets)]
        return MultiGraph(node_features=[torch.cat([g.node_features[0] for g in graphs])], edge_sets=sets)
    make = {'cylinder': lambda i, m: synthetic.cylinder_frame(seed=500 + i, nx=m[0], ny=m[1]),
            'plate': lambda i, m: synthetic.plate_frame(seed=500 + i, nx=m[0], ny=m[1], nz=m[2], obstacle=(m[0] // 2, m[1] // 2, 2))}
    classes = {'cylinder': system_model.CylinderModel, 'plate': system_model.PlateModel}
    out = {}
    for kind, meshes in RAGGED_MESHES.items():
        frames = [{k: v.cuda() for k, v in make[kind](i, m).items()} for i, m in enumerate(meshes)]
        B = len(frames)
        model = classes[kind](dict(params('none', 16), message_passing_steps=15))
        with torch.no_grad():
            model.build_graph(frames[0], True)                         # the normalisers see data once
            model.get_target(frames[0], True)
        forms = {}
        if 'per-frame' in routes:
            def per_frame_build():
                with torch.no_grad():
                    return concat_graphs([model.build_graph(f, False) for f in frames])

            def per_frame_loss():
                return torch.tensor([list(model.validation_step(model.expand_graph(model.build_graph(f, False), 0, B, False), f))
                                     for f in frames])
            forms['per-frame: build_graph x B + concatenation'] = per_frame_build
            forms['per-frame: build_graph + validation_step x B'] = per_frame_loss
        if 'ragged' in routes:
            def ragged_build():
                with torch.no_grad():
                    return model.build_graph_frames(frames, False)

            def ragged_loss():
                with torch.no_grad():
                    flat, frame_rows = model.concat_frames(frames)
                    graph = model.expand_graph_frames(model.build_graph_frames((flat, frame_rows), False), frame_rows, 0, B, False)
                    return torch.stack(model.validation_step_batch(graph, flat, frame_rows), dim=1).cpu()
            forms['ragged: build_graph_frames'] = ragged_build
            forms['ragged: build_graph_frames + validation_step_batch'] = ragged_loss
        row = {'frames': B, 'nodes per frame': [int(f['node_type'].shape[0]) for f in frames],
               'edges in the union': {e.name: int(e.senders.shape[0]) for e in concat_graphs(
                   [model.build_graph(f, False) for f in frames]).edge_sets}}
        if len(routes) == 2:
            a, b = forms['per-frame: build_graph + validation_step x B'](), forms['ragged: build_graph_frames + validation_step_batch']()
            row['max relative gap of the [B, 2] figures'] = float(((a - b).abs() / a.abs()).max())
        row['device launches per call'] = {k: _device_launches(fn) for k, fn in forms.items()}
        ms = {k: [] for k in forms}
        for r in range(warm + rounds):
            for k, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= warm:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        row.update({f'{k} ms': _stats(v) for k, v in ms.items()})
        out[kind] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--batched-only', action='store_true', help='only the per-frame against batched build / expand comparison')
    ap.add_argument('--noise', action='store_true', help='only the training noise: one launch per batch against the torch sequence per frame')
    ap.add_argument('--loss', action='store_true', help='only the loss: the torch sequence and the per-frame validation loop against frame_losses / one_step_errors(batch)')
    ap.add_argument('--ragged', action='store_true', help='only a batch of frames of different meshes: the per-frame route against build_graph_frames / validation_step_batch')
    ap.add_argument('--ragged-route', choices=('both', 'per-frame', 'ragged'), default='both', help='with --ragged: the routes to time')
    a = ap.parse_args()
    from hgn_amd import features, synthetic, system_model
    from hgn_amd.normalizer import Normalizer
    res = {}
    if a.noise:
        print(json.dumps({'training noise': noise_timing()}))
        return
    if a.loss:
        print(json.dumps({'frame losses': loss_timing()}))
        return
    if a.batched_only:
        print(json.dumps({'batched builds': batched_builds()}))
        return
    if a.ragged:
        routes = ('per-frame', 'ragged') if a.ragged_route == 'both' else (a.ragged_route,)
        print(json.dumps({'ragged batch': ragged_timing(routes)}))
        return
    frames = [synthetic.flag_frame(seed=i, nx=40, ny=40) for i in range(4)]
    cells = frames[0]['cells'].cuda()
    dev_frames = [{k: (cells if k == 'cells' else v.cuda()) for k, v in f.items()} for f in frames]

    for name, conn in (('build_graph', 'none'), ('build_graph+expand_graph(hyper,K=16)', 'hyper')):
        model = system_model.FlagModel(params(conn, 16))
        def one(i):
            g = model.build_graph(dev_frames[i % 4], True)
            return model.expand_graph(g, 1 + i, 10 ** 9, True) if conn != 'none' else g
        g = model.build_graph(dev_frames[0], True)
        if conn != 'none':
            model.expand_graph(g, 0, 10 ** 9, True)          # clustering: once per trajectory, not per frame
        for i in range(5):
            one(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.frames):
            one(i)
        torch.cuda.synchronize()
        res[name + ' ms/frame (gpu, eager)'] = (time.perf_counter() - t0) / a.frames * 1e3

    # the whole batch of frames in one go (FlagModel.build_graph_batch)
    model = system_model.FlagModel(params('none', 16))
    Bf = 128
    stacked = {k: (torch.stack([frames[i % 4][k] for i in range(Bf)]).cuda() if k not in ('cells', 'mesh_pos') else dev_frames[0][k])
               for k in frames[0]}
    for _ in range(3):
        model.build_graph_batch(stacked, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        model.build_graph_batch(stacked, True)
    torch.cuda.synchronize()
    res['build_graph_batch (128 frames) ms'] = (time.perf_counter() - t0) / 20 * 1e3

    # kernel-level rates at batch size
    B = 64
    s1, r1, _ = features.cells_to_edges(cells)
    N, E1 = 1600, s1.shape[0]
    off = (torch.arange(B, device='cuda') * N).repeat_interleave(E1)
    s, r = (s1.repeat(B) + off).contiguous(), (r1.repeat(B) + off).contiguous()
    world = torch.cat([f['world_pos'] for f in dev_frames] * (B // 4)).contiguous()
    mesh = torch.cat([f['mesh_pos'] for f in dev_frames] * (B // 4)).contiguous()
    E = s.shape[0]
    t = ev_time(lambda: features.rel_edge_features(world, mesh, s, r, want_len=True))
    bytes_rel = E * (16 + 28 + 4) + world.numel() * 4 + mesh.numel() * 4      # ids + row + length; positions once
    res['rel_edge_features'] = {'edges': E, 'ms': t, 'GB/s': bytes_rel / t / 1e6, 'algorithmic_bytes': bytes_rel}
    feat, _ = features.rel_edge_features(world, mesh, s, r)
    t = ev_time(lambda: features.col_stats(feat))
    res['col_stats'] = {'rows': E, 'ms': t, 'GB/s': feat.numel() * 4 / t / 1e6}
    nz = Normalizer(7, 'e')
    nz(feat)
    t = ev_time(lambda: features.normalize(feat, nz._acc_sum, nz._acc_sum_squared, nz._acc_count, 1e-8))
    res['normalize'] = {'rows': E, 'ms': t, 'GB/s': 2 * feat.numel() * 4 / t / 1e6}
    big = torch.cat([frames[0]['cells'] + i * N for i in range(B)]).cuda()
    t0 = time.perf_counter()
    for _ in range(5):
        features.cells_to_edges(big)
    torch.cuda.synchronize()
    res['cells_to_edges (64 meshes, 194 688 cells) ms'] = (time.perf_counter() - t0) / 5 * 1e3

    res['batched builds'] = batched_builds()

    if not a.no_cpu:
        from bench import cpu_baseline_features          # the oracle is timed by bench.py's cpu_baseline code only
        res['cpu oracle'] = cpu_baseline_features(frames)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
