"""Data-parallel training of batches of independent mesh graphs: one process per GPU, RCCL over xGMI.

The reference has no distributed code at all; what must hold is equivalence with the reference's
single-process step on the concatenated batch (MeshSimulator.py:141-152 with FlagModel.training_step, flag.py:146-154):

  * graphs are independent, so the batch shards at graph granularity with NO collective on the data path;
  * the loss is a mean over all NORMAL nodes of the *global* batch: each rank back-propagates its local SUM of squared
    errors, the NORMAL-node count rides in a spare slot behind the gradients, and after the all-reduce everything is scaled
    by 1 / (n_global * out_dim) -- the gradient of the global mean, with no collective between forward and backward;
  * gradients live in ONE flat fp32 buffer (parameter .grad tensors are views into it) and are summed -- together with that
    count -- by a handful of LARGE all-reduces over contiguous ranges of it (default 4 buckets, 9.3 MB in all for the 15-layer
    model: xGMI is point-to-point, ring collectives are per-link bound, so few large collectives beat many small ones), each
    launched as soon as the backward pass has left the layers it covers (last layers first) so that it runs beside the rest
    of the backward pass, and consumed by one fused Adam launch on the flat parameter buffer;
  * Normalizer statistics are sum-reduced across ranks at every accumulate (normalizer.py:53-63) so all replicas
    normalise identically.
"""
from typing import Callable, Iterable, Optional

import torch
import torch.distributed as dist
from torch import nn


def shard_indices(num_graphs: int, rank: int, world: int):
    """Graphs {g : g mod world == rank}."""
    return list(range(rank, num_graphs, world))


class FlatParams:
    """Re-homes every parameter of `module` into one contiguous buffer (and its gradient into a twin buffer).
    Parameter objects keep their identity, names and shapes; only their storage moves."""

    def __init__(self, module: nn.Module):
        params = [p for p in module.parameters() if p.requires_grad]
        lazy = [p for p in params if isinstance(p, nn.parameter.UninitializedParameter)]
        if lazy and not any(isinstance(m, nn.Linear) and not isinstance(m, nn.modules.lazy.LazyModuleMixin) for m in module.modules()):
            raise RuntimeError('materialise the lazy layers (run one forward) before flattening')
        # still lazy after a forward: modules the block schedule never calls (e.g. the `balance` edge model under a hyper block,
        # hypergraphnet.py:54 keeps only its five sets).  They have no gradient and no storage: left alone.
        params = [p for p in params if not isinstance(p, nn.parameter.UninitializedParameter)]
        self.params = params
        self.left_lazy = [n for n, p in module.named_parameters() if isinstance(p, nn.parameter.UninitializedParameter)]
        if self.left_lazy:
            import warnings
            warnings.warn('FlatParams: %d parameter(s) still lazy after the warm-up forward are NOT part of the flat buffer '
                          '(never broadcast, reduced or updated): %s' % (len(self.left_lazy), ', '.join(self.left_lazy[:8]) +
                                                                          (' ...' if len(self.left_lazy) > 8 else '')))
        self._module = module
        self._member = {id(p) for p in params}
        # every parameter starts on a 16-byte boundary: the kernels read biases / LayerNorm affine vectors as float4
        self.offsets = []
        total = 0
        for p in params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        dev = params[0].device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        # one spare 16-byte slot IN FRONT of the gradients: [NORMAL-node count 0 0 0 | grad (total)].  The count travels with the
        # range that holds the FIRST parameters, i.e. with the bucket that is reduced last (the backward pass reaches them last).
        self.grad_ext = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.grad = self.grad_ext[4:]
        self.count = self.grad_ext[0:1]
        for p, off in zip(params, self.offsets):
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view(p.shape)
            p.grad = self.grad[off:off + n].view(p.shape)
            p._hgn_grad = p.grad          # the kernels accumulate straight into this view (ops._grad_targets)
        self.numel = total
        from . import ops
        ops.storage_moved()               # every parameter has a new address: captured forward graphs (graphs.GraphedForward) re-capture

    def check_outsiders(self):
        """A module that was lazy when the buffer was laid out and has been exercised since (a batch with an edge set the warm-up
        graph lacked) owns parameters that no collective and no optimiser step sees: the replicas would diverge silently."""
        if not self.left_lazy:
            return
        bad = [n for n, p in self._module.named_parameters()
               if id(p) not in self._member and p.requires_grad and not isinstance(p, nn.parameter.UninitializedParameter)]
        if bad:
            raise RuntimeError('parameters materialised after FlatParams was built are outside the flat buffer: ' + ', '.join(bad[:8]))

    def zero_grad(self):
        self.grad_ext.zero_()
        for p, off in zip(self.params, self.offsets):     # autograd may have replaced .grad (e.g. after set_to_none)
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * off:
                p.grad = self.grad[off:off + n].view(p.shape)


class LRSchedule:
    """Learning rate of Adam's step t = 1, 2, ... : a linear warm-up over ``warmup_steps`` steps times an exponential decay from
    ``lr`` towards the floor ``lr_min``, by ``decay_rate`` per ``decay_steps`` steps counted from the end of the warm-up (the
    MeshGraphNets recipe: lr 1e-4 + 1e-6, lr_min 1e-6, decay_rate 0.1, decay_steps 5e6):

        lr(t) = w(t) * (lr_min + (lr - lr_min) * decay_rate ** (max(0, t - warmup_steps) / decay_steps)),
        w(t) = min(1, t / warmup_steps) for warmup_steps > 0, else 1;  decay_steps == 0: no decay, the bracket is lr.

    An immutable value (it pickles, compares and hashes by its fields).  `at` is that formula in Python doubles on the fields as
    given; the C ABI (`as_struct` -> hgn_adam_sched_t, what the device kernel evaluates) holds lr, lr_min and decay_rate as
    float, so host and device agree to the last bits of pow for fields that are float32 numbers (`as_float32` rounds them) and
    to 2^-24 relative per field otherwise.  The constructor refuses what the ABI refuses, with ValueError."""
    __slots__ = ('lr', 'warmup_steps', 'decay_steps', 'decay_rate', 'lr_min')

    def __init__(self, lr, warmup_steps=0, decay_steps=0, decay_rate=1.0, lr_min=0.0):
        import math
        lr, decay_rate, lr_min = float(lr), float(decay_rate), float(lr_min)
        for name, n in (('warmup_steps', warmup_steps), ('decay_steps', decay_steps)):
            if isinstance(n, bool) or int(n) != n or not 0 <= int(n) < 2 ** 31:
                raise ValueError(f'LRSchedule: {name} must be an integer in [0, 2^31), got {n!r}')
        if not math.isfinite(lr) or lr < 0:
            raise ValueError(f'LRSchedule: lr must be finite and >= 0, got {lr!r}')
        if not 0.0 <= lr_min <= lr:
            raise ValueError(f'LRSchedule: lr_min must lie in [0, lr], got {lr_min!r}')
        if not 0.0 < decay_rate <= 1.0:
            raise ValueError(f'LRSchedule: decay_rate must lie in (0, 1], got {decay_rate!r}')
        for name, val in (('lr', lr), ('warmup_steps', int(warmup_steps)), ('decay_steps', int(decay_steps)),
                          ('decay_rate', decay_rate), ('lr_min', lr_min)):
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value=None):
        raise AttributeError('LRSchedule is immutable')

    __delattr__ = __setattr__

    def fields(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __reduce__(self):
        return (LRSchedule, tuple(getattr(self, k) for k in self.__slots__))

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.fields() == other.fields()

    def __hash__(self):
        return hash(tuple(self.fields().items()))

    def __repr__(self):
        return 'LRSchedule(%s)' % ', '.join(f'{k}={v!r}' for k, v in self.fields().items())

    def at(self, t: int) -> float:
        """The rate of step t >= 1 (hgn_lr_at's formula, operation for operation)."""
        if int(t) != t or t < 1:
            raise ValueError(f'LRSchedule.at: steps count from 1, got {t!r}')
        t = int(t)
        rate = self.lr
        if self.decay_steps > 0:
            rate = self.lr_min + (self.lr - self.lr_min) * self.decay_rate ** (float(max(0, t - self.warmup_steps)) / float(self.decay_steps))
        if self.warmup_steps > 0 and t < self.warmup_steps:
            rate = (float(t) / float(self.warmup_steps)) * rate
        return rate

    def as_float32(self) -> 'LRSchedule':
        """The schedule the device evaluates: lr, lr_min and decay_rate rounded to float32."""
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
        lr = f32(self.lr)
        return LRSchedule(lr, self.warmup_steps, self.decay_steps, min(1.0, f32(self.decay_rate)), min(lr, f32(self.lr_min)))

    def as_struct(self, weight_decay: float = 0.0):
        """-> _lib.AdamSched (hgn_adam_sched_t) with this schedule and ``weight_decay``."""
        from . import _lib
        _check_weight_decay(self.lr, weight_decay)
        return _lib.AdamSched(self.lr, self.lr_min, self.warmup_steps, self.decay_steps, self.decay_rate, float(weight_decay))


def _check_weight_decay(lr, weight_decay):
    import math
    wd = float(weight_decay)
    if not math.isfinite(wd) or wd < 0:
        raise ValueError(f'weight_decay must be finite and >= 0, got {weight_decay!r}')
    if lr * wd >= 1.0:
        raise ValueError(f'lr * weight_decay must be < 1, got {lr!r} * {wd!r}')


def _torch_adam(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, weight_decay=0.0, decay_mask=None):
    """Reference-semantics Adam on flat tensors (used only where the HIP kernel cannot run: CPU gloo tests).  ``weight_decay``:
    torch.optim.AdamW's decoupled decay, p *= 1 - lr * weight_decay before the update, where ``decay_mask`` (None: everywhere)
    is not zero."""
    g = g * grad_scale
    if weight_decay > 0:
        if decay_mask is None:
            p.mul_(1 - lr * weight_decay)
        else:
            p.mul_(torch.where(decay_mask != 0, 1 - lr * weight_decay, 1.0).to(p.dtype))
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    p.addcdiv_(m, (v.sqrt() / (bc2 ** 0.5)).add_(eps), value=-lr / bc1)


def _map_tensors(obj, fn):
    """Apply fn to every tensor of a nested output (tensor, list / tuple, dict, or an object with `nodes` / `edges` such as
    modules._Latent); returns a structure of the same kind."""
    if isinstance(obj, torch.Tensor):
        return fn(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map_tensors(x, fn) for x in obj)
    if isinstance(obj, dict):
        return type(obj)((k, _map_tensors(v, fn)) for k, v in obj.items())
    if hasattr(obj, 'nodes') and hasattr(obj, 'edges'):
        import copy
        out = copy.copy(obj)
        out.nodes, out.edges = _map_tensors(obj.nodes, fn), _map_tensors(obj.edges, fn)
        return out
    return obj


class _BucketMark(torch.autograd.Function):
    """Identity on every tensor that crosses a bucket boundary of the model.  Its backward runs when the gradients of ALL of
    them are ready, i.e. when the backward pass has left every layer behind the boundary: the gradients of those layers'
    parameters are then complete (enqueued on the stream) and their range of the flat buffer can be reduced."""

    @staticmethod
    def forward(ctx, on_backward, *xs):
        ctx.on_backward = on_backward
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for x in xs)

    @staticmethod
    def backward(ctx, *gs):
        ctx.on_backward()
        return (None, *gs)


class _DetachedHook:
    """What a bucket-boundary hook becomes in a pickle / deep copy of the model: the copy belongs to no trainer."""

    def __call__(self, module, inputs, output):
        return None


class _BucketHook:
    """Forward hook at a bucket boundary (DataParallelTrainer._plan_buckets): threads a _BucketMark through the tensors that cross
    it.  A class instead of a closure so that a model with hooks installed still pickles (the reference checkpoints by
    `pickle.dump` of the object that holds the network, MeshSimulator.py:492-493): the hook itself is left out of the pickle."""

    def __init__(self, trainer, start: int):
        self.trainer, self.start = trainer, start

    def __reduce__(self):
        return (_DetachedHook, ())

    def _on_backward(self):
        self.trainer._reduce_from(self.start)

    def __call__(self, module, inputs, output):
        if not (self.trainer.overlap and torch.is_grad_enabled()):
            return None
        tensors = []
        _map_tensors(output, lambda x: tensors.append(x) or x)
        live = [x for x in tensors if x.requires_grad]
        if not live:
            return None
        marked = iter(_BucketMark.apply(self._on_backward, *live))
        return _map_tensors(output, lambda x: next(marked) if x.requires_grad else x)


class DataParallelTrainer:
    """fwd -> global-mean masked MSE -> bwd beside bucketed all-reduces -> fused Adam, on this rank's shard of the batch.

    ``buckets``: number of contiguous ranges the flat gradient buffer is reduced in (world > 1).  Boundaries are put between the
    message-passing blocks of a MeshGraphNet (``model.processor.graphnet_blocks``; ``bucket_after`` names other modules) so
    that the ranges hold about equal numbers of parameters; range k is all-reduced (asynchronously: RCCL's own stream, after
    the gradient kernels enqueued so far) from an autograd node at its boundary, while the backward pass goes on through the
    earlier layers.  The range of the first parameters goes last, after ``backward()`` has returned, and carries the node
    count.  The result is the same sum as one all-reduce of the whole buffer (every element is reduced exactly once).

    ``max_grad_norm``: clip the gradient of the global-mean loss by its global norm (torch.nn.utils.clip_grad_norm_'s formula)
    before Adam; ``skip_nonfinite``: a step whose gradient holds an inf or a NaN changes neither the parameters, nor m, v, nor
    the step count.  Both are device-side parts of the step, after the collective and the global-mean scaling
    (ops.grad_norm_clip -> ops.adam_step_clip: no host read, so a captured step keeps them), computed by every rank from the
    same all-reduced bits with a deterministic kernel: replicas stay bit-equal.  Either one puts the Adam step counter on the
    device (`t_dev`, created if ``device_step`` is off).  `grad_stats` ([norm, coef] of the last step) and `skipped_dev` (the
    number of skipped steps) are device tensors the trainer never reads: a caller logs them when it wants.  With both unset the
    step is launch for launch what it is without them.  On the device the clipped update is the library's own kernel, as with
    ``device_step``; an ``adam_fn`` is called for CPU tensors only (with the coefficient as its ``grad_scale``), and
    ``skip_nonfinite`` refuses any but `_torch_adam`.

    ``lr_schedule`` (an `LRSchedule`) and ``weight_decay`` (decoupled, torch.optim.AdamW's: p *= 1 - lr_t * weight_decay before
    the update, with the step's rate): the rate of a step is formed ON THE DEVICE from the step counter
    (ops.adam_step_sched in place of ops.adam_step_dev / ops.adam_step_clip), so a captured step replays a rate that moves.
    Either one puts the step counter on the device and creates `lr_dev`, one fp32 device element with the rate of the last
    counted step, which the trainer never reads.  ``weight_decay`` alone means the constant schedule at ``lr``.
    ``decay_filter(name, param) -> bool`` selects the tensors that decay; the default takes those with ``dim() >= 2`` (weights,
    not biases or LayerNorm vectors).  `decay_mask` is the uint8 mask over the flat buffer, built once, None when every tensor
    decays.  A skipped step decays nothing.  With both unset the step is launch for launch what it is without them.  CPU
    tensors take the same arithmetic in torch, with lr = schedule.at(step); ``weight_decay`` refuses an ``adam_fn`` other than
    `_torch_adam`.

    `state_dict()` / `load_state_dict()` carry the optimiser's side of a run -- m, v, the counters, the hyper-parameters, the
    layout of the flat buffer -- so that a run resumed from the model's and the trainer's state continues bit for bit."""

    def __init__(self, model: nn.Module, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 group: Optional[dist.ProcessGroup] = None, adam_fn: Optional[Callable] = None,
                 device_step: bool = False, wgrad_stream: bool = False, buckets: int = 4, bucket_after=None,
                 force_collectives: bool = False, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 lr_schedule: Optional[LRSchedule] = None, weight_decay: float = 0.0, decay_filter: Optional[Callable] = None):
        self.model = model
        from . import ops as _ops
        self.ctx = getattr(model, '_hgn_ctx', None) or _ops.default_context()      # the launch context of the model it trains (ops.Context)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # (force_collectives: a world of ONE rank still broadcasts / all-reduces -- the N > 1 code path rehearsed on one GPU over RCCL)
        self.collectives = self.world > 1 or (force_collectives and dist.is_available() and dist.is_initialized())
        self.fp = FlatParams(model)
        if self.collectives:                                         # identical replicas: rank 0's weights win
            dist.broadcast(self.fp.flat, src=0, group=group)
        self.m = torch.zeros_like(self.fp.flat)
        self.v = torch.zeros_like(self.fp.flat)
        self.t = 0
        # device-resident step counter: needed when step() is captured into a HIP graph (graphs.GraphedTrainStep)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=self.fp.flat.device) if device_step else None
        # clipping by the global norm / skipping a non-finite step: device-side parts of the step (class docstring)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.clip = self.max_grad_norm is not None or self.skip_nonfinite
        if self.skip_nonfinite and adam_fn is not None and adam_fn is not _torch_adam:
            raise ValueError('skip_nonfinite needs the trainer\'s own update (a skipped step must leave p, m and v untouched): '
                             'no adam_fn other than parallel._torch_adam')
        self.grad_stats = self.skipped_dev = None
        if self.clip:
            dev = self.fp.flat.device
            if self.t_dev is None:                                   # the skip decision is made on the device: so is the step count
                self.t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self.grad_stats = torch.zeros(2, dtype=torch.float32, device=dev)      # [norm, coef] of the last step; never read here
            self.skipped_dev = torch.zeros(1, dtype=torch.int32, device=dev)       # steps skipped as non-finite
        # learning-rate schedule / decoupled weight decay: the rate is formed on the device from the step counter (class docstring)
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError('lr_schedule must be a parallel.LRSchedule')
        self.weight_decay = float(weight_decay)
        self.lr_schedule = lr_schedule
        self.sched = lr_schedule if lr_schedule is not None else (LRSchedule(lr) if self.weight_decay != 0 else None)
        _check_weight_decay(self.sched.lr if self.sched is not None else lr, weight_decay)
        if self.weight_decay > 0 and adam_fn is not None and adam_fn is not _torch_adam:
            raise ValueError('weight_decay needs the trainer\'s own update (the decay is part of it): no adam_fn other than '
                             'parallel._torch_adam')
        self.lr_dev = self.decay_mask = self._sched_struct = None
        if self.sched is not None:
            dev = self.fp.flat.device
            if self.t_dev is None:                                   # the rate follows the device's step count
                self.t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self.lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)          # rate of the last counted step; never read here
            self._sched_struct = self.sched.as_struct(self.weight_decay)
            if self.weight_decay > 0:
                self.decay_mask = self._build_decay_mask(decay_filter)
        if adam_fn is None:
            from . import ops
            adam_fn = ops.adam_step
        self.adam_fn = adam_fn
        self.side = torch.cuda.Stream() if (wgrad_stream and self.fp.flat.is_cuda) else None
        self.overlap = True                                        # False: every range after the backward pass (graphs.GraphedShardStep)
        self._pending, self._done_upto = [], None
        self.bucket_starts = self._plan_buckets(max(1, int(buckets)), bucket_after) if self.collectives else []

    def _build_decay_mask(self, decay_filter):
        """uint8 over the flat buffer: 1 on the elements of the tensors ``decay_filter(name, param)`` selects (default: dim() >= 2);
        None when it selects every tensor (the padding between tensors holds zeros, which decay to zeros)."""
        if decay_filter is None:
            decay_filter = lambda name, param: param.dim() >= 2
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        chosen = [bool(decay_filter(name_of[id(p)], p)) for p in self.fp.params]
        if all(chosen):
            return None
        mask = torch.zeros(self.fp.numel, dtype=torch.uint8)
        for p, off, yes in zip(self.fp.params, self.fp.offsets, chosen):
            if yes:
                mask[off:off + p.numel()] = 1
        return mask.to(self.fp.flat.device)

    # ---- bucket plan ------------------------------------------------------------------------------------------------
    def _plan_buckets(self, n_buckets: int, bucket_after):
        """-> ascending offsets (into grad_ext) at which a new range starts; installs the boundary hooks."""
        if bucket_after is None:
            proc = getattr(getattr(self.model, 'processor', None), 'graphnet_blocks', None)
            blocks = list(proc) if proc is not None else []
            offset_of = {id(p): off for p, off in zip(self.fp.params, self.fp.offsets)}
            firsts = []                                            # (flat offset of a block's first parameter, block before it)
            for i in range(1, len(blocks)):
                ps = [p for p in blocks[i].parameters() if id(p) in offset_of]
                if ps:
                    firsts.append((min(offset_of[id(p)] for p in ps), blocks[i - 1]))
            chosen = []
            for k in range(1, n_buckets):                          # the boundary nearest to k / n_buckets of the buffer
                want = self.fp.numel * k / n_buckets
                if firsts:
                    best = min(firsts, key=lambda f: abs(f[0] - want))
                    if best not in chosen:
                        chosen.append(best)
            boundaries = sorted(chosen, key=lambda f: f[0])
        else:
            offset_of = {id(p): off for p, off in zip(self.fp.params, self.fp.offsets)}
            boundaries = []
            for mod_before, mod_after in bucket_after:            # explicit: (module whose output is the boundary, first module behind it)
                ps = [p for p in mod_after.parameters() if id(p) in offset_of]
                boundaries.append((min(offset_of[id(p)] for p in ps), mod_before))
            boundaries.sort(key=lambda f: f[0])
        starts = []
        for off, module in boundaries:
            start = off + 4                                        # (grad_ext = [count slot | grad])
            starts.append(start)
            module.register_forward_hook(self._make_hook(start))
        return starts

    def _make_hook(self, start: int):
        return _BucketHook(self, start)

    def _reduce_from(self, start: int):
        """All-reduce grad_ext[start : the range already under way), asynchronously."""
        end = self._done_upto if self._done_upto is not None else self.fp.grad_ext.numel()
        if start >= end:
            return
        if self.fp.flat.is_cuda:
            from . import ops
            ops.flush_wgrad(self.ctx)                              # queued node-level weight-gradient tasks of these layers
            if self.side is not None:
                torch.cuda.current_stream().wait_stream(self.side)
        self._pending.append(dist.all_reduce(self.fp.grad_ext[start:end], group=self.group, async_op=True))
        self._done_upto = start

    def step(self, graph, target: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        self.fp.check_outsiders()
        self.fp.zero_grad()
        self._pending, self._done_upto = [], None
        if self.fp.flat.is_cuda:
            from . import ops
            ops.discard_stale_wgrad(self.ctx)                        # tasks a failed backward pass left queued belong to no step
        if self.side is not None:
            from . import ops
            self.side.wait_stream(torch.cuda.current_stream())      # the zeroed gradient buffer is visible to the side stream
            self.ctx.wgrad_stream = self.side
        # (the count rides in the LAST range: written before the backward pass, reduced after it)
        self.fp.count.copy_(mask.sum().to(torch.float32).reshape(1))
        if self.fp.flat.is_cuda:
            ops.begin_step_packs(self.ctx)                            # one launch refreshes every packed weight image of the step
        out = self.model(graph)
        diff = (out - target) * mask.unsqueeze(1).to(out.dtype)       # masked without boolean indexing: no host sync, capturable
        sq = diff.square().sum()                                      # local SUM; scaled to the global mean after the collective
        sq.backward()
        if self.fp.flat.is_cuda:
            ops.end_step_packs(self.ctx)
        if self.side is not None:
            self.ctx.wgrad_stream = None
            torch.cuda.current_stream().wait_stream(self.side)      # join: all weight gradients are in the flat buffer
        return self.reduce_and_update(sq.detach(), out.shape[1])

    def step_unrolled(self, system_model, windows, n_steps: int, through_state: bool = True, is_training: bool = True,
                      noise_draw=None, frame_ids=None, checkpoint=None):
        """One optimiser step on the loss of an ``n_steps`` rollout unrolled under autograd
        (`system_model.unrolled_training_step`, whose arguments these are) with everything `step` gives a single step: the flat
        gradient buffer the kernels accumulate into, the all-reduce, the global-mean scaling, clipping and the fused Adam.
        ``system_model.learned_model`` must be this trainer's model.  ``windows`` are THIS RANK's windows: the caller shards them
        (`shard_indices`) and passes their global ids as ``frame_ids``, so that with ``noise_draw`` every window gets the noise
        sample a single process gives it; normaliser statistics are shared through `attach_normalizer_sync`.
        The loss is the mean over the free rows (`_loss_mask`: the same rows at every step) of this rank's W * N rows; the rank
        back-propagates loss * count with count = its number of free rows, which rides in the count slot, so that after the
        collective  sum_r(count_r * grad loss_r) / sum_r count_r  is the gradient of the mean over ALL windows, for any shard sizes.
        -> (this rank's share loss_r * count_r / sum count of that global mean, the per-step losses of this rank's windows).
        Collectives: the bucket hooks would fire once per network call, and a range may only leave after the LAST backward visit
        of its boundary; this step therefore runs with `overlap` off -- ONE collective over the whole buffer after backward(), as
        the captured path does -- and restores the setting.
        Packed weight images: the weights do not change inside the step and every network call asks for the same images.  The
        recording step (ops.begin_step_packs without a plan) sees every (MLP, form) pair n_steps times, PackPlan keeps each once;
        in later steps the plan's one launch refreshes them all before the first call and sets `plan_epoch`, after which every
        packs_of of the step -- calls 2 .. n_steps included -- finds its cached image under an unchanged key.  A plan recorded by
        `step` serves this method and the other way round (the same MLPs).
        ``checkpoint`` is handed on (None / False: the step above, launch for launch; True: activation checkpointing, see
        `unrolled_training_step`).  The rebuilt steps run inside this step's backward pass, i.e. between ops.begin_step_packs and
        ops.end_step_packs, with `overlap` off and the side stream set: they find the packed images of the first pass cached (a
        plan recorded by either kind of step serves the other), their weight gradients accumulate into the flat buffer step by step
        (ops.nested_backward: the deferred queue is flushed when a rebuilt step starts and when it ends, so slab workspaces live for
        one step), and the one collective still follows backward().
        Out of scope: HIP-graph capture of the unrolled step; a graph balancer; meshes that differ within a batch."""
        if checkpoint is not None and not isinstance(checkpoint, bool):
            raise TypeError(f'step_unrolled: checkpoint must be None, False or True, not {checkpoint!r}')
        if getattr(system_model, 'learned_model', None) is not self.model:
            raise ValueError('step_unrolled: system_model.learned_model is not the model this trainer was built on')
        self.fp.check_outsiders()
        self.fp.zero_grad()
        self._pending, self._done_upto = [], None
        cuda = self.fp.flat.is_cuda
        if cuda:
            from . import ops
            ops.discard_stale_wgrad(self.ctx)
        if self.side is not None:
            self.side.wait_stream(torch.cuda.current_stream())
            self.ctx.wgrad_stream = self.side
        node_type = windows['node_type'][:, 0]
        count = system_model._loss_mask({'node_type': node_type.reshape(-1, node_type.shape[-1])}).sum().to(torch.float32).reshape(1)
        self.fp.count.copy_(count)
        overlap, self.overlap = self.overlap, False
        try:
            if cuda:
                ops.begin_step_packs(self.ctx)
            loss, per_step = system_model.unrolled_training_step(windows, n_steps, through_state=through_state, is_training=is_training,
                                                                 noise_draw=noise_draw, frame_ids=frame_ids, checkpoint=checkpoint)
            (loss * count).backward()           # (`count`, not the slot: the slot shares its version counter with the gradients)
        finally:
            self.overlap = overlap
            if cuda:
                ops.end_step_packs(self.ctx)
            if self.side is not None:
                self.ctx.wgrad_stream = None
                torch.cuda.current_stream().wait_stream(self.side)
        return self.reduce_and_update(loss.detach() * count, 1), per_step

    def reduce_and_update(self, sq_local: torch.Tensor, width: int) -> torch.Tensor:
        """[local NORMAL-node count | gradients of the local squared-error sum] -> all-reduce (the ranges not yet under way; with
        nothing under way -- captured backward pass -- ONE collective over the whole buffer) -> scale to the gradient of the global mean (flag.py:150-152
        over the whole batch) -> fused Adam.  Returns this rank's share of the global-mean loss."""
        if self.collectives:
            # (no boundary fired -- world of one bucket, or a captured backward pass, graphs.GraphedShardStep, where nothing can
            # be overlapped: ONE collective over the whole buffer; otherwise the range of the first parameters + the count)
            self._reduce_from(0)
            for w in self._pending:
                w.wait()
            self._pending, self._done_upto = [], None
        inv = 1.0 / (self.fp.count * width)
        self.fp.grad.mul_(inv)
        self.t += 1
        if self.clip:
            self._clipped_update()
        elif self.sched is not None:
            self._scheduled_update()
        elif self.t_dev is not None:
            from . import ops
            ops.adam_step_dev(self.fp.flat, self.fp.grad, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps, self.t_dev)
        else:
            self.adam_fn(self.fp.flat, self.fp.grad, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps, self.t)
        if self.fp.flat.is_cuda:
            from . import ops
            self.ctx.invalidate_packs()             # the Adam kernel rewrote the parameters behind torch's version counters
        return (sq_local * inv).squeeze(0)

    def _clipped_update(self):
        """norm of the global-mean gradient -> [norm, coef] in `grad_stats`, step / skip counters -> Adam on coef * gradient.
        On the device two launches and one (ops.grad_norm_clip, ops.adam_step_clip), no host read; CPU tensors (the gloo host
        tests) take the same arithmetic in torch: the norm in fp64, clip_grad_norm_'s coefficient, the skip."""
        fp, (b1, b2) = self.fp, self.betas
        if fp.flat.is_cuda:
            from . import ops
            with ops.using(self.ctx):
                ops.grad_norm_clip(fp.grad, self.max_grad_norm, self.grad_stats, self.t_dev, self.skipped_dev, self.skip_nonfinite)
            if self.sched is not None:
                ops.adam_step_sched(fp.flat, fp.grad, self.m, self.v, self._sched_struct, b1, b2, self.eps, self.t_dev, count_step=False,
                                    coef=self.grad_stats[1:2], decay_mask=self.decay_mask, lr_out=self.lr_dev)
            else:
                ops.adam_step_clip(fp.flat, fp.grad, self.m, self.v, self.lr, b1, b2, self.eps, self.t_dev, self.grad_stats[1:2])
            return
        total = fp.grad.double().square().sum()
        norm = total.sqrt()
        coef = 1.0
        if self.max_grad_norm is not None and self.max_grad_norm > 0:
            c = self.max_grad_norm / (float(norm) + 1e-6)
            coef = float(torch.tensor(c, dtype=torch.float32)) if c < 1.0 else 1.0
        if self.skip_nonfinite and not bool(torch.isfinite(total)):
            coef = 0.0
            self.skipped_dev += 1
        else:
            self.t_dev += 1
        self.grad_stats[0], self.grad_stats[1] = norm.to(torch.float32), coef
        if coef != 0.0:
            self.adam_fn(fp.flat, fp.grad, self.m, self.v, self._host_rate(), b1, b2, self.eps, int(self.t_dev), grad_scale=coef,
                         **self._decay_keywords())

    def _host_rate(self) -> float:
        """CPU tensors: the rate of the step `t_dev` has just counted (and `lr_dev`), or the constant one."""
        if self.sched is None:
            return self.lr
        lr = self.sched.at(int(self.t_dev))
        self.lr_dev.fill_(lr)
        return lr

    def _decay_keywords(self):
        return dict(weight_decay=self.weight_decay, decay_mask=self.decay_mask) if self.weight_decay > 0 else {}

    def _scheduled_update(self):
        """Adam at the schedule's rate with decoupled weight decay, no clipping: one ops.adam_step_sched, which counts the step and
        forms the rate from the count on the device; CPU tensors: the same in torch at lr = schedule.at(step)."""
        fp, (b1, b2) = self.fp, self.betas
        if fp.flat.is_cuda:
            from . import ops
            ops.adam_step_sched(fp.flat, fp.grad, self.m, self.v, self._sched_struct, b1, b2, self.eps, self.t_dev, count_step=True,
                                decay_mask=self.decay_mask, lr_out=self.lr_dev)
            return
        self.t_dev += 1
        self.adam_fn(fp.flat, fp.grad, self.m, self.v, self._host_rate(), b1, b2, self.eps, int(self.t_dev), **self._decay_keywords())

    # ---- resume -----------------------------------------------------------------------------------------------------
    _STATE_TENSORS = ('m', 'v', 't_dev', 'skipped_dev', 'grad_stats', 'lr_dev')

    def _hyper_parameters(self):
        sched = self.lr_schedule.fields() if self.lr_schedule is not None else None
        return {'lr': float(self.lr), 'betas': [float(b) for b in self.betas], 'eps': float(self.eps), 'lr_schedule': sched,
                'weight_decay': self.weight_decay, 'max_grad_norm': self.max_grad_norm, 'skip_nonfinite': self.skip_nonfinite}

    def _layout(self):
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        return {'names': [name_of[id(p)] for p in self.fp.params], 'offsets': [int(o) for o in self.fp.offsets],
                'sizes': [int(p.numel()) for p in self.fp.params], 'numel': int(self.fp.numel)}

    def state_dict(self):
        """The optimiser's side of the run as CPU tensors and plain values (torch.save / torch.load(weights_only=True)): m, v, the
        host step count `t`, the device tensors that exist (t_dev, skipped_dev, grad_stats, lr_dev), the hyper-parameters and the
        layout of the flat buffer (parameter names, offsets, sizes).  The parameters travel in the model's state_dict."""
        state = {'t': int(self.t), 'hyper_parameters': self._hyper_parameters(), 'layout': self._layout()}
        for k in self._STATE_TENSORS:
            x = getattr(self, k)
            if x is not None:
                state[k] = x.detach().cpu().clone()
        return state

    def load_state_dict(self, state):
        """Take over m, v and the counters of `state_dict()`'s result, IN PLACE (captured graphs hold the tensors' addresses).  A
        flat-buffer layout that differs from this trainer's raises ValueError naming the first difference; hyper-parameters that
        differ are reported with a warning and this trainer's own stay in force.  The parameters are not touched: load the model's
        state_dict (before or after)."""
        mine, theirs = self._layout(), state['layout']
        for i, (a, b) in enumerate(zip(zip(mine['names'], mine['offsets'], mine['sizes']),
                                       zip(theirs['names'], theirs['offsets'], theirs['sizes']))):
            if a != b:
                raise ValueError('load_state_dict: the flat buffer is laid out differently: parameter %d is %s at offset %d with %d '
                                 'elements here, %s at offset %d with %d elements in the state' % ((i,) + a + b))
        if len(mine['names']) != len(theirs['names']) or mine['numel'] != theirs['numel']:
            raise ValueError('load_state_dict: the flat buffer is laid out differently: %d parameters in %d elements here, %d in %d '
                             'in the state' % (len(mine['names']), mine['numel'], len(theirs['names']), theirs['numel']))
        have, saved = self._hyper_parameters(), state.get('hyper_parameters', {})
        differ = [f'{k}: {have[k]!r} here, {saved.get(k)!r} in the state' for k in have if saved.get(k) != have[k]]
        if differ:
            import warnings
            warnings.warn('load_state_dict: hyper-parameters differ, this trainer\'s own stay in force -- ' + '; '.join(differ))
        for k in ('m', 'v'):
            if tuple(state[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f'load_state_dict: {k} has {tuple(state[k].shape)} elements, the flat buffer {tuple(self.m.shape)}')
        for k in self._STATE_TENSORS:
            x = getattr(self, k)
            if x is None:
                continue
            if k in state:
                x.copy_(state[k])
            elif k == 't_dev':                                       # saved by a trainer that counted on the host
                x.fill_(int(state['t']))
        self.t = int(state['t'])
        if self.fp.flat.is_cuda:
            self.ctx.invalidate_packs()


def attach_normalizer_sync(normalizers: Iterable, group: Optional[dist.ProcessGroup] = None):
    """Make every Normalizer accumulate GLOBAL batch statistics: (count, sum, sum^2) are sum-all-reduced."""
    def reduce_fn(count, data_sum, sq_sum):
        packed = torch.cat([count.reshape(1), data_sum.reshape(-1), sq_sum.reshape(-1)])
        dist.all_reduce(packed, group=group)
        n = data_sum.numel()
        return packed[:1], packed[1:1 + n].view_as(data_sum), packed[1 + n:].view_as(sq_sum)
    for nz in normalizers:
        nz._reduce_fn = reduce_fn
