"""System models with the reference's class API (src/model/abstract_system_model.py, flag.py, cylinder.py, plate.py): frame ->
graph features on the device, remote-graph expansion, training / validation step, one-step update and rollout around
the MI355X message-passing model.

Per frame the reference runs ~40 small torch ops plus Python loops; here ``build_graph`` is a fixed handful of HIP
launches (include/hgn_features.h): node features, relative edge features (+ edge lengths), one segment max/min pass
for the node dynamics, and three launches per normaliser.  The mesh topology (cells -> two-way edges, receiver CSR) is
computed once per ``cells`` tensor and reused for the whole trajectory (the reference recomputes it every frame,
flag.py:76-78).
"""
import contextlib
import math
from functools import reduce
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import nn, Tensor

from . import _lib, features, ops, topology
from . import rmp as _rmp
from .modules import MeshGraphNet
from .normalizer import Normalizer
from .util import EdgeSet, MultiGraph, MultiGraphWithPos, NodeType, device


def _value(t: Tensor) -> Tensor:
    """The tensor as a plain value (what `node_dynamic` and `unnormalized_edges` carry): itself unless it requires grad."""
    return t.detach() if t.requires_grad else t


def _carries_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.is_floating_point() and t.requires_grad for t in tensors)


def _masked_mse(target: Tensor, output: Tensor, mask: Tensor) -> Tensor:
    """MSELoss()(target[mask], output[mask]) (flag.py:150-152) without the boolean-index host sync."""
    m = mask.to(output.dtype).unsqueeze(1)
    return (((output - target) ** 2) * m).sum() / (m.sum() * output.shape[1])


class LockStep(NamedTuple):
    """What one model integrates, one instance per model class: read by `_loss_mask`, `validation_step`, `rollout_batch` and
    `unrolled_training_step`.  `d`, `ca`, `cp`, `free_types` and the fallback are the arguments of features.rollout_advance /
    advance_state: next = ca * state + output[:, :d] + cp * previous on the rows whose node type is free, the fallback elsewhere."""
    state: str                      # the series that is integrated
    prev: Optional[str]             # the series that receives the old state, or None
    d: int
    ca: float
    cp: float
    free_types: Tuple[int, ...]     # node types that are integrated (and enter the loss)
    per_step: Tuple[str, ...]       # the per-step series get_target reads
    fallback: Optional[str]         # the per-step series a row that is not free is put on; None: it keeps its own state
    differentiable: bool            # whether build_graph_batch is differentiable with respect to the state without `position_gradients`
    expand_steps: Optional[int]     # the num_steps a rollout hands to expand_graph_batch; None: the call's own
    record_before: bool             # a rollout records the state before the step (else the new one)
    inv_from: Optional[int]         # `inv_out` holds the inverse-normalised output columns from here on; None: not recorded
    errors: str                     # the series the recorded states are compared against
    target: str                     # the series validation_step compares the updated state against


class _CheckpointedStep(torch.autograd.Function):
    """One step of `unrolled_training_step(checkpoint=True)` as ONE autograd node: (model, frame, names, (W, t, n_steps, accumulate,
    last), the frame's tensors that require grad, the network's parameters that require grad) -> (loss, next state [W*N, d]; None
    for the last step).

    Forward of a step but the last: `_unroll_step` without gradients (a Function's forward runs that way), so the kernels take their
    inference forms and nothing of the step survives but what the node keeps: the frame -- its input state, the per-step series (views
    of the windows; at step 0 the noised frame-0 series), the shared mesh --, the clusters the step expanded with, the statistics
    every accumulating normaliser call normalised with (Normalizer.record: a few numbers per call) and the generator states from
    before a step that draws (the connector's `hyper_noise`, drawn where the step accumulates).
    Its backward: the step is rebuilt with gradients from fresh leaves of the stored state under `_rebuilding` (the first pass's
    statistics, clusters and draws) and back-propagated at once, as an engine run of its own inside ops.nested_backward, with the
    gradients that arrived for the loss and the next state (none for the state: `advance_state` is not run again).
    The last step is not rebuilt: its forward runs with gradients on leaves of its own and the node keeps that graph until its
    backward, which back-propagates it the same way and lets go of it.  (As plain autograd nodes the step's functions would hold
    their saves -- MLPFn and EdgeBlockFn keep them on the node, not with save_for_backward -- for as long as the loss is alive,
    i.e. under every rebuild.)
    What a backward returns for the frame's tensors and the parameters travels on through the outer run -- which visits these nodes
    from the last step to the first, so every target receives its contributions in the plain step's order -- and the step's
    activations die with the call, before the step before is rebuilt.  Parameters that accumulate into a trainer's flat buffer
    report None here, as ever."""
    FIXED = 4                                     # arguments in front of the tensors

    @staticmethod
    def forward(ctx, model, frame, names, meta, *tensors):
        W, t, n_steps, accumulate, last = meta
        ctx.set_materialize_grads(False)
        ctx.model, ctx.names, ctx.meta = model, names, meta
        ctx.weights = tensors[len(names):]
        if last:
            frame = dict(frame)
            for name in names:
                frame[name] = frame[name].detach().requires_grad_(True)
            with torch.enable_grad():
                loss, _, _ = model._unroll_step(frame, W, t, n_steps, accumulate, advance=False)
            ctx.live = ([frame[name] for name in names], loss)
            return loss.detach(), None
        ctx.frame = {name: x for name, x in frame.items() if name not in names}
        ctx.save_for_backward(*tensors[:len(names)])
        ctx.rng = (torch.get_rng_state(), torch.cuda.get_rng_state()) if accumulate and model._rmp else None
        normalizers = model._normalizers()
        for m in normalizers:
            m.record = []
        try:
            loss, nxt, _ = model._unroll_step(frame, W, t, n_steps, accumulate, advance=True, eager=True)
        finally:
            ctx.statistics = [m.__dict__.pop('record') for m in normalizers]
        ctx.clusters = (model._remote_graph._clusters, model._remote_graph._neighbors) if model._rmp else None
        return loss, nxt

    @staticmethod
    def backward(ctx, g_loss, g_next):
        model, (W, t, n_steps, accumulate, last) = ctx.model, ctx.meta
        launch_ctx = model.learned_model.__dict__.get('_hgn_ctx') or ops.default_context()
        needed = ctx.needs_input_grad[_CheckpointedStep.FIXED:]
        grads = {}
        if last:
            if ctx.live is None:
                raise RuntimeError('unrolled_training_step(checkpoint=True): the loss was back-propagated a second time; a checkpointed '
                                   'unroll frees every step as its backward pass leaves it, so it can be differentiated once '
                                   '(retain_graph has no effect) -- call it again, or take the plain step (checkpoint=None)')
            (leaves, loss), ctx.live = ctx.live, None
            inputs = leaves + list(ctx.weights)
            wanted = [x for x, need in zip(inputs, needed) if need]
            with ops.nested_backward(launch_ctx):
                if g_loss is not None and wanted and loss.requires_grad:
                    grads = dict(zip(map(id, wanted), torch.autograd.grad([loss], wanted, [g_loss], allow_unused=True)))
                del loss
            return (None,) * _CheckpointedStep.FIXED + tuple(grads.get(id(x)) for x in inputs)
        frame = dict(ctx.frame)
        for name, x in zip(ctx.names, ctx.saved_tensors):
            frame[name] = x.detach().requires_grad_(True)
        inputs = [frame[name] for name in ctx.names] + list(ctx.weights)
        wanted = [x for x, need in zip(inputs, needed) if need]
        with ops.nested_backward(launch_ctx), torch.enable_grad(), model._rebuilding(ctx.clusters, ctx.rng, ctx.statistics):
            loss, nxt, _ = model._unroll_step(frame, W, t, n_steps, accumulate, advance=g_next is not None, refresh=False)
            pairs = [(out, g) for out, g in ((loss, g_loss), (nxt, g_next)) if g is not None and out.requires_grad]
            if pairs and wanted:
                got = torch.autograd.grad([out for out, _ in pairs], wanted, [g for _, g in pairs], allow_unused=True)
                grads = dict(zip(map(id, wanted), got))
            del loss, nxt, pairs
        return (None,) * _CheckpointedStep.FIXED + tuple(grads.get(id(x)) for x in inputs)


class AbstractSystemModel(nn.Module):
    """The reference's system-model base (abstract_system_model.py:10-190) together with the constructor logic its three
    subclasses repeat (flag.py:21-63, cylinder.py:21-63, plate.py:21-67): normalisers, the optional graph balancer and remote
    message passing stages, and the learned MeshGraphNet over the resulting edge-set names.  Attribute names that the
    reference's trainer / pickles touch (`learned_model`, `_*_normalizer`, `_rmp`, `_balancer`, `_remote_graph`,
    `_graph_balancer`, `message_passing_steps`, ...) are kept."""
    _model_type = None
    _LOCKSTEP: LockStep = None
    # Run-time state, not model state: the captured HIP graphs of the rollout replay, the edges of the last mesh (`_mesh_edges`), of
    # the last union (`_union_mesh_edges`) and the plate's neighbour list (`_mesh_neighbours`).  Class-level defaults, so a model
    # unpickled from a checkpoint that lacks some of them starts with empty caches.
    _RUNTIME_CACHES = ('_fwd_cache', '_cells_key', '_cells_edges', '_batch_edges_key', '_batch_edges', '_nbr_key', '_nbr')
    _fwd_cache = _cells_key = _cells_edges = _batch_edges_key = _batch_edges = _nbr_key = _nbr = None
    # The same kind of state for ragged batches (build_graph_frames): the edges of the last few meshes (`_frame_mesh_edges`) and of the
    # last few unions of different meshes (`_frames_edges`); dropped from copies and pickles like the caches above.
    _RAGGED_CACHES = ('_meshes', '_unions')
    _meshes = _unions = None
    _MESH_CACHE_SIZE, _UNION_CACHE_SIZE = 32, 8         # how many meshes / batch compositions a model keeps the edges of

    def __init__(self, params, node_size: int, edge_size: int, remote_edge_size: int = 7,
                 edge_sets=('mesh_edges',)) -> None:
        super().__init__()
        self._params = params
        self.loss_fn = torch.nn.MSELoss()
        for attr, (width, name) in {'_output_normalizer': (3, 'output_normalizer'),
                                    '_node_normalizer': (node_size, 'node_normalizer'),
                                    '_node_dynamic_normalizer': (1, 'node_dynamic_normalizer'),
                                    '_mesh_edge_normalizer': (edge_size, 'mesh_edge_normalizer'),
                                    '_intra_edge_normalizer': (remote_edge_size, 'intra_edge_normalizer'),
                                    '_inter_edge_normalizer': (remote_edge_size, 'inter_edge_normalizer'),
                                    '_hyper_node_normalizer': (3, 'hyper_node_normalizer')}.items():
            setattr(self, attr, Normalizer(size=width, name=name))
        remote_cfg, balance_cfg = params.get('rmp'), params.get('graph_balancer')
        connector = remote_cfg.get('connector')
        # a stage is on unless its YAML entry says 'none' (flag.py:30-35)
        self._rmp = 'none' not in (remote_cfg.get('clustering'), connector)
        self._balancer = balance_cfg.get('algorithm') != 'none'
        self._multi = self._rmp and connector == 'multigraph'
        self._architecture = self._select_architecture(connector)
        self._rmp_frequency = remote_cfg.get('frequency')
        self._balance_frequency = balance_cfg.get('frequency')
        self.message_passing_steps = params.get('message_passing_steps')
        self.message_passing_aggregator = params.get('aggregation')
        self._visualized = False
        self.replay_rollout = True          # forward() without gradients replays a captured HIP graph per topology (graphs.GraphedForwardCache)
        self._edge_sets = list(edge_sets)
        if self._balancer:
            from . import graph_balancer as _gb
            self._graph_balancer = _gb.get_balancer(params)
            self._edge_sets.append('balance')
        if self._rmp:
            self._remote_graph = _rmp.get_rmp(params)
            self._edge_sets.extend(self._remote_graph.initialize(
                self._intra_edge_normalizer, self._inter_edge_normalizer, self._hyper_node_normalizer))
        self.learned_model = MeshGraphNet(
            output_size=params.get('size'), latent_size=128, num_layers=2,
            message_passing_steps=self.message_passing_steps,
            message_passing_aggregator=self.message_passing_aggregator,
            architecture=self._architecture, edge_sets=self._edge_sets).to(device)

    def __getstate__(self):
        """The reference pickles the whole system model at every checkpoint (MeshSimulator.py:492-493 `pickle.dump(self)`, with
        `_network` inside) and deep-copies it for evaluation.  Captured HIP graphs (the rollout replay cache) and the per-mesh
        edge caches are run-time state, not model state: a copy starts without them and captures again on its own device."""
        state = super().__getstate__()
        state.update(dict.fromkeys(self._RUNTIME_CACHES + self._RAGGED_CACHES))
        return state

    def _select_architecture(self, connector):
        return connector if self._rmp else 'none'                     # flag.py:36, cylinder.py:36

    # ---- topology, once per mesh ------------------------------------------------------------------------------
    def _mesh_edges(self, cells: Tensor, deform: bool = False):
        """util.triangles_to_edges on the device, cached while the same ``cells`` tensor (or equal content) comes in."""
        hit = self._cells_key is not None and (
            self._cells_key is cells or (self._cells_key.shape == cells.shape and self._cells_key.device == cells.device
                                         and torch.equal(self._cells_key, cells)))
        if not hit:
            s, r, _ = features.cells_to_edges(cells.to(device), deform)
            self._cells_key, self._cells_edges = cells, (s.contiguous(), r.contiguous())
        return self._cells_edges

    def _union_mesh_edges(self, senders: Tensor, receivers: Tensor, n_graphs: int, num_nodes: int):
        """Mesh edges of the disjoint union of ``n_graphs`` copies of one mesh: the ids of copy b are shifted by b * num_nodes
        (what batching.batch_graphs does), graph-major.  Built once per (mesh, batch size, node count)."""
        key = self._batch_edges_key                                      # (B, N, the mesh's sender tensor: _mesh_edges caches it)
        if key is None or key[0] != n_graphs or key[1] != num_nodes or key[2] is not senders:
            off = (torch.arange(n_graphs, device=senders.device) * num_nodes).repeat_interleave(senders.shape[0])
            self._batch_edges = ((senders.repeat(n_graphs) + off).contiguous(), (receivers.repeat(n_graphs) + off).contiguous())
            self._batch_edges_key = (n_graphs, num_nodes, senders)
        return self._batch_edges

    def _frame_mesh_edges(self, cells: Tensor, deform: bool = False):
        """`_mesh_edges` for batches that mix meshes: the same key (the ``cells`` tensor itself, else equal content) over the last
        `_MESH_CACHE_SIZE` meshes instead of the last one."""
        if self._meshes is None:
            self._meshes = []
        for key, edges in self._meshes:
            if key is cells:
                return edges
        for key, edges in self._meshes:
            if key.shape == cells.shape and key.device == cells.device and torch.equal(key, cells):
                return edges
        s, r, _ = features.cells_to_edges(cells.to(device), deform)
        edges = (s.contiguous(), r.contiguous())
        self._meshes = self._meshes[-(self._MESH_CACHE_SIZE - 1):] + [(cells, edges)]
        return edges

    def _frames_edges(self, cells, frame_rows: Tuple[int, ...], deform: bool = False):
        """Mesh edges of the disjoint union of frames of DIFFERENT meshes: ``cells[b]`` is the mesh of frame b, whose ids are shifted
        by the rows of the frames before it (what batching.batch_graphs does), graph-major.  Built once per batch composition -- the
        same meshes (`_frame_mesh_edges`) with the same row counts in the same order -- and then handed out as the same tensors, so the
        topology cache and the captured forward of a rollout see one topology."""
        if len(cells) != len(frame_rows):
            raise ValueError(f'{len(cells)} meshes for {len(frame_rows)} frames')
        meshes = [self._frame_mesh_edges(c, deform) for c in cells]
        if self._unions is None:
            self._unions = []
        for rows, held, union in self._unions:
            if rows == frame_rows and all(a[0] is b[0] for a, b in zip(held, meshes)):
                return union
        first, senders, receivers = 0, [], []
        for (s, r), n in zip(meshes, frame_rows):
            senders.append(s + first)
            receivers.append(r + first)
            first += n
        union = (torch.cat(senders).contiguous(), torch.cat(receivers).contiguous())
        self._unions = self._unions[-(self._UNION_CACHE_SIZE - 1):] + [(frame_rows, meshes, union)]
        return union

    @staticmethod
    def _union_rows(inputs: Dict, name: str, n_graphs: int, num_nodes: int) -> Tensor:
        """``inputs[name]`` as the [B*N, .] rows of the union: a [B, N, .] series is flattened, a shared [N, .] entry (one mesh for
        all frames) is repeated."""
        t = inputs[name].to(device)
        if t.dim() == 2:
            t = t.unsqueeze(0).expand(n_graphs, num_nodes, -1)
        return t.reshape(n_graphs * num_nodes, -1).contiguous()

    def _frame_rows(self, inputs: Dict, names, batched: bool, frame_rows=None):
        """What the one body behind build_graph, build_graph_batch and build_graph_frames works on: -> (rows, B, N), the series
        ``names`` and `mesh_pos` on the device.  A single frame: as they are, B is None.  A batch: [B, N, .] flattened to the [B*N, .]
        rows of the union (views: no launch), a shared `mesh_pos` repeated (`_union_rows`: the one copy a batch adds).  A ragged batch
        (``frame_rows`` given; ``inputs`` is what `concat_frames` returns): the rows as they are, B is the tuple ``frame_rows`` and N
        the number of rows of the union."""
        rows = {name: inputs[name].to(device) for name in names}
        if frame_rows is not None:
            rows['mesh_pos'] = inputs['mesh_pos'].to(device)
            total = rows['node_type'].shape[0]
            if sum(frame_rows) != total or any(t.shape[0] != total for t in rows.values()):
                raise ValueError(f'frames of {frame_rows} rows do not add up to the {total} rows given')
            return rows, tuple(frame_rows), total
        if not batched:
            rows['mesh_pos'] = inputs['mesh_pos'].to(device)
            return rows, None, rows['node_type'].shape[0]
        B, N = rows[names[0]].shape[0], rows[names[0]].shape[1]
        rows = {name: t.reshape(B * N, -1) for name, t in rows.items()}
        rows['mesh_pos'] = self._union_rows(inputs, 'mesh_pos', B, N)
        return rows, B, N

    def _frame_edges(self, cells: Tensor, B, N: int, deform: bool = False):
        """-> ((senders, receivers) of the frame, or of the union of B frames when B is not None; those of the one mesh).  A ragged
        batch (B a tuple of row counts, ``cells`` the meshes of its frames): the union of the different meshes, twice -- the union is
        the one mesh there is."""
        if isinstance(B, tuple):
            union = self._frames_edges(cells, B, deform)
            return union, union
        mesh = self._mesh_edges(cells, deform)
        return (mesh if B is None else self._union_mesh_edges(*mesh, B, N)), mesh

    @staticmethod
    def flatten_frames(inputs: Dict) -> Dict:
        """B stacked frames of one mesh -> the rows of their disjoint union: every per-node series [B, N, .] becomes [B*N, .]
        (frame b owns rows [b*N, (b+1)*N), the row order of build_graph_batch); entries shared by all frames (`cells`, a `mesh_pos`
        given once as [N, .]) are handed on as the same objects.  B and N are read from `node_type` [B, N, 1].  training_step,
        validation_step, get_target, update and the loss mask are element-wise over rows, so they take the result together with the
        graph of build_graph_batch / expand_graph_batch unchanged."""
        B, N = inputs['node_type'].shape[0], inputs['node_type'].shape[1]
        return {name: (t.reshape(B * N, -1) if name != 'cells' and torch.is_tensor(t) and t.dim() == 3 and tuple(t.shape[:2]) == (B, N)
                       else t) for name, t in inputs.items()}

    @staticmethod
    def concat_frames(frames) -> Tuple[Dict, Tuple[int, ...]]:
        """B frames of DIFFERENT meshes (a ragged batch) -> (flat, frame_rows): every per-node series [N_b, .] is concatenated to the
        [rows, .] rows of the disjoint union (frame b owns the N_b rows after those of the frames before it, the row order of
        build_graph_frames), `flat['cells']` is the list of the frames' `cells` (the same objects), and ``frame_rows`` = (N_0, ..,
        N_{B-1}) is read from `node_type`.  training_step, validation_step, get_target, update and the loss mask are element-wise over
        rows, so they take ``flat`` together with the graph of build_graph_frames / expand_graph_frames unchanged."""
        frames = list(frames)
        if not frames:
            raise ValueError('concat_frames: no frame')
        flat = {name: torch.cat([frame[name] for frame in frames]) for name in frames[0] if name != 'cells'}
        flat['cells'] = [frame['cells'] for frame in frames]
        return flat, tuple(int(frame['node_type'].shape[0]) for frame in frames)

    def build_graph_frames(self, frames, is_training: bool) -> MultiGraphWithPos:
        """Not in the reference (which builds one graph per frame and concatenates them with MeshSimulator._get_batched): B frames of
        DIFFERENT meshes -- a sequence of the dicts build_graph takes, e.g. frames of different trajectories of cylinder_flow or
        deforming_plate -- become the disjoint union of B graphs through the body build_graph and build_graph_batch run, in the handful
        of launches a single frame takes.  Node ids of frame b are shifted by the rows of the frames before it, as
        batching.batch_graphs does, and every edge set is graph-major: ids and features are those of the per-frame build_graph
        results concatenated.  Mesh edges are computed once per distinct mesh (the last `_MESH_CACHE_SIZE` are kept), the union's index
        tensors once per batch composition, so repeated calls hand the topology cache the same tensors; the plate's `world_edges` come
        from ONE features.radius_edges_ragged query over the neighbour CSR of the union.  A pair (`concat_frames` result, its
        ``frame_rows``) is taken in place of the sequence.  Gradients: the rules of build_graph_batch (`position_gradients` for the
        plate).
        Semantic difference to B separate build_graph calls, the one build_graph_batch documents: each normaliser accumulates ONCE,
        with the statistics of the whole batch."""
        if isinstance(frames, tuple) and len(frames) == 2 and isinstance(frames[0], dict):
            flat, frame_rows = frames
        else:
            flat, frame_rows = self.concat_frames(frames)
        return self._build(flat, is_training, batched=True, frame_rows=tuple(int(n) for n in frame_rows))

    def expand_graph_frames(self, graph: MultiGraphWithPos, frame_rows, step: int, num_steps: int, is_training: bool) -> MultiGraph:
        """``expand_graph_batch`` for the union build_graph_frames returns: without a connector and without a graph balancer the
        union comes back as a MultiGraph.  Out of scope: either stage on a ragged batch (HgnError) -- clusters and balance edges are
        per mesh, and batching.batch_graphs joins graphs of one size only: such frames take the per-frame route, build_graph and
        expand_graph on every frame, one graph per network call."""
        if self._balancer or self._rmp:
            raise _lib.HgnError('expand_graph_frames: remote message passing (connector) and the graph balancer have no form for a batch '
                                'of different meshes; take the per-frame route (build_graph and expand_graph on the frames one by one, '
                                'one graph per network call), or configure the model without these stages')
        return MultiGraph(node_features=graph.node_features, edge_sets=graph.edge_sets)

    @staticmethod
    def _refresh_due(step: int, num_steps: int, frequency) -> bool:
        """A stage configured with `frequency` f recomputes its once-per-period state (balance edges / clusters) at the steps
        that are multiples of ceil(num_steps / f): f = 1 -> only at step 0 of a trajectory."""
        return step % math.ceil(num_steps / frequency) == 0

    def expand_graph(self, graph: MultiGraphWithPos, step: int, num_steps: int, is_training: bool) -> MultiGraph:
        """The optional stages between build_graph and the network, in the reference's order (flag.py:130-141,
        cylinder.py:108-119, plate.py:202-216): graph balancer first (appends the `balance` edge set, renormalises the mesh
        edges), then remote message passing (hyper nodes + remote edge sets).  Clusters, curvature and which member decides a hyper
        node's spread are functions of the positions, so by default a graph that carries position gradients is refused instead of
        losing them.  With
        `position_gradients = True` the connector lets it in: the clustering reads detached values, the cluster means, spreads,
        hyper-node features and remote edge features are differentiated (the means by hgn_member_mean_bwd, the rest by the backward
        kernels of the frame -> graph step) and the labels, the spread winners and the noise sample are constants.  The graph balancer
        refuses in either case."""
        if (self._balancer or (self._rmp and not self.position_gradients)) and _carries_grad(
                graph.target_feature, graph.mesh_features, *graph.node_features, *(e.features for e in graph.edge_sets)):
            raise _lib.HgnError('expand_graph: the graph balancer and remote message passing (connector) stages are not differentiable '
                                'with respect to positions; build the graph from tensors that do not require grad, or under '
                                'torch.no_grad(), or configure the model without these stages.  A connector alone takes such a graph '
                                'with `model.position_gradients = True` (labels and spread winners are then constants)')
        if self._balancer:
            if self._refresh_due(step, num_steps, self._balance_frequency):
                self._graph_balancer.reset_balancer()
            graph = self._graph_balancer.create_graph(graph, self._mesh_edge_normalizer, is_training)
        if self._rmp:
            if self._refresh_due(step, num_steps, self._rmp_frequency):
                self._remote_graph.reset_clusters()
            graph = self._remote_graph.create_graph(graph, is_training)
        return graph

    def expand_graph_batch(self, graph: MultiGraphWithPos, n_graphs: int, step: int, num_steps: int, is_training: bool,
                           refresh: bool = True) -> MultiGraph:
        """Not in the reference (which expands every frame of a batch on its own and concatenates, MeshSimulator.py:159-234):
        ``expand_graph`` for the union of ``n_graphs`` frames that build_graph_batch returns.  Without a connector the union comes
        back as a MultiGraph.  With one, remote message passing runs ONCE over the union: the cluster labels are computed as in
        expand_graph (once per period, `_refresh_due`), from the first frame of the batch (rows [0, N) with its mesh edges; the
        reference also clusters once per trajectory, from the frame that arrives first), every graph gets its own K hyper nodes
        (hyper node k of graph b has union id B*N + b*K + k, the mapping of batching.batch_graphs) and each remote edge set lists
        its edges graph by graph -- ids and order of batch_graphs over the per-frame expand_graph results.
        Semantic difference to B expand_graph calls: each normaliser accumulates ONCE, with the statistics of the whole batch, and
        `hyper_noise` is drawn once per call for all B*K hyper nodes.
        Out of scope: a configured graph balancer (HgnError); meshes that differ within one batch go through build_graph_frames /
        expand_graph_frames, which take no connector.  Like expand_graph, a
        connector refuses a graph that carries position gradients unless `position_gradients` is set.
        ``refresh=False`` leaves the clusters as they are whatever ``step`` says: the rebuild of a checkpointed step
        (`unrolled_training_step(checkpoint=True)`) expands with the clusters its first pass used."""
        if self._balancer:
            raise _lib.HgnError('expand_graph_batch: the graph balancer stage has no batched form; expand the frames one by one with '
                                'expand_graph and batch them with batching.batch_graphs, or configure the model without a balancer')
        if not self._rmp:
            return MultiGraph(node_features=graph.node_features, edge_sets=graph.edge_sets)
        if not self.position_gradients and _carries_grad(
                graph.target_feature, graph.mesh_features, *graph.node_features, *(e.features for e in graph.edge_sets)):
            raise _lib.HgnError('expand_graph_batch: the remote message passing (connector) stage is not differentiable with respect to '
                                'positions; build the graph from tensors that do not require grad, or under torch.no_grad(), or '
                                'configure the model without this stage.  `model.position_gradients = True` lets the graph in (labels and '
                                'spread winners are then constants)')
        if refresh and self._refresh_due(step, num_steps, self._rmp_frequency):
            self._remote_graph.reset_clusters()
        return self._remote_graph.create_graph_batch(graph, int(n_graphs), is_training)

    def forward(self, graph):
        # Rollout / evaluation (no gradients, on the GPU): the network is replayed from a HIP graph captured per topology, from the
        # second time a topology is seen (graphs.GraphedForwardCache: bit-identical to the eager launches, half their time at one
        # graph per step).  `model.replay_rollout = False` keeps every launch eager.
        if (self.replay_rollout and not torch.is_grad_enabled() and graph.node_features[0].is_cuda
                and not torch.cuda.is_current_stream_capturing()):
            if self._fwd_cache is None:
                from . import graphs
                self._fwd_cache = graphs.GraphedForwardCache(self.learned_model)
            return self._fwd_cache(graph)
        return self.learned_model(graph)

    def evaluate(self) -> None:
        """abstract_system_model.py:187-190."""
        for module in (self, self.learned_model):
            module.eval()

    # ---- one training and one validation step for the three models ------------------------------------------------
    def _loss_mask(self, data_frame):
        """The rows whose node type is free (they are integrated, and only they enter the loss): one `eq` per free type."""
        t = data_frame['node_type'].to(device)[:, 0]
        return reduce(torch.logical_or, [torch.eq(t, value) for value in self._LOCKSTEP.free_types])

    # False: the training loss is the torch sequence `_masked_mse` behind `_loss_mask`, launch for launch what it was.  True (opt-in):
    # `training_step` and every step of `unrolled_training_step` take features.frame_losses(...).loss -- two HIP launches forward, one
    # backward, double sums in a fixed order.  A plain class-level value: a model unpickled from an older checkpoint reads False.
    loss_kernel = False

    def _training_loss(self, target_normalized: Tensor, network_output: Tensor, data_frame: Dict) -> Tensor:
        if self.loss_kernel:
            return features.frame_losses(network_output, target_normalized, data_frame['node_type'], self._LOCKSTEP.free_types).loss
        return _masked_mse(target_normalized, network_output, self._loss_mask(data_frame))

    def training_step(self, graph, data_frame):
        """flag.py:146-154, cylinder.py:123-136, plate.py:218-228."""
        network_output = self(graph)
        target_normalized = self.get_target(data_frame)
        return self._training_loss(target_normalized, network_output, data_frame)

    def training_step_batch(self, graph, data_frame, n_graphs) -> Tuple[Tensor, Tensor]:
        """Not in the reference, whose batched training step returns one scalar while it logs a loss per trajectory
        (MeshSimulator.py:151-156): `training_step` for the union graph of ``n_graphs`` frames (build_graph_batch /
        expand_graph_batch) and the flattened frames (`flatten_frames`), always through features.frame_losses.
        -> (loss over all rows, the loss of every frame [B] detached).  ``loss`` is what `training_step` returns with `loss_kernel =
        True`: the same squares summed in double, grouped by frame here and by 256 rows there, and rounded to fp32 once -- equal
        bits unless the two double sums fall on either side of an fp32 rounding boundary.
        ``n_graphs`` may be a sequence of per-frame row counts instead: the union of a ragged batch (build_graph_frames /
        expand_graph_frames) with the frames of `concat_frames` and its ``frame_rows``."""
        network_output = self(graph)
        target_normalized = self.get_target(data_frame)
        rows_per_frame, ragged = self._frame_split('training_step_batch', network_output.shape[0], n_graphs)
        res = features.frame_losses(network_output, target_normalized, data_frame['node_type'], self._LOCKSTEP.free_types,
                                    rows_per_frame, **ragged)
        return res.loss, res.per_frame.detach()

    @staticmethod
    def _frame_split(what: str, rows: int, n_graphs):
        """The third argument of the batched steps as features.frame_losses takes it -> (rows_per_frame, further keywords): an int B
        = frames of rows / B rows each; a sequence = the row count of every frame of a ragged batch (`frame_rows`)."""
        if isinstance(n_graphs, (tuple, list)):
            return None, {'frame_rows': tuple(int(n) for n in n_graphs)}
        if int(n_graphs) < 1 or rows % int(n_graphs):
            raise ValueError(f'{what}: {rows} rows do not split into {n_graphs} frames')
        return rows // int(n_graphs), {}

    @torch.no_grad()
    def validation_step(self, graph: MultiGraph, data_frame: Dict) -> Tuple[Tensor, Tensor]:
        """flag.py:156-167, cylinder.py:138-153, plate.py:230-244: -> (loss, error of the updated state against the target series)."""
        prediction = self(graph)
        target_normalized = self.get_target(data_frame, False)
        mask = self._loss_mask(data_frame)
        loss = _masked_mse(target_normalized, prediction, mask).item()
        updated = self.update(data_frame, prediction)
        new_state = updated if torch.is_tensor(updated) else updated[0]      # the flag's update returns the state alone
        state_error = _masked_mse(data_frame[self._LOCKSTEP.target].to(device), new_state, mask).item()
        return loss, state_error

    @torch.no_grad()
    def validation_step_batch(self, graph: MultiGraph, data_frame: Dict, n_graphs) -> Tuple[Tensor, Tensor]:
        """Not in the reference, which validates one frame per call (MeshSimulator.py:295-297): `validation_step` for the union graph
        of ``n_graphs`` frames (build_graph_batch / expand_graph_batch) and the flattened frames (`flatten_frames`).
        -> (loss [B], state_error [B]): float32 device tensors, entry b = what `validation_step` returns for frame b; no host read.
        The network, `get_target(flat, False)` and ONE features.frame_losses call, which forms the updated state with the constants
        of `_LOCKSTEP` (the bits of `update`) and compares it against the `_LOCKSTEP.target` series on the free rows.
        ``n_graphs`` may be a sequence of per-frame row counts instead (a ragged batch: build_graph_frames, `concat_frames`)."""
        ls = self._LOCKSTEP
        prediction = self(graph)
        target_normalized = self.get_target(data_frame, False)
        rows_per_frame, ragged = self._frame_split('validation_step_batch', prediction.shape[0], n_graphs)
        res = features.frame_losses(prediction, target_normalized, data_frame['node_type'], ls.free_types, rows_per_frame,
                                    state=(self._output_normalizer, data_frame[ls.state], ls.d, ls.ca,
                                           data_frame[ls.prev] if ls.prev else None, ls.cp, data_frame[ls.target]), **ragged)
        return res.per_frame, res.state_per_frame

    @torch.no_grad()
    def one_step_errors(self, trajectory: Dict[str, Tensor], batch=None, num_timesteps=None) -> Tensor:
        """What the reference's one_step_evaluator collects for one trajectory (MeshSimulator.py:292-297): [loss, state_error] of
        every frame -> [T, 2] float32 on the CPU.  ``trajectory``: [T, ...] series (`cells` and `mesh_pos` per frame, as a dataset
        yields them); ``num_timesteps``: only the first that many frames.
        ``batch`` = M > 0 on a model without a connector and without a graph balancer: consecutive chunks of M frames (the last one
        may be shorter) go through build_graph_batch(., False), expand_graph_batch(., M', first, T, False) and
        `validation_step_batch`; the figures stay on the device until ONE copy at the end.  The trajectory must be one mesh (`cells`
        of frame 0 is used for all frames).  Otherwise -- ``batch`` None or 0, or a model with a connector or a balancer, whose
        clusters and balance edges are per frame (the reason `n_step_computation` gives) -- the reference's own loop: build_graph,
        expand_graph(., t, T, False) and `validation_step` frame by frame, two host reads each.
        Semantic difference of the batched route, the one build_graph_batch documents: a normaliser that accumulates on every build
        (the flag's node-dynamic one) accumulates once per chunk, with the statistics of the chunk's frames, not once per frame."""
        frames = trajectory['cells'].shape[0] if num_timesteps is None else int(num_timesteps)
        if batch and int(batch) > 0 and not (self._rmp or self._balancer):
            series = {name: t[:frames].to(device) for name, t in trajectory.items() if name != 'cells'}
            cells = trajectory['cells'][0]
            chunks = []
            for first in range(0, frames, int(batch)):
                chunk = {name: t[first:first + int(batch)] for name, t in series.items()}
                chunk['cells'] = cells
                count = chunk['node_type'].shape[0]
                graph = self.expand_graph_batch(self.build_graph_batch(chunk, False), count, first, frames, False)
                chunks.append(torch.stack(self.validation_step_batch(graph, self.flatten_frames(chunk), count), dim=1))
            return torch.cat(chunks).cpu() if chunks else torch.zeros(0, 2)
        rows = []
        for t in range(frames):
            frame = {name: series[t] for name, series in trajectory.items()}
            graph = self.expand_graph(self.build_graph(frame, False), t, frames, False)
            rows.append(list(self.validation_step(graph, frame)))
        return torch.tensor(rows, dtype=torch.float32).reshape(frames, 2)

    # ---- evaluation helpers shared by the three models ------------------------------------------------------------
    @staticmethod
    def _first_frame(trajectory: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """Frame 0 of every series of a (possibly batch-of-one) trajectory, on the device."""
        return {name: torch.squeeze(series, 0)[0].to(device) for name, series in trajectory.items()}

    @staticmethod
    def _per_step_mse(truth: Tensor, predicted: Tensor) -> Tensor:
        """[T, N, D] x 2 -> [T]: squared error averaged over components, then over nodes (the reference's two nested means)."""
        return ((truth - predicted) ** 2).mean(dim=-1).mean(dim=-1).detach()

    # ---- lock-step evaluation: W windows of one mesh advance as one batch of W frames -------------------------------
    nstep_batch = None      # None: n_step_computation rolls the windows out one by one (the reference's loop); M > 0: M at a time
    # False: PlateModel's build_graph[_batch], a connector in expand_graph[_batch] and unrolled_training_step(through_state=True) for
    # either refuse tensors that require grad.  True (opt-in): they carry the gradient of everything that is smooth in the positions
    # -- means, differences, norms, normalisation -- and treat as constants what is piecewise constant in them: the cluster labels,
    # which pairs are world edges, which member wins a spread maximum (and the noise sample and the normaliser statistics).
    position_gradients = False

    @staticmethod
    def _window_start(windows: Dict[str, Tensor], name: str) -> Tensor:
        """Frame 0 of every window of a [W, T, N, .] series -> [W, N, .] on the device, in memory of its own (the windows may be
        overlapping views of one trajectory)."""
        return windows[name][:, 0].to(device, copy=True).contiguous()    # a copy: the state buffers are written, the trajectory is not

    @staticmethod
    def _shared_mesh(windows: Dict[str, Tensor]) -> Tuple[Tensor, Tensor]:
        """(cells [F, v], mesh_pos [N, .] or [W, N, .]) of a set of windows: `cells` given once, or with leading window / frame
        dimensions (the first one is taken: one mesh for all windows); `mesh_pos` given once, or as a [W, T, N, .] series whose
        frame 0 is used, as `rollout` uses frame 0 of its trajectory."""
        cells, mesh_pos = windows['cells'], windows['mesh_pos']
        while cells.dim() > 2:
            cells = cells[0]
        return cells, (mesh_pos[:, 0] if mesh_pos.dim() == 4 else mesh_pos).to(device)

    def _batch_errors(self, windows: Dict[str, Tensor], name: str, slab: Tensor) -> Tensor:
        """Per-step errors [W, steps] of a recorded [steps, W, N, d] slab against the windows' own frames, in one call."""
        truth = windows[name][:, :slab.shape[0]].to(device).transpose(0, 1)
        return self._per_step_mse(truth, slab).transpose(0, 1)

    @torch.no_grad()
    def rollout_batch(self, windows: Dict[str, Tensor], num_steps: int):
        """Not in the reference: `rollout` for W windows of ONE mesh at once.  The state series, the series that holds the old state
        (flag), the per-step fallback (plate: the scripted `target|world_pos`) and `node_type` are [W, T, N, .] (window w may be a
        view of a longer trajectory); `cells` and a `mesh_pos` shared by all windows are given once.  The W windows advance in lock
        step: every step is one build_graph_batch over the W current states (is_training=False; for the plate one radius query for
        all windows), expand_graph_batch, the network, and ONE features.rollout_advance launch with the constants of `_LOCKSTEP`.
        It integrates the free rows, keeps or scripts the others and writes the new state, the recorded row and the model's extra
        records (`_rollout_records`) straight into their slices of [steps, W, N, .] slabs.  -> `_rollout_result`: per window what
        `rollout` returns for it, stacked as [W, steps, N, .], and the errors [W, steps]."""
        ls = self._LOCKSTEP
        if num_steps is None:
            num_steps = windows[ls.state].shape[1]
        cells, mesh_pos = self._shared_mesh(windows)
        cur = self._window_start(windows, ls.state)
        prev = self._window_start(windows, ls.prev) if ls.prev else None
        node_type = self._window_start(windows, 'node_type').to(torch.int64)
        W, N = cur.shape[0], cur.shape[1]
        rows = lambda t: t.view(W * N, -1)
        scripted = None
        if ls.fallback:                                                 # [steps, W, N, d], transposed once
            scripted = windows[ls.fallback][:, :num_steps].to(device).transpose(0, 1).contiguous()
        slab = torch.empty(num_steps, W, N, ls.d, dtype=torch.float32, device=cur.device)
        records = self._rollout_records(lambda width: torch.empty(num_steps, W, N, width, dtype=torch.float32, device=cur.device))
        nxt, prev_nxt = torch.empty_like(cur), (torch.empty_like(prev) if ls.prev else None)
        frame = {'cells': cells, 'mesh_pos': mesh_pos, 'node_type': node_type}
        for step in range(num_steps):
            frame[ls.state] = cur
            if ls.prev:
                frame[ls.prev] = prev
            if ls.fallback:
                frame[ls.fallback] = scripted[step]
            graph = self.expand_graph_batch(self.build_graph_batch(frame, is_training=False), W, step, ls.expand_steps or num_steps,
                                            is_training=False)
            outputs = {name: rows(record[step]) for name, record in records.items()}
            if ls.prev:
                outputs['prev_out'] = rows(prev_nxt)                    # the old state goes into the swap buffer
            features.rollout_advance(self(graph), self._output_normalizer, rows(cur), ls.d, ls.ca, rows(prev) if ls.prev else None,
                                     ls.cp, rows(node_type), ls.free_types, rows(scripted[step]) if ls.fallback else None, rows(nxt),
                                     rec=rows(slab[step]), rec_before=ls.record_before, inv_from=ls.inv_from or 0, **outputs)
            cur, nxt, prev, prev_nxt = nxt, cur, prev_nxt, prev
        return (self._rollout_result(windows, node_type, slab.transpose(0, 1), **{k: v.transpose(0, 1) for k, v in records.items()}),
                self._batch_errors(windows, ls.errors, slab))

    @torch.no_grad()
    def rollout_frames(self, trajectories, num_steps: int):
        """Not in the reference: `rollout` for R trajectories of DIFFERENT meshes in lock step.  ``trajectories`` is a sequence of the
        dicts `rollout` takes ([T, N_r, .] series, `cells` and `mesh_pos` per frame), all with at least ``num_steps`` frames (None: the
        frames of the first one).  Every step is one union build over the R current states (the body of build_graph_frames on the
        concatenated rows, is_training=False; for the plate one radius query for all trajectories), expand_graph_frames, the network,
        and ONE features.rollout_advance launch over all rows with the constants of `_LOCKSTEP`, which writes the new state, the
        recorded row and the model's extra records straight into their slices of [steps, rows, .] slabs.  The meshes and node types are
        those of every trajectory's frame 0, as in `rollout`, so every step sees one batch composition and the same index tensors.
        -> a list, per trajectory (result, errors [steps]): what `rollout` returns for it (the recorded series are views of the slabs).
        Out of scope: a connector or a graph balancer (expand_graph_frames raises)."""
        ls = self._LOCKSTEP
        series = [{name: torch.squeeze(t, 0) for name, t in trajectory.items()} for trajectory in trajectories]
        if not series:
            return []
        if num_steps is None:
            num_steps = series[0][ls.state].shape[0]
        if any(t[name].shape[0] < num_steps for t in series for name in (ls.state,) + ((ls.fallback,) if ls.fallback else ())):
            raise ValueError(f'rollout_frames: every trajectory needs {num_steps} frames to advance in lock step')
        starts = [self._first_frame(trajectory) for trajectory in trajectories]
        flat, frame_rows = self.concat_frames(starts)                   # fresh memory: the state buffers are written, the trajectories are not
        total = sum(frame_rows)
        cur = flat[ls.state].float().contiguous()
        prev = flat[ls.prev].float().contiguous() if ls.prev else None
        node_type = flat['node_type'].to(torch.int64)
        scripted = None
        if ls.fallback:                                                 # [steps, rows, d], concatenated once
            scripted = torch.cat([t[ls.fallback][:num_steps].to(device) for t in series], dim=1).float().contiguous()
        slab = torch.empty(num_steps, total, ls.d, dtype=torch.float32, device=cur.device)
        records = self._rollout_records(lambda width: torch.empty(num_steps, total, width, dtype=torch.float32, device=cur.device))
        nxt, prev_nxt = torch.empty_like(cur), (torch.empty_like(prev) if ls.prev else None)
        frame = {'cells': flat['cells'], 'mesh_pos': flat['mesh_pos'], 'node_type': node_type}
        for step in range(num_steps):
            frame[ls.state] = cur
            if ls.prev:
                frame[ls.prev] = prev
            if ls.fallback:
                frame[ls.fallback] = scripted[step]
            graph = self.expand_graph_frames(self.build_graph_frames((frame, frame_rows), is_training=False), frame_rows, step,
                                             ls.expand_steps or num_steps, is_training=False)
            outputs = {name: record[step] for name, record in records.items()}
            if ls.prev:
                outputs['prev_out'] = prev_nxt                          # the old state goes into the swap buffer
            features.rollout_advance(self(graph), self._output_normalizer, cur, ls.d, ls.ca, prev, ls.cp, node_type, ls.free_types,
                                     scripted[step] if ls.fallback else None, nxt, rec=slab[step], rec_before=ls.record_before,
                                     inv_from=ls.inv_from or 0, **outputs)
            cur, nxt, prev, prev_nxt = nxt, cur, prev_nxt, prev
        results, first = [], 0
        for trajectory, t, start, n in zip(trajectories, series, starts, frame_rows):
            own = slice(first, first + n)
            result = self._rollout_result(trajectory, start['node_type'], slab[:, own], **{k: v[:, own] for k, v in records.items()})
            results.append((result, self._per_step_mse(t[ls.errors][:num_steps].to(device), slab[:, own])))
            first += n
        return results

    def _rollout_records(self, empty) -> Dict[str, Tensor]:
        """The slabs a model records beside the state, by the rollout_advance output that fills them; ``empty(width)`` makes one."""
        return {}

    @staticmethod
    def window_views(trajectory: Dict[str, Tensor], n_step: int, frames: int) -> Dict[str, Tensor]:
        """All frames - n_step sliding windows of n_step + 1 frames as strided views of the trajectory's series ([T, ...] ->
        [W, n_step + 1, ...], window w = frames w .. w + n_step): what n_step_computation's loop slices one window at a time,
        without a copy per window."""
        horizon, count = n_step + 1, frames - n_step
        views = {}
        for name, series in trajectory.items():
            if series.shape[0] < frames:
                raise ValueError(f'window_views: series {name!r} has {series.shape[0]} frames, {frames} asked for')
            views[name] = series.as_strided((count, horizon) + tuple(series.shape[1:]), (series.stride(0),) + tuple(series.stride()))
        return views

    # ---- seeded training noise: one launch for a batch of frames --------------------------------------------------------
    noise_seed = None       # the seed `add_noise` uses when the call gives none; a plain value (it travels in pickles, old ones read None)

    def add_noise(self, frames: Dict[str, Tensor], draw: int, frame_ids=None, seed=None, frame_rows=None) -> Dict[str, Tensor]:
        """The reference's training noise (src/data/preprocessing.py:84-98, once per frame) for one frame ([N, .] series) or for
        stacked frames ([B, N, .], what build_graph_batch takes) in ONE features.add_noise launch: normal(0, `noise`) on the NORMAL
        rows of ``frames[field]``, and (1 - `gamma`) times the same sample on ``frames['target|' + field]``; `field`, `noise` and
        `gamma` are the keys of the YAML's `model` section (`self._params`).  Only NodeType.NORMAL is perturbed, as in the reference
        -- not `_LOCKSTEP.free_types`: the cylinder's loss mask also holds OUTFLOW, its noise does not.
        The sample of a row depends on (``seed``, ``draw``, the frame's id, the node) alone: ``seed`` defaults to `self.noise_seed`
        (ValueError if both are None), ``draw`` counts the draws (the training step, say) and frame b has id ``frame_ids[b]``,
        default b.  A rank of a data-parallel run that passes the global ids of its frames gets the samples a single process gets.
        ``frame_rows`` (a sequence of row counts): ``frames`` is the ``flat`` of `concat_frames`, a ragged batch whose frame b has
        ``frame_rows[b]`` rows; still one launch, and every frame gets the samples it gets on its own with its id.
        -> a shallow copy of ``frames`` with `field` and `target|field` replaced by fresh tensors in the input's shape; every other
        entry is the same object (the flag's `prev|world_pos` is untouched, as in the reference) and the inputs are not written.  A
        scale of 0, or a `model` section without `noise`, returns the copy without a launch.
        Out of scope: the connector's `hyper_noise` keeps torch.normal; the reference's own src/data/preprocessing.py path through
        the shim is unchanged; noise inside captured graphs.  (parallel.DataParallelTrainer.step_unrolled hands a rank's global
        window ids through `unrolled_training_step` to this method; before a single-step `step` a rank calls it itself, with its
        own frame ids, before it builds its shard.)"""
        out = dict(frames)
        scale = self._params.get('noise')
        if not scale:
            return out
        seed = self.noise_seed if seed is None else seed
        if seed is None:
            raise ValueError('add_noise: no seed (pass `seed`, or set `model.noise_seed`)')
        field = self._params.get('field')
        x, target = frames[field].to(device), frames['target|' + field].to(device)
        rows_per_frame = x.shape[-2] if frame_rows is None else None
        noisy, noisy_target = features.add_noise(
            x.reshape(-1, x.shape[-1]), frames['node_type'].to(device).reshape(-1, 1), (NodeType.NORMAL.value,), float(scale), seed,
            draw, target.reshape(-1, target.shape[-1]), 1.0 - float(self._params.get('gamma')), rows_per_frame, frame_ids, frame_rows)
        out[field], out['target|' + field] = noisy.reshape(x.shape), noisy_target.reshape(target.shape)
        return out

    # ---- training on unrolled rollouts: the W windows advance in lock step, with autograd ---------------------------------
    def _unroll_step(self, frame: Dict, W: int, t: int, n_steps: int, accumulate: bool, advance: bool, eager: bool = False,
                     refresh: bool = True):
        """Step ``t`` of an unroll, the one body of `unrolled_training_step`: its plain loop, the first pass of a checkpointed step
        and that step's rebuild all run it.  ``frame``: the W current states with the per-step series of frame t.  -> (loss, the
        next state [W*N, d] or None without ``advance``, the state's rows [W*N, d]).  ``eager``: the network is called directly, never
        replayed from a captured graph (a first pass runs without gradients, where `forward` would replay); ``refresh``: whether
        expand_graph_batch may compute the clusters anew."""
        ls = self._LOCKSTEP
        graph = self.expand_graph_batch(self.build_graph_batch(frame, accumulate), W, t, n_steps, accumulate, refresh=refresh)
        flat = self.flatten_frames(frame)
        output = self.learned_model(graph) if eager else self(graph)
        loss = self._training_loss(self.get_target(flat, accumulate), output, flat)
        cur = flat[ls.state]
        if not advance:
            return loss, None, cur
        nxt, _ = features.advance_state(output, self._output_normalizer, cur, ls.d, ls.ca, flat[ls.prev] if ls.prev else None,
                                        ls.cp, flat['node_type'], ls.free_types, flat[ls.fallback] if ls.fallback else None)
        return loss, nxt, cur

    def _normalizers(self):
        return [m for m in self.modules() if isinstance(m, Normalizer)]

    @contextlib.contextmanager
    def _rebuilding(self, clusters, rng, statistics):
        """What the rebuild of a checkpointed step runs under, so that it sees what its first pass saw and leaves no second trace:
        every normaliser replays (``statistics`` = per normaliser, in `_normalizers` order, what Normalizer.record collected in the first
        pass: a call that accumulated then -- the flag's node-dynamic normaliser does on every build, the connector's intra-cluster one
        twice in a step -- accumulates nothing now and normalises with the statistics it had then); the clusters of the first pass in
        place (``clusters`` = the remote graph's (`_clusters`, `_neighbors`) then), put back afterwards; the generators -- ``rng`` =
        their (CPU, device) states before the first pass, None where the step draws nothing -- replayed for the connector's
        `hyper_noise` and left as they were found."""
        normalizers = self._normalizers()
        remote = self._remote_graph if self._rmp else None
        held = (remote._clusters, remote._neighbors) if remote is not None else None
        for m, seen in zip(normalizers, statistics):
            m.replay = iter(seen)
        if remote is not None:
            remote._clusters, remote._neighbors = clusters
        try:
            if rng is None:
                yield
            else:
                with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
                    torch.set_rng_state(rng[0])
                    torch.cuda.set_rng_state(rng[1])
                    yield
        finally:
            for m in normalizers:
                m.__dict__.pop('replay', None)
            if remote is not None:
                remote._clusters, remote._neighbors = held

    def unrolled_training_step(self, windows: Dict[str, Tensor], n_steps: int, through_state: bool = True,
                               is_training: bool = True, noise_draw=None, frame_ids=None, checkpoint=None) -> Tuple[Tensor, Tensor]:
        """Not in the reference, which trains on single steps only: the loss of an ``n_steps`` rollout unrolled under autograd, the
        remedy for rollout drift.  ``windows`` has the layout `rollout_batch` takes -- [W, T, N, .] series with T >= n_steps,
        `cells` and a `mesh_pos` shared by all windows given once -- and also holds the per-step series `get_target` reads
        (`target|world_pos`; cylinder: `target|velocity` and `pressure`).  All W windows advance in lock step.  Step t builds the
        frame of the W current states (node types and the initial state from frame 0, the targets from frame t; for the plate, frame
        t's `target|world_pos` is also the scripted motion), forms one union graph with build_graph_batch / expand_graph_batch, runs
        the network, takes the masked MSE against `get_target` of that frame exactly as `training_step` does, and gets the next
        state from ONE features.advance_state launch with the constants `rollout_batch` integrates with.
        Only step 0 sees dataset values, so with ``is_training`` only step 0 accumulates into the normalisers (the flag's
        node-dynamic normaliser accumulates on every build, as in `rollout_batch`).
        ``through_state=True``: the next state keeps its autograd history; gradients flow through advance_state, build_graph_batch
        and the state terms of get_target of all later steps.  ``through_state=False`` (push-forward): the state is detached before
        the next step, so every step's loss differentiates the parameters at that step only; this needs no differentiable graph
        construction and therefore also works for PlateModel and for models with a connector, which refuse ``through_state=True``
        with ``n_steps`` > 1 unless `position_gradients` is set (the gradient then holds the cluster labels, the world-edge
        membership and the spread winners of every step constant).  A configured graph balancer raises what expand_graph_batch raises.
        ``noise_draw`` (None: no noise, the launches of before): frame 0 of the noise field (the state series) and frame 0 of its
        `target|` series of all W windows are perturbed by ONE `add_noise` launch before step 0, with draw ``noise_draw``, the
        model's `noise_seed`, and window w as frame ``frame_ids[w]`` (default w).  The targets of the later steps are untouched: only
        step 0 holds dataset values, the reasoning that keeps the normalisers from accumulating there.
        -> (loss = the mean of the per-step losses, the per-step losses detached [n_steps]).  ``n_steps`` = 1 is `training_step` on
        the batched graph, bit for bit.
        This method returns an ordinary loss for any optimiser; parallel.DataParallelTrainer.step_unrolled takes it through the
        project's own trainer (flat gradient buffer, all-reduce to the mean over all ranks' windows, `max_grad_norm`, fused Adam).
        ``checkpoint`` (None / False: the step above, launch for launch; anything but None or a bool: TypeError): True trades one more
        forward per step but the last for the activations of all of them.  Steps 0 .. n_steps - 2 run without gradients (the
        inference forms of the kernels: no z saves) and keep their input state, the frame-0 series and what replays their draws
        (`_CheckpointedStep`); the last step runs with gradients right away, so ``n_steps`` = 1 is the plain step.  The backward pass
        visits the steps from the last to the first, rebuilds each from its stored state, back-propagates it at once with the
        gradient of its loss and (``through_state``) of the next state, and frees its activations before the step before it is
        rebuilt.  Same losses (equal bits), same normaliser statistics, same generator states and clusters afterwards; gradients arrive
        where the plain step's do, each target's contributions in the same order.  Such a loss is back-propagated once (every step is
        freed as the backward pass leaves it; a second pass raises RuntimeError); without gradients (`torch.no_grad()`) nothing would
        be kept anyway and the call takes the plain route.
        Out of scope: HIP-graph capture of the unrolled step; meshes that differ within a batch."""
        if checkpoint is not None and not isinstance(checkpoint, bool):
            raise TypeError(f'unrolled_training_step: checkpoint must be None, False or True, not {checkpoint!r}')
        ls = self._LOCKSTEP
        n_steps = int(n_steps)
        if n_steps < 1 or any(windows[name].shape[1] < n_steps for name in (ls.state,) + ls.per_step):
            raise ValueError(f'unrolled_training_step: n_steps = {n_steps} needs windows of at least that many frames (and n_steps >= 1)')
        if through_state and n_steps > 1 and not self.position_gradients and (self._rmp or not ls.differentiable):
            raise _lib.HgnError('unrolled_training_step: through_state=True differentiates build_graph_batch and expand_graph_batch with '
                                'respect to the state, which PlateModel and models with a connector cannot do; pass through_state=False '
                                '(push-forward: the state is detached between the steps), or set `model.position_gradients = True`')
        cells, mesh_pos = self._shared_mesh(windows)
        node_type = windows['node_type'][:, 0].to(device).to(torch.int64)
        W, N = node_type.shape[0], node_type.shape[1]
        first = {}                                                      # frame 0 of the series the noise replaces
        if noise_draw is not None:
            names = (self._params.get('field'), 'target|' + self._params.get('field'))
            noisy = self.add_noise(dict({name: windows[name][:, 0] for name in names}, node_type=node_type), noise_draw, frame_ids)
            first = {name: noisy[name] for name in names}
        frame = {'cells': cells, 'mesh_pos': mesh_pos, 'node_type': node_type,
                 ls.state: first.get(ls.state, windows[ls.state][:, 0]).to(device)}
        if ls.prev:
            frame[ls.prev] = windows[ls.prev][:, 0].to(device)
        stored = bool(checkpoint) and n_steps > 1 and torch.is_grad_enabled()       # without gradients nothing is kept anyway: the plain route
        if stored and not self.position_gradients and (self._rmp or not ls.differentiable) and _carries_grad(
                *(frame.get(name) for name in (ls.state, ls.prev, ls.fallback, 'mesh_pos') if name)):
            # (the plain step refuses this in build_graph_batch / expand_graph_batch; a first pass without gradients would not)
            raise _lib.HgnError('unrolled_training_step: PlateModel and models with a connector are not differentiable with respect to '
                                'positions; pass windows that do not require grad, or set `model.position_gradients = True`')
        weights = [p for p in self.learned_model.parameters() if p.requires_grad] if stored else []
        losses = []
        for t in range(n_steps):
            for name in ls.per_step:
                frame[name] = (first[name] if t == 0 and name in first else windows[name][:, t]).to(device)
            accumulate = bool(is_training) and t == 0
            if stored:
                names = [name for name, x in frame.items() if _carries_grad(x)]
                loss, nxt = _CheckpointedStep.apply(self, dict(frame), names, (W, t, n_steps, accumulate, t + 1 == n_steps),
                                                    *(frame[name] for name in names), *weights)
                cur = frame[ls.state]
            else:
                loss, nxt, cur = self._unroll_step(frame, W, t, n_steps, accumulate, advance=t + 1 < n_steps)
            losses.append(loss)
            if t + 1 == n_steps:
                break
            if not through_state:
                nxt, cur = nxt.detach(), cur.detach()
            frame[ls.state] = nxt.reshape(W, N, ls.d)
            if ls.prev:
                frame[ls.prev] = cur.reshape(W, N, ls.d)
        per_step_losses = torch.stack(losses)
        return per_step_losses.mean(), per_step_losses.detach()

    @torch.no_grad()
    def n_step_computation(self, trajectory: Dict[str, Tensor], n_step: int, num_timesteps=None) -> Tuple[Tensor, Tensor]:
        """Sliding n-step rollouts (flag.py:248-260): every window of n_step + 1 consecutive frames is rolled out from its
        first frame; returns (mean over windows of the window's mean error, mean over windows of its final-step error).
        With `self.nstep_batch = M > 0` (not in the reference) the windows advance in lock step, at most M at a time, through
        `rollout_batch`: one union graph of M frames per step instead of M graphs of one frame.  The windows are strided views of
        the trajectory, which must be one mesh throughout.  A model with a connector or a graph balancer ignores `nstep_batch` and
        takes the loop: the reference clusters (and balances) every window anew from that window's own first frame, while
        expand_graph_batch clusters once, from the first frame of the batch."""
        horizon = n_step + 1
        frames = trajectory['cells'].shape[0] if num_timesteps is None else num_timesteps
        batch = self.nstep_batch
        if batch and batch > 0 and frames > n_step and not (self._rmp or self._balancer):
            views = self.window_views({name: series.to(device) for name, series in trajectory.items()}, n_step, frames)
            cells = views.pop('cells')[0, 0]
            chunks = []
            for first in range(0, frames - n_step, int(batch)):
                windows = {name: series[first:first + int(batch)] for name, series in views.items()}
                windows['cells'] = cells
                chunks.append(self.rollout_batch(windows, horizon)[1])
            errors = torch.cat(chunks).cpu()
            window_means, window_finals = [e.mean() for e in errors], [e[-1] for e in errors]
            return torch.stack(window_means).mean(), torch.stack(window_finals).mean()
        window_means, window_finals = [], []
        for start in range(frames - n_step):
            window = {name: series[start:start + horizon] for name, series in trajectory.items()}
            errors = self.rollout(window, horizon)[1].cpu()
            window_means.append(errors.mean())
            window_finals.append(errors[-1])
        return torch.stack(window_means).mean(), torch.stack(window_finals).mean()


class FlagModel(AbstractSystemModel):
    """src/model/flag.py:17-260."""
    _model_type = 'flag'
    _TYPE_MAP = (0,) + (1,) * 9                  # flag.py:72: class = (node_type != NORMAL)
    _LOCKSTEP = LockStep(state='world_pos', prev='prev|world_pos', d=3, ca=2.0, cp=-1.0, free_types=(NodeType.NORMAL.value,),
                         per_step=('target|world_pos',), fallback=None, differentiable=True, expand_steps=399,      # 399: flag.py:236
                         record_before=True, inv_from=None, errors='world_pos', target='target|world_pos')

    def __init__(self, params):
        super().__init__(params, node_size=5, edge_size=7)

    def build_graph(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """flag.py:65-128."""
        return self._build(inputs, is_training, batched=False)

    def build_graph_batch(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """Not in the reference (which builds one graph per frame in Python and concatenates them with
        MeshSimulator._get_batched): B frames of ONE mesh -- `world_pos`, `prev|world_pos`, `node_type` with a leading batch
        dimension [B, N, .], `mesh_pos` [N, 2] or [B, N, 2], `cells` [F, 3] -- become the disjoint union of B graphs in the same
        handful of launches a single frame takes (node ids of frame b are offset by b*N, as batching.batch_graphs does).
        Semantic difference to B separate build_graph calls: each normaliser accumulates ONCE, with the statistics of the
        whole batch (same running sums and counts afterwards, `num_accumulations` grows by 1 instead of B)."""
        return self._build(inputs, is_training, batched=True)

    def _build(self, inputs: Dict, is_training: bool, batched: bool, frame_rows=None) -> MultiGraphWithPos:
        rows, B, N = self._frame_rows(inputs, ('world_pos', 'prev|world_pos', 'node_type'), batched, frame_rows)
        world_pos, mesh_pos = rows['world_pos'], rows['mesh_pos']
        # velocity (3) | one-hot(type != NORMAL) (2)                                              flag.py:68-74
        node_features = features.node_features(world_pos, rows['prev|world_pos'], rows['node_type'], self._TYPE_MAP, 2)
        (senders, receivers), _ = self._frame_edges(inputs['cells'], B, N)
        edge_features, length = features.rel_edge_features(world_pos, mesh_pos, senders, receivers, want_len=True)
        mesh_edges = EdgeSet(name='mesh_edges', features=self._mesh_edge_normalizer(edge_features, is_training),
                             receivers=receivers, senders=senders)
        # max - min incident edge length per node: both aggregates in one pass                      flag.py:100-115
        csr = topology.segment_csr(receivers, world_pos.shape[0], world_pos.device)
        mm = ops.aggregate([_value(length).unsqueeze(1)], [(csr.perm, csr.rowptr, csr.seg)], ('max', 'min'))
        node_dynamic = self._node_dynamic_normalizer(features.lincomb3(mm[:, 0], 1.0, mm[:, 1], -1.0))
        return MultiGraphWithPos(
            node_features=[self._node_normalizer(node_features, is_training)], edge_sets=[mesh_edges],
            target_feature=world_pos, mesh_features=mesh_pos, model_type=self._model_type, node_dynamic=node_dynamic,
            unnormalized_edges=EdgeSet(name='mesh_edges', features=_value(edge_features), receivers=receivers, senders=senders),
            obstacle_nodes=None)

    def update(self, inputs: Dict, per_node_network_output: Tensor) -> Tensor:
        """flag.py:169-180: next position = 2 cur + acceleration - prev."""
        acceleration = self._output_normalizer.inverse(per_node_network_output)
        return features.lincomb3(inputs['world_pos'].to(device), 2.0, acceleration, 1.0, inputs['prev|world_pos'], -1.0)

    def get_target(self, data_frame, is_training=True):
        """flag.py:182-190."""
        cur = data_frame['world_pos'].to(device)
        prev = data_frame['prev|world_pos'].to(device)
        tgt = data_frame['target|world_pos'].to(device)
        return self._output_normalizer(features.lincomb3(tgt, 1.0, cur, -2.0, prev, 1.0), is_training)

    @torch.no_grad()
    def rollout(self, trajectory: Dict[str, Tensor], num_steps: int) -> Tuple[Dict[str, Tensor], Tensor]:
        """flag.py:192-225."""
        if num_steps is None:
            num_steps = trajectory['cells'].shape[0]
        start = self._first_frame(trajectory)
        free = self._loss_mask(start).unsqueeze(1).expand(-1, 3)        # NORMAL nodes move; HANDLE nodes keep their position
        prev_pos, cur_pos, visited = start['prev|world_pos'], start['world_pos'], []
        for step in range(num_steps):
            prev_pos, cur_pos, visited = self._step_fn(start, prev_pos, cur_pos, visited, free, step)
        self._visualized = False
        predictions = torch.stack(visited)
        errors = self._per_step_mse(trajectory['world_pos'][:num_steps].to(device), predictions)
        return {'faces': trajectory['cells'], 'mesh_pos': trajectory['mesh_pos'], 'gt_pos': trajectory['world_pos'],
                'pred_pos': predictions}, errors

    def _rollout_result(self, windows, node_type, pred_pos):
        """rollout_batch: HANDLE nodes keep their position, the state BEFORE the step is recorded and the old state goes into the
        swap buffer; no extra records.  As in `rollout`, the node-dynamic normaliser accumulates on every build (flag.py:115), here
        once per step with the statistics of the W frames.  -> `pred_pos` [W, steps, N, 3]."""
        self._visualized = False
        return {'faces': windows['cells'], 'mesh_pos': windows['mesh_pos'], 'gt_pos': windows['world_pos'], 'pred_pos': pred_pos}

    @torch.no_grad()
    def _step_fn(self, initial_state, prev_pos, cur_pos, trajectory, mask, step):
        """flag.py:227-246."""
        frame = dict(initial_state)
        frame.update({'prev|world_pos': prev_pos, 'world_pos': cur_pos})
        graph = self.expand_graph(self.build_graph(frame, is_training=False), step, 399, is_training=False)   # 399: flag.py:236
        integrated = self.update(frame, self(graph))
        trajectory.append(cur_pos)                              # the trajectory records the state BEFORE the step
        return cur_pos, torch.where(mask, integrated, cur_pos), trajectory


class CylinderModel(AbstractSystemModel):
    """src/model/cylinder.py:17-240 (its remote edges use the 'plate' feature rule, cylinder.py:34)."""
    _model_type = 'plate'
    _TYPE_MAP = (0, -1, -1, -1, 1, 2, 3)        # cylinder.py:71-74: INFLOW->1, OUTFLOW->2, WALL_BOUNDARY->3
    _LOCKSTEP = LockStep(state='velocity', prev=None, d=2, ca=1.0, cp=0.0, free_types=(NodeType.NORMAL.value, NodeType.OUTFLOW.value),
                         per_step=('target|velocity', 'pressure'), fallback=None, differentiable=True, expand_steps=598,  # 598: cylinder.py:218
                         record_before=False, inv_from=2, errors='velocity', target='target|velocity')

    def __init__(self, params):
        super().__init__(params, node_size=6, edge_size=3)

    def build_graph(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """cylinder.py:65-106."""
        return self._build(inputs, is_training, batched=False)

    def build_graph_batch(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """Not in the reference (which builds one graph per frame and concatenates them with MeshSimulator._get_batched): B frames
        of ONE mesh -- `velocity`, `node_type` with a leading batch dimension [B, N, .], `mesh_pos` [N, 2] or [B, N, 2], `cells`
        [F, 3] -- become the disjoint union of B graphs in the handful of launches a single frame takes (node ids of frame b are
        offset by b*N, as batching.batch_graphs does); the fields are those build_graph fills.  Differentiable with respect to
        `velocity` exactly as build_graph is.
        Semantic difference to B separate build_graph calls: each normaliser accumulates ONCE, with the statistics of the whole
        batch (same running sums and counts afterwards, `num_accumulations` grows by 1 instead of B)."""
        return self._build(inputs, is_training, batched=True)

    def _build(self, inputs: Dict, is_training: bool, batched: bool, frame_rows=None) -> MultiGraphWithPos:
        rows, B, N = self._frame_rows(inputs, ('velocity', 'node_type'), batched, frame_rows)
        velocity, mesh_pos = rows['velocity'], rows['mesh_pos']
        node_features = features.node_features(velocity, None, rows['node_type'], self._TYPE_MAP, 4)
        (senders, receivers), _ = self._frame_edges(inputs['cells'], B, N)
        edge_features, _ = features.rel_edge_features(mesh_pos, None, senders, receivers)
        mesh_edges = EdgeSet(name='mesh_edges', features=self._mesh_edge_normalizer(edge_features, is_training),
                             receivers=receivers, senders=senders)
        return MultiGraphWithPos(
            node_features=[self._node_normalizer(node_features, is_training)], edge_sets=[mesh_edges],
            mesh_features=mesh_pos, target_feature=velocity, model_type=self._model_type,
            unnormalized_edges=EdgeSet(name='mesh_edges', features=_value(edge_features), receivers=receivers, senders=senders),
            node_dynamic=[], obstacle_nodes=None)

    def update(self, inputs: Dict, per_node_network_output: Tensor):
        """cylinder.py:155-165."""
        out = self._output_normalizer.inverse(per_node_network_output)
        velocity, pressure = out[:, :2], out[:, 2:]
        return features.lincomb3(inputs['velocity'].to(device), 1.0, velocity, 1.0), pressure

    def get_target(self, data_frame, is_training=True):
        """cylinder.py:167-173."""
        dv = features.lincomb3(data_frame['target|velocity'].to(device), 1.0, data_frame['velocity'], -1.0)
        return self._output_normalizer(torch.cat((dv, data_frame['pressure'].to(device)), dim=1), is_training)

    @torch.no_grad()
    def rollout(self, trajectory: Dict[str, Tensor], num_steps: int):
        """cylinder.py:175-208."""
        num_steps = trajectory['cells'].shape[0]                          # the whole trajectory, whatever was asked (cylinder.py:178)
        start = self._first_frame(trajectory)
        free = self._loss_mask(start).unsqueeze(1).expand(-1, 2)        # NORMAL and OUTFLOW nodes are integrated, the rest is prescribed
        velocity, pressure, velocities, pressures = start['velocity'], start['pressure'], [], []
        for step in range(num_steps):
            velocity, pressure, velocities, pressures = self._step_fn(start, velocity, pressure, velocities, pressures, step, free)
        pred_velocity = torch.stack(velocities)
        errors = self._per_step_mse(trajectory['velocity'][:num_steps].to(device), pred_velocity)
        return {'faces': trajectory['cells'], 'mesh_pos': trajectory['mesh_pos'], 'gt_velocity': trajectory['velocity'],
                'gt_pressure': trajectory['pressure'], 'pred_pressure': torch.stack(pressures), 'pred_velocity': pred_velocity}, errors

    def rollout_batch(self, windows: Dict[str, Tensor], num_steps: int):
        """The lock-step rollout of the base class.  Like `rollout`, it runs the whole window length T whatever `num_steps` says
        (cylinder.py:178); the NORMAL and OUTFLOW nodes are integrated, the state AFTER the step and the predicted pressure are
        recorded.  -> `pred_velocity` [W, T, N, 2], `pred_pressure` [W, T, N, 1], errors [W, T]."""
        return super().rollout_batch(windows, None)

    def rollout_frames(self, trajectories, num_steps: int):
        """The lock-step rollout of the base class for trajectories of different meshes.  Like `rollout`, it runs the whole length of
        the trajectories whatever `num_steps` says (cylinder.py:178): the length of the first one, which the others must reach."""
        return super().rollout_frames(trajectories, None)

    def _rollout_records(self, empty):
        return {'inv_out': empty(1)}                                      # the pressure column of the output

    def _rollout_result(self, windows, node_type, pred_velocity, inv_out):
        return {'faces': windows['cells'], 'mesh_pos': windows['mesh_pos'], 'gt_velocity': windows['velocity'],
                'gt_pressure': windows.get('pressure'), 'pred_pressure': inv_out, 'pred_velocity': pred_velocity}

    @torch.no_grad()
    def _step_fn(self, initial_state, velocity, pressure, trajectory, pressure_trajectory, step, mask):
        """cylinder.py:210-230."""
        frame = dict(initial_state)
        frame.update({'velocity': velocity, 'pressure': pressure})
        graph = self.expand_graph(self.build_graph(frame, is_training=False), step, 598, is_training=False)   # 598: cylinder.py:218
        integrated, new_pressure = self.update(frame, self(graph))
        new_velocity = torch.where(mask, integrated, velocity)
        trajectory.append(new_velocity)                         # here the state AFTER the step is recorded
        pressure_trajectory.append(new_pressure)
        return new_velocity, new_pressure, trajectory, pressure_trajectory


class PlateModel(AbstractSystemModel):
    """src/model/plate.py:17-340 (deforming plate: world edges from obstacle to plate nodes, 4-vertex cells)."""
    _model_type = 'plate'
    _TYPE_MAP = (0, 1, 2, 2)                     # plate.py:78: HANDLE (3) -> class 2
    _RADIUS = 0.03                               # plate.py:85
    _LOCKSTEP = LockStep(state='world_pos', prev=None, d=3, ca=1.0, cp=0.0, free_types=(NodeType.NORMAL.value,),
                         per_step=('target|world_pos',), fallback='target|world_pos', differentiable=False, expand_steps=None,
                         record_before=False, inv_from=0, errors='world_pos', target='target|world_pos')

    def __init__(self, params):
        super().__init__(params, node_size=6, edge_size=8, remote_edge_size=8, edge_sets=('mesh_edges', 'world_edges'))
        self._world_edge_normalizer = Normalizer(size=4, name='world_edge_normalizer')

    def _select_architecture(self, connector):
        return connector if (self._rmp or connector == 'repeated') else 'none'        # plate.py:37-39

    def build_graph(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """plate.py:69-200.  The world edges are a radius query of the positions: tensors that require grad are refused, unless
        `position_gradients` is set -- then the query reads detached values, which pairs are world edges is a constant, and the world
        and mesh edge features and the node features carry the gradient."""
        return self._build(inputs, is_training, batched=False)

    def build_graph_batch(self, inputs: Dict, is_training: bool) -> MultiGraphWithPos:
        """Not in the reference (which builds one graph per frame and concatenates them with MeshSimulator._get_batched): B frames
        of ONE mesh -- `world_pos`, `target|world_pos`, `node_type` with a leading batch dimension [B, N, .], `mesh_pos` [N, 3] or
        [B, N, 3], `cells` [F, 4] -- become the disjoint union of B graphs (node ids of frame b are offset by b*N, as
        batching.batch_graphs does); the fields are those build_graph fills, `obstacle_nodes` is [B*N].  The `world_edges` of all
        frames come from ONE radius query over the union (features.radius_edges_batch with the cached neighbour CSR of the one
        mesh): one host synchronisation for the batch instead of one per frame, and no pair crosses a frame.  Like build_graph,
        it refuses positions that require grad unless `position_gradients` is set.
        Semantic difference to B separate build_graph calls: each normaliser accumulates ONCE, with the statistics of the whole
        batch (same running sums and counts afterwards, `num_accumulations` grows by 1 instead of B)."""
        return self._build(inputs, is_training, batched=True)

    def _build(self, inputs: Dict, is_training: bool, batched: bool, frame_rows=None) -> MultiGraphWithPos:
        if not self.position_gradients and _carries_grad(inputs['world_pos'], inputs['mesh_pos'], inputs['target|world_pos']):
            method = 'build_graph_frames' if frame_rows else 'build_graph_batch' if batched else 'build_graph'
            raise _lib.HgnError(f'PlateModel.{method} is not differentiable with respect to '
                                'positions (its world edges are a radius query of world_pos); pass tensors that do not require grad, '
                                'or call it under torch.no_grad(), or set `model.position_gradients = True` (which pairs are world '
                                'edges is then a constant)')
        rows, B, N = self._frame_rows(inputs, ('world_pos', 'target|world_pos', 'node_type'), batched, frame_rows)
        world_pos, mesh_pos, node_type = rows['world_pos'], rows['mesh_pos'], rows['node_type']
        (senders, receivers), mesh = self._frame_edges(inputs['cells'], B, N, deform=True)
        # world edges: obstacle -> normal pairs closer than the radius that are not mesh edges (excluded through the neighbour CSR of
        # the ONE mesh, on local ids; a ragged batch: of the union, on union ids); a batch takes all its frames in one query
        #                                                                                                plate.py:84-110
        nbr_rowptr = self._mesh_neighbours(*mesh, N, world_pos.device)
        query = (self._RADIUS, NodeType.OBSTACLE.value, NodeType.NORMAL.value, nbr_rowptr, self._nbr)
        if frame_rows is not None:
            world_senders, world_receivers, _ = features.radius_edges_ragged(_value(world_pos), node_type, B, *query)
        elif batched:
            world_senders, world_receivers, _ = features.radius_edges_batch(_value(world_pos), node_type, B, *query)
        else:
            world_senders, world_receivers = features.radius_edges(_value(world_pos), node_type, *query)
        world_edge_features, _ = features.rel_edge_features(world_pos, None, world_senders, world_receivers)
        world_edges = EdgeSet(name='world_edges', features=self._world_edge_normalizer(world_edge_features, is_training),
                              receivers=world_receivers, senders=world_senders)
        mesh_edge_features, _ = features.rel_edge_features(world_pos, mesh_pos, senders, receivers)
        mesh_edges = EdgeSet(name='mesh_edges', features=self._mesh_edge_normalizer(mesh_edge_features, is_training),
                             receivers=receivers, senders=senders)
        # one-hot(3) | velocity of the kinematic (obstacle) nodes, zero elsewhere                      plate.py:186-195
        node_features = features.node_features(rows['target|world_pos'], world_pos, node_type, self._TYPE_MAP, 3, vel_first=False,
                                               vel_mask_type=NodeType.OBSTACLE.value)
        obstacle_nodes = torch.eq(node_type[:, 0], NodeType.OBSTACLE.value)
        return MultiGraphWithPos(
            node_features=[self._node_normalizer(node_features, is_training)], edge_sets=[mesh_edges, world_edges],
            mesh_features=mesh_pos, target_feature=world_pos, model_type=self._model_type,
            unnormalized_edges=EdgeSet(name='mesh_edges', features=_value(mesh_edge_features), receivers=receivers,
                                       senders=senders),
            node_dynamic=None, obstacle_nodes=obstacle_nodes)

    def _mesh_neighbours(self, senders: Tensor, receivers: Tensor, num_nodes: int, dev) -> Tensor:
        """Neighbour CSR of ONE mesh for the radius query: -> rowptr; `self._nbr` = the senders of every node's incoming edges,
        cached while the same mesh edges come in."""
        csr = topology.segment_csr(receivers, num_nodes, dev)                      # neighbours of n = senders of its edges
        if self._nbr_key is not senders:
            self._nbr = senders[csr.perm.long()].to(torch.int32).contiguous()
            self._nbr_key = senders
        return csr.rowptr

    def update(self, inputs: Dict, per_node_network_output: Tensor):
        """plate.py:246-257: next position = current + predicted velocity."""
        velocity = self._output_normalizer.inverse(per_node_network_output)
        cur_position = inputs['world_pos'].to(device)
        return features.lincomb3(cur_position, 1.0, velocity, 1.0), cur_position, velocity

    def get_target(self, data_frame, is_training=True):
        """plate.py:259-264."""
        v = features.lincomb3(data_frame['target|world_pos'].to(device), 1.0, data_frame['world_pos'], -1.0)
        return self._output_normalizer(v, is_training)

    @torch.no_grad()
    def rollout(self, trajectory: Dict[str, Tensor], num_steps: int):
        """plate.py:266-316."""
        if num_steps is None:
            num_steps = trajectory['cells'].shape[0]
        start = self._first_frame(trajectory)
        free = self._loss_mask(start).unsqueeze(1).expand(-1, 3)        # NORMAL nodes are predicted; obstacle / handle nodes are scripted
        scripted = trajectory['target|world_pos'].to(device)
        position, predicted, positions, velocities = start['world_pos'], [], [], []
        for step in range(num_steps):
            position, predicted, positions, velocities = self._step_fn(start, position, predicted, positions, velocities,
                                                                       scripted[step], step, free, num_steps)
        pred_pos = torch.stack(predicted)
        errors = self._per_step_mse(trajectory['world_pos'][:num_steps].to(device), pred_pos)
        # the viewer wants triangles: every 4-vertex cell (v0 v1 v2 v3) contributes (v0 v1 v2) and (v2 v3 v0)   plate.py:289-297
        cells = trajectory['cells']
        triangles = torch.cat((cells[..., 0:3], cells[..., [2, 3, 0]]), dim=-2)
        return {'faces': triangles, 'mesh_pos': trajectory['mesh_pos'],
                'mask': torch.eq(start['node_type'][:, 0], NodeType.OBSTACLE.value), 'gt_pos': trajectory['world_pos'],
                'pred_pos': pred_pos, 'cur_positions': torch.stack(positions), 'cur_velocities': torch.stack(velocities)}, errors

    def _rollout_records(self, empty):
        return {'prev_out': empty(3), 'inv_out': empty(3)}               # the position before the step; the predicted velocity

    def _rollout_result(self, windows, node_type, pred_pos, prev_out, inv_out):
        """rollout_batch: the NORMAL nodes move by the predicted velocity, the scripted ones are put on `target|world_pos[w, t]`.
        -> `pred_pos`, `cur_positions`, `cur_velocities` [W, steps, N, 3], `mask` [W, N]."""
        cells = windows['cells']
        triangles = torch.cat((cells[..., 0:3], cells[..., [2, 3, 0]]), dim=-2)                         # plate.py:289-297
        return {'faces': triangles, 'mesh_pos': windows['mesh_pos'],
                'mask': torch.eq(node_type[..., 0], NodeType.OBSTACLE.value), 'gt_pos': windows['world_pos'],
                'pred_pos': pred_pos, 'cur_positions': prev_out, 'cur_velocities': inv_out}

    @torch.no_grad()
    def _step_fn(self, initial_state, cur_pos, trajectory, cur_positions, cur_velocities, target_world_pos, step, mask,
                 num_steps):
        """plate.py:318-340."""
        frame = dict(initial_state)
        frame.update({'world_pos': cur_pos, 'target|world_pos': target_world_pos})
        graph = self.expand_graph(self.build_graph(frame, is_training=False), step, num_steps, is_training=False)
        integrated, position_before, velocity = self.update(frame, self(graph))
        new_pos = torch.where(mask, integrated, target_world_pos)       # scripted nodes follow the prescribed motion
        trajectory.append(new_pos)
        cur_positions.append(position_before)
        cur_velocities.append(velocity)
        return new_pos, trajectory, cur_positions, cur_velocities


def get_model(config) -> AbstractSystemModel:
    """src/model/get_model.py:13-22."""
    name = str(config['task']['dataset']).lower()
    if 'flag' in name:
        return FlagModel(config.get('model'))
    if 'plate' in name:
        return PlateModel(config.get('model'))
    if 'cylinder' in name:
        return CylinderModel(config.get('model'))
    raise NotImplementedError('Implement your algorithms here!')
