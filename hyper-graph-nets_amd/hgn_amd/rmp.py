"""Remote message passing: cluster the mesh, add hyper nodes and the three remote edge sets
(reference: src/rmp/remote_message_passing.py, hierarchical_connector.py, abstract_connector.py,
abstract_clustering_algorithm.py, k_means_clustering.py, spectral_clustering.py, gaussian_mixture.py,
random_clustering.py, get_rmp.py).

Split the way the hardware wants it:
  * cluster LABELS are a once-per-trajectory host step and stay on scikit-learn, like the reference;
  * everything the reference redoes per frame in Python loops over clusters (cluster means, spreads, hyper-node
    features, up / down / inter edge features, their normalisation) is device work here: the cluster membership
    becomes a CSR over the hyper nodes once, and each frame is a handful of launches of the segment-reduce and
    relative-feature kernels (include/hgn_mp.h, include/hgn_features.h) -- no per-cluster host loop, no host copy
    of positions.
"""
import math
import random
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import features, ops, topology
from .normalizer import Normalizer
from .util import EdgeSet, MultiGraph, MultiGraphWithPos, device


# ------------------------------------------------------------------------------------------------------------
# clustering (host, once per trajectory)
# ------------------------------------------------------------------------------------------------------------
class AbstractClusteringAlgorithm:
    """abstract_clustering_algorithm.py: ``run`` -> list of index tensors, plus ``neigboring_clusters``."""

    def __init__(self, num_clusters=10, sampling=False, alpha=0.5, threshold=0):
        self._num_clusters = num_clusters
        self._sampling = sampling
        self._alpha = alpha
        self._threshold = threshold
        self._labels = None
        self.neigboring_clusters = None

    def _cluster(self, graph: MultiGraphWithPos) -> Sequence[int]:
        raise NotImplementedError

    def run(self, graph: MultiGraphWithPos, number=0, b4=True) -> List[Tensor]:
        """abstract_clustering_algorithm.py:59-84."""
        labels = self._empty_cluster_handling([int(x) for x in self._cluster(graph)])
        self._labels = [-1] * number + labels if b4 else labels + [-1] * number
        self.neigboring_clusters = self.get_neigbors(graph, self._labels)
        if not self._sampling:
            return self._labels_to_indices(labels)
        spotter = self.spotter(graph, labels, self._alpha, self._threshold)
        exemplars = self.exemplars(labels, spotter, self._alpha)
        top_k = self.highest_dynamics(graph, labels, self._alpha)
        return self._combine_samples(spotter, exemplars, top_k)

    # ---- intra-cluster sampling (abstract_clustering_algorithm.py:148-229): which members of a cluster talk to its hyper
    # node.  Host logic on Python lists / sets with the `random` module, like the reference (its list and set orders decide
    # the order of the intra-cluster edges, so the same constructs are used); once per trajectory.
    def _reduce_samples(self, groups: List[List[int]], alpha: float, shuffle: bool) -> List[List[int]]:
        out = []
        for members in groups:
            if shuffle:
                random.shuffle(members)
            keep = min(len(members), max(int(alpha * 100), int(len(members) * alpha)))
            out.append(members[:keep])
        return out

    def spotter(self, graph: MultiGraphWithPos, labels: Sequence[int], alpha: float, threshold: int) -> List[List[int]]:
        """Border nodes: endpoints of mesh edges that cross clusters, kept if they occur at least `threshold` times."""
        es = [x for x in graph.edge_sets if x.name == 'mesh_edges'][0]
        lab = np.asarray(labels)
        snd, rcv = es.senders.cpu().numpy(), es.receivers.cpu().numpy()
        cross = np.nonzero(lab[snd] != lab[rcv])[0]
        groups = [[] for _ in range(self._num_clusters)]
        for e in cross.tolist():                                   # edge order, sender before receiver
            groups[int(lab[snd[e]])].append(int(snd[e]))
            groups[int(lab[rcv[e]])].append(int(rcv[e]))
        groups = [[x for x in set(g) if g.count(x) >= threshold] for g in groups]
        return self._reduce_samples(groups, alpha, True)

    def exemplars(self, labels: Sequence[int], spotter: List[List[int]], alpha: float) -> List[List[int]]:
        """Interior nodes: members of a cluster that were not picked as border nodes."""
        groups = [[] for _ in range(self._num_clusters)]
        for node, c in enumerate(labels):
            if node not in spotter[c]:
                groups[c].append(node)
        return self._reduce_samples(groups, alpha, True)

    def highest_dynamics(self, graph: MultiGraphWithPos, labels: Sequence[int], alpha: float) -> List[List[int]]:
        """Members with the largest node dynamics (max - min incident edge length, flag.py:100-115)."""
        dyn = graph.node_dynamic.detach().cpu()
        groups = [[] for _ in range(self._num_clusters)]
        for node, c in enumerate(labels):
            groups[c].append(node)
        groups = [sorted(g, key=lambda n: dyn[n], reverse=True) for g in groups]
        return self._reduce_samples(groups, alpha, False)

    def _combine_samples(self, spotter, exemplars, top_k) -> List[Tensor]:
        return [torch.tensor(list(set(spotter[i] + exemplars[i] + top_k[i]))) for i in range(self._num_clusters)]

    def _empty_cluster_handling(self, labels: List[int]) -> List[int]:
        """abstract_clustering_algorithm.py:91-102: an empty cluster steals a random node of a non-empty one."""
        result = [[] for _ in range(self._num_clusters)]
        for i, l in enumerate(labels):
            result[l].append(i)
        for i in range(self._num_clusters):
            if len(result[i]) == 0:
                donor = random.choice([x for x in range(self._num_clusters) if len(result[x]) > 0])
                labels[random.choice(result[donor])] = i
        return labels

    @staticmethod
    def _labels_to_indices(labels: Sequence[int]) -> List[Tensor]:
        """abstract_clustering_algorithm.py:104-122 (ascending node ids per cluster, label -1 skipped)."""
        lab = np.asarray(labels)
        return [torch.from_numpy(np.nonzero(lab == k)[0]) for k in range(int(lab.max()) + 1)]

    @staticmethod
    def get_neigbors(graph: MultiGraphWithPos, labels: Sequence[int]) -> List[Tensor]:
        """abstract_clustering_algorithm.py:124-145: unordered pairs of different labels joined by a mesh edge.
        (The reference's list order is Python set order; here: sorted pairs.)"""
        es = [x for x in graph.edge_sets if x.name == 'mesh_edges'][0]
        lab = np.asarray(labels)
        a = lab[es.senders.cpu().numpy()]
        b = lab[es.receivers.cpu().numpy()]
        keep = a != b
        lo, hi = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
        pairs = np.unique(np.stack([lo, hi], 1), axis=0) if lo.size else np.zeros((0, 2), dtype=np.int64)
        return [torch.tensor([int(p[0]), int(p[1])]) for p in pairs]

    def visualize_cluster(self, coordinates):          # logging only in the reference (wandb): no-op here
        return None


class KMeansClustering(AbstractClusteringAlgorithm):
    def _cluster(self, graph):                           # k_means_clustering.py:27-33
        import sklearn.cluster
        from sklearn.preprocessing import StandardScaler
        X = StandardScaler().fit_transform(graph.mesh_features.cpu().numpy()[:, :2])
        return sklearn.cluster.KMeans(n_clusters=self._num_clusters, random_state=0).fit(X).labels_


class GaussianMixtureClustering(AbstractClusteringAlgorithm):
    def _cluster(self, graph):                           # gaussian_mixture.py:24-30
        from sklearn.mixture import GaussianMixture
        from sklearn.preprocessing import StandardScaler
        X = StandardScaler().fit_transform(graph.target_feature.cpu().numpy())
        gm = GaussianMixture(n_components=self._num_clusters, random_state=0, init_params='k-means++').fit(X)
        return gm.predict(X)


class HDBSCANClustering(AbstractClusteringAlgorithm):
    """src/rmp/hdbscan.py:13-105 (`clustering: hdbscan`, get_rmp.py:68-69): density-based clusters of the standardised target
    features; the number of clusters is the algorithm's outcome and nodes it calls noise (label -1) belong to no cluster (they get
    no intra-cluster edges, abstract_clustering_algorithm.py:104-122 skips the label).

    The reference calls the third-party `hdbscan` wheel (requirements.txt, absent from this image and from /root/reference); here
    the same algorithm comes from scikit-learn's port, `sklearn.cluster.HDBSCAN`, with the reference's arguments (max / min cluster
    size, min_samples; `core_dist_n_jobs` / `prediction_data` are wheel-only and affect no label).  Labels are therefore pinned to
    scikit-learn (tests/golden/hdbscan_labels.json), not to the wheel.  Two things the reference leaves undone are done here,
    because without them its own path raises: `neigboring_clusters` is set (the reference's `run` override never assigns it and
    remote_message_passing.py:78 reads it), from the mesh edges between two different non-noise labels.  Intra-cluster sampling
    (`spotter` / `exemplars` through the wheel's condensed tree and soft membership vectors, hdbscan.py:71-101, marked "TODO: Fix
    sampling approach" there) needs internals scikit-learn does not expose: `intra_cluster_sampling.enabled` raises."""

    def __init__(self, sampling, max_cluster_size, min_cluster_size, min_samples, spotter_threshold):
        super().__init__(num_clusters=10, sampling=sampling, alpha=0.5, threshold=spotter_threshold)
        self._max_cluster_size = max_cluster_size
        self._min_cluster_size = min_cluster_size
        self._min_samples = min_samples
        self._spotter_threshold = spotter_threshold

    def _cluster(self, graph):                           # hdbscan.py:53-68
        import sklearn.cluster
        from sklearn.preprocessing import StandardScaler
        X = StandardScaler().fit_transform(graph.target_feature.detach().cpu().numpy())
        fit = sklearn.cluster.HDBSCAN(min_cluster_size=self._min_cluster_size, min_samples=self._min_samples,
                                      max_cluster_size=self._max_cluster_size, copy=True).fit(X)
        return fit.labels_

    def run(self, graph: MultiGraphWithPos, number=0, b4=True) -> List[Tensor]:
        """hdbscan.py:29-51; `number` / `b4`: the obstacle rows removed in front of / behind the clustered nodes
        (remote_message_passing.py:131), as in AbstractClusteringAlgorithm.run."""
        if self._sampling:
            raise NotImplementedError('hdbscan with intra_cluster_sampling: the reference samples through the hdbscan wheel\'s '
                                      'condensed tree and membership vectors (src/rmp/hdbscan.py:71-101), which scikit-learn\'s '
                                      'HDBSCAN does not expose')
        labels = [int(x) for x in self._cluster(graph)]
        self._labels = [-1] * number + labels if b4 else labels + [-1] * number
        clusters = self._labels_to_indices(labels) if labels and max(labels) >= 0 else []
        self._num_clusters = len(clusters)
        keep = [p for p in self.get_neigbors(graph, labels) if int(p[0]) >= 0]        # noise joins nothing
        self.neigboring_clusters = keep
        return clusters


class RandomClustering(AbstractClusteringAlgorithm):
    def _cluster(self, graph):                           # random_clustering.py:38-39
        return [int(x) for x in np.random.rand(graph.target_feature.shape[0]) * self._num_clusters]


class SpectralClustering(AbstractClusteringAlgorithm):
    def _cluster(self, graph):                           # spectral_clustering.py:26-64
        import sklearn.cluster
        X = self._compute_affinity_matrix(graph)
        sc = sklearn.cluster.SpectralClustering(n_clusters=self._num_clusters, random_state=0, affinity='precomputed',
                                                assign_labels='cluster_qr')
        return sc.fit(X).labels_

    @staticmethod
    def _compute_affinity_matrix(graph):
        """spectral_clustering.py:37-64: affinity = 1 / sqrt(|rel world|^2 + |rel mesh|^2) on mesh edges; edges of
        zero length get (largest finite affinity + 1)."""
        n = len(graph.node_features)
        e = graph.unnormalized_edges
        f = e.features.detach().cpu().double().numpy()
        s, r = e.senders.cpu().numpy(), e.receivers.cpu().numpy()
        with np.errstate(divide='ignore'):
            w = 1.0 / np.sqrt(f[:, 3] ** 2 + f[:, -1] ** 2)
        A = np.zeros((n, n), float)
        fin = np.isfinite(w)
        A[s[fin], r[fin]] = w[fin]
        A[s[~fin], r[~fin]] = (w[fin].max() if fin.any() else 0.0) + 1
        return A


# ------------------------------------------------------------------------------------------------------------
# connector (device, per frame)
# ------------------------------------------------------------------------------------------------------------
class _ClusterTopology:
    """Index tensors derived once from (clusters, neighbours, N): membership CSR over the K hyper nodes, the
    up/down edge ids and the inter-cluster edge ids.  Member order = concatenation of the cluster lists, the order in
    which the reference emits the intra-cluster edges (hierarchical_connector.py:85-100)."""

    def __init__(self, clusters: Sequence[Tensor], neighbors: Sequence[Tensor], num_nodes: int, fully_connect: bool,
                 dev):
        K = len(clusters)
        sizes = [int(len(c)) for c in clusters]
        members = torch.cat([torch.as_tensor(c).long() for c in clusters]).to(dev)
        label = torch.repeat_interleave(torch.arange(K), torch.tensor(sizes)).to(dev)
        hyper = label + num_nodes
        self.K, self.N, self.M, self.B = K, num_nodes, int(members.numel()), 1           # B: graphs the topology spans
        self.sizes = torch.tensor(sizes, dtype=torch.float32, device=dev)
        self.members, self.label, self.hyper = members, label, hyper
        csr = topology.CSR(label, K)
        # the kernels read data row perm[j]: compose with the member list so they read node rows directly
        self.node_perm = members[csr.perm.long()].to(torch.int32).contiguous()
        self.csr = csr
        # abstract_connector.py:86-87: senders = [s ; r], receivers = [r ; s]
        self.up_down_s = torch.cat([hyper, members]).contiguous()
        self.up_down_r = torch.cat([members, hyper]).contiguous()
        if fully_connect or K < 4:                       # hierarchical_connector.py:128-129, 207-212
            idx = torch.combinations(torch.arange(num_nodes, num_nodes + K), with_replacement=True)
            idx = idx[idx[:, 0] != idx[:, 1]]
        else:                                            # :132, :201-205
            idx = (torch.stack([torch.as_tensor(n).long() for n in neighbors]) + num_nodes) if len(neighbors) else \
                torch.zeros(0, 2, dtype=torch.int64)
        s, r = idx[:, 0].to(dev), idx[:, 1].to(dev)
        self.inter_s = torch.cat([s, r]).contiguous()
        self.inter_r = torch.cat([r, s]).contiguous()

    @classmethod
    def batched(cls, one: '_ClusterTopology', B: int) -> '_ClusterTopology':
        """The topology of the disjoint union of B graphs that share one clustering (not in the reference, which connects every
        frame on its own and concatenates, MeshSimulator.py:159-234): members of graph b are shifted by b*N, hyper node k of graph
        b has union id B*N + b*K + k (batching.batch_graphs with reference_compat=False), the inter-cluster pairs are replicated
        per graph, and every edge list is graph-major -- the order in which the per-frame sets concatenate.  K, N stay per graph;
        M, sizes, members, label, hyper, the CSR and the edge ids describe the union (B*K segments, B*M members)."""
        self = cls.__new__(cls)
        K, N, M, dev = one.K, one.N, one.M, one.members.device
        g = torch.arange(B, device=dev)
        members = (one.members.repeat(B) + (g * N).repeat_interleave(M)).contiguous()
        label = (one.label.repeat(B) + (g * K).repeat_interleave(M)).contiguous()
        hyper = label + B * N
        self.K, self.N, self.M, self.B = K, N, B * M, B
        self.sizes = one.sizes.repeat(B)
        self.members, self.label, self.hyper = members, label, hyper
        csr = topology.CSR(label, B * K)
        self.node_perm = members[csr.perm.long()].to(torch.int32).contiguous()
        self.csr = csr
        self.up_down_s = torch.cat([hyper, members]).contiguous()
        self.up_down_r = torch.cat([members, hyper]).contiguous()
        # one graph's inter-cluster edges are [s ; r] -> [r ; s] in local hyper ids N + k: shift them to B*N + b*K + k
        shift = (g * K).repeat_interleave(one.inter_s.shape[0]) + (B - 1) * N
        self.inter_s = (one.inter_s.repeat(B) + shift).contiguous()
        self.inter_r = (one.inter_r.repeat(B) + shift).contiguous()
        return self

    _node_side = None

    def node_side(self):
        """What the backward of the cluster mean walks (hgn_member_mean_bwd), built at the first gradient and kept: the member
        list as a CSR over the B*N node rows -- row n's memberships, as positions of the member list in ascending order -- and the
        cluster of every position as int32.  -> (rowptr [rows + 1], items [M], item_seg [M], rows)."""
        if self._node_side is None:
            rows = self.B * self.N
            csr = topology.segment_csr(self.members, rows, self.members.device)
            self._node_side = (csr.rowptr, csr.perm.contiguous(), self.label.to(torch.int32).contiguous(), rows)
        return self._node_side


class _MemberMeanFn(torch.autograd.Function):
    """The cluster means of HierarchicalConnector.run as an autograd node.  Forward: the launch ops.aggregate(('mean',)) makes
    without gradients (hgn_segment_reduce_fwd over the member rows), on detached rows.  Backward: hgn_member_mean_bwd, node-parallel
    over the rows -- ops.AggregateFn.backward runs over as many items as its input has rows, and the member list is shorter than
    that wherever rows belong to no cluster (obstacle rows, HDBSCAN noise, intra-cluster sampling)."""

    @staticmethod
    def forward(ctx, both, t):
        ctx.topo, ctx.like = t, (tuple(both.shape), both.device, both.dtype)
        return ops.aggregate([both.detach()], [(t.node_perm, t.csr.rowptr, t.csr.seg)], ('mean',))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_mean):
        from . import _lib
        t, (shape, dev, dtype) = ctx.topo, ctx.like
        rowptr, items, item_seg, rows = t.node_side()
        if shape[0] != rows:
            raise _lib.HgnError(f'member mean backward: {shape[0]} rows, the cluster topology spans {rows}')
        g = features._f32_rows(d_mean.to(dev))
        D = shape[1]
        d_data = torch.empty(rows, D, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().hgn_member_mean_bwd(
            features._ptr(g), features._ld(g), D, t.csr.rowptr.data_ptr(), t.csr.rowptr.shape[0] - 1, features._ptr(item_seg),
            rowptr.data_ptr(), features._ptr(items), rows, t.M, d_data.data_ptr(), D, _lib.stream_ptr()), 'hgn_member_mean_bwd')
        return d_data.to(dtype), None


class AbstractConnector:
    def __init__(self, fully_connect, noise_scale, hyper_node_features):
        self._intra_normalizer = None
        self._inter_normalizer = None
        self._hyper_normalizer = None
        self._fully_connect = fully_connect
        self._noise_scale = noise_scale
        self._hyper_node_features = hyper_node_features

    def initialize(self, intra: Normalizer, inter: Normalizer, hyper: Normalizer) -> List:
        self._intra_normalizer, self._inter_normalizer, self._hyper_normalizer = intra, inter, hyper
        return list()


class HierarchicalConnector(AbstractConnector):
    """hierarchical_connector.py:16-143 with the per-cluster Python loops replaced by segmented device passes."""

    def __init__(self, fully_connect, noise_scale, hyper_node_features):
        super().__init__(fully_connect, noise_scale, hyper_node_features)
        self._topo_key = None
        self._topo = None

    def initialize(self, intra, inter, hyper):
        super().initialize(intra, inter, hyper)
        return ['intra_cluster_to_mesh', 'intra_cluster_to_cluster', 'inter_cluster']

    def _cluster_topology(self, clusters, neighbors, N, dev, n_graphs: int = 1) -> _ClusterTopology:
        key = (id(clusters), len(clusters), N, id(neighbors), n_graphs)
        if self._topo_key != key:
            self._topo = _ClusterTopology(clusters, neighbors, N, self._fully_connect, dev)
            if n_graphs > 1:
                self._topo = _ClusterTopology.batched(self._topo, n_graphs)
            self._topo_key = key
            self._keep = (clusters, neighbors)           # the ids in the key stay valid while we hold the objects
        return self._topo

    def run(self, graph: MultiGraphWithPos, clusters: List[Tensor], neighbors: List[Tensor], is_training: bool,
            noise: Optional[Tensor] = None, n_graphs: int = 1) -> MultiGraph:
        """``n_graphs`` > 1: ``graph`` is the disjoint union of that many graphs of one mesh (build_graph_batch) and ``clusters`` /
        ``neighbors`` describe ONE of them; the same passes then run once over the union (_ClusterTopology.batched): one
        segment-mean pass, one relative-feature pass per remote set, one max pass for the spreads; noise is [B*K, C]."""
        if graph.model_type not in ('flag', 'plate'):
            raise Exception('Model type is not specified in RippleNodeConnector.')       # abstract_connector.py:97
        nf = graph.node_features.to(device)
        N = nf.shape[0] // n_graphs
        cf = torch.cat((graph.target_feature.to(device), graph.mesh_features.to(device)), dim=1)   # :29
        t = self._cluster_topology(clusters, neighbors, N, cf.device, n_graphs)
        C = cf.shape[1]
        # cluster means of [clustering features | node features]: one segment-mean pass over the member rows
        both = torch.cat((cf, nf), dim=1)
        if features._needs_grad(both):                   # position gradients (AbstractSystemModel.position_gradients): same launch
            means_all = _MemberMeanFn.apply(both, t)
        else:
            means_all = ops.aggregate([both], [(t.node_perm, t.csr.rowptr, t.csr.seg)], ('mean',))     # :39-45
        means, nf_means = means_all[:, :C], means_all[:, C:]
        if noise is None and is_training and self._noise_scale is not None:                         # :48-51
            noise = torch.normal(torch.zeros_like(means), std=self._noise_scale)
        if noise is not None:
            means = means + noise.to(means.device)
        tf = torch.cat((cf, means), dim=0).contiguous()               # rows [mesh ; hyper] (abstract_connector.py:85)
        world, mesh = tf[:, :3], tf[:, 3:]
        # intra-cluster edges, both directions in one pass: first half hyper->mesh, second half mesh->hyper
        f_ud, _ = features.rel_edge_features(world, mesh, t.up_down_s, t.up_down_r)
        if self._hyper_node_features:                                  # :54-71
            spread_world_d = f_ud[:t.M, 3]                             # |mean[:3] - point[:3]| is the down-edge length
            if C == 6:
                spread_mesh_d = f_ud[:t.M, 7]
            else:                                                      # columns [-3:] straddle world and mesh (flag)
                _, spread_mesh_d = features.rel_edge_features(tf[:, C - 3:], None, t.up_down_s[:t.M],
                                                              t.up_down_r[:t.M], want_feat=False, want_len=True)
            d = torch.stack((spread_mesh_d, spread_world_d), dim=1).contiguous()
            spreads = ops.aggregate([d], [(t.csr.perm, t.csr.rowptr, t.csr.seg)], ('max',))
            aug = torch.cat((t.sizes.unsqueeze(1), spreads), dim=1)
            aug = self._hyper_normalizer(aug, is_training)
            nf_means = torch.cat((nf_means, aug), dim=1)
        e_c = self._intra_normalizer(f_ud[t.M:], is_training)          # :104 (to_cluster is normalised first)
        e_m = self._intra_normalizer(f_ud[:t.M], is_training)          # :117
        to_cluster = EdgeSet('intra_cluster_to_cluster', e_c, t.up_down_s[t.M:], t.up_down_r[t.M:])
        to_mesh = EdgeSet('intra_cluster_to_mesh', e_m, t.up_down_s[:t.M], t.up_down_r[:t.M])
        f_i, _ = features.rel_edge_features(world, mesh, t.inter_s, t.inter_r)
        inter = EdgeSet('inter_cluster', self._inter_normalizer(f_i, is_training), t.inter_s, t.inter_r)
        edge_sets = list(graph.edge_sets)
        edge_sets.extend([to_cluster, to_mesh, inter])                 # :140-141
        return MultiGraph(node_features=[nf, nf_means.contiguous()], edge_sets=edge_sets)


class MultigraphConnector(HierarchicalConnector):
    """multigraph_connector.py:11-89: the hierarchical expansion folded into ONE edge set -- node rows get a 2-way and edge
    rows a 4-way one-hot tag (mesh / inter-cluster / to-cluster / to-mesh) and all remote edges are appended to
    'mesh_edges'; 'world_edges' passes through where the model has them.  Pure data movement on top of HierarchicalConnector.run."""

    def initialize(self, intra, inter, hyper):
        AbstractConnector.initialize(self, intra, inter, hyper)
        return []

    def run(self, graph, clusters, neighbors, is_training, noise=None, n_graphs: int = 1) -> MultiGraph:
        g = super().run(graph, clusters, neighbors, is_training, noise, n_graphs)
        nf, hnf = g.node_features

        def tag(x, k, n):
            t = torch.zeros(x.shape[0], n, dtype=x.dtype, device=x.device)
            t[:, k] = 1
            return torch.cat((x, t), dim=1)
        by_name = {e.name: e for e in g.edge_sets}
        order = ('mesh_edges', 'inter_cluster', 'intra_cluster_to_cluster', 'intra_cluster_to_mesh')
        parts = [by_name[n] for n in order]

        def merge(rows):
            """The four parts behind one another; for a union of graphs, graph by graph (every part is graph-major with the same
            number of rows per graph), which is the order in which per-frame merged sets concatenate."""
            if n_graphs == 1:
                return torch.cat(rows, dim=0)
            return torch.cat([x.reshape((n_graphs, x.shape[0] // n_graphs) + tuple(x.shape[1:])) for x in rows], dim=1).flatten(0, 1)
        merged = EdgeSet(name='mesh_edges',
                         features=merge([tag(e.features, k, 4) for k, e in enumerate(parts)]),
                         senders=merge([e.senders.to(device) for e in parts]),
                         receivers=merge([e.receivers.to(device) for e in parts]))
        # 'world_edges' alone passes through (multigraph_connector.py:83: any other set, 'balance' included, is dropped), and only
        # where the model has them: the reference indexes the set unconditionally (:30) and so fails for the flag model
        rest = [e for e in g.edge_sets if e.name == 'world_edges']
        return MultiGraph(node_features=[tag(nf, 0, 2), tag(hnf, 1, 2)], edge_sets=[merged] + rest)


class RemoteMessagePassing:
    """remote_message_passing.py:11-150."""

    def __init__(self, clustering_algorithm: AbstractClusteringAlgorithm, connector: AbstractConnector):
        self._clustering_algorithm = clustering_algorithm
        self._node_connector = connector
        self._clusters = None
        self._neighbors = None

    def initialize(self, intra: Normalizer, inter: Normalizer, hyper: Normalizer) -> List:
        return self._node_connector.initialize(intra, inter, hyper)

    def create_graph(self, graph: MultiGraphWithPos, is_training: bool) -> MultiGraph:
        graph = graph._replace(node_features=graph.node_features[0])          # :67
        if self._clusters is None:
            values = self._values(graph)                                      # labels are no function autograd could follow
            if values.obstacle_nodes is not None:
                self.remove_obstacles(values)
            else:
                self._clusters = self._clustering_algorithm.run(values)
            self._neighbors = self._clustering_algorithm.neigboring_clusters
        return self._node_connector.run(graph, self._clusters, self._neighbors, is_training)

    def create_graph_batch(self, graph: MultiGraphWithPos, n_graphs: int, is_training: bool) -> MultiGraph:
        """create_graph for the disjoint union of ``n_graphs`` frames of one mesh (build_graph_batch): the clusters come, once,
        from the first frame of the batch (through remove_obstacles where there are obstacle nodes); the connector then runs once
        over the union."""
        graph = graph._replace(node_features=graph.node_features[0])
        if self._clusters is None:
            first = self._first_frame_graph(self._values(graph), n_graphs)
            if first.obstacle_nodes is not None:
                self.remove_obstacles(first)
            else:
                self._clusters = self._clustering_algorithm.run(first)
            self._neighbors = self._clustering_algorithm.neigboring_clusters
        return self._node_connector.run(graph, self._clusters, self._neighbors, is_training, n_graphs=n_graphs)

    @staticmethod
    def _values(graph: MultiGraphWithPos) -> MultiGraphWithPos:
        """The graph as the clustering sees it: every tensor that requires grad replaced by its detached value (the clustering
        algorithms, remove_obstacles and the sampling helpers hand tensors to numpy); the graph itself where none does."""
        def val(t):
            return t.detach() if torch.is_tensor(t) and t.requires_grad else t

        def edges(es):
            return es if es is None else EdgeSet(es.name, val(es.features), es.senders, es.receivers)
        sets = [e for e in (*graph.edge_sets, graph.unnormalized_edges) if e is not None]
        tensors = [graph.node_features, graph.target_feature, graph.mesh_features, graph.node_dynamic] + [e.features for e in sets]
        if not any(torch.is_tensor(t) and t.requires_grad for t in tensors):
            return graph
        return graph._replace(node_features=val(graph.node_features), target_feature=val(graph.target_feature),
                              mesh_features=val(graph.mesh_features), node_dynamic=val(graph.node_dynamic),
                              unnormalized_edges=edges(graph.unnormalized_edges), edge_sets=[edges(e) for e in graph.edge_sets])

    @staticmethod
    def _first_frame_graph(graph: MultiGraphWithPos, n_graphs: int) -> MultiGraphWithPos:
        """Graph 0 of a union of ``n_graphs`` graphs of one mesh: rows [0, N) and the first E / B mesh edges (graph-major lists:
        those of graph 0, in local ids)."""
        N = graph.node_features.shape[0] // n_graphs

        def head(es):
            if es is None:
                return None
            E = es.senders.shape[0] // n_graphs
            return EdgeSet(es.name, es.features[:E], es.senders[:E], es.receivers[:E])
        rows = lambda t: t[:N] if torch.is_tensor(t) else t
        return graph._replace(node_features=graph.node_features[:N], target_feature=graph.target_feature[:N],
                              mesh_features=graph.mesh_features[:N], node_dynamic=rows(graph.node_dynamic),
                              obstacle_nodes=rows(graph.obstacle_nodes), unnormalized_edges=head(graph.unnormalized_edges),
                              edge_sets=[head(e) for e in graph.edge_sets if e.name == 'mesh_edges'])

    def remove_obstacles(self, graph: MultiGraphWithPos) -> None:
        """remote_message_passing.py:82-137: cluster only the non-obstacle nodes (the obstacle block is contiguous, at
        the start or at the end of the node list); cluster members keep their ids in the full graph.  Host-side index
        work, once per trajectory."""
        idx = graph.obstacle_nodes.nonzero().squeeze(1).cpu()
        fst, lst = int(idx[0]), int(idx[-1])
        e = graph.unnormalized_edges
        s, r, f = e.senders.cpu(), e.receivers.cpu(), e.features.cpu()
        if fst == 0:                                                   # keep [lst + 1, end)
            keep = slice(lst + 1, None)
            m = (s > lst) & (r > lst)
            new_edges = EdgeSet('mesh_edges', f[m], s[m] - lst - 1, r[m] - lst - 1)
            offset, b4 = lst + 1, True
        else:                                                          # keep [0, fst)
            keep = slice(0, fst)
            m = (s < fst) & (r < fst)
            new_edges = EdgeSet('mesh_edges', f[m], s[m], r[m])
            offset, b4 = lst - fst + 1, False
        new_graph = graph._replace(node_features=graph.node_features[keep], target_feature=graph.target_feature[keep],
                                   mesh_features=graph.mesh_features[keep], unnormalized_edges=new_edges)
        self._clusters = self._clustering_algorithm.run(new_graph, offset, b4)
        if fst == 0:
            self._clusters = [c + (lst + 1) for c in self._clusters]

    def reset_clusters(self):
        self._clusters = None

    def visualize_cluster(self, graph):
        self._clustering_algorithm.visualize_cluster(graph)


def get_rmp(config) -> RemoteMessagePassing:
    """get_rmp.py:19-26."""
    rmp = config['rmp']
    clustering = get_clustering_algorithm(str(rmp['clustering']).lower(), config)
    connector = get_connector(str(rmp['connector']).lower(), config)
    return RemoteMessagePassing(clustering, connector)


def get_clustering_algorithm(name: str, config) -> Optional[AbstractClusteringAlgorithm]:
    """get_rmp.py:29-81."""
    rmp = config['rmp']
    samp = rmp.get('intra_cluster_sampling', {})
    args = (rmp['num_clusters'], samp.get('enabled', False), samp.get('alpha', 0.5), samp.get('spotter_threshold', 0))
    table = {'random': RandomClustering, 'spectral': SpectralClustering, 'gmm': GaussianMixtureClustering,
             'kmeans': KMeansClustering, 'k-means': KMeansClustering}
    if name == 'none':
        return None
    if name == 'hdbscan':                                # get_rmp.py:47-69: its own block of the configuration
        h = rmp['hdbscan']
        return HDBSCANClustering(samp.get('enabled', False), h['max_cluster_size'], h['min_cluster_size'], h['min_samples'],
                                 h['spotter_threshold'])
    if name in table:
        return table[name](*args)
    raise NotImplementedError('Implement your clustering algorithms here!')


def get_connector(name: str, config) -> Optional[AbstractConnector]:
    """get_rmp.py:84-96."""
    rmp = config['rmp']
    noise = None if rmp['hyper_noise'] == 'none' else rmp['hyper_noise']
    if name in ('hyper', 'hetero', 'multiscale'):
        return HierarchicalConnector(rmp['fully_connect'], noise, rmp['hyper_node_features'])
    if name == 'multi':
        return MultigraphConnector(rmp['fully_connect'], noise, rmp['hyper_node_features'])
    if name in ('none', 'repeated'):
        return None
    raise NotImplementedError('Implement your connectors here!')
