/* hgn_features.h -- C ABI of the frame -> graph-feature step that feeds the message-passing path
 * ("next" rows f2 feature construction and f3 remote-graph assembly).
 * Same library (libhgn_mp.so), same conventions as hgn_mp.h: int status (0 ok, <0 HGN_E_*), hgn_last_error(),
 * caller-owned device buffers incl. workspace, everything enqueued on the hipStream_t passed in, no allocation.
 * Byte / index work: outputs are bit-exact for the integer parts and fp32 for the features.
 *
 * Replaces, on the reference side (file:line under /root/reference/src):
 *   util.py:50-89                    triangles_to_edges                      -> hgn_cells_to_edges
 *   model/flag.py:67-93, plate.py:165-183, cylinder.py:81-87,
 *   rmp/abstract_connector.py:84-98  relative position features of an edge set -> hgn_rel_edge_features
 *   model/flag.py:68-74, cylinder.py:67-76, plate.py:75-79,186-195
 *                                    velocity + one-hot node features          -> hgn_node_features
 *   model/plate.py:84-110            world edges (cdist + masks + nonzero)      -> hgn_radius_edges_count/_fill
 *   model/plate.py:84-110 per frame + algorithms/MeshSimulator.py:159-234 (_get_batched)
 *                                    world edges of a batch of frames, one query -> hgn_radius_edges_batch_count/_fill
 *   graph_balancer/ricci.py:128-301  balanced Forman curvature kernels (SDRF)   -> hgn_forman_curvature/_post_delta
 *   model/flag.py:178,188, cylinder.py:163,171  target / integrator arithmetic   -> hgn_lincomb3
 *   model/flag.py:169-180,243, cylinder.py:155-165, plate.py:246-257,328
 *                                    one rollout step's state update            -> hgn_rollout_advance
 *                                    and its derivative (unrolled training)     -> hgn_rollout_advance_bwd
 *   rmp/hierarchical_connector.py:39-45  derivative of the cluster means         -> hgn_member_mean_bwd
 *   migration/normalizer.py:40-71    Normalizer.forward / inverse / _accumulate -> hgn_col_stats,
 *                                                                              hgn_normalizer_update, hgn_normalize
 *   data/preprocessing.py:84-98      Preprocessing._add_noise, per frame         -> hgn_training_noise (a batch of frames)
 *   model/flag.py:146-167, cylinder.py:123-153, plate.py:218-244
 *                                    the masked MSE of training / validation_step -> hgn_frame_losses (per frame of a batch), _bwd
 *   the three batch entries above for frames of different meshes (a ragged batch) -> hgn_radius_edges_ragged_count/_fill,
 *                                    hgn_training_noise_ragged, hgn_frame_losses_ragged, _ragged_bwd
 */
#ifndef HGN_FEATURES_H
#define HGN_FEATURES_H
#include <stddef.h>
#include <stdint.h>
#include "hgn_mp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HGN_MAX_FEATURE_WIDTH 32 /* widest row hgn_col_stats / hgn_normalize accept (reference: <= 12) */

/* ---- util.py:50-89 ---------------------------------------------------------------------------------------
 * cells [n_cells, verts] int64 row-major, verts = 3 (triangles) or 4 (`deform=True`: edges 0-1, 1-2, 2-3, 3-0).
 * Unique undirected edges as (max, min) pairs in lexicographic order (what torch.unique(dim=0) returns), then
 * both directions: senders = [max.. ; min..], receivers = [min.. ; max..].
 * senders / receivers: device int64 with capacity 2*verts*n_cells each; *n_unique (HOST) receives the number of
 * undirected edges (valid prefix = 2 * n_unique).  Synchronises the stream (topology step, once per mesh).
 * HGN_E_RANGE if a vertex id is outside [0, 2^31). */
int hgn_cells_to_edges_workspace_bytes(int64_t n_cells, int verts, size_t* bytes);
int hgn_cells_to_edges(const int64_t* cells, int64_t n_cells, int verts, int64_t* senders, int64_t* receivers,
                       int64_t* n_unique /*host*/, void* workspace, size_t ws_bytes, void* stream);

/* ---- relative-position features of an edge set -----------------------------------------------------------
 * row e of feat = [ a[s]-a[r] (da) , |a[s]-a[r]| , b[s]-b[r] (db) , |b[s]-b[r]| ]   (s = senders[e], r = receivers[e])
 * a [n_rows, lda], b [n_rows, ldb] fp32; 1 <= da <= 3; db in 0..3 (db = 0: b unused, row = da+1 floats).
 * feat (nullable) [E, ldf] with ldf >= row width; len_a (nullable) [E] receives |a[s]-a[r]| (flag.py:101-113).
 * Precondition: ids in [0, n_rows) (checked by hgn_csr_build on the same id arrays); out-of-range ids are
 * skipped (row left untouched), never dereferenced. */
int hgn_rel_edge_features(const float* a, int64_t lda, int da, const float* b, int64_t ldb, int db, int64_t n_rows,
                          const int64_t* senders, const int64_t* receivers, int64_t E, float* feat, int64_t ldf,
                          float* len_a, void* stream);

/* ---- node features ------------------------------------------------------------------------------------------
 * out row n = [ v (d floats) | one_hot(cls, n_classes) ]  (vel_first = 1)  or  [ one_hot | v ]  (vel_first = 0)
 *   v   = cur[n] - prev[n]  (prev NULL: cur[n]; cur NULL: zeros);  if vel_mask_type >= 0, v is kept only on rows
 *         whose node_type equals vel_mask_type (plate.py:186-194: obstacle rows), else 0
 *   cls = map[node_type[n]] when map != NULL (device int32 table of map_len entries; flag: type!=0 -> 1;
 *         cylinder.py:71-74; plate.py:78), else node_type[n]; a class outside [0, n_classes) leaves the one-hot 0.
 * node_type int64 with element stride ldt (the reference passes node_type[:, 0]). */
int hgn_node_features(const float* cur, const float* prev, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                      const int32_t* map, int map_len, int n_classes, int vel_first, int vel_mask_type, int64_t N,
                      float* out, int64_t ldo, void* stream);

/* ---- normalizer.py ------------------------------------------------------------------------------------------
 * hgn_col_stats: batch[0:F] = column sums, batch[F:2F] = column sums of squares of x [rows, F] (contiguous),
 *   accumulated in fp64, fixed order (deterministic), rounded once to fp32 (normalizer.py:57-58).
 * hgn_normalizer_update: the running statistics += batch statistics iff *num_acc < max_acc (normalizer.py:42,
 *   59-62; the gate is evaluated on the device: no host sync); count = rows of the (global) batch.
 * hgn_normalize: out = (x - mean) / max(std, eps)            (inverse = 0, normalizer.py:45,64-71)
 *                out = x * max(std, eps) + mean              (inverse = 1, normalizer.py:47-49)
 *   mean = acc_sum / max(acc_count, 1), std = sqrt(|acc_sumsq / max(acc_count,1) - mean^2|). */
int hgn_col_stats_workspace_bytes(int64_t rows, int F, size_t* bytes);
int hgn_col_stats(const float* x, int64_t rows, int F, float* batch /*[2F]*/, void* workspace, size_t ws_bytes,
                  void* stream);
int hgn_normalizer_update(float* acc_sum, float* acc_sumsq, float* acc_count, float* num_acc, const float* batch,
                          const float* count /*device [1]*/, int F, float max_acc, void* stream);
int hgn_normalize(const float* x, int64_t rows, int F, const float* acc_sum, const float* acc_sumsq,
                  const float* acc_count, float eps, int inverse, float* out, void* stream);

/* ---- backward of the three feature kernels above (position gradients of a frame -> graph step) ---------------
 * The statistics of the normaliser are constants of the graph: nothing flows into acc_sum / acc_sumsq / acc_count.
 *
 * hgn_rel_edge_features_bwd: d_feat [E, ldf] (nullable), d_len [E] (nullable) -> d_a [n_rows, da], d_b [n_rows, db]
 *   (contiguous, each nullable).  With u = a[s]-a[r]: g = d_feat[0:da] + (d_feat[da] + d_len) * u/|u| is added to row s and
 *   subtracted from row r (likewise for b, without d_len); an edge of zero length contributes nothing through the norm term.
 *   Parallel over the n_rows nodes: (rowptr_s, perm_s) = CSR of the edges by sender, (rowptr_r, perm_r) by receiver, both as
 *   hgn_csr_build makes them over the SAME id arrays (perm = position in the caller's edge order).  A node walks its outgoing,
 *   then its incoming edges in CSR order and writes its row once: no float atomics, equal bits on every run, zeros for a node
 *   without edges.  A node with more than 32 edges is summed by one wavefront, the others by one thread each; max_degree = an
 *   upper bound of the edges (out + in) of any node, or < 0 when unknown (<= 32: the wavefront pass is not launched).
 *   Ids outside [0, n_rows) / [0, E) are skipped, never dereferenced.  E = 0 or both gradients NULL: zero rows.
 * hgn_node_features_bwd: d_out [N, ldo] -> d_cur, d_prev [N, d] (contiguous, each nullable): the velocity columns pass +d to
 *   cur and -d to prev, zero on the rows the forward masked (vel_mask_type >= 0); the one-hot columns carry nothing.
 * hgn_normalize_bwd: d_x = d_out / max(std, eps) (inverse = 0) or d_out * max(std, eps) (inverse = 1), std formed exactly as
 *   in hgn_normalize. */
int hgn_rel_edge_features_bwd(const float* d_feat, int64_t ldf, const float* d_len, const float* a, int64_t lda, int da,
                              const float* b, int64_t ldb, int db, int64_t n_rows, const int64_t* senders,
                              const int64_t* receivers, int64_t E, const int32_t* rowptr_s, const int32_t* perm_s,
                              const int32_t* rowptr_r, const int32_t* perm_r, int64_t max_degree, float* d_a, float* d_b,
                              void* stream);
int hgn_node_features_bwd(const float* d_out, int64_t ldo, int d, int n_classes, int vel_first, const int64_t* node_type,
                          int64_t ldt, int vel_mask_type, int64_t N, float* d_cur, float* d_prev, void* stream);
int hgn_normalize_bwd(const float* d_out, int64_t rows, int F, const float* acc_sum, const float* acc_sumsq,
                      const float* acc_count, float eps, int inverse, float* d_x, void* stream);

/* ---- world edges by radius (plate.py:84-110) ---------------------------------------------------------------
 * Directed pairs (s, r), s != r, with |pos[s] - pos[r]| < radius, node_type[s] == sender_type, node_type[r] ==
 * receiver_type (a negative type = any), and (s, r) not adjacent in the mesh given as a CSR (nbr_rowptr [N+1],
 * nbr [nnz]: neighbours of node n = nbr[nbr_rowptr[n] .. nbr_rowptr[n+1]); nullable = no exclusion).  Output order =
 * torch.nonzero of the reference's N x N mask: ascending s, then ascending r.  Distances are evaluated as
 * sqrt(sum (pos[s]-pos[r])^2) in fp32 (the reference's cdist switches to the |a|^2+|b|^2-2ab form for N > 25, which
 * differs only for pairs within fp32 noise of the radius).
 * Two calls (the result size is data dependent): _count fills offsets[N+1] (device int32, exclusive prefix of the per-
 * sender counts, offsets[N] = total) and returns the total on the HOST (synchronises the stream); _fill writes
 * senders / receivers [total] int64.  One wavefront per sender row; no N x N matrix is formed. */
int hgn_radius_edges_workspace_bytes(int64_t N, size_t* bytes);
int hgn_radius_edges_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t N,
                           float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                           const int32_t* nbr, int32_t* offsets /*[N+1]*/, int64_t* total /*host*/, void* workspace,
                           size_t ws_bytes, void* stream);
int hgn_radius_edges_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t N,
                          float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                          const int32_t* nbr, const int32_t* offsets, int64_t* senders, int64_t* receivers,
                          void* stream);

/* ---- world edges of a whole batch of frames (plate.py:84-110 once per frame, MeshSimulator.py:159-234 for the union) ----
 * The reference builds the world edges of every frame of a batch on its own and then concatenates the graphs with ids
 * shifted by i * num_nodes (_get_batched).  Here the radius query runs once over the disjoint union of n_graphs graphs of
 * nodes_per_graph (N) nodes each: pos / node_type hold the B*N rows of the union, graph b owns rows [b*N, (b+1)*N).
 * A pair (s, r) is reported only if both ends lie in the same graph.  nbr_rowptr [N+1] / nbr is the CSR of ONE mesh in
 * local ids (nullable), shared by all graphs (frames of one trajectory share `cells`); the exclusion is tested on
 * (s - b*N, r - b*N), no union CSR is built.  Types, radius and the distance expression (sqrtf of the fp32 sum of squares,
 * < radius) are those of hgn_radius_edges_count.  Output: union ids in ascending (s, r) order = the concatenation over b of
 * what hgn_radius_edges_count/_fill return for graph b, shifted by b*N.
 * _count fills offsets [B*N+1] (device int32, exclusive prefix of the per-sender counts, offsets[B*N] = total) and, when
 * graph_offsets is not NULL, graph_offsets [B+1] (device int32: graph_offsets[b] = offsets[b*N] = edges before graph b,
 * graph_offsets[B] = total), and returns the total on the HOST: ONE stream synchronisation for the batch instead of B.
 * _fill writes senders / receivers [total] int64.  One wavefront per sender row sweeps the N receivers of its own graph in
 * chunks of 64: B*N*N/64 chunk iterations, not (B*N)^2/64; sender rows of another type leave at once.
 * HGN_E_INVALID: n_graphs < 1, nodes_per_graph < 0, n_graphs * nodes_per_graph > 0x7ffffffe, whatever hgn_radius_edges_count
 * refuses (d outside 1..3, ld < d, ldt < 1, radius not >= 0, null pos / node_type with rows, only one of nbr_rowptr / nbr),
 * null outputs, workspace too small. */
int hgn_radius_edges_batch_workspace_bytes(int64_t n_graphs, int64_t nodes_per_graph, size_t* bytes);
int hgn_radius_edges_batch_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                 int64_t n_graphs, int64_t nodes_per_graph, float radius, int sender_type,
                                 int receiver_type, const int32_t* nbr_rowptr, const int32_t* nbr,
                                 int32_t* offsets /*[B*N+1]*/, int32_t* graph_offsets /*[B+1], nullable*/,
                                 int64_t* total /*host*/, void* workspace, size_t ws_bytes, void* stream);
int hgn_radius_edges_batch_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                int64_t n_graphs, int64_t nodes_per_graph, float radius, int sender_type,
                                int receiver_type, const int32_t* nbr_rowptr, const int32_t* nbr, const int32_t* offsets,
                                int64_t* senders, int64_t* receivers, void* stream);

/* ---- balanced Forman curvature (graph_balancer/ricci.py:128-301, the two numba-CUDA kernels of SDRF) -------------
 * Dense fp32 adjacency A [N,N] (row-major, entries 0/1), A2 = A*A [N,N], d_in[i] = column sums, d_out[j] = row sums.
 * hgn_forman_curvature: C[i,j] for the nnz listed pairs (ei[e], ej[e]) with A != 0; C must be zero-filled by the caller
 *   (the reference's dense kernel writes 0 for non-edges).  One wavefront per edge sweeps k = 0..N-1 (count and maximum
 *   of the positive four-cycle terms by wave reduction), then evaluates the closed form in fp64 and rounds to fp32 once per
 *   store -- the typing of the reference's numba kernel (int literal x float32 -> float64), so equal inputs give equal bits
 *   and the argmin/argmax ties of SDRF resolve identically.
 * hgn_forman_post_delta: D[I,J] = curvature of edge (x,y) after inserting (i_nb[I], j_nb[J]); -1000 where i == j or the
 *   pair is already an edge (ricci.py:206-208); d_in_x = sum A[:,x], d_out_y = sum A[y,:]. */
int hgn_forman_curvature(const float* A, const float* A2, const float* d_in, const float* d_out, int64_t N,
                         const int32_t* ei, const int32_t* ej, int64_t nnz, float* C, void* stream);
int hgn_forman_post_delta(const float* A, const float* A2, float d_in_x, float d_out_y, int64_t N, int32_t x, int32_t y,
                          const int32_t* i_nb, int32_t dim_i, const int32_t* j_nb, int32_t dim_j, float* D, void* stream);

/* ---- targets and the one-step integrator ---------------------------------------------------------------------
 * out[i] = (ca*a[i] + cb*b[i]) + cc*c[i]   (c nullable), each product and sum rounded separately (no fma), so that
 *   flag.py:188  target - 2*cur + prev   (a=target, b=cur, c=prev; 1, -2, 1)
 *   flag.py:178  2*cur + acc - prev      (a=cur, b=acc, c=prev; 2, 1, -1)
 *   cylinder.py:163,171                  (a +/- b)
 * come out bit-identical to the reference's left-to-right fp32 evaluation.  n = number of elements (contiguous). */
int hgn_lincomb3(const float* a, float ca, const float* b, float cb, const float* c, float cc, int64_t n, float* out,
                 void* stream);

/* ---- one rollout step's state update (flag.py:169-180,243, cylinder.py:155-165, plate.py:246-257,328) ----------
 * What Normalizer.inverse -> hgn_lincomb3 -> torch.where -> append do in a rollout step, in ONE launch and with the same
 * device expressions in the same order (hgn_normalize with inverse = 1, then hgn_lincomb3 with cb = 1): equal bits.
 * Per row r of net_out [rows, ld_out] (the network output, normalised; out_cols columns, which must equal the normaliser
 * width F) and per column c:
 *   x     = net_out[r,c] * max(std[c], eps) + mean[c]                    (statistics as in hgn_normalize)
 *   c >= inv_from:  inv[r, c - inv_from] = x                           (inv nullable: cylinder's pressure with inv_from = d,
 *                                                                         plate's velocity with inv_from = 0)
 *   c <  d:         v    = (ca * cur[r,c] + x) + cp * prev[r,c]          (prev nullable: the last term is left out)
 *                   next[r,c] = v  if bit node_type[r] of free_mask is set  (types outside [0, 32) are never free)
 *                               else fallback[r,c]                       (fallback nullable: cur[r,c]; plate: the scripted target)
 *                   rec[r,c]      = rec_before ? cur[r,c] : next[r,c]    (rec nullable: the slice of the recorded trajectory;
 *                                                                         flag records the state BEFORE the step)
 *                   prev_out[r,c] = cur[r,c]                             (prev_out nullable: flag's next prev|world_pos,
 *                                                                         plate's cur_positions)
 * Every matrix has its own row stride (>= its row width), so an output may be a column slice of a wider slab.  Outputs must
 * not overlap inputs or each other.  node_type int64 with element stride ldt.  One thread per element of net_out, vector
 * loads and stores only: no atomics, no LDS, rows independent, equal bits on every run.
 * HGN_E_INVALID: null statistics, F outside 1..HGN_MAX_FEATURE_WIDTH, out_cols != F, rows outside [0, 2^31), d outside 1..F,
 * inv_from outside 0..F, a row stride that is zero or smaller than its row, null net_out / cur / node_type / next with
 * rows > 0. */
int hgn_rollout_advance(const float* net_out, int64_t ld_out, int out_cols, int F, const float* acc_sum,
                        const float* acc_sumsq, const float* acc_count, float eps, const float* cur, int64_t ld_cur, int d,
                        float ca, const float* prev, int64_t ld_prev, float cp, const int64_t* node_type, int64_t ldt,
                        uint32_t free_mask, const float* fallback, int64_t ld_fb, int64_t rows, float* next, int64_t ld_next,
                        float* rec, int64_t ld_rec, int rec_before, float* prev_out, int64_t ld_po, float* inv,
                        int64_t ld_inv, int inv_from, void* stream);

/* ---- backward of the state update (flag.py:169-180,243, cylinder.py:155-165, plate.py:246-257,328) --------------
 * The exact derivative of what hgn_rollout_advance computes (Normalizer.inverse, then ca*cur + x + cp*prev, then the per-row
 * choice by node type), for unrolled multi-step training: ONE launch, flat over [rows, F] like the forward, 256 threads per
 * block, no LDS, no atomics, equal bits on every run.  The statistics are constants (nothing flows into them); s[c] =
 * max(std[c], eps) is formed from acc_sum / acc_sumsq / acc_count / eps exactly as the forward forms it.
 * In:  d_next [rows, d] (nullable), d_inv [rows, F - inv_from] (nullable): the gradients of the forward's `next` and `inv`.
 * Out (each nullable, at least one given): d_net [rows, F], d_cur / d_prev / d_fallback [rows, d].  Every element of every
 * output given is written exactly once, zeros included: the buffers need no initialisation.
 * Per element, with g = d_next[r,c] (0 when absent or c >= d) and h = d_inv[r, c - inv_from] (0 when absent or c < inv_from):
 *   free row (bit node_type[r] of free_mask set; types outside [0, 32) are never free):
 *     d_net = s[c] * (g + h)     d_cur = ca * g     d_prev = cp * g     d_fallback = 0
 *   any other row:
 *     d_net = s[c] * h           d_prev = 0         d_cur = g without a fallback (has_fallback = 0), 0 with one
 *                                                   d_fallback = g with a fallback, 0 without
 * No fma contraction: every product and sum is rounded on its own.  Every matrix has its own row stride (>= its row width).
 * HGN_E_INVALID: null statistics, F outside 1..HGN_MAX_FEATURE_WIDTH, rows outside [0, 2^31), d outside 1..F, inv_from outside
 * 0..F, a row stride that is zero or smaller than its row, no output asked for, null node_type with rows > 0.  rows = 0: no-op. */
int hgn_rollout_advance_bwd(const float* d_next, int64_t ld_dnext, const float* d_inv, int64_t ld_dinv, int inv_from, int F,
                            const float* acc_sum, const float* acc_sumsq, const float* acc_count, float eps, int d, float ca,
                            float cp, const int64_t* node_type, int64_t ldt, uint32_t free_mask, int has_fallback,
                            int64_t rows, float* d_net, int64_t ld_dnet, float* d_cur, int64_t ld_dcur, float* d_prev,
                            int64_t ld_dprev, float* d_fallback, int64_t ld_dfb, void* stream);

/* ---- seeded training noise for a batch of frames (src/data/preprocessing.py:84-98, Preprocessing._add_noise) -----------------
 * What the reference does per frame with torch.normal, torch.where and two in-place additions -- a normal(0, std_) sample per
 * element of frame[field], zeroed on every row whose node type is not free, added to the field and, scaled by (1 - gamma), to
 * `target|field` -- for all frames of a batch in ONE launch, one thread per row, 256 threads per block, into fresh outputs.
 * Plain vector loads and stores: no LDS, no atomics; equal bits on every run.
 * x [rows, ldx], target (nullable) [rows, ld_tgt], out_x [rows, ld_ox], out_target (null iff target is) [rows, ld_ot]; d = 1..4
 * columns; node_type int64 with element stride ldt.  The rows are rows / rows_per_frame frames of rows_per_frame nodes each.
 * Generator: counter-based, so the sample of a row is a pure function of (seed, draw, frame id, node) and of nothing else -- not of
 * the frame's place in the batch, not of the batch size, not of the process that holds the frame.  Row r has f = r / rows_per_frame,
 * n = r % rows_per_frame and fid = frame_ids ? (uint32)frame_ids[f] : (uint32)f (frame_ids: device int64, one per frame).  It takes
 * the four words w_0..w_3 of Philox4x32-10 with counter (n, fid, (uint32)draw, (uint32)(draw >> 32)), key ((uint32)seed,
 * (uint32)(seed >> 32)), multipliers 0xD2511F53 / 0xCD9E8D57 and key increments 0x9E3779B9 / 0xBB67AE85 (Random123's constants
 * and known answers).  Box-Muller in fp32 with the accurate logf / sqrtf / cosf / sinf: k_i = w_i >> 9, u1 = (k_0 + 0.5) 2^-23
 * (exact, in (0, 1)), u2 = k_1 2^-23, rad = sqrtf(-2 logf(u1)), theta = 2 pi u2, z_0 = rad cosf(theta), z_1 = rad sinf(theta);
 * z_2, z_3 likewise from w_2, w_3.  Column c uses z_c.
 * A row is free when its type lies in [0, 32) and that bit of free_mask is set (the convention of hgn_rollout_advance).
 *   free row:       nz = std_ * z_c;  out_x = x + nz;  out_target = target + target_scale * nz    (every product and sum rounded
 *                                                                                                   on its own: no fma)
 *   any other row:  out_x = x, out_target = target, copied bit for bit
 * Every matrix has its own row stride; outputs must not overlap inputs; every output element is written exactly once.
 * rows = 0: no-op.  HGN_E_INVALID before any launch: d outside 1..4, rows outside [0, 2^31), rows_per_frame < 1 or not dividing
 * rows, a row stride smaller than d (ldt < 1), std_ negative or not finite, target and out_target not both null or both given,
 * null x / node_type / out_x with rows > 0. */
int hgn_training_noise(const float* x, int64_t ldx, int d, const int64_t* node_type, int64_t ldt, uint32_t free_mask,
                       int64_t rows, int64_t rows_per_frame, const int64_t* frame_ids /* nullable */, uint64_t seed,
                       uint64_t draw, float std_, const float* target /* nullable */, int64_t ld_tgt, float target_scale,
                       float* out_x, int64_t ld_ox, float* out_target /* null iff target is */, int64_t ld_ot, void* stream);

/* ---- per-frame losses of a batch of frames (flag.py:146-167, cylinder.py:123-153, plate.py:218-244: training_step and
 * validation_step; algorithms/MeshSimulator.py:151-156 "loss per trajectory", :295-297 [loss, pos_error] per frame) --------------
 * The masked mean squared error of the reference -- MSELoss()(target[mask], output[mask]), and for validation the same error of the
 * updated state -- for every frame of a batch and for the batch as a whole, without a host read.  The rows are B = rows /
 * rows_per_frame frames of rows_per_frame nodes each.
 * In:  net_out [rows, ld_out] (the network output, F columns), target [rows, ld_tgt] (the normalised target, as get_target returns
 *      it), node_type int64 with element stride ldt; a row is free when its type lies in [0, 32) and that bit of free_mask is set
 *      (the convention of hgn_rollout_advance).  Every matrix has its own row stride.
 *      State part, given whole or not at all: acc_sum / acc_sumsq / acc_count / eps of the output normaliser, cur [rows, ld_cur]
 *      (d columns), ca, prev (nullable) [rows, ld_prev] with cp, state_target [rows, ld_st] (d columns).  Without it d, ca, cp, eps
 *      and the strides of the absent matrices are not read.
 * Out: loss [B+1] float, state_err [B+1] float (null exactly when there is no state part), count [B+1] int64.  Entry f < B belongs
 *      to frame f, entry B to all rows.  With n_f = the number of free rows of frame f:
 *        S_f = sum over the free rows r of f, c < F, of ((double)net_out[r,c] - (double)target[r,c])^2
 *        loss[f] = (float)(S_f / ((double)n_f * F))          loss[B] = (float)(sum_f S_f / ((double)(sum_f n_f) * F))
 *        x = net_out[r,c] * max(std[c], eps) + mean[c],  v = (ca * cur[r,c] + x) + cp * prev[r,c]   for c < d, in fp32, every product
 *            and sum rounded on its own, the last term left out without prev: the expressions of hgn_rollout_advance, so v has the
 *            bits of the model's `update`
 *        E_f = sum over the free rows r of f, c < d, of ((double)v - (double)state_target[r,c])^2
 *        state_err[f] = (float)(E_f / ((double)n_f * d)),   state_err[B] likewise from the sums over all frames
 *        count[f] = n_f,  count[B] = sum_f n_f
 *      One rounding to fp32 per entry.  n_f = 0 gives IEEE 0 / 0 = NaN in that entry (what the reference's mean over no element
 *      gives) and leaves every other per-frame entry as it is.  Rows that are not free are not read beyond their type.
 * Order: a frame is cut into chunks of HGN_LOSS_CHUNK_ROWS rows counted from the frame's own first row; one thread per row adds the
 * squares of its row in ascending column order; the partial sums are doubles and meet in a fixed order: the lanes of a wavefront by
 * halving strides, the four wavefronts of a chunk as (0 + 1) + (2 + 3), the chunks of a frame in ascending order, and for entry B
 * the frames in ascending order.  No atomics.  Hence: two runs give equal bits; and loss[f], state_err[f] and count[f] depend on the
 * rows of frame f alone -- not on the frame's place in the batch and not on B.
 * At most two launches (partials, then one workgroup that finalises); the partials live in the caller's workspace
 * (hgn_frame_losses_workspace_bytes; 8-byte aligned).  Plain vector loads and stores.
 * rows = 0: no-op.  HGN_E_INVALID before any launch: F outside 1..HGN_MAX_FEATURE_WIDTH, rows outside [0, 2^31), rows_per_frame < 1
 * or not dividing rows, a state part given in part (prev without the rest included), state_err null with a state part or given
 * without one, d outside 1..F with a state part, a row stride smaller than its row (ldt < 1), null net_out / target / node_type /
 * loss / count with rows > 0, a workspace that is null, misaligned or too small. */
#define HGN_LOSS_CHUNK_ROWS 256 /* rows of a frame per chunk (= threads of a workgroup of the partial pass) */
int hgn_frame_losses_workspace_bytes(int64_t rows, int64_t rows_per_frame, size_t* bytes);
int hgn_frame_losses(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F, const int64_t* node_type,
                     int64_t ldt, uint32_t free_mask, int64_t rows, int64_t rows_per_frame, const float* acc_sum,
                     const float* acc_sumsq, const float* acc_count, float eps, const float* cur, int64_t ld_cur, int d, float ca,
                     const float* prev /* nullable */, int64_t ld_prev, float cp, const float* state_target, int64_t ld_st,
                     float* loss /*[B+1]*/, float* state_err /*[B+1] or null without a state part*/, int64_t* count /*[B+1]*/,
                     void* workspace, size_t ws_bytes, void* stream);

/* ---- backward of the per-frame losses ------------------------------------------------------------------------------------------
 * ONE launch, flat over [rows, F], 256 threads per block, no LDS, no atomics, equal bits on every run.  count [B+1] is the forward's;
 * g [B+1] holds the upstream gradients of `loss` (nullable as a whole = all zero; the caller zero-fills entries that got none).
 * Nothing flows through state_err: it is an evaluation figure, not a training loss.
 *   free row of frame f:  w = (float)((double)g[f] / ((double)count[f] * F) + (double)g[B] / ((double)count[B] * F))
 *                         d_net[r,c] = (2 * (net_out[r,c] - target[r,c])) * w     the difference and the product each rounded once in
 *                                                                                fp32 (the doubling is exact)
 *   any other row:        d_net[r,c] = 0
 *   d_target[r,c] = -d_net[r,c]
 * d_net [rows, ld_dnet] and d_target [rows, ld_dtgt] are each nullable, at least one must be given; every element of every output
 * given is written exactly once, so the buffers need no initialisation.
 * rows = 0: no-op.  HGN_E_INVALID before any launch: F outside 1..HGN_MAX_FEATURE_WIDTH, rows outside [0, 2^31), rows_per_frame < 1
 * or not dividing rows, a row stride smaller than its row (ldt < 1), no output asked for, null net_out / target / node_type / count
 * with rows > 0. */
int hgn_frame_losses_bwd(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F, const int64_t* node_type,
                         int64_t ldt, uint32_t free_mask, int64_t rows, int64_t rows_per_frame, const int64_t* count,
                         const float* g /* nullable */, float* d_net, int64_t ld_dnet, float* d_target, int64_t ld_dtgt,
                         void* stream);

/* ==== ragged batches: frames of different meshes in one batch ===================================================================
 * cylinder_flow and deforming_plate give every trajectory its own mesh, so a batch that mixes trajectories has frames of different
 * sizes.  A ragged batch is B frames of frame_rows = (N_0, .., N_{B-1}) rows, every N_b >= 1, rows = sum N_b; frame b owns the union
 * rows [P_b, P_{b+1}), P the exclusive prefix of frame_rows.  Every entry below takes the batch twice:
 *   frame_rows  HOST   const int64_t [B]     validated before any launch
 *   frame_ptr   DEVICE const int32_t [B+1]   = P, the caller's contract (built once per distinct batch shape and kept)
 * HGN_E_INVALID with the entry's name, before any launch: B < 1, an entry < 1, a sum that differs from rows (so rows = 0 is refused:
 * there is no empty ragged batch), rows >= 2^31, null frame_rows or frame_ptr, and whatever the uniform entry refuses.
 * The kernels clamp every bound they read from frame_ptr to [0, rows] and search it for a frame in [0, B): a frame_ptr that is not
 * the prefix of frame_rows gives wrong figures, never a read or write outside the caller's buffers.
 * Plain vector loads and stores, no atomics, equal bits on every run, 256 threads per workgroup, as the uniform kernels. */

/* ---- world edges of a ragged batch (plate.py:84-110 once per frame, MeshSimulator.py:159-234 for the union) ----------------------
 * hgn_radius_edges_batch_* for graphs of different sizes: pos / node_type hold the rows of the union, graph b owns rows
 * [P_b, P_{b+1}), a pair (s, r) is reported only if both ends lie in the same graph.  Every graph has its own mesh: nbr_rowptr
 * [rows+1] / nbr is the neighbour CSR of the UNION, rows and entries in union ids (both null = no exclusion).  Types, radius and the
 * distance expression are those of hgn_radius_edges_count.  Output: union ids in ascending (s, r) order = the concatenation over b of
 * what hgn_radius_edges_count/_fill return for graph b alone, shifted by P_b.
 * _count fills offsets [rows+1] (device int32, exclusive prefix of the per-sender counts, offsets[rows] = total) and, when
 * graph_offsets is not NULL, graph_offsets [B+1] (device int32: graph_offsets[b] = offsets[P_b] = edges before graph b,
 * graph_offsets[B] = total), and returns the total on the HOST: ONE stream synchronisation for the batch.  _fill writes senders /
 * receivers [total] int64.  One wavefront per sender row finds its graph by bisection of frame_ptr and sweeps the receivers of that
 * graph in chunks of 64: sum_b N_b^2 / 64 chunk iterations; sender rows of another type leave at once.
 * HGN_E_INVALID: the ragged refusals above with rows > 0x7ffffffe, whatever hgn_radius_edges_count refuses (d outside 1..3, ld < d,
 * ldt < 1, radius not >= 0, null pos / node_type, only one of nbr_rowptr / nbr), null outputs, workspace too small. */
int hgn_radius_edges_ragged_workspace_bytes(int64_t rows, const int64_t* frame_rows /*host [B]*/, int64_t n_graphs, size_t* bytes);
int hgn_radius_edges_ragged_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t rows,
                                  const int64_t* frame_rows /*host [B]*/, const int32_t* frame_ptr /*device [B+1]*/,
                                  int64_t n_graphs, float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                  const int32_t* nbr, int32_t* offsets /*[rows+1]*/, int32_t* graph_offsets /*[B+1] nullable*/,
                                  int64_t* total /*host*/, void* workspace, size_t ws_bytes, void* stream);
int hgn_radius_edges_ragged_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t rows,
                                 const int64_t* frame_rows /*host [B]*/, const int32_t* frame_ptr /*device [B+1]*/,
                                 int64_t n_graphs, float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                 const int32_t* nbr, const int32_t* offsets, int64_t* senders, int64_t* receivers, void* stream);

/* ---- seeded training noise for a ragged batch (src/data/preprocessing.py:84-98, Preprocessing._add_noise) -------------------------
 * hgn_training_noise with row r -> (f, n = r - P_f) found by bisection of frame_ptr, fid = frame_ids ? (uint32)frame_ids[f] :
 * (uint32)f.  The same Philox4x32-10 counter (n, fid, draw lo, draw hi), key and Box-Muller, the same free-row rule and arithmetic:
 * a row's sample stays a function of (seed, draw, frame id, node) alone, so the rows of frame f have the bits hgn_training_noise gives
 * that frame on its own with frame id fid.  ONE launch, one thread per row.
 * HGN_E_INVALID before any launch: the ragged refusals above and whatever hgn_training_noise refuses (d outside 1..4, a row stride
 * smaller than d, ldt < 1, std_ negative or not finite, target and out_target not both null or both given, null x / node_type /
 * out_x). */
int hgn_training_noise_ragged(const float* x, int64_t ldx, int d, const int64_t* node_type, int64_t ldt, uint32_t free_mask,
                              int64_t rows, const int64_t* frame_rows /*host [B]*/, const int32_t* frame_ptr /*device [B+1]*/,
                              int64_t n_frames, const int64_t* frame_ids /* nullable */, uint64_t seed, uint64_t draw, float std_,
                              const float* target /* nullable */, int64_t ld_tgt, float target_scale, float* out_x, int64_t ld_ox,
                              float* out_target /* null iff target is */, int64_t ld_ot, void* stream);

/* ---- per-frame losses of a ragged batch (flag.py:146-167, cylinder.py:123-153, plate.py:218-244: training_step and
 * validation_step; algorithms/MeshSimulator.py:151-156 "loss per trajectory", :295-297 [loss, pos_error] per frame) --------------
 * The outputs, formulas and NaN rule of hgn_frame_losses / _bwd with frame f = rows [P_f, P_{f+1}).  The order is the documented one:
 * chunks of HGN_LOSS_CHUNK_ROWS rows counted from the frame's own first row, lanes by halving strides, the four wavefronts as
 * (0 + 1) + (2 + 3), chunks ascending, frames ascending for entry B.  Hence
 *   - entries f < B have the bits that hgn_frame_losses gives for that frame alone;
 *   - with all N_b equal, all B+1 entries and the whole backward have the bits of the uniform entries.
 * Forward: at most two launches, nothing is read on the host.  The partial pass is a grid of B x ceil(max N_b / HGN_LOSS_CHUNK_ROWS)
 * workgroups -- workgroup (f, k) takes chunk k of frame f and leaves at once when the frame has no such chunk -- and one workgroup
 * finalises, adding for every frame the chunks it has.  The workspace holds one partial triple per workgroup of that grid
 * (hgn_frame_losses_ragged_workspace_bytes: grows with B and with max N_b; 8-byte aligned).
 * Backward: ONE launch, flat over [rows, F]; the frame of a row by bisection of frame_ptr; count [B+1] is the forward's, g [B+1] as in
 * hgn_frame_losses_bwd.
 * HGN_E_INVALID before any launch: the ragged refusals above, a grid of B x chunks that does not fit one launch (>= 2^31 workgroups),
 * and whatever hgn_frame_losses / _bwd refuse (F outside 1..HGN_MAX_FEATURE_WIDTH, a state part given in part, state_err null with a
 * state part or given without one, d outside 1..F with a state part, a row stride smaller than its row, ldt < 1, no output asked for,
 * null net_out / target / node_type / loss / count, a workspace that is null, misaligned or too small). */
int hgn_frame_losses_ragged_workspace_bytes(int64_t rows, const int64_t* frame_rows /*host [B]*/, int64_t n_frames, size_t* bytes);
int hgn_frame_losses_ragged(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                            const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows,
                            const int64_t* frame_rows /*host [B]*/, const int32_t* frame_ptr /*device [B+1]*/, int64_t n_frames,
                            const float* acc_sum, const float* acc_sumsq, const float* acc_count, float eps, const float* cur,
                            int64_t ld_cur, int d, float ca, const float* prev /* nullable */, int64_t ld_prev, float cp,
                            const float* state_target, int64_t ld_st, float* loss /*[B+1]*/,
                            float* state_err /*[B+1] or null without a state part*/, int64_t* count /*[B+1]*/, void* workspace,
                            size_t ws_bytes, void* stream);
int hgn_frame_losses_ragged_bwd(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                                const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows,
                                const int64_t* frame_rows /*host [B]*/, const int32_t* frame_ptr /*device [B+1]*/, int64_t n_frames,
                                const int64_t* count, const float* g /* nullable */, float* d_net, int64_t ld_dnet,
                                float* d_target, int64_t ld_dtgt, void* stream);

/* ---- backward of the connector's cluster mean (hierarchical_connector.py:39-45; rmp.py HierarchicalConnector.run, the line
 * `means_all = ops.aggregate([both], [(t.node_perm, t.csr.rowptr, t.csr.seg)], ('mean',))`) ----------------------------------
 * mean[s] = (1 / count(s)) * sum of data[member] over the members of cluster s.  The member list has M entries and need not
 * cover the rows: obstacle rows (remote_message_passing.py:82-137), HDBSCAN noise and rows that intra-cluster sampling left out
 * belong to no cluster, and a row may be a member more than once.  hgn_segment_reduce_bwd cannot serve that: it runs over as
 * many items as the output has rows and writes only the rows it meets.  This entry is node-parallel instead:
 *   seg_rowptr [S+1]   CSR row pointer of the member list by cluster: count(s) = seg_rowptr[s+1] - seg_rowptr[s]
 *   item_seg   [M]     cluster of member-list position j
 *   node_rowptr [rows+1], node_items [M]   CSR of the member list by node row: the positions j at which row n is listed
 *   d_data[n, c] = sum over q in [node_rowptr[n], node_rowptr[n+1]), in that order, of
 *                  d_mean[item_seg[node_items[q]], c] / (float)count(.)          (g = 0.f; g += v / (float)cnt)
 * ONE launch, flat over [rows, D], 256 threads per block; every element of d_data is written exactly once, 0 for a row in no
 * cluster, so the buffer needs no initialisation; no atomics, no LDS, equal bits on every run.  The expression is that of
 * hgn_segment_reduce_bwd's mean for D != 128: where the members are a partition of the rows the two agree bit for bit.
 * d_mean [S, ld_dmean], d_data [rows, ld], D >= 1 columns, both row strides >= D.  Ids outside their range are skipped.
 * HGN_E_INVALID: D < 1, ld < D, ld_dmean < D, rows / M / S outside [0, 2^31), M > 0 with S = 0, null d_data with rows > 0, any
 * other null pointer with rows > 0 and M > 0.  rows = 0: no-op.  M = 0 with rows > 0: d_data is zero-filled. */
int hgn_member_mean_bwd(const float* d_mean, int64_t ld_dmean, int D, const int32_t* seg_rowptr, int64_t S,
                        const int32_t* item_seg, const int32_t* node_rowptr, const int32_t* node_items, int64_t rows,
                        int64_t M, float* d_data, int64_t ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif
