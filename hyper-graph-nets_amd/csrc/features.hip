// Frame -> graph features (include/hgn_features.h): cell edges, relative-position edge features, node features and
// the online normaliser.  All of it is HBM-bound byte / index work over [E, <=8] and [N, <=12] rows: flat,
// fully coalesced passes, fp64 accumulation for the statistics, fixed-order reductions (deterministic).
#include <hipcub/hipcub.hpp>
#include "hgn_host.h"
#include "../../include/hgn_features.h"

// The reference evaluates these features op by op in fp32 (every product and sum rounded): no fma contraction in
// this translation unit, so that e.g. E[x^2] - mean^2 cancels exactly the way normalizer.py:70 does.
#pragma clang fp contract(off)

namespace hgn {

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ----------------------------------------------------------------------------------------------------------
// util.py:50-89 -- unique undirected cell edges, two-way
// ----------------------------------------------------------------------------------------------------------
__global__ void cell_keys_kernel(const int64_t* __restrict__ cells, long n_cells, int verts,
                                 unsigned long long* __restrict__ keys, int* __restrict__ flag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells * verts) return;
  const long c = i / verts;
  const int k = (int)(i - c * verts);
  const int64_t u = cells[c * verts + k];
  const int64_t v = cells[c * verts + (k + 1 == verts ? 0 : k + 1)];
  if (u < 0 || v < 0 || u > 0x7fffffffLL || v > 0x7fffffffLL) { atomicOr(flag, 1); keys[i] = 0; return; }
  const unsigned long long hi = (unsigned long long)(u > v ? u : v), lo = (unsigned long long)(u > v ? v : u);
  keys[i] = (hi << 32) | lo;
}

__global__ void two_way_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ n_unique,
                               int64_t* __restrict__ senders, int64_t* __restrict__ receivers) {
  const long n = *n_unique;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const int64_t hi = (int64_t)(k >> 32), lo = (int64_t)(k & 0xffffffffULL);
  senders[i] = hi; receivers[i] = lo;
  senders[n + i] = lo; receivers[n + i] = hi;
}

// ----------------------------------------------------------------------------------------------------------
// relative-position edge features: one thread per edge
// ----------------------------------------------------------------------------------------------------------
__global__ void rel_edge_kernel(const float* __restrict__ a, long lda, int da, const float* __restrict__ b, long ldb,
                                int db, long n_rows, const int64_t* __restrict__ snd, const int64_t* __restrict__ rcv,
                                long E, float* __restrict__ feat, long ldf, float* __restrict__ len_a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t s = snd[e], r = rcv[e];
  if (s < 0 || r < 0 || s >= n_rows || r >= n_rows) return;
  float ra[3], rb[3];
  float qa = 0.f, qb = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ra[i] = i < da ? a[s * lda + i] - a[r * lda + i] : 0.f;
    qa += ra[i] * ra[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    rb[i] = i < db ? b[s * ldb + i] - b[r * ldb + i] : 0.f;
    qb += rb[i] * rb[i];
  }
  const float na = sqrtf(qa);
  if (len_a) len_a[e] = na;
  if (feat) {
    float* o = feat + e * ldf;
    for (int i = 0; i < da; ++i) o[i] = ra[i];
    o[da] = na;
    if (db > 0) {
      for (int i = 0; i < db; ++i) o[da + 1 + i] = rb[i];
      o[da + 1 + db] = sqrtf(qb);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------
// node features: flat over [N, d + n_classes]
// ----------------------------------------------------------------------------------------------------------
__global__ void node_feat_kernel(const float* __restrict__ cur, const float* __restrict__ prev, long ld, int d,
                                 const int64_t* __restrict__ node_type, long ldt, const int* __restrict__ map,
                                 int map_len, int n_classes, int vel_first, int vel_mask_type, long N,
                                 float* __restrict__ out, long ldo) {
  const int W = d + n_classes;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * W) return;
  const long n = i / W;
  const int c = (int)(i - n * W);
  const int64_t t = node_type[n * ldt];
  const int vc = vel_first ? c : c - n_classes;      // velocity column or <0 / >=d
  float v;
  if (vc >= 0 && vc < d) {
    v = cur ? cur[n * ld + vc] - (prev ? prev[n * ld + vc] : 0.f) : 0.f;
    if (vel_mask_type >= 0 && t != vel_mask_type) v = 0.f;
  } else {
    const int oc = vel_first ? c - d : c;
    int64_t cls = t;
    if (map) cls = (t >= 0 && t < map_len) ? map[t] : -1;
    v = cls == oc ? 1.f : 0.f;
  }
  out[n * ldo + c] = v;
}

// ----------------------------------------------------------------------------------------------------------
// normaliser
// ----------------------------------------------------------------------------------------------------------
constexpr int ST = 256;          // threads per block of the statistics pass
constexpr int MAXBLK = 1024;

// Flat pass: the active threads of the grid are a multiple of F, so a thread always sees one column.
__global__ void col_stats_kernel(const float* __restrict__ x, long n_elem, int F, int active_per_block,
                                 double* __restrict__ part /*[gridDim.x][2F]*/) {
  __shared__ double s1[ST], s2[ST];
  const int t = threadIdx.x;
  double a = 0.0, q = 0.0;
  if (t < active_per_block) {
    const long stride = (long)gridDim.x * active_per_block;
    for (long i = (long)blockIdx.x * active_per_block + t; i < n_elem; i += stride) {
      const double v = (double)x[i];
      a += v; q += v * v;
    }
  }
  s1[t] = a; s2[t] = q;
  __syncthreads();
  if (t < F) {                  // column of thread u is (blockIdx.x*active + u) % F == u % F (active % F == 0)
    double A = 0.0, Q = 0.0;
    for (int u = t; u < active_per_block; u += F) { A += s1[u]; Q += s2[u]; }
    part[(long)blockIdx.x * 2 * F + t] = A;
    part[(long)blockIdx.x * 2 * F + F + t] = Q;
  }
}

// One block: 256 threads = G groups x 2F columns; a group strides over the block partials, groups are folded in
// fixed order (deterministic).
__global__ void col_stats_final_kernel(const double* __restrict__ part, int nblk, int F, float* __restrict__ batch) {
  __shared__ double sh[ST];
  const int t = threadIdx.x, W = 2 * F, G = ST / W;
  const int c = t % W, g = t / W;
  double A = 0.0;
  if (g < G)
    for (int b = g; b < nblk; b += G) A += part[(long)b * W + c];
  sh[t] = A;
  __syncthreads();
  if (t < W) {
    double S = 0.0;
    for (int k = 0; k < G; ++k) S += sh[k * W + t];
    batch[t] = (float)S;
  }
}

__global__ void normalizer_update_kernel(float* acc_sum, float* acc_sumsq, float* acc_count, float* num_acc,
                                         const float* __restrict__ batch, const float* __restrict__ count, int F,
                                         float max_acc) {
  const int t = threadIdx.x;
  const bool go = *num_acc < max_acc;
  __syncthreads();
  if (!go) return;
  if (t < F) { acc_sum[t] += batch[t]; acc_sumsq[t] += batch[F + t]; }
  if (t == 0) { *acc_count += *count; *num_acc += 1.f; }
}

__global__ void normalize_kernel(const float* __restrict__ x, long n_elem, int F, const float* __restrict__ acc_sum,
                                 const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count, float eps,
                                 int inverse, float* __restrict__ out) {
  __shared__ float mean[HGN_MAX_FEATURE_WIDTH], sd[HGN_MAX_FEATURE_WIDTH];
  if ((int)threadIdx.x < F) {
    const float safe = fmaxf(*acc_count, 1.f);
    const float m = acc_sum[threadIdx.x] / safe;
    const float s = sqrtf(fabsf(acc_sumsq[threadIdx.x] / safe - m * m));   // no fma (file-wide): mean^2 is rounded
    mean[threadIdx.x] = m;
    sd[threadIdx.x] = fmaxf(s, eps);
  }
  __syncthreads();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_elem) return;
  const int c = (int)(i % F);
  out[i] = inverse ? x[i] * sd[c] + mean[c] : (x[i] - mean[c]) / sd[c];
}

__global__ void lincomb3_kernel(const float* __restrict__ a, float ca, const float* __restrict__ b, float cb,
                                const float* __restrict__ c, float cc, long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = ca * a[i] + cb * b[i];          // contraction is off in this file: three roundings
  if (c) v = v + cc * c[i];
  out[i] = v;
}

// One rollout step's state update, flat over [rows, F]: the expressions of normalize_kernel (inverse) and lincomb3_kernel in their
// order, then the selection torch.where makes.  The two statistics of a column are formed per thread (three loads) instead of
// once per block: same operations on the same values, same bits, no LDS.
__global__ void rollout_advance_kernel(const float* __restrict__ net_out, long ld_out, int F, const float* __restrict__ acc_sum,
                                       const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count, float eps,
                                       const float* __restrict__ cur, long ld_cur, int d, float ca,
                                       const float* __restrict__ prev, long ld_prev, float cp,
                                       const int64_t* __restrict__ node_type, long ldt, unsigned free_mask,
                                       const float* __restrict__ fallback, long ld_fb, long rows, float* __restrict__ next,
                                       long ld_next, float* __restrict__ rec, long ld_rec, int rec_before,
                                       float* __restrict__ prev_out, long ld_po, float* __restrict__ inv, long ld_inv,
                                       int inv_from) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const long r = i / F;
  const int c = (int)(i - r * F);
  const float safe = fmaxf(*acc_count, 1.f);
  const float m = acc_sum[c] / safe;
  const float s = fmaxf(sqrtf(fabsf(acc_sumsq[c] / safe - m * m)), eps);
  const float x = net_out[r * ld_out + c] * s + m;                 // Normalizer.inverse
  if (inv && c >= inv_from) inv[r * ld_inv + (c - inv_from)] = x;
  if (c >= d) return;                                              // a column that is not integrated (cylinder: pressure)
  const float q = cur[r * ld_cur + c];
  float v = ca * q + 1.f * x;                                      // lincomb3 with cb = 1
  if (prev) v = v + cp * prev[r * ld_prev + c];
  const int64_t t = node_type[r * ldt];
  const bool is_free = t >= 0 && t < 32 && ((free_mask >> (unsigned)t) & 1u);
  const float nx = is_free ? v : (fallback ? fallback[r * ld_fb + c] : q);
  next[r * ld_next + c] = nx;
  if (rec) rec[r * ld_rec + c] = rec_before ? q : nx;
  if (prev_out) prev_out[r * ld_po + c] = q;
}

// Backward of rollout_advance_kernel, flat over [rows, F] like the forward: the scale of a column is formed per thread with the
// forward's expressions, every output element is written exactly once (zeros included), no LDS, no atomics.
// g = d_next[r,c] (0 when absent or c >= d), h = d_inv[r, c - inv_from] (0 when absent or c < inv_from).
__global__ void rollout_advance_bwd_kernel(const float* __restrict__ d_next, long ld_dn, const float* __restrict__ d_inv,
                                           long ld_di, int inv_from, int F, const float* __restrict__ acc_sum,
                                           const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count, float eps,
                                           int d, float ca, float cp, const int64_t* __restrict__ node_type, long ldt,
                                           unsigned free_mask, int has_fallback, long rows, float* __restrict__ d_net,
                                           long ld_net, float* __restrict__ d_cur, long ld_dc, float* __restrict__ d_prev,
                                           long ld_dp, float* __restrict__ d_fb, long ld_df) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const long r = i / F;
  const int c = (int)(i - r * F);
  const float g = (d_next && c < d) ? d_next[r * ld_dn + c] : 0.f;
  const float h = (d_inv && c >= inv_from) ? d_inv[r * ld_di + (c - inv_from)] : 0.f;
  const int64_t t = node_type[r * ldt];
  const bool is_free = t >= 0 && t < 32 && ((free_mask >> (unsigned)t) & 1u);
  if (d_net) {
    const float safe = fmaxf(*acc_count, 1.f);
    const float m = acc_sum[c] / safe;
    const float s = fmaxf(sqrtf(fabsf(acc_sumsq[c] / safe - m * m)), eps);   // the forward's s_c
    d_net[r * ld_net + c] = s * (is_free ? g + h : h);
  }
  if (c >= d) return;
  if (d_cur) d_cur[r * ld_dc + c] = is_free ? ca * g : (has_fallback ? 0.f : g);
  if (d_prev) d_prev[r * ld_dp + c] = is_free ? cp * g : 0.f;
  if (d_fb) d_fb[r * ld_df + c] = (is_free || !has_fallback) ? 0.f : g;
}

// Training noise (data/preprocessing.py:84-98), one thread per row.  The sample of a row is a pure function of (seed, draw, frame id,
// node): Philox4x32-10 with counter (node, frame id, draw lo, draw hi) and key (seed lo, seed hi) gives four words, Box-Muller in
// fp32 turns them into four normals, column c takes z_c.  Nothing depends on where the row sits in the batch.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// u1 = (k_a + 0.5) 2^-23 lies in (0, 1) and is exact in fp32 (k < 2^23), u2 = k_b 2^-23 in [0, 1); the accurate library functions.
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& za, float& zb) {
  const float u1 = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;
  const float u2 = (float)(wb >> 9) * 0x1p-23f;
  const float rad = sqrtf(-2.f * logf(u1));
  const float theta = 6.283185307179586f * u2;
  za = rad * cosf(theta);
  zb = rad * sinf(theta);
}

__global__ void training_noise_kernel(const float* __restrict__ x, long ldx, int d, const int64_t* __restrict__ node_type, long ldt,
                                      unsigned free_mask, long rows, long rows_per_frame, const int64_t* __restrict__ frame_ids,
                                      unsigned key0, unsigned key1, unsigned draw0, unsigned draw1, float std_,
                                      const float* __restrict__ target, long ld_tgt, float target_scale, float* __restrict__ out_x,
                                      long ld_ox, float* __restrict__ out_target, long ld_ot) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int64_t t = node_type[r * ldt];
  const bool is_free = t >= 0 && t < 32 && ((free_mask >> (unsigned)t) & 1u);
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (is_free) {
    const long f = r / rows_per_frame;
    const unsigned node = (unsigned)(r - f * rows_per_frame);
    const unsigned fid = frame_ids ? (unsigned)frame_ids[f] : (unsigned)f;
    unsigned w[4];
    philox4x32_10(node, fid, draw0, draw1, key0, key1, w);
    box_muller(w[0], w[1], z[0], z[1]);
    if (d > 2) box_muller(w[2], w[3], z[2], z[3]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= d) break;
    const float xv = x[r * ldx + c];
    if (!is_free) {                                                 // a copy, bit for bit (-0.0 and NaN payloads included)
      out_x[r * ld_ox + c] = xv;
      if (target) out_target[r * ld_ot + c] = target[r * ld_tgt + c];
      continue;
    }
    // Plain products and sums: contraction is off in this file, so each is rounded on its own.  (__fmul_rn / __fadd_rn are inlined
    // as ordinary operations that the compiler does fuse: the emitted code had v_fmac for x + std * z.)
    const float nz = std_ * z[c];
    out_x[r * ld_ox + c] = xv + nz;
    if (target) {
      const float scaled = target_scale * nz;
      out_target[r * ld_ot + c] = target[r * ld_tgt + c] + scaled;
    }
  }
}

// Per-frame masked mean squared errors (flag.py:150-167, cylinder.py:123-153, plate.py:218-244; MeshSimulator.py:151-156,295-297).
// A frame is cut into chunks of HGN_LOSS_CHUNK_ROWS rows counted from ITS OWN first row; one workgroup per chunk, one thread per row.
// A thread adds the squares of its row in ascending column order; partials are doubles and meet lanes -> waves -> (finalise) chunks of
// a frame in ascending order -> frames in ascending order for the entry over all rows.  No atomics: equal bits on every run, and what
// a frame gets depends on its own rows alone.  The statistics of a column are formed once per workgroup with the expressions of
// rollout_advance_kernel (same operations on the same values: same bits), and v is that kernel's v.
static_assert(HGN_LOSS_CHUNK_ROWS == 256, "one thread per row of a chunk, four wavefronts per workgroup");
__device__ __forceinline__ double loss_block_sum(double s, double* lds) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);    // (every thread: only thread 0's copy is used)
}

__global__ __launch_bounds__(HGN_LOSS_CHUNK_ROWS) void frame_losses_partial_kernel(
    const float* __restrict__ net_out, long ld_out, const float* __restrict__ target, long ld_tgt, int F,
    const int64_t* __restrict__ node_type, long ldt, unsigned free_mask, long rows_per_frame, long chunks_per_frame,
    const float* __restrict__ acc_sum, const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count, float eps,
    const float* __restrict__ cur, long ld_cur, int d, float ca, const float* __restrict__ prev, long ld_prev, float cp,
    const float* __restrict__ state_target, long ld_st, double* __restrict__ part_s, double* __restrict__ part_e,
    long long* __restrict__ part_n) {
  __shared__ float mean[HGN_MAX_FEATURE_WIDTH], sd[HGN_MAX_FEATURE_WIDTH];
  __shared__ double lds_s[HGN_LOSS_CHUNK_ROWS / 64], lds_e[HGN_LOSS_CHUNK_ROWS / 64];
  __shared__ int lds_n[HGN_LOSS_CHUNK_ROWS / 64];
  const int t = threadIdx.x;
  if (cur && t < d) {
    const float safe = fmaxf(*acc_count, 1.f);
    const float m = acc_sum[t] / safe;
    mean[t] = m;
    sd[t] = fmaxf(sqrtf(fabsf(acc_sumsq[t] / safe - m * m)), eps);
  }
  __syncthreads();
  const long f = (long)blockIdx.x / chunks_per_frame;
  const long k = (long)blockIdx.x - f * chunks_per_frame;
  const long local = k * HGN_LOSS_CHUNK_ROWS + t;               // the row's place in its frame
  bool is_free = false;
  double s = 0.0, e = 0.0;
  if (local < rows_per_frame) {
    const long r = f * rows_per_frame + local;
    const int64_t ty = node_type[r * ldt];
    is_free = ty >= 0 && ty < 32 && ((free_mask >> (unsigned)ty) & 1u);
    if (is_free) {
      const float* o = net_out + r * ld_out;
      const float* g = target + r * ld_tgt;
      for (int c = 0; c < F; ++c) {
        const double diff = (double)o[c] - (double)g[c];
        s += diff * diff;
      }
      if (cur) {
        for (int c = 0; c < d; ++c) {
          const float x = o[c] * sd[c] + mean[c];                // Normalizer.inverse
          float v = ca * cur[r * ld_cur + c] + 1.f * x;          // lincomb3 with cb = 1
          if (prev) v = v + cp * prev[r * ld_prev + c];
          const double diff = (double)v - (double)state_target[r * ld_st + c];
          e += diff * diff;
        }
      }
    }
  }
  const int n_wave = __popcll(__ballot(is_free));
  if ((t & 63) == 0) lds_n[t >> 6] = n_wave;
  const double S = loss_block_sum(s, lds_s);                     // its barrier also covers lds_n
  const double E = loss_block_sum(e, lds_e);
  if (t == 0) {
    part_s[blockIdx.x] = S;
    part_e[blockIdx.x] = E;
    part_n[blockIdx.x] = (long long)((lds_n[0] + lds_n[1]) + (lds_n[2] + lds_n[3]));
  }
}

// One workgroup.  Frames are taken 256 at a time: thread t adds the chunks of frame base + t in ascending order and writes the frame's
// entries; the three running totals are then advanced over these 256 frames in ascending order by one thread each.
__global__ __launch_bounds__(256) void frame_losses_final_kernel(const double* __restrict__ part_s, const double* __restrict__ part_e,
                                                                 const long long* __restrict__ part_n, long n_frames,
                                                                 long chunks_per_frame, int F, int d, float* __restrict__ loss,
                                                                 float* __restrict__ state_err, int64_t* __restrict__ count) {
  __shared__ double fs[256], fe[256];
  __shared__ long long fn[256];
  __shared__ double tot_s, tot_e;
  __shared__ long long tot_n;
  const int t = threadIdx.x;
  if (t == 0) { tot_s = 0.0; tot_e = 0.0; tot_n = 0; }
  for (long base = 0; base < n_frames; base += 256) {
    const long f = base + t;
    double S = 0.0, E = 0.0;
    long long n = 0;
    if (f < n_frames) {
      for (long k = 0; k < chunks_per_frame; ++k) {
        const long b = f * chunks_per_frame + k;
        S += part_s[b]; E += part_e[b]; n += part_n[b];
      }
      loss[f] = (float)(S / ((double)n * (double)F));              // n = 0: IEEE 0 / 0 = NaN
      if (state_err) state_err[f] = (float)(E / ((double)n * (double)d));
      count[f] = (int64_t)n;
    }
    fs[t] = S; fe[t] = E; fn[t] = n;
    __syncthreads();
    const int live = (int)(n_frames - base < 256 ? n_frames - base : 256);
    if (t == 0) { double a = tot_s; for (int j = 0; j < live; ++j) a += fs[j]; tot_s = a; }
    if (t == 64) { double a = tot_e; for (int j = 0; j < live; ++j) a += fe[j]; tot_e = a; }
    if (t == 128) { long long a = tot_n; for (int j = 0; j < live; ++j) a += fn[j]; tot_n = a; }
    __syncthreads();
  }
  if (t == 0) {
    loss[n_frames] = (float)(tot_s / ((double)tot_n * (double)F));
    if (state_err) state_err[n_frames] = (float)(tot_e / ((double)tot_n * (double)d));
    count[n_frames] = (int64_t)tot_n;
  }
}

// Backward of the losses with respect to the network output and the target, flat over [rows, F]: a free row of frame f gets
// (2 (net - target)) * w with w = g[f] / (n_f F) + g[B] / (n_all F) formed in double and rounded once; every other row gets zeros.
// Every element of every output given is written exactly once.  No LDS, no atomics.
__global__ void frame_losses_bwd_kernel(const float* __restrict__ net_out, long ld_out, const float* __restrict__ target, long ld_tgt,
                                        int F, const int64_t* __restrict__ node_type, long ldt, unsigned free_mask, long rows,
                                        long rows_per_frame, const int64_t* __restrict__ count, const float* __restrict__ g,
                                        float* __restrict__ d_net, long ld_dn, float* __restrict__ d_target, long ld_dt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const long r = i / F;
  const int c = (int)(i - r * F);
  const int64_t ty = node_type[r * ldt];
  const bool is_free = ty >= 0 && ty < 32 && ((free_mask >> (unsigned)ty) & 1u);
  float v = 0.f;
  if (is_free && g) {
    const long f = r / rows_per_frame, B = rows / rows_per_frame;
    const float w = (float)((double)g[f] / ((double)count[f] * (double)F) + (double)g[B] / ((double)count[B] * (double)F));
    const float diff = net_out[r * ld_out + c] - target[r * ld_tgt + c];
    v = (2.f * diff) * w;
  }
  if (d_net) d_net[r * ld_dn + c] = v;
  if (d_target) d_target[r * ld_dt + c] = -v;
}

// ----------------------------------------------------------------------------------------------------------
// ragged batches: B frames of N_0 .. N_{B-1} rows, frame f = rows [frame_ptr[f], frame_ptr[f+1]) of the union
// ----------------------------------------------------------------------------------------------------------
// frame_ptr [B+1] is the caller's device copy of the exclusive prefix of the frame sizes the entry validated on the host.  The kernels
// below never trust it for an address: a bound read from it is clamped to [0, rows] and an end below its start gives an empty frame,
// and the search returns a frame in [0, B), so a wrong array gives wrong figures and nothing else.
__device__ __forceinline__ long ragged_bound(const int* __restrict__ frame_ptr, long i, long rows) {
  const long v = frame_ptr[i];
  return v < 0 ? 0 : (v > rows ? rows : v);
}

// the frame that owns row r: the last f in [0, B) with frame_ptr[f] <= r (reads entries 1 .. B-1 only)
__device__ __forceinline__ long ragged_frame_of(const int* __restrict__ frame_ptr, long B, long r) {
  long lo = 0, hi = B - 1;
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if ((long)frame_ptr[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// hgn_training_noise for a ragged batch: training_noise_kernel with (frame, node) found from frame_ptr -- the same counter, key and
// Box-Muller, so the rows of a frame have the bits the uniform kernel gives that frame with the same frame id.
__global__ void training_noise_ragged_kernel(const float* __restrict__ x, long ldx, int d, const int64_t* __restrict__ node_type,
                                             long ldt, unsigned free_mask, long rows, const int* __restrict__ frame_ptr, long n_frames,
                                             const int64_t* __restrict__ frame_ids, unsigned key0, unsigned key1, unsigned draw0,
                                             unsigned draw1, float std_, const float* __restrict__ target, long ld_tgt,
                                             float target_scale, float* __restrict__ out_x, long ld_ox,
                                             float* __restrict__ out_target, long ld_ot) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int64_t t = node_type[r * ldt];
  const bool is_free = t >= 0 && t < 32 && ((free_mask >> (unsigned)t) & 1u);
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (is_free) {
    const long f = ragged_frame_of(frame_ptr, n_frames, r);
    const unsigned node = (unsigned)(r - ragged_bound(frame_ptr, f, rows));
    const unsigned fid = frame_ids ? (unsigned)frame_ids[f] : (unsigned)f;
    unsigned w[4];
    philox4x32_10(node, fid, draw0, draw1, key0, key1, w);
    box_muller(w[0], w[1], z[0], z[1]);
    if (d > 2) box_muller(w[2], w[3], z[2], z[3]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= d) break;
    const float xv = x[r * ldx + c];
    if (!is_free) {                                                 // a copy, bit for bit (-0.0 and NaN payloads included)
      out_x[r * ld_ox + c] = xv;
      if (target) out_target[r * ld_ot + c] = target[r * ld_tgt + c];
      continue;
    }
    const float nz = std_ * z[c];                                   // plain products and sums, as in training_noise_kernel
    out_x[r * ld_ox + c] = xv + nz;
    if (target) {
      const float scaled = target_scale * nz;
      out_target[r * ld_ot + c] = target[r * ld_tgt + c] + scaled;
    }
  }
}

// hgn_frame_losses for a ragged batch.  Workgroup (f, k) of a grid of B x max_chunks takes chunk k of frame f, counted from the
// frame's own first row; a workgroup past its frame's last chunk leaves at once and writes nothing (the finalising pass reads only
// the chunks a frame has).  Per row and per workgroup the operations and their order are those of frame_losses_partial_kernel.
__global__ __launch_bounds__(HGN_LOSS_CHUNK_ROWS) void frame_losses_ragged_partial_kernel(
    const float* __restrict__ net_out, long ld_out, const float* __restrict__ target, long ld_tgt, int F,
    const int64_t* __restrict__ node_type, long ldt, unsigned free_mask, long rows, const int* __restrict__ frame_ptr,
    long max_chunks, const float* __restrict__ acc_sum, const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count,
    float eps, const float* __restrict__ cur, long ld_cur, int d, float ca, const float* __restrict__ prev, long ld_prev, float cp,
    const float* __restrict__ state_target, long ld_st, double* __restrict__ part_s, double* __restrict__ part_e,
    long long* __restrict__ part_n) {
  __shared__ float mean[HGN_MAX_FEATURE_WIDTH], sd[HGN_MAX_FEATURE_WIDTH];
  __shared__ double lds_s[HGN_LOSS_CHUNK_ROWS / 64], lds_e[HGN_LOSS_CHUNK_ROWS / 64];
  __shared__ int lds_n[HGN_LOSS_CHUNK_ROWS / 64];
  const int t = threadIdx.x;
  const long f = (long)blockIdx.x / max_chunks;
  const long k = (long)blockIdx.x - f * max_chunks;
  const long first = ragged_bound(frame_ptr, f, rows);
  const long frame_rows = ragged_bound(frame_ptr, f + 1, rows) - first;       // <= 0: an empty frame
  if (k * HGN_LOSS_CHUNK_ROWS >= frame_rows) return;                          // uniform per workgroup, before any barrier
  if (cur && t < d) {
    const float safe = fmaxf(*acc_count, 1.f);
    const float m = acc_sum[t] / safe;
    mean[t] = m;
    sd[t] = fmaxf(sqrtf(fabsf(acc_sumsq[t] / safe - m * m)), eps);
  }
  __syncthreads();
  const long local = k * HGN_LOSS_CHUNK_ROWS + t;               // the row's place in its frame
  bool is_free = false;
  double s = 0.0, e = 0.0;
  if (local < frame_rows) {
    const long r = first + local;
    const int64_t ty = node_type[r * ldt];
    is_free = ty >= 0 && ty < 32 && ((free_mask >> (unsigned)ty) & 1u);
    if (is_free) {
      const float* o = net_out + r * ld_out;
      const float* g = target + r * ld_tgt;
      for (int c = 0; c < F; ++c) {
        const double diff = (double)o[c] - (double)g[c];
        s += diff * diff;
      }
      if (cur) {
        for (int c = 0; c < d; ++c) {
          const float x = o[c] * sd[c] + mean[c];                // Normalizer.inverse
          float v = ca * cur[r * ld_cur + c] + 1.f * x;          // lincomb3 with cb = 1
          if (prev) v = v + cp * prev[r * ld_prev + c];
          const double diff = (double)v - (double)state_target[r * ld_st + c];
          e += diff * diff;
        }
      }
    }
  }
  const int n_wave = __popcll(__ballot(is_free));
  if ((t & 63) == 0) lds_n[t >> 6] = n_wave;
  const double S = loss_block_sum(s, lds_s);                     // its barrier also covers lds_n
  const double E = loss_block_sum(e, lds_e);
  if (t == 0) {
    part_s[blockIdx.x] = S;
    part_e[blockIdx.x] = E;
    part_n[blockIdx.x] = (long long)((lds_n[0] + lds_n[1]) + (lds_n[2] + lds_n[3]));
  }
}

// One workgroup: frame_losses_final_kernel with every frame's own number of chunks.
__global__ __launch_bounds__(256) void frame_losses_ragged_final_kernel(const double* __restrict__ part_s,
                                                                        const double* __restrict__ part_e,
                                                                        const long long* __restrict__ part_n, long n_frames,
                                                                        long rows, const int* __restrict__ frame_ptr, long max_chunks,
                                                                        int F, int d, float* __restrict__ loss,
                                                                        float* __restrict__ state_err, int64_t* __restrict__ count) {
  __shared__ double fs[256], fe[256];
  __shared__ long long fn[256];
  __shared__ double tot_s, tot_e;
  __shared__ long long tot_n;
  const int t = threadIdx.x;
  if (t == 0) { tot_s = 0.0; tot_e = 0.0; tot_n = 0; }
  for (long base = 0; base < n_frames; base += 256) {
    const long f = base + t;
    double S = 0.0, E = 0.0;
    long long n = 0;
    if (f < n_frames) {
      const long frame_rows = ragged_bound(frame_ptr, f + 1, rows) - ragged_bound(frame_ptr, f, rows);
      long chunks = frame_rows > 0 ? (frame_rows + HGN_LOSS_CHUNK_ROWS - 1) / HGN_LOSS_CHUNK_ROWS : 0;
      if (chunks > max_chunks) chunks = max_chunks;                 // (only a frame_ptr that is not the prefix of frame_rows)
      for (long k = 0; k < chunks; ++k) {
        const long b = f * max_chunks + k;
        S += part_s[b]; E += part_e[b]; n += part_n[b];
      }
      loss[f] = (float)(S / ((double)n * (double)F));              // n = 0: IEEE 0 / 0 = NaN
      if (state_err) state_err[f] = (float)(E / ((double)n * (double)d));
      count[f] = (int64_t)n;
    }
    fs[t] = S; fe[t] = E; fn[t] = n;
    __syncthreads();
    const int live = (int)(n_frames - base < 256 ? n_frames - base : 256);
    if (t == 0) { double a = tot_s; for (int j = 0; j < live; ++j) a += fs[j]; tot_s = a; }
    if (t == 64) { double a = tot_e; for (int j = 0; j < live; ++j) a += fe[j]; tot_e = a; }
    if (t == 128) { long long a = tot_n; for (int j = 0; j < live; ++j) a += fn[j]; tot_n = a; }
    __syncthreads();
  }
  if (t == 0) {
    loss[n_frames] = (float)(tot_s / ((double)tot_n * (double)F));
    if (state_err) state_err[n_frames] = (float)(tot_e / ((double)tot_n * (double)d));
    count[n_frames] = (int64_t)tot_n;
  }
}

// frame_losses_bwd_kernel with the row's frame found from frame_ptr: the same w, difference and product.
__global__ void frame_losses_ragged_bwd_kernel(const float* __restrict__ net_out, long ld_out, const float* __restrict__ target,
                                               long ld_tgt, int F, const int64_t* __restrict__ node_type, long ldt, unsigned free_mask,
                                               long rows, const int* __restrict__ frame_ptr, long n_frames,
                                               const int64_t* __restrict__ count, const float* __restrict__ g,
                                               float* __restrict__ d_net, long ld_dn, float* __restrict__ d_target, long ld_dt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const long r = i / F;
  const int c = (int)(i - r * F);
  const int64_t ty = node_type[r * ldt];
  const bool is_free = ty >= 0 && ty < 32 && ((free_mask >> (unsigned)ty) & 1u);
  float v = 0.f;
  if (is_free && g) {
    const long f = ragged_frame_of(frame_ptr, n_frames, r), B = n_frames;
    const float w = (float)((double)g[f] / ((double)count[f] * (double)F) + (double)g[B] / ((double)count[B] * (double)F));
    const float diff = net_out[r * ld_out + c] - target[r * ld_tgt + c];
    v = (2.f * diff) * w;
  }
  if (d_net) d_net[r * ld_dn + c] = v;
  if (d_target) d_target[r * ld_dt + c] = -v;
}

// Backward of the cluster mean of the connector (hierarchical_connector.py:39-45; rmp.py: `means_all = ...` in
// HierarchicalConnector.run) with respect to the node rows.  Node-parallel, flat over [rows, D]: thread (n, c) walks row n's own
// memberships q in [node_rowptr[n], node_rowptr[n+1]) in that order -- j = node_items[q] is a position of the member list, s =
// item_seg[j] its cluster -- and adds d_mean[s, c] / (float)count(s), the expression of seg_bwd_generic_kernel's HGN_OP_MEAN
// branch (segment.hip), so a partition of the rows gives that kernel's bits.  Every element is written exactly once, 0 for a row
// in no cluster (obstacle rows, noise, rows a sampling left out): no atomics, no LDS, no pre-zeroed output, equal bits on every run.
// Ids outside their ranges are skipped, never dereferenced.
__global__ void member_mean_bwd_kernel(const float* __restrict__ d_mean, long ld_dm, int D, const int* __restrict__ seg_rowptr,
                                       long S, const int* __restrict__ item_seg, const int* __restrict__ node_rowptr,
                                       const int* __restrict__ node_items, long rows, long M, float* __restrict__ d_data,
                                       long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * D) return;
  const long n = i / D;
  const int c = (int)(i - n * D);
  float g = 0.f;
  if (M > 0) {
    const int q0 = node_rowptr[n], q1 = node_rowptr[n + 1];
    for (int q = q0; q < q1; ++q) {
      if (q < 0 || q >= M) continue;
      const long j = node_items[q];
      if (j < 0 || j >= M) continue;
      const long s = item_seg[j];
      if (s < 0 || s >= S) continue;
      const int cnt = seg_rowptr[s + 1] - seg_rowptr[s];
      g += d_mean[s * ld_dm + c] / (float)(cnt > 0 ? cnt : 1);
    }
  }
  d_data[n * ld + c] = g;
}

// ----------------------------------------------------------------------------------------------------------
// world edges by radius: one wavefront per sender row, receivers in chunks of 64 (ballot keeps ascending order)
// ----------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void radius_edges_kernel(const float* __restrict__ pos, long ld, int d, const int64_t* __restrict__ node_type,
                                    long ldt, long N, float radius, int sender_type, int receiver_type,
                                    const int* __restrict__ nbr_rowptr, const int* __restrict__ nbr,
                                    int* __restrict__ counts, const int* __restrict__ offsets,
                                    int64_t* __restrict__ senders, int64_t* __restrict__ receivers) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= N) return;
  const bool active = sender_type < 0 || node_type[s * ldt] == sender_type;      // uniform per wave
  if (!active) { if (!FILL && lane == 0) counts[s] = 0; return; }
  float ps[3];
  for (int i = 0; i < 3; ++i) ps[i] = i < d ? pos[s * ld + i] : 0.f;
  const int nb0 = nbr_rowptr ? nbr_rowptr[s] : 0, nb1 = nbr_rowptr ? nbr_rowptr[s + 1] : 0;
  long base = FILL ? offsets[s] : 0;
  int total = 0;
  for (long r0 = 0; r0 < N; r0 += 64) {
    const long r = r0 + lane;
    bool hit = false;
    if (r < N && r != s && (receiver_type < 0 || node_type[r * ldt] == receiver_type)) {
      float q = 0.f;
      for (int i = 0; i < 3; ++i) {
        const float df = i < d ? ps[i] - pos[r * ld + i] : 0.f;
        q = q + df * df;
      }
      hit = sqrtf(q) < radius;
      if (hit)
        for (int k = nb0; k < nb1; ++k)
          if (nbr[k] == (int)r) { hit = false; break; }
    }
    const unsigned long long m = __ballot(hit);
    if (FILL && hit) {
      const int before = __popcll(m & ((1ULL << lane) - 1ULL));
      senders[base + before] = s;
      receivers[base + before] = r;
    }
    const int c = __popcll(m);
    base += c;
    total += c;
  }
  if (!FILL && lane == 0) counts[s] = total;
}

// The same query over the disjoint union of n_graphs graphs of N nodes each (rows = n_graphs * N): sender row s of graph
// b = s / N sweeps only the receivers [b*N, (b+1)*N) of its own graph, so the work is rows * N / 64 chunk iterations and no
// pair crosses a graph boundary.  The neighbour CSR is the one of a single mesh (local ids), shared by every graph.
template <bool FILL>
__global__ void radius_edges_batch_kernel(const float* __restrict__ pos, long ld, int d,
                                          const int64_t* __restrict__ node_type, long ldt, long rows, long N, float radius,
                                          int sender_type, int receiver_type, const int* __restrict__ nbr_rowptr,
                                          const int* __restrict__ nbr, int* __restrict__ counts,
                                          const int* __restrict__ offsets, int64_t* __restrict__ senders,
                                          int64_t* __restrict__ receivers) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= rows) return;
  const bool active = sender_type < 0 || node_type[s * ldt] == sender_type;      // uniform per wave
  if (!active) { if (!FILL && lane == 0) counts[s] = 0; return; }
  const long g0 = (s / N) * N;                       // first row of the sender's graph
  const long sl = s - g0;                            // local id: the row of the shared neighbour CSR
  float ps[3];
  for (int i = 0; i < 3; ++i) ps[i] = i < d ? pos[s * ld + i] : 0.f;
  const int nb0 = nbr_rowptr ? nbr_rowptr[sl] : 0, nb1 = nbr_rowptr ? nbr_rowptr[sl + 1] : 0;
  long base = FILL ? offsets[s] : 0;
  int total = 0;
  for (long r0 = 0; r0 < N; r0 += 64) {
    const long rl = r0 + lane;                       // local receiver id, < N checked before any read
    const long r = g0 + rl;
    bool hit = false;
    if (rl < N && r != s && (receiver_type < 0 || node_type[r * ldt] == receiver_type)) {
      float q = 0.f;
      for (int i = 0; i < 3; ++i) {
        const float df = i < d ? ps[i] - pos[r * ld + i] : 0.f;
        q = q + df * df;
      }
      hit = sqrtf(q) < radius;
      if (hit)
        for (int k = nb0; k < nb1; ++k)
          if (nbr[k] == (int)rl) { hit = false; break; }
    }
    const unsigned long long m = __ballot(hit);
    if (FILL && hit) {
      const int before = __popcll(m & ((1ULL << lane) - 1ULL));
      senders[base + before] = s;
      receivers[base + before] = r;
    }
    const int c = __popcll(m);
    base += c;
    total += c;
  }
  if (!FILL && lane == 0) counts[s] = total;
}

// graph_offsets[b] = offsets[b * N] for b = 0 .. n_graphs (the last entry is the total)
__global__ void graph_offsets_kernel(const int* __restrict__ offsets, long n_graphs, long N, int* __restrict__ graph_offsets) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > n_graphs) return;
  graph_offsets[b] = offsets[b * N];
}

// The same query over the disjoint union of graphs of different sizes: sender row s finds its graph b from frame_ptr (uniform per
// wave) and sweeps only the receivers [frame_ptr[b], frame_ptr[b+1]) -- sum_b N_b^2 / 64 chunk iterations, and no pair crosses a
// graph boundary.  Every graph has its own mesh: the neighbour CSR is that of the union, rows and entries in union ids.
template <bool FILL>
__global__ void radius_edges_ragged_kernel(const float* __restrict__ pos, long ld, int d,
                                           const int64_t* __restrict__ node_type, long ldt, long rows,
                                           const int* __restrict__ frame_ptr, long n_graphs, float radius, int sender_type,
                                           int receiver_type, const int* __restrict__ nbr_rowptr, const int* __restrict__ nbr,
                                           int* __restrict__ counts, const int* __restrict__ offsets,
                                           int64_t* __restrict__ senders, int64_t* __restrict__ receivers) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= rows) return;
  const bool active = sender_type < 0 || node_type[s * ldt] == sender_type;      // uniform per wave
  if (!active) { if (!FILL && lane == 0) counts[s] = 0; return; }
  const long b = ragged_frame_of(frame_ptr, n_graphs, s);
  const long g0 = ragged_bound(frame_ptr, b, rows), g1 = ragged_bound(frame_ptr, b + 1, rows);   // the sender's graph, inside [0, rows]
  float ps[3];
  for (int i = 0; i < 3; ++i) ps[i] = i < d ? pos[s * ld + i] : 0.f;
  const int nb0 = nbr_rowptr ? nbr_rowptr[s] : 0, nb1 = nbr_rowptr ? nbr_rowptr[s + 1] : 0;
  long base = FILL ? offsets[s] : 0;
  int total = 0;
  for (long r0 = g0; r0 < g1; r0 += 64) {
    const long r = r0 + lane;                        // union id of the receiver, < g1 <= rows checked before any read
    bool hit = false;
    if (r < g1 && r != s && (receiver_type < 0 || node_type[r * ldt] == receiver_type)) {
      float q = 0.f;
      for (int i = 0; i < 3; ++i) {
        const float df = i < d ? ps[i] - pos[r * ld + i] : 0.f;
        q = q + df * df;
      }
      hit = sqrtf(q) < radius;
      if (hit)
        for (int k = nb0; k < nb1; ++k)
          if (nbr[k] == (int)r) { hit = false; break; }
    }
    const unsigned long long m = __ballot(hit);
    if (FILL && hit) {
      const int before = __popcll(m & ((1ULL << lane) - 1ULL));
      senders[base + before] = s;
      receivers[base + before] = r;
    }
    const int c = __popcll(m);
    base += c;
    total += c;
  }
  if (!FILL && lane == 0) counts[s] = total;
}

// graph_offsets[b] = offsets[frame_ptr[b]] for b = 0 .. n_graphs (the last entry is the total)
__global__ void graph_offsets_ragged_kernel(const int* __restrict__ offsets, const int* __restrict__ frame_ptr, long n_graphs,
                                            long rows, int* __restrict__ graph_offsets) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > n_graphs) return;
  graph_offsets[b] = offsets[ragged_bound(frame_ptr, b, rows)];
}

// ----------------------------------------------------------------------------------------------------------
// balanced Forman curvature (SDRF): one wavefront per edge / per candidate pair
// ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_count_max(int& cnt, float& mx) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
}

// closed form of ricci.py:185-191 / 256-262 in the reference kernel's typing: fp64 expression, fp32 stores
__device__ __forceinline__ float forman_value(double dmax, double dmin, double a2, double a, int sharp, double lam) {
  float c = (float)(((2 / dmax) + (2 / dmin) - 2) + (2 / dmax + 1 / dmin) * a2 * a);
  if (lam > 0) c = (float)((double)c + (double)sharp / (dmax * lam));
  return c;
}

__global__ void forman_curvature_kernel(const float* __restrict__ A, const float* __restrict__ A2,
                                        const float* __restrict__ d_in, const float* __restrict__ d_out, long N,
                                        const int* __restrict__ ei, const int* __restrict__ ej, long nnz,
                                        float* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (e >= nnz) return;
  const long i = ei[e], j = ej[e];
  const float aij = A[i * N + j];
  if (aij == 0.f) { if (lane == 0) C[i * N + j] = 0.f; return; }
  const float di = d_in[i], dj = d_out[j];
  const float dmax = di > dj ? di : dj, dmin = di > dj ? dj : di;
  if (dmax * dmin == 0.f) { if (lane == 0) C[i * N + j] = 0.f; return; }
  int cnt = 0;
  float mx = 0.f;
  for (long k = lane; k < N; k += 64) {
    const float aik = A[i * N + k], akj = A[k * N + j];
    const float t1 = akj * (A2[i * N + k] - aik) * aij;
    const float t2 = aik * (A2[k * N + j] - akj) * aij;
    if (t1 > 0.f) { ++cnt; mx = fmaxf(mx, t1); }
    if (t2 > 0.f) { ++cnt; mx = fmaxf(mx, t2); }
  }
  wave_count_max(cnt, mx);
  if (lane == 0) C[i * N + j] = forman_value(dmax, dmin, A2[i * N + j], aij, cnt, mx);
}

__global__ void forman_post_delta_kernel(const float* __restrict__ A, const float* __restrict__ A2, float d_in_x0,
                                         float d_out_y0, long N, int x, int y, const int* __restrict__ i_nb, int dim_i,
                                         const int* __restrict__ j_nb, int dim_j, float* __restrict__ D) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= (long)dim_i * dim_j) return;
  const int I = (int)(p / dim_j), J = (int)(p % dim_j);
  const long i = i_nb[I], j = j_nb[J];
  if (i == j || A[i * N + j] != 0.f) { if (lane == 0) D[p] = -1000.f; return; }
  double dx = d_in_x0, dy = d_out_y0;
  if (j == x) dx += 1; else if (i == y) dy += 1;
  if (dx * dy == 0) { if (lane == 0) D[p] = 0.f; return; }
  const double dmax = dx > dy ? dx : dy, dmin = dx > dy ? dy : dx;
  const float axy = A[(long)x * N + y];
  double a2xy = A2[(long)x * N + y];
  if (x == i && A[j * N + y] != 0.f) a2xy += A[j * N + y];
  else if (y == j && A[(long)x * N + i] != 0.f) a2xy += A[(long)x * N + i];
  const float ajy = A[j * N + y], axi = A[(long)x * N + i];
  int cnt = 0;
  float mx = 0.f;
  for (long z = lane; z < N; z += 64) {
    float azy = A[z * N + y], axz = A[(long)x * N + z];
    float a2zy = A2[z * N + y], a2xz = A2[(long)x * N + z];
    if (z == i && y == j) azy += 1.f;
    if (x == i && z == j) axz += 1.f;
    if (z == i && ajy != 0.f) a2zy += ajy;
    if (x == i && A[j * N + z] != 0.f) a2xz += A[j * N + z];
    if (y == j && A[z * N + i] != 0.f) a2zy += A[z * N + i];
    if (z == j && axi != 0.f) a2xz += axi;
    const float t1 = azy * (a2xz - axz) * axy;          // small integers: exact in fp32
    const float t2 = axz * (a2zy - azy) * axy;
    if (t1 > 0.f) { ++cnt; mx = fmaxf(mx, t1); }
    if (t2 > 0.f) { ++cnt; mx = fmaxf(mx, t2); }
  }
  wave_count_max(cnt, mx);
  if (lane == 0) D[p] = forman_value(dmax, dmin, a2xy, axy, cnt, mx);
}

// ----------------------------------------------------------------------------------------------------------
// backward of the feature kernels (the statistics of the normaliser are constants: nothing flows into them)
// ----------------------------------------------------------------------------------------------------------
// Relative-position features.  With u = a[s]-a[r] the gradient of u is g = d_feat[0:da] + (d_feat[da] + d_len) * u/|u|
// (the norm term is dropped where |u| = 0); node s receives +g, node r receives -g.  Parallel over NODES: a node walks
// its outgoing edges (CSR by sender), then its incoming ones (CSR by receiver), in CSR order, and writes its row once:
// no atomics, the same bits on every run.  Per edge it reads the edge id, the other end's id and row and 8-32 bytes
// of d_feat -- gathered, so the pass is bound by memory latency: a thread per node while a node has few edges (a mesh
// node has ~12), a wavefront per node above REL_BWD_WAVE_DEG (lanes stride over the edge list, xor-butterfly sum).
constexpr int REL_BWD_WAVE_DEG = 32;

struct RelBwd {
  const float *a, *b, *d_feat, *d_len;
  long lda, ldb, ldf;
  int da, db;
  long n_rows, E;
  const int64_t *snd, *rcv;
  const int *rp_s, *perm_s, *rp_r, *perm_r;
  float *d_a, *d_b;
};

__device__ __forceinline__ int clamp_ptr(int v, long E) { return v < 0 ? 0 : (v > E ? (int)E : v); }

// position k of the sender (out = true) or receiver CSR of node n: adds the edge's share to ga / gb
__device__ __forceinline__ void rel_bwd_edge(const RelBwd& p, const float* an, const float* bn, int k, bool out, float* ga,
                                             float* gb) {
  const long e = out ? p.perm_s[k] : p.perm_r[k];
  if (e < 0 || e >= p.E) return;
  const int64_t o = out ? p.rcv[e] : p.snd[e];
  if (o < 0 || o >= p.n_rows) return;
  const float sg = out ? 1.f : -1.f;
  const float* df = p.d_feat ? p.d_feat + e * p.ldf : nullptr;
  if (p.d_a) {
    float u[3], q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float ao = i < p.da ? p.a[o * p.lda + i] : 0.f;
      u[i] = i < p.da ? (out ? an[i] - ao : ao - an[i]) : 0.f;      // a[s] - a[r], as the forward forms it
      q += u[i] * u[i];
    }
    const float c = (df ? df[p.da] : 0.f) + (p.d_len ? p.d_len[e] : 0.f);
    const float nrm = sqrtf(q);
    const float w = nrm > 0.f ? c / nrm : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i < p.da) ga[i] += sg * ((df ? df[i] : 0.f) + w * u[i]);
  }
  if (p.d_b && df) {
    const float* dg = df + p.da + 1;
    float u[3], q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float bo = i < p.db ? p.b[o * p.ldb + i] : 0.f;
      u[i] = i < p.db ? (out ? bn[i] - bo : bo - bn[i]) : 0.f;
      q += u[i] * u[i];
    }
    const float nrm = sqrtf(q);
    const float w = nrm > 0.f ? dg[p.db] / nrm : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i < p.db) gb[i] += sg * (dg[i] + w * u[i]);
  }
}

__device__ __forceinline__ void rel_bwd_own_rows(const RelBwd& p, long n, float* an, float* bn) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    an[i] = (p.d_a && i < p.da) ? p.a[n * p.lda + i] : 0.f;
    bn[i] = (p.d_b && i < p.db) ? p.b[n * p.ldb + i] : 0.f;
  }
}

// split != 0: rows of more than REL_BWD_WAVE_DEG edges are left to rel_edge_bwd_wave_kernel
__global__ void rel_edge_bwd_thread_kernel(RelBwd p, int split) {
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.n_rows) return;
  const int s0 = clamp_ptr(p.rp_s[n], p.E), s1 = clamp_ptr(p.rp_s[n + 1], p.E);
  const int r0 = clamp_ptr(p.rp_r[n], p.E), r1 = clamp_ptr(p.rp_r[n + 1], p.E);
  if (split && (long)(s1 - s0) + (r1 - r0) > REL_BWD_WAVE_DEG) return;
  float an[3], bn[3], ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
  rel_bwd_own_rows(p, n, an, bn);
  for (int k = s0; k < s1; ++k) rel_bwd_edge(p, an, bn, k, true, ga, gb);
  for (int k = r0; k < r1; ++k) rel_bwd_edge(p, an, bn, k, false, ga, gb);
  if (p.d_a)
    for (int i = 0; i < p.da; ++i) p.d_a[n * p.da + i] = ga[i];
  if (p.d_b)
    for (int i = 0; i < p.db; ++i) p.d_b[n * p.db + i] = gb[i];
}

// one wavefront per row of more than REL_BWD_WAVE_DEG edges (the other rows belong to the thread kernel)
__global__ void rel_edge_bwd_wave_kernel(RelBwd p) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n >= p.n_rows) return;
  const int s0 = clamp_ptr(p.rp_s[n], p.E), s1 = clamp_ptr(p.rp_s[n + 1], p.E);
  const int r0 = clamp_ptr(p.rp_r[n], p.E), r1 = clamp_ptr(p.rp_r[n + 1], p.E);
  const long n_out = s1 > s0 ? s1 - s0 : 0, n_in = r1 > r0 ? r1 - r0 : 0;
  if (n_out + n_in <= REL_BWD_WAVE_DEG) return;                  // uniform per wave
  float an[3], bn[3], ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
  rel_bwd_own_rows(p, n, an, bn);
  for (long j = lane; j < n_out + n_in; j += 64) {               // outgoing edges first, then incoming, lane-strided
    if (j < n_out) rel_bwd_edge(p, an, bn, s0 + (int)j, true, ga, gb);
    else rel_bwd_edge(p, an, bn, r0 + (int)(j - n_out), false, ga, gb);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)                              // fixed pairing: deterministic
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ga[i] += __shfl_xor(ga[i], o);
      gb[i] += __shfl_xor(gb[i], o);
    }
  if (lane == 0) {
    if (p.d_a)
      for (int i = 0; i < p.da; ++i) p.d_a[n * p.da + i] = ga[i];
    if (p.d_b)
      for (int i = 0; i < p.db; ++i) p.d_b[n * p.db + i] = gb[i];
  }
}

// node features: the velocity columns pass +d to cur and -d to prev (zero on rows the forward masked); flat over [N, d]
__global__ void node_feat_bwd_kernel(const float* __restrict__ d_out, long ldo, int d, int n_classes, int vel_first,
                                     const int64_t* __restrict__ node_type, long ldt, int vel_mask_type, long N,
                                     float* __restrict__ d_cur, float* __restrict__ d_prev) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * d) return;
  const long n = i / d;
  const int c = (int)(i - n * d);
  float g = d_out[n * ldo + (vel_first ? c : c + n_classes)];
  if (vel_mask_type >= 0 && node_type[n * ldt] != vel_mask_type) g = 0.f;
  if (d_cur) d_cur[i] = g;
  if (d_prev) d_prev[i] = -g;
}

__global__ void normalize_bwd_kernel(const float* __restrict__ d_out, long n_elem, int F, const float* __restrict__ acc_sum,
                                     const float* __restrict__ acc_sumsq, const float* __restrict__ acc_count, float eps,
                                     int inverse, float* __restrict__ d_x) {
  __shared__ float sd[HGN_MAX_FEATURE_WIDTH];
  if ((int)threadIdx.x < F) {                                   // the std of normalize_kernel, op for op
    const float safe = fmaxf(*acc_count, 1.f);
    const float m = acc_sum[threadIdx.x] / safe;
    const float s = sqrtf(fabsf(acc_sumsq[threadIdx.x] / safe - m * m));
    sd[threadIdx.x] = fmaxf(s, eps);
  }
  __syncthreads();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_elem) return;
  const int c = (int)(i % F);
  d_x[i] = inverse ? d_out[i] * sd[c] : d_out[i] / sd[c];
}

static int stats_blocks(int64_t rows, int F, int* active) {
  *active = (ST / F) * F;
  const int64_t n = rows * F;
  int64_t nb = (n + (int64_t)(*active) * 16 - 1) / ((int64_t)(*active) * 16);
  if (nb < 1) nb = 1;
  if (nb > MAXBLK) nb = MAXBLK;
  return (int)nb;
}

}  // namespace hgn

using namespace hgn;

static size_t cells_cub_bytes(int64_t n) {
  size_t t1 = 0, t2 = 0;
  (void)hipcub::DeviceRadixSort::SortKeys<unsigned long long>(nullptr, t1, nullptr, nullptr, (int)n, 0, 64);
  (void)hipcub::DeviceSelect::Unique<unsigned long long*, unsigned long long*, int*>(nullptr, t2, nullptr, nullptr, nullptr, (int)n);
  return t1 > t2 ? t1 : t2;
}

extern "C" int hgn_cells_to_edges_workspace_bytes(int64_t n_cells, int verts, size_t* bytes) {
  if (!bytes || n_cells < 0 || (verts != 3 && verts != 4) || n_cells * verts > 0x7fffffff)
    return hgn_fail(HGN_E_INVALID, "hgn_cells_to_edges_workspace_bytes: bad size (verts must be 3 or 4)");
  const int64_t n = n_cells * verts;
  *bytes = 256 + 3 * up256((size_t)n * 8) + up256(cells_cub_bytes(n)) + 256;
  return HGN_OK;
}

extern "C" int hgn_cells_to_edges(const int64_t* cells, int64_t n_cells, int verts, int64_t* senders, int64_t* receivers,
                                  int64_t* n_unique, void* workspace, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  size_t need = 0;
  if (hgn_cells_to_edges_workspace_bytes(n_cells, verts, &need) != HGN_OK) return HGN_E_INVALID;
  if (!n_unique || !workspace || ws_bytes < need || (n_cells > 0 && (!cells || !senders || !receivers)))
    return hgn_fail(HGN_E_INVALID, "hgn_cells_to_edges: null pointer or workspace too small");
  *n_unique = 0;
  if (n_cells == 0) return HGN_OK;
  ProfScope ps(13, (double)n_cells, stream);
  const int64_t n = n_cells * verts;
  char* w = (char*)workspace;
  int* flag = (int*)w;                   // [0] range flag, [1] number of unique keys
  unsigned long long* k0 = (unsigned long long*)(w + 256);
  unsigned long long* k1 = (unsigned long long*)(w + 256 + up256((size_t)n * 8));
  unsigned long long* k2 = (unsigned long long*)(w + 256 + 2 * up256((size_t)n * 8));
  void* temp = w + 256 + 3 * up256((size_t)n * 8);
  size_t temp_bytes = cells_cub_bytes(n);
  if (hipMemsetAsync(flag, 0, 16, stream) != hipSuccess) return hgn_check_launch("hgn_cells_to_edges memset");
  hipLaunchKernelGGL(cell_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cells, (long)n_cells, verts,
                     k0, flag);
  size_t tb = temp_bytes;
  if (hipcub::DeviceRadixSort::SortKeys<unsigned long long>(temp, tb, k0, k1, (int)n, 0, 64, stream) != hipSuccess)
    return hgn_check_launch("hgn_cells_to_edges sort");
  tb = temp_bytes;
  if (hipcub::DeviceSelect::Unique(temp, tb, k1, k2, flag + 1, (int)n, stream) != hipSuccess)
    return hgn_check_launch("hgn_cells_to_edges unique");
  hipLaunchKernelGGL(two_way_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, k2, flag + 1, senders,
                     receivers);
  int host[2] = {0, 0};
  if (hipMemcpyAsync(host, flag, 2 * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return hgn_check_launch("hgn_cells_to_edges readback");
  if (host[0]) return hgn_fail(HGN_E_RANGE, "hgn_cells_to_edges: vertex id outside [0, 2^31)");
  *n_unique = host[1];
  return hgn_check_launch("hgn_cells_to_edges");
}

extern "C" int hgn_rel_edge_features(const float* a, int64_t lda, int da, const float* b, int64_t ldb, int db,
                                     int64_t n_rows, const int64_t* senders, const int64_t* receivers, int64_t E,
                                     float* feat, int64_t ldf, float* len_a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (E < 0 || n_rows < 0 || da < 1 || da > 3 || db < 0 || db > 3 || lda < da || (db > 0 && ldb < db))
    return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features: widths must satisfy 1<=da<=3, 0<=db<=3, ld >= width");
  const int W = da + 1 + (db > 0 ? db + 1 : 0);
  if (feat && ldf < W) return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features: ldf smaller than the feature row");
  if (E == 0) return HGN_OK;
  if (!a || (db > 0 && !b) || !senders || !receivers || (!feat && !len_a))
    return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features: null pointer");
  ProfScope ps(13, (double)E, stream);
  hipLaunchKernelGGL(rel_edge_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, a, (long)lda, da, b,
                     (long)ldb, db, (long)n_rows, senders, receivers, (long)E, feat, (long)ldf, len_a);
  return hgn_check_launch("hgn_rel_edge_features");
}

extern "C" int hgn_node_features(const float* cur, const float* prev, int64_t ld, int d, const int64_t* node_type,
                                 int64_t ldt, const int32_t* map, int map_len, int n_classes, int vel_first,
                                 int vel_mask_type, int64_t N, float* out, int64_t ldo, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 0 || d < 0 || n_classes < 0 || d + n_classes < 1 || d + n_classes > HGN_MAX_FEATURE_WIDTH || ldo < d + n_classes ||
      (cur && ld < d) || ldt < 1 || (map && map_len < 1))
    return hgn_fail(HGN_E_INVALID, "hgn_node_features: bad widths / strides");
  if (N == 0) return HGN_OK;
  if (!node_type || !out || (prev && !cur)) return hgn_fail(HGN_E_INVALID, "hgn_node_features: null pointer");
  ProfScope ps(13, (double)N, stream);
  const int64_t n = N * (d + n_classes);
  hipLaunchKernelGGL(node_feat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cur, prev, (long)ld, d,
                     node_type, (long)ldt, map, map_len, n_classes, vel_first, vel_mask_type, (long)N, out, (long)ldo);
  return hgn_check_launch("hgn_node_features");
}

extern "C" int hgn_col_stats_workspace_bytes(int64_t rows, int F, size_t* bytes) {
  if (!bytes || rows < 0 || F < 1 || F > HGN_MAX_FEATURE_WIDTH)
    return hgn_fail(HGN_E_INVALID, "hgn_col_stats_workspace_bytes: bad size (1 <= F <= 32)");
  *bytes = (size_t)MAXBLK * 2 * F * sizeof(double);
  return HGN_OK;
}

extern "C" int hgn_col_stats(const float* x, int64_t rows, int F, float* batch, void* workspace, size_t ws_bytes,
                             void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  size_t need = 0;
  if (hgn_col_stats_workspace_bytes(rows, F, &need) != HGN_OK) return HGN_E_INVALID;
  if (!batch || !workspace || ws_bytes < need || (rows > 0 && !x))
    return hgn_fail(HGN_E_INVALID, "hgn_col_stats: null pointer or workspace too small");
  ProfScope ps(13, (double)rows, stream);
  int active = 0;
  const int nblk = stats_blocks(rows, F, &active);
  hipLaunchKernelGGL(col_stats_kernel, dim3(nblk), dim3(ST), 0, stream, x, (long)(rows * F), F, active, (double*)workspace);
  hipLaunchKernelGGL(col_stats_final_kernel, dim3(1), dim3(ST), 0, stream, (const double*)workspace, nblk, F, batch);
  return hgn_check_launch("hgn_col_stats");
}

extern "C" int hgn_normalizer_update(float* acc_sum, float* acc_sumsq, float* acc_count, float* num_acc,
                                     const float* batch, const float* count, int F, float max_acc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || !acc_sum || !acc_sumsq || !acc_count || !num_acc || !batch || !count)
    return hgn_fail(HGN_E_INVALID, "hgn_normalizer_update: null pointer or bad width");
  hipLaunchKernelGGL(normalizer_update_kernel, dim3(1), dim3(64), 0, stream, acc_sum, acc_sumsq, acc_count, num_acc, batch,
                     count, F, max_acc);
  return hgn_check_launch("hgn_normalizer_update");
}

extern "C" int hgn_normalize(const float* x, int64_t rows, int F, const float* acc_sum, const float* acc_sumsq,
                             const float* acc_count, float eps, int inverse, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (rows < 0 || F < 1 || F > HGN_MAX_FEATURE_WIDTH || !acc_sum || !acc_sumsq || !acc_count)
    return hgn_fail(HGN_E_INVALID, "hgn_normalize: null pointer or bad width");
  if (rows == 0) return HGN_OK;
  if (!x || !out) return hgn_fail(HGN_E_INVALID, "hgn_normalize: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, (long)n, F, acc_sum,
                     acc_sumsq, acc_count, eps, inverse, out);
  return hgn_check_launch("hgn_normalize");
}

extern "C" int hgn_lincomb3(const float* a, float ca, const float* b, float cb, const float* c, float cc, int64_t n,
                            float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0) return hgn_fail(HGN_E_INVALID, "hgn_lincomb3: negative size");
  if (n == 0) return HGN_OK;
  if (!a || !b || !out) return hgn_fail(HGN_E_INVALID, "hgn_lincomb3: null pointer");
  hipLaunchKernelGGL(lincomb3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, ca, b, cb, c, cc, (long)n,
                     out);
  return hgn_check_launch("hgn_lincomb3");
}

extern "C" int hgn_rollout_advance(const float* net_out, int64_t ld_out, int out_cols, int F, const float* acc_sum,
                                   const float* acc_sumsq, const float* acc_count, float eps, const float* cur, int64_t ld_cur,
                                   int d, float ca, const float* prev, int64_t ld_prev, float cp, const int64_t* node_type,
                                   int64_t ldt, uint32_t free_mask, const float* fallback, int64_t ld_fb, int64_t rows,
                                   float* next, int64_t ld_next, float* rec, int64_t ld_rec, int rec_before, float* prev_out,
                                   int64_t ld_po, float* inv, int64_t ld_inv, int inv_from, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || !acc_sum || !acc_sumsq || !acc_count)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance: null pointer or bad width");
  if (out_cols != F)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance: the network output's column count does not match the normaliser width");
  if (rows < 0 || rows > 0x7fffffff || d < 1 || d > F || inv_from < 0 || inv_from > F)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance: bad sizes (0 <= rows < 2^31, 1 <= d <= F, 0 <= inv_from <= F)");
  if (ld_out < F || ld_cur < d || ld_next < d || ldt < 1 || (prev && ld_prev < d) || (fallback && ld_fb < d) ||
      (rec && ld_rec < d) || (prev_out && ld_po < d) || (inv && ld_inv < F - inv_from) || (inv && ld_inv < 1))
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance: bad widths / strides (a row stride is zero or smaller than its row)");
  if (rows == 0) return HGN_OK;
  if (!net_out || !cur || !node_type || !next) return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(rollout_advance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, net_out, (long)ld_out, F,
                     acc_sum, acc_sumsq, acc_count, eps, cur, (long)ld_cur, d, ca, prev, (long)ld_prev, cp, node_type, (long)ldt,
                     (unsigned)free_mask, fallback, (long)ld_fb, (long)rows, next, (long)ld_next, rec, (long)ld_rec, rec_before,
                     prev_out, (long)ld_po, inv, (long)ld_inv, inv_from);
  return hgn_check_launch("hgn_rollout_advance");
}

extern "C" int hgn_rollout_advance_bwd(const float* d_next, int64_t ld_dnext, const float* d_inv, int64_t ld_dinv, int inv_from,
                                       int F, const float* acc_sum, const float* acc_sumsq, const float* acc_count, float eps,
                                       int d, float ca, float cp, const int64_t* node_type, int64_t ldt, uint32_t free_mask,
                                       int has_fallback, int64_t rows, float* d_net, int64_t ld_dnet, float* d_cur,
                                       int64_t ld_dcur, float* d_prev, int64_t ld_dprev, float* d_fallback, int64_t ld_dfb,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || !acc_sum || !acc_sumsq || !acc_count)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance_bwd: null pointer or bad width");
  if (rows < 0 || rows > 0x7fffffff || d < 1 || d > F || inv_from < 0 || inv_from > F)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance_bwd: bad sizes (0 <= rows < 2^31, 1 <= d <= F, 0 <= inv_from <= F)");
  if (ldt < 1 || (d_next && ld_dnext < d) || (d_inv && ld_dinv < F - inv_from) || (d_inv && ld_dinv < 1) ||
      (d_net && ld_dnet < F) || (d_cur && ld_dcur < d) || (d_prev && ld_dprev < d) || (d_fallback && ld_dfb < d))
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance_bwd: bad widths / strides (a row stride is zero or smaller than its row)");
  if (!d_net && !d_cur && !d_prev && !d_fallback)
    return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance_bwd: no output asked for (d_net, d_cur, d_prev and d_fallback are all null)");
  if (rows == 0) return HGN_OK;
  if (!node_type) return hgn_fail(HGN_E_INVALID, "hgn_rollout_advance_bwd: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(rollout_advance_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_next, (long)ld_dnext,
                     d_inv, (long)ld_dinv, inv_from, F, acc_sum, acc_sumsq, acc_count, eps, d, ca, cp, node_type, (long)ldt,
                     (unsigned)free_mask, has_fallback, (long)rows, d_net, (long)ld_dnet, d_cur, (long)ld_dcur, d_prev,
                     (long)ld_dprev, d_fallback, (long)ld_dfb);
  return hgn_check_launch("hgn_rollout_advance_bwd");
}

extern "C" int hgn_training_noise(const float* x, int64_t ldx, int d, const int64_t* node_type, int64_t ldt, uint32_t free_mask,
                                  int64_t rows, int64_t rows_per_frame, const int64_t* frame_ids, uint64_t seed, uint64_t draw,
                                  float std_, const float* target, int64_t ld_tgt, float target_scale, float* out_x, int64_t ld_ox,
                                  float* out_target, int64_t ld_ot, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (d < 1 || d > 4 || rows < 0 || rows > 0x7fffffff || rows_per_frame < 1 || rows % rows_per_frame != 0)
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise: bad sizes (1 <= d <= 4, 0 <= rows < 2^31, rows_per_frame >= 1 and divides rows)");
  if ((target == nullptr) != (out_target == nullptr))
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise: target and out_target must both be given or both be null");
  if (ldx < d || ld_ox < d || ldt < 1 || (target && (ld_tgt < d || ld_ot < d)))
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (!(std_ >= 0.f) || std_ > 3.4028234e38f)
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise: the standard deviation must be finite and not negative");
  if (rows == 0) return HGN_OK;
  if (!x || !node_type || !out_x) return hgn_fail(HGN_E_INVALID, "hgn_training_noise: null pointer");
  ProfScope ps(13, (double)rows, stream);
  hipLaunchKernelGGL(training_noise_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, x, (long)ldx, d, node_type,
                     (long)ldt, (unsigned)free_mask, (long)rows, (long)rows_per_frame, frame_ids, (unsigned)(seed & 0xffffffffu),
                     (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32), std_, target, (long)ld_tgt,
                     target_scale, out_x, (long)ld_ox, out_target, (long)ld_ot);
  return hgn_check_launch("hgn_training_noise");
}

// -> the number of chunks (= workgroups of the partial pass) of rows / rows_per_frame frames, or -1 for sizes the entries refuse
static int64_t loss_chunks(int64_t rows, int64_t rows_per_frame, int64_t* chunks_per_frame) {
  if (rows < 0 || rows > 0x7fffffff || rows_per_frame < 1 || rows % rows_per_frame != 0) return -1;
  *chunks_per_frame = (rows_per_frame + HGN_LOSS_CHUNK_ROWS - 1) / HGN_LOSS_CHUNK_ROWS;
  return (rows / rows_per_frame) * *chunks_per_frame;
}

extern "C" int hgn_frame_losses_workspace_bytes(int64_t rows, int64_t rows_per_frame, size_t* bytes) {
  int64_t cpf = 0;
  const int64_t chunks = loss_chunks(rows, rows_per_frame, &cpf);
  if (!bytes || chunks < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_workspace_bytes: bad sizes (0 <= rows < 2^31, rows_per_frame >= 1 and divides rows)");
  *bytes = (size_t)chunks * 3 * sizeof(double);
  return HGN_OK;
}

extern "C" int hgn_frame_losses(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                                const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows, int64_t rows_per_frame,
                                const float* acc_sum, const float* acc_sumsq, const float* acc_count, float eps, const float* cur,
                                int64_t ld_cur, int d, float ca, const float* prev, int64_t ld_prev, float cp,
                                const float* state_target, int64_t ld_st, float* loss, float* state_err, int64_t* count,
                                void* workspace, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int64_t cpf = 0;
  const int64_t chunks = loss_chunks(rows, rows_per_frame, &cpf);
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || chunks < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: bad sizes (1 <= F <= 32, 0 <= rows < 2^31, rows_per_frame >= 1 and divides rows)");
  const int given = (acc_sum != nullptr) + (acc_sumsq != nullptr) + (acc_count != nullptr) + (cur != nullptr) + (state_target != nullptr);
  if ((given != 0 && given != 5) || (given == 0 && prev))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: the state part (statistics, cur, state_target; prev optional) must be given whole or not at all");
  const bool with_state = given == 5;
  if (with_state != (state_err != nullptr))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: state_err must be given exactly when the state part is");
  if (with_state && (d < 1 || d > F)) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: bad state width (1 <= d <= F)");
  if (ld_out < F || ld_tgt < F || ldt < 1 || (with_state && (ld_cur < d || ld_st < d || (prev && ld_prev < d))))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (rows == 0) return HGN_OK;
  if (!net_out || !target || !node_type || !loss || !count) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: null pointer");
  if (!workspace || ((uintptr_t)workspace & 7)) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: null or misaligned workspace");
  if (ws_bytes < (size_t)chunks * 3 * sizeof(double))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses: workspace too small (hgn_frame_losses_workspace_bytes)");
  ProfScope ps(13, (double)rows, stream);
  double* part_s = (double*)workspace;
  double* part_e = part_s + chunks;
  long long* part_n = (long long*)(part_e + chunks);
  hipLaunchKernelGGL(frame_losses_partial_kernel, dim3((unsigned)chunks), dim3(HGN_LOSS_CHUNK_ROWS), 0, stream, net_out, (long)ld_out,
                     target, (long)ld_tgt, F, node_type, (long)ldt, (unsigned)free_mask, (long)rows_per_frame, (long)cpf, acc_sum,
                     acc_sumsq, acc_count, eps, cur, (long)ld_cur, d, ca, prev, (long)ld_prev, cp, state_target, (long)ld_st, part_s,
                     part_e, part_n);
  hipLaunchKernelGGL(frame_losses_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)part_s, (const double*)part_e,
                     (const long long*)part_n, (long)(rows / rows_per_frame), (long)cpf, F, with_state ? d : 1, loss, state_err, count);
  return hgn_check_launch("hgn_frame_losses");
}

extern "C" int hgn_frame_losses_bwd(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                                    const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows, int64_t rows_per_frame,
                                    const int64_t* count, const float* g, float* d_net, int64_t ld_dnet, float* d_target,
                                    int64_t ld_dtgt, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int64_t cpf = 0;
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || loss_chunks(rows, rows_per_frame, &cpf) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_bwd: bad sizes (1 <= F <= 32, 0 <= rows < 2^31, rows_per_frame >= 1 and divides rows)");
  if (ld_out < F || ld_tgt < F || ldt < 1 || (d_net && ld_dnet < F) || (d_target && ld_dtgt < F))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_bwd: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (!d_net && !d_target) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_bwd: no output asked for (d_net and d_target are both null)");
  if (rows == 0) return HGN_OK;
  if (!net_out || !target || !node_type || !count) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_bwd: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(frame_losses_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, net_out, (long)ld_out, target,
                     (long)ld_tgt, F, node_type, (long)ldt, (unsigned)free_mask, (long)rows, (long)rows_per_frame, count, g, d_net,
                     (long)ld_dnet, d_target, (long)ld_dtgt);
  return hgn_check_launch("hgn_frame_losses_bwd");
}

// The host half of a ragged batch: -> the largest frame, or -1 when the array is refused (null, n_frames < 1, an entry < 1, a sum
// that differs from rows, rows > max_rows).  Every ragged entry calls it before it launches anything.
static int64_t ragged_max_rows(int64_t rows, const int64_t* frame_rows, int64_t n_frames, int64_t max_rows) {
  if (!frame_rows || n_frames < 1 || rows < 1 || rows > max_rows || n_frames > rows) return -1;
  int64_t sum = 0, largest = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    const int64_t n = frame_rows[f];
    if (n < 1 || n > rows - sum) return -1;
    sum += n;
    if (n > largest) largest = n;
  }
  return sum == rows ? largest : -1;
}

#define HGN_RAGGED_SIZES "0 < rows < 2^31, n_frames >= 1, every frame_rows[f] >= 1, their sum = rows, frame_rows and frame_ptr not null"

// -> the workgroups of the partial pass (n_frames * the chunks of the largest frame), or -1 for what the entries refuse
static int64_t ragged_loss_chunks(int64_t rows, const int64_t* frame_rows, int64_t n_frames, int64_t* max_chunks) {
  const int64_t largest = ragged_max_rows(rows, frame_rows, n_frames, 0x7fffffff);
  if (largest < 0) return -1;
  *max_chunks = (largest + HGN_LOSS_CHUNK_ROWS - 1) / HGN_LOSS_CHUNK_ROWS;
  return n_frames > 0x7fffffffLL / *max_chunks ? -1 : n_frames * *max_chunks;
}

extern "C" int hgn_training_noise_ragged(const float* x, int64_t ldx, int d, const int64_t* node_type, int64_t ldt, uint32_t free_mask,
                                         int64_t rows, const int64_t* frame_rows, const int32_t* frame_ptr, int64_t n_frames,
                                         const int64_t* frame_ids, uint64_t seed, uint64_t draw, float std_, const float* target,
                                         int64_t ld_tgt, float target_scale, float* out_x, int64_t ld_ox, float* out_target,
                                         int64_t ld_ot, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (d < 1 || d > 4 || !frame_ptr || ragged_max_rows(rows, frame_rows, n_frames, 0x7fffffff) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise_ragged: bad sizes (1 <= d <= 4, " HGN_RAGGED_SIZES ")");
  if ((target == nullptr) != (out_target == nullptr))
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise_ragged: target and out_target must both be given or both be null");
  if (ldx < d || ld_ox < d || ldt < 1 || (target && (ld_tgt < d || ld_ot < d)))
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise_ragged: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (!(std_ >= 0.f) || std_ > 3.4028234e38f)
    return hgn_fail(HGN_E_INVALID, "hgn_training_noise_ragged: the standard deviation must be finite and not negative");
  if (!x || !node_type || !out_x) return hgn_fail(HGN_E_INVALID, "hgn_training_noise_ragged: null pointer");
  ProfScope ps(13, (double)rows, stream);
  hipLaunchKernelGGL(training_noise_ragged_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, x, (long)ldx, d,
                     node_type, (long)ldt, (unsigned)free_mask, (long)rows, frame_ptr, (long)n_frames, frame_ids,
                     (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(draw & 0xffffffffu), (unsigned)(draw >> 32),
                     std_, target, (long)ld_tgt, target_scale, out_x, (long)ld_ox, out_target, (long)ld_ot);
  return hgn_check_launch("hgn_training_noise_ragged");
}

extern "C" int hgn_frame_losses_ragged_workspace_bytes(int64_t rows, const int64_t* frame_rows, int64_t n_frames, size_t* bytes) {
  int64_t max_chunks = 0;
  const int64_t chunks = ragged_loss_chunks(rows, frame_rows, n_frames, &max_chunks);
  if (!bytes || chunks < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged_workspace_bytes: bad sizes (0 < rows < 2^31, n_frames >= 1, every "
                                   "frame_rows[f] >= 1, their sum = rows, n_frames * chunks of the largest frame < 2^31)");
  *bytes = (size_t)chunks * 3 * sizeof(double);
  return HGN_OK;
}

extern "C" int hgn_frame_losses_ragged(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                                       const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows,
                                       const int64_t* frame_rows, const int32_t* frame_ptr, int64_t n_frames, const float* acc_sum,
                                       const float* acc_sumsq, const float* acc_count, float eps, const float* cur, int64_t ld_cur,
                                       int d, float ca, const float* prev, int64_t ld_prev, float cp, const float* state_target,
                                       int64_t ld_st, float* loss, float* state_err, int64_t* count, void* workspace,
                                       size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int64_t max_chunks = 0;
  const int64_t chunks = ragged_loss_chunks(rows, frame_rows, n_frames, &max_chunks);
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || !frame_ptr || chunks < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: bad sizes (1 <= F <= 32, " HGN_RAGGED_SIZES
                                   ", n_frames * chunks of the largest frame < 2^31)");
  const int given = (acc_sum != nullptr) + (acc_sumsq != nullptr) + (acc_count != nullptr) + (cur != nullptr) + (state_target != nullptr);
  if ((given != 0 && given != 5) || (given == 0 && prev))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: the state part (statistics, cur, state_target; prev optional) must be given whole or not at all");
  const bool with_state = given == 5;
  if (with_state != (state_err != nullptr))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: state_err must be given exactly when the state part is");
  if (with_state && (d < 1 || d > F)) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: bad state width (1 <= d <= F)");
  if (ld_out < F || ld_tgt < F || ldt < 1 || (with_state && (ld_cur < d || ld_st < d || (prev && ld_prev < d))))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (!net_out || !target || !node_type || !loss || !count) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: null pointer");
  if (!workspace || ((uintptr_t)workspace & 7)) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: null or misaligned workspace");
  if (ws_bytes < (size_t)chunks * 3 * sizeof(double))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged: workspace too small (hgn_frame_losses_ragged_workspace_bytes)");
  ProfScope ps(13, (double)rows, stream);
  double* part_s = (double*)workspace;
  double* part_e = part_s + chunks;
  long long* part_n = (long long*)(part_e + chunks);
  hipLaunchKernelGGL(frame_losses_ragged_partial_kernel, dim3((unsigned)chunks), dim3(HGN_LOSS_CHUNK_ROWS), 0, stream, net_out,
                     (long)ld_out, target, (long)ld_tgt, F, node_type, (long)ldt, (unsigned)free_mask, (long)rows, frame_ptr,
                     (long)max_chunks, acc_sum, acc_sumsq, acc_count, eps, cur, (long)ld_cur, d, ca, prev, (long)ld_prev, cp,
                     state_target, (long)ld_st, part_s, part_e, part_n);
  hipLaunchKernelGGL(frame_losses_ragged_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)part_s, (const double*)part_e,
                     (const long long*)part_n, (long)n_frames, (long)rows, frame_ptr, (long)max_chunks, F, with_state ? d : 1, loss,
                     state_err, count);
  return hgn_check_launch("hgn_frame_losses_ragged");
}

extern "C" int hgn_frame_losses_ragged_bwd(const float* net_out, int64_t ld_out, const float* target, int64_t ld_tgt, int F,
                                           const int64_t* node_type, int64_t ldt, uint32_t free_mask, int64_t rows,
                                           const int64_t* frame_rows, const int32_t* frame_ptr, int64_t n_frames,
                                           const int64_t* count, const float* g, float* d_net, int64_t ld_dnet, float* d_target,
                                           int64_t ld_dtgt, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (F < 1 || F > HGN_MAX_FEATURE_WIDTH || !frame_ptr || ragged_max_rows(rows, frame_rows, n_frames, 0x7fffffff) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged_bwd: bad sizes (1 <= F <= 32, " HGN_RAGGED_SIZES ")");
  if (ld_out < F || ld_tgt < F || ldt < 1 || (d_net && ld_dnet < F) || (d_target && ld_dtgt < F))
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged_bwd: bad strides (a row stride is smaller than its row, or ldt < 1)");
  if (!d_net && !d_target)
    return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged_bwd: no output asked for (d_net and d_target are both null)");
  if (!net_out || !target || !node_type || !count) return hgn_fail(HGN_E_INVALID, "hgn_frame_losses_ragged_bwd: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(frame_losses_ragged_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, net_out, (long)ld_out,
                     target, (long)ld_tgt, F, node_type, (long)ldt, (unsigned)free_mask, (long)rows, frame_ptr, (long)n_frames, count,
                     g, d_net, (long)ld_dnet, d_target, (long)ld_dtgt);
  return hgn_check_launch("hgn_frame_losses_ragged_bwd");
}

extern "C" int hgn_member_mean_bwd(const float* d_mean, int64_t ld_dmean, int D, const int32_t* seg_rowptr, int64_t S,
                                  const int32_t* item_seg, const int32_t* node_rowptr, const int32_t* node_items, int64_t rows,
                                  int64_t M, float* d_data, int64_t ld, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (D < 1 || ld < D || ld_dmean < D) return hgn_fail(HGN_E_INVALID, "hgn_member_mean_bwd: bad widths / strides (D >= 1, ld >= D, ld_dmean >= D)");
  if (rows < 0 || rows > 0x7fffffff || M < 0 || M > 0x7fffffff || S < 0 || S > 0x7fffffff)
    return hgn_fail(HGN_E_INVALID, "hgn_member_mean_bwd: bad sizes (0 <= rows, M, S < 2^31)");
  if ((rows > 0 && !d_data) || (rows > 0 && M > 0 && (!d_mean || !seg_rowptr || !item_seg || !node_rowptr || !node_items)))
    return hgn_fail(HGN_E_INVALID, "hgn_member_mean_bwd: null pointer");
  if (M > 0 && S < 1) return hgn_fail(HGN_E_INVALID, "hgn_member_mean_bwd: members without a segment (M > 0 needs S >= 1)");
  if (rows == 0) return HGN_OK;
  const int64_t n = rows * D;
  if ((n + 255) / 256 > 0x7fffffff) return hgn_fail(HGN_E_INVALID, "hgn_member_mean_bwd: rows * D does not fit one launch");
  ProfScope ps(13, (double)rows, stream);
  hipLaunchKernelGGL(member_mean_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_mean, (long)ld_dmean, D,
                     seg_rowptr, (long)S, item_seg, node_rowptr, node_items, (long)rows, (long)M, d_data, (long)ld);
  return hgn_check_launch("hgn_member_mean_bwd");
}

extern "C" int hgn_radius_edges_workspace_bytes(int64_t N, size_t* bytes) {
  if (!bytes || N < 0 || N > 0x7ffffffe) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_workspace_bytes: bad size");
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum<int*, int*>(nullptr, t, nullptr, nullptr, (int)(N + 1));
  *bytes = up256((size_t)(N + 1) * 4) + up256(t) + 256;
  return HGN_OK;
}

static int radius_args_ok(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t N,
                          float radius, const int32_t* nbr_rowptr, const int32_t* nbr) {
  if (N < 0 || d < 1 || d > 3 || ld < d || ldt < 1 || !(radius >= 0.f)) return 0;
  if (N > 0 && (!pos || !node_type)) return 0;
  if ((nbr_rowptr == nullptr) != (nbr == nullptr)) return 0;
  return 1;
}

extern "C" int hgn_radius_edges_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t N,
                                      float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                      const int32_t* nbr, int32_t* offsets, int64_t* total, void* workspace,
                                      size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  size_t need = 0;
  if (hgn_radius_edges_workspace_bytes(N, &need) != HGN_OK) return HGN_E_INVALID;
  if (!radius_args_ok(pos, ld, d, node_type, ldt, N, radius, nbr_rowptr, nbr) || !offsets || !total || !workspace ||
      ws_bytes < need)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_count: bad argument or workspace too small");
  *total = 0;
  ProfScope ps(13, (double)N, stream);
  int* counts = (int*)workspace;
  void* temp = (char*)workspace + up256((size_t)(N + 1) * 4);
  size_t tb = need - up256((size_t)(N + 1) * 4);
  if (hipMemsetAsync(counts, 0, (size_t)(N + 1) * 4, stream) != hipSuccess) return hgn_check_launch("hgn_radius_edges_count memset");
  if (N > 0)
    hipLaunchKernelGGL(radius_edges_kernel<false>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                       node_type, (long)ldt, (long)N, radius, sender_type, receiver_type, nbr_rowptr, nbr, counts,
                       (const int*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
  if (hipcub::DeviceScan::ExclusiveSum(temp, tb, counts, offsets, (int)(N + 1), stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_count scan");
  int host_total = 0;
  if (hipMemcpyAsync(&host_total, offsets + N, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_count readback");
  *total = host_total;
  return hgn_check_launch("hgn_radius_edges_count");
}

extern "C" int hgn_radius_edges_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt, int64_t N,
                                     float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                     const int32_t* nbr, const int32_t* offsets, int64_t* senders, int64_t* receivers,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!radius_args_ok(pos, ld, d, node_type, ldt, N, radius, nbr_rowptr, nbr) || !offsets)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_fill: bad argument");
  if (N == 0) return HGN_OK;
  if (!senders || !receivers) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_fill: null output");
  ProfScope ps(13, (double)N, stream);
  hipLaunchKernelGGL(radius_edges_kernel<true>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                     node_type, (long)ldt, (long)N, radius, sender_type, receiver_type, nbr_rowptr, nbr, (int*)nullptr,
                     offsets, senders, receivers);
  return hgn_check_launch("hgn_radius_edges_fill");
}

// rows of the union, or -1 when the batch shape is refused (n_graphs < 1, nodes_per_graph < 0, more than 0x7ffffffe rows)
static int64_t radius_batch_rows(int64_t n_graphs, int64_t nodes_per_graph) {
  if (n_graphs < 1 || nodes_per_graph < 0) return -1;
  if (nodes_per_graph > 0 && n_graphs > 0x7ffffffeLL / nodes_per_graph) return -1;
  return n_graphs * nodes_per_graph;
}

static size_t radius_batch_counts_bytes(int64_t rows) { return up256((size_t)(rows + 1) * 4); }

extern "C" int hgn_radius_edges_batch_workspace_bytes(int64_t n_graphs, int64_t nodes_per_graph, size_t* bytes) {
  const int64_t rows = radius_batch_rows(n_graphs, nodes_per_graph);
  if (!bytes || rows < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_workspace_bytes: bad size (n_graphs >= 1, nodes_per_graph >= 0, "
                                   "n_graphs * nodes_per_graph <= 0x7ffffffe)");
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum<int*, int*>(nullptr, t, nullptr, nullptr, (int)(rows + 1));
  *bytes = radius_batch_counts_bytes(rows) + up256(t) + 256;
  return HGN_OK;
}

extern "C" int hgn_radius_edges_batch_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                            int64_t n_graphs, int64_t nodes_per_graph, float radius, int sender_type,
                                            int receiver_type, const int32_t* nbr_rowptr, const int32_t* nbr,
                                            int32_t* offsets, int32_t* graph_offsets, int64_t* total, void* workspace,
                                            size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = radius_batch_rows(n_graphs, nodes_per_graph);
  if (rows < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_count: bad batch shape (n_graphs >= 1, nodes_per_graph >= 0, "
                                   "n_graphs * nodes_per_graph <= 0x7ffffffe)");
  if (!radius_args_ok(pos, ld, d, node_type, ldt, rows, radius, nbr_rowptr, nbr))
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_count: bad argument");
  if (!offsets || !total) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_count: null output");
  size_t need = 0;
  if (hgn_radius_edges_batch_workspace_bytes(n_graphs, nodes_per_graph, &need) != HGN_OK || !workspace || ws_bytes < need)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_count: workspace missing or too small");
  *total = 0;
  ProfScope ps(13, (double)rows, stream);
  int* counts = (int*)workspace;
  void* temp = (char*)workspace + radius_batch_counts_bytes(rows);
  size_t tb = need - radius_batch_counts_bytes(rows);
  if (hipMemsetAsync(counts, 0, (size_t)(rows + 1) * 4, stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_batch_count memset");
  if (rows > 0)
    hipLaunchKernelGGL(radius_edges_batch_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                       node_type, (long)ldt, (long)rows, (long)nodes_per_graph, radius, sender_type, receiver_type, nbr_rowptr,
                       nbr, counts, (const int*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
  if (hipcub::DeviceScan::ExclusiveSum(temp, tb, counts, offsets, (int)(rows + 1), stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_batch_count scan");
  if (graph_offsets)
    hipLaunchKernelGGL(graph_offsets_kernel, dim3((unsigned)((n_graphs + 256) / 256)), dim3(256), 0, stream,
                       (const int*)offsets, (long)n_graphs, (long)nodes_per_graph, graph_offsets);
  int host_total = 0;
  if (hipMemcpyAsync(&host_total, offsets + rows, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_batch_count readback");
  *total = host_total;
  return hgn_check_launch("hgn_radius_edges_batch_count");
}

extern "C" int hgn_radius_edges_batch_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                           int64_t n_graphs, int64_t nodes_per_graph, float radius, int sender_type,
                                           int receiver_type, const int32_t* nbr_rowptr, const int32_t* nbr,
                                           const int32_t* offsets, int64_t* senders, int64_t* receivers, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = radius_batch_rows(n_graphs, nodes_per_graph);
  if (rows < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_fill: bad batch shape (n_graphs >= 1, nodes_per_graph >= 0, "
                                   "n_graphs * nodes_per_graph <= 0x7ffffffe)");
  if (!radius_args_ok(pos, ld, d, node_type, ldt, rows, radius, nbr_rowptr, nbr) || !offsets)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_fill: bad argument");
  if (rows == 0) return HGN_OK;
  if (!senders || !receivers) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_batch_fill: null output");
  ProfScope ps(13, (double)rows, stream);
  hipLaunchKernelGGL(radius_edges_batch_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                     node_type, (long)ldt, (long)rows, (long)nodes_per_graph, radius, sender_type, receiver_type, nbr_rowptr, nbr,
                     (int*)nullptr, offsets, senders, receivers);
  return hgn_check_launch("hgn_radius_edges_batch_fill");
}

#define HGN_RAGGED_GRAPHS "0 < rows <= 0x7ffffffe, n_graphs >= 1, every frame_rows[b] >= 1, their sum = rows"

extern "C" int hgn_radius_edges_ragged_workspace_bytes(int64_t rows, const int64_t* frame_rows, int64_t n_graphs, size_t* bytes) {
  if (!bytes || ragged_max_rows(rows, frame_rows, n_graphs, 0x7ffffffe) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_workspace_bytes: bad size (" HGN_RAGGED_GRAPHS ")");
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum<int*, int*>(nullptr, t, nullptr, nullptr, (int)(rows + 1));
  *bytes = radius_batch_counts_bytes(rows) + up256(t) + 256;
  return HGN_OK;
}

extern "C" int hgn_radius_edges_ragged_count(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                             int64_t rows, const int64_t* frame_rows, const int32_t* frame_ptr, int64_t n_graphs,
                                             float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                             const int32_t* nbr, int32_t* offsets, int32_t* graph_offsets, int64_t* total,
                                             void* workspace, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!frame_ptr || ragged_max_rows(rows, frame_rows, n_graphs, 0x7ffffffe) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_count: bad batch shape (" HGN_RAGGED_GRAPHS ", frame_ptr not null)");
  if (!radius_args_ok(pos, ld, d, node_type, ldt, rows, radius, nbr_rowptr, nbr))
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_count: bad argument");
  if (!offsets || !total) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_count: null output");
  size_t need = 0;
  if (hgn_radius_edges_ragged_workspace_bytes(rows, frame_rows, n_graphs, &need) != HGN_OK || !workspace || ws_bytes < need)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_count: workspace missing or too small");
  *total = 0;
  ProfScope ps(13, (double)rows, stream);
  int* counts = (int*)workspace;
  void* temp = (char*)workspace + radius_batch_counts_bytes(rows);
  size_t tb = need - radius_batch_counts_bytes(rows);
  if (hipMemsetAsync(counts, 0, (size_t)(rows + 1) * 4, stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_ragged_count memset");
  hipLaunchKernelGGL(radius_edges_ragged_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                     node_type, (long)ldt, (long)rows, frame_ptr, (long)n_graphs, radius, sender_type, receiver_type, nbr_rowptr, nbr,
                     counts, (const int*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
  if (hipcub::DeviceScan::ExclusiveSum(temp, tb, counts, offsets, (int)(rows + 1), stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_ragged_count scan");
  if (graph_offsets)
    hipLaunchKernelGGL(graph_offsets_ragged_kernel, dim3((unsigned)((n_graphs + 256) / 256)), dim3(256), 0, stream,
                       (const int*)offsets, frame_ptr, (long)n_graphs, (long)rows, graph_offsets);
  int host_total = 0;
  if (hipMemcpyAsync(&host_total, offsets + rows, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return hgn_check_launch("hgn_radius_edges_ragged_count readback");
  *total = host_total;
  return hgn_check_launch("hgn_radius_edges_ragged_count");
}

extern "C" int hgn_radius_edges_ragged_fill(const float* pos, int64_t ld, int d, const int64_t* node_type, int64_t ldt,
                                            int64_t rows, const int64_t* frame_rows, const int32_t* frame_ptr, int64_t n_graphs,
                                            float radius, int sender_type, int receiver_type, const int32_t* nbr_rowptr,
                                            const int32_t* nbr, const int32_t* offsets, int64_t* senders, int64_t* receivers,
                                            void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!frame_ptr || ragged_max_rows(rows, frame_rows, n_graphs, 0x7ffffffe) < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_fill: bad batch shape (" HGN_RAGGED_GRAPHS ", frame_ptr not null)");
  if (!radius_args_ok(pos, ld, d, node_type, ldt, rows, radius, nbr_rowptr, nbr) || !offsets)
    return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_fill: bad argument");
  if (!senders || !receivers) return hgn_fail(HGN_E_INVALID, "hgn_radius_edges_ragged_fill: null output");
  ProfScope ps(13, (double)rows, stream);
  hipLaunchKernelGGL(radius_edges_ragged_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, pos, (long)ld, d,
                     node_type, (long)ldt, (long)rows, frame_ptr, (long)n_graphs, radius, sender_type, receiver_type, nbr_rowptr, nbr,
                     (int*)nullptr, offsets, senders, receivers);
  return hgn_check_launch("hgn_radius_edges_ragged_fill");
}

extern "C" int hgn_forman_curvature(const float* A, const float* A2, const float* d_in, const float* d_out, int64_t N,
                                    const int32_t* ei, const int32_t* ej, int64_t nnz, float* C, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 0 || nnz < 0 || N > 46340) return hgn_fail(HGN_E_INVALID, "hgn_forman_curvature: bad size (dense N x N, N <= 46340)");
  if (nnz == 0) return HGN_OK;
  if (!A || !A2 || !d_in || !d_out || !ei || !ej || !C) return hgn_fail(HGN_E_INVALID, "hgn_forman_curvature: null pointer");
  ProfScope ps(13, (double)nnz, stream);
  hipLaunchKernelGGL(forman_curvature_kernel, dim3((unsigned)((nnz + 3) / 4)), dim3(256), 0, stream, A, A2, d_in, d_out, (long)N,
                     ei, ej, (long)nnz, C);
  return hgn_check_launch("hgn_forman_curvature");
}

extern "C" int hgn_forman_post_delta(const float* A, const float* A2, float d_in_x, float d_out_y, int64_t N, int32_t x,
                                     int32_t y, const int32_t* i_nb, int32_t dim_i, const int32_t* j_nb, int32_t dim_j, float* D,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 1 || N > 46340 || x < 0 || y < 0 || x >= N || y >= N || dim_i < 0 || dim_j < 0)
    return hgn_fail(HGN_E_INVALID, "hgn_forman_post_delta: bad size / index");
  if (dim_i == 0 || dim_j == 0) return HGN_OK;
  if (!A || !A2 || !i_nb || !j_nb || !D) return hgn_fail(HGN_E_INVALID, "hgn_forman_post_delta: null pointer");
  ProfScope ps(13, (double)dim_i * dim_j, stream);
  const long pairs = (long)dim_i * dim_j;
  hipLaunchKernelGGL(forman_post_delta_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, stream, A, A2, d_in_x, d_out_y,
                     (long)N, x, y, i_nb, dim_i, j_nb, dim_j, D);
  return hgn_check_launch("hgn_forman_post_delta");
}

extern "C" int hgn_rel_edge_features_bwd(const float* d_feat, int64_t ldf, const float* d_len, const float* a, int64_t lda,
                                         int da, const float* b, int64_t ldb, int db, int64_t n_rows,
                                         const int64_t* senders, const int64_t* receivers, int64_t E,
                                         const int32_t* rowptr_s, const int32_t* perm_s, const int32_t* rowptr_r,
                                         const int32_t* perm_r, int64_t max_degree, float* d_a, float* d_b, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (E < 0 || E > 0x7fffffffLL || n_rows < 0 || da < 1 || da > 3 || db < 0 || db > 3 || lda < da || (db > 0 && ldb < db))
    return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features_bwd: sizes must satisfy 1<=da<=3, 0<=db<=3, ld >= width, E < 2^31");
  const int W = da + 1 + (db > 0 ? db + 1 : 0);
  if (d_feat && ldf < W) return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features_bwd: ldf smaller than the feature row");
  if (d_b && db == 0) return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features_bwd: d_b given with db = 0");
  if (n_rows == 0 || (!d_a && !d_b)) return HGN_OK;
  if (E == 0 || (!d_feat && !d_len)) {                 // no edge, or no gradient arriving: every row is zero
    if ((d_a && hipMemsetAsync(d_a, 0, (size_t)n_rows * da * sizeof(float), stream) != hipSuccess) ||
        (d_b && hipMemsetAsync(d_b, 0, (size_t)n_rows * db * sizeof(float), stream) != hipSuccess))
      return hgn_check_launch("hgn_rel_edge_features_bwd memset");
    return HGN_OK;
  }
  if (!a || (d_b && !b) || !senders || !receivers || !rowptr_s || !perm_s || !rowptr_r || !perm_r)
    return hgn_fail(HGN_E_INVALID, "hgn_rel_edge_features_bwd: null pointer");
  ProfScope ps(13, (double)E, stream);
  RelBwd p;
  p.a = a; p.b = b; p.d_feat = d_feat; p.d_len = d_len;
  p.lda = (long)lda; p.ldb = (long)ldb; p.ldf = (long)ldf;
  p.da = da; p.db = db; p.n_rows = (long)n_rows; p.E = (long)E;
  p.snd = senders; p.rcv = receivers;
  p.rp_s = rowptr_s; p.perm_s = perm_s; p.rp_r = rowptr_r; p.perm_r = perm_r;
  p.d_a = d_a; p.d_b = d_b;
  const int split = (max_degree < 0 || max_degree > REL_BWD_WAVE_DEG) ? 1 : 0;
  hipLaunchKernelGGL(rel_edge_bwd_thread_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, p, split);
  if (split)
    hipLaunchKernelGGL(rel_edge_bwd_wave_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, stream, p);
  return hgn_check_launch("hgn_rel_edge_features_bwd");
}

extern "C" int hgn_node_features_bwd(const float* d_out, int64_t ldo, int d, int n_classes, int vel_first,
                                     const int64_t* node_type, int64_t ldt, int vel_mask_type, int64_t N, float* d_cur,
                                     float* d_prev, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 0 || d < 0 || n_classes < 0 || d + n_classes < 1 || d + n_classes > HGN_MAX_FEATURE_WIDTH || ldo < d + n_classes ||
      ldt < 1)
    return hgn_fail(HGN_E_INVALID, "hgn_node_features_bwd: bad widths / strides");
  if (N == 0 || d == 0 || (!d_cur && !d_prev)) return HGN_OK;
  if (!d_out || (vel_mask_type >= 0 && !node_type)) return hgn_fail(HGN_E_INVALID, "hgn_node_features_bwd: null pointer");
  ProfScope ps(13, (double)N, stream);
  const int64_t n = N * d;
  hipLaunchKernelGGL(node_feat_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_out, (long)ldo, d,
                     n_classes, vel_first, node_type, (long)ldt, vel_mask_type, (long)N, d_cur, d_prev);
  return hgn_check_launch("hgn_node_features_bwd");
}

extern "C" int hgn_normalize_bwd(const float* d_out, int64_t rows, int F, const float* acc_sum, const float* acc_sumsq,
                                 const float* acc_count, float eps, int inverse, float* d_x, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (rows < 0 || F < 1 || F > HGN_MAX_FEATURE_WIDTH || !acc_sum || !acc_sumsq || !acc_count)
    return hgn_fail(HGN_E_INVALID, "hgn_normalize_bwd: null pointer or bad width");
  if (rows == 0) return HGN_OK;
  if (!d_out || !d_x) return hgn_fail(HGN_E_INVALID, "hgn_normalize_bwd: null pointer");
  ProfScope ps(13, (double)rows, stream);
  const int64_t n = rows * F;
  hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_out, (long)n, F, acc_sum,
                     acc_sumsq, acc_count, eps, inverse, d_x);
  return hgn_check_launch("hgn_normalize_bwd");
}
