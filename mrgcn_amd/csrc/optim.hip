// Streaming kernels of the epoch that surround the layer: masked-ReLU backward, the
// cross-entropy over labelled rows (mrgcn/tasks/node_classification.py:439-444), the global
// gradient norm + clip coefficient (clip_grad_norm_(…, 1.0), :192) and Adam (:35-37, :193).
// All are HBM-bound: float4 accesses, grid-stride over <= 2048 blocks.  At AM scale the
// Adam pass over weight_I (2.67 GB x 7 streams) dominates the epoch.
#include <cstdlib>

#include <algorithm>

#include "common.hpp"
#include "config.hpp"
#include "xent_row.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;

inline int stream_grid(int64_t n_vec) {
  int64_t b = (n_vec + kTB - 1) / kTB;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int)b;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

__device__ __forceinline__ float block_sum(float x) {  // result valid in thread 0
  __shared__ float s_part[kTB / kWave];
  x = wave_sum(x);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_part[w] = x;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < kTB / kWave; ++i) t += s_part[i];
  return t;
}

// the same on row-strided operands (a layer output kept in a buffer with padded rows): 16 lanes per row
__global__ void k_relu_bwd_rows(const float *__restrict__ dY, int64_t ldd, const float *__restrict__ Y, int64_t ldy,
                                int64_t rows, int F, float *__restrict__ out, int64_t ldo) {
  const int f0 = threadIdx.x & 15;
  const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> 4;
  for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; r < rows; r += step)
    for (int f = f0; f < F; f += 16) out[r * ldo + f] = Y[r * ldy + f] > 0.f ? dY[r * ldd + f] : 0.f;
}

// out = dY * (Y > 0)
__global__ void k_relu_bwd(const float *__restrict__ dY, const float *__restrict__ Y, int64_t n,
                           float *__restrict__ out) {
  const int64_t nv = n >> 2;
  const float4 *d4 = reinterpret_cast<const float4 *>(dY);
  const float4 *y4 = reinterpret_cast<const float4 *>(Y);
  float4 *o4 = reinterpret_cast<float4 *>(out);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 d = d4[i], y = y4[i], o;
    o.x = y.x > 0.f ? d.x : 0.f;
    o.y = y.y > 0.f ? d.y : 0.f;
    o.z = y.z > 0.f ? d.z : 0.f;
    o.w = y.w > 0.f ? d.w : 0.f;
    o4[i] = o;
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += blockDim.x)
      out[i] = Y[i] > 0.f ? dY[i] : 0.f;
}

// flags[i] = 1 when row i of X holds anything but zeros (NaN counts as something)
__global__ void k_rows_nonzero(const float *__restrict__ X, int64_t ld, int F, int64_t nrows,
                               uint8_t *__restrict__ flags, int vec_ok) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float *row = X + i * ld;
    bool nz = false;
    int q = 0;
    if (vec_ok)
      for (; q + 4 <= F; q += 4) {
        const float4 t = *reinterpret_cast<const float4 *>(row + q);
        nz |= (t.x != 0.f) | (t.y != 0.f) | (t.z != 0.f) | (t.w != 0.f);
      }
    for (; q < F; ++q) nz |= row[q] != 0.f;
    flags[i] = nz ? 1 : 0;
  }
}

// the same for wide rows (F > 32): a wave per row, lanes along the row (a thread per row reads 64 rows of F floats
// with a stride of F: 104 us for 14 541 x 200 at the FB15k-237 shape against a few us of bytes)
__global__ __launch_bounds__(256) void k_rows_nonzero_wide(const float *__restrict__ X, int64_t ld, int F, int64_t nrows,
                                                           uint8_t *__restrict__ flags) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < nrows;
       i += ((int64_t)gridDim.x * blockDim.x) >> 6) {
    const float *row = X + i * ld;
    bool nz = false;
    for (int q = lane; q < F; q += 64) nz |= row[q] != 0.f;
    const uint64_t any = __ballot(nz);
    if (lane == 0) flags[i] = any ? 1 : 0;
  }
}

// sum of squares -> double accumulator (one atomic per block).  At most 512 blocks, four 16-byte pieces in flight per
// thread: a double atomic on ONE address costs ~12 ns — with 2 048 blocks the adds alone took 25 of the kernel's 31 us
// (AIFB's 48 MB gradient, FB15k-237's 23 MB).
__global__ void k_sumsq(const float *__restrict__ x, int64_t n, double *__restrict__ accum) {
  const int64_t nv = n >> 2;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = x4[i + u * stride < nv ? i + u * stride : i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u * stride < nv) {
        s = fmaf(v[u].x, v[u].x, s);
        s = fmaf(v[u].y, v[u].y, s);
        s = fmaf(v[u].z, v[u].z, s);
        s = fmaf(v[u].w, v[u].w, s);
      }
    }
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += blockDim.x) s = fmaf(x[i], x[i], s);
  float t = block_sum(s);
  if (threadIdx.x == 0) atomicAdd(accum, (double)t);
}

// clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6))
// Adam on a parameter made of `nrows` rows of `rowlen` floats (weight_I in its node-major layout: one row
// = the B*F floats of a node) whose gradient exists for some rows only — a semi-supervised epoch gives
// gradient to the nodes within reach of a label, with few labelled nodes half of the AM node table gets
// none, ever.  `ever[r]` = 0: row r never received gradient — g = m = v = 0, the update is the identity
// and nothing is read or written (weight_decay must be 0); `cur[r]` = 0 but ever: the gradient is zero
// this step (g is not read: its row may be unwritten).  Rows with cur = 1 are marked ever.
// One thread per float4 of a row (rowlen % 4 == 0; k_adam_rows_scalar: per float), rows walked by the grid.
__global__ __launch_bounds__(256) void k_adam_rows_scalar(float *__restrict__ p, const float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v,
                                                          int64_t nrows, int rowlen, const uint8_t *__restrict__ cur,
                                                          uint8_t *__restrict__ ever, float lr, float b1, float b2,
                                                          float eps, float bc1, float bc2_sqrt,
                                                          const float *__restrict__ scale,
                                                          const float *__restrict__ bc_dev) {
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  const float sc = scale ? *scale : 1.f;
  const float step = lr / bc1;
  const int64_t n = nrows * rowlen;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / rowlen;
    const bool c = cur[r] != 0;
    if (!c && !ever[r]) continue;
    float gg = (c ? g[i] : 0.f) * sc;
    float mm = fmaf(b1, m[i], (1.f - b1) * gg);
    float vv = fmaf(b2, v[i], (1.f - b2) * gg * gg);
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] -= step * (mm / denom);
    m[i] = mm;
    v[i] = vv;
  }
}
// rows that took gradient count as `ever` from now on (after the update pass: no thread may see the flag change
// under its feet)
__global__ void k_rows_mark_ever(const uint8_t *__restrict__ cur, uint8_t *__restrict__ ever, int64_t nrows) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nrows && cur[r]) ever[r] = 1;
}

template <int RB>  // rows per block step
__global__ __launch_bounds__(256) void k_adam_rows(float *__restrict__ p, const float *__restrict__ g,
                                                   float *__restrict__ m, float *__restrict__ v,
                                                   int64_t nrows, int rowlen4, const uint8_t *__restrict__ cur,
                                                   uint8_t *__restrict__ ever, float lr, float b1, float b2,
                                                   float eps, float bc1, float bc2_sqrt,
                                                   const float *__restrict__ scale,
                                                   const float *__restrict__ bc_dev) {
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  const float sc = scale ? *scale : 1.f;
  const float step = lr / bc1;
  float4 *p4 = reinterpret_cast<float4 *>(p);
  const float4 *g4 = reinterpret_cast<const float4 *>(g);
  float4 *m4 = reinterpret_cast<float4 *>(m);
  float4 *v4 = reinterpret_cast<float4 *>(v);
  auto upd = [&](float &pp, float gg, float &mm, float &vv) {  // == k_adam with wd = 0
    gg *= sc;
    mm = fmaf(b1, mm, (1.f - b1) * gg);
    vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
    float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
  };
  // a block takes RB consecutive rows per step: RB * rowlen4 float4s, thread t the t-th, t + 256-th, ...
  const int per = RB * rowlen4;
  for (int64_t r0 = (int64_t)blockIdx.x * RB; r0 < nrows; r0 += (int64_t)gridDim.x * RB) {
    for (int t = threadIdx.x; t < per; t += blockDim.x) {
      const int rr = t / rowlen4;
      const int64_t r = r0 + rr;
      if (r >= nrows) break;
      const bool c = cur[r] != 0;
      if (!c && !ever[r]) continue;
      const int64_t i = r * rowlen4 + (t - rr * rowlen4);
      float4 P = p4[i], M = m4[i], V = v4[i];
      float4 G = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c) G = g4[i];
      upd(P.x, G.x, M.x, V.x);
      upd(P.y, G.y, M.y, V.y);
      upd(P.z, G.z, M.z, V.z);
      upd(P.w, G.w, M.w, V.w);
      p4[i] = P;
      m4[i] = M;
      v4[i] = V;
      if (c && t == rr * rowlen4) ever[r] = 1;  // (readers of the same row see cur = 1 either way)
    }
  }
}

// Adam on the rows `index[c]` of a parameter (rows of rowlen4 16-byte pieces) with the gradient of row index[c] in
// row c of a COMPACT gradient — the literal operand of a featureless layer without bases (functional._SpmmLiteral): the
// only rows of the (R*N) x F table that ever see gradient are the graph's compact columns, whatever the label set; the
// others keep zero moments and never move (weight_decay = 0).  One thread per piece, a one-shot grid; the arithmetic is
// k_adam's with wd = 0.  `index` holds distinct rows.
__global__ __launch_bounds__(256) void k_adam_index_rows(float *__restrict__ p, const float *__restrict__ g,
                                                         int64_t ldg4, float *__restrict__ m, float *__restrict__ v,
                                                         const int32_t *__restrict__ index, int64_t n, int rowlen4,
                                                         float lr, float b1, float b2, float eps, float bc1,
                                                         float bc2_sqrt, const float *__restrict__ scale,
                                                         const float *__restrict__ bc_dev) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * rowlen4) return;
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  const float sc = scale ? *scale : 1.f;
  const float step = lr / bc1;
  const int64_t c = i / rowlen4;
  const int q = (int)(i - c * rowlen4);
  const int64_t at = (int64_t)index[c] * rowlen4 + q;
  float4 *p4 = reinterpret_cast<float4 *>(p) + at;
  float4 *m4 = reinterpret_cast<float4 *>(m) + at;
  float4 *v4 = reinterpret_cast<float4 *>(v) + at;
  const float4 G = reinterpret_cast<const float4 *>(g)[c * ldg4 + q];
  float4 P = *p4, M = *m4, V = *v4;
  auto upd = [&](float &pp, float gg, float &mm, float &vv) {  // == k_adam with wd = 0
    gg *= sc;
    mm = fmaf(b1, mm, (1.f - b1) * gg);
    vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
    float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
  };
  upd(P.x, G.x, M.x, V.x);
  upd(P.y, G.y, M.y, V.y);
  upd(P.z, G.z, M.z, V.z);
  upd(P.w, G.w, M.w, V.w);
  *p4 = P;
  *m4 = M;
  *v4 = V;
}

__global__ void k_clip_coef(const double *__restrict__ sumsq, float max_norm, float *__restrict__ coef,
                            float *__restrict__ norm) {
  float nrm = (float)sqrt(*sumsq);
  float c = max_norm / (nrm + 1e-6f);
  *coef = c < 1.f ? c : 1.f;
  if (norm) *norm = nrm;
}

// torch.optim.Adam (amsgrad = False, maximize = False), gradient pre-scaled by *scale
template <bool NT>
__global__ void k_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                       float *__restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                       float wd, float bc1, float bc2_sqrt, const float *__restrict__ scale,
                       const float *__restrict__ bc_dev) {
  if (bc_dev) {  // bias corrections kept on the device (graph-capturable steps)
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  const float sc = scale ? *scale : 1.f;
  const float step = lr / bc1;
  const int64_t nv = n >> 2;
  float4 *p4 = reinterpret_cast<float4 *>(p);
  const float4 *g4 = reinterpret_cast<const float4 *>(g);
  float4 *m4 = reinterpret_cast<float4 *>(m);
  float4 *v4 = reinterpret_cast<float4 *>(v);
  auto upd = [&](float &pp, float gg, float &mm, float &vv) {
    gg *= sc;
    if (wd != 0.f) gg = fmaf(wd, pp, gg);
    mm = fmaf(b1, mm, (1.f - b1) * gg);
    vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
    float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
  };
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 P, G, M, V;
    if (NT) {  // streamed once per step: keep it out of the way of resident data
      using v4f = __attribute__((ext_vector_type(4))) float;
      auto ld = [](const float4 *q) {
        v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(q));
        return make_float4(t.x, t.y, t.z, t.w);
      };
      P = ld(&p4[i]); G = ld(&g4[i]); M = ld(&m4[i]); V = ld(&v4[i]);
    } else {
      P = p4[i]; G = g4[i]; M = m4[i]; V = v4[i];
    }
    upd(P.x, G.x, M.x, V.x);
    upd(P.y, G.y, M.y, V.y);
    upd(P.z, G.z, M.z, V.z);
    upd(P.w, G.w, M.w, V.w);
    if (NT) {
      using v4f = __attribute__((ext_vector_type(4))) float;
      auto st = [](float4 x, float4 *q) {
        v4f t = {x.x, x.y, x.z, x.w};
        __builtin_nontemporal_store(t, reinterpret_cast<v4f *>(q));
      };
      st(P, &p4[i]); st(M, &m4[i]); st(V, &v4[i]);
    } else {
      p4[i] = P; m4[i] = M; v4[i] = V;
    }
  }
  if (blockIdx.x == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += blockDim.x) {
      float P = p[i], M = m[i], V = v[i];
      upd(P, g[i], M, V);
      p[i] = P;
      m[i] = M;
      v[i] = V;
    }
}

// The same with the gradient kept COMPACT: drows[i, :] = d loss / d logits[idx[i], :] (n x C) — the dense N x C
// gradient (73 MB at the AM shape, all zeros but n rows) is only formed by the backward (k_xent_scatter), scaled by
// the upstream gradient on the way: no dense multiply, and the rows that hold anything are known (row flags).
__global__ __launch_bounds__(1024) void k_xent_rows(const float *__restrict__ logits, int64_t ld, int C,
                                                    const int64_t *__restrict__ idx, const int64_t *__restrict__ target,
                                                    int64_t n, float *__restrict__ loss, float *__restrict__ drows,
                                                    int single_block) {
  float my = 0.f;
  const float inv_n = 1.f / (float)n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // (the next row's index and target are fetched under this row's work: one round trip less per row and thread)
  int64_t row_n = idx[first < n ? first : n - 1], t_n = target[first < n ? first : n - 1];
  for (int64_t i = first; i < n; i += stride) {
    const float *z = logits + row_n * ld;
    const int64_t t = t_n;
    {
      const int64_t nx = i + stride < n ? i + stride : n - 1;
      row_n = idx[nx];
      t_n = target[nx];
    }
    // (the row's loads, softmax and gradient row: xent_row.hpp, shared with nc_batches.hip)
    const XentRow r = xent_row(z, C, t, inv_n, drows ? drows + i * C : nullptr);
    my += (r.lse - r.zt) * inv_n;
  }
  // block sum over up to 16 waves
  __shared__ float s_part[16];
  my = wave_sum(my);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = my;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += s_part[i];
    if (single_block) *loss = t; else atomicAdd(loss, t);
  }
}

// dlogits[idx[i], :] += g * drows[i, :] (a node may be listed twice: atomics), flags[idx[i]] = 1
__global__ void k_xent_scatter(const float *__restrict__ drows, const int64_t *__restrict__ idx, int64_t n, int C,
                               const float *__restrict__ g, float *__restrict__ dlogits, int64_t ldd,
                               uint8_t *__restrict__ flags) {
  const float gg = g ? *g : 1.f;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * C; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / C;
    const int c = (int)(t - i * C);
    const float v = gg * drows[t];
    atomicAdd(&dlogits[idx[i] * ldd + c], v);
    if (flags && c == 0) flags[idx[i]] = 1;
  }
}

// ---- the optimizer tail of the SMALL parameters in two launches --------------------------------------------------
// An epoch's dense parameters besides the node table are a handful of KB-sized tensors (comp tables, W_F, biases,
// the decoder's relations).  One kernel per tensor and phase (sum of squares, Adam) is ~6 us of launch each inside a
// replayed hipGraph — 15 nodes for 5 tensors.  Here: ONE launch squares every tensor, adds the sums that arrived
// from elsewhere (the row-sparse node table's ||g||^2: device doubles), and its last block turns the total into the
// clip coefficient and advances the device step counter; ONE launch applies Adam to all of them.
constexpr int kMultiMax = 16;
struct MultiSumsq {
  const float *g[kMultiMax];
  int64_t n[kMultiMax];
  int32_t blk0[kMultiMax + 1];  // first block of each tensor
  int32_t n_tensors;
  const double *extra[kMultiMax];  // further squared norms to add (device doubles)
  int32_t n_extra;
};
// *accum += the squared norms of up to kMultiMax tensors: the launches in front of k_sumsq_multi when a model has more
// small tensors than one launch takes (an MRGCN with encoders: ~40)
__global__ __launch_bounds__(kTB) void k_sumsq_multi_accum(MultiSumsq a, double *__restrict__ accum) {
  int t = 0;
  while (t + 1 < a.n_tensors && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  const int nb = a.blk0[t + 1] - a.blk0[t], b = blockIdx.x - a.blk0[t];
  const float *x = a.g[t];
  const int64_t n = a.n[t], nv = n >> 2;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float s = 0.f;
  for (int64_t i = (int64_t)b * kTB + threadIdx.x; i < nv; i += (int64_t)nb * kTB) {
    float4 v = x4[i];
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  if (b == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += kTB) s = fmaf(x[i], x[i], s);
  const float tot = block_sum(s);
  if (threadIdx.x == 0 && tot != 0.f) atomicAdd(accum, (double)tot);
}

// `accum` / `ticket` must be zero on entry; the last block leaves them zero again (self-cleaning)
__global__ __launch_bounds__(kTB) void k_sumsq_multi(MultiSumsq a, double *__restrict__ accum,
                                                     unsigned int *__restrict__ ticket, float max_norm,
                                                     double *__restrict__ sumsq_out, float *__restrict__ coef,
                                                     float *__restrict__ norm, int64_t *__restrict__ step, float b1,
                                                     float b2, float *__restrict__ bc) {
  int t = 0;
  while (t + 1 < a.n_tensors && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  const int nb = a.blk0[t + 1] - a.blk0[t], b = blockIdx.x - a.blk0[t];
  const float *x = a.g[t];
  const int64_t n = a.n[t], nv = n >> 2;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float s = 0.f;
  const int64_t stride = (int64_t)nb * kTB;
  for (int64_t i = (int64_t)b * kTB + threadIdx.x; i < nv; i += 4 * stride) {  // four pieces in flight (clamped loads)
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = x4[i + u * stride < nv ? i + u * stride : i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u * stride < nv) {
        s = fmaf(v[u].x, v[u].x, s);
        s = fmaf(v[u].y, v[u].y, s);
        s = fmaf(v[u].z, v[u].z, s);
        s = fmaf(v[u].w, v[u].w, s);
      }
    }
  }
  if (b == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += kTB) s = fmaf(x[i], x[i], s);
  const float tot = block_sum(s);
  if (threadIdx.x == 0) {
    atomicAdd(accum, (double)tot);
    __threadfence();
    const unsigned int seen = atomicAdd(ticket, 1u);
    if (seen == gridDim.x - 1) {  // every block's sum is in
      double total = atomicAdd(accum, 0.0);
      for (int e = 0; e < a.n_extra; ++e) total += *a.extra[e];
      if (sumsq_out) *sumsq_out = total;
      const float nrm = (float)sqrt(total);
      if (coef) {
        const float c = max_norm / (nrm + 1e-6f);
        *coef = (max_norm > 0.f && c < 1.f) ? c : 1.f;
      }
      if (norm) *norm = nrm;
      if (step) {  // ++*step; bc = {1 - b1^step, sqrt(1 - b2^step)} (k_adam_bias)
        const int64_t tt = *step + 1;
        *step = tt;
        bc[0] = (float)(1.0 - pow((double)b1, (double)tt));
        bc[1] = (float)sqrt(1.0 - pow((double)b2, (double)tt));
      }
      *accum = 0.0;
      *ticket = 0u;
    }
  }
}

// ---- the same squared norms in a fixed order (torch.use_deterministic_algorithms(True)) -------------------------------
// A block's float sum (block_sum: a fixed tree) becomes a double partial; the last block to take a ticket adds the
// partials in block order.  Grids are functions of the sizes only.  `partials`: >= mrgcn_sumsq_det_workspace() bytes;
// `ticket` is zero at the first call and left zero.
constexpr int kDetMaxBlocks = kMultiMax * 64;
__device__ __forceinline__ float sumsq_part(const float *__restrict__ x, int64_t n, int b, int nb) {
  const int64_t nv = n >> 2;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float s = 0.f;
  const int64_t stride = (int64_t)nb * kTB;
  for (int64_t i = (int64_t)b * kTB + threadIdx.x; i < nv; i += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = x4[i + u * stride < nv ? i + u * stride : i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u * stride < nv) {
        s = fmaf(v[u].x, v[u].x, s);
        s = fmaf(v[u].y, v[u].y, s);
        s = fmaf(v[u].z, v[u].z, s);
        s = fmaf(v[u].w, v[u].w, s);
      }
    }
  }
  if (b == 0)
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += kTB) s = fmaf(x[i], x[i], s);
  return block_sum(s);
}
// thread 0: publish this block's partial; true in the block that arrives last (which then sees every partial)
__device__ __forceinline__ bool det_last_block(double part, double *__restrict__ partials,
                                               unsigned int *__restrict__ ticket) {
  partials[blockIdx.x] = part;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned int seen = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (seen != gridDim.x - 1) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return true;
}
__device__ __forceinline__ double det_ordered_sum(const double *__restrict__ partials, unsigned int *__restrict__ ticket) {
  double t = 0.0;
  for (unsigned int b = 0; b < gridDim.x; ++b) t += partials[b];
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return t;
}
__device__ __forceinline__ int multi_tensor_of(const MultiSumsq &a) {
  int t = 0;
  while (t + 1 < a.n_tensors && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  return t;
}

__global__ __launch_bounds__(kTB) void k_sumsq_det(const float *__restrict__ x, int64_t n, double *__restrict__ accum,
                                                   double *__restrict__ partials, unsigned int *__restrict__ ticket) {
  const float t = sumsq_part(x, n, blockIdx.x, gridDim.x);
  if (threadIdx.x == 0 && det_last_block((double)t, partials, ticket)) *accum += det_ordered_sum(partials, ticket);
}

__global__ __launch_bounds__(kTB) void k_sumsq_multi_accum_det(MultiSumsq a, double *__restrict__ accum,
                                                               double *__restrict__ partials,
                                                               unsigned int *__restrict__ ticket) {
  const int t = multi_tensor_of(a);
  const float s = sumsq_part(a.g[t], a.n[t], blockIdx.x - a.blk0[t], a.blk0[t + 1] - a.blk0[t]);
  if (threadIdx.x == 0 && det_last_block((double)s, partials, ticket)) *accum += det_ordered_sum(partials, ticket);
}

__global__ __launch_bounds__(kTB) void k_sumsq_multi_det(MultiSumsq a, double *__restrict__ accum,
                                                         unsigned int *__restrict__ ticket, float max_norm,
                                                         double *__restrict__ sumsq_out, float *__restrict__ coef,
                                                         float *__restrict__ norm, int64_t *__restrict__ step, float b1,
                                                         float b2, float *__restrict__ bc,
                                                         double *__restrict__ partials) {
  const int t = multi_tensor_of(a);
  const float s = sumsq_part(a.g[t], a.n[t], blockIdx.x - a.blk0[t], a.blk0[t + 1] - a.blk0[t]);
  if (threadIdx.x == 0 && det_last_block((double)s, partials, ticket)) {
    double total = *accum + det_ordered_sum(partials, ticket);
    for (int e = 0; e < a.n_extra; ++e) total += *a.extra[e];
    if (sumsq_out) *sumsq_out = total;
    const float nrm = (float)sqrt(total);
    if (coef) {
      const float c = max_norm / (nrm + 1e-6f);
      *coef = (max_norm > 0.f && c < 1.f) ? c : 1.f;
    }
    if (norm) *norm = nrm;
    if (step) {
      const int64_t tt = *step + 1;
      *step = tt;
      bc[0] = (float)(1.0 - pow((double)b1, (double)tt));
      bc[1] = (float)sqrt(1.0 - pow((double)b2, (double)tt));
    }
    *accum = 0.0;
  }
}

struct MultiAdam {
  float *p[kMultiMax];
  const float *g[kMultiMax];
  float *m[kMultiMax];
  float *v[kMultiMax];
  int64_t n[kMultiMax];
  float lr[kMultiMax], wd[kMultiMax];
  int32_t blk0[kMultiMax + 1];
  int32_t n_tensors;
};
__global__ __launch_bounds__(kTB) void k_adam_multi(MultiAdam a, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                    const float *__restrict__ scale, const float *__restrict__ bc_dev) {
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  int t = 0;
  while (t + 1 < a.n_tensors && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  const int nb = a.blk0[t + 1] - a.blk0[t], b = blockIdx.x - a.blk0[t];
  float *p = a.p[t];
  const float *g = a.g[t];
  float *m = a.m[t], *v = a.v[t];
  const int64_t n = a.n[t];
  const float sc = scale ? *scale : 1.f, wd = a.wd[t];
  const float step = a.lr[t] / bc1;
  for (int64_t i = (int64_t)b * kTB + threadIdx.x; i < n; i += (int64_t)nb * kTB) {  // == k_adam's update
    float gg = g[i] * sc, pp = p[i], mm = m[i], vv = v[i];
    if (wd != 0.f) gg = fmaf(wd, pp, gg);
    mm = fmaf(b1, mm, (1.f - b1) * gg);
    vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

// ---- L1 / L2 weight penalties on dense and flagged-row parameters (tasks/link_prediction.py:306-326) -----------------
// The reference adds l1 sum|p| + l2 sum p^2 over the `weight*` parameters to the loss, so r(p) = l1 sgn(p) + 2 l2 p is
// part of every such gradient when clip_grad_norm_ looks at it.  Two launches over a list of <= kMultiMax tensors do
// that without touching the gradients: k_penalty_norm_multi sums (g + r(p))^2, |p| and p^2; k_adam_reg_multi is
// k_adam_multi's update on gg = (g + r(p)) scale + wd p.  A tensor may carry row flags: row i of its gradient buffer
// counts only where flags[i] != 0, and the other rows of the buffer are never read (a flagged-off load reads the
// parameter's own piece instead and a select drops it).  Both are one-shot over their tensors: a block owns a
// contiguous tile whose size depends on the tensor's size only, every load of a step is issued before the first use.
constexpr int kPenMaxBlocks = 4096;         // blocks of one norm launch (its partials: 3 doubles each)
constexpr int kPenTensorBlocks = 1024;      // blocks one tensor may take of them
constexpr int64_t kPenTile = 4 * 4 * kTB;   // floats of a block's smallest tile: four 16-byte pieces per thread
constexpr int kPenSumChunk = 1024;          // partials per sum the last block stages in LDS at a time
struct MultiPen {
  const float *p[kMultiMax];
  const float *g[kMultiMax];          // nullable: no gradient this step
  const uint8_t *flags[kMultiMax];    // nullable: every row counts
  int64_t n[kMultiMax];
  int64_t per_block[kMultiMax];       // floats per block: a multiple of kPenTile
  int32_t row_len[kMultiMax];
  int32_t vec[kMultiMax];             // 16-byte pieces (aligned bases, rows of whole pieces)
  int32_t blk0[kMultiMax + 1];
  int32_t n_tensors;
};
__device__ __forceinline__ float pen_grad(float p, float l1, float l2x2) {  // l1 sgn(p) + 2 l2 p, sgn(0) = 0
  const float sg = (float)(p > 0.f) - (float)(p < 0.f);
  return fmaf(l2x2, p, l1 * sg);
}
// the row of 16-byte piece q (rows of rl4 pieces) / of element i
__device__ __forceinline__ int64_t pen_row(int64_t i, int32_t len) {
  return i <= 0x7fffffffLL ? (int64_t)((uint32_t)i / (uint32_t)len) : i / len;
}

__global__ __launch_bounds__(kTB) void k_penalty_norm_multi(MultiPen a, float l1, float l2x2, int pen,
                                                            double *__restrict__ out3, double *__restrict__ partials,
                                                            unsigned int *__restrict__ ticket) {
  int t = 0;
  while (t + 1 < a.n_tensors && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  const int b = blockIdx.x - a.blk0[t];
  const float *__restrict__ p = a.p[t];
  const float *__restrict__ g = a.g[t];
  const uint8_t *__restrict__ fl = a.flags[t];
  const int64_t n = a.n[t], per = a.per_block[t];
  const int32_t len = a.row_len[t];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  auto add = [&](float pp, float gg) {
    const float x = pen ? gg + pen_grad(pp, l1, l2x2) : gg;
    s0 = fmaf(x, x, s0);
    s1 += fabsf(pp);
    s2 = fmaf(pp, pp, s2);
  };
  if (a.vec[t]) {
    const int64_t nv = n >> 2, q0 = ((int64_t)b * per) >> 2, q1 = min(q0 + (per >> 2), nv);
    const int32_t rl4 = len >> 2;
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 4 * kTB) {
      int64_t qq[4];
      bool on[4];
      float4 P[4], G[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) qq[u] = q + u * kTB < q1 ? q + u * kTB : q;
#pragma unroll
      for (int u = 0; u < 4; ++u) on[u] = g != nullptr && (fl == nullptr || fl[pen_row(qq[u], rl4)] != 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) P[u] = p4[qq[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) G[u] = (on[u] ? g4 : p4)[qq[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (q + u * kTB < q1) {
          add(P[u].x, on[u] ? G[u].x : 0.f);
          add(P[u].y, on[u] ? G[u].y : 0.f);
          add(P[u].z, on[u] ? G[u].z : 0.f);
          add(P[u].w, on[u] ? G[u].w : 0.f);
        }
      }
    }
    if (b == 0)  // (a flagged tensor has rows of whole pieces: no tail)
      for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += kTB) add(p[i], g ? g[i] : 0.f);
  } else {
    const int64_t e0 = (int64_t)b * per, e1 = min(e0 + per, n);
    for (int64_t i = e0 + threadIdx.x; i < e1; i += 4 * kTB) {
      int64_t ii[4];
      bool on[4];
      float P[4], G[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ii[u] = i + u * kTB < e1 ? i + u * kTB : i;
#pragma unroll
      for (int u = 0; u < 4; ++u) on[u] = g != nullptr && (fl == nullptr || fl[pen_row(ii[u], len)] != 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) P[u] = p[ii[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) G[u] = (on[u] ? g : p)[ii[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u * kTB < e1) add(P[u], on[u] ? G[u] : 0.f);
    }
  }
  // the *_det scheme: a fixed float tree per block -> double partials -> added in block order by the last block
  const float t0 = block_sum(s0), t1 = block_sum(s1), t2 = block_sum(s2);
  __shared__ int s_last;
  __shared__ double s_stage[3][kPenSumChunk];
  const unsigned int nb = gridDim.x;
  if (threadIdx.x == 0) {
    partials[(int64_t)nb + blockIdx.x] = (double)t1;
    partials[2 * (int64_t)nb + blockIdx.x] = (double)t2;
    s_last = det_last_block((double)t0, partials, ticket) ? 1 : 0;  // (its release covers the two stores above)
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double tot = 0.0;
  for (unsigned int c0 = 0; c0 < nb; c0 += kPenSumChunk) {
    const unsigned int m = min(nb - c0, (unsigned int)kPenSumChunk);
    __syncthreads();
    for (unsigned int k = threadIdx.x; k < 3 * m; k += kTB) s_stage[k / m][k % m] = partials[(int64_t)(k / m) * nb + c0 + k % m];
    __syncthreads();
    if (threadIdx.x < 3)
      for (unsigned int k = 0; k < m; ++k) tot += s_stage[threadIdx.x][k];
  }
  if (threadIdx.x < 3) out3[threadIdx.x] += tot;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct MultiAdamReg {
  float *p[kMultiMax];
  const float *g[kMultiMax];
  const uint8_t *flags[kMultiMax];
  float *m[kMultiMax];
  float *v[kMultiMax];
  int64_t n[kMultiMax];
  float lr[kMultiMax], wd[kMultiMax];
  int32_t row_len[kMultiMax];
  int32_t vec[kMultiMax];
  int64_t blk0[kMultiMax + 1];
  int32_t n_tensors;
};
constexpr int kAdamRegPieces = 2;  // 16-byte pieces (or floats, on the scalar path) per thread
__global__ __launch_bounds__(kTB) void k_adam_reg_multi(MultiAdamReg a, float l1, float l2x2, int pen, float b1, float b2,
                                                        float eps, float bc1, float bc2_sqrt,
                                                        const float *__restrict__ scale,
                                                        const float *__restrict__ bc_dev) {
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  int t = 0;
  while (t + 1 < a.n_tensors && (int64_t)blockIdx.x >= a.blk0[t + 1]) ++t;
  const int64_t b = (int64_t)blockIdx.x - a.blk0[t];
  float *__restrict__ p = a.p[t];
  const float *__restrict__ g = a.g[t];
  const uint8_t *__restrict__ fl = a.flags[t];
  float *__restrict__ m = a.m[t];
  float *__restrict__ v = a.v[t];
  const int64_t n = a.n[t];
  const int32_t len = a.row_len[t];
  const float sc = scale ? *scale : 1.f, wd = a.wd[t];
  const float step = a.lr[t] / bc1;
  auto upd = [&](float &pp, float g0, float &mm, float &vv) {  // k_adam_multi's update on (g + r(p)) scale + wd p
    float gg = (pen ? g0 + pen_grad(pp, l1, l2x2) : g0) * sc;
    if (wd != 0.f) gg = fmaf(wd, pp, gg);
    mm = fmaf(b1, mm, (1.f - b1) * gg);
    vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
  };
  constexpr int U = kAdamRegPieces;
  if (a.vec[t]) {
    const int64_t nv = n >> 2, q = b * (U * kTB) + threadIdx.x;
    const int32_t rl4 = len >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float4 *m4 = reinterpret_cast<float4 *>(m);
    float4 *v4 = reinterpret_cast<float4 *>(v);
    if (q < nv) {
      int64_t qq[U];
      bool on[U];
      float4 P[U], G[U], M[U], V[U];
#pragma unroll
      for (int u = 0; u < U; ++u) qq[u] = q + u * kTB < nv ? q + u * kTB : q;
#pragma unroll
      for (int u = 0; u < U; ++u) on[u] = g != nullptr && (fl == nullptr || fl[pen_row(qq[u], rl4)] != 0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        P[u] = p4[qq[u]];
        M[u] = m4[qq[u]];
        V[u] = v4[qq[u]];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) G[u] = (on[u] ? g4 : reinterpret_cast<const float4 *>(p))[qq[u]];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u == 0 || q + u * kTB < nv) {
          upd(P[u].x, on[u] ? G[u].x : 0.f, M[u].x, V[u].x);
          upd(P[u].y, on[u] ? G[u].y : 0.f, M[u].y, V[u].y);
          upd(P[u].z, on[u] ? G[u].z : 0.f, M[u].z, V[u].z);
          upd(P[u].w, on[u] ? G[u].w : 0.f, M[u].w, V[u].w);
          p4[qq[u]] = P[u];
          m4[qq[u]] = M[u];
          v4[qq[u]] = V[u];
        }
      }
    }
    if (b == 0)
      for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += kTB) {
        float P = p[i], M = m[i], V = v[i];
        upd(P, g ? g[i] : 0.f, M, V);
        p[i] = P;
        m[i] = M;
        v[i] = V;
      }
  } else {
    const int64_t i = b * (U * kTB) + threadIdx.x;
    if (i >= n) return;
    int64_t ii[U];
    bool on[U];
    float P[U], G[U], M[U], V[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ii[u] = i + u * kTB < n ? i + u * kTB : i;
#pragma unroll
    for (int u = 0; u < U; ++u) on[u] = g != nullptr && (fl == nullptr || fl[pen_row(ii[u], len)] != 0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      P[u] = p[ii[u]];
      M[u] = m[ii[u]];
      V[u] = v[ii[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) G[u] = (on[u] ? g : (const float *)p)[ii[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u == 0 || i + u * kTB < n) {
        upd(P[u], on[u] ? G[u] : 0.f, M[u], V[u]);
        p[ii[u]] = P[u];
        m[ii[u]] = M[u];
        v[ii[u]] = V[u];
      }
    }
  }
}

// mean cross-entropy over labelled rows + its gradient w.r.t. the logits.
// one thread per labelled row (C is small: the number of classes)
__global__ void k_xent(const float *__restrict__ logits, int64_t ld, int C,
                       const int64_t *__restrict__ idx, const int64_t *__restrict__ target, int64_t n,
                       float *__restrict__ loss, float *__restrict__ dlogits, int64_t ldd) {
  float my = 0.f;
  const float inv_n = 1.f / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float *z = logits + idx[i] * ld;
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
    const float lse = logf(se) + mx;
    const int64_t t = target[i];
    my += (lse - z[t]) * inv_n;
    if (dlogits) {
      float *d = dlogits + idx[i] * ldd;
      for (int c = 0; c < C; ++c) {
        float pr = expf(z[c] - lse);
        atomicAdd(&d[c], (pr - (c == t ? 1.f : 0.f)) * inv_n);  // a node may be listed twice
      }
    }
  }
  float t = block_sum(my);
  if (threadIdx.x == 0) atomicAdd(loss, t);
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

namespace mrgcn {
// Streaming yardsticks (measurement only: bench.py's extra.device_copy_gbps_hip / extra.triad_gbps): what a plain
// float4 copy and a 3-read / 3-write elementwise pass (the memory shape of a dense Adam step) reach on the box.
using yf4 = __attribute__((ext_vector_type(4))) float;
__global__ __launch_bounds__(256) void k_probe_copy4(const yf4 *__restrict__ a, yf4 *__restrict__ b, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) b[i] = a[i];
}
template <bool NT>
__global__ __launch_bounds__(256) void k_probe_triad4(yf4 *__restrict__ p, yf4 *__restrict__ m, yf4 *__restrict__ v,
                                                      int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    yf4 P, M, V;
    if (NT) { P = __builtin_nontemporal_load(p + i); M = __builtin_nontemporal_load(m + i); V = __builtin_nontemporal_load(v + i); }
    else { P = p[i]; M = m[i]; V = v[i]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // Adam's arithmetic on a constant gradient
      const float g = 1e-3f;
      M[k] = fmaf(0.9f, M[k], 0.1f * g);
      V[k] = fmaf(0.999f, V[k], 0.001f * g * g);
      P[k] -= 0.01f * (M[k] / (sqrtf(V[k]) + 1e-8f));
    }
    if (NT) { __builtin_nontemporal_store(P, p + i); __builtin_nontemporal_store(M, m + i); __builtin_nontemporal_store(V, v + i); }
    else { p[i] = P; m[i] = M; v[i] = V; }
  }
}
}  // namespace mrgcn

namespace mrgcn {
// dst[row, 0:F] = src[perm[k], 0:F] where row == sorted_rows[k], zeros for every other row: the dense gradient of a
// table of which only some rows received any (the literal (R*N) x out weight_I of a layer without bases: autograd of
// graph.py:75 — torch produced it as zeros_like + index_copy_, two passes over the table).  A lane group per row, a
// binary search in the sorted list of touched rows (cache resident), one pass over dst.
__global__ __launch_bounds__(256) void k_scatter_rows_zero_fill(const int32_t *__restrict__ sorted_rows,
                                                                const int32_t *__restrict__ perm, int64_t n_touched,
                                                                const float *__restrict__ src, int64_t ldS, int F,
                                                                float *__restrict__ dst, int64_t n_rows) {
  const int P = (F + 3) >> 2;  // 16-byte pieces of a row
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / P;
  const int piece = (int)(t - row * P);
  if (row >= n_rows) return;
  int64_t lo = 0, hi = n_touched;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_rows[mid] < row) lo = mid + 1; else hi = mid;
  }
  const bool hit = lo < n_touched && sorted_rows[lo] == row;
  const float *s = hit ? src + (int64_t)perm[lo] * ldS : nullptr;
  float *d = dst + row * F;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int f = 4 * piece + u;
    if (f < F) d[f] = hit ? s[f] : 0.f;
  }
}
// out[f] = sum over the rows m of X[m][f] (rows with row_flags[m] == 0 are neither read nor added): the bias gradient of a
// narrow layer (autograd of `AFW + self.b`, graph.py:98-101) — torch's reduction of a 1.67 M x 10 matrix along its
// long side runs at 0.12 TB/s (0.55 ms); this is one coalesced pass and a fixed-order sum of the blocks' partials.
constexpr int kColsumBlocks = 1024;
template <int FT>
__global__ __launch_bounds__(256) void k_colsum_rows(const float *__restrict__ X, int64_t ld, int64_t M, int F,
                                                     const uint8_t *__restrict__ row_flags,
                                                     float *__restrict__ partials /* [gridDim.x][FT] */) {
  float acc[FT];
#pragma unroll
  for (int f = 0; f < FT; ++f) acc[f] = 0.f;
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    if (row_flags && !row_flags[m]) continue;
    const float *row = X + m * ld;
#pragma unroll
    for (int f = 0; f < FT; ++f)
      if (f < F) acc[f] += row[f];
  }
  __shared__ float s_part[4][FT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    float v = acc[f];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) s_part[wv][f] = v;
  }
  __syncthreads();
  if (threadIdx.x < FT)
    partials[(int64_t)blockIdx.x * FT + threadIdx.x] =
        (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

template <int FT>
__global__ __launch_bounds__(64) void k_colsum_final(const float *__restrict__ partials, int n_blocks, int F,
                                                     float *__restrict__ out) {
  // lane (f, q): column f, blocks q, q + 64 / FT, ... in order; the q sums meet through a fixed butterfly
  constexpr int Q = 64 / FT;
  const int f = threadIdx.x % FT, q = threadIdx.x / FT;
  float v = 0.f;
  for (int b = q; b < n_blocks; b += 8 * Q) {  // eight loads in flight (one at a time: 60 us for 1 024 partials), same order
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = partials[(int64_t)(b + u * Q < n_blocks ? b + u * Q : b) * FT + f];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (b + u * Q < n_blocks) v += x[u];
  }
#pragma unroll
  for (int off = FT; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  if (q == 0 && f < F) out[f] = v;
}
}  // namespace mrgcn

extern "C" {

int mrgcn_scatter_rows_zero_fill_f32(const int32_t *sorted_rows, const int32_t *perm, int64_t n_touched,
                                     const float *src, int64_t ldS, int32_t F, float *dst, int64_t n_rows, void *stream) {
  MRGCN_REQUIRE(dst && n_rows >= 0 && F > 0 && n_touched >= 0, "NULL / sizes");
  MRGCN_REQUIRE(n_touched == 0 || (sorted_rows && perm && src && ldS >= F), "NULL / ldS");
  if (n_rows == 0) return MRGCN_OK;
  const int64_t threads = n_rows * ((F + 3) / 4);
  mrgcn::k_scatter_rows_zero_fill<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
      sorted_rows, perm, n_touched, src, ldS, F, dst, n_rows);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_colsum_rows_workspace(int32_t F) { return F > 0 && F <= 16 ? (int64_t)mrgcn::kColsumBlocks * 16 : -1; }

int mrgcn_colsum_rows_f32(const float *X, int64_t ld, int64_t M, int32_t F, const uint8_t *row_flags, float *out,
                          float *workspace, int64_t workspace_floats, void *stream) {
  MRGCN_REQUIRE(X && out && workspace, "NULL");
  MRGCN_REQUIRE(F > 0 && F <= 16 && ld >= F && M >= 0, "F (1..16) / ld / M");
  MRGCN_REQUIRE(workspace_floats >= mrgcn_colsum_rows_workspace(F), "workspace (mrgcn_colsum_rows_workspace floats)");
  hipStream_t s = (hipStream_t)stream;
  int blocks = (int)std::min<int64_t>(mrgcn::kColsumBlocks, (M + 255) / 256);
  if (blocks < 1) blocks = 1;
  if (F <= 4) {
    mrgcn::k_colsum_rows<4><<<dim3(blocks), dim3(256), 0, s>>>(X, ld, M, F, row_flags, workspace);
    mrgcn::k_colsum_final<4><<<dim3(1), dim3(64), 0, s>>>(workspace, blocks, F, out);
  } else if (F <= 8) {
    mrgcn::k_colsum_rows<8><<<dim3(blocks), dim3(256), 0, s>>>(X, ld, M, F, row_flags, workspace);
    mrgcn::k_colsum_final<8><<<dim3(1), dim3(64), 0, s>>>(workspace, blocks, F, out);
  } else {
    mrgcn::k_colsum_rows<16><<<dim3(blocks), dim3(256), 0, s>>>(X, ld, M, F, row_flags, workspace);
    mrgcn::k_colsum_final<16><<<dim3(1), dim3(64), 0, s>>>(workspace, blocks, F, out);
  }
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

// The yardsticks as ONE-SHOT grids (a thread per 16-byte piece): what the memory system gives a stream whose work is
// handed out in address order by the block dispatcher — 6.25 TB/s (copy) / 6.0 TB/s (triad, nontemporal) on the bench
// boxes, MI355X_MICROARCH.md's 6.29.  The `_persistent` forms are round 5's (2 048 resident blocks striding through
// the arrays: 4.8 / 4.9 TB/s): the shape a kernel with per-block state is stuck with (tools/lab/copy_lab.hip).
int mrgcn_probe_copy_f32(const float *src, float *dst, int64_t n, void *stream) {
  MRGCN_REQUIRE(src && dst && n >= 0 && n % 4 == 0, "NULL / n % 4");
  MRGCN_REQUIRE(((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  const int64_t n4 = n / 4;
  mrgcn::k_probe_copy4<<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
      (const mrgcn::yf4 *)src, (mrgcn::yf4 *)dst, n4);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_probe_copy_persistent_f32(const float *src, float *dst, int64_t n, void *stream) {
  MRGCN_REQUIRE(src && dst && n >= 0 && n % 4 == 0, "NULL / n % 4");
  MRGCN_REQUIRE(((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  mrgcn::k_probe_copy4<<<dim3(256 * 8), dim3(256), 0, (hipStream_t)stream>>>((const mrgcn::yf4 *)src, (mrgcn::yf4 *)dst, n / 4);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_probe_triad_persistent_f32(float *p, float *m, float *v, int64_t n, void *stream) {
  MRGCN_REQUIRE(p && m && v && n >= 0 && n % 4 == 0, "NULL / n % 4");
  MRGCN_REQUIRE(((((uintptr_t)p) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  mrgcn::k_probe_triad4<false><<<dim3(256 * 8), dim3(256), 0, (hipStream_t)stream>>>((mrgcn::yf4 *)p, (mrgcn::yf4 *)m, (mrgcn::yf4 *)v, n / 4);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_probe_triad_f32(float *p, float *m, float *v, int64_t n, void *stream) {
  MRGCN_REQUIRE(p && m && v && n >= 0 && n % 4 == 0, "NULL / n % 4");
  MRGCN_REQUIRE(((((uintptr_t)p) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  const int64_t n4 = n / 4;
  mrgcn::k_probe_triad4<true><<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>((mrgcn::yf4 *)p, (mrgcn::yf4 *)m, (mrgcn::yf4 *)v, n4);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_relu_bwd_f32(const float *dY, const float *Y, int64_t n, float *out, void *stream) {
  MRGCN_REQUIRE(dY && Y && out, "NULL");
  MRGCN_REQUIRE((((uintptr_t)dY | (uintptr_t)Y | (uintptr_t)out) & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  k_relu_bwd<<<dim3(stream_grid(n >> 2)), dim3(kTB), 0, (hipStream_t)stream>>>(dY, Y, n, out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_relu_bwd_rows_f32(const float *dY, int64_t ld_dY, const float *Y, int64_t ldY, int64_t rows, int32_t F,
                            float *out, int64_t ld_out, void *stream) {
  MRGCN_REQUIRE(dY && Y && out, "NULL");
  MRGCN_REQUIRE(rows >= 0 && F > 0 && ld_dY >= F && ldY >= F && ld_out >= F, "F / leading dimensions");
  if (rows == 0) return MRGCN_OK;
  k_relu_bwd_rows<<<dim3(stream_grid(rows * 16)), dim3(kTB), 0, (hipStream_t)stream>>>(dY, ld_dY, Y, ldY, rows, F, out,
                                                                                      ld_out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_rows_nonzero_f32(const float *X, int64_t ld, int32_t F, int64_t nrows, uint8_t *flags,
                           void *stream) {
  MRGCN_REQUIRE(X && flags, "NULL");
  MRGCN_REQUIRE(F > 0 && ld >= F, "F / ld");
  if (nrows == 0) return MRGCN_OK;
  const int vec_ok = (ld % 4 == 0) && (((uintptr_t)X & 15) == 0);
  if (F > 32) k_rows_nonzero_wide<<<dim3(stream_grid(nrows * 64)), dim3(256), 0, (hipStream_t)stream>>>(X, ld, F, nrows, flags);
  else k_rows_nonzero<<<dim3(stream_grid(nrows)), dim3(kTB), 0, (hipStream_t)stream>>>(X, ld, F, nrows, flags, vec_ok);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_sumsq_accum_f32(const float *x, int64_t n, double *accum, void *stream) {
  MRGCN_REQUIRE(x && accum, "NULL");
  MRGCN_REQUIRE(((uintptr_t)x & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  k_sumsq<<<dim3(std::min(stream_grid(((n >> 2) + 3) / 4), 512)), dim3(kTB), 0, (hipStream_t)stream>>>(x, n, accum);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_clip_coef_f32(const double *sumsq, float max_norm, float *coef, float *norm, void *stream) {
  MRGCN_REQUIRE(sumsq && coef, "NULL");
  k_clip_coef<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(sumsq, max_norm, coef, norm);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

static int adam_impl(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int64_t step,
                     const float *grad_scale, const float *bc_dev, void *stream);

int mrgcn_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, float weight_decay,
                        int64_t step, const float *grad_scale, void *stream) {
  return adam_impl(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                   nullptr, stream);
}

static int adam_impl(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int64_t step,
                     const float *grad_scale, const float *bc_dev, void *stream) {
  MRGCN_REQUIRE(param && grad && exp_avg && exp_avg_sq, "NULL");
  MRGCN_REQUIRE(step >= 1, "step counts from 1");
  MRGCN_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int nt_mode = (int)cfg(CFG_ADAM_NT);
  const int grid_cap = (int)cfg(CFG_ADAM_GRID);
  int64_t blocks = ((n >> 2) + kTB - 1) / kTB;
  if (blocks < 1) blocks = 1;
  if (blocks > grid_cap) blocks = grid_cap;
  if (nt_mode)
    k_adam<true><<<dim3((unsigned)blocks), dim3(kTB), 0, (hipStream_t)stream>>>(
        param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, (float)bc1,
        (float)sqrt(bc2), grad_scale, bc_dev);
  else
    k_adam<false><<<dim3((unsigned)blocks), dim3(kTB), 0, (hipStream_t)stream>>>(
        param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, (float)bc1,
        (float)sqrt(bc2), grad_scale, bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"

namespace mrgcn {
namespace {
// step counter and Adam bias corrections on the device: ++*step; bc = {1 - b1^step, sqrt(1 - b2^step)}
__global__ void k_adam_bias(int64_t *__restrict__ step, float b1, float b2, float *__restrict__ bc) {
  const int64_t t = *step + 1;
  *step = t;
  bc[0] = (float)(1.0 - pow((double)b1, (double)t));
  bc[1] = (float)sqrt(1.0 - pow((double)b2, (double)t));
}
}  // namespace
}  // namespace mrgcn

extern "C" {

int mrgcn_adam_step_rows_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t nrows,
                             int32_t rowlen, const uint8_t *row_cur, uint8_t *row_ever, float lr, float beta1,
                             float beta2, float eps, int64_t step, const float *bc_dev, const float *grad_scale,
                             void *stream) {
  MRGCN_REQUIRE(param && grad && exp_avg && exp_avg_sq && row_cur && row_ever, "NULL");
  MRGCN_REQUIRE(step >= 1 || bc_dev, "step counts from 1");
  MRGCN_REQUIRE(nrows >= 0 && rowlen > 0, "nrows / rowlen");
  if (nrows == 0) return MRGCN_OK;
  const double bc1 = bc_dev ? 1.0 : 1.0 - pow((double)beta1, (double)step);
  const double bc2 = bc_dev ? 1.0 : 1.0 - pow((double)beta2, (double)step);
  const int rowlen4 = rowlen >> 2;
  hipStream_t s = (hipStream_t)stream;
  if (rowlen % 4 != 0 ||
      ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)) {
    int64_t blocks = (nrows * rowlen + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    mrgcn::k_adam_rows_scalar<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(
        param, grad, exp_avg, exp_avg_sq, nrows, rowlen, row_cur, row_ever, lr, beta1, beta2, eps, (float)bc1,
        (float)sqrt(bc2), grad_scale, bc_dev);
    mrgcn::k_rows_mark_ever<<<dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s>>>(row_cur, row_ever, nrows);
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  // rows per block step: about 2 float4s per thread
#define ROWS_GO(RB_)                                                                                        \
  do {                                                                                                      \
    int64_t blocks = (nrows + RB_ - 1) / RB_;                                                               \
    if (blocks > 8192) blocks = 8192;                                                                       \
    mrgcn::k_adam_rows<RB_><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(                                   \
        param, grad, exp_avg, exp_avg_sq, nrows, rowlen4, row_cur, row_ever, lr, beta1, beta2, eps,         \
        (float)bc1, (float)sqrt(bc2), grad_scale, bc_dev);                                                  \
  } while (0)
  if (rowlen4 >= 256) ROWS_GO(1);
  else if (rowlen4 >= 64) ROWS_GO(4);
  else if (rowlen4 >= 16) ROWS_GO(16);
  else ROWS_GO(64);
#undef ROWS_GO
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_adam_step_index_rows_f32(float *param, const float *grad, int64_t ld_grad, float *exp_avg,
                                   float *exp_avg_sq, const int32_t *index, int64_t n_index, int32_t rowlen, float lr,
                                   float beta1, float beta2, float eps, int64_t step, const float *bc_dev,
                                   const float *grad_scale, void *stream) {
  MRGCN_REQUIRE(param && grad && exp_avg && exp_avg_sq && index, "NULL");
  MRGCN_REQUIRE(step >= 1 || bc_dev, "step counts from 1");
  MRGCN_REQUIRE(n_index >= 0 && rowlen > 0 && rowlen % 4 == 0 && ld_grad >= rowlen && ld_grad % 4 == 0,
                "rows of whole 16-byte pieces (rowlen, ld_grad multiples of 4)");
  MRGCN_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "param / grad / moments must be 16-byte aligned");
  if (n_index == 0) return MRGCN_OK;
  const double bc1 = bc_dev ? 1.0 : 1.0 - pow((double)beta1, (double)step);
  const double bc2 = bc_dev ? 1.0 : 1.0 - pow((double)beta2, (double)step);
  const int rowlen4 = rowlen >> 2;
  const int64_t blocks = (n_index * rowlen4 + 255) / 256;
  MRGCN_REQUIRE(blocks <= 0x7fffffff, "too many rows for one launch");
  mrgcn::k_adam_index_rows<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
      param, grad, ld_grad >> 2, exp_avg, exp_avg_sq, index, n_index, rowlen4, lr, beta1, beta2, eps, (float)bc1,
      (float)sqrt(bc2), grad_scale, bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_adam_bias_f32(int64_t *step_dev, float beta1, float beta2, float *bc_dev, void *stream) {
  MRGCN_REQUIRE(step_dev && bc_dev, "NULL");
  mrgcn::k_adam_bias<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(step_dev, beta1, beta2, bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_adam_step_dev_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay,
                            const float *bc_dev, const float *grad_scale, void *stream) {
  MRGCN_REQUIRE(bc_dev, "bc_dev is NULL");
  return adam_impl(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, 1, grad_scale,
                   bc_dev, stream);
}

int mrgcn_softmax_xent_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx,
                           const int64_t *target, int64_t n, float *loss, float *dlogits,
                           int64_t ldd, int64_t num_rows, void *stream) {
  MRGCN_REQUIRE(logits && idx && target && loss, "NULL");
  MRGCN_REQUIRE(C > 0 && ld >= C && n > 0, "C / ld / n");
  hipStream_t s = (hipStream_t)stream;
  MRGCN_HIP_TRY(mrgcn::fill_async(loss, 0, sizeof(float), s));
  if (dlogits) {
    MRGCN_REQUIRE(ldd >= C && num_rows > 0, "ldd / num_rows");
    MRGCN_HIP_TRY(mrgcn::fill_async(dlogits, 0, (size_t)num_rows * ldd * sizeof(float), s));
  }
  int grid = (int)((n + kTB - 1) / kTB);
  if (grid > 1024) grid = 1024;
  k_xent<<<dim3(grid), dim3(kTB), 0, s>>>(logits, ld, C, idx, target, n, loss, dlogits, ldd);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}


int mrgcn_softmax_xent_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx, const int64_t *target,
                                int64_t n, float *loss, float *drows, void *stream) {
  MRGCN_REQUIRE(logits && idx && target && loss, "NULL");
  MRGCN_REQUIRE(C > 0 && ld >= C && n > 0, "C / ld / n");
  hipStream_t s = (hipStream_t)stream;
  const int single = n <= 16384;
  if (!single) MRGCN_HIP_TRY(mrgcn::fill_async(loss, 0, sizeof(float), s));
  int grid = single ? 1 : (int)((n + 1023) / 1024);
  if (grid > 256) grid = 256;
  mrgcn::k_xent_rows<<<dim3(grid), dim3(1024), 0, s>>>(logits, ld, C, idx, target, n, loss, drows, single);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_softmax_xent_bwd_f32(const float *drows, const int64_t *idx, int64_t n, int32_t C, const float *g,
                               float *dlogits, int64_t ldd, int64_t num_rows, uint8_t *row_flags, void *stream) {
  MRGCN_REQUIRE(drows && idx && dlogits, "NULL");
  MRGCN_REQUIRE(C > 0 && ldd >= C && n > 0 && num_rows > 0, "C / ldd / n / num_rows");
  hipStream_t s = (hipStream_t)stream;
  MRGCN_HIP_TRY(mrgcn::fill_async(dlogits, 0, (size_t)num_rows * ldd * sizeof(float), s));
  if (row_flags) MRGCN_HIP_TRY(mrgcn::fill_async(row_flags, 0, (size_t)num_rows, s));
  int grid = (int)((n * C + kTB - 1) / kTB);
  if (grid > 1024) grid = 1024;
  mrgcn::k_xent_scatter<<<dim3(grid), dim3(kTB), 0, s>>>(drows, idx, n, C, g, dlogits, ldd, row_flags);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_sumsq_clip_multi_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, int32_t n_extra,
                               const double *const *extra, double *accum, uint32_t *ticket, float max_norm,
                               double *sumsq_out, float *coef, float *norm, int64_t *step_dev, float beta1,
                               float beta2, float *bc_dev, void *stream) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax && n_extra >= 0 && n_extra <= mrgcn::kMultiMax,
                "at most 16 tensors / extra sums per call, at least one tensor");
  MRGCN_REQUIRE(grads && numel && accum && ticket && (n_extra == 0 || extra), "NULL");
  MRGCN_REQUIRE(!step_dev || bc_dev, "bc_dev is NULL");
  mrgcn::MultiSumsq a{};
  a.n_tensors = n_tensors;
  a.n_extra = n_extra;
  int blk = 0;
  for (int t = 0; t < n_tensors; ++t) {
    MRGCN_REQUIRE(grads[t] && numel[t] >= 0 && ((uintptr_t)grads[t] & 15) == 0, "gradient: NULL / 16-byte alignment");
    a.g[t] = grads[t];
    a.n[t] = numel[t];
    a.blk0[t] = blk;
    int64_t nb = ((numel[t] >> 2) + kTB - 1) / kTB;
    blk += (int)(nb < 1 ? 1 : (nb > 64 ? 64 : nb));
  }
  a.blk0[n_tensors] = blk;
  for (int e = 0; e < n_extra; ++e) {
    MRGCN_REQUIRE(extra[e], "extra sum is NULL");
    a.extra[e] = extra[e];
  }
  mrgcn::k_sumsq_multi<<<dim3(blk), dim3(kTB), 0, (hipStream_t)stream>>>(a, accum, ticket, max_norm, sumsq_out, coef,
                                                                        norm, step_dev, beta1, beta2, bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_sumsq_accum_multi_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, double *accum,
                                void *stream) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax && grads && numel && accum, "1..16 tensors per call");
  mrgcn::MultiSumsq a{};
  a.n_tensors = n_tensors;
  int blk = 0;
  for (int t = 0; t < n_tensors; ++t) {
    MRGCN_REQUIRE(grads[t] && numel[t] >= 0 && ((uintptr_t)grads[t] & 15) == 0, "gradient: NULL / 16-byte alignment");
    a.g[t] = grads[t];
    a.n[t] = numel[t];
    a.blk0[t] = blk;
    int64_t nb = (numel[t] / 4 + kTB - 1) / kTB;
    blk += (int)(nb < 1 ? 1 : (nb > 64 ? 64 : nb));
  }
  a.blk0[n_tensors] = blk;
  a.n_extra = 0;
  mrgcn::k_sumsq_multi_accum<<<dim3(blk), dim3(kTB), 0, (hipStream_t)stream>>>(a, accum);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_adam_step_multi_f32(int32_t n_tensors, float *const *params, const float *const *grads,
                              float *const *exp_avg, float *const *exp_avg_sq, const int64_t *numel, const float *lr,
                              const float *weight_decay, float beta1, float beta2, float eps, int64_t step,
                              const float *bc_dev, const float *grad_scale, void *stream) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax, "1..16 tensors per call");
  MRGCN_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && lr && weight_decay, "NULL");
  MRGCN_REQUIRE(step >= 1 || bc_dev, "step counts from 1");
  mrgcn::MultiAdam a{};
  a.n_tensors = n_tensors;
  int blk = 0;
  for (int t = 0; t < n_tensors; ++t) {
    MRGCN_REQUIRE(params[t] && grads[t] && exp_avg[t] && exp_avg_sq[t] && numel[t] >= 0, "NULL tensor");
    a.p[t] = params[t]; a.g[t] = grads[t]; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t];
    a.n[t] = numel[t]; a.lr[t] = lr[t]; a.wd[t] = weight_decay[t];
    a.blk0[t] = blk;
    int64_t nb = (numel[t] + kTB - 1) / kTB;
    blk += (int)(nb < 1 ? 1 : (nb > 256 ? 256 : nb));
  }
  a.blk0[n_tensors] = blk;
  const double bc1 = bc_dev ? 1.0 : 1.0 - pow((double)beta1, (double)step);
  const double bc2 = bc_dev ? 1.0 : 1.0 - pow((double)beta2, (double)step);
  mrgcn::k_adam_multi<<<dim3(blk), dim3(kTB), 0, (hipStream_t)stream>>>(a, beta1, beta2, eps, (float)bc1,
                                                                       (float)sqrt(bc2), grad_scale, bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

// ---- L1 / L2 penalties on dense and flagged-row parameters ------------------------------------------------------------
int64_t mrgcn_penalty_norm_workspace(void) { return (int64_t)mrgcn::kPenMaxBlocks * 3 * (int64_t)sizeof(double); }

// one tensor of a penalty list: sizes, and whether it moves as 16-byte pieces (`others`: its further base addresses)
static int penalty_tensor(const void *param, const void *grad, uintptr_t others, int64_t numel, const uint8_t *flags,
                          int32_t row_len, int32_t &vec) {
  MRGCN_REQUIRE(param && numel >= 0, "parameter: NULL / numel");
  MRGCN_REQUIRE(!flags || (row_len > 0 && numel % row_len == 0), "row flags need row_len > 0 that divides numel");
  vec = ((((uintptr_t)param | (uintptr_t)grad | others) & 15) == 0) && (!flags || row_len % 4 == 0);
  return MRGCN_OK;
}

int mrgcn_penalty_norm_multi_f32(int32_t n_tensors, const float *const *params, const float *const *grads,
                                 const int64_t *numel, const uint8_t *const *row_flags, const int32_t *row_len, float l1,
                                 float l2, double *out3, double *partials, uint32_t *ticket, void *stream) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax, "1..16 tensors per call");
  MRGCN_REQUIRE(params && grads && numel && out3 && partials && ticket && (!row_flags || row_len), "NULL");
  MRGCN_REQUIRE(l1 >= 0.f && l2 >= 0.f, "l1 / l2 must not be negative");
  mrgcn::MultiPen a{};
  a.n_tensors = n_tensors;
  int64_t blk = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const uint8_t *fl = row_flags ? row_flags[t] : nullptr;
    const int32_t len = fl ? row_len[t] : 0;
    if (int rc = penalty_tensor(params[t], grads[t], 0, numel[t], fl, len, a.vec[t])) return rc;
    a.p[t] = params[t]; a.g[t] = grads[t]; a.flags[t] = fl; a.n[t] = numel[t]; a.row_len[t] = len;
    int64_t per = mrgcn::kPenTile;
    int64_t nb = (numel[t] + per - 1) / per;
    if (nb > mrgcn::kPenTensorBlocks) {  // (sizes only: the same grid on every device and run)
      per = ((numel[t] + mrgcn::kPenTensorBlocks - 1) / mrgcn::kPenTensorBlocks + mrgcn::kPenTile - 1) /
            mrgcn::kPenTile * mrgcn::kPenTile;
      nb = (numel[t] + per - 1) / per;
    }
    a.per_block[t] = per;
    a.blk0[t] = (int32_t)blk;
    blk += nb < 1 ? 1 : nb;
  }
  a.blk0[n_tensors] = (int32_t)blk;
  MRGCN_REQUIRE(blk <= mrgcn::kPenMaxBlocks, "too many elements for one launch (a tensor above 2^20 elements: its own)");
  mrgcn::k_penalty_norm_multi<<<dim3((unsigned)blk), dim3(kTB), 0, (hipStream_t)stream>>>(
      a, l1, 2.f * l2, (l1 > 0.f || l2 > 0.f) ? 1 : 0, out3, partials, ticket);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_adam_step_reg_multi_f32(int32_t n_tensors, float *const *params, const float *const *grads,
                                  const int64_t *numel, const uint8_t *const *row_flags, const int32_t *row_len,
                                  float *const *exp_avg, float *const *exp_avg_sq, const float *lr,
                                  const float *weight_decay, float l1, float l2, float beta1, float beta2, float eps,
                                  int64_t step, const float *bc_dev, const float *grad_scale, void *stream) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax, "1..16 tensors per call");
  MRGCN_REQUIRE(params && grads && numel && exp_avg && exp_avg_sq && lr && weight_decay && (!row_flags || row_len),
                "NULL");
  MRGCN_REQUIRE(step >= 1 || bc_dev, "step counts from 1");
  MRGCN_REQUIRE(l1 >= 0.f && l2 >= 0.f, "l1 / l2 must not be negative");
  mrgcn::MultiAdamReg a{};
  a.n_tensors = n_tensors;
  int64_t blk = 0;
  const int64_t per_thread_block = (int64_t)mrgcn::kAdamRegPieces * kTB;
  for (int t = 0; t < n_tensors; ++t) {
    MRGCN_REQUIRE(exp_avg[t] && exp_avg_sq[t], "NULL moments");
    const uint8_t *fl = row_flags ? row_flags[t] : nullptr;
    const int32_t len = fl ? row_len[t] : 0;
    if (int rc = penalty_tensor(params[t], grads[t], (uintptr_t)exp_avg[t] | (uintptr_t)exp_avg_sq[t], numel[t], fl, len,
                                a.vec[t]))
      return rc;
    a.p[t] = params[t]; a.g[t] = grads[t]; a.flags[t] = fl; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t];
    a.n[t] = numel[t]; a.lr[t] = lr[t]; a.wd[t] = weight_decay[t]; a.row_len[t] = len;
    const int64_t units = a.vec[t] ? (numel[t] >> 2) : numel[t];
    const int64_t nb = (units + per_thread_block - 1) / per_thread_block;
    a.blk0[t] = blk;
    blk += nb < 1 ? 1 : nb;
  }
  a.blk0[n_tensors] = blk;
  MRGCN_REQUIRE(blk <= 0x7fffffff, "too many elements for one launch");
  const double bc1 = bc_dev ? 1.0 : 1.0 - pow((double)beta1, (double)step);
  const double bc2 = bc_dev ? 1.0 : 1.0 - pow((double)beta2, (double)step);
  mrgcn::k_adam_reg_multi<<<dim3((unsigned)blk), dim3(kTB), 0, (hipStream_t)stream>>>(
      a, l1, 2.f * l2, (l1 > 0.f || l2 > 0.f) ? 1 : 0, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale,
      bc_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

// ---- deterministic squared norms ----------------------------------------------------------------------------------
int64_t mrgcn_sumsq_det_workspace(void) { return (int64_t)mrgcn::kDetMaxBlocks * (int64_t)sizeof(double); }

int mrgcn_sumsq_accum_det_f32(const float *x, int64_t n, double *accum, double *partials, uint32_t *ticket,
                              void *stream) {
  MRGCN_REQUIRE(x && accum && partials && ticket, "NULL");
  MRGCN_REQUIRE(((uintptr_t)x & 15) == 0, "16-byte alignment");
  if (n == 0) return MRGCN_OK;
  mrgcn::k_sumsq_det<<<dim3(std::min(stream_grid(((n >> 2) + 3) / 4), 512)), dim3(kTB), 0, (hipStream_t)stream>>>(
      x, n, accum, partials, ticket);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

static int multi_sumsq_args(int32_t n_tensors, const float *const *grads, const int64_t *numel, mrgcn::MultiSumsq &a,
                            int &blk) {
  MRGCN_REQUIRE(n_tensors >= 1 && n_tensors <= mrgcn::kMultiMax && grads && numel, "1..16 tensors per call");
  a.n_tensors = n_tensors;
  blk = 0;
  for (int t = 0; t < n_tensors; ++t) {
    MRGCN_REQUIRE(grads[t] && numel[t] >= 0 && ((uintptr_t)grads[t] & 15) == 0, "gradient: NULL / 16-byte alignment");
    a.g[t] = grads[t];
    a.n[t] = numel[t];
    a.blk0[t] = blk;
    int64_t nb = ((numel[t] >> 2) + kTB - 1) / kTB;
    blk += (int)(nb < 1 ? 1 : (nb > 64 ? 64 : nb));
  }
  a.blk0[n_tensors] = blk;
  return MRGCN_OK;
}

int mrgcn_sumsq_accum_multi_det_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, double *accum,
                                    double *partials, uint32_t *ticket, void *stream) {
  MRGCN_REQUIRE(accum && partials && ticket, "NULL");
  mrgcn::MultiSumsq a{};
  int blk = 0;
  if (int rc = multi_sumsq_args(n_tensors, grads, numel, a, blk)) return rc;
  mrgcn::k_sumsq_multi_accum_det<<<dim3(blk), dim3(kTB), 0, (hipStream_t)stream>>>(a, accum, partials, ticket);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_sumsq_clip_multi_det_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, int32_t n_extra,
                                   const double *const *extra, double *accum, uint32_t *ticket, float max_norm,
                                   double *sumsq_out, float *coef, float *norm, int64_t *step_dev, float beta1,
                                   float beta2, float *bc_dev, double *partials, void *stream) {
  MRGCN_REQUIRE(n_extra >= 0 && n_extra <= mrgcn::kMultiMax, "at most 16 extra sums per call");
  MRGCN_REQUIRE(accum && ticket && partials && (n_extra == 0 || extra), "NULL");
  MRGCN_REQUIRE(!step_dev || bc_dev, "bc_dev is NULL");
  mrgcn::MultiSumsq a{};
  int blk = 0;
  if (int rc = multi_sumsq_args(n_tensors, grads, numel, a, blk)) return rc;
  a.n_extra = n_extra;
  for (int e = 0; e < n_extra; ++e) {
    MRGCN_REQUIRE(extra[e], "extra sum is NULL");
    a.extra[e] = extra[e];
  }
  mrgcn::k_sumsq_multi_det<<<dim3(blk), dim3(kTB), 0, (hipStream_t)stream>>>(a, accum, ticket, max_norm, sumsq_out, coef,
                                                                            norm, step_dev, beta1, beta2, bc_dev,
                                                                            partials);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
