// Weight decay and L1 / L2 penalties on the row-sparse node-table step (gfx950).
//
// The reference's task loop (tasks/node_classification.py:35-37, :172-193) hands `weight_decay` to optim.Adam, adds
// l1 . sum|p| + l2 . sum p^2 over the parameters named `weight*` to the loss, clips the total gradient norm and steps.
// With any of the three numbers non-zero EVERY block of the node table weight_I moves every step, so the update visits
// all N nodes — but the gradient of the loss still lives on the gradient support only, and the fused Adam pass
// (rgcn_fused.hip: k_adam_rows_once) already rebuilds each node's gradient block from dM and comp in registers.  The
// two kernels here are that pass over nodes 0 .. N-1 instead of the support's list:
//
//   k_reg_norm      (L1 / L2 only)  sum (g + r(p))^2, sum |p|, sum p^2 with r(p) = l1 sign(p) + 2 l2 p: what
//                                   clip_grad_norm_ sees of the node table, and the penalty's value.  One read of the
//                                   table.  Weight decay needs no such pass: torch adds wd . p inside Adam.step, after
//                                   the clip.
//   k_adam_rows_reg                 the k_adam_rows_once update with gg = (g + r(p)) . scale + wd . p.
//
// Both are ONE-SHOT grids for the reasons written above k_adam_rows_once: a wave owns a few consecutive nodes, takes
// each node's live columns from the support's per-node ranges (a node without live columns has g = 0), reads the comp
// row of each live column straight from the L2-resident table into lanes, issues every load unconditionally at clamped
// addresses and moves blocks as 16-byte pieces with nontemporal loads and stores.  The gradient rebuild restates
// k_adam_rows_once's ballot / lane-permute loop (the same fmaf chain per element) rather than sharing it, so that
// kernel's code object stays as it was.
//
// Reach: the shapes mrgcn_adam_rows_fused_supported accepts with B F / 4 <= 128 (two pieces per lane) and an even F —
// the reach of the one-shot forms on a support (support.hip: k_mix_bwd_stream).

#include <cmath>

#include "common.hpp"
#include "config.hpp"

namespace mrgcn {
namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRegTB = 256;       // four waves
constexpr int kRegNormNPW = 4;    // nodes per wave of the norm pass (loads only: registers are cheap)
constexpr int kRegReduceTB = 1024;

// (basis, feature) of the lane's elements: (b << 8) | f
template <int NH>
__device__ __forceinline__ void lane_elements(int (&bf)[NH][4], int lane, int nv, int F) {
  const unsigned magicF = 65536u / (unsigned)F + 1u;  // e / F == (e * magicF) >> 16 for e * F < 2^16 (B F <= 1024)
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned e = 4u * (unsigned)min(lane + 64 * h, nv - 1) + (unsigned)k;
      const unsigned bb = (e * magicF) >> 16;
      bf[h][k] = (int)((bb << 8) | (e - bb * (unsigned)F));
    }
}

// g[h][k] = sum over the node's live columns c in [n0, n1) of comp[rel_c][b] . dM[c][f] — k_adam_rows_once's loop:
// the 16-lane group kq holds column cb + kq (relation `rm`, gradient row `dm`), c4[kk] the comp row of group kk's
// column (lane b: comp[r][b]).  The first four columns arrive loaded; a node with more loads the next four here.
template <int NH>
__device__ __forceinline__ void rebuild_block(float (&g)[NH][4], const int (&bf)[NH][4], int32_t n0, int32_t n1,
                                              int32_t rm, float dm, float (&c4)[4],
                                              const int32_t *__restrict__ lrel, const float *__restrict__ dM,
                                              int64_t ldM, const float *__restrict__ comp, int B, int F, int lane) {
  const int kq = lane >> 4, oq = lane & 15;
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int k = 0; k < 4; ++k) g[h][k] = 0.f;
  bool lv = n0 + kq < n1;
  for (int32_t cb = n0;;) {
    const uint64_t bl = __builtin_amdgcn_ballot_w64(lv && oq == 0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (!((bl >> (16 * kk)) & 1ull)) continue;  // wave uniform: past the node's columns
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          g[h][k] = fmaf(__shfl(c4[kk], bf[h][k] >> 8), __shfl(dm, 16 * kk + (bf[h][k] & 255)), g[h][k]);
    }
    cb += 4;
    if (cb >= n1) break;  // (few nodes have more than four live columns)
    const int32_t cc = min(cb + kq, n1 - 1);
    lv = cb + kq < n1;
    rm = lrel[cc];
    dm = dM[(int64_t)cc * ldM + min(oq, F - 1)];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      c4[kk] = comp[(int64_t)__builtin_amdgcn_readlane(rm, 16 * kk) * B + min(lane, B - 1)];
  }
}

// the penalty's gradient: l1 sign(p) + 2 l2 p, sign(0) = 0
__device__ __forceinline__ float penalty_grad(float p, float l1, float l2x2) {
  const float sg = (float)(p > 0.f) - (float)(p < 0.f);
  return fmaf(l2x2, p, l1 * sg);
}

// ---- the norm pass: per-block partials (three doubles each), no atomics ------------------------------------------------
template <int NH>
__global__ __launch_bounds__(kRegTB) void k_reg_norm(const int32_t *__restrict__ nlptr, const int32_t *__restrict__ lrel,
                                                     const float *__restrict__ dM, int64_t ldM,
                                                     const float *__restrict__ comp, int64_t N, int64_t Lc, int B, int F,
                                                     const float *__restrict__ p, float l1, float l2x2,
                                                     double *__restrict__ partials) {
  constexpr int NPW = kRegNormNPW;
  __shared__ double s_part[kRegTB / 64][3];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t i0 = w * NPW;  // (a wave past the end repeats the last node and counts nothing)
  const int nv = (B * F) >> 2;
  const int kq = lane >> 4, oq = lane & 15;
  int64_t j[NPW];
  int32_t n0[NPW], n1[NPW];
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    j[t] = min(i0 + t, N - 1);
    n0[t] = nlptr[j[t]];
    n1[t] = nlptr[j[t] + 1];
  }
  f4 P[NPW][NH];
  int32_t rmine[NPW];
  float dmine[NPW];
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    const f4 *p4 = reinterpret_cast<const f4 *>(p) + j[t] * (int64_t)nv;
#pragma unroll
    for (int h = 0; h < NH; ++h) P[t][h] = __builtin_nontemporal_load(p4 + min(lane + 64 * h, nv - 1));
    const int32_t cc0 = (int32_t)max(min((int64_t)min(n0[t] + kq, n1[t] - 1), Lc - 1), (int64_t)0);
    rmine[t] = lrel[cc0];
    dmine[t] = dM[(int64_t)cc0 * ldM + min(oq, F - 1)];
  }
  int bf[NH][4];
  lane_elements<NH>(bf, lane, nv, F);
  float cv[NPW][4];
#pragma unroll
  for (int t = 0; t < NPW; ++t)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      cv[t][kk] = comp[(int64_t)__builtin_amdgcn_readlane(rmine[t], 16 * kk) * B + min(lane, B - 1)];
  double a_g = 0.0, a_1 = 0.0, a_2 = 0.0;
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    float g[NH][4];
    float c4[4] = {cv[t][0], cv[t][1], cv[t][2], cv[t][3]};
    rebuild_block<NH>(g, bf, n0[t], n1[t], rmine[t], dmine[t], c4, lrel, dM, ldM, comp, B, F, lane);
    if (i0 + t >= N) continue;  // wave uniform
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      if (lane + 64 * h >= nv) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float pp = P[t][h][k];
        const double x = (double)(g[h][k] + penalty_grad(pp, l1, l2x2));
        const double pd = (double)pp;
        a_g = fma(x, x, a_g);
        a_1 += fabs(pd);
        a_2 = fma(pd, pd, a_2);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // a fixed tree
    a_g += __shfl_xor(a_g, o);
    a_1 += __shfl_xor(a_1, o);
    a_2 += __shfl_xor(a_2, o);
  }
  if (lane == 0) {
    s_part[wv][0] = a_g;
    s_part[wv][1] = a_1;
    s_part[wv][2] = a_2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
#pragma unroll
    for (int u = 0; u < kRegTB / 64; ++u) t += s_part[u][threadIdx.x];
    partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// the partials in block order: thread t takes blocks t, t + 1024, ..., then a fixed tree
__global__ __launch_bounds__(kRegReduceTB) void k_reg_norm_reduce(const double *__restrict__ partials, int64_t nblocks,
                                                                  double *__restrict__ out3) {
  __shared__ double s[3][kRegReduceTB];
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nblocks; b += kRegReduceTB) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += partials[b * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int o = kRegReduceTB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out3[threadIdx.x] = s[threadIdx.x][0];
}

// ---- the regularised row Adam: every node, gg = (g + r(p)) scale + wd p ------------------------------------------------
template <int NH, int NPW>
__global__ __launch_bounds__(kRegTB) void k_adam_rows_reg(
    const int32_t *__restrict__ nlptr, const int32_t *__restrict__ lrel, const float *__restrict__ dM, int64_t ldM,
    const float *__restrict__ comp, int64_t N, int64_t Lc, int B, int F, float *__restrict__ p, float *__restrict__ m,
    float *__restrict__ v, uint8_t *__restrict__ ever, float lr, float b1, float b2, float eps, float bc1,
    float bc2_sqrt, float wd, float l1, float l2x2, const float *__restrict__ scale,
    const float *__restrict__ bc_dev) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t i0 = w * NPW;
  if (i0 >= N) return;  // wave uniform
  const int nv = (B * F) >> 2;  // 16-byte pieces of a block
  const int kq = lane >> 4, oq = lane & 15;
  // round 1: the nodes' live column ranges (clamped: a wave past the end repeats the last node and stores nothing)
  int64_t j[NPW];
  int32_t n0[NPW], n1[NPW];
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    j[t] = min(i0 + t, N - 1);
    n0[t] = nlptr[j[t]];
    n1[t] = nlptr[j[t] + 1];
  }
  // round 2: the nodes' blocks, and relation / gradient row of their first four live columns
  f4 P[NPW][NH], M[NPW][NH], V[NPW][NH];
  int32_t rmine[NPW];
  float dmine[NPW];
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    const f4 *p4 = reinterpret_cast<const f4 *>(p) + j[t] * (int64_t)nv;
    const f4 *m4 = reinterpret_cast<const f4 *>(m) + j[t] * (int64_t)nv;
    const f4 *v4 = reinterpret_cast<const f4 *>(v) + j[t] * (int64_t)nv;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int q = min(lane + 64 * h, nv - 1);
      P[t][h] = __builtin_nontemporal_load(p4 + q);
      M[t][h] = __builtin_nontemporal_load(m4 + q);
      V[t][h] = __builtin_nontemporal_load(v4 + q);
    }
    // (a node without live columns reads some valid column and uses none of it)
    const int32_t cc0 = (int32_t)max(min((int64_t)min(n0[t] + kq, n1[t] - 1), Lc - 1), (int64_t)0);
    rmine[t] = lrel[cc0];
    dmine[t] = dM[(int64_t)cc0 * ldM + min(oq, F - 1)];
  }
  if (bc_dev) {
    bc1 = bc_dev[0];
    bc2_sqrt = bc_dev[1];
  }
  const float sc = scale ? *scale : 1.f;
  const float step = lr / bc1;
  int bf[NH][4];
  lane_elements<NH>(bf, lane, nv, F);
  // round 3: the comp rows of those columns (lane b: comp[r][b]) — four unconditional loads per node
  float cv[NPW][4];
#pragma unroll
  for (int t = 0; t < NPW; ++t)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      cv[t][kk] = comp[(int64_t)__builtin_amdgcn_readlane(rmine[t], 16 * kk) * B + min(lane, B - 1)];
#pragma unroll
  for (int t = 0; t < NPW; ++t) {
    float g[NH][4];
    float c4[4] = {cv[t][0], cv[t][1], cv[t][2], cv[t][3]};
    rebuild_block<NH>(g, bf, n0[t], n1[t], rmine[t], dmine[t], c4, lrel, dM, ldM, comp, B, F, lane);
    if (i0 + t >= N) continue;  // wave uniform
    f4 *p4 = reinterpret_cast<f4 *>(p) + j[t] * (int64_t)nv;
    f4 *m4 = reinterpret_cast<f4 *>(m) + j[t] * (int64_t)nv;
    f4 *v4 = reinterpret_cast<f4 *>(v) + j[t] * (int64_t)nv;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pp = P[t][h][k], mm = M[t][h][k], vv = V[t][h][k];
        // torch's order: the penalty is part of .grad and is clipped, Adam adds the decay afterwards.  With
        // wd = l1 = l2 = 0 this is g * sc, then k_adam_rows_once's chain.
        const float gg = fmaf(wd, pp, (g[h][k] + penalty_grad(pp, l1, l2x2)) * sc);
        mm = fmaf(b1, mm, (1.f - b1) * gg);
        vv = fmaf(b2, vv, (1.f - b2) * gg * gg);
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        pp -= step * (mm / denom);
        P[t][h][k] = pp;
        M[t][h][k] = mm;
        V[t][h][k] = vv;
      }
      const int q = lane + 64 * h;
      if (q < nv) {
        __builtin_nontemporal_store(P[t][h], p4 + q);
        __builtin_nontemporal_store(M[t][h], m4 + q);
        __builtin_nontemporal_store(V[t][h], v4 + q);
      }
    }
    if (lane == 0) ever[j[t]] = 1;
  }
}

bool reg_shape_ok(const mrgcn_support_t *q, int32_t B, int32_t F) {
  return q && q->plan && mrgcn_adam_rows_fused_supported(q->plan, B, F) && (B * F) / 4 <= 128 && (F & 1) == 0;
}

int64_t reg_norm_blocks(int64_t N) {
  const int64_t waves = (N + kRegNormNPW - 1) / kRegNormNPW;
  return (waves + kRegTB / 64 - 1) / (kRegTB / 64);
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int64_t mrgcn_support_reg_norm_workspace(const mrgcn_support_t *q, int32_t B, int32_t F) {
  if (!reg_shape_ok(q, B, F)) return -1;
  return reg_norm_blocks(q->plan->num_nodes) * 3 * (int64_t)sizeof(double);
}

int mrgcn_support_reg_norm_f32(const mrgcn_support_t *q, const float *dM, int64_t ldM, const float *comp, int32_t B,
                               int32_t F, const float *param, float l1, float l2, double *out3, void *workspace,
                               int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(q && comp && param && out3, "NULL");
  if (!reg_shape_ok(q, B, F)) {
    set_error("mrgcn_support_reg_norm_f32: shape outside mrgcn_support_reg_norm_workspace");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(dM || q->L == 0, "NULL");
  MRGCN_REQUIRE(ldM >= F, "ldM");
  MRGCN_REQUIRE((((uintptr_t)param) & 15) == 0, "param must be 16-byte aligned");
  MRGCN_REQUIRE(l1 >= 0.f && l2 >= 0.f, "l1 / l2");
  const int64_t N = q->plan->num_nodes;
  const int64_t nblocks = reg_norm_blocks(N);
  MRGCN_REQUIRE(workspace && (((uintptr_t)workspace) & 7) == 0 && workspace_bytes >= nblocks * 3 * (int64_t)sizeof(double),
                "workspace (mrgcn_support_reg_norm_workspace bytes, 8-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const int32_t *lrel = q->lrel;
  if (q->L == 0) {  // no live column: every load of a column lands in valid memory and nothing of it is used
    lrel = q->nlptr;
    dM = param;
    ldM = 0;
    comp = param;
  }
  double *partials = (double *)workspace;
  if ((B * F) / 4 <= 64)
    k_reg_norm<1><<<dim3((unsigned)nblocks), dim3(kRegTB), 0, s>>>(q->nlptr, lrel, dM, ldM, comp, N, q->L, B, F, param,
                                                                   l1, 2.f * l2, partials);
  else
    k_reg_norm<2><<<dim3((unsigned)nblocks), dim3(kRegTB), 0, s>>>(q->nlptr, lrel, dM, ldM, comp, N, q->L, B, F, param,
                                                                   l1, 2.f * l2, partials);
  MRGCN_HIP_TRY(hipGetLastError());
  k_reg_norm_reduce<<<dim3(1), dim3(kRegReduceTB), 0, s>>>(partials, nblocks, out3);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_support_adam_rows_reg_f32(const mrgcn_support_t *q, const float *dM, int64_t ldM, const float *comp,
                                    int32_t B, int32_t F, float *param, float *exp_avg, float *exp_avg_sq,
                                    uint8_t *row_ever, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, float l1, float l2, int64_t step, const float *bc_dev,
                                    const float *grad_scale, void *stream) {
  MRGCN_REQUIRE(q && comp && param && exp_avg && exp_avg_sq && row_ever, "NULL");
  if (!reg_shape_ok(q, B, F)) {
    set_error("mrgcn_support_adam_rows_reg_f32: shape outside mrgcn_support_reg_norm_workspace");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(dM || q->L == 0, "NULL");
  MRGCN_REQUIRE(ldM >= F, "ldM");
  MRGCN_REQUIRE(((((uintptr_t)param) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) == 0,
                "param / moments must be 16-byte aligned");
  MRGCN_REQUIRE(bc_dev || step >= 1, "step");
  MRGCN_REQUIRE(weight_decay >= 0.f && l1 >= 0.f && l2 >= 0.f, "weight_decay / l1 / l2");
  float bc1 = 1.f, bc2s = 1.f;
  if (!bc_dev) {
    bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = q->plan->num_nodes;
  const int32_t *lrel = q->lrel;
  if (q->L == 0) {  // (see mrgcn_support_reg_norm_f32)
    lrel = q->nlptr;
    dM = param;
    ldM = 0;
    comp = param;
  }
  const int nv = (B * F) / 4;
  // a node block of one piece per lane is at most 1 KB per array: two nodes per wave; of two pieces, one (the sibling's
  // measured best at the AM shape)
  const int npw = nv <= 64 ? 2 : 1;
  const int64_t waves = (N + npw - 1) / npw;
  const dim3 grid((unsigned)((waves + kRegTB / 64 - 1) / (kRegTB / 64)));
#define ADAM_REG_GO(NH_, NPW_)                                                                                      \
  k_adam_rows_reg<NH_, NPW_><<<grid, dim3(kRegTB), 0, s>>>(q->nlptr, lrel, dM, ldM, comp, N, q->L, B, F, param,      \
                                                           exp_avg, exp_avg_sq, row_ever, lr, beta1, beta2, eps, bc1, \
                                                           bc2s, weight_decay, l1, 2.f * l2, grad_scale, bc_dev)
  if (nv <= 64) ADAM_REG_GO(1, 2);
  else ADAM_REG_GO(2, 1);
#undef ADAM_REG_GO
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
