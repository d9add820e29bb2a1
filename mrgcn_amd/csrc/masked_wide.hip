// The WIDE featureless input layer of a mini-batch as a masked pass (masked.hip) without the compact operand M: the
// link-prediction encoder of configs/fb15k-237.toml / wn18rr.toml in mini-batch mode (gcn_batchsize = 32:
// tasks/link_prediction.py:477-530 + rgcn.py:91-128), one `mrgcn` layer N x 200, 2 bases, no bias, ReLU.
//
// Shapes: 1 <= B <= 4 bases, 16 < F <= 256, F % 4 == 0, weight_I node-major V[j][b][0:F] (the family wide_input.hip
// serves for full batches).  Lane l of a wave holds features 4l .. 4l+3 of a row (one 16-byte piece).
//
// Forward, one block of 16 waves per flagged row q (the support's forward CSR; wave w takes the row's 64-entry pieces
// w, w + 16, ..., the waves' sums meet in LDS in a fixed order):
//     Y[q] = relu( sum over entries e of q: v[e] * sum_b comp[r_e][b] V[j_e][b] )
// The entries' columns, values, relations and nodes are fetched lane-parallel (one coalesced load each for up to 64
// entries), then the V rows of U entries at a time are issued straight-line at clamped indices before any arithmetic.
// The general pair mrgcn_support_mix_fwd_f32 + mrgcn_support_spmm_fwd_f32 forms M ([L] x F, written once and read
// once) first; this reads V straight.
//
// Backward, one block of 4 waves per live node j (the support's column-major arrays; a node's live columns are
// consecutive, wave w takes columns w, w + 4, ..., the waves' dV sums meet in LDS in a fixed order):
//     dm_k        = sum over entries e of live column k: v[e] dY[ROWRANK[row_e]]      (registers, never stored)
//     dV[j][b]    = sum over k of node j: comp[r_k][b] dm_k                            (one store per node)
//     D[k][b]     = <dm_k, V[j][b]>                                                   (B floats per live column)
//     ||dV_j||^2  = one double per node
// then dcomp[r] = the D rows of relation r and ||dV||^2 = the per-node doubles, both summed in a fixed order by the
// support's relation-major chunk kernels (support.hip).  No atomics: the same bits every run.
#include "common.hpp"

namespace mrgcn {
namespace {

using f32x4m = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float lane_f(float v, int i) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

template <int BT, int NW>
__global__ __launch_bounds__(64 * NW) void k_sup_wide_fwd(const int32_t *__restrict__ fptr,
                                                      const int32_t *__restrict__ fcol,
                                                      const float *__restrict__ fval,
                                                      const int32_t *__restrict__ lrel,
                                                      const int32_t *__restrict__ lnode_ord,
                                                      const int32_t *__restrict__ lnode, int64_t NR,
                                                      const float *__restrict__ V, const float *__restrict__ comp,
                                                      int F, float *__restrict__ Y, int64_t ldY, int relu) {
  constexpr int U = BT <= 2 ? 8 : 4;  // entries whose V rows are in flight together
  __shared__ f32x4m s_acc[NW][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t q = blockIdx.x;
  const int F4 = F >> 2;
  const bool active = lane < F4;
  const int lo = active ? lane : 0;
  const f32x4m *V4 = reinterpret_cast<const f32x4m *>(V);
  const int32_t e0 = fptr[q], e1 = fptr[q + 1];
  f32x4m acc = {0.f, 0.f, 0.f, 0.f};
  for (int32_t base = e0 + 64 * wv; base < e1; base += 64 * NW) {  // wave w: pieces w, w + NW, ... of 64 entries
    const int cnt = (e1 - base < 64) ? e1 - base : 64;
    const int32_t e = base + (lane < cnt ? lane : cnt - 1);
    const int32_t k = fcol[e];
    const float v = fval[e];
    const int32_t r = lrel[k];
    const int32_t j = lnode[lnode_ord[k]];
    float w[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) w[b] = comp[(int64_t)r * BT + b];
    for (int i0 = 0; i0 < cnt; i0 += U) {
      f32x4m x[U][BT];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // every load of the step, unconditional at clamped entries
        const int ii = (i0 + u < cnt) ? i0 + u : cnt - 1;
        const int64_t jj = __builtin_amdgcn_readlane(j, ii);
#pragma unroll
        for (int b = 0; b < BT; ++b) x[u][b] = V4[(jj * BT + b) * F4 + lo];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < cnt) {  // wave uniform
          const int ii = i0 + u;
          f32x4m m = lane_f(w[0], ii) * x[u][0];
#pragma unroll
          for (int b = 1; b < BT; ++b) m += lane_f(w[b], ii) * x[u][b];
          acc += lane_f(v, ii) * m;
        }
      }
    }
  }
  s_acc[wv][lane] = acc;
  __syncthreads();
  if (wv != 0) return;
  acc = s_acc[0][lane];
#pragma unroll
  for (int w = 1; w < NW; ++w) acc += s_acc[w][lane];  // (the waves' partial sums in a fixed order)
  if (relu) {
    acc.x = acc.x > 0.f ? acc.x : 0.f;
    acc.y = acc.y > 0.f ? acc.y : 0.f;
    acc.z = acc.z > 0.f ? acc.z : 0.f;
    acc.w = acc.w > 0.f ? acc.w : 0.f;
  }
  if (active) *reinterpret_cast<f32x4m *>(Y + q * ldY + 4 * lane) = acc;
}

template <int BT, int NW>
__global__ __launch_bounds__(64 * NW) void k_sup_wide_bwd(const int32_t *__restrict__ lnode,
                                                      const int32_t *__restrict__ lnptr,
                                                      const int32_t *__restrict__ lrel,
                                                      const int32_t *__restrict__ lptr,
                                                      const int32_t *__restrict__ lrow_rank,
                                                      const float *__restrict__ lval, int64_t NL,
                                                      const float *__restrict__ dY, int64_t ldY,
                                                      const float *__restrict__ V, const float *__restrict__ comp,
                                                      int F, float *__restrict__ dV, float *__restrict__ D,
                                                      double *__restrict__ sq_node) {
  constexpr int U = 8;  // dY rows in flight together
  __shared__ f32x4m s_acc[NW][BT][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t t = blockIdx.x;
  const int F4 = F >> 2;
  const bool active = lane < F4;
  const int lo = active ? lane : 0;
  const int64_t ld4 = ldY >> 2;
  const f32x4m *V4 = reinterpret_cast<const f32x4m *>(V);
  const f32x4m *dY4 = reinterpret_cast<const f32x4m *>(dY);
  const f32x4m zero = {0.f, 0.f, 0.f, 0.f};
  const int64_t j = lnode[t];
  const int32_t k0 = lnptr[t], k1 = lnptr[t + 1];
  f32x4m Vb[BT], accV[BT];
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    Vb[b] = active ? V4[(j * BT + b) * F4 + lane] : zero;
    accV[b] = zero;
  }
  // wave w takes the node's live columns w, w + NW, ...: 64 of them per round
  for (int32_t kb = k0 + wv; kb < k1; kb += 64 * NW) {
    // the relation, entry range and comp row of up to 64 live columns of the node, one coalesced load each
    const int ncol = (k1 - kb + NW - 1) / NW < 64 ? (k1 - kb + NW - 1) / NW : 64;
    const int32_t kl = kb + NW * (lane < ncol ? lane : ncol - 1);
    const int32_t r = lrel[kl], p0 = lptr[kl], p1 = lptr[kl + 1];
    float w[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) w[b] = comp[(int64_t)r * BT + b];
    for (int c = 0; c < ncol; ++c) {
      const int32_t a0 = __builtin_amdgcn_readlane(p0, c), a1 = __builtin_amdgcn_readlane(p1, c);
      f32x4m dm = zero;
      for (int32_t eb = a0; eb < a1; eb += 64) {
        const int cnt = (a1 - eb < 64) ? a1 - eb : 64;
        const int32_t e = eb + (lane < cnt ? lane : cnt - 1);
        const int32_t rr = lrow_rank[e];
        const float vv = lval[e];
        for (int i0 = 0; i0 < cnt; i0 += U) {
          f32x4m x[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int ii = (i0 + u < cnt) ? i0 + u : cnt - 1;
            x[u] = dY4[(int64_t)__builtin_amdgcn_readlane(rr, ii) * ld4 + lo];
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (i0 + u < cnt) dm += lane_f(vv, i0 + u) * x[u];  // (wave uniform)
        }
      }
      if (!active) dm = zero;
      const int64_t k = kb + (int64_t)NW * c;
#pragma unroll
      for (int b = 0; b < BT; ++b) {
        accV[b] += lane_f(w[b], c) * dm;
        const f32x4m pr = dm * Vb[b];
        const float d = wave_sum((pr.x + pr.y) + (pr.z + pr.w));
        if (lane == 0) D[k * BT + b] = d;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BT; ++b) s_acc[wv][b][lane] = accV[b];
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    accV[b] = s_acc[0][b][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) accV[b] += s_acc[w][b][lane];  // (the waves' partial sums in a fixed order)
  }
  double sq = 0.0;
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    if (active) *reinterpret_cast<f32x4m *>(dV + (j * BT + b) * F + 4 * lane) = accV[b];
    sq += (double)accV[b].x * accV[b].x + (double)accV[b].y * accV[b].y + (double)accV[b].z * accV[b].z +
          (double)accV[b].w * accV[b].w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  if (lane == 0) sq_node[t] = sq;
}

bool wide_shape(int B, int F) { return B >= 1 && B <= 4 && F > 16 && F <= 256 && F % 4 == 0; }

}  // namespace
}  // namespace mrgcn

extern "C" {

using namespace mrgcn;

int32_t mrgcn_support_wide_supported(const mrgcn_support_t *q, int32_t B, int32_t F) {
  return (q && q->has_forward && wide_shape(B, F)) ? 1 : 0;
}

int mrgcn_support_wide_fwd_f32(const mrgcn_support_t *q, const float *V, const float *comp, int32_t B, int32_t F,
                               float *Y, int64_t ldY, int32_t relu, void *stream) {
  MRGCN_REQUIRE(q && q->has_forward, "the support was not created with MRGCN_SUPPORT_FORWARD");
  MRGCN_REQUIRE(V && comp && Y, "NULL");
  if (!wide_shape(B, F)) {
    set_error("mrgcn_support_wide_fwd_f32: shape outside 1 <= B <= 4, 16 < F <= 256, F % 4 == 0");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(ldY >= F && ldY % 4 == 0, "ldY (>= F, a multiple of 4)");
  MRGCN_REQUIRE(((((uintptr_t)V) | ((uintptr_t)Y)) & 15) == 0, "V and Y must be 16-byte aligned");
  if (q->NR == 0) return MRGCN_OK;
  hipStream_t s = (hipStream_t)stream;
  // a block of kFwdWaves waves per flagged row (a batch has a few hundred rows, some of them hubs with thousands of
  // entries: one wave per row left those as a serial tail of a few hundred waves)
  constexpr int kFwdWaves = 16;
  const dim3 grid((unsigned)q->NR), tb(64 * kFwdWaves);
#define WIDE_FWD(BB)                                                                                               \
  k_sup_wide_fwd<BB, kFwdWaves><<<grid, tb, 0, s>>>(q->fptr, q->fcol, q->fval, q->lrel, q->lnode_ord, q->lnode, q->NR, V, comp, \
                                         F, Y, ldY, relu)
  switch (B) {
    case 1: WIDE_FWD(1); break;
    case 2: WIDE_FWD(2); break;
    case 3: WIDE_FWD(3); break;
    default: WIDE_FWD(4); break;
  }
#undef WIDE_FWD
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_support_wide_bwd_workspace(const mrgcn_support_t *q, int32_t B) {
  if (!q || B <= 0) return 0;
  // D [L][B] | slab [chunks][B] | ||dV_j||^2 per live node (doubles, 8-byte aligned)
  return ((q->L + q->wide.n_chunks) * (int64_t)B + 1) / 2 * 2 + 2 * (q->NL > 0 ? q->NL : 1);
}

int mrgcn_support_wide_bwd_f32(const mrgcn_support_t *q, const float *dY, int64_t ldY, const float *V,
                               const float *comp, int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp,
                               double *dV_sumsq, float *workspace, int64_t workspace_floats, void *stream) {
  MRGCN_REQUIRE(q && q->has_forward, "the support was not created with MRGCN_SUPPORT_FORWARD");
  MRGCN_REQUIRE(dY && V && comp && dV && dcomp, "NULL");
  if (!wide_shape(B, F)) {
    set_error("mrgcn_support_wide_bwd_f32: shape outside 1 <= B <= 4, 16 < F <= 256, F % 4 == 0");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(ldY >= F && ldY % 4 == 0, "ldY (>= F, a multiple of 4)");
  MRGCN_REQUIRE(((((uintptr_t)V) | ((uintptr_t)dY) | ((uintptr_t)dV)) & 15) == 0,
                "dY, V and dV must be 16-byte aligned");
  MRGCN_REQUIRE(workspace && workspace_floats >= mrgcn_support_wide_bwd_workspace(q, B) &&
                    (((uintptr_t)workspace) & 7) == 0,
                "workspace (mrgcn_support_wide_bwd_workspace floats, 8-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const mrgcn_plan *p = q->plan;
  if (dense)
    MRGCN_HIP_TRY(mrgcn::fill_async(dV, 0, (size_t)p->num_nodes * B * F * sizeof(float), s));
  float *D = workspace;
  float *slab = D + q->L * (int64_t)B;
  double *sq_node = reinterpret_cast<double *>(workspace + ((q->L + q->wide.n_chunks) * (int64_t)B + 1) / 2 * 2);
  if (q->NL > 0) {
    // a block of kBwdWaves waves per live node (the columns of a hub node spread over its waves)
    constexpr int kBwdWaves = 4;
    const dim3 grid((unsigned)q->NL), tb(64 * kBwdWaves);
#define WIDE_BWD(BB)                                                                                                \
  k_sup_wide_bwd<BB, kBwdWaves><<<grid, tb, 0, s>>>(q->lnode, q->lnptr, q->lrel, q->lptr, q->lrow_rank, q->lval, q->NL, dY, ldY, \
                                         V, comp, F, dV, D, sq_node)
    switch (B) {
      case 1: WIDE_BWD(1); break;
      case 2: WIDE_BWD(2); break;
      case 3: WIDE_BWD(3); break;
      default: WIDE_BWD(4); break;
    }
#undef WIDE_BWD
    MRGCN_HIP_TRY(hipGetLastError());
  }
  return support_dcomp_from_D(q, D, B, slab, sq_node, q->NL, dcomp, dV_sumsq, s);
}

}  // extern "C"
