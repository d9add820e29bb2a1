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
//
// Two tables (mrgcn_support_wide_feat_*): a wide layer WITH a feature term (the multimodal link-prediction encoders,
// input or hidden layer) adds P [NL][B][F] = X . V_F by live-node rank (basis_xform.hip) as a second table with its own
// comp_F and value mode (1, or v_e for full-batch values).  The same entries are read once for both; U halves so that
// U x 2B rows stay in flight.  The backward reads the dY rows of a column once for dm_I and dm_F and writes dV rows,
// dP rows by rank, D_I and D_F per live column; dcomp and dcomp_F both go through the chunk kernels.
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

// HI: the input table V (node-major [N][B][F], values v_e); HF: the feature table P (by live-node rank [NL][B][F],
// values w_e = v_e when `fv`, else 1).  Both read the same entries once; per wave Y = acc_I + acc_F.
template <int BT, int NW, bool HI = true, bool HF = false>
__global__ __launch_bounds__(64 * NW) void k_sup_wide_fwd(const int32_t *__restrict__ fptr,
                                                      const int32_t *__restrict__ fcol,
                                                      const float *__restrict__ fval,
                                                      const int32_t *__restrict__ lrel,
                                                      const int32_t *__restrict__ lnode_ord,
                                                      const int32_t *__restrict__ lnode, int64_t NR,
                                                      const float *__restrict__ V, const float *__restrict__ comp,
                                                      int F, float *__restrict__ Y, int64_t ldY, int relu,
                                                      const float *__restrict__ P = nullptr,
                                                      const float *__restrict__ compF = nullptr, int fv = 0) {
  // entries whose table rows are in flight together (U x B rows per table: two tables halve U)
  constexpr int U = (HI && HF) ? (BT <= 2 ? 4 : 2) : (BT <= 2 ? 8 : 4);
  __shared__ f32x4m s_acc[NW][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t q = blockIdx.x;
  const int F4 = F >> 2;
  const bool active = lane < F4;
  const int lo = active ? lane : 0;
  const f32x4m *V4 = reinterpret_cast<const f32x4m *>(V);
  const f32x4m *P4 = reinterpret_cast<const f32x4m *>(P);
  const int32_t e0 = fptr[q], e1 = fptr[q + 1];
  f32x4m acc = {0.f, 0.f, 0.f, 0.f}, accF = {0.f, 0.f, 0.f, 0.f};
  for (int32_t base = e0 + 64 * wv; base < e1; base += 64 * NW) {  // wave w: pieces w, w + NW, ... of 64 entries
    const int cnt = (e1 - base < 64) ? e1 - base : 64;
    const int32_t e = base + (lane < cnt ? lane : cnt - 1);
    const int32_t k = fcol[e];
    const float v = fval[e];
    const float vf = fv ? v : 1.f;
    const int32_t r = lrel[k];
    const int32_t o = lnode_ord[k];
    const int32_t j = HI ? lnode[o] : 0;
    float w[BT], wf[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      if constexpr (HI) w[b] = comp[(int64_t)r * BT + b];
      if constexpr (HF) wf[b] = compF[(int64_t)r * BT + b];
    }
    for (int i0 = 0; i0 < cnt; i0 += U) {
      f32x4m x[U][HI ? BT : 1], p[U][HF ? BT : 1];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // every load of the step, unconditional at clamped entries
        const int ii = (i0 + u < cnt) ? i0 + u : cnt - 1;
        if constexpr (HI) {
          const int64_t jj = __builtin_amdgcn_readlane(j, ii);
#pragma unroll
          for (int b = 0; b < BT; ++b) x[u][b] = V4[(jj * BT + b) * F4 + lo];
        }
        if constexpr (HF) {
          const int64_t oo = __builtin_amdgcn_readlane(o, ii);
#pragma unroll
          for (int b = 0; b < BT; ++b) p[u][b] = P4[(oo * BT + b) * F4 + lo];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u < cnt) {  // wave uniform
          const int ii = i0 + u;
          if constexpr (HI) {
            f32x4m m = lane_f(w[0], ii) * x[u][0];
#pragma unroll
            for (int b = 1; b < BT; ++b) m += lane_f(w[b], ii) * x[u][b];
            acc += lane_f(v, ii) * m;
          }
          if constexpr (HF) {
            f32x4m m = lane_f(wf[0], ii) * p[u][0];
#pragma unroll
            for (int b = 1; b < BT; ++b) m += lane_f(wf[b], ii) * p[u][b];
            accF += lane_f(vf, ii) * m;
          }
        }
      }
    }
  }
  if constexpr (HF) acc = HI ? acc + accF : accF;
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

// HI: dV rows of the input table, D [L][B], ||dV_j||^2; HF: dP rows of the feature table (by rank t), DF [L][B]
// from dm_F = sum w_e dY (w_e = v_e when `fv`, else 1).  The dY rows of a column are read once for both.
template <int BT, int NW, bool HI = true, bool HF = false>
__global__ __launch_bounds__(64 * NW) void k_sup_wide_bwd(const int32_t *__restrict__ lnode,
                                                      const int32_t *__restrict__ lnptr,
                                                      const int32_t *__restrict__ lrel,
                                                      const int32_t *__restrict__ lptr,
                                                      const int32_t *__restrict__ lrow_rank,
                                                      const float *__restrict__ lval, int64_t NL,
                                                      const float *__restrict__ dY, int64_t ldY,
                                                      const float *__restrict__ V, const float *__restrict__ comp,
                                                      int F, float *__restrict__ dV, float *__restrict__ D,
                                                      double *__restrict__ sq_node,
                                                      const float *__restrict__ P = nullptr,
                                                      const float *__restrict__ compF = nullptr, int fv = 0,
                                                      float *__restrict__ dP = nullptr,
                                                      float *__restrict__ DF = nullptr) {
  constexpr int U = 8;  // dY rows in flight together
  constexpr int NT = (HI ? 1 : 0) + (HF ? 1 : 0);
  __shared__ f32x4m s_acc[NW][NT * BT][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t t = blockIdx.x;
  const int F4 = F >> 2;
  const bool active = lane < F4;
  const int lo = active ? lane : 0;
  const int64_t ld4 = ldY >> 2;
  const f32x4m *V4 = reinterpret_cast<const f32x4m *>(V);
  const f32x4m *P4 = reinterpret_cast<const f32x4m *>(P);
  const f32x4m *dY4 = reinterpret_cast<const f32x4m *>(dY);
  const f32x4m zero = {0.f, 0.f, 0.f, 0.f};
  const int64_t j = lnode[t];
  const int32_t k0 = lnptr[t], k1 = lnptr[t + 1];
  f32x4m Vb[HI ? BT : 1], accV[HI ? BT : 1], Pb[HF ? BT : 1], accP[HF ? BT : 1];
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    if constexpr (HI) {
      Vb[b] = active ? V4[(j * BT + b) * F4 + lane] : zero;
      accV[b] = zero;
    }
    if constexpr (HF) {
      Pb[b] = active ? P4[(t * BT + b) * F4 + lane] : zero;
      accP[b] = zero;
    }
  }
  // wave w takes the node's live columns w, w + NW, ...: 64 of them per round
  for (int32_t kb = k0 + wv; kb < k1; kb += 64 * NW) {
    // the relation, entry range and comp row of up to 64 live columns of the node, one coalesced load each
    const int ncol = (k1 - kb + NW - 1) / NW < 64 ? (k1 - kb + NW - 1) / NW : 64;
    const int32_t kl = kb + NW * (lane < ncol ? lane : ncol - 1);
    const int32_t r = lrel[kl], p0 = lptr[kl], p1 = lptr[kl + 1];
    float w[BT], wf[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      if constexpr (HI) w[b] = comp[(int64_t)r * BT + b];
      if constexpr (HF) wf[b] = compF[(int64_t)r * BT + b];
    }
    for (int c = 0; c < ncol; ++c) {
      const int32_t a0 = __builtin_amdgcn_readlane(p0, c), a1 = __builtin_amdgcn_readlane(p1, c);
      f32x4m dm = zero, dmf = zero;
      for (int32_t eb = a0; eb < a1; eb += 64) {
        const int cnt = (a1 - eb < 64) ? a1 - eb : 64;
        const int32_t e = eb + (lane < cnt ? lane : cnt - 1);
        const int32_t rr = lrow_rank[e];
        const float vv = lval[e];
        const float vf = fv ? vv : 1.f;
        for (int i0 = 0; i0 < cnt; i0 += U) {
          f32x4m x[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int ii = (i0 + u < cnt) ? i0 + u : cnt - 1;
            x[u] = dY4[(int64_t)__builtin_amdgcn_readlane(rr, ii) * ld4 + lo];
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (i0 + u < cnt) {  // (wave uniform)
              if constexpr (HI) dm += lane_f(vv, i0 + u) * x[u];
              if constexpr (HF) dmf += lane_f(vf, i0 + u) * x[u];
            }
        }
      }
      const int64_t k = kb + (int64_t)NW * c;
      if constexpr (HI) {
        if (!active) dm = zero;
#pragma unroll
        for (int b = 0; b < BT; ++b) {
          accV[b] += lane_f(w[b], c) * dm;
          const f32x4m pr = dm * Vb[b];
          const float d = wave_sum((pr.x + pr.y) + (pr.z + pr.w));
          if (lane == 0) D[k * BT + b] = d;
        }
      }
      if constexpr (HF) {
        if (!active) dmf = zero;
#pragma unroll
        for (int b = 0; b < BT; ++b) {
          accP[b] += lane_f(wf[b], c) * dmf;
          const f32x4m pr = dmf * Pb[b];
          const float d = wave_sum((pr.x + pr.y) + (pr.z + pr.w));
          if (lane == 0) DF[k * BT + b] = d;
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    if constexpr (HI) s_acc[wv][b][lane] = accV[b];
    if constexpr (HF) s_acc[wv][(HI ? BT : 0) + b][lane] = accP[b];
  }
  __syncthreads();
  if (wv != 0) return;
  if constexpr (HF) {
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      f32x4m a = s_acc[0][(HI ? BT : 0) + b][lane];
#pragma unroll
      for (int w = 1; w < NW; ++w) a += s_acc[w][(HI ? BT : 0) + b][lane];  // (fixed order)
      if (active) *reinterpret_cast<f32x4m *>(dP + (t * BT + b) * F + 4 * lane) = a;
    }
  }
  if constexpr (HI) {
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

int mrgcn_support_wide_feat_fwd_f32(const mrgcn_support_t *q, const float *V, const float *comp, const float *P,
                                    const float *comp_F, int32_t feature_values, int32_t B, int32_t F, float *Y,
                                    int64_t ldY, int32_t relu, void *stream) {
  MRGCN_REQUIRE(q && q->has_forward, "the support was not created with MRGCN_SUPPORT_FORWARD");
  MRGCN_REQUIRE(P && comp_F && Y && (!V == !comp), "NULL (V and comp are both given or both NULL)");
  if (!wide_shape(B, F)) {
    set_error("mrgcn_support_wide_feat_fwd_f32: shape outside 1 <= B <= 4, 16 < F <= 256, F % 4 == 0");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(ldY >= F && ldY % 4 == 0, "ldY (>= F, a multiple of 4)");
  MRGCN_REQUIRE(((((uintptr_t)V) | ((uintptr_t)P) | ((uintptr_t)Y)) & 15) == 0, "V, P and Y must be 16-byte aligned");
  if (q->NR == 0) return MRGCN_OK;
  hipStream_t s = (hipStream_t)stream;
  constexpr int kFwdWaves = 16;
  const dim3 grid((unsigned)q->NR), tb(64 * kFwdWaves);
  const int fv = feature_values ? 1 : 0;
#define FEAT_FWD(BB, HI)                                                                                           \
  k_sup_wide_fwd<BB, kFwdWaves, HI, true><<<grid, tb, 0, s>>>(q->fptr, q->fcol, q->fval, q->lrel, q->lnode_ord,     \
                                                              q->lnode, q->NR, V, comp, F, Y, ldY, relu, P, comp_F, fv)
#define FEAT_FWD_B(HI)                \
  switch (B) {                        \
    case 1: FEAT_FWD(1, HI); break;   \
    case 2: FEAT_FWD(2, HI); break;   \
    case 3: FEAT_FWD(3, HI); break;   \
    default: FEAT_FWD(4, HI); break;  \
  }
  if (V) {
    FEAT_FWD_B(true)
  } else {
    FEAT_FWD_B(false)
  }
#undef FEAT_FWD_B
#undef FEAT_FWD
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_support_wide_feat_bwd_workspace(const mrgcn_support_t *q, int32_t B) {
  if (!q || B <= 0) return 0;
  // D_I [L][B] | D_F [L][B] | slab [chunks][B] (shared: the two dcomp passes run one after the other) | ||dV_j||^2
  return ((2 * q->L + q->wide.n_chunks) * (int64_t)B + 1) / 2 * 2 + 2 * (q->NL > 0 ? q->NL : 1);
}

int mrgcn_support_wide_feat_bwd_f32(const mrgcn_support_t *q, const float *dY, int64_t ldY, const float *V,
                                    const float *comp, const float *P, const float *comp_F, int32_t feature_values,
                                    int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp, double *dV_sumsq,
                                    float *dP, float *dcomp_F, float *workspace, int64_t workspace_floats,
                                    void *stream) {
  MRGCN_REQUIRE(q && q->has_forward, "the support was not created with MRGCN_SUPPORT_FORWARD");
  MRGCN_REQUIRE(dY && P && comp_F && dP && dcomp_F, "NULL");
  MRGCN_REQUIRE((!V && !comp && !dV && !dcomp) || (V && comp && dV && dcomp),
                "V, comp, dV and dcomp are all given (input term) or all NULL");
  if (!wide_shape(B, F)) {
    set_error("mrgcn_support_wide_feat_bwd_f32: shape outside 1 <= B <= 4, 16 < F <= 256, F % 4 == 0");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(ldY >= F && ldY % 4 == 0, "ldY (>= F, a multiple of 4)");
  MRGCN_REQUIRE(((((uintptr_t)V) | ((uintptr_t)dY) | ((uintptr_t)dV) | ((uintptr_t)P) | ((uintptr_t)dP)) & 15) == 0,
                "dY, V, dV, P and dP must be 16-byte aligned");
  MRGCN_REQUIRE(workspace && workspace_floats >= mrgcn_support_wide_feat_bwd_workspace(q, B) &&
                    (((uintptr_t)workspace) & 7) == 0,
                "workspace (mrgcn_support_wide_feat_bwd_workspace floats, 8-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const mrgcn_plan *p = q->plan;
  const bool hi = V != nullptr;
  if (hi && dense)
    MRGCN_HIP_TRY(mrgcn::fill_async(dV, 0, (size_t)p->num_nodes * B * F * sizeof(float), s));
  float *D = workspace;
  float *DF = D + q->L * (int64_t)B;
  float *slab = DF + q->L * (int64_t)B;
  double *sq_node =
      reinterpret_cast<double *>(workspace + ((2 * q->L + q->wide.n_chunks) * (int64_t)B + 1) / 2 * 2);
  const int fv = feature_values ? 1 : 0;
  if (q->NL > 0) {
    constexpr int kBwdWaves = 4;
    const dim3 grid((unsigned)q->NL), tb(64 * kBwdWaves);
#define FEAT_BWD(BB, HI)                                                                                            \
  k_sup_wide_bwd<BB, kBwdWaves, HI, true><<<grid, tb, 0, s>>>(q->lnode, q->lnptr, q->lrel, q->lptr, q->lrow_rank,    \
                                                              q->lval, q->NL, dY, ldY, V, comp, F, dV, D, sq_node,   \
                                                              P, comp_F, fv, dP, DF)
#define FEAT_BWD_B(HI)                \
  switch (B) {                        \
    case 1: FEAT_BWD(1, HI); break;   \
    case 2: FEAT_BWD(2, HI); break;   \
    case 3: FEAT_BWD(3, HI); break;   \
    default: FEAT_BWD(4, HI); break;  \
  }
    if (hi) {
      FEAT_BWD_B(true)
    } else {
      FEAT_BWD_B(false)
    }
#undef FEAT_BWD_B
#undef FEAT_BWD
    MRGCN_HIP_TRY(hipGetLastError());
  }
  if (hi) {
    const int rc = support_dcomp_from_D(q, D, B, slab, sq_node, q->NL, dcomp, dV_sumsq, s);
    if (rc != MRGCN_OK) return rc;
  }
  return support_dcomp_from_D(q, DF, B, slab, nullptr, 0, dcomp_F, nullptr, s);
}

}  // extern "C"
