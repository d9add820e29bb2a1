// The basis-GEMM form of a wide layer's feature term on a forward support (masked_wide.hip, two tables): instead of
// W_F[r] = sum_b comp_F[r][b] V_F[b] (graph.py:83-85) and X . W_F[r] for every relation (graph.py:93-95), the live
// nodes' rows are multiplied with the B bases once,
//     P[l][b] = X[l] . V_F[b]                         [NL][B][F], l = live-node rank (one product K -> B F)
// and the relation mix happens in the gather (sum_b comp_F[r][b] P[l][b]).  The gradients of that product:
//     dX[l]   = sum_b dP[l][b] . V_F[b]^T             (a reduction over B F)
//     dV_F[b] = X^T . dP[:, b]                        (a reduction over the live nodes)
// All three on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32), 64 x 64 block tiles, 4 waves of 32 x 32, element
// loaders (X rows are any width K >= 1 and any stride: nothing is copied or padded).  X rows are read through the
// live-node list when the caller hands over the whole feature matrix (x_by_node).  dV_F sums fixed chunks of
// kRowsPerChunk live nodes into a workspace and adds the chunks in order in a second pass: no atomics, the same bits
// every run.
#include "common.hpp"

namespace mrgcn {
namespace {

using f32x4b = __attribute__((ext_vector_type(4))) float;

constexpr int kBT = 64, kBK = 16, kBP = kBK + 4;  // tile, K step, padded LDS row
constexpr int kRowsPerChunk = 512;                // live nodes per dV_F partial (a multiple of kBK)

struct BxArgs {
  const float *X;
  int64_t ldx;
  const int32_t *xrow;  // nullable: the X row of live rank l is xrow[l]
  const float *VF, *dP;
  float *C;
  int64_t ldc;
  int M, N, K;  // the product's shape
  int Kx, F, BF;
};

// MODE 0: P = X . [V_F[0] | ... | V_F[B-1]]     M = NL, N = B F, K = Kx,   C[m][n] (ldc)
// MODE 1: dX = dP . V_F^T                        M = NL, N = Kx,  K = B F,  C[m][n] (ldc)
// MODE 2: dV_F partial = X^T . dP over a chunk   M = Kx, N = B F, K = NL,   C[z][m][n]
template <int MODE>
__device__ __forceinline__ float bx_a(const BxArgs &g, int m, int k, int kend) {
  if (m >= g.M || k >= kend) return 0.f;
  if constexpr (MODE == 0) return g.X[(int64_t)(g.xrow ? g.xrow[m] : m) * g.ldx + k];
  else if constexpr (MODE == 1) return g.dP[(int64_t)m * g.BF + k];
  else return g.X[(int64_t)(g.xrow ? g.xrow[k] : k) * g.ldx + m];
}
template <int MODE>
__device__ __forceinline__ float bx_b(const BxArgs &g, int k, int n, int kend) {
  if (k >= kend || n >= g.N) return 0.f;
  if constexpr (MODE == 0) {
    const int b = n / g.F, f = n - b * g.F;
    return g.VF[((int64_t)b * g.Kx + k) * g.F + f];
  } else if constexpr (MODE == 1) {
    const int b = k / g.F, f = k - b * g.F;
    return g.VF[((int64_t)b * g.Kx + n) * g.F + f];
  } else {
    return g.dP[(int64_t)k * g.BF + n];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_bx_gemm(BxArgs g) {
  __shared__ __align__(16) float As[kBT][kBP];  // [m][k]
  __shared__ __align__(16) float Bs[kBT][kBP];  // [n][k]
  const int m0 = blockIdx.y * kBT, n0 = blockIdx.x * kBT;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;  // this wave's 32 x 32 quarter
  const int lm = lane & 15, kq = lane >> 4;
  const int kbeg = MODE == 2 ? (int)blockIdx.z * kRowsPerChunk : 0;
  const int kend = MODE == 2 ? (kbeg + kRowsPerChunk < g.K ? kbeg + kRowsPerChunk : g.K) : g.K;
  f32x4b acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4b{0.f, 0.f, 0.f, 0.f};
  // loader mapping: thread t fills As[t / 4][4 (t % 4) + 0..3] and the same of Bs
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;
  for (int k0 = kbeg; k0 < kend; k0 += kBK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[lr][lk + i] = bx_a<MODE>(g, m0 + lr, k0 + lk + i, kend);
      Bs[lr][lk + i] = bx_b<MODE>(g, k0 + lk + i, n0 + lr, kend);
    }
    __syncthreads();
    f32x4b av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      av[i] = *reinterpret_cast<const f32x4b *>(&As[wm + i * 16 + lm][4 * kq]);
      bv[i] = *reinterpret_cast<const f32x4b *>(&Bs[wn + i * 16 + lm][4 * kq]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // k slot kq of the s-th MFMA stands for k = k0 + 4 kq + s
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
      }
    __syncthreads();
  }
  // D: lane (n = lane & 15, q = lane >> 4) holds rows 4q + reg of its 16 x 16 tile
  float *C = MODE == 2 ? g.C + (int64_t)blockIdx.z * g.M * g.N : g.C;
  const int64_t ldc = MODE == 2 ? g.N : g.ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = m0 + wm + i * 16 + 4 * kq + reg, n = n0 + wn + j * 16 + lm;
        if (m < g.M && n < g.N) C[(int64_t)m * ldc + n] = acc[i][j][reg];
      }
}

// dV_F[b][k][f] = sum over chunks z (in order) of part[z][k][b F + f]
__global__ __launch_bounds__(256) void k_bx_dvf_sum(const float *__restrict__ part, int nz, int Kx, int F, int BF,
                                                    float *__restrict__ dVF) {
  const int64_t total = (int64_t)Kx * BF;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += part[(int64_t)z * total + i];
    const int k = (int)(i / BF), n = (int)(i - (int64_t)k * BF);
    const int b = n / F, f = n - b * F;
    dVF[((int64_t)b * Kx + k) * F + f] = s;
  }
}

int64_t dvf_chunks(int64_t NL) { return (NL + kRowsPerChunk - 1) / kRowsPerChunk; }

}  // namespace
}  // namespace mrgcn

extern "C" {

using namespace mrgcn;

int mrgcn_support_basis_xform_f32(const mrgcn_support_t *q, const float *X, int64_t ldX, int32_t x_by_node, int32_t K,
                                  const float *V_F, int32_t B, int32_t F, float *P, void *stream) {
  MRGCN_REQUIRE(q && X && V_F && P, "NULL");
  MRGCN_REQUIRE(K >= 1 && B >= 1 && F >= 1 && ldX >= K, "shape (K, B, F >= 1, ldX >= K)");
  MRGCN_REQUIRE((int64_t)B * F < (1 << 20) && q->NL < ((int64_t)1 << 31), "shape (B F, NL)");
  if (q->NL == 0) return MRGCN_OK;
  BxArgs g{X, ldX, x_by_node ? q->lnode : nullptr, V_F, nullptr, P, (int64_t)B * F, (int)q->NL, B * F, K, K, F, B * F};
  const dim3 grid((unsigned)((g.N + kBT - 1) / kBT), (unsigned)((g.M + kBT - 1) / kBT));
  k_bx_gemm<0><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_support_basis_xform_bwd_workspace(const mrgcn_support_t *q, int32_t K, int32_t B, int32_t F) {
  if (!q || K <= 0 || B <= 0 || F <= 0) return 0;
  return dvf_chunks(q->NL) * K * (int64_t)B * F;
}

int mrgcn_support_basis_xform_bwd_f32(const mrgcn_support_t *q, const float *dP, const float *X, int64_t ldX,
                                      int32_t x_by_node, int32_t K, const float *V_F, int32_t B, int32_t F, float *dX,
                                      int64_t ld_dX, float *dV_F, float *workspace, int64_t workspace_floats,
                                      void *stream) {
  MRGCN_REQUIRE(q && dP && X && V_F, "NULL");
  MRGCN_REQUIRE(K >= 1 && B >= 1 && F >= 1 && ldX >= K, "shape (K, B, F >= 1, ldX >= K)");
  MRGCN_REQUIRE((int64_t)B * F < (1 << 20) && q->NL < ((int64_t)1 << 31), "shape (B F, NL)");
  hipStream_t s = (hipStream_t)stream;
  const int NL = (int)q->NL, BF = B * F;
  if (dX && NL > 0) {
    MRGCN_REQUIRE(ld_dX >= K, "ld_dX >= K");
    BxArgs g{X, ldX, nullptr, V_F, dP, dX, ld_dX, NL, K, BF, K, F, BF};
    const dim3 grid((unsigned)((K + kBT - 1) / kBT), (unsigned)((NL + kBT - 1) / kBT));
    k_bx_gemm<1><<<grid, dim3(256), 0, s>>>(g);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  if (dV_F) {
    const int64_t nz = dvf_chunks(NL);
    MRGCN_REQUIRE(nz == 0 || (workspace && workspace_floats >= mrgcn_support_basis_xform_bwd_workspace(q, K, B, F)),
                  "workspace (mrgcn_support_basis_xform_bwd_workspace floats)");
    if (nz > 0) {
      BxArgs g{X, ldX, x_by_node ? q->lnode : nullptr, V_F, dP, workspace, BF, K, BF, NL, K, F, BF};
      const dim3 grid((unsigned)((BF + kBT - 1) / kBT), (unsigned)((K + kBT - 1) / kBT), (unsigned)nz);
      k_bx_gemm<2><<<grid, dim3(256), 0, s>>>(g);
      MRGCN_HIP_TRY(hipGetLastError());
    }
    const int64_t total = (int64_t)K * BF;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 1024);
    k_bx_dvf_sum<<<dim3(blocks), dim3(256), 0, s>>>(workspace, (int)nz, K, F, BF, dV_F);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  return MRGCN_OK;
}

}  // extern "C"
