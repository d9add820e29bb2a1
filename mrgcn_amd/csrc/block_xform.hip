// Block-diagonal relation transform (Schlichtkrull et al. 2018, "Modeling Relational Data with Graph Convolutional
// Networks", eq. 4): W_r = blockdiag(Q_r[0], ..., Q_r[NB-1]) with blocks of ki x fo = (K / NB) x (F / NB), so input
// columns b ki .. b ki + ki - 1 feed output columns b fo .. b fo + fo - 1 only.  Per compact column c = (j_c, r_c):
//     Out[o(c), b fo + q]  = sum_{k < ki} X[j_c, b ki + k] . W[r_c, b, k, q]                       (forward)
//     dX[j, b ki + k]      = sum_{c in node j} sum_{q < fo} W[r_c, b, k, q] . dM[c, b fo + q]     (backward)
//     dW[r, b, k, q]       = sum_{c : r_c = r} X[j_c, b ki + k] . dM[c, b fo + q]
// W is [R][NB][ki][fo] = R slabs of K fo floats.  The blocks are 1 x 1 to 64 x 64 and a column costs 2 K fo FLOPs against
// 4 (K + F) bytes of rows: VALU work behind a row stream, not matrix-core work.
//
// Layout of the launches: the plan's relation-major order (RPERM, cut into chunks of <= kRelChunk columns of one
// (band, relation) group) is cut once more into UNITS of kBlkCols columns; unit u = 4 chunk + sub.  One block per unit,
// the relation's slab staged once in LDS (forward), a wave per column with lanes over the output features.
//
// Summation orders (all fixed; no float atomics anywhere in this file):
//   forward  k rising, every product and every sum rounded to float32 separately (contraction off): equal to the numpy
//            mirror mrgcn_amd.host.block_transform32 bit for bit;
//   dX       one block per node: four consecutive runs of its columns, one per wave, each in rising compact id with q
//            rising inside a column; the four partial rows are added in wave order;
//   dW       a unit's columns in RPERM order into a partial slab of K fo floats; a second launch adds a relation's
//            slabs in chunk order, units rising inside a chunk.  A relation without columns gets zeros.
#include "common.hpp"

namespace mrgcn {
namespace {

constexpr int kBlkCols = 256;                            // compact columns per unit
constexpr int kBlkSubs = kRelChunk / kBlkCols;           // units per chunk of the plan's order
constexpr int kBlkMaxW = 256;                            // K, F <= this (the widths the SpMM views serve)
constexpr int kBlkMaxBlock = 64;                         // ki, fo <= this
constexpr int kBlkDxSlab = 1024;                         // slabs of up to this many floats are staged per wave in dX
constexpr int kBlkTile = 16;                             // columns staged per step of the dW walk
constexpr int kBlkOutPerThread = 8;                      // dW outputs a thread keeps in registers per sweep
constexpr int kBlkSweep = 256 * kBlkOutPerThread;        // dW outputs per sweep of a block
static_assert(kRelChunk % kBlkCols == 0, "units cut chunks evenly");

struct BlkUnit {
  int rel, beg, end;  // relation, RPERM range; beg >= end: nothing to do
};

__device__ __forceinline__ BlkUnit blk_unit(const int32_t *__restrict__ chunk_rel, const int32_t *__restrict__ chunk_beg,
                                            const int32_t *__restrict__ chunk_end, int u) {
  const int ch = u / kBlkSubs, sub = u - ch * kBlkSubs;
  BlkUnit t;
  t.rel = chunk_rel[ch];
  const int cend = chunk_end[ch];
  t.beg = chunk_beg[ch] + sub * kBlkCols;
  t.end = t.beg + kBlkCols < cend ? t.beg + kBlkCols : cend;
  return t;
}

// grid: one block per unit; dynamic LDS: K fo floats (the relation's slab) + 4 x kBlkMaxW (a wave's X row)
__global__ __launch_bounds__(256) void k_blk_fwd(const int32_t *__restrict__ chunk_rel, const int32_t *__restrict__ chunk_beg,
                                                 const int32_t *__restrict__ chunk_end, const int32_t *__restrict__ rnode,
                                                 const int32_t *__restrict__ rout, const float *__restrict__ X, int64_t ldX,
                                                 int K, const float *__restrict__ W, int ki, int fo, int F,
                                                 float *__restrict__ Out, int64_t ldOut) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) float blk_lds[];
  const BlkUnit t = blk_unit(chunk_rel, chunk_beg, chunk_end, blockIdx.x);
  if (t.beg >= t.end) return;  // (the whole block: nobody waits at the barrier below)
  const int slab = K * fo;
  float *Ws = blk_lds;
  const float *Wr = W + (int64_t)t.rel * slab;
  for (int i = threadIdx.x; i < slab; i += 256) Ws[i] = Wr[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float *xs = blk_lds + slab + wv * kBlkMaxW;
  const int ld = (int)ldOut;
  for (int i = t.beg + wv; i < t.end; i += 4) {
    const float *x = X + (int64_t)rnode[i] * ldX;
    float *o = Out + (int64_t)rout[i] * ldOut;
    for (int k = lane; k < K; k += 64) xs[k] = x[k];
    wave_lds_fence();
    for (int f = lane; f < ld; f += 64) {
      float acc = 0.f;
      if (f < F) {
        const int b = f / fo, q = f - b * fo;
        const float *xb = xs + b * ki, *wb = Ws + b * ki * fo + q;
        for (int k = 0; k < ki; ++k) {
          const float p = xb[k] * wb[k * fo];
          acc = acc + p;
        }
      }
      o[f] = acc;
    }
    wave_lds_fence();
  }
}

// grid: one block per node.  Its columns NPTR[j] .. NPTR[j+1] are cut into four consecutive runs, one per wave; a wave adds
// its run in rising compact id (q rising inside a column) and the four partial rows are added in wave order: a fixed
// order whatever the launch.  The next column's dM row and weight slab are loaded into registers while the current
// one is computed from LDS (a hub node's walk is a chain of dependent loads otherwise).  Every row of dX is written.
__global__ __launch_bounds__(256) void k_blk_dx(const int32_t *__restrict__ nptr, const int32_t *__restrict__ urel,
                                                const float *__restrict__ dM, int64_t ldM, const float *__restrict__ W,
                                                int K, int ki, int fo, int F, float *__restrict__ dX, int64_t lddX) {
  __shared__ __align__(16) float gs[4][kBlkMaxW];
  __shared__ __align__(16) float wsh[4][kBlkDxSlab];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j = blockIdx.x;
  const int c0 = nptr[j], c1 = nptr[j + 1];
  const int per = (c1 - c0 + 3) >> 2;
  const int a = c0 + wv * per < c1 ? c0 + wv * per : c1, b = a + per < c1 ? a + per : c1;
  constexpr int NK = kBlkMaxW / 64, NS = kBlkDxSlab / 64;
  float acc[NK];
  int woff[NK], goff[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    acc[i] = 0.f;
    const int kk = lane + 64 * i;
    const int kc = kk < K ? kk : 0;  // (clamped: lanes past K compute on row 0 and store nothing)
    woff[i] = kc * fo;
    goff[i] = (kc / ki) * fo;
  }
  const int slab = K * fo;
  // a slab of up to kBlkDxSlab floats goes through the wave's LDS, read with whole-line loads: a lane's fo weights are
  // fo floats at a stride of fo between lanes, which read from memory touches every line of the slab fo times
  const bool stage = slab <= kBlkDxSlab;
  float *g = gs[wv], *wl = wsh[wv];
  float gn[NK], wn[NS];
  const float *Wr = W;
  auto fetch = [&](int c) {  // straight-line loads at clamped positions
    const float *gm = dM + (int64_t)c * ldM;
    Wr = W + (int64_t)urel[c] * slab;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int f = lane + 64 * i;
      gn[i] = gm[f < F ? f : 0];
    }
    if (stage) {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int e = lane + 64 * i;
        wn[i] = Wr[e < slab ? e : 0];
      }
    }
  };
  if (a < b) fetch(a);
  for (int c = a; c < b; ++c) {
    const float *Wc = Wr;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int f = lane + 64 * i;
      if (f < F) g[f] = gn[i];
    }
    if (stage) {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int e = lane + 64 * i;
        if (e < slab) wl[e] = wn[i];
      }
    }
    wave_lds_fence();
    if (c + 1 < b) fetch(c + 1);
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      if (64 * i < K) {
        const float *gb = g + goff[i];
        float s = acc[i];
        if (stage) {
          const float *w = wl + woff[i];
          for (int q = 0; q < fo; ++q) s += w[q] * gb[q];
        } else {
          const float *w = Wc + woff[i];
          for (int q = 0; q < fo; ++q) s += w[q] * gb[q];
        }
        acc[i] = s;
      }
    }
    wave_lds_fence();
  }
  // the four partial rows, added in wave order
#pragma unroll
  for (int i = 0; i < NK; ++i) g[lane + 64 * i] = acc[i];
  __syncthreads();
  const int kk = threadIdx.x;
  if (kk < K) dX[j * lddX + kk] = ((gs[0][kk] + gs[1][kk]) + gs[2][kk]) + gs[3][kk];
}

// grid: one block per unit; the partial slab of unit u goes to part[u][K fo].  dynamic LDS: kBlkTile x (K + F) floats
__global__ __launch_bounds__(256) void k_blk_dw_part(const int32_t *__restrict__ chunk_rel, const int32_t *__restrict__ chunk_beg,
                                                     const int32_t *__restrict__ chunk_end, const int32_t *__restrict__ rperm,
                                                     const int32_t *__restrict__ rnode, const float *__restrict__ X, int64_t ldX,
                                                     int K, const float *__restrict__ dM, int64_t ldM, int ki, int fo, int F,
                                                     float *__restrict__ part) {
  extern __shared__ __align__(16) float blk_lds[];
  const BlkUnit t = blk_unit(chunk_rel, chunk_beg, chunk_end, blockIdx.x);
  if (t.beg >= t.end) return;  // (an empty unit's slab is neither written nor read)
  const int slab = K * fo;
  float *xs = blk_lds, *gs = blk_lds + kBlkTile * K;
  float *out = part + (int64_t)blockIdx.x * slab;
  for (int o0 = 0; o0 < slab; o0 += kBlkSweep) {
    float acc[kBlkOutPerThread];
    int xoff[kBlkOutPerThread], goff[kBlkOutPerThread];
#pragma unroll
    for (int i = 0; i < kBlkOutPerThread; ++i) {
      acc[i] = 0.f;
      const int o = o0 + i * 256 + threadIdx.x;
      const int oc = o < slab ? o : 0;  // (clamped: threads past the slab compute on output 0 and store nothing)
      const int kk = oc / fo, q = oc - kk * fo;
      xoff[i] = kk;
      goff[i] = (kk / ki) * fo + q;
    }
    for (int i0 = t.beg; i0 < t.end; i0 += kBlkTile) {
      const int nt = t.end - i0 < kBlkTile ? t.end - i0 : kBlkTile;
      __syncthreads();  // the previous tile is read
      for (int e = threadIdx.x; e < nt * K; e += 256) {
        const int tt = e / K, k = e - tt * K;
        xs[e] = X[(int64_t)rnode[i0 + tt] * ldX + k];
      }
      for (int e = threadIdx.x; e < nt * F; e += 256) {
        const int tt = e / F, f = e - tt * F;
        gs[e] = dM[(int64_t)rperm[i0 + tt] * ldM + f];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kBlkOutPerThread; ++i) {
        if (o0 + i * 256 < slab) {  // (uniform over the block)
          float a = acc[i];
          for (int tt = 0; tt < nt; ++tt) a += xs[tt * K + xoff[i]] * gs[tt * F + goff[i]];
          acc[i] = a;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBlkOutPerThread; ++i) {
      const int o = o0 + i * 256 + threadIdx.x;
      if (o < slab) out[o] = acc[i];
    }
  }
}

// grid: (ceil(K fo / 256), R): dW[r][o] = the slabs of relation r's units, chunks in the order of relchunk_ids, units
// rising inside a chunk
__global__ __launch_bounds__(256) void k_blk_dw_sum(const int32_t *__restrict__ chunk_ptr, const int32_t *__restrict__ chunk_ids,
                                                    const int32_t *__restrict__ chunk_beg, const int32_t *__restrict__ chunk_end,
                                                    const float *__restrict__ part, int slab, float *__restrict__ dW) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (o >= slab) return;
  float s = 0.f;
  for (int ci = chunk_ptr[r]; ci < chunk_ptr[r + 1]; ++ci) {
    const int ch = chunk_ids[ci];
    const int n = chunk_end[ch] - chunk_beg[ch];
    for (int sub = 0; sub * kBlkCols < n; ++sub) s += part[((int64_t)ch * kBlkSubs + sub) * slab + o];
  }
  dW[(int64_t)r * slab + o] = s;
}

bool blk_shape_ok(int K, int F, int NB) {
  if (NB < 1 || K < 1 || F < 1 || K > kBlkMaxW || F > kBlkMaxW || K % NB || F % NB) return false;
  const int ki = K / NB, fo = F / NB;
  return ki <= kBlkMaxBlock && fo <= kBlkMaxBlock && (int64_t)K * fo * 4 <= 64 * 1024;
}

}  // namespace
}  // namespace mrgcn

extern "C" {

using namespace mrgcn;

int32_t mrgcn_block_transform_supported(const mrgcn_plan_t *p, int32_t K, int32_t F, int32_t NB) {
  return p && p->num_relations < 65536 && blk_shape_ok(K, F, NB) ? 1 : 0;
}

int mrgcn_block_transform_fwd_f32(const mrgcn_plan_t *p, const float *X, int64_t ldX, int32_t K, const float *W,
                                  int32_t NB, int32_t F, float *Out, int64_t ldOut, int32_t operand_order,
                                  void *stream) {
  MRGCN_REQUIRE(p && X && W && Out, "NULL");
  MRGCN_REQUIRE(mrgcn_block_transform_supported(p, K, F, NB),
                "block transform: NB divides K and F, blocks of 1..64 x 1..64, K, F <= 256, K (F / NB) <= 16384");
  MRGCN_REQUIRE(ldX >= K && ldOut >= F && ldOut <= INT32_MAX, "ldX >= K, F <= ldOut <= INT32_MAX");
  if (p->ncols == 0 || p->n_relchunks == 0) return MRGCN_OK;
  const int ki = K / NB, fo = F / NB;
  const size_t lds = ((size_t)K * fo + 4 * kBlkMaxW) * sizeof(float);
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_blk_fwd, lds));
  k_blk_fwd<<<dim3((unsigned)p->n_relchunks * kBlkSubs), dim3(256), lds, (hipStream_t)stream>>>(
      p->relchunk_rel, p->relchunk_beg, p->relchunk_end, p->rnode, operand_order ? p->rmpos : p->rperm, X, ldX, K, W, ki,
      fo, F, Out, ldOut);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_block_transform_bwd_workspace(const mrgcn_plan_t *p, int32_t K, int32_t F, int32_t NB, int32_t need_dX,
                                            int32_t need_dW) {
  (void)need_dX;
  if (!p || !blk_shape_ok(K, F, NB) || !need_dW) return 0;
  return (int64_t)p->n_relchunks * kBlkSubs * K * (F / NB);
}

int mrgcn_block_transform_bwd_f32(const mrgcn_plan_t *p, const float *dM, int64_t ldM, const float *X, int64_t ldX,
                                  int32_t K, const float *W, int32_t NB, int32_t F, float *dX, int64_t lddX, float *dW,
                                  float *workspace, int64_t workspace_floats, void *stream) {
  MRGCN_REQUIRE(p && dM, "NULL");
  MRGCN_REQUIRE(mrgcn_block_transform_supported(p, K, F, NB),
                "block transform: NB divides K and F, blocks of 1..64 x 1..64, K, F <= 256, K (F / NB) <= 16384");
  MRGCN_REQUIRE(ldM >= F, "ldM >= F");
  hipStream_t s = (hipStream_t)stream;
  const int ki = K / NB, fo = F / NB, slab = K * fo;
  if (dX) {
    MRGCN_REQUIRE(W && lddX >= K, "dX needs W and lddX >= K");
    if (p->num_nodes > 0) {
      k_blk_dx<<<dim3((unsigned)p->num_nodes), dim3(256), 0, s>>>(p->nptr, p->urel, dM, ldM, W, K, ki, fo, F, dX, lddX);
      MRGCN_HIP_TRY(hipGetLastError());
    }
  }
  if (dW) {
    MRGCN_REQUIRE(X && ldX >= K, "dW needs X and ldX >= K");
    const int64_t need = mrgcn_block_transform_bwd_workspace(p, K, F, NB, 0, 1);
    MRGCN_REQUIRE(need == 0 || (workspace && workspace_floats >= need),
                  "workspace (mrgcn_block_transform_bwd_workspace floats)");
    if (p->n_relchunks > 0) {
      const size_t lds = (size_t)kBlkTile * (K + F) * sizeof(float);
      k_blk_dw_part<<<dim3((unsigned)p->n_relchunks * kBlkSubs), dim3(256), lds, s>>>(
          p->relchunk_rel, p->relchunk_beg, p->relchunk_end, p->rperm, p->rnode, X, ldX, K, dM, ldM, ki, fo, F, workspace);
      MRGCN_HIP_TRY(hipGetLastError());
    }
    if (p->num_relations > 0) {
      k_blk_dw_sum<<<dim3((unsigned)((slab + 255) / 256), (unsigned)p->num_relations), dim3(256), 0, s>>>(
          p->relchunk_ptr, p->relchunk_ids, p->relchunk_beg, p->relchunk_end, workspace, slab, dW);
      MRGCN_HIP_TRY(hipGetLastError());
    }
  }
  return MRGCN_OK;
}

}  // extern "C"
