// The backward of a semi-supervised epoch on a GRADIENT SUPPORT (common.hpp: mrgcn_support; built in plan.hip).
//
// The reference's autograd runs the backward of graph.py:62-102 densely: dD = A^T dY over all (R*N) rows although the
// loss (node_classification.py:439-444) only touches the labelled rows.  Rounds 1-3 skipped the zeros per epoch (flag
// the live rows of dY, mark the columns they touch, compact lists in LDS, skip dead nodes).  With the label set fixed
// all of that is the same every epoch, so it is decided ONCE: the support numbers the live columns 0..L-1 in
// (node, relation) order and keeps, per live column, only the entries that sit in live rows.  Per epoch:
//
//   dM[k]      = sum over kept entries (k_spmm on the filtered view: a plain CSR product over L short rows)
//   D[k][b]    = <dM[k], V[j_k][b]>,  ||dV||^2            one pass over the live nodes' V blocks: k_mix_bwd_stream (a
//                                                         one-shot grid, blocks as 16-byte pieces) or k_mix_bwd_sup
//                                                         (resident, comp in LDS); lane = basis in the arithmetic, a
//                                                         node's live columns are consecutive rows
//   dcomp[r]   = sum of the D rows of relation r          relation-major walk of D (k_dcomp_chunks / _final)
//   dW, dX     = the matrix-core transforms on the support's relation-major lists (xform_mfma.hip, unchanged kernels)
//   Adam       = k_adam_rows_fused with (node -> live range, relation per live column) in place of the plan's arrays
//
// No atomics, no flags, no zero fills: every output is written whole, in a fixed order.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.hpp"
#include "config.hpp"

namespace mrgcn {
namespace {

constexpr int kSupTB = 512;
constexpr int kSqParts = 2048;  // per-block partial sums of ||dV||^2 (doubles), added in block order by k_dcomp_final
// list entries per wave of the one-shot form.  AM epoch, kernel medians under the tracer on one box: the resident
// kernel 568 us, one entry per wave 519, two 452, four 447 (68 VGPRs, seven waves per SIMD): two kept
constexpr int kStreamNPW = 2;

// F floats of one basis row (rows 4 F bytes apart: 8-byte aligned when F is even).  EXACT: F == FT, known at compile
// time — the loads are then straight-line code (a run-time F puts every piece behind a branch, and the waitcnt pass
// drains all outstanding loads at the first use behind a merge: DESIGN §3, "straight-line loads")
typedef float f32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
template <int FT, bool EXACT>
__device__ __forceinline__ void load_basis_row(const float *__restrict__ p, int F, float (&v)[FT]) {
  if constexpr (EXACT) {
    if constexpr ((FT & 1) == 0) {
#pragma unroll
      for (int o = 0; o + 4 <= FT; o += 4) {
        const f32x4_a8 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_a8 *>(p + o));  // (read once per epoch)
        v[o] = t.x; v[o + 1] = t.y; v[o + 2] = t.z; v[o + 3] = t.w;
      }
      if constexpr ((FT & 3) != 0) {
        typedef float f32x2_nt __attribute__((ext_vector_type(2)));
        const f32x2_nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x2_nt *>(p + (FT & ~3)));
        v[FT & ~3] = t.x;
        v[(FT & ~3) + 1] = t.y;
      }
    } else {
#pragma unroll
      for (int o = 0; o < FT; ++o) v[o] = p[o];
    }
    return;
  }
  if ((F & 1) == 0) {
#pragma unroll
    for (int o = 0; o < FT; o += 4) {
      if (o + 4 <= F && o + 4 <= FT) {
        const f32x4_a8 t = *reinterpret_cast<const f32x4_a8 *>(p + o);
        v[o] = t.x; v[o + 1] = t.y; v[o + 2] = t.z; v[o + 3] = t.w;
      } else {
#pragma unroll
        for (int u = o; u < o + 4 && u < FT; u += 2) {
          if (u < F) {
            const float2 t = *reinterpret_cast<const float2 *>(p + u);
            v[u] = t.x;
            if (u + 1 < FT) v[u + 1] = t.y;
          } else {
            v[u] = 0.f;
            if (u + 1 < FT) v[u + 1] = 0.f;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int o = 0; o < FT; ++o) v[o] = (o < F) ? p[o] : 0.f;
  }
}

// Norm-only backward of the basis mix over the live nodes (see the file comment).  A wave fetches the (node, live
// range) pairs of 64 live nodes with one coalesced load each and walks them NB at a time: the loads of NB nodes — lane
// b its 4 F-byte row of each node's V block, the 16-lane group q row klo + q of each node's dM rows and its relation —
// are issued back to back at clamped addresses in one basic block, then the nodes are finished one after the other
// (the pass is bound by bytes in flight per wave: one node at a time it ran at 2.9 TB/s of its own traffic).  `comp`
// lives in LDS (the relation ids arrive with the loads; a dependent global load per column would put a second round
// trip on every node).  v_readlane hands a dM row and its relation round; lane b stores D[k][b] (a live column's B
// products: one 4 B-byte row per column, coalesced) and keeps the column's share of its dV row for the squared norm.
// Nodes with more than four live columns (9 % at the AM shape) walk the rest of their columns with direct loads.
template <int FT, int NB, bool EXACT>
__global__ __launch_bounds__(kSupTB) void k_mix_bwd_sup(const int32_t *__restrict__ lnode,
                                                           const int32_t *__restrict__ lnptr,
                                                           const int32_t *__restrict__ lrel,
                                                           const float *__restrict__ dM, int64_t ldM,
                                                           const float *__restrict__ V, const float *__restrict__ comp,
                                                           int64_t NL, int R, int B, int F_, float *__restrict__ D,
                                                           double *__restrict__ sq_part, int epw) {
  const int F = EXACT ? FT : F_;  // (a compile-time constant in the shapes that matter)
  extern __shared__ __align__(16) float s_comp[];  // [R][B]
  for (int t = threadIdx.x; t < R * B; t += blockDim.x) s_comp[t] = comp[t];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = blockDim.x >> 6;
  const bool on = lane < B;
  const int b = on ? lane : 0;
  const int kq = lane >> 4, oq = lane & 15;
  const int oqc = oq < F ? oq : F - 1;
  const int64_t nwaves = (int64_t)gridDim.x * nw;
  float sq = 0.f;
  // (`epw` <= 64 list entries per wave and round: 64 on a large support; a small one spreads its few entries over many
  // waves instead of walking 64 of them as one serial chain)
  for (int64_t base = ((int64_t)blockIdx.x * nw + wv) * epw; base < NL; base += nwaves * epw) {
    const int64_t me = (base + lane < NL) ? base + lane : NL - 1;
    const int32_t jn = lnode[me], k0v = lnptr[me], k1v = lnptr[me + 1];
    const int cnt = (int)((NL - base < epw) ? NL - base : epw);
    for (int i0 = 0; i0 < cnt; i0 += NB) {
      int32_t klo[NB], khi[NB], rmine[NB];
      float v[NB][FT], dmine[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {  // every load of the step, unconditional at clamped addresses
        const int ii = (i0 + u < cnt) ? i0 + u : cnt - 1;
        const int32_t j = __builtin_amdgcn_readlane(jn, ii);
        klo[u] = __builtin_amdgcn_readlane(k0v, ii);
        khi[u] = __builtin_amdgcn_readlane(k1v, ii);
        load_basis_row<FT, EXACT>(V + ((int64_t)j * B + b) * F, F, v[u]);
        const int32_t kk = (klo[u] + kq < khi[u]) ? klo[u] + kq : klo[u];
        dmine[u] = dM[(int64_t)kk * ldM + oqc];
        rmine[u] = lrel[kk];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i0 + u < cnt) {  // wave uniform
          float acc[FT];
#pragma unroll
          for (int o = 0; o < FT; ++o) acc[o] = 0.f;
          const int nc = (khi[u] - klo[u] < 4) ? khi[u] - klo[u] : 4;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            if (t < nc) {  // wave uniform
              const int r = __builtin_amdgcn_readlane(rmine[u], 16 * t);
              const float w = s_comp[r * B + b];
              float d[FT];
#pragma unroll
              for (int o = 0; o < FT; ++o)
                d[o] = (o < F) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dmine[u]),
                                                                                      16 * t + o))
                               : 0.f;
              float dot = 0.f;
#pragma unroll
              for (int o = 0; o < FT; ++o) dot = fmaf(d[o], v[u][o], dot);
              if (on) D[(int64_t)(klo[u] + t) * B + b] = dot;
#pragma unroll
              for (int o = 0; o < FT; ++o) acc[o] = fmaf(w, d[o], acc[o]);
            }
          }
          for (int32_t kb = klo[u] + 4; kb < khi[u]; kb += 4) {  // (few nodes have more than four live columns)
            const int32_t kk = (kb + kq < khi[u]) ? kb + kq : kb;
            const float dm = dM[(int64_t)kk * ldM + oqc];
            const int32_t rm = lrel[kk];
            const int nc2 = (khi[u] - kb < 4) ? khi[u] - kb : 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (t < nc2) {
                const int r = __builtin_amdgcn_readlane(rm, 16 * t);
                const float w = s_comp[r * B + b];
                float d[FT];
#pragma unroll
                for (int o = 0; o < FT; ++o)
                  d[o] = (o < F) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dm), 16 * t + o))
                                 : 0.f;
                float dot = 0.f;
#pragma unroll
                for (int o = 0; o < FT; ++o) dot = fmaf(d[o], v[u][o], dot);
                if (on) D[(int64_t)(kb + t) * B + b] = dot;
#pragma unroll
                for (int o = 0; o < FT; ++o) acc[o] = fmaf(w, d[o], acc[o]);
              }
            }
          }
          if (on) {
#pragma unroll
            for (int o = 0; o < FT; ++o)
              if (o < F) sq = fmaf(acc[o], acc[o], sq);
          }
        }
      }
    }
  }
  __shared__ float s_sq[kSupTB / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  if (lane == 0) s_sq[wv] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += (double)s_sq[i];
    sq_part[blockIdx.x] = t;
  }
}

// k_mix_bwd_stream: the same pass as a ONE-SHOT grid, modelled on k_adam_rows_once (rgcn_fused.hip), which walks the
// same list at the fabric's one-shot rate.  A wave owns NPW consecutive list entries and ends: no persistent loop, no
// block-wide table, nothing shared between waves but the four squared-norm parts that meet behind the block's only
// barrier, at its very end.  Rounds of straight-line loads at clamped addresses: (1) the list entries (wave uniform),
// (2) the node's V block as B F / 4 contiguous 16-byte pieces, lane q piece q (+ 64 h), nontemporal, and with them the
// relation and dM row of the node's first four live columns (16-lane group kq: column klo + kq), (3) the comp rows of
// those columns from the (L2-resident) table, lane b: comp[r][b].  The pieces then cross a wave-private LDS tile
// (B F floats per node in flight) into k_mix_bwd_sup's register layout — lane b holds V[j][b][0..F) — and from there
// the arithmetic is k_mix_bwd_sup's, fmaf for fmaf: D has the same bits.  Nodes with more than four live columns go
// on four at a time, reloading rows and comp values as the Adam kernel does.
// Reach (the launcher): B F % 4 == 0, B F <= 1024 (NH <= 4), B <= 64, F <= 16 and EVEN (an odd F would put every
// other row of the tile off the 8-byte grid of the paired LDS reads: it keeps the resident kernel), V 16-byte aligned.
// EXACT: F == FT; otherwise FT = 16 and the rows are padded with zeros as k_mix_bwd_sup<FT, NB, false> pads them.
// ||dV||^2: a wave's lanes by xor shuffle, the block's four waves in wave order in double -> blk_part[block]; the fold
// blocks of k_dcomp_chunks bring those down to <= kSqParts doubles, k_dcomp_final adds them: a fixed order throughout.
using f32x4s = __attribute__((ext_vector_type(4))) float;
using f32x2s = __attribute__((ext_vector_type(2))) float;
template <int FT, int NH, int NPW, bool EXACT>
__global__ __launch_bounds__(256) void k_mix_bwd_stream(const int32_t *__restrict__ lnode,
                                                        const int32_t *__restrict__ lnptr,
                                                        const int32_t *__restrict__ lrel,
                                                        const float *__restrict__ dM, int64_t ldM,
                                                        const float *__restrict__ V, const float *__restrict__ comp,
                                                        int64_t NL, int B, int F_, float *__restrict__ D,
                                                        double *__restrict__ blk_part) {
  const int F = EXACT ? FT : F_;
  extern __shared__ __align__(16) float s_tile[];  // [4 waves][NPW][B F]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nv = (B * F) >> 2;  // 16-byte pieces of a block
  const bool on = lane < B;
  const int b = on ? lane : 0;
  const int kq = lane >> 4, oq = lane & 15;
  const int oqc = oq < F ? oq : F - 1;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + wv) * NPW;
  // round 1: the list entries (a wave past the end repeats the last entry and stores nothing for it)
  int64_t j[NPW];
  int32_t klo[NPW], khi[NPW];
#pragma unroll
  for (int u = 0; u < NPW; ++u) {
    const int64_t i = (i0 + u < NL) ? i0 + u : NL - 1;
    j[u] = lnode[i];
    klo[u] = lnptr[i];
    khi[u] = lnptr[i + 1];
  }
  // round 2: the blocks, and relation / gradient row of the first four live columns
  f32x4s pc[NPW][NH];
  int32_t rmine[NPW];
  float dmine[NPW];
#pragma unroll
  for (int u = 0; u < NPW; ++u) {
    const f32x4s *v4 = reinterpret_cast<const f32x4s *>(V) + j[u] * (int64_t)nv;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int q = (lane + 64 * h < nv) ? lane + 64 * h : nv - 1;
      pc[u][h] = __builtin_nontemporal_load(v4 + q);  // (read once per epoch)
    }
    const int32_t kk = (klo[u] + kq < khi[u]) ? klo[u] + kq : klo[u];
    dmine[u] = dM[(int64_t)kk * ldM + oqc];
    rmine[u] = lrel[kk];
  }
  // round 3: the comp rows of those columns (the first column's row where the node has fewer than four)
  float cv[NPW][4];
#pragma unroll
  for (int u = 0; u < NPW; ++u)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      cv[u][t] = comp[(int64_t)__builtin_amdgcn_readlane(rmine[u], 16 * t) * B + b];
  // the pieces cross the wave's tile: written in piece order, read as the 8-byte pairs of row b.  The writes are
  // unconditional at the clamped piece numbers of the loads (lanes past the block's end write the last piece again,
  // the same bytes): behind a guard the compiler sinks the piece's LOAD into the guarded block and waits for it there
  float *tile = s_tile + (size_t)wv * NPW * (4 * nv);
#pragma unroll
  for (int u = 0; u < NPW; ++u)
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int q = (lane + 64 * h < nv) ? lane + 64 * h : nv - 1;
      reinterpret_cast<f32x4s *>(tile + (size_t)u * 4 * nv)[q] = pc[u][h];
    }
  wave_lds_fence();
  float sq = 0.f;
#pragma unroll
  for (int u = 0; u < NPW; ++u) {
    float v[FT];
    const float *row = tile + (size_t)u * 4 * nv + b * F;
#pragma unroll
    for (int o = 0; o < FT; o += 2) {
      if (EXACT || o < F) {
        const f32x2s t = *reinterpret_cast<const f32x2s *>(row + o);
        v[o] = t.x; v[o + 1] = t.y;
      } else {
        v[o] = 0.f; v[o + 1] = 0.f;
      }
    }
    // (a wave past the end of the list works on the repeated last entry and keeps nothing: an early exit here would
    // let the compiler sink the loads above into the guarded block, behind the wait for the tile)
    const bool keep = on && i0 + u < NL;
    float acc[FT];
#pragma unroll
    for (int o = 0; o < FT; ++o) acc[o] = 0.f;
    int32_t rm = rmine[u];
    float dm = dmine[u];
    float c4[4] = {cv[u][0], cv[u][1], cv[u][2], cv[u][3]};
    for (int32_t kb = klo[u];;) {
      const int nc = (khi[u] - kb < 4) ? khi[u] - kb : 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nc) {  // wave uniform
          const float w = c4[t];
          float d[FT];
#pragma unroll
          for (int o = 0; o < FT; ++o)
            d[o] = (o < F) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dm), 16 * t + o))
                           : 0.f;
          float dot = 0.f;
#pragma unroll
          for (int o = 0; o < FT; ++o) dot = fmaf(d[o], v[o], dot);
          if (keep) D[(int64_t)(kb + t) * B + b] = dot;
#pragma unroll
          for (int o = 0; o < FT; ++o) acc[o] = fmaf(w, d[o], acc[o]);
        }
      }
      kb += 4;
      if (kb >= khi[u]) break;  // (few nodes have more than four live columns)
      const int32_t kk = (kb + kq < khi[u]) ? kb + kq : kb;
      dm = dM[(int64_t)kk * ldM + oqc];
      rm = lrel[kk];
#pragma unroll
      for (int t = 0; t < 4; ++t) c4[t] = comp[(int64_t)__builtin_amdgcn_readlane(rm, 16 * t) * B + b];
    }
    if (keep) {
#pragma unroll
      for (int o = 0; o < FT; ++o)
        if (o < F) sq = fmaf(acc[o], acc[o], sq);
    }
  }
  __shared__ float s_sq[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  if (lane == 0) s_sq[wv] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 4; ++i) t += (double)s_sq[i];
    blk_part[blockIdx.x] = t;
  }
}

// One fold block of the one-shot form's squared norm: sq_part[f] = the contiguous slice [f per, (f + 1) per) of the
// per-block parts, thread t adding the slice's elements t, t + 256, ... in rising order, the 256 sums then in thread
// order pairwise by wave 0.  Appended to the k_dcomp_chunks launch as the blocks behind the last chunk.
__device__ __forceinline__ void fold_sq_parts(const double *__restrict__ blk_part, int64_t n_blk, int64_t per, int f,
                                              double *__restrict__ sq_part) {
  __shared__ double s_fold[256];
  const int64_t beg = (int64_t)f * per, end = (beg + per < n_blk) ? beg + per : n_blk;
  double t = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256) t += blk_part[i];
  s_fold[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < 64) {
    double a = (s_fold[threadIdx.x] + s_fold[threadIdx.x + 64]) + (s_fold[threadIdx.x + 128] + s_fold[threadIdx.x + 192]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (threadIdx.x == 0) sq_part[f] = a;
  }
}

// slab[chunk][b] = sum of D[k][b] over the live columns k of one relation-major chunk (<= kRelChunk columns of one
// (node band, relation) group).  A row of D is B floats = P = B / 4 16-byte pieces: lane l takes piece l % P of row
// slot l / P, so one load instruction brings 64 / P rows (six at B = 40) and eight of them are in flight per wave; the
// four waves take a quarter of the chunk each.  The row slots meet in LDS, added in a fixed order.
// Blocks behind the last chunk (the one-shot mix backward appends them) fold its squared-norm parts: fold_sq_parts.
template <int P>
__global__ __launch_bounds__(256) void k_dcomp_chunks(const int32_t *__restrict__ chunk_beg,
                                                      const int32_t *__restrict__ chunk_end,
                                                      const int32_t *__restrict__ lperm, const float *__restrict__ D,
                                                      float *__restrict__ slab, int n_chunks,
                                                      const double *__restrict__ blk_part, int64_t n_blk, int64_t fold_per,
                                                      double *__restrict__ sq_part) {
  constexpr int RPI = 64 / P;  // rows per load instruction
  constexpr int B = 4 * P;
  __shared__ f32x4s s_acc[4][RPI][P];
  if ((int)blockIdx.x >= n_chunks) {  // block uniform
    fold_sq_parts(blk_part, n_blk, fold_per, (int)blockIdx.x - n_chunks, sq_part);
    return;
  }
  const int chunk = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int slot = lane / P, piece = lane - slot * P;
  const bool on = slot < RPI;
  const int32_t beg = chunk_beg[chunk], end = chunk_end[chunk];
  const int32_t per = (end - beg + 3) >> 2;
  const int32_t a0 = beg + wv * per, a1 = (a0 + per < end) ? a0 + per : end;
  const f32x4s *D4 = reinterpret_cast<const f32x4s *>(D);
  constexpr int U = (64 / RPI) < 8 ? (64 / RPI) : 8;  // load instructions per step (U * RPI <= 64 row numbers)
  f32x4s acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int32_t e0 = a0; e0 < a1; e0 += U * RPI) {
    const int32_t mine = (e0 + lane < a1) ? lperm[e0 + lane] : 0;
    f32x4s x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = u * RPI + (on ? slot : 0);
      const int32_t k = __shfl(mine, t, 64);
      x[u] = D4[(int64_t)k * P + piece];  // (row 0 where the chunk has ended: masked below)
    }
#pragma unroll
    for (int u = 0; u < U; u += 2) {
      if (on && e0 + u * RPI + slot < a1) acc0 += x[u];
      if (u + 1 < U && on && e0 + (u + 1) * RPI + slot < a1) acc1 += x[u + 1 < U ? u + 1 : u];
    }
  }
  if (on) s_acc[wv][slot][piece] = acc0 + acc1;
  __syncthreads();
  if (threadIdx.x < (unsigned)B) {
    const int pc = threadIdx.x >> 2, el = threadIdx.x & 3;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int sl = 0; sl < RPI; ++sl) t += s_acc[w][sl][pc][el];
    slab[(int64_t)chunk * B + threadIdx.x] = t;
  }
}

// any B: lane = basis, one row per load instruction
__global__ __launch_bounds__(256) void k_dcomp_chunks_any(const int32_t *__restrict__ chunk_beg,
                                                          const int32_t *__restrict__ chunk_end,
                                                          const int32_t *__restrict__ lperm,
                                                          const float *__restrict__ D, int B,
                                                          float *__restrict__ slab, int n_chunks,
                                                          const double *__restrict__ blk_part, int64_t n_blk,
                                                          int64_t fold_per, double *__restrict__ sq_part) {
  __shared__ float s_part[4][64];
  if ((int)blockIdx.x >= n_chunks) {  // block uniform
    fold_sq_parts(blk_part, n_blk, fold_per, (int)blockIdx.x - n_chunks, sq_part);
    return;
  }
  const int chunk = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t beg = chunk_beg[chunk], end = chunk_end[chunk];
  const int32_t per = (end - beg + 3) >> 2;
  const int32_t a0 = beg + wv * per, a1 = (a0 + per < end) ? a0 + per : end;
  const int bb = lane < B ? lane : 0;
  float acc0 = 0.f, acc1 = 0.f;
  for (int32_t e0 = a0; e0 < a1; e0 += 64) {
    const int32_t mine = (e0 + lane < a1) ? lperm[e0 + lane] : 0;
    const int cnt = (a1 - e0 < 64) ? a1 - e0 : 64;
    for (int t = 0; t < cnt; t += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int tt = (t + u < cnt) ? t + u : cnt - 1;
        const int32_t k = __builtin_amdgcn_readlane(mine, tt);
        x[u] = D[(int64_t)k * B + bb];
      }
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        if (t + u < cnt) acc0 += x[u];
        if (t + u + 1 < cnt) acc1 += x[u + 1];
      }
    }
  }
  s_part[wv][lane] = acc0 + acc1;
  __syncthreads();
  if (threadIdx.x < (unsigned)B)
    slab[(int64_t)chunk * B + threadIdx.x] =
        (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

// dcomp[r][b] = sum of relation r's chunk slabs (wave w adds chunks w, w + 4, ... in order, the four partial sums
// meet in LDS; zeros for a relation without live columns); the block after the last relation adds the per-block parts
// of ||dV||^2
__global__ __launch_bounds__(256) void k_dcomp_final(const int32_t *__restrict__ chunk_ptr,
                                                     const int32_t *__restrict__ chunk_ids,
                                                     const float *__restrict__ slab, int R, int B,
                                                     float *__restrict__ dcomp, const double *__restrict__ sq_part,
                                                     int n_parts, double *__restrict__ sumsq) {
  __shared__ float s_part[4][64];
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (r == R) {
    if (!sumsq || wv != 0) return;
    double t = 0.0;
    for (int i = lane; i < n_parts; i += 64) t += sq_part[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) *sumsq = t;
    return;
  }
  // wave w adds the relation's chunks w, w + 4, w + 8, ... — alternately into s0 and s1, each in rising order.  Sixteen
  // of them per step: their ids with one coalesced load, then sixteen slab rows in flight (a chunk at a time was two
  // dependent round trips each: 21 us for the 1 600 chunks of AM's self-loop relation)
  float s0 = 0.f, s1 = 0.f;
  {
    const int c0 = chunk_ptr[r] + wv, c1 = chunk_ptr[r + 1];
    const int K = c1 > c0 ? (c1 - c0 + 3) / 4 : 0;  // this wave's chunks
    const int bl = lane < B ? lane : B - 1;
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int kk = k0 + (lane & 15);
      const int32_t idv = chunk_ids[c0 + 4 * (kk < K ? kk : K - 1)];
      float x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = slab[(int64_t)__builtin_amdgcn_readlane(idv, u) * B + bl];
#pragma unroll
      for (int u = 0; u < 16; u += 2) {
        if (k0 + u < K) s0 += x[u];
        if (k0 + u + 1 < K) s1 += x[u + 1];
      }
    }
  }
  s_part[wv][lane] = s0 + s1;
  __syncthreads();
  if (threadIdx.x < (unsigned)B)
    dcomp[(int64_t)r * B + threadIdx.x] =
        (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

// ---- dW from per-(row, relation) sums of a constant X (common.hpp: mrgcn_support::Pairs) ----------------------------
// 16 bytes of a 4-byte aligned row (a wide X row is K floats, any K)
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// sum of val_e . X[node_e, kc .. kc + 4) over the entries [b, e) of one piece, in entry order.  Eight rows per step:
// their loads are issued back to back at clamped entry numbers (the node and value of an entry are wave uniform), the
// adds follow in order
__device__ __forceinline__ f32x4s pair_piece_sum(const int32_t *__restrict__ node, const float *__restrict__ val,
                                                 const float *__restrict__ X, int64_t ldX, int kc, int32_t b, int32_t e) {
  f32x4s acc = {0.f, 0.f, 0.f, 0.f};
  for (int32_t i = b; i < e; i += 8) {
    f32x4s x[8];
    float a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int32_t ii = (i + u < e) ? i + u : e - 1;
      a[u] = val[ii];
      x[u] = *reinterpret_cast<const f32x4_a4 *>(X + (int64_t)node[ii] * ldX + kc);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      f32x4s t;
      t.x = fmaf(a[u], x[u].x, acc.x); t.y = fmaf(a[u], x[u].y, acc.y);
      t.z = fmaf(a[u], x[u].z, acc.z); t.w = fmaf(a[u], x[u].w, acc.w);
      acc = (i + u < e) ? t : acc;  // (wave uniform)
    }
  }
  return acc;
}

// S[p, :] of four consecutive pairs per block.  Lane l owns the columns 4 l .. 4 l + 3 of a 256-column slice; the last
// lane of a row loads at K - 4 and keeps the columns that are its own.  A pair of up to kPairPiece entries is one
// wave's; a longer one is cut into pieces of kPairPiece entries that the block's four waves sum four at a time, the
// partial sums meeting in LDS where wave 0 adds them in piece order.  Runs once per X: kept simple.
__global__ __launch_bounds__(256) void k_pair_sums(const int32_t *__restrict__ pair_ptr, const int32_t *__restrict__ node,
                                                   const float *__restrict__ val, int64_t P,
                                                   const float *__restrict__ X, int64_t ldX, int K,
                                                   float *__restrict__ S) {
  __shared__ f32x4s s_part[4][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t p0 = (int64_t)blockIdx.x * 4;
  for (int kb = 0; kb < K; kb += 256) {
    const int kcol = kb + 4 * lane;
    const int kc = kcol < K - 4 ? kcol : K - 4;
    auto store = [&](int64_t p, const f32x4s &v) {
      float *dst = S + p * K;
      if (kcol < K) {
        if (kc + 0 >= kcol) dst[kc + 0] = v.x;
        if (kc + 1 >= kcol) dst[kc + 1] = v.y;
        if (kc + 2 >= kcol) dst[kc + 2] = v.z;
        dst[kc + 3] = v.w;
      }
    };
    if (p0 + wv < P) {
      const int32_t b = pair_ptr[p0 + wv], e = pair_ptr[p0 + wv + 1];
      if (e - b <= kPairPiece) store(p0 + wv, pair_piece_sum(node, val, X, ldX, kc, b, e));
    }
    for (int u = 0; u < 4 && p0 + u < P; ++u) {  // (block uniform)
      const int32_t b = pair_ptr[p0 + u], e = pair_ptr[p0 + u + 1];
      if (e - b <= kPairPiece) continue;
      f32x4s acc = {0.f, 0.f, 0.f, 0.f};
      for (int32_t r0 = b; r0 < e; r0 += 4 * kPairPiece) {
        const int32_t pb = r0 + wv * kPairPiece;
        const int32_t pe = pb + kPairPiece < e ? pb + kPairPiece : e;
        f32x4s part = {0.f, 0.f, 0.f, 0.f};
        if (pb < e) part = pair_piece_sum(node, val, X, ldX, kc, pb, pe);
        s_part[wv][lane] = part;
        __syncthreads();
        if (wv == 0) {
#pragma unroll
          for (int w = 0; w < 4; ++w)
            if (r0 + w * kPairPiece < e) acc += s_part[w][lane];
        }
        __syncthreads();
      }
      if (wv == 0) store(p0 + u, acc);
    }
  }
}

// slab[chunk][k][f] = sum over the chunk's pairs p (rising) of S[p][k] . dY[row_p][f].  Thread k streams column k of
// the chunk's S rows (a row is one coalesced read of the block), eight rows in flight; a pair's dY row is block
// uniform.  FT: F rounded up to whole fours.
template <int FT>
__global__ __launch_bounds__(256) void k_dw_pairs(const int32_t *__restrict__ chunk_beg,
                                                  const int32_t *__restrict__ chunk_end,
                                                  const int32_t *__restrict__ pair_row, const float *__restrict__ S,
                                                  int K, const float *__restrict__ dY, int64_t ldY, int F,
                                                  float *__restrict__ slab) {
  const int32_t p0 = chunk_beg[blockIdx.x], p1 = chunk_end[blockIdx.x];
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    float acc[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[f] = 0.f;
    for (int32_t p = p0; p < p1; p += 8) {
      float sv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) sv[u] = S[(int64_t)((p + u < p1) ? p + u : p1 - 1) * K + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (p + u < p1) {  // (block uniform)
          const float *__restrict__ g = dY + (int64_t)pair_row[p + u] * ldY;
#pragma unroll
          for (int f = 0; f < FT; ++f)
            if (f < F) acc[f] = fmaf(sv[u], g[f], acc[f]);
        }
      }
    }
    float *dst = slab + ((int64_t)blockIdx.x * K + k) * F;
#pragma unroll
    for (int f = 0; f < FT; ++f)
      if (f < F) dst[f] = acc[f];
  }
}

// dW[r][t] = relation r's chunk slabs added in chunk order (in the manner of k_dw_reduce, one writer per element at
// any chunk count: no atomics); zeros for a relation without pairs
__global__ __launch_bounds__(256) void k_dw_pairs_reduce(const int32_t *__restrict__ chunk_ptr,
                                                         const float *__restrict__ slab, int KF,
                                                         float *__restrict__ dW) {
  const int r = blockIdx.x;
  const int t = blockIdx.y * blockDim.x + threadIdx.x;
  if (t >= KF) return;
  const int c0 = chunk_ptr[r], c1 = chunk_ptr[r + 1];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = c0;
  for (; c + 4 <= c1; c += 4) {
    s0 += slab[(int64_t)c * KF + t];
    s1 += slab[(int64_t)(c + 1) * KF + t];
    s2 += slab[(int64_t)(c + 2) * KF + t];
    s3 += slab[(int64_t)(c + 3) * KF + t];
  }
  for (; c < c1; ++c) s0 += slab[(int64_t)c * KF + t];
  dW[(int64_t)r * KF + t] = (s0 + s1) + (s2 + s3);
}

__global__ void k_xent_scatter_rows(const float *__restrict__ drows, const int64_t *__restrict__ idx, int64_t n, int C,
                                    const float *__restrict__ g, float *__restrict__ dlogits, int64_t ldd) {
  const float gg = g ? *g : 1.f;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * C; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / C;
    const int c = (int)(t - i * C);
    dlogits[idx[i] * ldd + c] = gg * drows[t];
  }
}

}  // namespace

int support_dcomp_from_D(const mrgcn_support *q, const float *D, int B, float *slab, const double *sq_part,
                         int64_t n_parts, float *dcomp, double *sumsq, hipStream_t s) {
  const mrgcn_support::Order &o = q->wide;
  const int R = (int)q->plan->num_relations;
  if (o.n_chunks > 0) {
    k_dcomp_chunks_any<<<dim3((unsigned)o.n_chunks), dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, B, slab,
                                                                         o.n_chunks, nullptr, 0, 0, nullptr);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  k_dcomp_final<<<dim3((unsigned)(R + 1)), dim3(256), 0, s>>>(o.chunk_ptr, o.chunk_ids, slab, R, B, dcomp, sq_part,
                                                             (int)n_parts, sumsq);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}
}  // namespace mrgcn

extern "C" {

using namespace mrgcn;

int mrgcn_support_spmm_t_f32(const mrgcn_support_t *q, const float *dY, int64_t ldY, int32_t F, float *dM, int64_t ldM,
                             void *stream) {
  MRGCN_REQUIRE(q && dY && dM, "NULL");
  MRGCN_REQUIRE(F > 0 && ldY >= F && ldM >= F, "F / leading dimensions");
  return spmm_on_view(q->tview(), dY, ldY, F, dM, ldM, q->partials, (hipStream_t)stream);
}

// blocks of the one-shot mix backward: four waves of kStreamNPW list entries each
static inline int64_t stream_blocks(int64_t NL) { return ((NL + kStreamNPW - 1) / kStreamNPW + 3) / 4; }

int64_t mrgcn_support_mix_bwd_workspace(const mrgcn_support_t *q, int32_t B) {
  if (!q || B <= 0) return 0;
  // D [L][B] (16-byte aligned rows when B % 4 == 0) | slab [chunks][B] | parts of ||dV||^2 (kSqParts doubles, 8-byte
  // aligned) | the one-shot form's per-block parts (one double per eight live nodes)
  return ((q->L + q->wide.n_chunks) * (int64_t)B + 3) / 4 * 4 + 2 * (int64_t)kSqParts + 2 * stream_blocks(q->NL);
}

int mrgcn_support_mix_bwd_f32(const mrgcn_support_t *q, const float *dM, int64_t ldM, const float *V,
                              const float *comp, int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp,
                              double *dV_sumsq, float *workspace, int64_t workspace_floats, void *stream) {
  MRGCN_REQUIRE(q && dM && V && comp && dcomp, "NULL");
  MRGCN_REQUIRE(B > 0 && F > 0 && ldM >= F, "B / F / ldM");
  hipStream_t s = (hipStream_t)stream;
  const mrgcn_plan *p = q->plan;
  const int R = (int)p->num_relations;
  const int64_t N = p->num_nodes;
  if (dV) {  // the gradient itself: the wave-over-nodes kernel of rgcn_fused.hip on the support's arrays
    MRGCN_HIP_TRY(mrgcn::fill_async(dcomp, 0, (size_t)R * B * sizeof(float), s));
    int rc = mix_bwd_nm_arrays(q->nlptr, q->lrel, N, R, -1, dM, ldM, V, comp, B, F, dV, dcomp, dV_sumsq, s, nullptr,
                               dense ? nullptr : q->node_scratch);
    if (rc < 0) {
      set_error("mrgcn_support_mix_bwd_f32: shape outside the node-major kernel's limits (F <= 16, B <= 64)");
      return MRGCN_ERR_UNSUPPORTED;
    }
    return rc;
  }
  MRGCN_REQUIRE(F <= 16 && B <= 64, "the norm-only pass needs F <= 16, B <= 64");
  MRGCN_REQUIRE((F & 1) || (((uintptr_t)V) & 7) == 0, "V must be 8-byte aligned");
  MRGCN_REQUIRE(workspace && workspace_floats >= mrgcn_support_mix_bwd_workspace(q, B) && (((uintptr_t)workspace) & 7) == 0,
                "workspace (mrgcn_support_mix_bwd_workspace floats, 8-byte aligned)");
  const mrgcn_support::Order &o = q->wide;
  float *D = workspace;
  float *slab = D + q->L * (int64_t)B;
  double *sq_part = reinterpret_cast<double *>(workspace + ((q->L + o.n_chunks) * (int64_t)B + 3) / 4 * 4);
  double *blk_part = sq_part + kSqParts;
  const bool dvec = (B % 4 == 0) && (((uintptr_t)D) % 16 == 0);
  // the D rows by relation, with `n_fold` blocks appended that fold the one-shot form's per-block parts
  auto dcomp_chunks = [&](int64_t n_fold, int64_t n_blk, int64_t fold_per) {
    const dim3 cg((unsigned)(o.n_chunks + n_fold));
    if (dvec && B == 40)
      k_dcomp_chunks<10><<<cg, dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, slab, o.n_chunks, blk_part, n_blk, fold_per, sq_part);
    else if (dvec && B == 32)
      k_dcomp_chunks<8><<<cg, dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, slab, o.n_chunks, blk_part, n_blk, fold_per, sq_part);
    else if (dvec && B == 16)
      k_dcomp_chunks<4><<<cg, dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, slab, o.n_chunks, blk_part, n_blk, fold_per, sq_part);
    else if (dvec && B == 8)
      k_dcomp_chunks<2><<<cg, dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, slab, o.n_chunks, blk_part, n_blk, fold_per, sq_part);
    else
      k_dcomp_chunks_any<<<cg, dim3(256), 0, s>>>(o.chunk_beg, o.chunk_end, o.lperm, D, B, slab, o.n_chunks, blk_part, n_blk, fold_per, sq_part);
  };
  // the one-shot form (k_mix_bwd_stream) wherever it applies, at every NL
  const int one_shot = (int)cfg(CFG_SUP_MIX_STREAM);
  if (one_shot > 0 && (B * F) % 4 == 0 && B * F <= 1024 && (F & 1) == 0 && (((uintptr_t)V) & 15) == 0) {
    const int nv = (B * F) / 4;
    const int nh = nv <= 64 ? 1 : nv <= 128 ? 2 : 4;
    const int64_t n_blk = q->NL > 0 ? stream_blocks(q->NL) : 0;
    // at least 256 parts per fold block, at most kSqParts fold blocks
    const int64_t fold_per = std::max<int64_t>(256, (n_blk + kSqParts - 1) / kSqParts);
    const int64_t n_fold = (n_blk + fold_per - 1) / fold_per;
    const size_t tile = (size_t)4 * kStreamNPW * B * F * sizeof(float);
#define STREAM_GO2(T, NH_, EX_)                                                                                     \
  k_mix_bwd_stream<T, NH_, kStreamNPW, EX_><<<dim3((unsigned)n_blk), dim3(256), tile, s>>>(                       \
      q->lnode, q->lnptr, q->lrel, dM, ldM, V, comp, q->NL, B, F, D, blk_part)
#define STREAM_GO(T, EX_)                     \
  do {                                        \
    if (nh == 1) STREAM_GO2(T, 1, EX_);       \
    else if (nh == 2) STREAM_GO2(T, 2, EX_);  \
    else STREAM_GO2(T, 4, EX_);               \
  } while (0)
    if (n_blk > 0) {
      switch (F) {
        case 4: STREAM_GO(4, true); break;
        case 8: STREAM_GO(8, true); break;
        case 10: STREAM_GO(10, true); break;
        case 12: STREAM_GO(12, true); break;
        case 16: STREAM_GO(16, true); break;
        default: STREAM_GO(16, false); break;
      }
      MRGCN_HIP_TRY(hipGetLastError());
    }
#undef STREAM_GO
#undef STREAM_GO2
    if (o.n_chunks + n_fold > 0) {
      dcomp_chunks(n_fold, n_blk, fold_per);
      MRGCN_HIP_TRY(hipGetLastError());
    }
    k_dcomp_final<<<dim3((unsigned)(R + 1)), dim3(256), 0, s>>>(o.chunk_ptr, o.chunk_ids, slab, R, B, dcomp, sq_part,
                                                               (int)n_fold, dV_sumsq);
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  // The resident form (k_mix_bwd_sup).  The timings below describe IT, not the one-shot form above:
  // nodes in flight per wave (NB) x waves per CU.  512-thread blocks with two nodes per step (62 VGPRs at F = 10: three
  // blocks of eight waves per CU, bounded by the 42 KB of comp in LDS)
  // AM shape, kernel alone on one box: 512x1 598 us, 512x2 512, 512x4 557, 1024x2 501
  // (a small support: a wave's 64 list entries are one serial chain of 64 / NB steps — 122 us at MUTAG's 23 k nodes with
  // two per step; four per step halve the chain where occupancy does not matter)
  const size_t lds = (size_t)R * B * sizeof(float);
  MRGCN_REQUIRE(lds <= 64 * 1024, "R * B * 4 must fit 64 KB of LDS");
  const int nb = q->NL < 262144 ? 4 : 2;
  constexpr int nw = kSupTB / 64;
  int epw = 64;
  if (q->NL < 262144) {  // ~4096 waves' worth of entries each, a multiple of the step
    epw = (int)((q->NL / 4096 + nb - 1) / nb * nb);
    epw = std::min(64, std::max(epw, nb));
  }
  int64_t grid = (q->NL + (int64_t)epw * nw - 1) / ((int64_t)epw * nw);
  int per_cu = (int)std::min<size_t>(4, (160 * 1024) / (lds + 1024));
  if (per_cu < 1) per_cu = 1;
  // a resident grid striding through the list
  if (grid > 256 * per_cu) grid = 256 * per_cu;
  if (grid > kSqParts) grid = kSqParts;
  if (grid < 1) grid = 1;
  const int FT = (F == 10 || F == 11) ? F : (F + 3) / 4 * 4;
#define SUP_GO2(T, NB_, EX_)                                                                                      \
  do {                                                                                                            \
    auto kfn = k_mix_bwd_sup<T, NB_, EX_>;                                                                        \
    MRGCN_HIP_TRY(mrgcn::raise_lds_limit((const void *)kfn, lds));                                                \
    kfn<<<dim3((unsigned)grid), dim3(kSupTB), lds, s>>>(q->lnode, q->lnptr, q->lrel, dM, ldM, V, comp, q->NL,  \
                                                           R, B, F, D, sq_part, epw);                             \
  } while (0)
#define SUP_GO(T)                        \
  do {                                   \
    if (F != T) SUP_GO2(T, 1, false);    \
    else if (nb == 4) SUP_GO2(T, 4, true); \
    else SUP_GO2(T, 2, true);            \
  } while (0)
  if (q->NL > 0) {
    switch (FT) {
      case 4: SUP_GO(4); break;
      case 8: SUP_GO(8); break;
      case 10: SUP_GO(10); break;
      case 11: SUP_GO(11); break;
      case 12: SUP_GO(12); break;
      default: SUP_GO(16); break;
    }
  }
#undef SUP_GO
#undef SUP_GO2
  MRGCN_HIP_TRY(hipGetLastError());
  if (o.n_chunks > 0) {
    dcomp_chunks(0, 0, 0);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  k_dcomp_final<<<dim3((unsigned)(R + 1)), dim3(256), 0, s>>>(o.chunk_ptr, o.chunk_ids, slab, R, B, dcomp, sq_part,
                                                             q->NL > 0 ? (int)grid : 0, dV_sumsq);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_support_adam_rows_fused_f32(const mrgcn_support_t *q, const float *dM, int64_t ldM, const float *comp,
                                      int32_t B, int32_t F, float *param, float *exp_avg, float *exp_avg_sq,
                                      uint8_t *row_ever, float lr, float beta1, float beta2, float eps, int64_t step,
                                      const float *bc_dev, const float *grad_scale, int32_t ever_outside,
                                      void *stream) {
  MRGCN_REQUIRE(q && dM && comp && param && exp_avg && exp_avg_sq && row_ever, "NULL");
  MRGCN_REQUIRE(mrgcn_adam_rows_fused_supported(q->plan, B, F), "shape outside mrgcn_adam_rows_fused_supported");
  MRGCN_REQUIRE(ldM >= F, "ldM");
  MRGCN_REQUIRE(((((uintptr_t)param) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) == 0,
                "param / moments must be 16-byte aligned");
  MRGCN_REQUIRE(bc_dev || step >= 1, "step");
  const mrgcn_plan *p = q->plan;
  return adam_rows_fused_arrays(q->nlptr, q->lrel, nullptr, p->num_nodes, (int)p->num_relations, dM, ldM, comp, B, F,
                                param, exp_avg, exp_avg_sq, q->node_flags, row_ever, lr, beta1, beta2, eps, step,
                                bc_dev, grad_scale, (hipStream_t)stream, q->lnode, q->lnptr, q->NL, ever_outside);
}

int64_t mrgcn_support_rel_transform_bwd_workspace(const mrgcn_support_t *q, int32_t K, int32_t F, int32_t need_dX,
                                                  int32_t need_dW) {
  if (!q) return -1;
  if (!xform_use_mfma()) return -1;
  if (need_dW && !xform_mfma_dw_supported(K, F)) return -1;
  if (need_dX && !(xform_mfma_dx_supported(F, K))) return -1;
  const int64_t a = need_dX ? q->L * (((int64_t)K + 3) / 4 * 4) : 0;
  const int64_t b = need_dW ? (int64_t)q->order_for(K).n_relchunks * K * F : 0;
  const int64_t m = a > b ? a : b;
  return m > 0 ? m : 1;
}

static int support_rel_transform_bwd(const mrgcn_support_t *q, const float *dM, int64_t ldM, const void *X_, bool x_bf16,
                                     int64_t ldX, int32_t K, const float *W, int32_t F, float *dX, int64_t lddX,
                                     float *dW, float *workspace, int64_t workspace_floats,
                                     int32_t relu_mask_from_x, void *stream) {
  const float *X = (const float *)X_;
  MRGCN_REQUIRE(q && dM && X && W, "NULL");
  MRGCN_REQUIRE(!(x_bf16 && relu_mask_from_x), "the ReLU mask is read from fp32 rows");
  MRGCN_REQUIRE(K > 0 && F > 0 && ldX >= K && ldM >= F, "K / F / leading dimensions");
  const int64_t need = mrgcn_support_rel_transform_bwd_workspace(q, K, F, dX != nullptr, dW != nullptr);
  if (need < 0) {
    set_error("mrgcn_support_rel_transform_bwd_f32: shape outside the matrix-core transforms' limits");
    return MRGCN_ERR_UNSUPPORTED;
  }
  MRGCN_REQUIRE(workspace && workspace_floats >= need, "workspace (mrgcn_support_rel_transform_bwd_workspace floats)");
  MRGCN_REQUIRE(!relu_mask_from_x || (dX && K <= 16), "the masked dX needs K <= 16");
  hipStream_t s = (hipStream_t)stream;
  const mrgcn_plan *p = q->plan;
  if (dW) {
    const RelOrder o = q->order_for(K);
    int rc = xform_mfma_dw(p, o, o.rnode, X_, ldX, K, dM, ldM, F, dW, workspace, workspace_floats, s, nullptr, x_bf16);
    if (rc != MRGCN_OK) return rc;
  }
  if (dX) {
    MRGCN_REQUIRE(lddX >= K, "lddX");
    const int64_t ldZ = ((int64_t)K + 3) / 4 * 4;
    // Z[k, 0:K] = dM[k, 0:F] . W[r_k]^T on the matrix cores, then dX[j] = sum of node j's Z rows (every row written)
    int rc = xform_mfma_fwd(p, q->order_for(F), nullptr, nullptr, dM, ldM, F, W, true, K, workspace, ldZ, s, false,
                            nullptr);
    if (rc != MRGCN_OK) return rc;
    // (a node of up to 8 live columns is summed by its own lane: the wave-cooperative walk takes the live nodes of a
    // wave one after the other — 41 us at the AM shape and at AIFB's 8 k nodes alike)
    rc = segment_sum_arrays(q->nlptr, p->num_nodes, q->L, workspace, ldZ, K, dX, lddX, s,
                            relu_mask_from_x ? X : nullptr, ldX, 8);
    if (rc != MRGCN_OK) return rc;
  }
  return MRGCN_OK;
}

int mrgcn_support_rel_transform_bwd_f32(const mrgcn_support_t *q, const float *dM, int64_t ldM, const float *X,
                                        int64_t ldX, int32_t K, const float *W, int32_t F, float *dX, int64_t lddX,
                                        float *dW, float *workspace, int64_t workspace_floats,
                                        int32_t relu_mask_from_x, void *stream) {
  return support_rel_transform_bwd(q, dM, ldM, X, false, ldX, K, W, F, dX, lddX, dW, workspace, workspace_floats,
                                   relu_mask_from_x, stream);
}

// the same with the layer's input in bf16 rows (the bf16 pipeline's X: ldX in elements); dW's sums stay fp32
int mrgcn_support_rel_transform_bwd_xbf16(const mrgcn_support_t *q, const float *dM, int64_t ldM, const uint16_t *X,
                                          int64_t ldX, int32_t K, const float *W, int32_t F, float *dX, int64_t lddX,
                                          float *dW, float *workspace, int64_t workspace_floats, void *stream) {
  return support_rel_transform_bwd(q, dM, ldM, X, true, ldX, K, W, F, dX, lddX, dW, workspace, workspace_floats, 0,
                                   stream);
}

int mrgcn_support_pair_sums_info(const mrgcn_support_t *q, int32_t K, mrgcn_pair_sums_info_t *h, void *stream) {
  MRGCN_REQUIRE(q && h, "NULL");
  MRGCN_REQUIRE(K >= 0, "K");
  int rc = support_pairs(q, (hipStream_t)stream);
  if (rc != MRGCN_OK) return rc;
  const mrgcn_support::Pairs &pr = q->pairs;
  h->pairs = pr.built ? pr.P : -1;
  h->table_bytes = pr.built ? pr.P * (int64_t)K * (int64_t)sizeof(float) : 0;
  h->chunks = pr.n_chunks;
  h->chunk_pairs = kPairChunk;
  h->piece_entries = kPairPiece;
  h->max_pair_entries = pr.max_pair_entries;
  h->device_bytes = pr.device_bytes;
  return MRGCN_OK;
}

int mrgcn_support_pair_sums_build_f32(const mrgcn_support_t *q, const float *X, int64_t ldX, int32_t K, float *S,
                                      void *stream) {
  MRGCN_REQUIRE(q && X && S, "NULL");
  MRGCN_REQUIRE(K >= 4 && ldX >= K, "K >= 4 / ldX");
  MRGCN_REQUIRE((((uintptr_t)X) & 3) == 0, "X must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int rc = support_pairs(q, s);
  if (rc != MRGCN_OK) return rc;
  const mrgcn_support::Pairs &pr = q->pairs;
  MRGCN_REQUIRE(pr.built, "the pair structure is built outside a stream capture (mrgcn_support_pair_sums_info)");
  if (pr.P == 0) return MRGCN_OK;
  k_pair_sums<<<dim3((unsigned)((pr.P + 3) / 4)), dim3(256), 0, s>>>(pr.pair_ptr, pr.node, pr.val, pr.P, X, ldX, K, S);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_support_dw_pairs_workspace(const mrgcn_support_t *q, int32_t K, int32_t F) {
  if (!q || !q->pairs.built || K <= 0 || F <= 0 || F > 16) return -1;
  const int64_t n = (int64_t)q->pairs.n_chunks * K * F;
  return n > 0 ? n : 1;
}

int mrgcn_support_dw_pairs_f32(const mrgcn_support_t *q, const float *S, int32_t K, const float *dY, int64_t ldY,
                               int32_t F, float *dW, float *workspace, int64_t workspace_floats, void *stream) {
  MRGCN_REQUIRE(q && dY && dW, "NULL");
  MRGCN_REQUIRE(K > 0 && F > 0 && F <= 16 && ldY >= F, "K / F <= 16 / ldY");
  const mrgcn_support::Pairs &pr = q->pairs;
  MRGCN_REQUIRE(pr.built, "the pair structure is built outside a stream capture (mrgcn_support_pair_sums_info)");
  MRGCN_REQUIRE(pr.P == 0 || S, "NULL");
  MRGCN_REQUIRE(workspace && workspace_floats >= mrgcn_support_dw_pairs_workspace(q, K, F),
                "workspace (mrgcn_support_dw_pairs_workspace floats)");
  hipStream_t s = (hipStream_t)stream;
  const int R = (int)q->plan->num_relations;
  if (pr.n_chunks > 0) {
    const dim3 grid((unsigned)pr.n_chunks), block((unsigned)(((K < 256 ? K : 256) + 63) / 64 * 64));
    switch ((F + 3) / 4) {
      case 1: k_dw_pairs<4><<<grid, block, 0, s>>>(pr.chunk_beg, pr.chunk_end, pr.pair_row, S, K, dY, ldY, F, workspace); break;
      case 2: k_dw_pairs<8><<<grid, block, 0, s>>>(pr.chunk_beg, pr.chunk_end, pr.pair_row, S, K, dY, ldY, F, workspace); break;
      case 3: k_dw_pairs<12><<<grid, block, 0, s>>>(pr.chunk_beg, pr.chunk_end, pr.pair_row, S, K, dY, ldY, F, workspace); break;
      default: k_dw_pairs<16><<<grid, block, 0, s>>>(pr.chunk_beg, pr.chunk_end, pr.pair_row, S, K, dY, ldY, F, workspace); break;
    }
    MRGCN_HIP_TRY(hipGetLastError());
  }
  if (R > 0) {
    k_dw_pairs_reduce<<<dim3((unsigned)R, (unsigned)((K * F + 255) / 256)), dim3(256), 0, s>>>(pr.chunk_ptr, workspace,
                                                                                              K * F, dW);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  return MRGCN_OK;
}

int mrgcn_softmax_xent_bwd_rows_f32(const float *drows, const int64_t *idx, int64_t n, int32_t C, const float *g,
                                    float *dlogits, int64_t ldd, void *stream) {
  MRGCN_REQUIRE(drows && idx && dlogits, "NULL");
  MRGCN_REQUIRE(C > 0 && ldd >= C && n > 0, "C / ldd / n");
  int grid = (int)((n * C + 255) / 256);
  if (grid > 1024) grid = 1024;
  k_xent_scatter_rows<<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>(drows, idx, n, C, g, dlogits, ldd);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
