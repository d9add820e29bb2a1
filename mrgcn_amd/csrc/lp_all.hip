// The 1-vs-all softmax decoder: every query vector Q[q] (a fact's subject-relation or relation-object pair vector,
// built by the caller: this unit does not know the scorer) is scored against ALL rows of the candidate table E under a
// softmax cross-entropy,
//     x[q][c] = Q[q] . E[c]      loss = (1/m) sum_q (log sum_c exp x[q][c] - x[q][target[q]])
// — the objective DistMult and ComplEx are normally trained with (Kadlec, Bajgar, Kleindienst: "Knowledge Base
// Completion: Baselines Strike Back", 2017; Lacroix, Usunier, Obozinski: "Canonical Tensor Decomposition for Knowledge
// Base Completion", ICML 2018; Ruffinelli, Broscheit, Gemulla: "You CAN Teach an Old Dog New Tricks!", ICLR 2020).  The
// reference has the sampled BCE only (mrgcn/tasks/link_prediction.py:645-665, :550-554), so the papers stand where a
// reference call site would.  The [m, N] score matrix is never stored: all three kernels compute 64 x 64 score tiles
// on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32; lane maps as basis_xform.hip's k_bx_gemm) and consume them
// in registers.
//   tile      the ROW side (64 rows, 16 per wave) sits in registers as the A operand for the whole kernel, the STREAM
//             side passes through LDS 64 rows at a time as the B operand; the next tile's rows are loaded into
//             registers while the present one is multiplied.  Every load is straight-line at a clamped position;
//             what a padded row or column holds is masked out of every sum.
//   forward   rows = queries, stream = candidates.  A wave keeps (max, sum) of its 16 queries: per tile the new max is
//             decided first, the tile is exponentiated against it, the running sum is scaled once.  x[q][target[q]]
//             is taken from the same tile.  With few query tiles the candidates are cut into fixed chunks over
//             gridDim.y; the chunk pairs are merged in chunk order, lse written (as a float and the remainder the
//             float leaves of the float64 value), and lse - xt summed in float64 in a fixed order and rounded once.
//   backward  G[q][c] = (exp(x[q][c] - lse[q]) - [c == target[q]]) gl / m, recomputed tile by tile.
//             dQ = G . E: rows = queries, stream = candidates; dE = G^T . Q: rows = candidates, stream = queries.  A
//             wave's 16 x 64 piece of G goes through its own LDS rows to become the A operand of the second product,
//             whose B operand is the stream tile that is in LDS already.  A block stores its own rows: every output
//             row has one owner, nothing is added.
// No float atomics anywhere: the same bits on every run, with or without torch.use_deterministic_algorithms.
#include "lp_tile.hpp"

namespace mrgcn {
namespace {

// forward: block (x, y) = query tile x, candidate chunk y -> pairs[y][q] = (max, sum of exp(x - max)) over the chunk,
// xt[q] from the block whose chunk holds target[q]
template <int NT>
__global__ __launch_bounds__(256) void k_lp_all_fwd(const float *__restrict__ Q, int64_t ldQ, int64_t m,
                                                    const float *__restrict__ E, int64_t ldE, int64_t N, int H,
                                                    const int64_t *__restrict__ target, int64_t chunk,
                                                    float *__restrict__ pairs, float *__restrict__ xt) {
  extern __shared__ __align__(16) float lp_all_lds[];
  float *Es = lp_all_lds;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = (H + 15) / 16 * 4, lds = 4 * hq + 4;
  const int64_t q0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t cbeg = (int64_t)blockIdx.y * chunk, cend = cbeg + chunk < N ? cbeg + chunk : N;
  const int64_t ntiles = (cend - cbeg + kAT - 1) / kAT;
  f32x4a a[4 * NT], nxt[4 * NT];
  load_rows<NT>(Q, ldQ, q0, m, H, lm, kq, a);
  load_tile<NT>(E, ldE, cbeg, N, H, hq, nxt);
  int64_t tg[4];
  float mx[4], sm[4], xv[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t q = q0 + 4 * kq + reg;
    tg[reg] = target[q < m ? q : m - 1];
    mx[reg] = -INFINITY;
    sm[reg] = 0.f;
    xv[reg] = 0.f;
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t c0 = cbeg + t * kAT;
    store_tile<NT>(Es, lds, hq, nxt);
    __syncthreads();
    load_tile<NT>(E, ldE, t + 1 < ntiles ? c0 + kAT : c0, N, H, hq, nxt);  // (the last tile once more: no branch)
    f32x4a acc[4];
    score_tile<NT>(a, Es, lds, H, lm, kq, acc);
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float x[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + 16 * j + lm;
        x[j] = c < cend ? acc[j][reg] : -INFINITY;
        tmax = fmaxf(tmax, x[j]);
        if (c < cend && c == tg[reg]) xv[reg] = acc[j][reg];
      }
      // the new max first, then the tile against it, then the running sum scaled once (a tile has a live column,
      // so the new max is finite and exp(-inf - max) = 0 covers both the first tile and the padded columns)
      const float mn = fmaxf(mx[reg], row_max(tmax));
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) p += expf(x[j] - mn);
      sm[reg] = sm[reg] * expf(mx[reg] - mn) + row_sum(p);
      mx[reg] = mn;
    }
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float v = row_sum(xv[reg]);  // one lane of the row holds it, the others 0
    const int64_t q = q0 + 4 * kq + reg;
    if (lm == 0 && q < m) {
      float *p = pairs + ((int64_t)blockIdx.y * m + q) * 2;
      p[0] = mx[reg];
      p[1] = sm[reg];
      if (tg[reg] >= cbeg && tg[reg] < cend) xt[q] = v;
    }
  }
}

// lse[q] (and its remainder lse[m + q]) from the chunk pairs in chunk order; part[block] = sum of the block's
// lse - xt, float64 in a fixed tree
__global__ __launch_bounds__(kMergeTB) void k_lp_all_merge(const float *__restrict__ pairs, int64_t nchunks, int64_t m,
                                                           const float *__restrict__ xt, float *__restrict__ lse,
                                                           double *__restrict__ part) {
  __shared__ double red[kMergeTB];
  const int64_t q = (int64_t)blockIdx.x * kMergeTB + threadIdx.x;
  double d = 0.0;
  if (q < m) {
    float M = -INFINITY;
    for (int64_t k = 0; k < nchunks; ++k) M = fmaxf(M, pairs[(k * m + q) * 2]);
    double S = 0.0;
    for (int64_t k = 0; k < nchunks; ++k)
      S += (double)pairs[(k * m + q) * 2 + 1] * (double)expf(pairs[(k * m + q) * 2] - M);
    // lse as a float and what the float leaves of it: the backward subtracts both, so that exp(x - lse) does not
    // carry half an ulp of lse (7.6e-6 relative at lse = 200)
    const double l = (double)M + log(S);
    const float hi = (float)l;
    lse[q] = hi;
    lse[m + q] = (float)(l - (double)hi);
    d = l - (double)xt[q];
  }
  red[threadIdx.x] = d;
  __syncthreads();
  for (int off = kMergeTB / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// *loss = (float)(sum of the parts / m): thread t adds parts t, t + 256, ... in order, then the same tree
__global__ __launch_bounds__(kMergeTB) void k_lp_all_loss(const double *__restrict__ part, int64_t nparts, int64_t m,
                                                          float *__restrict__ loss) {
  __shared__ double red[kMergeTB];
  double d = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += kMergeTB) d += part[i];
  red[threadIdx.x] = d;
  __syncthreads();
  for (int off = kMergeTB / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] / (double)m);
}

// backward.  TRANS = false: dQ — rows R = Q [nR = m], stream S = E [nS = N]; TRANS = true: dE — rows R = E [nR = N],
// stream S = Q [nS = m].  out[r][:] = sum over stream rows s of G(r, s) S[s][:], G the softmax gradient of the pair.
template <int NT, bool TRANS>
__global__ __launch_bounds__(256) void k_lp_all_bwd(const float *__restrict__ R, int64_t ldR, int64_t nR,
                                                    const float *__restrict__ S, int64_t ldS, int64_t nS, int H,
                                                    const int64_t *__restrict__ target, const float *__restrict__ lse,
                                                    const float *__restrict__ gl, int64_t m, float *__restrict__ out,
                                                    int64_t ldo) {
  extern __shared__ __align__(16) float lp_all_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = (H + 15) / 16 * 4, lds = 4 * hq + 4;
  float *Ss = lp_all_lds;
  float *Gs = lp_all_lds + kAT * lds + 16 * wv * kAGP;  // the wave's own 16 rows of the G tile
  const int64_t r0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t ntiles = (nS + kAT - 1) / kAT;
  const float sc = gl[0] / (float)m;
  f32x4a a[4 * NT], nxt[4 * NT], acc2[4 * NT];
  load_rows<NT>(R, ldR, r0, nR, H, lm, kq, a);
  load_tile<NT>(S, ldS, 0, nS, H, hq, nxt);
#pragma unroll
  for (int nt = 0; nt < 4 * NT; ++nt) acc2[nt] = f32x4a{0.f, 0.f, 0.f, 0.f};
  // what belongs to a ROW of the pair tile (TRANS: to a column, read per tile)
  int64_t tgr[4];
  float lser[4], lorr[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t r = r0 + 4 * kq + reg;
    tgr[reg] = TRANS ? r : target[r < nR ? r : nR - 1];
    lser[reg] = TRANS ? 0.f : lse[r < nR ? r : nR - 1];
    lorr[reg] = TRANS ? 0.f : lse[m + (r < nR ? r : nR - 1)];
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t s0 = t * kAT;
    store_tile<NT>(Ss, lds, hq, nxt);
    __syncthreads();
    load_tile<NT>(S, ldS, t + 1 < ntiles ? s0 + kAT : s0, nS, H, hq, nxt);
    int64_t tgc[4];
    float lsec[4], lorc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t s = s0 + 16 * j + lm;
      tgc[j] = TRANS ? target[s < nS ? s : nS - 1] : s;
      lsec[j] = TRANS ? lse[s < nS ? s : nS - 1] : 0.f;
      lorc[j] = TRANS ? lse[m + (s < nS ? s : nS - 1)] : 0.f;
    }
    f32x4a acc[4];
    score_tile<NT>(a, Ss, lds, H, lm, kq, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = s0 + 16 * j + lm < nS;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float d = (acc[j][reg] - (TRANS ? lsec[j] : lser[reg])) - (TRANS ? lorc[j] : lorr[reg]);
        float e = expf(d);
        if (tgr[reg] == tgc[j]) e = expm1f(d);  // the target's p - 1 without the cancellation (one lane of a row)
        Gs[(4 * kq + reg) * kAGP + 16 * j + lm] = live ? e * sc : 0.f;
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f32x4a g = *reinterpret_cast<const f32x4a *>(Gs + lm * kAGP + 16 * kk + 4 * kq);
      const float *b = Ss + (16 * kk + 4 * kq) * lds + lm;  // k slot kq of the s-th MFMA: stream row 16 kk + 4 kq + s
#pragma unroll
      for (int nt = 0; nt < 4 * NT; ++nt)
        if (16 * nt < H) acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g.x, b[16 * nt], acc2[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < 4 * NT; ++nt)
        if (16 * nt < H) acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g.y, b[lds + 16 * nt], acc2[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < 4 * NT; ++nt)
        if (16 * nt < H) acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g.z, b[2 * lds + 16 * nt], acc2[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < 4 * NT; ++nt)
        if (16 * nt < H) acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g.w, b[3 * lds + 16 * nt], acc2[nt], 0, 0, 0);
    }
    wave_lds_fence();
    __syncthreads();
  }
  // D: lane (lm, kq) holds rows 4 kq + reg, column 16 nt + lm
#pragma unroll
  for (int nt = 0; nt < 4 * NT; ++nt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t r = r0 + 4 * kq + reg;
      const int n = 16 * nt + lm;
      if (r < nR && n < H) out[r * ldo + n] = acc2[nt][reg];
    }
}

template <int NT>
int launch_fwd(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int H,
               const int64_t *target, float *pairs, float *xt, hipStream_t s) {
  const size_t lds = stream_lds(H);
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_lp_all_fwd<NT>, lds));
  const dim3 grid((unsigned)((m + kAT - 1) / kAT), (unsigned)chunks_of(m, N));
  k_lp_all_fwd<NT><<<grid, dim3(256), lds, s>>>(Q, ldQ, m, E, ldE, N, H, target, chunk_of(m, N), pairs, xt);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

template <int NT, bool TRANS>
int launch_bwd(const float *R, int64_t ldR, int64_t nR, const float *S, int64_t ldS, int64_t nS, int H,
               const int64_t *target, const float *lse, const float *gl, int64_t m, float *out, int64_t ldo,
               hipStream_t s) {
  const size_t lds = stream_lds(H) + (size_t)kAT * kAGP * sizeof(float);
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_lp_all_bwd<NT, TRANS>, lds));
  const dim3 grid((unsigned)((nR + kAT - 1) / kAT));
  k_lp_all_bwd<NT, TRANS><<<grid, dim3(256), lds, s>>>(R, ldR, nR, S, ldS, nS, H, target, lse, gl, m, out, ldo);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

// ---- the bf16 forms (lp_tile.hpp: the bf16 tile) ---------------------------------------------------------------------
// The same three kernels on bf16 TABLES of Q and E (mrgcn_cast_rows_bf16, once per forward): x[q][c] = Q~[q] . E~[c]
// with fp32 sums on v_mfma_f32_16x16x32_bf16; everything after the scores — the online (max, sum), the target's score,
// the exponentials of the gradient tile, expm1f at the target — is the f32 kernels' code, in fp32.  G is rounded to
// bf16 once, as it is stored for the second product, dQ = G~ . E~ and dE = G~^T . Q~ with fp32 sums and fp32 outputs: the
// gradient of the loss as computed, the operands' rounding passed straight through.  The second product's stream
// operand is read from the score product's own LDS image by the transposed read (second_product_bf16).
template <int NK>
__global__ __launch_bounds__(256) void k_lp_all_fwd_bf16(const uint16_t *__restrict__ Q, int64_t ldQ, int64_t m,
                                                         const uint16_t *__restrict__ E, int64_t ldE, int64_t N, int H,
                                                         const int64_t *__restrict__ target, int64_t chunk,
                                                         float *__restrict__ pairs, float *__restrict__ xt) {
  extern __shared__ __align__(16) uint16_t lp_all_lds16[];
  uint16_t *Es = lp_all_lds16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = hp32(H) / 8;
  const int64_t q0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t cbeg = (int64_t)blockIdx.y * chunk, cend = cbeg + chunk < N ? cbeg + chunk : N;
  const int64_t ntiles = (cend - cbeg + kAT - 1) / kAT;
  bf16x8a a[NK], nxt[NK];
  load_rows_bf16<NK>(Q, ldQ, q0, m, H, lm, kq, a);
  load_tile_bf16<NK>(E, ldE, cbeg, N, H, hq, nxt);
  int64_t tg[4];
  float mx[4], sm[4], xv[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t q = q0 + 4 * kq + reg;
    tg[reg] = target[q < m ? q : m - 1];
    mx[reg] = -INFINITY;
    sm[reg] = 0.f;
    xv[reg] = 0.f;
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t c0 = cbeg + t * kAT;
    store_tile_bf16<NK>(Es, H, hq, nxt);
    __syncthreads();
    load_tile_bf16<NK>(E, ldE, t + 1 < ntiles ? c0 + kAT : c0, N, H, hq, nxt);  // (the last tile once more: no branch)
    f32x4a acc[4];
    score_tile_bf16<NK>(a, Es, H, lm, kq, acc);
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float x[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + 16 * j + lm;
        x[j] = c < cend ? acc[j][reg] : -INFINITY;
        tmax = fmaxf(tmax, x[j]);
        if (c < cend && c == tg[reg]) xv[reg] = acc[j][reg];
      }
      const float mn = fmaxf(mx[reg], row_max(tmax));  // (k_lp_all_fwd's order: max, tile, one scaling of the sum)
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) p += expf(x[j] - mn);
      sm[reg] = sm[reg] * expf(mx[reg] - mn) + row_sum(p);
      mx[reg] = mn;
    }
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float v = row_sum(xv[reg]);  // one lane of the row holds it, the others 0
    const int64_t q = q0 + 4 * kq + reg;
    if (lm == 0 && q < m) {
      float *p = pairs + ((int64_t)blockIdx.y * m + q) * 2;
      p[0] = mx[reg];
      p[1] = sm[reg];
      if (tg[reg] >= cbeg && tg[reg] < cend) xt[q] = v;
    }
  }
}

// TRANS as k_lp_all_bwd: false = dQ (rows Q, stream E), true = dE (rows E, stream Q); out is fp32
template <int NK, bool TRANS>
__global__ __launch_bounds__(256) void k_lp_all_bwd_bf16(const uint16_t *__restrict__ R, int64_t ldR, int64_t nR,
                                                         const uint16_t *__restrict__ S, int64_t ldS, int64_t nS, int H,
                                                         const int64_t *__restrict__ target,
                                                         const float *__restrict__ lse, const float *__restrict__ gl,
                                                         int64_t m, float *__restrict__ out, int64_t ldo) {
  extern __shared__ __align__(16) uint16_t lp_all_lds16[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = hp32(H) / 8;
  uint16_t *Ss = lp_all_lds16;
  uint16_t *Gs = lp_all_lds16 + kAT * tile_ld<NK>() + 16 * wv * kBGP;  // the wave's own 16 rows of the G tile
  const int64_t r0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t ntiles = (nS + kAT - 1) / kAT;
  const float sc = gl[0] / (float)m;
  bf16x8a a[NK], nxt[NK];
  f32x4a acc2[2 * NK];
  load_rows_bf16<NK>(R, ldR, r0, nR, H, lm, kq, a);
  load_tile_bf16<NK>(S, ldS, 0, nS, H, hq, nxt);
#pragma unroll
  for (int nt = 0; nt < 2 * NK; ++nt) acc2[nt] = f32x4a{0.f, 0.f, 0.f, 0.f};
  int64_t tgr[4];
  float lser[4], lorr[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t r = r0 + 4 * kq + reg;
    tgr[reg] = TRANS ? r : target[r < nR ? r : nR - 1];
    lser[reg] = TRANS ? 0.f : lse[r < nR ? r : nR - 1];
    lorr[reg] = TRANS ? 0.f : lse[m + (r < nR ? r : nR - 1)];
  }
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t s0 = t * kAT;
    store_tile_bf16<NK>(Ss, H, hq, nxt);
    __syncthreads();
    load_tile_bf16<NK>(S, ldS, t + 1 < ntiles ? s0 + kAT : s0, nS, H, hq, nxt);
    int64_t tgc[4];
    float lsec[4], lorc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t s = s0 + 16 * j + lm;
      tgc[j] = TRANS ? target[s < nS ? s : nS - 1] : s;
      lsec[j] = TRANS ? lse[s < nS ? s : nS - 1] : 0.f;
      lorc[j] = TRANS ? lse[m + (s < nS ? s : nS - 1)] : 0.f;
    }
    f32x4a acc[4];
    score_tile_bf16<NK>(a, Ss, H, lm, kq, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = s0 + 16 * j + lm < nS;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float d = (acc[j][reg] - (TRANS ? lsec[j] : lser[reg])) - (TRANS ? lorc[j] : lorr[reg]);
        float e = expf(d);
        if (tgr[reg] == tgc[j]) e = expm1f(d);  // the target's p - 1 without the cancellation (one lane of a row)
        store_g_bf16(Gs, lm, kq, j, reg, live ? e * sc : 0.f);
      }
    }
    wave_lds_fence();
    second_product_bf16<NK>(Gs, Ss, H, lm, kq, acc2);
    wave_lds_fence();
    __syncthreads();
  }
  // D: lane (lm, kq) holds rows 4 kq + reg, column 16 nt + lm
#pragma unroll
  for (int nt = 0; nt < 2 * NK; ++nt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t r = r0 + 4 * kq + reg;
      const int n = 16 * nt + lm;
      if (r < nR && n < H) out[r * ldo + n] = acc2[nt][reg];
    }
}

template <int NK>
int launch_fwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N, int H,
                    const int64_t *target, float *pairs, float *xt, hipStream_t s) {
  const size_t lds = stream_lds_bf16<NK>();
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_lp_all_fwd_bf16<NK>, lds));
  const dim3 grid((unsigned)((m + kAT - 1) / kAT), (unsigned)chunks_of(m, N));
  k_lp_all_fwd_bf16<NK><<<grid, dim3(256), lds, s>>>(Q, ldQ, m, E, ldE, N, H, target, chunk_of(m, N), pairs, xt);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

template <int NK, bool TRANS>
int launch_bwd_bf16(const uint16_t *R, int64_t ldR, int64_t nR, const uint16_t *S, int64_t ldS, int64_t nS, int H,
                    const int64_t *target, const float *lse, const float *gl, int64_t m, float *out, int64_t ldo,
                    hipStream_t s) {
  const size_t lds = stream_lds_bf16<NK>() + g_lds_bf16();
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_lp_all_bwd_bf16<NK, TRANS>, lds));
  const dim3 grid((unsigned)((nR + kAT - 1) / kAT));
  k_lp_all_bwd_bf16<NK, TRANS><<<grid, dim3(256), lds, s>>>(R, ldR, nR, S, ldS, nS, H, target, lse, gl, m, out, ldo);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int32_t mrgcn_lp_all_supported(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N,
                               int32_t H) {
  return Q && E && shape_ok(Q, ldQ, m, E, ldE, N, H) ? 1 : 0;
}

int64_t mrgcn_lp_all_chunk(void) { return kAllChunk; }

int64_t mrgcn_lp_all_workspace(int64_t m, int64_t N, int32_t H) {
  if (m < 1 || N < 1 || H < 1 || m >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return -1;
  // pairs [chunks][m][2] floats | parts [ceil(m / 256)] doubles
  return align256(chunks_of(m, N) * m * 2 * 4) + align256((m + kMergeTB - 1) / kMergeTB * 8);
}

int mrgcn_lp_all_fwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                         const int64_t *target, float *lse, float *xt, float *loss, void *workspace,
                         int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(Q && E && target && lse && xt && loss, "lp_all_fwd: NULL");
  MRGCN_REQUIRE(shape_ok(Q, ldQ, m, E, ldE, N, H),
                "lp_all_fwd: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, strides of whole 16-byte pieces)");
  MRGCN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= mrgcn_lp_all_workspace(m, N, H),
                "lp_all_fwd: workspace (mrgcn_lp_all_workspace bytes, 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = chunks_of(m, N), nparts = (m + kMergeTB - 1) / kMergeTB;
  float *pairs = (float *)workspace;
  double *parts = (double *)((char *)workspace + align256(nchunks * m * 2 * 4));
#define LP_ALL_FWD(NT) launch_fwd<NT>(Q, ldQ, m, E, ldE, N, H, target, pairs, xt, s)
  const int rc = LP_ALL_BY_WIDTH(H, LP_ALL_FWD);
#undef LP_ALL_FWD
  if (rc != MRGCN_OK) return rc;
  k_lp_all_merge<<<dim3((unsigned)nparts), dim3(kMergeTB), 0, s>>>(pairs, nchunks, m, xt, lse, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  k_lp_all_loss<<<dim3(1), dim3(kMergeTB), 0, s>>>(parts, nparts, m, loss);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_lp_all_bwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                         const int64_t *target, const float *lse, const float *gl, float *dQ, int64_t lddQ, float *dE,
                         int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)workspace;
  (void)workspace_bytes;  // the backward keeps nothing between its launches
  MRGCN_REQUIRE(Q && E && target && lse && gl, "lp_all_bwd: NULL");
  MRGCN_REQUIRE(shape_ok(Q, ldQ, m, E, ldE, N, H),
                "lp_all_bwd: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, strides of whole 16-byte pieces)");
  MRGCN_REQUIRE((!dQ || lddQ >= H) && (!dE || lddE >= H), "lp_all_bwd: lddQ, lddE >= H");
  hipStream_t s = (hipStream_t)stream;
  if (dQ) {
#define LP_ALL_DQ(NT) launch_bwd<NT, false>(Q, ldQ, m, E, ldE, N, H, target, lse, gl, m, dQ, lddQ, s)
    const int rc = LP_ALL_BY_WIDTH(H, LP_ALL_DQ);
#undef LP_ALL_DQ
    if (rc != MRGCN_OK) return rc;
  }
  if (dE) {
#define LP_ALL_DE(NT) launch_bwd<NT, true>(E, ldE, N, Q, ldQ, m, H, target, lse, gl, m, dE, lddE, s)
    const int rc = LP_ALL_BY_WIDTH(H, LP_ALL_DE);
#undef LP_ALL_DE
    if (rc != MRGCN_OK) return rc;
  }
  return MRGCN_OK;
}

int32_t mrgcn_lp_all_supported_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE,
                                    int64_t N, int32_t H) {
  return Q && E && shape_ok_bf16(Q, ldQ, m, E, ldE, N, H) ? 1 : 0;
}

int mrgcn_lp_all_fwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                          int32_t H, const int64_t *target, float *lse, float *xt, float *loss, void *workspace,
                          int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(Q && E && target && lse && xt && loss, "lp_all_fwd_bf16: NULL");
  MRGCN_REQUIRE(shape_ok_bf16(Q, ldQ, m, E, ldE, N, H),
                "lp_all_fwd_bf16: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, bf16 rows of ld % 32 == 0, ld >= "
                "32 ceil(H / 32), 16-byte aligned)");
  MRGCN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= mrgcn_lp_all_workspace(m, N, H),
                "lp_all_fwd_bf16: workspace (mrgcn_lp_all_workspace bytes, 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = chunks_of(m, N), nparts = (m + kMergeTB - 1) / kMergeTB;
  float *pairs = (float *)workspace;
  double *parts = (double *)((char *)workspace + align256(nchunks * m * 2 * 4));
#define LP_ALL_FWD16(NK) launch_fwd_bf16<NK>(Q, ldQ, m, E, ldE, N, H, target, pairs, xt, s)
  const int rc = LP_BF16_BY_WIDTH(H, LP_ALL_FWD16);
#undef LP_ALL_FWD16
  if (rc != MRGCN_OK) return rc;
  k_lp_all_merge<<<dim3((unsigned)nparts), dim3(kMergeTB), 0, s>>>(pairs, nchunks, m, xt, lse, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  k_lp_all_loss<<<dim3(1), dim3(kMergeTB), 0, s>>>(parts, nparts, m, loss);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_lp_all_bwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                          int32_t H, const int64_t *target, const float *lse, const float *gl, float *dQ, int64_t lddQ,
                          float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)workspace;
  (void)workspace_bytes;  // the backward keeps nothing between its launches
  MRGCN_REQUIRE(Q && E && target && lse && gl, "lp_all_bwd_bf16: NULL");
  MRGCN_REQUIRE(shape_ok_bf16(Q, ldQ, m, E, ldE, N, H),
                "lp_all_bwd_bf16: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, bf16 rows of ld % 32 == 0, ld >= "
                "32 ceil(H / 32), 16-byte aligned)");
  MRGCN_REQUIRE((!dQ || lddQ >= H) && (!dE || lddE >= H), "lp_all_bwd_bf16: lddQ, lddE >= H");
  hipStream_t s = (hipStream_t)stream;
  if (dQ) {
#define LP_ALL_DQ16(NK) launch_bwd_bf16<NK, false>(Q, ldQ, m, E, ldE, N, H, target, lse, gl, m, dQ, lddQ, s)
    const int rc = LP_BF16_BY_WIDTH(H, LP_ALL_DQ16);
#undef LP_ALL_DQ16
    if (rc != MRGCN_OK) return rc;
  }
  if (dE) {
#define LP_ALL_DE16(NK) launch_bwd_bf16<NK, true>(E, ldE, N, Q, ldQ, m, H, target, lse, gl, m, dE, lddE, s)
    const int rc = LP_BF16_BY_WIDTH(H, LP_ALL_DE16);
#undef LP_ALL_DE16
    if (rc != MRGCN_OK) return rc;
  }
  return MRGCN_OK;
}

}  // extern "C"
