// The KvsAll decoder ("1-N scoring"): every DISTINCT query vector Q[q] (the pair vector of an (s, p, ?) or (?, p, o)
// query, built by the caller: this unit does not know the scorer) is scored against ALL rows of the candidate table E
// under a binary cross-entropy whose target is multi-hot — all known answers of the query are positives — and label
// smoothed,
//     x[q][c] = Q[q] . E[c]    Y'[q][c] = (1 - eps) [c in ans(q)] + eps / N    loss = mean over m N of bce(x, Y')
// — the objective of Dettmers, Minervini, Stenetorp, Riedel: "Convolutional 2D Knowledge Graph Embeddings", AAAI 2018
// (section "1-N scoring"; label smoothing after Szegedy et al.: "Rethinking the Inception Architecture for Computer
// Vision", CVPR 2016), which Ruffinelli, Broscheit, Gemulla ("You CAN Teach an Old Dog New Tricks!", ICLR 2020) found,
// with 1-vs-all, to train DistMult and ComplEx best.  The reference has the sampled BCE only
// (mrgcn/tasks/link_prediction.py:645-665, :550-554), so the papers stand where a reference call site would.
//
// No label enters the dense kernels.  With softplus(x) = log(1 + e^x),
//     sum_c bce(x[q][c], Y'[q][c]) = sum_c softplus(x[q][c]) - (eps / N) sum_c x[q][c] - (1 - eps) sum_{c in ans(q)} x[q][c]
//     d / dx[q][c]                 = sigmoid(x[q][c]) - eps / N - (1 - eps) [c in ans(q)]
// so the work is a DENSE part over the [m, N] scores, which are never stored (lp_tile.hpp's 64 x 64 tiles, as
// lp_all.hip), and a SPARSE correction over the nnz (query, answer) pairs.
//   forward   k_kv_fwd        per query and candidate chunk (sum softplus(x), sum x) over the live candidates
//             k_kv_pos        P[q] = sum_{c in ans(q)} Q[q] . E[c], a wave per query, the answers in list order
//             k_kv_merge      the chunk pairs added in chunk order in float64, per_query = S - (eps / N) X - (1 - eps) P,
//                             block partials in a fixed float64 tree; k_kv_loss: their sum / (m N), rounded once
//   backward  k_kv_bwd        G = (sigmoid(x) - eps / N) gl / (m N) on live pairs; dQ = G . E, dE = G^T . Q, one owning
//                             block per output row (k_lp_all_bwd's structure).  The labels' part, -(1 - eps) on
//                             the listed pairs, enters the G tile as it is formed: a lane per row walks the row's list
//                             — the answers of query r for dQ, the queries that have candidate r as an answer for dE;
//                             both ascend, as the tiles do — into a 64-bit mask of the tile's columns, and a listed
//                             pair takes G = (eps (1 - 1 / N) - sigmoid(-x)) gl / (m N), with sigmoid(-x) = 1 -
//                             sigmoid(x) from the same exponential, not by the subtraction.  (Subtracting the part
//                             from the finished row instead, out[r] -= (1 - eps) gl / (m N) sum T[a], cancels: a row
//                             whose listed pairs score high then keeps the rounding of a sum it no longer holds.)
// No float atomics anywhere: the same bits on every run, with or without torch.use_deterministic_algorithms.
#include "lp_tile.hpp"

namespace mrgcn {
namespace {

// log(1 + e^x) without overflow
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float wave_sum64(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// forward, dense: block (x, y) = query tile x, candidate chunk y -> pairs[y][q] = (sum softplus(x), sum x) over the
// chunk's candidates.  A lane adds its own columns tile after tile; the 16 lanes of a row meet once, at the end.
template <int NT>
__global__ __launch_bounds__(256) void k_kv_fwd(const float *__restrict__ Q, int64_t ldQ, int64_t m,
                                                const float *__restrict__ E, int64_t ldE, int64_t N, int H,
                                                int64_t chunk, float *__restrict__ pairs) {
  extern __shared__ __align__(16) float lp_kv_lds[];
  float *Es = lp_kv_lds;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = (H + 15) / 16 * 4, lds = 4 * hq + 4;
  const int64_t q0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t cbeg = (int64_t)blockIdx.y * chunk, cend = cbeg + chunk < N ? cbeg + chunk : N;
  const int64_t ntiles = (cend - cbeg + kAT - 1) / kAT;
  f32x4a a[4 * NT], nxt[4 * NT];
  load_rows<NT>(Q, ldQ, q0, m, H, lm, kq, a);
  load_tile<NT>(E, ldE, cbeg, N, H, hq, nxt);
  float sp[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t c0 = cbeg + t * kAT;
    store_tile<NT>(Es, lds, hq, nxt);
    __syncthreads();
    load_tile<NT>(E, ldE, t + 1 < ntiles ? c0 + kAT : c0, N, H, hq, nxt);  // (the last tile once more: no branch)
    f32x4a acc[4];
    score_tile<NT>(a, Es, lds, H, lm, kq, acc);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = c0 + 16 * j + lm < cend;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float x = acc[j][reg];
        sp[reg] += live ? softplus(x) : 0.f;
        sx[reg] += live ? x : 0.f;
      }
    }
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float s = row_sum(sp[reg]), x = row_sum(sx[reg]);
    const int64_t q = q0 + 4 * kq + reg;
    if (lm == 0 && q < m) {
      float *p = pairs + ((int64_t)blockIdx.y * m + q) * 2;
      p[0] = s;
      p[1] = x;
    }
  }
}

// forward, sparse: pos[q] = sum over the answers of q, in list order, of Q[q] . E[c].  A wave per query, lane l the
// 16-byte piece l of a row, four answer rows in flight (distmult_group.hip's pattern); the lanes meet once per query.
__global__ __launch_bounds__(256) void k_kv_pos(const float *__restrict__ Q, int64_t ldQ, int64_t m,
                                                const float *__restrict__ E, int64_t ldE, int H,
                                                const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                float *__restrict__ pos) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= m) return;  // (wave uniform; no barrier below)
  const bool on = 4 * lane < H;
  const int f0 = on ? 4 * lane : 0;
  const f32x4a qv = *reinterpret_cast<const f32x4a *>(Q + q * ldQ + f0);
  const int64_t beg = ptr[q], end = ptr[q + 1];
  float acc = 0.f;
  for (int64_t k = beg; k < end; k += 4) {
    f32x4a ev[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = idx[k + u < end ? k + u : end - 1];
      ev[u] = *reinterpret_cast<const f32x4a *>(E + c * ldE + f0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k + u < end) {  // wave uniform
        const f32x4a p = qv * ev[u];
        acc += (p.x + p.y) + (p.z + p.w);
      }
    }
  }
  acc = wave_sum64(on ? acc : 0.f);
  if (lane == 0) pos[q] = acc;
}

// per_query[q] = S - (eps / N) X - (1 - eps) P, S and X the chunk pairs added in chunk order in float64;
// part[block] = the sum of the block's values, float64 in a fixed tree
__global__ __launch_bounds__(kMergeTB) void k_kv_merge(const float *__restrict__ pairs, int64_t nchunks, int64_t m,
                                                       const float *__restrict__ pos, double eps_n, double keep,
                                                       float *__restrict__ per_query, double *__restrict__ part) {
  __shared__ double red[kMergeTB];
  const int64_t q = (int64_t)blockIdx.x * kMergeTB + threadIdx.x;
  double d = 0.0;
  if (q < m) {
    double S = 0.0, X = 0.0;
    for (int64_t k = 0; k < nchunks; ++k) {
      S += (double)pairs[(k * m + q) * 2];
      X += (double)pairs[(k * m + q) * 2 + 1];
    }
    d = S - eps_n * X - keep * (double)pos[q];
    if (per_query) per_query[q] = (float)d;
  }
  red[threadIdx.x] = d;
  __syncthreads();
  for (int off = kMergeTB / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// *loss = (float)(sum of the parts / count): thread t adds parts t, t + 256, ... in order, then the same tree
__global__ __launch_bounds__(kMergeTB) void k_kv_loss(const double *__restrict__ part, int64_t nparts, double count,
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
  if (threadIdx.x == 0) *loss = (float)(red[0] / count);
}

// backward, dense.  dQ: rows R = Q [nR = m], stream S = E [nS = N]; dE: rows R = E [nR = N], stream S = Q [nS = m] —
// with no label in it the gradient of a pair does not know which side is which, so both are this one kernel.
// out[r][:] = sum over stream rows s of G(r, s) S[s][:] with, on live pairs and sc = gl / count,
// G = (sigmoid(x) - eps_n) sc off the lists and (eps_in - sigmoid(-x)) sc on them, eps_in = eps (1 - 1 / N):
// sigmoid(x) - eps / N - (1 - eps) written without the cancellation.  list(r) = idx[ptr[r] .. ptr[r + 1]), ascending
// stream rows.
template <int NT>
__global__ __launch_bounds__(256) void k_kv_bwd(const float *__restrict__ R, int64_t ldR, int64_t nR,
                                                const float *__restrict__ S, int64_t ldS, int64_t nS, int H,
                                                const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                float eps_n, float eps_in, const float *__restrict__ gl, double count,
                                                float *__restrict__ out, int64_t ldo) {
  extern __shared__ __align__(16) float lp_kv_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = (H + 15) / 16 * 4, lds = 4 * hq + 4;
  float *Ss = lp_kv_lds;
  float *Gs = lp_kv_lds + kAT * lds + 16 * wv * kAGP;  // the wave's own 16 rows of the G tile
  const int64_t r0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t ntiles = (nS + kAT - 1) / kAT;
  const float sc = (float)((double)gl[0] / count);
  f32x4a a[4 * NT], nxt[4 * NT], acc2[4 * NT];
  load_rows<NT>(R, ldR, r0, nR, H, lm, kq, a);
  load_tile<NT>(S, ldS, 0, nS, H, hq, nxt);
  // lane i < 16 of a wave walks the list of the wave's row i: `cur` is its next listed stream row
  int64_t lp = 0, le = 0;
  if (lane < 16 && r0 + lane < nR) {
    lp = ptr[r0 + lane];
    le = ptr[r0 + lane + 1];
  }
  int64_t cur = lp < le ? (int64_t)idx[lp] : INT64_MAX;
#pragma unroll
  for (int nt = 0; nt < 4 * NT; ++nt) acc2[nt] = f32x4a{0.f, 0.f, 0.f, 0.f};
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t s0 = t * kAT;
    store_tile<NT>(Ss, lds, hq, nxt);
    __syncthreads();
    load_tile<NT>(S, ldS, t + 1 < ntiles ? s0 + kAT : s0, nS, H, hq, nxt);
    f32x4a acc[4];
    score_tile<NT>(a, Ss, lds, H, lm, kq, acc);
    // the tile's listed columns of row i as bit c - s0 of lane i's mask; lane (lm, kq) then takes its four rows'
    unsigned long long mine = 0;
    while (cur < s0 + kAT) {  // (lanes past 15 and rows without a listed pair in this tile: never entered)
      if (cur >= s0) mine |= 1ull << (int)(cur - s0);   // (a list that does not ascend marks nothing outside the tile)
      ++lp;
      cur = lp < le ? (int64_t)idx[lp] : INT64_MAX;
    }
    unsigned long long mk[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) mk[reg] = __shfl(mine, 4 * kq + reg, kWave);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = s0 + 16 * j + lm < nS;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        // one exponential gives both sigmoids: r = 1 / (1 + e^-|x|) is that of |x|, e r that of -|x|
        const float x = acc[j][reg], e = expf(-fabsf(x)), r = 1.f / (1.f + e), er = e * r;
        const float sg = x >= 0.f ? r : er, om = x >= 0.f ? er : r;   // sigmoid(x), sigmoid(-x)
        const bool listed = (mk[reg] >> (16 * j + lm)) & 1;
        Gs[(4 * kq + reg) * kAGP + 16 * j + lm] = live ? (listed ? eps_in - om : sg - eps_n) * sc : 0.f;
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
int launch_fwd(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int H, float *pairs,
               hipStream_t s) {
  const size_t lds = stream_lds(H);
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_kv_fwd<NT>, lds));
  const dim3 grid((unsigned)((m + kAT - 1) / kAT), (unsigned)chunks_of(m, N));
  k_kv_fwd<NT><<<grid, dim3(256), lds, s>>>(Q, ldQ, m, E, ldE, N, H, chunk_of(m, N), pairs);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

template <int NT>
int launch_bwd(const float *R, int64_t ldR, int64_t nR, const float *S, int64_t ldS, int64_t nS, int H,
               const int64_t *ptr, const int32_t *idx, float eps_n, float eps_in, const float *gl, double count,
               float *out, int64_t ldo, hipStream_t s) {
  const size_t lds = stream_lds(H) + (size_t)kAT * kAGP * sizeof(float);
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_kv_bwd<NT>, lds));
  const dim3 grid((unsigned)((nR + kAT - 1) / kAT));
  k_kv_bwd<NT><<<grid, dim3(256), lds, s>>>(R, ldR, nR, S, ldS, nS, H, ptr, idx, eps_n, eps_in, gl, count, out, ldo);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

// ---- the bf16 forms (lp_tile.hpp: the bf16 tile; lp_all.hip: what is rounded where) ----------------------------------
// The dense kernels on bf16 TABLES of Q and E: scores Q~ . E~ with fp32 sums, the softplus, the sigmoids and the list
// masks in fp32 as above, G rounded to bf16 once as it is stored, out = G~ . S~ in fp32.
template <int NK>
__global__ __launch_bounds__(256) void k_kv_fwd_bf16(const uint16_t *__restrict__ Q, int64_t ldQ, int64_t m,
                                                     const uint16_t *__restrict__ E, int64_t ldE, int64_t N, int H,
                                                     int64_t chunk, float *__restrict__ pairs) {
  extern __shared__ __align__(16) uint16_t lp_kv_lds16[];
  uint16_t *Es = lp_kv_lds16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = hp32(H) / 8;
  const int64_t q0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t cbeg = (int64_t)blockIdx.y * chunk, cend = cbeg + chunk < N ? cbeg + chunk : N;
  const int64_t ntiles = (cend - cbeg + kAT - 1) / kAT;
  bf16x8a a[NK], nxt[NK];
  load_rows_bf16<NK>(Q, ldQ, q0, m, H, lm, kq, a);
  load_tile_bf16<NK>(E, ldE, cbeg, N, H, hq, nxt);
  float sp[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t c0 = cbeg + t * kAT;
    store_tile_bf16<NK>(Es, H, hq, nxt);
    __syncthreads();
    load_tile_bf16<NK>(E, ldE, t + 1 < ntiles ? c0 + kAT : c0, N, H, hq, nxt);  // (the last tile once more: no branch)
    f32x4a acc[4];
    score_tile_bf16<NK>(a, Es, H, lm, kq, acc);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = c0 + 16 * j + lm < cend;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float x = acc[j][reg];
        sp[reg] += live ? softplus(x) : 0.f;
        sx[reg] += live ? x : 0.f;
      }
    }
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float s = row_sum(sp[reg]), x = row_sum(sx[reg]);
    const int64_t q = q0 + 4 * kq + reg;
    if (lm == 0 && q < m) {
      float *p = pairs + ((int64_t)blockIdx.y * m + q) * 2;
      p[0] = s;
      p[1] = x;
    }
  }
}

// pos[q] from the bf16 rows, in fp32 (the products exact): a wave per query, lane l the 16-byte piece l of a row
// (8 elements), four answer rows in flight
__global__ __launch_bounds__(256) void k_kv_pos_bf16(const uint16_t *__restrict__ Q, int64_t ldQ, int64_t m,
                                                     const uint16_t *__restrict__ E, int64_t ldE, int H,
                                                     const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                     float *__restrict__ pos) {
  using u32x4a = __attribute__((ext_vector_type(4))) uint32_t;
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= m) return;  // (wave uniform; no barrier below)
  const bool on = 8 * lane < H;   // (the piece lies inside [0, Hp): whole, zeros past H)
  const int f0 = on ? 8 * lane : 0;
  const u32x4a qv = *reinterpret_cast<const u32x4a *>(Q + q * ldQ + f0);
  const int64_t beg = ptr[q], end = ptr[q + 1];
  float acc = 0.f;
  for (int64_t k = beg; k < end; k += 4) {
    u32x4a ev[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = idx[k + u < end ? k + u : end - 1];
      ev[u] = *reinterpret_cast<const u32x4a *>(E + c * ldE + f0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k + u < end) {  // wave uniform
        float p[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[2 * i] = __uint_as_float(qv[i] << 16) * __uint_as_float(ev[u][i] << 16);
          p[2 * i + 1] = __uint_as_float(qv[i] & 0xffff0000u) * __uint_as_float(ev[u][i] & 0xffff0000u);
        }
        acc += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
      }
    }
  }
  acc = wave_sum64(on ? acc : 0.f);
  if (lane == 0) pos[q] = acc;
}

template <int NK>
__global__ __launch_bounds__(256) void k_kv_bwd_bf16(const uint16_t *__restrict__ R, int64_t ldR, int64_t nR,
                                                     const uint16_t *__restrict__ S, int64_t ldS, int64_t nS, int H,
                                                     const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                     float eps_n, float eps_in, const float *__restrict__ gl,
                                                     double count, float *__restrict__ out, int64_t ldo) {
  extern __shared__ __align__(16) uint16_t lp_kv_lds16[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lm = lane & 15, kq = lane >> 4;
  const int hq = hp32(H) / 8;
  uint16_t *Ss = lp_kv_lds16;
  uint16_t *Gs = lp_kv_lds16 + kAT * tile_ld<NK>() + 16 * wv * kBGP;  // the wave's own 16 rows of the G tile
  const int64_t r0 = (int64_t)blockIdx.x * kAT + 16 * wv;
  const int64_t ntiles = (nS + kAT - 1) / kAT;
  const float sc = (float)((double)gl[0] / count);
  bf16x8a a[NK], nxt[NK];
  f32x4a acc2[2 * NK];
  load_rows_bf16<NK>(R, ldR, r0, nR, H, lm, kq, a);
  load_tile_bf16<NK>(S, ldS, 0, nS, H, hq, nxt);
  // lane i < 16 of a wave walks the list of the wave's row i: `cur` is its next listed stream row
  int64_t lp = 0, le = 0;
  if (lane < 16 && r0 + lane < nR) {
    lp = ptr[r0 + lane];
    le = ptr[r0 + lane + 1];
  }
  int64_t cur = lp < le ? (int64_t)idx[lp] : INT64_MAX;
#pragma unroll
  for (int nt = 0; nt < 2 * NK; ++nt) acc2[nt] = f32x4a{0.f, 0.f, 0.f, 0.f};
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t s0 = t * kAT;
    store_tile_bf16<NK>(Ss, H, hq, nxt);
    __syncthreads();
    load_tile_bf16<NK>(S, ldS, t + 1 < ntiles ? s0 + kAT : s0, nS, H, hq, nxt);
    f32x4a acc[4];
    score_tile_bf16<NK>(a, Ss, H, lm, kq, acc);
    unsigned long long mine = 0;
    while (cur < s0 + kAT) {  // (lanes past 15 and rows without a listed pair in this tile: never entered)
      if (cur >= s0) mine |= 1ull << (int)(cur - s0);   // (a list that does not ascend marks nothing outside the tile)
      ++lp;
      cur = lp < le ? (int64_t)idx[lp] : INT64_MAX;
    }
    unsigned long long mk[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) mk[reg] = __shfl(mine, 4 * kq + reg, kWave);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = s0 + 16 * j + lm < nS;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        // one exponential gives both sigmoids: r = 1 / (1 + e^-|x|) is that of |x|, e r that of -|x|
        const float x = acc[j][reg], e = expf(-fabsf(x)), r = 1.f / (1.f + e), er = e * r;
        const float sg = x >= 0.f ? r : er, om = x >= 0.f ? er : r;   // sigmoid(x), sigmoid(-x)
        const bool listed = (mk[reg] >> (16 * j + lm)) & 1;
        store_g_bf16(Gs, lm, kq, j, reg, live ? (listed ? eps_in - om : sg - eps_n) * sc : 0.f);
      }
    }
    wave_lds_fence();   // (the list walk above diverges; the lanes have met again before the transposed reads)
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
                    float *pairs, hipStream_t s) {
  const size_t lds = stream_lds_bf16<NK>();
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_kv_fwd_bf16<NK>, lds));
  const dim3 grid((unsigned)((m + kAT - 1) / kAT), (unsigned)chunks_of(m, N));
  k_kv_fwd_bf16<NK><<<grid, dim3(256), lds, s>>>(Q, ldQ, m, E, ldE, N, H, chunk_of(m, N), pairs);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

template <int NK>
int launch_bwd_bf16(const uint16_t *R, int64_t ldR, int64_t nR, const uint16_t *S, int64_t ldS, int64_t nS, int H,
                    const int64_t *ptr, const int32_t *idx, float eps_n, float eps_in, const float *gl, double count,
                    float *out, int64_t ldo, hipStream_t s) {
  const size_t lds = stream_lds_bf16<NK>() + g_lds_bf16();
  MRGCN_HIP_TRY(raise_lds_limit((const void *)k_kv_bwd_bf16<NK>, lds));
  const dim3 grid((unsigned)((nR + kAT - 1) / kAT));
  k_kv_bwd_bf16<NK><<<grid, dim3(256), lds, s>>>(R, ldR, nR, S, ldS, nS, H, ptr, idx, eps_n, eps_in, gl, count, out,
                                                  ldo);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

inline bool eps_ok(double e) { return e >= 0.0 && e < 1.0; }  // (a NaN fails both)
inline int64_t pairs_bytes(int64_t m, int64_t N) { return align256(chunks_of(m, N) * m * 2 * 4); }

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int32_t mrgcn_lp_kvsall_supported(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N,
                                  int32_t H) {
  return Q && E && shape_ok(Q, ldQ, m, E, ldE, N, H) ? 1 : 0;
}

int64_t mrgcn_lp_kvsall_workspace(int64_t m, int64_t N, int32_t H) {
  if (m < 1 || N < 1 || H < 1 || m >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return -1;
  // pairs [chunks][m][2] floats | pos [m] floats | parts [ceil(m / 256)] doubles
  return pairs_bytes(m, N) + align256(m * 4) + align256((m + kMergeTB - 1) / kMergeTB * 8);
}

int mrgcn_lp_kvsall_fwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                            const int64_t *ans_ptr, const int32_t *ans_idx, double label_smoothing, float *per_query,
                            float *loss, void *workspace, int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(Q && E && ans_ptr && ans_idx && loss, "lp_kvsall_fwd: NULL");
  MRGCN_REQUIRE(shape_ok(Q, ldQ, m, E, ldE, N, H),
                "lp_kvsall_fwd: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, strides of whole 16-byte pieces)");
  MRGCN_REQUIRE(eps_ok(label_smoothing), "lp_kvsall_fwd: label_smoothing in [0, 1)");
  MRGCN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= mrgcn_lp_kvsall_workspace(m, N, H),
                "lp_kvsall_fwd: workspace (mrgcn_lp_kvsall_workspace bytes, 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = chunks_of(m, N), nparts = (m + kMergeTB - 1) / kMergeTB;
  float *pairs = (float *)workspace;
  float *pos = (float *)((char *)workspace + pairs_bytes(m, N));
  double *parts = (double *)((char *)pos + align256(m * 4));
#define LP_KV_FWD(NT) launch_fwd<NT>(Q, ldQ, m, E, ldE, N, H, pairs, s)
  const int rc = LP_ALL_BY_WIDTH(H, LP_KV_FWD);
#undef LP_KV_FWD
  if (rc != MRGCN_OK) return rc;
  k_kv_pos<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s>>>(Q, ldQ, m, E, ldE, H, ans_ptr, ans_idx, pos);
  MRGCN_HIP_TRY(hipGetLastError());
  k_kv_merge<<<dim3((unsigned)nparts), dim3(kMergeTB), 0, s>>>(pairs, nchunks, m, pos, label_smoothing / (double)N,
                                                                1.0 - label_smoothing, per_query, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  k_kv_loss<<<dim3(1), dim3(kMergeTB), 0, s>>>(parts, nparts, (double)m * (double)N, loss);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_lp_kvsall_bwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                            const int64_t *ans_ptr, const int32_t *ans_idx, const int64_t *cand_ptr,
                            const int32_t *cand_qry, double label_smoothing, const float *gl, float *dQ, int64_t lddQ,
                            float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)workspace;
  (void)workspace_bytes;  // the backward keeps nothing between its launches
  MRGCN_REQUIRE(Q && E && gl && (!dQ || (ans_ptr && ans_idx)) && (!dE || (cand_ptr && cand_qry)),
                "lp_kvsall_bwd: NULL (dQ needs the answer lists, dE the candidates' query lists)");
  MRGCN_REQUIRE(shape_ok(Q, ldQ, m, E, ldE, N, H),
                "lp_kvsall_bwd: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, strides of whole 16-byte pieces)");
  MRGCN_REQUIRE(eps_ok(label_smoothing), "lp_kvsall_bwd: label_smoothing in [0, 1)");
  MRGCN_REQUIRE((!dQ || lddQ >= H) && (!dE || lddE >= H), "lp_kvsall_bwd: lddQ, lddE >= H");
  hipStream_t s = (hipStream_t)stream;
  const double count = (double)m * (double)N;
  const float eps_n = (float)(label_smoothing / (double)N);
  const float eps_in = (float)(label_smoothing * (1.0 - 1.0 / (double)N));
  if (dQ) {
#define LP_KV_DQ(NT) launch_bwd<NT>(Q, ldQ, m, E, ldE, N, H, ans_ptr, ans_idx, eps_n, eps_in, gl, count, dQ, lddQ, s)
    const int rc = LP_ALL_BY_WIDTH(H, LP_KV_DQ);
#undef LP_KV_DQ
    if (rc != MRGCN_OK) return rc;
  }
  if (dE) {
#define LP_KV_DE(NT) launch_bwd<NT>(E, ldE, N, Q, ldQ, m, H, cand_ptr, cand_qry, eps_n, eps_in, gl, count, dE, lddE, s)
    const int rc = LP_ALL_BY_WIDTH(H, LP_KV_DE);
#undef LP_KV_DE
    if (rc != MRGCN_OK) return rc;
  }
  return MRGCN_OK;
}

int32_t mrgcn_lp_kvsall_supported_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE,
                                       int64_t N, int32_t H) {
  return Q && E && shape_ok_bf16(Q, ldQ, m, E, ldE, N, H) ? 1 : 0;
}

int mrgcn_lp_kvsall_fwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                             int32_t H, const int64_t *ans_ptr, const int32_t *ans_idx, double label_smoothing,
                             float *per_query, float *loss, void *workspace, int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(Q && E && ans_ptr && ans_idx && loss, "lp_kvsall_fwd_bf16: NULL");
  MRGCN_REQUIRE(shape_ok_bf16(Q, ldQ, m, E, ldE, N, H),
                "lp_kvsall_fwd_bf16: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, bf16 rows of ld % 32 == 0, ld "
                ">= 32 ceil(H / 32), 16-byte aligned)");
  MRGCN_REQUIRE(eps_ok(label_smoothing), "lp_kvsall_fwd_bf16: label_smoothing in [0, 1)");
  MRGCN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= mrgcn_lp_kvsall_workspace(m, N, H),
                "lp_kvsall_fwd_bf16: workspace (mrgcn_lp_kvsall_workspace bytes, 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = chunks_of(m, N), nparts = (m + kMergeTB - 1) / kMergeTB;
  float *pairs = (float *)workspace;
  float *pos = (float *)((char *)workspace + pairs_bytes(m, N));
  double *parts = (double *)((char *)pos + align256(m * 4));
#define LP_KV_FWD16(NK) launch_fwd_bf16<NK>(Q, ldQ, m, E, ldE, N, H, pairs, s)
  const int rc = LP_BF16_BY_WIDTH(H, LP_KV_FWD16);
#undef LP_KV_FWD16
  if (rc != MRGCN_OK) return rc;
  k_kv_pos_bf16<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s>>>(Q, ldQ, m, E, ldE, H, ans_ptr, ans_idx, pos);
  MRGCN_HIP_TRY(hipGetLastError());
  k_kv_merge<<<dim3((unsigned)nparts), dim3(kMergeTB), 0, s>>>(pairs, nchunks, m, pos, label_smoothing / (double)N,
                                                                1.0 - label_smoothing, per_query, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  k_kv_loss<<<dim3(1), dim3(kMergeTB), 0, s>>>(parts, nparts, (double)m * (double)N, loss);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_lp_kvsall_bwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                             int32_t H, const int64_t *ans_ptr, const int32_t *ans_idx, const int64_t *cand_ptr,
                             const int32_t *cand_qry, double label_smoothing, const float *gl, float *dQ, int64_t lddQ,
                             float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)workspace;
  (void)workspace_bytes;  // the backward keeps nothing between its launches
  MRGCN_REQUIRE(Q && E && gl && (!dQ || (ans_ptr && ans_idx)) && (!dE || (cand_ptr && cand_qry)),
                "lp_kvsall_bwd_bf16: NULL (dQ needs the answer lists, dE the candidates' query lists)");
  MRGCN_REQUIRE(shape_ok_bf16(Q, ldQ, m, E, ldE, N, H),
                "lp_kvsall_bwd_bf16: shape (H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, bf16 rows of ld % 32 == 0, ld "
                ">= 32 ceil(H / 32), 16-byte aligned)");
  MRGCN_REQUIRE(eps_ok(label_smoothing), "lp_kvsall_bwd_bf16: label_smoothing in [0, 1)");
  MRGCN_REQUIRE((!dQ || lddQ >= H) && (!dE || lddE >= H), "lp_kvsall_bwd_bf16: lddQ, lddE >= H");
  hipStream_t s = (hipStream_t)stream;
  const double count = (double)m * (double)N;
  const float eps_n = (float)(label_smoothing / (double)N);
  const float eps_in = (float)(label_smoothing * (1.0 - 1.0 / (double)N));
  if (dQ) {
#define LP_KV_DQ16(NK) \
  launch_bwd_bf16<NK>(Q, ldQ, m, E, ldE, N, H, ans_ptr, ans_idx, eps_n, eps_in, gl, count, dQ, lddQ, s)
    const int rc = LP_BF16_BY_WIDTH(H, LP_KV_DQ16);
#undef LP_KV_DQ16
    if (rc != MRGCN_OK) return rc;
  }
  if (dE) {
#define LP_KV_DE16(NK) \
  launch_bwd_bf16<NK>(E, ldE, N, Q, ldQ, m, H, cand_ptr, cand_qry, eps_n, eps_in, gl, count, dE, lddE, s)
    const int rc = LP_BF16_BY_WIDTH(H, LP_KV_DE16);
#undef LP_KV_DE16
    if (rc != MRGCN_OK) return rc;
  }
  return MRGCN_OK;
}

}  // extern "C"
