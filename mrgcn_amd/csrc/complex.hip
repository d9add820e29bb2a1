// ComplEx decoder beside DistMult (Trouillon, Welbl, Riedel, Gaussier, Bouchard: "Complex Embeddings for Simple Link
// Prediction", ICML 2016, eq. 11): score(s, p, o) = Re sum_k e_s[k] r[k] conj(e_o[k]) over K = H / 2 complex numbers.
// The reference has DistMult only (mrgcn/tasks/link_prediction.py:645-665), so the paper stands where a reference call
// site would.  No new parameters: a row of the encoder's [N, H] output or of the `relations` table [R, H] is read as
// K real parts followed by K imaginary parts.
//   score     a wave per four triples (their rows in flight together), lanes over k, a fixed shuffle tree per
//             triple: a pure function of its inputs
//   backward  with g the score's gradient, and a row x = (xr | xi):
//               dE[s]   += g (rr or + ri oi | rr oi - ri or)
//               dE[o]   += g (sr rr - si ri | si rr + sr ri)
//               dRel[p] += g (sr or + si oi | sr oi - si or)
//             ONE route: along the caller's STABLE orders of the triples by s / p / o (SortedTriples,
//             mrgcn_distmult_orders) a wave sums a run of equal targets in registers; every row has one owner per
//             pass, runs that cross a wave's span meet in a slab and are added in wave order.  No float atomics: the
//             same bits on every run, with or without torch.use_deterministic_algorithms.
// Candidate scores (ranks, top-k) are lp_score.hpp's lp_stage<kLpComplEx> inside lp_eval.hip / distmult_topk.hip.
#include "common.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;
constexpr int kRun = 32;    // sorted triples per wave
constexpr int kCxK = 128;   // complex numbers per pass of a wave (2 per lane): grid.y covers K
constexpr int kFwdTPW = 4;  // triples per wave of the forward
constexpr int kJoin = 16;   // slab partials a joining wave keeps in flight

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// (A form with 8-byte loads of neighbouring pairs, as the backward has, was measured slower here: 100 us against 85 us
// at the FB15k-237 shape.)
__global__ __launch_bounds__(kTB) void k_complex_fwd(const float *__restrict__ E, int64_t ldE,
                                                     const float *__restrict__ Rel, int64_t ldR, int K,
                                                     const int64_t *__restrict__ tr, int64_t n,
                                                     float *__restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kTB / kWave) + (threadIdx.x >> 6);
  const int64_t t0 = w * kFwdTPW;
  if (t0 >= n) return;
  const int cnt = (int)((n - t0 < kFwdTPW) ? n - t0 : kFwdTPW);
  // the rows of the wave's kFwdTPW triples in flight together (one triple per wave waits a full memory latency per
  // 64 columns with six loads in flight)
  const float *s[kFwdTPW], *p[kFwdTPW], *o[kFwdTPW];
  float acc[kFwdTPW];
#pragma unroll
  for (int u = 0; u < kFwdTPW; ++u) {
    const int64_t t = t0 + (u < cnt ? u : cnt - 1);
    s[u] = E + tr[3 * t] * ldE;
    p[u] = Rel + tr[3 * t + 1] * ldR;
    o[u] = E + tr[3 * t + 2] * ldE;
    acc[u] = 0.f;
  }
  for (int k = lane; k < K; k += kWave) {
    float sr[kFwdTPW], si[kFwdTPW], rr[kFwdTPW], ri[kFwdTPW], xr[kFwdTPW], xi[kFwdTPW];
#pragma unroll
    for (int u = 0; u < kFwdTPW; ++u) {
      sr[u] = s[u][k]; si[u] = s[u][K + k];
      rr[u] = p[u][k]; ri[u] = p[u][K + k];
      xr[u] = o[u][k]; xi[u] = o[u][K + k];
    }
#pragma unroll
    for (int u = 0; u < kFwdTPW; ++u)
      acc[u] += (sr[u] * rr[u] - si[u] * ri[u]) * xr[u] + (si[u] * rr[u] + sr[u] * ri[u]) * xi[u];
  }
#pragma unroll
  for (int u = 0; u < kFwdTPW; ++u) {
    const float a = wave_sum(acc[u]);
    if (lane == 0 && u < cnt) scores[t0 + u] = a;
  }
}

// VEC (the backward's kernels): a lane takes the two neighbouring complex numbers k0 + 2 lane and the one after it as
// ONE 8-byte load of the real and one of the imaginary parts (K even, rows of an even stride from 8-byte aligned
// bases) where the scalar form takes k0 + lane and k0 + lane + 64.
using f32x2 = __attribute__((ext_vector_type(2))) float;

// a lane's two complex numbers of a row: k0 + lane and k0 + lane + 64 — VEC: k0 + 2 lane and the one after it — (zero
// past K); v = re0, re1, im0, im1
template <bool VEC>
__device__ __forceinline__ void cx_load(const float *__restrict__ row, int lane, int k0, int K, float v[4]) {
  if constexpr (VEC) {
    const int k = k0 + 2 * lane;
    const f32x2 z = {0.f, 0.f};
    const f32x2 re = k < K ? *reinterpret_cast<const f32x2 *>(row + k) : z;
    const f32x2 im = k < K ? *reinterpret_cast<const f32x2 *>(row + K + k) : z;
    v[0] = re.x; v[1] = re.y; v[2] = im.x; v[3] = im.y;
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + lane + kWave * j;
    v[j] = k < K ? row[k] : 0.f;
    v[2 + j] = k < K ? row[K + k] : 0.f;
  }
}
template <bool VEC, bool ADD>
__device__ __forceinline__ void cx_store(float *__restrict__ row, int lane, int k0, int K, const float v[4]) {
  if constexpr (VEC) {
    const int k = k0 + 2 * lane;
    if (k < K) {
      f32x2 *pr = reinterpret_cast<f32x2 *>(row + k), *pi = reinterpret_cast<f32x2 *>(row + K + k);
      f32x2 re = {v[0], v[1]}, im = {v[2], v[3]};
      if (ADD) {
        re += *pr;
        im += *pi;
      }
      *pr = re;
      *pi = im;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + lane + kWave * j;
    if (k < K) {
      row[k] = ADD ? row[k] + v[j] : v[j];
      row[K + k] = ADD ? row[K + k] + v[2 + j] : v[2 + j];
    }
  }
}

// flags of a pass-1 wave: its last run goes on past its span and starts in it (the wave owns the run) / its span holds
// one run that started before it and goes on after it (the run passes through)
constexpr int32_t kOwner = 1, kThrough = 2;

// WHICH: the column the triples are sorted by and the row the sums go to — 0: s (a = r, b = o, a conj-multiplied),
// 1: p (a = s, b = o, likewise), 2: o (a = s, b = r, a plain complex product).
//   WHICH != 2   re = ar br + ai bi     im = ar bi - ai br
//   WHICH == 2   re = ar br - ai bi     im = ai br + ar bi
template <int WHICH, bool VEC>
__global__ __launch_bounds__(kTB) void k_complex_bwd_runs(
    const float *__restrict__ E, int64_t ldE, const float *__restrict__ Rel, int64_t ldR, int K,
    const int64_t *__restrict__ tr, const int64_t *__restrict__ order, int64_t n, const float *__restrict__ g,
    float *__restrict__ out, int64_t ldo, float *__restrict__ slab, int32_t *__restrict__ flags,
    int32_t *__restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kTB / kWave) + (threadIdx.x >> 6);
  const int64_t t0 = w * kRun;
  if (t0 >= n) return;
  const int H = 2 * K;
  const int k0 = (int)blockIdx.y * kCxK;
  const int cnt = (int)((n - t0 < kRun) ? n - t0 : kRun);
  // lane l < cnt: sorted triple t0 + l; lane kRun: the one before the span, lane kRun + 1: the one after it
  int64_t pos = lane < cnt ? t0 + lane : lane == kRun ? t0 - 1 : lane == kRun + 1 ? t0 + cnt : -1;
  if (pos >= n) pos = -1;
  int32_t si = 0, pi = 0, oi = 0, kk = -1;
  float gi = 0.f;
  if (pos >= 0) {
    const int64_t i = order[pos];
    si = (int32_t)tr[3 * i]; pi = (int32_t)tr[3 * i + 1]; oi = (int32_t)tr[3 * i + 2];
    kk = WHICH == 0 ? si : WHICH == 1 ? pi : oi;
    gi = g[i];
  }
  const int32_t key_prev = __builtin_amdgcn_readlane(kk, kRun), key_next = __builtin_amdgcn_readlane(kk, kRun + 1);
  const int32_t key_first = __builtin_amdgcn_readlane(kk, 0);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int32_t cur = key_first;
  bool first = true;
  auto flush = [&](bool last) {
    if (first && cur == key_prev) cx_store<VEC, false>(slab + (2 * w) * (int64_t)H, lane, k0, K, acc);
    else if (last && cur == key_next) cx_store<VEC, false>(slab + (2 * w + 1) * (int64_t)H, lane, k0, K, acc);
    else cx_store<VEC, true>(out + (int64_t)cur * ldo, lane, k0, K, acc);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = 0.f;
  };
  for (int tb = 0; tb < cnt; tb += 4) {
    float a[4][4], b[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // four triples' rows in flight
      const int tt = (tb + u < cnt) ? tb + u : cnt - 1;
      const int64_t s_ = __builtin_amdgcn_readlane(si, tt), p_ = __builtin_amdgcn_readlane(pi, tt),
                    o_ = __builtin_amdgcn_readlane(oi, tt);
      cx_load<VEC>(WHICH == 0 ? Rel + p_ * ldR : E + s_ * ldE, lane, k0, K, a[u]);
      cx_load<VEC>(WHICH == 2 ? Rel + p_ * ldR : E + o_ * ldE, lane, k0, K, b[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (tb + u < cnt) {  // wave uniform
        const int32_t key = __builtin_amdgcn_readlane(kk, tb + u);
        const float gt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gi), tb + u));
        if (key != cur) {
          flush(false);
          first = false;
          cur = key;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float ar = a[u][j] * gt, ai = a[u][2 + j] * gt, br = b[u][j], bi = b[u][2 + j];
          if (WHICH == 2) {
            acc[j] += ar * br - ai * bi;
            acc[2 + j] += ai * br + ar * bi;
          } else {
            acc[j] += ar * br + ai * bi;
            acc[2 + j] += ar * bi - ai * br;
          }
        }
      }
    }
  }
  flush(true);
  if (lane == 0 && blockIdx.y == 0) {
    const bool single = key_first == cur, from_prev = key_first == key_prev, to_next = cur == key_next;
    flags[w] = (to_next && !(single && from_prev) ? kOwner : 0) | (single && from_prev && to_next ? kThrough : 0);
    keys[w] = cur;
  }
}

// the owner of a crossing run: its partial, then the first-run partials of the waves after it in wave order (those the
// run passes through, and the one it ends in)
template <bool VEC>
__global__ __launch_bounds__(kTB) void k_complex_bwd_join(int K, int64_t nw, const int32_t *__restrict__ flags,
                                                          const int32_t *__restrict__ keys,
                                                          const float *__restrict__ slab, float *__restrict__ out,
                                                          int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kTB / kWave) + (threadIdx.x >> 6);
  if (w >= nw || !(flags[w] & kOwner)) return;
  const int H = 2 * K;
  const int k0 = (int)blockIdx.y * kCxK;
  float acc[4];
  cx_load<VEC>(slab + (2 * w + 1) * (int64_t)H, lane, k0, K, acc);
  for (int64_t v = w + 1; v < nw;) {
    const int64_t q = v + lane;
    const uint64_t stop = __ballot(!(q < nw && (flags[q] & kThrough)));
    int m = stop ? __builtin_ctzll(stop) + 1 : kWave;  // partials to add from v on (the last one ends the run)
    if (m > nw - v) m = (int)(nw - v);
    // kJoin partials in flight, added in wave order: a hub relation's run crosses a thousand waves at the FB15k-237
    // shape, and its owner pays one memory latency per round (four in flight: 183 us for that one row)
    for (int j = 0; j < m; j += kJoin) {
      float p[kJoin][4];
#pragma unroll
      for (int u = 0; u < kJoin; ++u)
        cx_load<VEC>(slab + (2 * (v + (j + u < m ? j + u : m - 1))) * (int64_t)H, lane, k0, K, p[u]);
#pragma unroll
      for (int u = 0; u < kJoin; ++u)
        if (j + u < m)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += p[u][k];
    }
    if (stop) break;
    v += kWave;
  }
  cx_store<VEC, true>(out + (int64_t)keys[w] * ldo, lane, k0, K, acc);
}

template <int WHICH, bool VEC>
void bwd_column(dim3 grid, hipStream_t st, const float *E, int64_t ldE, const float *Rel, int64_t ldR, int K,
                const int64_t *tr, const int64_t *order, int64_t n, const float *g, float *out, int64_t ldo,
                float *slab, int32_t *flags, int32_t *keys, int64_t nw) {
  k_complex_bwd_runs<WHICH, VEC><<<grid, kTB, 0, st>>>(E, ldE, Rel, ldR, K, tr, order, n, g, out, ldo, slab, flags, keys);
  k_complex_bwd_join<VEC><<<grid, kTB, 0, st>>>(K, nw, flags, keys, slab, out, ldo);
}

template <bool VEC>
void bwd_columns(dim3 grid, hipStream_t st, const float *E, int64_t ldE, const float *Rel, int64_t ldR, int K,
                 const int64_t *tr, int64_t n, const float *g, const int64_t *os, const int64_t *op, const int64_t *oo,
                 float *dE, int64_t lddE, float *dRel, int64_t lddR, float *slab, int32_t *flags, int32_t *keys,
                 int64_t nw) {
  if (dE) {
    bwd_column<0, VEC>(grid, st, E, ldE, Rel, ldR, K, tr, os, n, g, dE, lddE, slab, flags, keys, nw);
    bwd_column<2, VEC>(grid, st, E, ldE, Rel, ldR, K, tr, oo, n, g, dE, lddE, slab, flags, keys, nw);
  }
  if (dRel) bwd_column<1, VEC>(grid, st, E, ldE, Rel, ldR, K, tr, op, n, g, dRel, lddR, slab, flags, keys, nw);
}

// may a lane take pairs of neighbouring complex numbers as 8-byte pieces?
inline bool pairs_ok(int K, const float *E, int64_t ldE, const float *Rel, int64_t ldR) {
  return K % 2 == 0 && ldE % 2 == 0 && ldR % 2 == 0 && (((uintptr_t)E | (uintptr_t)Rel) & 7) == 0;
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int mrgcn_complex_score_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                            const int64_t *triples, int64_t n, float *scores, void *stream) {
  MRGCN_REQUIRE(E && Rel && triples && scores && H > 0 && n >= 0, "complex_score: bad argument");
  MRGCN_REQUIRE(H % 2 == 0, "complex_score: H must be even (H / 2 complex numbers per row)");
  if (n == 0) return MRGCN_OK;
  const int per = kTB / kWave;
  const int64_t waves = (n + kFwdTPW - 1) / kFwdTPW;
  const unsigned blocks = (unsigned)((waves + per - 1) / per);
  k_complex_fwd<<<blocks, kTB, 0, (hipStream_t)stream>>>(E, ldE, Rel, ldR, H / 2, triples, n, scores);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_complex_bwd_workspace(int64_t n, int32_t H) {
  if (n < 0 || H <= 0 || H % 2 != 0) return -1;
  const int64_t nw = (n + kRun - 1) / kRun;
  // slab [2 nw, H] floats | flags [nw] | keys [nw]
  return (2 * nw * H * 4 + 255) / 256 * 256 + 2 * ((nw * 4 + 255) / 256 * 256);
}

int mrgcn_complex_score_bwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                const int64_t *triples, int64_t n, const float *dscores, const int64_t *order_s,
                                const int64_t *order_p, const int64_t *order_o, float *dE, int64_t lddE, float *dRel,
                                int64_t lddR, void *workspace, int64_t workspace_bytes, void *stream) {
  MRGCN_REQUIRE(E && Rel && triples && dscores && H > 0 && n >= 0 && n < ((int64_t)1 << 31),
                "complex_score_bwd: bad argument");
  MRGCN_REQUIRE(H % 2 == 0, "complex_score_bwd: H must be even (H / 2 complex numbers per row)");
  if (n == 0 || (!dE && !dRel)) return MRGCN_OK;
  MRGCN_REQUIRE((!dE || (order_s && order_o)) && (!dRel || order_p), "complex_score_bwd: missing order");
  MRGCN_REQUIRE(workspace && workspace_bytes >= mrgcn_complex_bwd_workspace(n, H),
                "complex_score_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int K = H / 2;
  const int64_t nw = (n + kRun - 1) / kRun;
  char *w = (char *)workspace;
  float *slab = (float *)w;
  int32_t *flags = (int32_t *)(w + (2 * nw * H * 4 + 255) / 256 * 256);
  int32_t *keys = (int32_t *)((char *)flags + (nw * 4 + 255) / 256 * 256);
  const dim3 grid((unsigned)((nw + kTB / kWave - 1) / (kTB / kWave)), (unsigned)((K + kCxK - 1) / kCxK));
  if (pairs_ok(K, E, ldE, Rel, ldR) && (!dE || (lddE % 2 == 0 && ((uintptr_t)dE & 7) == 0)) &&
      (!dRel || (lddR % 2 == 0 && ((uintptr_t)dRel & 7) == 0)))
    bwd_columns<true>(grid, st, E, ldE, Rel, ldR, K, triples, n, dscores, order_s, order_p, order_o, dE, lddE, dRel,
                      lddR, slab, flags, keys, nw);
  else
    bwd_columns<false>(grid, st, E, ldE, Rel, ldR, K, triples, n, dscores, order_s, order_p, order_o, dE, lddE, dRel,
                       lddR, slab, flags, keys, nw);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
