// The DistMult candidate scores shared by the rank kernel (distmult.hip: k_rank_counts) and the top-k kernel
// (distmult_topk.hip: k_topk_tiles): ONE body, so that a fact that "ranks 3" sits at position 3 of the list
// predict_topk returns — the same float32 products in the same order, bit for bit.
// lp_score_tiles below is the same sum for several candidates per thread (lp_batches.hip: a batch's own small table).
// The body takes a scorer (template parameter SC, lp_stage below): DistMult, whose instantiation is the arithmetic it
// always was, and ComplEx, which stages one pair vector per side and runs the tail side's inner loop on both.
#pragma once

#include "common.hpp"

namespace mrgcn {

constexpr int kLpTB = 256;  // candidates per block (one per thread)
constexpr int kLpFB = 8;    // facts / queries per block
constexpr int kLpHT = 64;   // h tile of the per-fact vectors in LDS

// Et[h, c] = E[c, h] on `s` (distmult.hip)
hipError_t lp_transpose(const float *E, int64_t ldE, int64_t N, int H, float *Et, hipStream_t s);

__device__ __forceinline__ bool in_sorted(const int32_t *__restrict__ a, int64_t lo, int64_t hi, int32_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t v = a[mid];
    if (v == key) return true;
    if (v < key) lo = mid + 1; else hi = mid;
  }
  return false;
}

// rank = greater + round_half_even((ties - 1) / 2) + 1 (link_prediction.py:633-641): the rule of distmult.hip's
// k_rank_final, kept here for the rank kernels of other units (lp_eval.hip)
__device__ __forceinline__ int64_t lp_rank_of(int64_t gt, int64_t eq) {
  const int64_t m = eq - 1;                       // >= 0: the fact's own answer always ties and is never masked
  int64_t half = m >> 1;
  if ((m & 1) && (half & 1)) half += 1;           // x.5 rounds to the even neighbour
  return gt + half + 1;
}

// The scoring functions a candidate body serves.  DistMult (link_prediction.py:645-665): sum_h (E[s,h] Rel[p,h]) E[o,h].
// ComplEx (Trouillon et al. 2016, eq. 11): Re sum_k e_s[k] r[k] conj(e_o[k]) over K = H / 2 complex numbers, a row's
// first K columns the real and its last K the imaginary parts.
constexpr int kLpDistMult = 0;
constexpr int kLpComplEx = 1;

// The staged values of column hh for one (anchor, relation) pair.  DistMult: tail side a = E[anchor,hh] Rel[rel,hh];
// head side a = Rel[rel,hh], b = E[anchor,hh] (the candidate is multiplied in first, as the reference associates).
// ComplEx: a = q[hh], the pair vector whose plain dot product with a candidate's row IS the score, on either side
// (b unused) — with x the anchor's row, r the relation's, k = hh mod K:
//   tail (anchor = s)   q[k] = xr rr - xi ri     q[K + k] = xi rr + xr ri
//   head (anchor = o)   q[k] = rr xr + ri xi     q[K + k] = rr xi - ri xr
// each product rounded to float32, then the sum or difference rounded once (nothing contracted).  Column hh reads its
// partner column hh +- K of both rows from global memory; K need not be a multiple of the h tile.
template <int SC>
__device__ __forceinline__ void lp_stage(const float *__restrict__ E, int64_t ldE, const float *__restrict__ Rel,
                                         int64_t ldR, int H, bool head, int64_t anchor, int64_t rel, int hh, float &a,
                                         float &b) {
#pragma clang fp contract(off)
  if constexpr (SC == kLpComplEx) {
    const int K = H >> 1;
    const bool im = hh >= K;
    const int k = im ? hh - K : hh;
    const float *x = E + anchor * ldE, *r = Rel + rel * ldR;
    const float xr = x[k], xi = x[K + k], rr = r[k], ri = r[K + k];
    const float p1 = im ? xi * rr : xr * rr;
    const float p2 = im ? xr * ri : xi * ri;
    a = (im != head) ? p1 + p2 : p1 - p2;
    b = 0.f;
  } else {
    const float pv = Rel[rel * ldR + hh];
    const float ev = E[anchor * ldE + hh];
    if (head) {
      a = pv;
      b = ev;
    } else {
      a = ev * pv;
    }
  }
}

// acc[i] = the score of candidate c (this thread's; `live` = c < N) for pair i < nfb of the block, candidates read
// coalesced from the transposed table.  head == false: the candidate fills the tail slot,
// acc += (E[anchor,h] Rel[rel,h]) * E[c,h]; head == true: the head slot, acc += (E[c,h] Rel[rel,h]) * E[anchor,h];
// sequential over h = 0 .. H-1, nothing contracted.  ids(i, anchor, rel) names pair i's rows.  Every thread of the
// block must call it (barriers); s_a / s_b are the block's [kLpFB][kLpHT] staging arrays.
template <int SC = kLpDistMult, class Ids>
__device__ __forceinline__ void lp_score_tile(const float *__restrict__ Et, int64_t N, int H,
                                              const float *__restrict__ E, int64_t ldE,
                                              const float *__restrict__ Rel, int64_t ldR, bool head, int64_t c,
                                              bool live, int nfb, Ids ids, float (*s_a)[kLpHT], float (*s_b)[kLpHT],
                                              float (&acc)[kLpFB]) {
#pragma clang fp contract(off)
  const bool two = head && SC == kLpDistMult;   // two products per h (the ComplEx pair vector is staged whole)
#pragma unroll
  for (int i = 0; i < kLpFB; ++i) acc[i] = 0.f;
  for (int h0 = 0; h0 < H; h0 += kLpHT) {
    const int hn = (H - h0) < kLpHT ? (H - h0) : kLpHT;
    __syncthreads();
    for (int i = threadIdx.x; i < kLpFB * kLpHT; i += kLpTB) {
      const int fi = i / kLpHT, h = i % kLpHT;
      float a = 0.f, b = 0.f;
      if (fi < nfb && h < hn) {
        int64_t anchor, rel;
        ids(fi, anchor, rel);
        lp_stage<SC>(E, ldE, Rel, ldR, H, head, anchor, rel, h0 + h, a, b);
      }
      s_a[fi][h] = a;
      s_b[fi][h] = b;
    }
    __syncthreads();
    if (live) {
      for (int h = 0; h < hn; ++h) {
        const float e = Et[(int64_t)(h0 + h) * N + c];
        if (two) {
#pragma unroll
          for (int i = 0; i < kLpFB; ++i) {
            const float ep = e * s_a[i][h];
            const float epo = ep * s_b[i][h];
            acc[i] = acc[i] + epo;
          }
        } else {
#pragma unroll
          for (int i = 0; i < kLpFB; ++i) {
            const float spe = s_a[i][h] * e;
            acc[i] = acc[i] + spe;
          }
        }
      }
    }
  }
}

// One h step of lp_score_tile's sum for CT candidates (values e[j]) and the block's kLpFB pairs: the same float32
// operations in the same order.
template <int CT, bool HEAD>
__device__ __forceinline__ void lp_score_step(const float (*s_a)[kLpHT], const float (*s_b)[kLpHT], int h,
                                              const float (&e)[CT], float (&acc)[CT][kLpFB]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < kLpFB; ++i) {
    const float a = s_a[i][h];
    if (HEAD) {
      const float b = s_b[i][h];
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const float ep = e[j] * a;
        const float epo = ep * b;
        acc[j][i] = acc[j][i] + epo;
      }
    } else {
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const float spe = a * e[j];
        acc[j][i] = acc[j][i] + spe;
      }
    }
  }
}

constexpr int kLpHC = 16;   // h values of a candidate fetched ahead of their use (lp_score_tiles)

// The hn staged h values of one h tile for CT candidates: the candidates' values of kLpHC consecutive h are loaded
// first, straight-line at clamped positions (kLpHC * CT loads in flight: a load per step behind its use pays a full
// memory latency per h), then added in rising h.
template <int CT, bool HEAD>
__device__ __forceinline__ void lp_score_htile(const float *__restrict__ row, int64_t N, int hn,
                                               const int64_t (&cc)[CT], const float (*s_a)[kLpHT],
                                               const float (*s_b)[kLpHT], float (&acc)[CT][kLpFB]) {
  for (int hc = 0; hc < hn; hc += kLpHC) {
    float e[kLpHC][CT];
#pragma unroll
    for (int k = 0; k < kLpHC; ++k) {
      const int h = (hc + k) < hn ? hc + k : hn - 1;
#pragma unroll
      for (int j = 0; j < CT; ++j) e[k][j] = row[(int64_t)h * N + cc[j]];
    }
    if (hc + kLpHC <= hn) {
#pragma unroll
      for (int k = 0; k < kLpHC; ++k) lp_score_step<CT, HEAD>(s_a, s_b, hc + k, e[k], acc);
    } else {
#pragma unroll
      for (int k = 0; k < kLpHC; ++k)
        if (hc + k < hn) lp_score_step<CT, HEAD>(s_a, s_b, hc + k, e[k], acc);
    }
  }
}

// lp_score_tile for CT candidates per thread at once — c, c + kLpTB, ..., c + (CT - 1) kLpTB — so that a block which owns
// its pairs across several candidate tiles (lp_batches.hip) stages the pairs' vectors once and reads each staged value
// from LDS once for all CT candidates: acc[j][i] = the score of candidate c + j kLpTB for pair i, by the SAME float32
// operations in the same order as lp_score_tile (bit for bit; tests/test_gpu_lp_batches_kernels.py).  Candidates past
// the table are read at the clamped id N - 1 (straight-line loads, no branch); their acc is not meaningful.
template <int CT, int SC = kLpDistMult, class Ids>
__device__ __forceinline__ void lp_score_tiles(const float *__restrict__ Et, int64_t N, int H,
                                               const float *__restrict__ E, int64_t ldE,
                                               const float *__restrict__ Rel, int64_t ldR, bool head, int64_t c,
                                               int nfb, Ids ids, float (*s_a)[kLpHT], float (*s_b)[kLpHT],
                                               float (&acc)[CT][kLpFB]) {
#pragma clang fp contract(off)
  int64_t cc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int64_t cj = c + (int64_t)j * kLpTB;
    cc[j] = cj < N ? cj : N - 1;
#pragma unroll
    for (int i = 0; i < kLpFB; ++i) acc[j][i] = 0.f;
  }
  for (int h0 = 0; h0 < H; h0 += kLpHT) {
    const int hn = (H - h0) < kLpHT ? (H - h0) : kLpHT;
    __syncthreads();
    for (int i = threadIdx.x; i < kLpFB * kLpHT; i += kLpTB) {
      const int fi = i / kLpHT, h = i % kLpHT;
      float a = 0.f, b = 0.f;
      if (fi < nfb && h < hn) {
        int64_t anchor, rel;
        ids(fi, anchor, rel);
        lp_stage<SC>(E, ldE, Rel, ldR, H, head, anchor, rel, h0 + h, a, b);
      }
      s_a[fi][h] = a;
      s_b[fi][h] = b;
    }
    __syncthreads();
    const float *row = Et + (int64_t)h0 * N;
    if (head && SC == kLpDistMult)
      lp_score_htile<CT, true>(row, N, hn, cc, s_a, s_b, acc);
    else
      lp_score_htile<CT, false>(row, N, hn, cc, s_a, s_b, acc);
  }
}

}  // namespace mrgcn
