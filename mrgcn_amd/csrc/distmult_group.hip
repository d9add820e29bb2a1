// Grouped DistMult loss over a fact's keyed negatives (link prediction):
//   score  mrgcn/tasks/link_prediction.py:645-665   sum_h (E[s,h] * Rel[p,h]) * E[o,h]
//   loss   :550-554                                  BCEWithLogitsLoss (mean), here with a positive weight, or the
//                                                    per-fact softmax loss over the fact and its negatives
// The triples have NegativeSampler's layout (csrc/lp_negatives.hip): rows [0, n) are the facts, row n + i * rate + j is
// negative j of fact i, which keeps fact i's predicate and one of its two ends.  The flat decoder (distmult.hip) scores
// and differentiates the n * (1 + rate) rows as independent triples: three gathered rows each in the forward, two rows
// in each of three sorted backward passes.  Here a wave owns a GROUP — fact i and its negatives: it reads the fact's
// three rows once and ONE row per negative (the changed end), and it knows the group, which the softmax loss needs.
//
// Side rule: a negative whose column 0 differs from the fact's subject is head-corrupted (changed end = column 0), any
// other is tail-corrupted (changed end = column 2).  A negative equal to its fact is therefore a tail negative with the
// fact's own object, and the fact itself is member 0 of its group under the same rule: score (s p) c with c = o.
//
//   forward   k_group_fwd<LOSS>     scores (the bits of k_distmult_fwd4: same products, lane sum and wave_sum),
//                                   g = dloss / dscore, block partials of the loss; k_group_final adds the partials in
//                                   a fixed order (no float atomic on the loss)
//   backward  k_group_bwd<SCRATCH>  A = g0 o + sum_tail g_j c_j and Hd = sum_head g_j c_j in registers, then
//                                     dE[s] += p A,  dE[o] += p (g0 s + Hd),  dRel[p] += s A + o Hd,
//                                     dE[c_j] += g_j (s p)  (tail)  or  g_j (p o)  (head)
//             SCRATCH = false       everything by row atomics (mini-batches: too few rows to collide)
//             SCRATCH = true        the three per-fact rows STORED to [n, H] scratch, the changed ends written as sort
//                                   keys; k_group_rows_sum adds the stored rows along the facts' stored orders (runs of
//                                   equal target summed in registers), a one-key radix sort orders the negatives by
//                                   changed end and k_group_bwd_negs run-sums their contributions the same way
// The upstream gradient is a device scalar, read by the backward kernels.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.hpp"
#include "config.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;
constexpr int kWaves = kTB / kWave;
constexpr int kGroupBlocks = 4096;   // grid cap of the group kernels (waves stride over the groups): the partials' count
constexpr int kRun = 32;             // sorted entries per wave and run, as k_distmult_bwd_sorted4
constexpr int kRelRuns = 4;          // runs per wave along the predicate order (few keys, long segments)
using f32x4d = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, kWave));
  return x;
}
__device__ __forceinline__ float lane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ void row_atomic(float *__restrict__ o, const f32x4d v) {
  if (v.x != 0.f) atomicAdd(o + 0, v.x);
  if (v.y != 0.f) atomicAdd(o + 1, v.y);
  if (v.z != 0.f) atomicAdd(o + 2, v.z);
  if (v.w != 0.f) atomicAdd(o + 3, v.w);
}

// ---- forward: scores, dloss/dscore and the loss partials, one wave per group ----------------------------------------
// LOSS 0: BCE with positive weight w, mean over n (1 + rate) scores (inv = 1 / that count);  LOSS 1: -log softmax of the
// fact among its group, mean over facts (inv = 1 / n).  Member m of group i: m = 0 the fact (row i), m >= 1 negative
// m - 1 (row n + i rate + m - 1).  A lane holds four features of a row and, per chunk of 64 members, one member's ids
// and score.
template <int LOSS>
__global__ __launch_bounds__(kTB) void k_group_fwd(const float *__restrict__ E, int64_t ldE,
                                                   const float *__restrict__ Rel, int64_t ldR, int H,
                                                   const int64_t *__restrict__ tr, int64_t n, int rate, float w,
                                                   float inv, float *scores, float *__restrict__ g,
                                                   float *__restrict__ partial) {
  __shared__ float s_part[kWaves];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const bool on = 4 * lane < H;
  const int f0 = on ? 4 * lane : 0;
  const int members = rate + 1;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wv; i < n; i += nwaves) {
    const int64_t si = tr[3 * i], pi = tr[3 * i + 1], oi = tr[3 * i + 2];
    const f32x4d sv = *reinterpret_cast<const f32x4d *>(E + si * ldE + f0);
    const f32x4d pv = *reinterpret_cast<const f32x4d *>(Rel + pi * ldR + f0);
    const f32x4d ov = *reinterpret_cast<const f32x4d *>(E + oi * ldE + f0);
    const int64_t nb = n + i * (int64_t)rate - 1;   // member m >= 1 is row nb + m
    float mx = -INFINITY, se = 0.f, x0 = 0.f, my = 0.f;
    for (int m0 = 0; m0 < members; m0 += kWave) {
      const int cnt = members - m0 < kWave ? members - m0 : kWave;
      const int m = m0 + (lane < cnt ? lane : cnt - 1);
      const int64_t row = m == 0 ? i : nb + m;
      const int32_t c0 = (int32_t)tr[3 * row], c2 = (int32_t)tr[3 * row + 2];
      const int hd = c0 != (int32_t)si;
      const int32_t ch = hd ? c0 : c2;
      for (int tb = 0; tb < cnt; tb += 4) {
        f32x4d cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four members' rows in flight
          const int tt = tb + u < cnt ? tb + u : cnt - 1;
          const int64_t ci = __builtin_amdgcn_readlane(ch, tt);
          cv[u] = *reinterpret_cast<const f32x4d *>(E + ci * ldE + f0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (tb + u < cnt) {  // wave uniform
            // (s p) c for a tail member, (c p) o for a head member: k_distmult_fwd4's association with c in its slot
            const f32x4d q = __builtin_amdgcn_readlane(hd, tb + u) ? cv[u] * pv * ov : sv * pv * cv[u];
            float a = on ? (q.x + q.y) + (q.z + q.w) : 0.f;
            a = wave_sum(a);
            if (lane == tb + u) my = a;
          }
        }
      }
      const bool mine = lane < cnt;
      if (mine) scores[row] = my;
      if (LOSS == 0) {
        if (mine) {
          const float y = m == 0 ? 1.f : 0.f;
          const float k = 1.f + (w - 1.f) * y;
          acc += (1.f - y) * my + k * (log1pf(expf(-fabsf(my))) + fmaxf(-my, 0.f));
          g[row] = (k * (1.f / (1.f + expf(-my))) - w * y) * inv;
        }
      } else {
        if (m0 == 0) x0 = lane_f(my, 0);
        const float cm = wave_max(mine ? my : -INFINITY);
        const float nm = fmaxf(mx, cm);
        se = se * expf(mx - nm) + wave_sum(mine ? expf(my - nm) : 0.f);
        mx = nm;
      }
    }
    if (LOSS == 1) {
      const float lse = mx + logf(se);
      if (lane == 0) acc += lse - x0;
      for (int m0 = 0; m0 < members; m0 += kWave) {
        const int m = m0 + lane;
        if (m < members) {
          const int64_t row = m == 0 ? i : nb + m;
          // (a lane reads back the score it stored itself; a group of at most 64 still holds it)
          const float x = members <= kWave ? my : scores[row];
          g[row] = (expf(x - lse) - (m == 0 ? 1.f : 0.f)) * inv;
        }
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s_part[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < kWaves; ++k) t += s_part[k];
    partial[blockIdx.x] = t;
  }
}

// the block partials added in a fixed order: thread t takes partials t, t + 256, ..., then the threads in order
__global__ __launch_bounds__(kTB) void k_group_final(const float *__restrict__ partial, int nb, float inv,
                                                     float *__restrict__ loss) {
  __shared__ float s_sum[kTB];
  float acc = 0.f;
  for (int b = threadIdx.x; b < nb; b += kTB) acc += partial[b];
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int half = kTB / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = s_sum[0] * inv;
}

// ---- backward over the groups ---------------------------------------------------------------------------------------
// SCRATCH: rows_s / rows_p / rows_o [n, H] take the fact's three rows, keys / idx [n rate] the negatives' changed ends and
// their numbers (what the radix sort takes); nothing is added to dE / dRel here.  Otherwise everything is added by atomics.
template <bool SCRATCH>
__global__ __launch_bounds__(kTB) void k_group_bwd(const float *__restrict__ E, int64_t ldE,
                                                   const float *__restrict__ Rel, int64_t ldR, int H,
                                                   const int64_t *__restrict__ tr, int64_t n, int rate,
                                                   const float *__restrict__ g, const float *__restrict__ up,
                                                   float *__restrict__ rows_s, float *__restrict__ rows_p,
                                                   float *__restrict__ rows_o, int32_t *__restrict__ keys,
                                                   int32_t *__restrict__ idx, float *__restrict__ dE, int64_t lddE,
                                                   float *__restrict__ dRel, int64_t lddR) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const bool on = 4 * lane < H;
  const int f0 = on ? 4 * lane : 0;
  const float upv = *up;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wv; i < n; i += nwaves) {
    const int64_t si = tr[3 * i], pi = tr[3 * i + 1], oi = tr[3 * i + 2];
    const f32x4d sv = *reinterpret_cast<const f32x4d *>(E + si * ldE + f0);
    const f32x4d pv = *reinterpret_cast<const f32x4d *>(Rel + pi * ldR + f0);
    const f32x4d ov = *reinterpret_cast<const f32x4d *>(E + oi * ldE + f0);
    const float g0 = g[i] * upv;
    const f32x4d sp = sv * pv, po = pv * ov;
    f32x4d A = ov * g0, Hd = {0.f, 0.f, 0.f, 0.f};
    const int64_t k0 = i * (int64_t)rate;   // the group's first negative
    for (int j0 = 0; j0 < rate; j0 += kWave) {
      const int cnt = rate - j0 < kWave ? rate - j0 : kWave;
      const int64_t k = k0 + j0 + (lane < cnt ? lane : cnt - 1);
      const int32_t c0 = (int32_t)tr[3 * (n + k)], c2 = (int32_t)tr[3 * (n + k) + 2];
      const int hd = c0 != (int32_t)si;
      const int32_t ch = hd ? c0 : c2;
      const float gj = g[n + k] * upv;
      if (SCRATCH && lane < cnt) {
        keys[k] = ch;
        idx[k] = (int32_t)k;
      }
      for (int tb = 0; tb < cnt; tb += 4) {
        f32x4d cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four negatives' rows in flight
          const int tt = tb + u < cnt ? tb + u : cnt - 1;
          const int64_t ci = __builtin_amdgcn_readlane(ch, tt);
          cv[u] = *reinterpret_cast<const f32x4d *>(E + ci * ldE + f0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (tb + u < cnt) {  // wave uniform
            const bool h = __builtin_amdgcn_readlane(hd, tb + u) != 0;
            const float gt = lane_f(gj, tb + u);
            if (h) Hd += cv[u] * gt;
            else A += cv[u] * gt;
            if (!SCRATCH && on && gt != 0.f) {
              const int64_t ci = __builtin_amdgcn_readlane(ch, tb + u);
              row_atomic(dE + ci * lddE + f0, (h ? po : sp) * gt);
            }
          }
        }
      }
    }
    const f32x4d rs = pv * A, ro = pv * (sv * g0 + Hd), rp = sv * A + ov * Hd;
    if (on) {
      if (SCRATCH) {
        *reinterpret_cast<f32x4d *>(rows_s + i * H + f0) = rs;
        *reinterpret_cast<f32x4d *>(rows_p + i * H + f0) = rp;
        *reinterpret_cast<f32x4d *>(rows_o + i * H + f0) = ro;
      } else {
        row_atomic(dE + si * lddE + f0, rs);
        row_atomic(dE + oi * lddE + f0, ro);
        row_atomic(dRel + pi * lddR + f0, rp);
      }
    }
  }
}

// out[key(fact)] += rows[fact] along `order` (the facts sorted by column COL of their triples): a wave walks RUNS runs of
// kRun sorted facts, keeps the open sum in registers across them and adds it when the key changes (k_distmult_bwd_sorted4's
// walk, one stored row per fact instead of two gathered rows and a product).
template <int RUNS>
__global__ __launch_bounds__(kTB) void k_group_rows_sum(const float *__restrict__ rows, int H,
                                                        const int64_t *__restrict__ tr, int col,
                                                        const int64_t *__restrict__ order, int64_t n,
                                                        float *__restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w * RUNS * kRun >= n) return;
  const bool on = 4 * lane < H;
  const int f0 = on ? 4 * lane : 0;
  f32x4d acc = {0.f, 0.f, 0.f, 0.f};
  int32_t cur = -1;
  auto flush = [&]() {
    if (cur >= 0 && on) row_atomic(out + (int64_t)cur * ldo + f0, acc);
    acc = f32x4d{0.f, 0.f, 0.f, 0.f};
  };
#pragma unroll 1
  for (int run = 0; run < RUNS; ++run) {
    const int64_t t0 = (w * RUNS + run) * kRun;
    if (t0 >= n) break;
    const int cnt = (int)((n - t0 < kRun) ? n - t0 : kRun);
    const int32_t fi = (int32_t)order[t0 + (lane < cnt ? lane : cnt - 1)];
    const int32_t key = (int32_t)tr[3 * (int64_t)fi + col];
    for (int tb = 0; tb < cnt; tb += 4) {
      f32x4d a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // four facts' rows in flight
        const int tt = (tb + u < cnt) ? tb + u : cnt - 1;
        const int64_t r = __builtin_amdgcn_readlane(fi, tt);
        a[u] = *reinterpret_cast<const f32x4d *>(rows + r * H + f0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (tb + u < cnt) {  // wave uniform
          const int32_t kk = __builtin_amdgcn_readlane(key, tb + u);
          if (kk != cur) {
            flush();
            cur = kk;
          }
          acc += a[u];
        }
      }
    }
  }
  flush();
}

// dE[c] += g (s p) or g (p o) along the negatives sorted by changed end c (skeys, sidx: the radix sort's output), runs
// of equal c summed in registers.  Negative k belongs to fact k / rate and sits in row n + k.
__global__ __launch_bounds__(kTB) void k_group_bwd_negs(const float *__restrict__ E, int64_t ldE,
                                                        const float *__restrict__ Rel, int64_t ldR, int H,
                                                        const int64_t *__restrict__ tr, int64_t n, int rate,
                                                        const int32_t *__restrict__ skeys,
                                                        const int32_t *__restrict__ sidx, int64_t total,
                                                        const float *__restrict__ g, const float *__restrict__ up,
                                                        float *__restrict__ dE, int64_t lddE) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t t0 = w * kRun;
  if (t0 >= total) return;
  const bool on = 4 * lane < H;
  const int f0 = on ? 4 * lane : 0;
  const float upv = *up;
  const int cnt = (int)((total - t0 < kRun) ? total - t0 : kRun);
  const int64_t t = t0 + (lane < cnt ? lane : cnt - 1);
  const int32_t key = skeys[t];
  const int32_t k32 = sidx[t];
  const int64_t k = k32, i = k32 / rate;   // (n rate < 2^31: a 32-bit division)
  const int32_t s_ = (int32_t)tr[3 * i], p_ = (int32_t)tr[3 * i + 1], o_ = (int32_t)tr[3 * i + 2];
  const int32_t other = ((int32_t)tr[3 * (n + k)] != s_) ? o_ : s_;   // head negative: p o, tail negative: s p
  const float gk = g[n + k] * upv;
  f32x4d acc = {0.f, 0.f, 0.f, 0.f};
  int32_t cur = -1;
  auto flush = [&]() {
    if (cur >= 0 && on) row_atomic(dE + (int64_t)cur * lddE + f0, acc);
    acc = f32x4d{0.f, 0.f, 0.f, 0.f};
  };
  for (int tb = 0; tb < cnt; tb += 4) {
    f32x4d a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // four negatives' rows in flight
      const int tt = (tb + u < cnt) ? tb + u : cnt - 1;
      const int64_t pr = __builtin_amdgcn_readlane(p_, tt), er = __builtin_amdgcn_readlane(other, tt);
      a[u] = *reinterpret_cast<const f32x4d *>(Rel + pr * ldR + f0);
      b[u] = *reinterpret_cast<const f32x4d *>(E + er * ldE + f0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (tb + u < cnt) {  // wave uniform
        const int32_t kk = __builtin_amdgcn_readlane(key, tb + u);
        const float gt = lane_f(gk, tb + u);
        if (kk != cur) {
          flush();
          cur = kk;
        }
        acc += (a[u] * gt) * b[u];
      }
    }
  }
  flush();
}

inline int key_bits(int64_t bound) {
  int b = 1;
  while (b < 31 && (bound >> b) != 0) ++b;
  return b;
}
inline size_t sort_temp(int64_t total) {
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                           (int32_t *)nullptr, (int)total, 0, 31, (hipStream_t)0);
  return (tb + 255) / 256 * 256;
}
inline int64_t pad256(int64_t b) { return (b + 255) / 256 * 256; }
inline unsigned group_blocks(int64_t n) {
  const int64_t b = (n + kWaves - 1) / kWaves;
  return (unsigned)(b < kGroupBlocks ? b : kGroupBlocks);
}
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace mrgcn

extern "C" {

int32_t mrgcn_distmult_group_supported(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                       int64_t num_nodes, int64_t num_relations, int64_t n, int32_t rate) {
  using namespace mrgcn;
  const int64_t lim = (int64_t)1 << 31;
  return cfg(CFG_LP_VEC4) != 0 && H > 0 && H % 4 == 0 && H <= 256 && ldE % 4 == 0 && ldR % 4 == 0 && aligned16(E) &&
         aligned16(Rel) && num_nodes > 0 && num_relations > 0 && num_nodes < lim && num_relations < lim && n > 0 &&
         rate >= 1 && n * ((int64_t)rate + 1) < lim;
}

int64_t mrgcn_distmult_group_fwd_workspace(void) { return (int64_t)mrgcn::kGroupBlocks * (int64_t)sizeof(float); }

int mrgcn_distmult_group_fwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                 const int64_t *triples, int64_t n, int32_t rate, int32_t loss_kind, float pos_weight,
                                 float *scores, float *dscores, float *loss, void *workspace, int64_t workspace_bytes,
                                 void *stream) {
  using namespace mrgcn;
  MRGCN_REQUIRE(E && Rel && triples && scores && dscores && loss, "distmult_group_fwd: NULL argument");
  MRGCN_REQUIRE(mrgcn_distmult_group_supported(E, ldE, Rel, ldR, H, 1, 1, n, rate),
                "distmult_group_fwd: rows of whole 16-byte pieces (H % 4 == 0, H <= 256, aligned), n (1 + rate) < 2^31");
  MRGCN_REQUIRE(loss_kind == MRGCN_GROUP_LOSS_BCE || loss_kind == MRGCN_GROUP_LOSS_SOFTMAX, "distmult_group_fwd: loss kind");
  MRGCN_REQUIRE(workspace && workspace_bytes >= mrgcn_distmult_group_fwd_workspace(), "distmult_group_fwd: workspace");
  hipStream_t st = (hipStream_t)stream;
  float *partial = (float *)workspace;
  const unsigned blocks = group_blocks(n);
  if (loss_kind == MRGCN_GROUP_LOSS_BCE) {
    const float inv = (float)(1.0 / ((double)n * (1.0 + rate)));
    k_group_fwd<0><<<blocks, kTB, 0, st>>>(E, ldE, Rel, ldR, H, triples, n, rate, pos_weight, inv, scores, dscores,
                                           partial);
    k_group_final<<<1, kTB, 0, st>>>(partial, (int)blocks, inv, loss);
  } else {
    const float inv = (float)(1.0 / (double)n);
    k_group_fwd<1><<<blocks, kTB, 0, st>>>(E, ldE, Rel, ldR, H, triples, n, rate, 1.f, inv, scores, dscores, partial);
    k_group_final<<<1, kTB, 0, st>>>(partial, (int)blocks, inv, loss);
  }
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_distmult_group_bwd_workspace(int64_t n, int32_t rate, int32_t H) {
  using namespace mrgcn;
  if (n <= 0 || rate < 1 || H <= 0 || n * (int64_t)rate >= ((int64_t)1 << 31)) return -1;
  const int64_t total = n * (int64_t)rate;
  return 3 * pad256(n * H * 4) + 4 * pad256(total * 4) + (int64_t)sort_temp(total);
}

int mrgcn_distmult_group_bwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                 const int64_t *triples, int64_t n, int32_t rate, const float *dscores,
                                 const float *upstream, int64_t num_nodes, const int64_t *order_s,
                                 const int64_t *order_p, const int64_t *order_o, float *dE, int64_t lddE, float *dRel,
                                 int64_t lddR, void *workspace, int64_t workspace_bytes, void *stream) {
  using namespace mrgcn;
  MRGCN_REQUIRE(E && Rel && triples && dscores && upstream && dE && dRel, "distmult_group_bwd: NULL argument");
  MRGCN_REQUIRE(mrgcn_distmult_group_supported(E, ldE, Rel, ldR, H, num_nodes, 1, n, rate) && lddE % 4 == 0 &&
                    lddR % 4 == 0 && aligned16(dE) && aligned16(dRel),
                "distmult_group_bwd: rows of whole 16-byte pieces (H % 4 == 0, H <= 256, aligned), n (1 + rate) < 2^31");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = group_blocks(n);
  if (!order_s && !order_p && !order_o) {   // the atomic route
    k_group_bwd<false><<<blocks, kTB, 0, st>>>(E, ldE, Rel, ldR, H, triples, n, rate, dscores, upstream, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, dE, lddE, dRel, lddR);
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  MRGCN_REQUIRE(order_s && order_p && order_o, "distmult_group_bwd: the three orders of the facts, or none");
  MRGCN_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= mrgcn_distmult_group_bwd_workspace(n, rate, H),
                "distmult_group_bwd: workspace");
  const int64_t total = n * (int64_t)rate;
  char *w = (char *)workspace;
  const int64_t rb = pad256(n * H * 4), kb = pad256(total * 4);
  float *rows_s = (float *)w, *rows_p = (float *)(w + rb), *rows_o = (float *)(w + 2 * rb);
  int32_t *k_in = (int32_t *)(w + 3 * rb), *i_in = (int32_t *)(w + 3 * rb + kb), *k_out = (int32_t *)(w + 3 * rb + 2 * kb),
          *i_out = (int32_t *)(w + 3 * rb + 3 * kb);
  void *tmp = w + 3 * rb + 4 * kb;
  size_t tb = sort_temp(total);
  k_group_bwd<true><<<blocks, kTB, 0, st>>>(E, ldE, Rel, ldR, H, triples, n, rate, dscores, upstream, rows_s, rows_p,
                                            rows_o, k_in, i_in, nullptr, 0, nullptr, 0);
  const int64_t waves = (n + kRun - 1) / kRun;
  const unsigned ge = (unsigned)((waves + kWaves - 1) / kWaves);
  const unsigned gr = (unsigned)(((waves + kRelRuns - 1) / kRelRuns + kWaves - 1) / kWaves);
  k_group_rows_sum<1><<<ge, kTB, 0, st>>>(rows_s, H, triples, 0, order_s, n, dE, lddE);
  k_group_rows_sum<1><<<ge, kTB, 0, st>>>(rows_o, H, triples, 2, order_o, n, dE, lddE);
  k_group_rows_sum<kRelRuns><<<gr, kTB, 0, st>>>(rows_p, H, triples, 1, order_p, n, dRel, lddR);
  MRGCN_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, k_in, k_out, i_in, i_out, (int)total, 0,
                                                   key_bits(num_nodes - 1), st));
  const int64_t nwaves = (total + kRun - 1) / kRun;
  k_group_bwd_negs<<<(unsigned)((nwaves + kWaves - 1) / kWaves), kTB, 0, st>>>(E, ldE, Rel, ldR, H, triples, n, rate,
                                                                               k_out, i_out, total, dscores, upstream,
                                                                               dE, lddE);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
