// Literal encodings of a mini-batch on the device (reference mrgcn/data/batch.py:272-316 `mksubset`, :25-68 `pad_` /
// `to_dense_`, data/utils.py:109-152 the collate helpers).  Every encoding set is resident in HBM (uploaded once by
// DeviceEncodings); a batch is
//   mrgcn_literal_rows       one launch, one block per set: which members the batch's nodes carry (the set's node ->
//                            member map), their batch positions (ascending) and the members in the set's own order,
//                            the per-set count and the widths the padding rule needs
//   (the caller reads the [num_sets + 1, 4] stats back once and allocates)
//   mrgcn_literal_gather_rows fixed-width rows (X0, numeric sets, the node-id / seq_length columns): one launch over a
//                            table of byte-row gathers
//   mrgcn_literal_tokens     token members -> [k, L] int64, pad symbol beyond a member's length and for -1 tokens
//   mrgcn_literal_csr_dense  CSR members [C, w] -> [k, C, L] float32, every element stored once (zeros included)
// Integer / copy work bound by HBM: wave64, consecutive lanes on consecutive 16-byte pieces of the output, no atomics,
// the inner loops load through clamped indices and select afterwards instead of loading behind a branch.
#include "common.hpp"

using namespace mrgcn;

namespace {

constexpr int kRowsTB = 1024;   // one block per set: 16 waves scan the batch 1024 nodes at a time
constexpr int kTB = 256;
constexpr int kMaxJobs = 32;    // entries of a descriptor table passed by value (larger tables: several launches)

struct RowsTable {
  mrgcn_literal_set s[kMaxJobs];
};
struct GatherTable {
  mrgcn_literal_gather g[kMaxJobs];
};

__device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// Block-wide exclusive prefix of `flag` over the block's 1024 lanes; `total` = the block's count.
__device__ __forceinline__ int64_t block_prefix(bool flag, int64_t *wave_tot, int64_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int64_t below = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = __popcll(b);
  __syncthreads();
  int64_t off = 0, tot = 0;
  for (int w = 0; w < kRowsTB / 64; ++w) {
    const int64_t c = wave_tot[w];
    off += w < wave ? c : 0;
    tot += c;
  }
  __syncthreads();  // (wave_tot is rewritten by the next chunk)
  total = tot;
  return off + below;
}

__device__ __forceinline__ int64_t block_max(int64_t v, int64_t *red) {
  for (int o = 32; o > 0; o >>= 1) v = imax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t m = 0;
  for (int w = 0; w < kRowsTB / 64; ++w) m = imax(m, red[w]);
  __syncthreads();
  return m;
}

// blockIdx.x = set.  out_member / out_pos: [num_sets, n_nodes]; stats: [num_sets + 1, 4] = (count, max seq_length,
// max width, max extent) per set, then (node ids out of range, 0, 0, 0).
// Block 0 of the first launch also counts the node ids outside [0, num_nodes) (a launch with no set does only that).
__global__ void __launch_bounds__(kRowsTB) k_lit_rows(RowsTable tab, int32_t nt, int32_t first, int32_t total,
                                                      int64_t num_nodes, const int64_t *__restrict__ nodes,
                                                      int64_t n_nodes, int64_t *__restrict__ out_member,
                                                      int64_t *__restrict__ out_pos, int64_t *__restrict__ stats) {
  __shared__ int64_t wave_tot[kRowsTB / 64];
  const int set = blockIdx.x;
  if (first == 0 && set == 0) {
    int64_t bad = 0;
    for (int64_t p = threadIdx.x; p < n_nodes; p += kRowsTB) {
      const int64_t node = nodes[p];
      bad += (node < 0 || node >= num_nodes) ? 1 : 0;
    }
    bad = block_max(bad, wave_tot);  // (a lane's count; > 0 is all the caller needs)
    if (threadIdx.x == 0) stats[4 * (int64_t)total] = bad;
  }
  if (set >= nt) return;
  const int64_t slot = first + set;
  const mrgcn_literal_set d = tab.s[set];
  int64_t *mem = out_member + slot * n_nodes;
  int64_t *pos = out_pos + slot * n_nodes;
  int32_t *mflag = d.member_flags;  // (unordered sets only) one word per member
  if (!d.ordered) {
    for (int64_t m = threadIdx.x; m < d.members; m += kRowsTB) mflag[m] = 0;
    __syncthreads();
  }
  int64_t base = 0, mx_seq = 0, mx_w = 0, mx_e = 0;
  for (int64_t p0 = 0; p0 < n_nodes; p0 += kRowsTB) {
    const int64_t p = p0 + threadIdx.x;
    const bool in = p < n_nodes;
    const int64_t node = nodes[imin(p, n_nodes - 1)];
    const bool ok = node >= 0 && node < num_nodes;
    const int32_t m32 = d.member_of_node[imin(imax(node, 0), num_nodes - 1)];
    const bool hit = in && ok && m32 >= 0;
    const int64_t m = hit ? (int64_t)m32 : 0;
    // (members >= 1 whenever a node maps to one; the member arrays hold at least one entry)
    const int64_t sq = d.seq_lengths[m], w = d.widths ? d.widths[m] : 0, e = d.extents ? d.extents[m] : 0;
    mx_seq = imax(mx_seq, hit ? sq : 0);
    mx_w = imax(mx_w, hit ? w : 0);
    mx_e = imax(mx_e, hit ? e : 0);
    int64_t tot;
    const int64_t i = base + block_prefix(hit, wave_tot, tot);
    if (hit) {
      pos[i] = p;
      if (d.ordered) mem[i] = m;
      else mflag[m] = 1;
    }
    base += tot;
  }
  if (!d.ordered) {  // the selected members in the set's own order (np.in1d(nodes_idx, common))
    __syncthreads();
    int64_t b2 = 0;
    for (int64_t m0 = 0; m0 < d.members; m0 += kRowsTB) {
      const int64_t m = m0 + threadIdx.x;
      const bool hit = m < d.members && mflag[imin(m, d.members - 1)] != 0;
      int64_t tot;
      const int64_t i = b2 + block_prefix(hit, wave_tot, tot);
      if (hit) mem[i] = m;
      b2 += tot;
    }
  }
  mx_seq = block_max(mx_seq, wave_tot);
  mx_w = block_max(mx_w, wave_tot);
  mx_e = block_max(mx_e, wave_tot);
  if (threadIdx.x == 0) {
    int64_t *st = stats + 4 * slot;
    st[0] = base, st[1] = mx_seq, st[2] = mx_w, st[3] = mx_e;
  }
}

template <typename U>
__device__ __forceinline__ void gather_units(const mrgcn_literal_gather &g, int64_t tid, int64_t nthreads) {
  const int64_t upr = g.row_bytes / (int64_t)sizeof(U);
  const int64_t n = g.count * upr;
  const U *__restrict__ src = (const U *)g.src;
  U *__restrict__ dst = (U *)g.dst;
  for (int64_t u = tid; u < n; u += nthreads) {
    const int64_t i = u / upr, w = u - i * upr;
    const int64_t r = imin(imax(g.index[i], 0), g.src_rows - 1);
    dst[u] = src[r * upr + w];
  }
}

// blockIdx.y = gather; dst[i, :] = src[index[i], :] in pieces of `unit` bytes (16 where rows and pointers allow)
__global__ void __launch_bounds__(kTB) k_lit_gather(GatherTable tab) {
  const mrgcn_literal_gather g = tab.g[blockIdx.y];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  switch (g.unit) {
    case 16: gather_units<int4>(g, tid, nt); break;
    case 8: gather_units<int64_t>(g, tid, nt); break;
    case 4: gather_units<int32_t>(g, tid, nt); break;
    case 2: gather_units<int16_t>(g, tid, nt); break;
    default: gather_units<int8_t>(g, tid, nt); break;
  }
}

__device__ __forceinline__ int64_t token_at(const int64_t *__restrict__ tokens, const int64_t *__restrict__ offsets,
                                            const int64_t *__restrict__ members, int64_t e, int64_t L, int64_t pad) {
  const int64_t i = e / L, t = e - i * L;
  const int64_t m = members[i];
  const int64_t o = offsets[m], len = offsets[m + 1] - o;
  const int64_t v = tokens[o + (t < len ? t : 0)];  // (the token array holds one entry more than its members)
  return (t < len && v != -1) ? v : pad;
}

// out [k, L] int64, two elements (one 16-byte store) per thread step
__global__ void __launch_bounds__(kTB) k_lit_tokens(const int64_t *__restrict__ tokens,
                                                    const int64_t *__restrict__ offsets,
                                                    const int64_t *__restrict__ members, int64_t k, int64_t L,
                                                    int64_t pad, int64_t *__restrict__ out) {
  const int64_t n = k * L, npairs = (n + 1) / 2;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < npairs; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = 2 * j;
    const int64_t a = token_at(tokens, offsets, members, e, L, pad);
    if (e + 1 < n) {
      const int64_t b = token_at(tokens, offsets, members, e + 1, L, pad);
      *(longlong2 *)(out + e) = make_longlong2(a, b);
    } else {
      out[e] = a;
    }
  }
}

__device__ __forceinline__ float csr_at(const float *__restrict__ vals, const int32_t *__restrict__ cols,
                                        const int64_t *__restrict__ rowptr, const int64_t *__restrict__ members,
                                        int64_t e, int64_t C, int64_t L) {
  const int64_t row = e / L, t = e - row * L;
  const int64_t i = row / C, r = row - i * C;
  const int64_t *rp = rowptr + members[i] * (C + 1) + r;
  const int64_t rs = rp[0], re = rp[1];
  int64_t lo = rs, cnt = re - rs;  // lower_bound of t among the row's (sorted, distinct) columns
  while (cnt > 0) {
    const int64_t half = cnt >> 1;
    const bool less = cols[lo + half] < t;
    lo = less ? lo + half + 1 : lo;
    cnt = less ? cnt - half - 1 : half;
  }
  const int32_t c = cols[lo];  // (lo <= re: the column / value arrays hold one entry more than their entries)
  const float v = vals[lo];
  return (lo < re && c == t) ? v : 0.0f;
}

// out [k, C, L] float32, four elements (one 16-byte store) per thread step
__global__ void __launch_bounds__(kTB) k_lit_csr_dense(const float *__restrict__ vals,
                                                       const int32_t *__restrict__ cols,
                                                       const int64_t *__restrict__ rowptr,
                                                       const int64_t *__restrict__ members, int64_t k, int64_t C,
                                                       int64_t L, float *__restrict__ out) {
  const int64_t n = k * C * L, nq = (n + 3) / 4;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nq; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = 4 * j;
    if (e + 3 < n) {
      float4 q;
      q.x = csr_at(vals, cols, rowptr, members, e, C, L);
      q.y = csr_at(vals, cols, rowptr, members, e + 1, C, L);
      q.z = csr_at(vals, cols, rowptr, members, e + 2, C, L);
      q.w = csr_at(vals, cols, rowptr, members, e + 3, C, L);
      *(float4 *)(out + e) = q;
    } else {
      for (int64_t x = e; x < n; ++x) out[x] = csr_at(vals, cols, rowptr, members, x, C, L);
    }
  }
}

inline unsigned grid_for(int64_t items, int64_t cap = 8192) {
  int64_t g = (items + kTB - 1) / kTB;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

}  // namespace

extern "C" {

int mrgcn_literal_rows(const mrgcn_literal_set *sets, int32_t num_sets, int64_t num_nodes, const int64_t *nodes,
                       int64_t n_nodes, int64_t *out_member, int64_t *out_pos, int64_t *stats, void *stream) {
  MRGCN_REQUIRE(stats && (num_sets == 0 || sets), "NULL");
  MRGCN_REQUIRE(num_sets >= 0 && num_nodes > 0 && n_nodes >= 0 && num_nodes < ((int64_t)1 << 31), "sizes");
  MRGCN_REQUIRE(n_nodes == 0 || nodes, "nodes");
  hipStream_t s = (hipStream_t)stream;
  MRGCN_HIP_TRY(hipMemsetAsync(stats, 0, sizeof(int64_t) * 4 * ((size_t)num_sets + 1), s));
  if (n_nodes == 0) {  // nothing selected: counts and widths stay 0
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  MRGCN_REQUIRE(num_sets == 0 || (out_member && out_pos), "outputs");
  for (int32_t i = 0; i < num_sets; ++i) {
    const mrgcn_literal_set &d = sets[i];
    MRGCN_REQUIRE(d.member_of_node && d.seq_lengths && d.members >= 0, "set arrays");
    MRGCN_REQUIRE(d.ordered || d.members == 0 || d.member_flags, "member_flags of an unordered set");
  }
  int32_t i0 = 0;
  do {
    RowsTable tab;
    const int32_t nt = num_sets - i0 < kMaxJobs ? num_sets - i0 : kMaxJobs;
    for (int32_t j = 0; j < nt; ++j) tab.s[j] = sets[i0 + j];
    k_lit_rows<<<dim3((unsigned)(nt > 0 ? nt : 1)), kRowsTB, 0, s>>>(tab, nt, i0, num_sets, num_nodes, nodes,
                                                                       n_nodes, out_member, out_pos, stats);
    i0 += kMaxJobs;
  } while (i0 < num_sets);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_literal_gather_rows(const mrgcn_literal_gather *gathers, int32_t num_gathers, void *stream) {
  MRGCN_REQUIRE(num_gathers >= 0 && (num_gathers == 0 || gathers), "gathers");
  hipStream_t s = (hipStream_t)stream;
  int64_t most = 0;
  for (int32_t i = 0; i < num_gathers; ++i) {
    const mrgcn_literal_gather &g = gathers[i];
    MRGCN_REQUIRE(g.count >= 0 && g.row_bytes > 0 && g.src_rows >= 0, "gather sizes");
    MRGCN_REQUIRE(g.count == 0 || (g.src && g.dst && g.index && g.src_rows > 0), "gather pointers");
    MRGCN_REQUIRE(g.unit == 1 || g.unit == 2 || g.unit == 4 || g.unit == 8 || g.unit == 16, "unit");
    MRGCN_REQUIRE(g.row_bytes % g.unit == 0 && (uintptr_t)g.src % g.unit == 0 && (uintptr_t)g.dst % g.unit == 0,
                  "unit does not divide the rows / pointers");
    const int64_t units = g.count * (g.row_bytes / g.unit);
    most = units > most ? units : most;
  }
  if (most > 0) {
    for (int32_t i0 = 0; i0 < num_gathers; i0 += kMaxJobs) {
      GatherTable tab;
      const int32_t nt = num_gathers - i0 < kMaxJobs ? num_gathers - i0 : kMaxJobs;
      for (int32_t j = 0; j < nt; ++j) tab.g[j] = gathers[i0 + j];
      k_lit_gather<<<dim3(grid_for(most, 2048), (unsigned)nt), kTB, 0, s>>>(tab);
    }
  }
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_literal_tokens(const int64_t *tokens, const int64_t *offsets, const int64_t *members, int64_t k, int64_t L,
                         int64_t pad_symbol, int64_t *out, void *stream) {
  MRGCN_REQUIRE(k >= 0 && L > 0, "k / L");
  if (k == 0) return MRGCN_OK;
  MRGCN_REQUIRE(tokens && offsets && members && out, "NULL");
  MRGCN_REQUIRE((uintptr_t)out % 16 == 0, "out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  k_lit_tokens<<<grid_for((k * L + 1) / 2), kTB, 0, s>>>(tokens, offsets, members, k, L, pad_symbol, out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_literal_csr_dense(const float *values, const int32_t *columns, const int64_t *row_ptr,
                            const int64_t *members, int64_t k, int64_t C, int64_t L, float *out, void *stream) {
  MRGCN_REQUIRE(k >= 0 && C > 0 && L > 0, "k / C / L");
  if (k == 0) return MRGCN_OK;
  MRGCN_REQUIRE(values && columns && row_ptr && members && out, "NULL");
  MRGCN_REQUIRE((uintptr_t)out % 16 == 0, "out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  k_lit_csr_dense<<<grid_for((k * C * L + 3) / 4), kTB, 0, s>>>(values, columns, row_ptr, members, k, C, L, out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
