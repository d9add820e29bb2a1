/*
 * mrgcn_hip.h — C ABI of libmrgcn_hip.so (MI355X / gfx950).
 *
 * The reference (wxwilcke/mrgcn) has no FFI: its hot path leans on PyTorch ATen ops
 * called from Python.  Every entry point below replaces one such call site
 * (file:line relative to the reference tree) and is what a ctypes binding in the
 * reference's `mrgcn/layers/graph.py` would bind.
 *
 * Conventions
 *   - plain C, no C++ / torch types; every pointer is a DEVICE pointer unless the
 *     parameter name starts with `h_` (host);
 *   - every call returns MRGCN_OK (0) or an error code; the message is available
 *     from mrgcn_last_error() (thread local);
 *   - compute calls are asynchronous and stream ordered on `stream` (a hipStream_t,
 *     passed as void*; NULL = the null stream); they never allocate and never
 *     synchronise, so they may be captured into a hipGraph;
 *   - mrgcn_plan_create / _destroy / _export / mrgcn_event_* may allocate and
 *     synchronise;
 *   - buffers are caller owned; a plan owns its index copies, which are immutable after
 *     creation, and the SCRATCH of its products (partial sums of rows cut into chunks, the
 *     arrival counters of the in-kernel finalize), which every product launch writes.  The
 *     plan keeps one scratch set PER STREAM: products of one plan may be in flight on several
 *     streams (and be submitted from several threads) at once; products submitted to the same
 *     stream are ordered by it.  The first product a plan sees on a second, third, ... stream
 *     allocates that stream's set — the one exception to "compute calls never allocate": make
 *     that first call outside a stream capture (it fails with MRGCN_ERR_INVALID inside one).
 *     A gradient support (mrgcn_support_*) keeps ONE scratch set: one product in flight per support.
 */
#ifndef MRGCN_HIP_H
#define MRGCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRGCN_ABI_VERSION 5

enum mrgcn_status {
  MRGCN_OK = 0,
  MRGCN_ERR_INVALID = 1,     /* bad argument (shape, alignment, NULL, enum) */
  MRGCN_ERR_HIP = 2,         /* a HIP runtime call failed */
  MRGCN_ERR_UNSUPPORTED = 3, /* valid request this build cannot serve */
  MRGCN_ERR_RANGE = 4        /* an index in the input is out of range */
};

enum mrgcn_val_dtype { MRGCN_VAL_I8 = 0, MRGCN_VAL_F32 = 1 };

/* plan flags */
#define MRGCN_PLAN_PRUNE_ZEROS 1u /* drop entries whose value is exactly 0 (legal: they
                                     contribute nothing) */
#define MRGCN_PLAN_REPLICATE 2u   /* compact operand with REPLICAS: every entry of a column read by fewer than
                                     16 rows gets an operand row of its own, placed where its reader streams
                                     (see mrgcn_operand_replicate); hot columns keep one shared row */
#define MRGCN_PLAN_NO_REPLICATE 4u /* never replicate, whatever the default (env MRGCN_REPLICATE) says */
#define MRGCN_PLAN_LEAN 8u        /* a plan for a small, short-lived adjacency (the slices of a re-sampled mini-batch):
                                   * the COMPACT view keeps the rows in their own order and the operand in compact-column
                                   * order (no class-major ranks, no first-touch operand order, no replicas, one
                                   * transform order), its products run on the general row kernel.  Same results up to
                                   * the summation order inside a row; about half the build passes and host round trips. */

/* which sparse view of the plan a product runs on */
enum mrgcn_view {
  MRGCN_VIEW_LITERAL = 0, /* rows = output nodes, cols = r*N + j (the reference's layout) */
  MRGCN_VIEW_COMPACT = 1, /* rows = output nodes, cols = rows of the compact operand M
                             (compact column c is stored at row MPOS[c]) */
  MRGCN_VIEW_TRANSPOSED = 2 /* rows = touched columns in (j, r) order, cols = output nodes */
};

/* arrays retrievable with mrgcn_plan_export (all int32 unless noted) */
enum mrgcn_plan_array {
  MRGCN_ARR_ROWPTR = 0,   /* [num_rows+1]  CSR row pointers                           */
  MRGCN_ARR_LCOL = 1,     /* [nnz]         literal column r*N + j, sorted within a row */
  MRGCN_ARR_CCOL = 2,     /* [nnz]         compact column id                           */
  MRGCN_ARR_VAL = 3,      /* [nnz] float   values (A.float())                          */
  MRGCN_ARR_CPTR = 4,     /* [ncols+1]     CSC pointers over compact columns           */
  MRGCN_ARR_CROW = 5,     /* [nnz]         output row of each CSC entry                */
  MRGCN_ARR_CVAL = 6,     /* [nnz] float   value of each CSC entry                     */
  MRGCN_ARR_UREL = 7,     /* [ncols]       relation r of each compact column           */
  MRGCN_ARR_UNODE = 8,    /* [ncols]       source node j of each compact column        */
  MRGCN_ARR_NPTR = 9,     /* [num_nodes+1] compact-column range of each source node    */
  MRGCN_ARR_ROWIDX = 10,  /* [nnz]         output row of each CSR entry                */
  MRGCN_ARR_ULCOL = 11,   /* [ncols]       literal column r*N + j of each compact column */
  MRGCN_ARR_RPERM = 12,   /* [ncols]       compact ids sorted by (node band, relation, node) */
  MRGCN_ARR_RELPTR = 13,  /* [bands*R+1]   range of each (band, relation) group inside RPERM */
  MRGCN_ARR_MPOS = 14,    /* [ncols]       row of the compact operand M that holds column c */
  MRGCN_ARR_MCOL = 15,    /* [nnz]         operand row per entry of the COMPACT view, whose rows are walked
                                           CLASS-MAJOR (ranks, see ROWMAP / PTR3); a row's entries in
                                           rising operand row                                      */
  MRGCN_ARR_MVAL = 16,    /* [nnz] float   values in MCOL's entry order                */
  MRGCN_ARR_ROWMAP = 17,  /* [num_rows]    COMPACT view: rank -> output row.  Ranks = rows sorted by class
                                           (<= 8 entries, <= 32, more), row order inside a class      */
  MRGCN_ARR_PTR3 = 18     /* [num_rows+1]  COMPACT view: entry range of each rank inside MCOL / MVAL  */
};

typedef struct mrgcn_plan mrgcn_plan_t;

typedef struct mrgcn_plan_info {
  int64_t num_rows;      /* rows of A (output nodes)                     */
  int64_t num_nodes;     /* N: source nodes per relation block           */
  int64_t num_relations; /* R                                            */
  int64_t nnz;           /* stored entries after optional pruning        */
  int64_t ncols;         /* distinct non-empty columns (n_cols_touched)  */
  int64_t max_row_nnz;
  int64_t max_col_nnz;
  int64_t long_rows;     /* rows handled by the split-row path           */
  int64_t long_cols;
  int64_t device_bytes;  /* bytes of device memory the plan owns         */
  int64_t operand_rows;  /* rows of the compact operand M: ncols, or more with MRGCN_PLAN_REPLICATE */
  int64_t replicas;      /* operand rows that are copies (mrgcn_operand_replicate fills them)       */
} mrgcn_plan_info_t;

/* ---- library ---------------------------------------------------------------- */
int mrgcn_abi_version(void);
/* ---- configuration ----------------------------------------------------------------------------------------------
 * Every switch the library's launchers look at lives in ONE table (csrc/config.hip): initialised once, on the first
 * read, from the MRGCN_* environment variables of the same names (upper case, prefixed), changed afterwards only by
 * mrgcn_config_set.  No compute entry point reads the environment or caches a switch: a value set here takes effect
 * at the next call (plans keep what they were built with).  Names: mrgcn_config_name(0 .. count - 1), e.g.
 * "adam_list", "node_band"; the environment spelling ("MRGCN_ADAM_LIST") is accepted too. */
int32_t mrgcn_config_count(void);
const char *mrgcn_config_name(int32_t i);
const char *mrgcn_config_doc(int32_t i);
int mrgcn_config_get(const char *name, int64_t *value);
int mrgcn_config_set(const char *name, int64_t value);
const char *mrgcn_arch(void);       /* "gfx950" */
const char *mrgcn_last_error(void); /* message of the last failing call on this thread */

/* ---- graph plan ---------------------------------------------------------------
 * Built once per adjacency (A is static across epochs).  Input is exactly what the
 * reference hands to GraphConvolution.forward: the uncoalesced COO of
 * mrgcn/data/utils.py:165-170 (int64 indices 2 x nnz, given here as two rows) with
 * int8 values (mrgcn/data/batch.py:144-149) or float32 values.  Replaces the
 * per-call `A.float()` of mrgcn/layers/graph.py:75,:95 (done once here).
 * Requires num_relations*num_nodes < 2^31 and nnz < 2^31. */
int mrgcn_plan_create(mrgcn_plan_t **plan, int64_t num_rows, int64_t num_nodes,
                      int32_t num_relations, int64_t nnz, const int64_t *coo_rows,
                      const int64_t *coo_cols, const void *coo_vals, int32_t val_dtype,
                      uint32_t flags, void *stream);
/* The same plan straight from the CSR arrays the dataset archive holds (`A.npz`:
 * mrgcn/data/io/tarball.py:151-157; device int32 indptr / indices, float32 data), without the
 * host-side `.nonzero()` expansion to an int64 COO (data/utils.py:165-170).
 * boundary_cast_i8 != 0 applies the reference's int8 truncation of the values (batch.py:144-149). */
int mrgcn_plan_create_csr(mrgcn_plan_t **plan, int64_t num_rows, int64_t num_nodes,
                          int32_t num_relations, int64_t nnz, const int32_t *indptr,
                          const int32_t *indices, const float *data, int32_t boundary_cast_i8,
                          uint32_t flags, void *stream);
/* The same two constructors with a hint: the row sizes (bytes) of the compact operands M the plan's COMPACT
 * products will read — 4 * F for the packed rows of a layer of F outputs (F not a multiple of four), 4 * roundup(F, 4)
 * for padded rows, 2 * ld for bf16 rows.  The order of M keeps columns that several rows read off the positions
 * whose row would straddle a 128-byte line for any of these sizes (a re-read then costs one line, not two; AM
 * shape, F = 10: 158 -> 148 us with 40-byte rows).  The hint only permutes the operand rows (MPOS): products are
 * the same up to the order in which a row's terms are added.  At most four sizes are
 * used; without a hint (or through the plain constructors) 48-byte rows are assumed. */
int mrgcn_plan_create_hinted(mrgcn_plan_t **plan, int64_t num_rows, int64_t num_nodes,
                             int32_t num_relations, int64_t nnz, const int64_t *coo_rows,
                             const int64_t *coo_cols, const void *coo_vals, int32_t val_dtype,
                             uint32_t flags, const int32_t *operand_row_bytes, int32_t n_row_bytes,
                             void *stream);
int mrgcn_plan_create_csr_hinted(mrgcn_plan_t **plan, int64_t num_rows, int64_t num_nodes,
                                 int32_t num_relations, int64_t nnz, const int32_t *indptr,
                                 const int32_t *indices, const float *data, int32_t boundary_cast_i8,
                                 uint32_t flags, const int32_t *operand_row_bytes, int32_t n_row_bytes,
                                 void *stream);
/* A VALUE OVERLAY of `parent`: a second plan that BORROWS every index array, descriptor and order of the parent and OWNS
 * fresh copies of the values (VAL, MVAL, CVAL; one array on a lean plan, aliased as the parent's is) and its own product
 * scratch.  Every entry point that takes a plan runs unchanged on it and reads its values; the parent's arrays are never
 * written.  mrgcn_edge_dropout_draw_f32 rewrites the overlay's values.  The parent must outlive the overlay; destroying
 * the overlay (mrgcn_plan_destroy / _destroy_after) frees only what it owns.  Not inside a stream capture (it allocates,
 * and the first overlay of a plan builds the per-entry coordinates the draw reads).  Refused: an overlay of an overlay,
 * a plan with operand replicas; mrgcn_support_create* refuse an overlay (a support copies values out of its plan). */
int mrgcn_plan_create_overlay(const mrgcn_plan_t *parent, mrgcn_plan_t **child, void *stream);
int mrgcn_plan_is_overlay(const mrgcn_plan_t *plan);
int mrgcn_plan_destroy(mrgcn_plan_t *plan);
/* mrgcn_plan_destroy waits for ALL work in flight on the plan's device.  _destroy_after waits only for `event` (a
 * hipEvent_t the caller recorded behind the last work that uses the plan, on whichever stream; NULL: nothing used it)
 * and for the plan's own build: other streams keep running — for callers that drop the plans of finished mini-batch
 * steps while the next batch is being built (mrgcn_amd.data.batch.BatchPrefetcher). */
int mrgcn_plan_destroy_after(mrgcn_plan_t *plan, void *event);
int mrgcn_plan_info(const mrgcn_plan_t *plan, mrgcn_plan_info_t *h_info);
/* copies one plan array to HOST memory (tests: index parity is bit-exact) */
int mrgcn_plan_export(const mrgcn_plan_t *plan, int32_t which, void *h_dst, int64_t capacity_bytes);
/* device pointer + element count of one plan array (owned by the plan, read only) */
int mrgcn_plan_array(const mrgcn_plan_t *plan, int32_t which, const void **d_ptr, int64_t *h_count);

/* ---- sparse x dense ------------------------------------------------------------
 * Y[i, 0:F] = sum_e val[e] * D[col[e], 0:F]  (+ bias[0:F])  (optionally ReLU'd)
 * over the entries e of row i of the chosen view.
 *   view LITERAL    : replaces torch.mm(A.float(), W_I / FW_F), graph.py:75,:95
 *   view COMPACT    : same product on a dense operand that holds only touched rows
 *   view TRANSPOSED : dM[c] = sum val * dY[row]; the autograd of the above
 *                     (SparseAddmmBackward: dDense = A^T dY)
 * `out_index` (nullable, int32 [rows of view]) redirects output row i to
 * Y[out_index[i]] — used to scatter compact rows into the literal (R*N) x F gradient.
 * D, Y row-major with leading dimensions ldD, ldY (in floats).
 * `relu` is a flag word: MRGCN_SPMM_RELU (= 1, what callers always passed for "apply ReLU") and
 * MRGCN_SPMM_PAD_WRITABLE: columns F .. min(ldY, 4*ceil(F/4)) - 1 of every row of Y belong to the
 * caller's buffer and may be overwritten with zeros.  Rows of F = 10 / 11 in a buffer of ldY = 12 then
 * leave as three 16-byte stores and consecutive rows complete their 128-byte lines (COMPACT view,
 * F <= 16: the product runs 5 % faster); without the flag nothing outside [0, F) is touched. */
#define MRGCN_SPMM_RELU 1
#define MRGCN_SPMM_PAD_WRITABLE 2
/* COMPACT view, F <= 16: rows cut into several chunks are by default finished inside the product kernel by the
 * wave that delivers the row's last partial sum (fixed summation order: results are bitwise reproducible and equal
 * to the two-pass form's).  This flag asks for the two-pass form: a second launch adds the partial sums. */
#define MRGCN_SPMM_TWO_PASS 4
int mrgcn_spmm_f32(const mrgcn_plan_t *plan, int32_t view, const float *D, int64_t ldD,
                   int32_t F, float *Y, int64_t ldY, const float *bias, int32_t relu,
                   const int32_t *out_index, void *stream);
/* the same product with the dense operand D stored in bf16 (raw uint16_t, ldD in elements),
 * fp32 values, fp32 accumulation and fp32 Y — the {bf16 dense} half of the SpMM set
 * (the reference has no bf16, tolerance is stated where it is used) */
int mrgcn_spmm_bf16(const mrgcn_plan_t *plan, int32_t view, const uint16_t *D, int64_t ldD,
                    int32_t F, float *Y, int64_t ldY, const float *bias, int32_t relu,
                    const int32_t *out_index, void *stream);

/* Fills the replicas of a compact operand built on a plan with MRGCN_PLAN_REPLICATE: the producers below
 * write each compact column once (row MPOS[c]); this call copies the row of every column read by 2..15
 * output rows to the operand rows of its other readers, so that the forward product reads M front to back
 * instead of fetching one 128-byte line per re-read 40-byte row.  `row_bytes` = leading dimension in bytes
 * (multiple of 4).  A no-op on a plan without replicas.  (AM shape: product 202 -> 189 us, the copies 79 us:
 * not the default.) */
int mrgcn_operand_replicate(const mrgcn_plan_t *plan, void *M, int64_t row_bytes, void *stream);

/* ---- compact dense operand: forward -----------------------------------------------
 * M is [ncols, ldM] row-major with one row per touched column c = (node j_c, relation
 * r_c); column c lives at row MPOS[c] (hot columns first, then single-use columns in the
 * order of the output row that reads them).  Producers write the WHOLE padded row (zeros in
 * [F, ldM)) and never read M: the one scattered pass of the forward is write-only.
 * `addend` (nullable, [ncols, ldA] in plain compact order) is added on the fly — it carries
 * the other term of the layer.  The backward operand dM (output of the TRANSPOSED view) is in
 * plain compact order.
 *
 * basis mix — replaces einsum('rb,bij->rij', weight_I_comp, weight_I.view(B,N,out)) and the
 * view to (R*N, out) of graph.py:69-72, restricted to the rows the product will read:
 *     M[MPOS[c], 0:F] = addend[c, 0:F] + sum_b comp[r_c, b] * V[j_c, b, 0:F]
 *     comp: [R, B];  V: NODE-MAJOR basis table [N][B][F] — the B rows of a node are one contiguous
 *     block of B*F floats.  It is the [B][N][F] -> [N][B][F] transpose of the reference's weight_I
 *     (graph.py:50-51: (B*N, out), row b*N + j): mrgcn_amd.layers.graph.GraphConvolution keeps its
 *     parameter in this layout and converts in its state-dict hooks. */
int mrgcn_basis_mix_fwd_f32(const mrgcn_plan_t *plan, const float *V, const float *comp, int32_t B,
                            int32_t F, const float *addend, int64_t ldA, float *M, int64_t ldM,
                            void *stream);
/* no-bases input term (graph.py:67-68): M[MPOS[c], 0:F] = addend[c, 0:F] + W[r_c*N + j_c, 0:F] */
int mrgcn_gather_rows_f32(const mrgcn_plan_t *plan, const float *W, int32_t F, const float *addend,
                          int64_t ldA, float *M, int64_t ldM, void *stream);
/* Basis contraction of weight_F (graph.py:83-85): W[r, :] = sum_b comp[r, b] * V[b, :] with V = weight_F viewed as
 * (B, X = in * out), W = (R, X) — and its backward: dV[b, :] = sum_r comp[r, b] * dW[r, :], dcomp[r, b] =
 * <dW[r, :], V[b, :]> (either output nullable).  One launch each; fixed summation order. */
int mrgcn_basis_contract_f32(const float *comp, const float *V, int32_t R, int32_t B, int64_t X, float *W,
                             void *stream);
int mrgcn_basis_contract_bwd_f32(const float *comp, const float *V, const float *dW, int32_t R, int32_t B, int64_t X,
                                 float *dcomp, float *dV, void *stream);

/* relation transform — replaces einsum('ij,bjk->bik', X, W_F) + reshape of graph.py:93-94,
 * restricted to touched columns (f32 MFMA 16x16x4 when K <= 256 and F <= 64):
 *     Out[o(c), 0:F] = X[j_c, 0:K] . W[r_c, 0:K, 0:F]          X: [N, ldX], W: [R, K, F]
 * o(c) = c (plain compact order, e.g. to serve as `addend`) or MPOS[c] (`operand_order` != 0).  Every kernel form
 * writes the whole padded row, zeros in [F, ldOut), for any F <= ldOut <= INT32_MAX, and nothing else.  F <= 64: a
 * wider transform is an error (MRGCN_ERR_INVALID) — tile the feature dimension: one call per slice of W's columns,
 * each with an output of its own. */
int mrgcn_rel_transform_fwd_f32(const mrgcn_plan_t *plan, const float *X, int64_t ldX, int32_t K,
                                const float *W, int32_t F, float *Out, int64_t ldOut,
                                int32_t operand_order, void *stream);
/* bf16-operand forms of the three forward operand builders: M / Out is bf16 (raw uint16_t,
 * leading dimension in elements), every input stays fp32 and every sum is fp32, one rounding
 * at the store.  basis_mix: B <= 64. */
int mrgcn_basis_mix_fwd_bf16(const mrgcn_plan_t *plan, const float *V, const float *comp, int32_t B,
                             int32_t F, const float *addend, int64_t ldA, uint16_t *M, int64_t ldM,
                             void *stream);
int mrgcn_gather_rows_bf16(const mrgcn_plan_t *plan, const float *W, int32_t F, const float *addend,
                           int64_t ldA, uint16_t *M, int64_t ldM, void *stream);
int mrgcn_rel_transform_fwd_bf16(const mrgcn_plan_t *plan, const float *X, int64_t ldX, int32_t K,
                                 const float *W, int32_t F, uint16_t *Out, int64_t ldOut,
                                 int32_t operand_order, void *stream);

/* ---- the bf16 pipeline (BASELINE config 3; SURVEY 8d "dense operands in bf16 with fp32 accumulation") ---------
 * The reference computes graph.py:93-95 in fp32 and has no reduced precision anywhere; in this mode every ACTIVATION
 * the layer reads or writes in bulk is stored in bf16 — the layer input X (rows of ldX elements, ldX % 8 == 0, zeros
 * past K), the feature term's rows (`addend`), the compact operand M — while parameters, every accumulation, the
 * layer output Y and the whole backward's sums stay fp32.
 *   mrgcn_cast_rows_bf16          dst[row, 0:ldDst] = [ bf16(src[row, 0:K]) | 0 ]  (round to nearest even)
 *   mrgcn_rel_transform_fwd_xbf16 mrgcn_rel_transform_fwd_f32 on bf16 input rows, v_mfma_f32_16x16x32_bf16 (W is
 *                                 rounded to bf16 as it is staged): K <= 256, F <= ldOut <= 16; Out fp32 or bf16
 *   mrgcn_basis_mix_fwd_abf16     mrgcn_basis_mix_fwd_f32 / _bf16 with the addend rows in bf16 (ldA elements)
 *   mrgcn_support_rel_transform_bwd_xbf16   (below, with the gradient supports) */
int mrgcn_cast_rows_bf16(const float *src, int64_t ldSrc, int64_t rows, int32_t K, uint16_t *dst, int64_t ldDst,
                         void *stream);
int32_t mrgcn_rel_transform_xbf16_supported(const mrgcn_plan_t *plan, int32_t K, int32_t F, int64_t ldX,
                                            int64_t ldOut);
int mrgcn_rel_transform_fwd_xbf16(const mrgcn_plan_t *plan, const uint16_t *X, int64_t ldX, int32_t K,
                                  const float *W, int32_t F, void *Out, int64_t ldOut, int32_t operand_order,
                                  int32_t out_bf16, void *stream);
int mrgcn_basis_mix_fwd_abf16(const mrgcn_plan_t *plan, const float *V, const float *comp, int32_t B, int32_t F,
                              const uint16_t *addend, int64_t ldA, void *M, int64_t ldM, int32_t out_bf16,
                              void *stream);


/* ---- compact dense operand: backward (autograd of graph.py:69-72, :93-94) -------------
 *     dV[j, b, :]  = sum_{c in node j} comp[r_c, b] * dM[c, :]          (node-major, like V)
 *     dcomp[r, b]  = sum_{c: r_c = r} <dM[c, :], V[j_c, b, :]>           (zeroed inside)
 * col_live (nullable): the liveness byte per compact column that mrgcn_spmm_transposed_live_f32 wrote;
 *     rows of dM flagged 0 are never read — they may be unwritten — and where a kernel has to read every
 *     row they are overwritten with zeros first (hence the non-const dM).  NULL: every column counts.
 * node_cur (nullable): ROW-SPARSE gradient.  A node without a live compact column has a zero gradient
 *     block; with node_cur given such blocks of dV are left UNWRITTEN (and their V blocks unread) and
 *     node_cur[j] = 1 / 0 says which nodes were written — only mrgcn_adam_step_rows_f32 may consume such a
 *     gradient.  NULL: every block of dV is written (zeros where there is no gradient).
 * dV_sumsq (nullable): *dV_sumsq += ||dV||^2 (device double), for the global clip norm.
 * dV may be NULL when node_cur and dV_sumsq are given (norm-only pass in front of mrgcn_adam_step_rows_fused_f32). */
int mrgcn_basis_mix_bwd_f32(const mrgcn_plan_t *plan, float *dM, int64_t ldM, const uint8_t *col_live,
                            const float *V, const float *comp, int32_t B, int32_t F, float *dV,
                            uint8_t *node_cur, float *dcomp, double *dV_sumsq, void *stream);

/* The same two gradients for a WIDE featureless layer with few bases (B <= 4, 16 < F <= 256, F % 4 == 0: the
 * link-prediction encoder of configs/fb15k-237.toml, N x 200 with 2 bases) straight from the layer's output gradient,
 * without the compact operand dM (one 4 F-byte row per touched column, written once and read twice by the pair
 * mrgcn_spmm_f32(TRANSPOSED) + mrgcn_basis_mix_bwd_f32):
 *     dV[j][b][:] = sum_{entries e = (i, (j, r), a)} comp[r][b] * a * dY[i][:]     (every block written)
 *     dcomp[r][b] = sum_{entries of relation r} a * <dY[i][:], V[j][b][:]>
 * over the plan's CSC entries, which are contiguous per source node.  The caller cuts the nodes' entry ranges into
 * UNITS of a few hundred entries (unit_node / unit_beg / unit_end, entry numbers of the CSC order; unit_multi[u] != 0
 * when its node has several units: those add with float atomics, the others store) and provides `erel`, the relation
 * of every CSC entry (mrgcn_plan_entry_relations, once per plan).  dY: [num_rows, ldY], 16-byte aligned rows. */
int mrgcn_plan_entry_relations(const mrgcn_plan_t *plan, int32_t *erel, void *stream);
int32_t mrgcn_wide_input_bwd_supported(const mrgcn_plan_t *plan, int32_t B, int32_t F);
int mrgcn_wide_input_bwd_f32(const mrgcn_plan_t *plan, const int32_t *erel, const int32_t *unit_node,
                             const int32_t *unit_beg, const int32_t *unit_end, const uint8_t *unit_multi,
                             int64_t n_units, const float *dY, int64_t ldY, const float *V, const float *comp,
                             int32_t B, int32_t F, float *dV, float *dcomp, void *stream);
/* The same, BITWISE REPRODUCIBLE (no float atomic): a unit of a node with several units writes its partial sums to
 * slot unit_slot[u] of the workspace (-1: the node's only unit, stored straight into dV) and a second launch adds a
 * node's slots in unit order (hub_node / hub_ptr: the nodes with several units and their slot ranges); dcomp is summed
 * per wave, per block and over the blocks in fixed orders.  What lets the units be small (64 entries: hub nodes stop
 * being the tail of the launch) without the atomics' reordering of cancelling sums. */
int64_t mrgcn_wide_input_bwd_det_workspace(const mrgcn_plan_t *plan, int64_t n_slots, int32_t B, int32_t F);
int mrgcn_wide_input_bwd_det_f32(const mrgcn_plan_t *plan, const int32_t *erel, const int32_t *unit_node,
                                 const int32_t *unit_beg, const int32_t *unit_end, const int32_t *unit_slot,
                                 int64_t n_units, const int32_t *hub_node, const int32_t *hub_ptr, int64_t n_hubs,
                                 int64_t n_slots, const float *dY, int64_t ldY, const float *V, const float *comp,
                                 int32_t B, int32_t F, float *dV, float *dcomp, float *workspace,
                                 int64_t workspace_floats, void *stream);

/*     dX[j, 0:K]  = sum_{c in node j} W[r_c] . dM[c, :]     (nullable; every row written)
 *     dW[r, :, :] = sum_{c: r_c = r} X[j_c, :]^T dM[c, :]    (nullable; zeroed inside)
 * `workspace` (nullable; size from mrgcn_rel_transform_bwd_workspace) lets dX run on the matrix
 * cores (per-column products, then a segmented sum per node) and dW reduce per-chunk partial
 * slabs instead of contended global atomics.                                              */
int64_t mrgcn_rel_transform_bwd_workspace(const mrgcn_plan_t *plan, int32_t K, int32_t F,
                                          int32_t need_dX, int32_t need_dW); /* floats */
int mrgcn_rel_transform_bwd_f32(const mrgcn_plan_t *plan, const float *dM, int64_t ldM,
                                const float *X, int64_t ldX, int32_t K, const float *W, int32_t F,
                                float *dX, int64_t lddX, float *dW, float *workspace,
                                int64_t workspace_floats, void *stream);
/* Same with a liveness byte per compact column (`col_live[c]` = 0: row c of dM is all zeros;
 * nullable = every column live).  In a semi-supervised epoch only the columns that feed a row
 * within reach of a labelled node carry gradient (autograd of graph.py:93-95 multiplies the
 * zeros like everything else); dead columns add exact zeros to dW and dX and are skipped.  Results
 * equal mrgcn_rel_transform_bwd_f32's.  Rows of dM flagged 0 are never read (they may be unwritten);
 * where a fallback kernel has to read every row they are overwritten with zeros first.  `col_live` comes from mrgcn_spmm_transposed_live_f32
 * (or mrgcn_rows_nonzero_f32(dM)). */
int mrgcn_rel_transform_bwd_live_f32(const mrgcn_plan_t *plan, float *dM, int64_t ldM,
                                     const uint8_t *col_live, const float *X, int64_t ldX,
                                     int32_t K, const float *W, int32_t F, float *dX, int64_t lddX,
                                     float *dW, float *workspace, int64_t workspace_floats,
                                     void *stream);
/* mrgcn_rel_transform_bwd_live_f32 with the layer-input gradient finished in the same pass (K <= 16, matrix-core
 * path: ask mrgcn_rel_transform_bwd_masked_supported): `relu_mask_from_x` != 0 multiplies dX by the mask X > 0 — X
 * is then the output of a ReLU (a hidden layer's input, rgcn.py:86-87), and X > 0 is that ReLU's own mask, so the
 * layer that produced X has nothing left to mask; `row_live_out` (nullable, one byte per node) receives "this row
 * of dX holds anything but zeros" — the flags mrgcn_spmm_transposed_live_flagged_f32 takes; `node_live` (nullable;
 * with `col_live`): the per-node flags that call wrote next to `col_live`, read instead of every node's column flags. */
int32_t mrgcn_rel_transform_bwd_masked_supported(const mrgcn_plan_t *plan, int32_t K, int32_t F,
                                                 int64_t workspace_floats);
int mrgcn_rel_transform_bwd_masked_f32(const mrgcn_plan_t *plan, float *dM, int64_t ldM, const uint8_t *col_live,
                                       const float *X, int64_t ldX, int32_t K, const float *W, int32_t F,
                                       float *dX, int64_t lddX, float *dW, float *workspace,
                                       int64_t workspace_floats, int32_t relu_mask_from_x,
                                       uint8_t *row_live_out, const uint8_t *node_live, void *stream);
/* Y[c, 0:F] = sum_i A'[i, c] * D[i, 0:F] — mrgcn_spmm_f32 on MRGCN_VIEW_TRANSPOSED (the autograd
 * of torch.mm(A, .), graph.py:75,:95) for an operand whose rows are mostly zeros, as the output
 * gradient of a layer is when few nodes are labelled: rows of D that hold only zeros are not
 * gathered (their products are zeros; rows of up to 32 entries are bitwise those of mrgcn_spmm_f32).
 * `scratch` (mrgcn_spmm_transposed_live_scratch(plan) bytes, 16-byte aligned) holds the liveness
 * of the rows of D; `col_live` ([ncols] bytes) receives 0 for rows of Y that are certainly all
 * zeros, 1 otherwise — the input of mrgcn_rel_transform_bwd_live_f32.  `live_rows` (nullable,
 * device) receives the number of rows of D that are not all zeros (-1 when F > 16, where the
 * general product runs): with more than about a quarter of the rows live the general
 * mrgcn_spmm_f32 is the faster call (AM shape: 211 us at 0.3 % live rows, 467 us general,
 * 860 us with every row live), so callers keep the last count and choose.
 * `write_dead_rows` = 0 leaves the rows of Y whose flag is 0 UNWRITTEN (their zeros are 90 % of this
 * call's stores): only for consumers that take `col_live` — mrgcn_basis_mix_bwd_f32 and
 * mrgcn_rel_transform_bwd_live_f32. */
int64_t mrgcn_spmm_transposed_live_scratch(const mrgcn_plan_t *plan); /* bytes */
int mrgcn_spmm_transposed_live_f32(const mrgcn_plan_t *plan, const float *D, int64_t ldD, int32_t F,
                                   float *Y, int64_t ldY, uint8_t *scratch, uint8_t *col_live,
                                   int32_t *live_rows, int32_t write_dead_rows, void *stream);
/* The same with the row flags of D given (`row_flags`, nullable: one byte per row of D, 0 = the row is all
 * zeros — written by the producer of D, mrgcn_rel_transform_bwd_masked_f32): D is not scanned for them.
 * `node_live` (nullable, one byte per source node) receives "this node has a live column" — what
 * mrgcn_rel_transform_bwd_masked_f32 takes to skip the nodes without any. */
int mrgcn_spmm_transposed_live_flagged_f32(const mrgcn_plan_t *plan, const float *D, int64_t ldD, int32_t F,
                                           float *Y, int64_t ldY, uint8_t *scratch, uint8_t *col_live,
                                           int32_t *live_rows, int32_t write_dead_rows,
                                           const uint8_t *row_flags, uint8_t *node_live, void *stream);
/* flags[i] = 1 when X[i, 0:F] holds anything but (+-)0 — NaN counts — else 0. */
int mrgcn_rows_nonzero_f32(const float *X, int64_t ld, int32_t F, int64_t nrows, uint8_t *flags,
                           void *stream);

/* ---- gradient support: the backward of a semi-supervised epoch on dense index spaces -------------------------
 * The reference's autograd multiplies the zeros of a layer's output gradient like everything else
 * (node_classification.py:439-444 takes the loss over the labelled rows Y_hat[idx] only; graph.py:75,:95 then run
 * dense).  Which rows of that gradient CAN hold anything follows from the label set and the graph alone: the
 * labelled rows at the last layer, and below it the source nodes of the columns those rows read.  A support fixes
 * that knowledge once per (plan, row set): `row_flags` (device, one byte per output row: 1 = the row of dY may be
 * non-zero) -> the LIVE compact columns (touched by a flagged row), numbered 0..L-1 in (node, relation) order, the
 * entries of those columns that sit in flagged rows, the nodes that own a live column (NODE_FLAGS: the row set of
 * the layer below) and the live columns in the plan's relation-major orders.  The calls below then take dM and
 * every per-column product as [L, ld] arrays indexed by live number: nothing is marked, scanned or skipped per epoch.
 * Results equal those of the plan-level calls with the matching liveness flags (dead entries add exact zeros).
 * A support is immutable after creation and refers to its plan (destroy the support first).  create / destroy
 * allocate and synchronise; the compute calls are stream ordered and capturable. */
typedef struct mrgcn_support mrgcn_support_t;
typedef struct mrgcn_support_info {
  int64_t live_cols;    /* L                                             */
  int64_t live_entries; /* entries of live columns inside flagged rows   */
  int64_t live_nodes;   /* nodes that own a live column                  */
  int64_t device_bytes;
  int64_t chunks_wide, chunks_narrow; /* relation-major chunks of the two transform orders */
  int64_t flagged_rows; /* NR (MRGCN_SUPPORT_FORWARD supports; -1 otherwise) */
} mrgcn_support_info_t;
enum mrgcn_support_array_id {
  MRGCN_SUP_COL_FLAGS = 0,  /* uint8 [ncols]     1 = live                                   */
  MRGCN_SUP_NODE_FLAGS = 1, /* uint8 [num_nodes] 1 = owns a live column                     */
  MRGCN_SUP_LCOL = 2,       /* int32 [L]         compact column of each live column, rising  */
  MRGCN_SUP_LREL = 3,       /* int32 [L]         its relation                                */
  MRGCN_SUP_NLPTR = 4,      /* int32 [num_nodes+1] node -> range of live numbers             */
  MRGCN_SUP_LPTR = 5,       /* int32 [L+1]       entry range of each live column             */
  MRGCN_SUP_LROW = 6,       /* int32 [E]         output row of each kept entry               */
  MRGCN_SUP_LVAL = 7,       /* float [E]         its value                                   */
  MRGCN_SUP_LNODE = 8,      /* int32 [live_nodes] nodes that own a live column, rising       */
  MRGCN_SUP_LPERM = 9,      /* int32 [L]         live numbers in (node band, relation, node) order */
  /* MRGCN_SUPPORT_FORWARD supports only (count 0 otherwise): */
  MRGCN_SUP_FROW = 10,      /* int32 [NR]        flagged rows, rising                        */
  MRGCN_SUP_FPTR = 11,      /* int32 [NR+1]      entry range of each flagged row             */
  MRGCN_SUP_FCOL = 12,      /* int32 [E]         live number of each entry's column (the plan's row order) */
  MRGCN_SUP_FVAL = 13,      /* float [E]         its stored value                            */
  MRGCN_SUP_LNODE_ORD = 14, /* int32 [L]         rank of the live column's node in LNODE     */
  MRGCN_SUP_ROWRANK = 15,   /* int32 [num_rows]  rank in FROW, -1 for rows outside the set   */
  /* the (row, relation) pairs, once mrgcn_support_pair_sums_info has built them (count 0 before): */
  MRGCN_SUP_PAIR_PTR = 16,     /* int32 [P+1]    entry range of each pair in the pair order        */
  MRGCN_SUP_PAIR_ROW = 17,     /* int32 [P]      output row of each pair                           */
  MRGCN_SUP_REL_PAIR_PTR = 18, /* int32 [R+1]    pair range of each relation                       */
  MRGCN_SUP_PAIR_NODE = 19,    /* int32 [E]      source node of each entry in the pair order       */
  MRGCN_SUP_PAIR_VAL = 20,     /* float [E]      its stored value                                  */
  MRGCN_SUP_PAIR_CHUNK_PTR = 21 /* int32 [R+1]   chunk range of each relation (mrgcn_support_dw_pairs_f32) */
};
int mrgcn_support_create(mrgcn_support_t **support, const mrgcn_plan_t *plan, const uint8_t *row_flags,
                         void *stream);
/* flags: MRGCN_SUPPORT_FORWARD also keeps the flagged rows as a CSR over (flagged row, live column), the ranks of
 * rows and nodes and the relation-major orders by live-node rank: what the masked-pass calls below need. */
#define MRGCN_SUPPORT_FORWARD 1u
int mrgcn_support_create_ex(mrgcn_support_t **support, const mrgcn_plan_t *plan, const uint8_t *row_flags,
                            uint32_t flags, void *stream);
/* n supports at once: supports[0] on row_flags, supports[i+1] on NODE_FLAGS of supports[i] (the samples of the n layers
 * of a mini-batch, batch.py:222-231).  One host wait for the whole chain.  rows = nodes (the stacked adjacency). */
int mrgcn_support_create_chain(mrgcn_support_t **supports, int32_t n, const mrgcn_plan_t *plan,
                               const uint8_t *row_flags, uint32_t flags, void *stream);
int mrgcn_support_destroy(mrgcn_support_t *support);
/* The same without waiting for the device, for a support that lived for one step (a mini-batch): the caller states
 * that every call that used the support was submitted to the stream it was created on (or is ordered before that
 * stream's tail); its memory is handed to later work on that stream. */
int mrgcn_support_destroy_ordered(mrgcn_support_t *support);
int mrgcn_support_info(const mrgcn_support_t *support, mrgcn_support_info_t *h_info);
int mrgcn_support_array(const mrgcn_support_t *support, int32_t which, const void **d_ptr, int64_t *h_count);
/* dM[k, 0:F] = sum over the kept entries e of live column k of val[e] * dY[row[e], 0:F] — the TRANSPOSED product
 * (autograd of torch.mm(A, .), graph.py:75,:95) restricted to the support; rows of dY outside the row set are never
 * read (they may be unwritten). */
int mrgcn_support_spmm_t_f32(const mrgcn_support_t *support, const float *dY, int64_t ldY, int32_t F, float *dM,
                             int64_t ldM, void *stream);
/* mrgcn_basis_mix_bwd_f32 on the support (dM: [L, ldM] by live number).
 *   dV == NULL : the norm-only pass in front of mrgcn_support_adam_rows_fused_f32: dcomp and *dV_sumsq (both
 *                WRITTEN, not accumulated: no zeroing by the caller, fixed summation order) — one pass over the
 *                live nodes' V blocks that stores each live column's B products, then a relation-major sum of
 *                those rows: no atomics anywhere.  `workspace`: mrgcn_support_mix_bwd_workspace(support, B) floats,
 *                8-byte aligned, laid out as
 *                  D [L][B] | slab [chunks][B] (padded to whole fours) | 2048 doubles: parts of ||dV||^2 |
 *                  ceil(NL / 8) doubles: the per-block parts of the one-shot form.
 *                Two forms (configuration row `sup_mix_stream`): 1 — a one-shot grid, a wave per two live nodes, V blocks
 *                as 16-byte pieces, taken when B F % 4 == 0, B F <= 1024, B <= 64, F <= 16 and even, V 16-byte
 *                aligned; its per-block parts of ||dV||^2 are folded by blocks appended to the relation-major sum's
 *                launch; 0, and every other shape — the resident kernel with `comp` in LDS.  D and dcomp have the
 *                same bits under both; ||dV||^2 differs in the last bits (its parts are grouped differently) and is
 *                bitwise reproducible under either.
 *   dV != NULL : the gradient itself; `dense` != 0 writes every block (zeros for nodes outside the support),
 *                dense == 0 only the blocks of the support's nodes (row-sparse: mrgcn_adam_step_rows_f32 with
 *                NODE_FLAGS as row_cur).  dcomp written; *dV_sumsq (nullable) ACCUMULATED into. */
int64_t mrgcn_support_mix_bwd_workspace(const mrgcn_support_t *support, int32_t B); /* floats */
int mrgcn_support_mix_bwd_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM, const float *V,
                              const float *comp, int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp,
                              double *dV_sumsq, float *workspace, int64_t workspace_floats, void *stream);
/* mrgcn_adam_step_rows_fused_f32 on the support: row_cur = NODE_FLAGS.  The support's nodes are walked as a list
 * (two node blocks in flight per wave, nontemporal p / m / v); `ever_outside` != 0 adds the pass over the nodes that
 * are flagged in row_ever without being nodes of this support (moments from steps on another row set: they decay,
 * their parameters drift on, as torch.optim.Adam does for a zero gradient).  0: the caller states there are none
 * (every step since row_ever was zeroed ran on this support) and that pass is not launched. */
int mrgcn_support_adam_rows_fused_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM, const float *comp,
                                      int32_t B, int32_t F, float *param, float *exp_avg, float *exp_avg_sq,
                                      uint8_t *row_ever, float lr, float beta1, float beta2, float eps, int64_t step,
                                      const float *bc_dev, const float *grad_scale, int32_t ever_outside,
                                      void *stream);
/* The node-table step under the reference's regularisation settings (node_classification.py:35-37,172-193:
 * `weight_decay` handed to optim.Adam, l1_lambda . sum|p| + l2_lambda . sum p^2 added to the loss, then backward,
 * clip_grad_norm_, optimizer.step()).  With any of the three non-zero every node block moves every step; the loss's
 * gradient still lives on the support only, so both passes walk nodes 0 .. N-1 as one-shot grids and rebuild each
 * node's gradient block g from its live columns of dM and comp in registers (a node without live columns: g = 0).
 * r(p) = l1 sign(p) + 2 l2 p in fp32, sign(0) = 0.
 * Shapes: those of mrgcn_adam_rows_fused_supported with B F / 4 <= 128 and F even; any other shape: a negative
 * workspace size / MRGCN_ERR_UNSUPPORTED, nothing written.
 *
 * mrgcn_support_reg_norm_f32 (node_classification.py:172-193: what clip_grad_norm_ sees of the node table, and the
 * penalty's value): out3 = { sum (g + r(p))^2, sum |p|, sum p^2 } over the whole table, in double from the element on,
 * WRITTEN (not accumulated); per-block partials in `workspace` (mrgcn_support_reg_norm_workspace BYTES, 8-byte
 * aligned) summed in block order by a second small launch: no atomics, bitwise reproducible.  Not needed for weight
 * decay alone: torch adds wd . p inside Adam.step, after the clip. */
int64_t mrgcn_support_reg_norm_workspace(const mrgcn_support_t *support, int32_t B, int32_t F);
int mrgcn_support_reg_norm_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM, const float *comp,
                               int32_t B, int32_t F, const float *param, float l1, float l2, double *out3,
                               void *workspace, int64_t workspace_bytes, void *stream);
/* mrgcn_support_adam_rows_fused_f32's update over ALL N nodes (node_classification.py:35-37,172-193) with
 *   gg = (g + r(p)) . grad_scale + weight_decay . p
 * — torch's order: the penalty is part of .grad and is clipped, Adam adds the decay afterwards.  Sets row_ever[j] = 1
 * for every node.  `step` / `bc_dev` / `grad_scale` as there.  With weight_decay = l1 = l2 = 0 the per-element chain is
 * that kernel's. */
int mrgcn_support_adam_rows_reg_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM, const float *comp,
                                    int32_t B, int32_t F, float *param, float *exp_avg, float *exp_avg_sq,
                                    uint8_t *row_ever, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, float l1, float l2, int64_t step, const float *bc_dev,
                                    const float *grad_scale, void *stream);
/* mrgcn_rel_transform_bwd_masked_f32 on the support: dW (nullable; written whole) and dX (nullable; every row
 * written, zeros outside NODE_FLAGS; `relu_mask_from_x` as there).  workspace:
 * mrgcn_support_rel_transform_bwd_workspace floats. */
int64_t mrgcn_support_rel_transform_bwd_workspace(const mrgcn_support_t *support, int32_t K, int32_t F,
                                                  int32_t need_dX, int32_t need_dW);
int mrgcn_support_rel_transform_bwd_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM, const float *X,
                                        int64_t ldX, int32_t K, const float *W, int32_t F, float *dX, int64_t lddX,
                                        float *dW, float *workspace, int64_t workspace_floats,
                                        int32_t relu_mask_from_x, void *stream);
/* dW of the relation transform from a TABLE of per-(row, relation) sums of a constant layer input X.  The support's
 * kept entries, sorted by (relation, output row, the transposed view's entry order), fall into P pairs; with
 *   S[p, 0:K]  = sum over the entries e of pair p of val_e . X[node_e, 0:K]          (mrgcn_support_pair_sums_build_f32)
 *   dW[r]      = sum over the pairs p of relation r of S[p]^T . dY[row_p, 0:F]       (mrgcn_support_dw_pairs_f32)
 * which is the dW of mrgcn_support_rel_transform_bwd_f32 with the sums reassociated: S depends on the graph, the row
 * set and X only, so a caller whose X is data builds it once and every epoch reads P rows of K floats in order
 * instead of gathering the X row of every live column.  No float atomics, fixed summation orders (a pair's entries in
 * the sorted order, pairs longer than `piece_entries` in pieces added in piece order; dW in chunks of `chunk_pairs`
 * pairs added in chunk order): both calls are bitwise reproducible.
 *   _info       builds the pair structure on first use (device work and host waits on `stream`; inside a stream
 *               capture nothing is built and an unbuilt structure reports pairs = -1)
 *   _build_f32  S [P, K] dense rows (K >= 4); X rows 4-byte aligned
 *   _dw_pairs   dY as the layer received it (only rows of the support's row set are read); dW [R, K, F] written whole
 *               (zeros for a relation without pairs); F <= 16; workspace: mrgcn_support_dw_pairs_workspace floats */
typedef struct mrgcn_pair_sums_info {
  int64_t pairs;            /* P (-1: not built, see above) */
  int64_t table_bytes;      /* P * K * 4 */
  int64_t chunks;           /* blocks of the dW pass */
  int64_t chunk_pairs;      /* pairs per chunk at most */
  int64_t piece_entries;    /* entries per piece of a pair's sum */
  int64_t max_pair_entries; /* entries of the longest pair */
  int64_t device_bytes;     /* of the pair structure */
} mrgcn_pair_sums_info_t;
int mrgcn_support_pair_sums_info(const mrgcn_support_t *support, int32_t K, mrgcn_pair_sums_info_t *h_info,
                                 void *stream);
int mrgcn_support_pair_sums_build_f32(const mrgcn_support_t *support, const float *X, int64_t ldX, int32_t K, float *S,
                                      void *stream);
int64_t mrgcn_support_dw_pairs_workspace(const mrgcn_support_t *support, int32_t K, int32_t F); /* floats */
int mrgcn_support_dw_pairs_f32(const mrgcn_support_t *support, const float *S, int32_t K, const float *dY,
                               int64_t ldY, int32_t F, float *dW, float *workspace, int64_t workspace_floats,
                               void *stream);
/* the same with the layer input X in bf16 rows (the bf16 pipeline; ldX in elements): dW's products and sums are fp32
 * on the widened elements; dX (= dM . W^T summed per node) never reads X */
int mrgcn_support_rel_transform_bwd_xbf16(const mrgcn_support_t *support, const float *dM, int64_t ldM,
                                          const uint16_t *X, int64_t ldX, int32_t K, const float *W, int32_t F,
                                          float *dX, int64_t lddX, float *dW, float *workspace,
                                          int64_t workspace_floats, void *stream);
/* dlogits[idx[i], 0:C] = *g * drows[i, 0:C] for the n labelled rows ONLY (idx without repeats): the rest of dlogits
 * is not touched — for a consumer that reads the labelled rows only (mrgcn_support_spmm_t_f32).  The 73 MB zero fill
 * of mrgcn_softmax_xent_bwd_f32 (AM shape) goes away. */
int mrgcn_softmax_xent_bwd_rows_f32(const float *drows, const int64_t *idx, int64_t n, int32_t C, const float *g,
                                    float *dlogits, int64_t ldd, void *stream);

/* ---- a mini-batch layer as a masked pass over the full graph's plan ------------------------
 * Replaces, for a re-sampled batch, the slice tensors and the per-batch plans of the frontier path below
 * (mrgcn/data/batch.py:185-263, mrgcn/models/rgcn.py:91-128, mrgcn/layers/graph.py:62-102 with A_idx): the sample of
 * a layer is the row-flag array of a MRGCN_SUPPORT_FORWARD support, its neighbours are the support's live nodes
 * (LNODE = getNeighboursSparse(A, sample)), and every array is compact: activations [NR, F] by FROW rank, the
 * neighbours' features / embeddings [live_nodes, K] by LNODE rank, per-column operands [L, ld] by live number.
 * The sample of the layer below is NODE_FLAGS of this one.
 *   spmm_fwd       Y[q] = act(bias + sum_e v[e] D[FCOL[e]]) over row FROW[q]'s entries; v = the stored values
 *                  (use_values != 0: the input term, graph.py:75) or all ones (the feature term on the sliced
 *                  adjacency, whose values sliceSparseCOO drops: batch.py:258-270).
 *   spmm_t_compact dM[k] = sum over live column k's entries of v[e] dY[ROWRANK[row[e]]]  (dY: [NR, ldY])
 *   mix_fwd        M[k] = sum_b comp[LREL[k], b] V[node of k, b]        (graph.py:66-74 on the live columns)
 *   rel_transform_fwd / _bwd_compact   T[k] = X[LNODE_ORD[k]] . W[LREL[k]] (graph.py:83-95) and its backward: dW
 *                  (nullable, written whole), dX [live_nodes, lddX] (nullable, every row written;
 *                  `relu_mask_from_x` as mrgcn_rel_transform_bwd_masked_f32); workspace:
 *                  mrgcn_support_rel_transform_bwd_workspace floats.  x_by_node != 0: X is the whole feature
 *                  matrix, one row per NODE (the rows X[LNODE] are picked inside the transform instead of by a
 *                  gather in front of it; dX stays by LNODE rank).  Shapes: mrgcn_support_rel_transform_supported
 *                  (need_dX: the input gradient is wanted too — inputs of up to 64 floats per row).
 * The weight_I gradient of the input term is mrgcn_support_mix_bwd_f32 / mrgcn_support_adam_rows_fused_f32 above
 * (dM by live number, V blocks by node id).  One product per support in flight. */
int mrgcn_support_spmm_fwd_f32(const mrgcn_support_t *support, int32_t use_values, const float *D, int64_t ldD,
                               int32_t F, float *Y, int64_t ldY, const float *bias, int32_t relu, void *stream);
int mrgcn_support_spmm_t_compact_f32(const mrgcn_support_t *support, int32_t use_values, const float *dY, int64_t ldY,
                                     int32_t F, float *dM, int64_t ldM, void *stream);
int mrgcn_support_mix_fwd_f32(const mrgcn_support_t *support, const float *V, const float *comp, int32_t B, int32_t F,
                              float *M, int64_t ldM, void *stream);
/* weight_I WITHOUT bases (the reference's literal (R*N) x F table, graph.py:72-74) on the live columns:
 * scatter == 0: M[k] = table[LREL[k] * N + node(k)];  scatter != 0: table is zeroed whole, then those rows = M[k]. */
int mrgcn_support_literal_rows_f32(const mrgcn_support_t *support, int32_t scatter, float *table, int32_t F, float *M,
                                   int64_t ldM, void *stream);
/* The WIDE featureless input layer on a forward support (masked_wide.hip): 1 <= B <= 4 bases, 16 < F <= 256,
 * F % 4 == 0, V node-major [N][B][F] (16-byte aligned), no compact operand M.  The reference's mini-batch
 * link-prediction encoder (tasks/link_prediction.py:477-530 batches through rgcn.py:91-128 into graph.py:66-81:
 * AI = A[sample] . (comp (x) weight_I), then the ReLU of rgcn.py:86-87).
 *   _fwd_f32   Y[q] = relu?( sum over FPTR entries e of flagged row q: FVAL[e] sum_b comp[LREL[c]][b] V[node(c)][b] ),
 *              rows by FROW rank, whole rows written (replaces mrgcn_support_mix_fwd_f32 + _spmm_fwd_f32 there).
 *   _bwd_f32   from dY [NR] x F (rows by FROW rank, the ReLU mask already applied): dV rows of the support's nodes
 *              (NODE_FLAGS; dense != 0 zeroes the rest of the [N][B][F] table first), dcomp [R][B] written whole and
 *              *dV_sumsq (nullable) = ||dV||^2, all summed in a fixed order (no atomics: bitwise reproducible).
 *              Replaces mrgcn_support_spmm_t_compact_f32 + mrgcn_support_mix_bwd_f32 for this shape family. */
int32_t mrgcn_support_wide_supported(const mrgcn_support_t *support, int32_t B, int32_t F);
int mrgcn_support_wide_fwd_f32(const mrgcn_support_t *support, const float *V, const float *comp, int32_t B, int32_t F,
                               float *Y, int64_t ldY, int32_t relu, void *stream);
int64_t mrgcn_support_wide_bwd_workspace(const mrgcn_support_t *support, int32_t B); /* floats */
int mrgcn_support_wide_bwd_f32(const mrgcn_support_t *support, const float *dY, int64_t ldY, const float *V,
                               const float *comp, int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp,
                               double *dV_sumsq, float *workspace, int64_t workspace_floats, void *stream);
/* The WIDE layer WITH a feature term on a forward support (masked_wide.hip, two tables; the multimodal
 * link-prediction encoders of configs/ml100k+.toml / yago3-10+.toml in mini-batch mode), same shapes as above
 * (mrgcn_support_wide_supported).  The feature term is reassociated through P = X . V_F (mrgcn_support_basis_xform_f32):
 *   _fwd_f32   Y[q] = relu?( sum over FPTR entries e of q:  v_e sum_b comp[LREL[c]][b] V[node(c)][b]      (V, comp: NULL
 *                                                                                        on a layer without input term)
 *                                                 + w_e sum_b comp_F[LREL[c]][b] P[rank(c)][b] )
 *              P [NL][B][F] by live-node rank (16-byte aligned), w_e = v_e when feature_values, else 1.
 *   _bwd_f32   from dY (ReLU mask applied): dV / dcomp / *dV_sumsq exactly as mrgcn_support_wide_bwd_f32 (all NULL
 *              without input term), dP [NL][B][F] written whole and dcomp_F [R][B] written whole; one pass over the dY
 *              rows, fixed-order sums, no atomics. */
int mrgcn_support_wide_feat_fwd_f32(const mrgcn_support_t *support, const float *V, const float *comp, const float *P,
                                    const float *comp_F, int32_t feature_values, int32_t B, int32_t F, float *Y,
                                    int64_t ldY, int32_t relu, void *stream);
int64_t mrgcn_support_wide_feat_bwd_workspace(const mrgcn_support_t *support, int32_t B); /* floats */
int mrgcn_support_wide_feat_bwd_f32(const mrgcn_support_t *support, const float *dY, int64_t ldY, const float *V,
                                    const float *comp, const float *P, const float *comp_F, int32_t feature_values,
                                    int32_t B, int32_t F, float *dV, int32_t dense, float *dcomp, double *dV_sumsq,
                                    float *dP, float *dcomp_F, float *workspace, int64_t workspace_floats,
                                    void *stream);
/* The basis transform of that feature term on the matrix cores (basis_xform.hip, exact fp32):
 *   _f32       P[l][b][f] = sum_k X[row(l)][k] V_F[b][k][f], l < NL; row(l) = LNODE[l] when x_by_node (X holds every
 *              node), else l (X holds the live nodes by rank).  V_F [B][K][F] (the reference's weight_F), K >= 1.
 *   _bwd_f32   dX [NL] x K (ld_dX; by rank, nullable) = sum_b dP[:, b] . V_F[b]^T and dV_F [B][K][F] (nullable) =
 *              X^T . dP, the live nodes summed in fixed chunks and the chunks in order: no atomics. */
int mrgcn_support_basis_xform_f32(const mrgcn_support_t *support, const float *X, int64_t ldX, int32_t x_by_node,
                                  int32_t K, const float *V_F, int32_t B, int32_t F, float *P, void *stream);
int64_t mrgcn_support_basis_xform_bwd_workspace(const mrgcn_support_t *support, int32_t K, int32_t B,
                                                int32_t F); /* floats */
int mrgcn_support_basis_xform_bwd_f32(const mrgcn_support_t *support, const float *dP, const float *X, int64_t ldX,
                                      int32_t x_by_node, int32_t K, const float *V_F, int32_t B, int32_t F, float *dX,
                                      int64_t ld_dX, float *dV_F, float *workspace, int64_t workspace_floats,
                                      void *stream);
int32_t mrgcn_support_rel_transform_supported(const mrgcn_support_t *support, int32_t K, int32_t F, int32_t need_dX);
int mrgcn_support_rel_transform_fwd_f32(const mrgcn_support_t *support, const float *X, int64_t ldX, int32_t x_by_node,
                                        int32_t K, const float *W, int32_t F, float *T, int64_t ldT, void *stream);
int mrgcn_support_rel_transform_bwd_compact_f32(const mrgcn_support_t *support, const float *dM, int64_t ldM,
                                                const float *X, int64_t ldX, int32_t x_by_node, int32_t K,
                                                const float *W, int32_t F,
                                                float *dX, int64_t lddX, float *dW, float *workspace,
                                                int64_t workspace_floats, int32_t relu_mask_from_x, void *stream);

/* ---- epoch kernels around the layers ----------------------------------------------
 * out = dY * (Y > 0): backward of the nn.ReLU between layers (rgcn.py:86-87) */
int mrgcn_relu_bwd_f32(const float *dY, const float *Y, int64_t n, float *out, void *stream);
/* dst[n_rows, F] (contiguous) = the rows of `src` scattered to their places, zeros everywhere else, in ONE pass:
 * dst[sorted_rows[k], :] = src[perm[k], 0:F] (sorted_rows rising, without repeats).  The dense gradient of the literal
 * (R*N) x out `weight_I` of a layer without bases (autograd of graph.py:75): sorted_rows = the plan's touched literal
 * columns in rising order, perm = their compact ids, src = the compact gradient rows. */
int mrgcn_scatter_rows_zero_fill_f32(const int32_t *sorted_rows, const int32_t *perm, int64_t n_touched,
                                     const float *src, int64_t ldS, int32_t F, float *dst, int64_t n_rows, void *stream);
/* out[0:F] = the column sums of X[M, F] (row stride ld) over the rows with row_flags[m] != 0 (NULL: every row; rows
 * flagged 0 are not read — they may be unwritten).  The bias gradient `dY.sum(0)` of a narrow layer (autograd of
 * `AFW + self.b`, graph.py:98-101) in one pass, summed in a fixed order.  F <= 16; workspace of
 * mrgcn_colsum_rows_workspace(F) floats (-1: F outside the kernel's range). */
int64_t mrgcn_colsum_rows_workspace(int32_t F);
int mrgcn_colsum_rows_f32(const float *X, int64_t ld, int64_t M, int32_t F, const uint8_t *row_flags, float *out,
                          float *workspace, int64_t workspace_floats, void *stream);
/* Streaming yardsticks for measurement (bench.py: extra.device_copy_gbps_hip, extra.triad_gbps): dst = src as a plain
 * float4 copy, and a 3-read / 3-write elementwise pass with Adam's arithmetic (the memory shape of a dense optimizer
 * step).  n % 4 == 0, 16-byte aligned.  Nothing in the package calls them. */
int mrgcn_probe_copy_f32(const float *src, float *dst, int64_t n, void *stream);
int mrgcn_probe_triad_f32(float *p, float *m, float *v, int64_t n, void *stream);
/* the same two as PERSISTENT grids (2 048 resident blocks striding through the arrays): what a kernel with per-block
 * state reaches — 4.8 / 4.9 TB/s on the bench boxes against 6.25 / 6.0 for the one-shot grids above */
int mrgcn_probe_copy_persistent_f32(const float *src, float *dst, int64_t n, void *stream);
int mrgcn_probe_triad_persistent_f32(float *p, float *m, float *v, int64_t n, void *stream);
/* the same with row-strided operands: out[r, 0:F] = dY[r, 0:F] * (Y[r, 0:F] > 0) — the layer output Y of the
 * COMPACT product may live in a buffer with padded rows (MRGCN_SPMM_PAD_WRITABLE) */
int mrgcn_relu_bwd_rows_f32(const float *dY, int64_t ld_dY, const float *Y, int64_t ldY, int64_t rows, int32_t F,
                            float *out, int64_t ld_out, void *stream);
/* loss = mean_i CE(logits[idx[i]], target[i]); dlogits (nullable, [num_rows, ldd]) is zeroed
 * and receives d loss / d logits.  nn.CrossEntropyLoss over Y_hat[idx]
 * (node_classification.py:439-444) and its backward. */
int mrgcn_softmax_xent_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx,
                           const int64_t *target, int64_t n, float *loss, float *dlogits,
                           int64_t ldd, int64_t num_rows, void *stream);
/* The same loss with its gradient kept compact — drows (nullable, [n, C]) = d loss / d logits[idx[i], :] — and the
 * backward that forms the dense gradient from it: dlogits = 0, dlogits[idx[i], :] += *g * drows[i, :] (g: device
 * float, nullable = 1), row_flags (nullable, [num_rows] bytes) = 1 at the labelled rows, 0 elsewhere (the flags
 * mrgcn_spmm_transposed_live_flagged_f32 takes).  No dense pass besides the zero fill. */
int mrgcn_softmax_xent_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx, const int64_t *target,
                                int64_t n, float *loss, float *drows, void *stream);
int mrgcn_softmax_xent_bwd_f32(const float *drows, const int64_t *idx, int64_t n, int32_t C, const float *g,
                               float *dlogits, int64_t ldd, int64_t num_rows, uint8_t *row_flags, void *stream);
/* *accum += sum(x^2)  (accum is a device double, zeroed by the caller once per step) */
int mrgcn_sumsq_accum_f32(const float *x, int64_t n, double *accum, void *stream);
/* clip_grad_norm_(…, max_norm) (node_classification.py:192): norm = sqrt(*sumsq),
 * coef = min(1, max_norm / (norm + 1e-6)); both stay on the device */
int mrgcn_clip_coef_f32(const double *sumsq, float max_norm, float *coef, float *norm, void *stream);
/* The clip of the SMALL dense parameters in one launch (<= 16 tensors; host arrays of device pointers / sizes):
 * sum of squares of every gradient, plus `extra` device doubles (squared norms that arrived from elsewhere: the
 * row-sparse node table's), -> *sumsq_out (nullable), the coefficient min(1, max_norm / (norm + 1e-6)) -> *coef
 * (nullable; max_norm <= 0: 1), the norm -> *norm (nullable) and — with `step_dev` — the device step counter and
 * bias corrections of mrgcn_adam_bias_f32.  `accum` (double) and `ticket` (uint32) are scratch words that must be
 * zero at the first call; the kernel leaves them zero.  Replaces n mrgcn_sumsq_accum_f32 + mrgcn_clip_coef_f32 +
 * mrgcn_adam_bias_f32 launches (each ~6 us inside a replayed hipGraph). */
/* *accum += the squared norms of <= 16 tensors in one launch (the launches in front of mrgcn_sumsq_clip_multi_f32 for a
 * model with more small tensors than one call takes; `accum` is the same scratch word, which that call reads and clears) */
int mrgcn_sumsq_accum_multi_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, double *accum,
                                void *stream);
int mrgcn_sumsq_clip_multi_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, int32_t n_extra,
                               const double *const *extra, double *accum, uint32_t *ticket, float max_norm,
                               double *sumsq_out, float *coef, float *norm, int64_t *step_dev, float beta1,
                               float beta2, float *bc_dev, void *stream);
/* The three sums above in a fixed order, for torch.use_deterministic_algorithms(True): per-block double partials of a
 * fixed tree, added in block order by the block that arrives last; grids depend on the sizes only, never on the
 * device.  Same results bit for bit on every run.  `partials`: device scratch of mrgcn_sumsq_det_workspace() bytes
 * (fully written before it is read); `ticket`: a uint32 that is zero at the first call, left zero.  The _clip_ form
 * takes the arguments of mrgcn_sumsq_clip_multi_f32 (its ticket is the same word) and `partials`. */
int64_t mrgcn_sumsq_det_workspace(void);
int mrgcn_sumsq_accum_det_f32(const float *x, int64_t n, double *accum, double *partials, uint32_t *ticket,
                              void *stream);
int mrgcn_sumsq_accum_multi_det_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, double *accum,
                                    double *partials, uint32_t *ticket, void *stream);
int mrgcn_sumsq_clip_multi_det_f32(int32_t n_tensors, const float *const *grads, const int64_t *numel, int32_t n_extra,
                                   const double *const *extra, double *accum, uint32_t *ticket, float max_norm,
                                   double *sumsq_out, float *coef, float *norm, int64_t *step_dev, float beta1,
                                   float beta2, float *bc_dev, double *partials, void *stream);
/* mrgcn_adam_step_f32 / _dev_f32 for <= 16 small tensors in one launch (per-tensor lr / weight_decay; bc_dev
 * nullable: host-side bias corrections from `step`). */
int mrgcn_adam_step_multi_f32(int32_t n_tensors, float *const *params, const float *const *grads,
                              float *const *exp_avg, float *const *exp_avg_sq, const int64_t *numel, const float *lr,
                              const float *weight_decay, float beta1, float beta2, float eps, int64_t step,
                              const float *bc_dev, const float *grad_scale, void *stream);
/* The L1 / L2 weight penalty of the link-prediction loop (tasks/link_prediction.py:306-326: l1 sum|p| + l2 sum p^2 over
 * the `weight*` parameters joins the loss, is differentiated, clipped with it by clip_grad_norm_ and stepped) on
 * <= 16 float32 tensors per launch, without rewriting a gradient.  Tensor t: params[t], grads[t] (nullable: no
 * gradient this step), numel[t], and — with row_flags (nullable array) — row_flags[t] (nullable uint8 [numel / row_len])
 * and row_len[t]: row i of the gradient buffer counts only where row_flags[t][i] != 0; its other rows are never read.
 * r(p) = l1 sgn(p) + 2 l2 p, sgn(0) = 0.
 * mrgcn_penalty_norm_multi_f32 ADDS sum (g + r(p))^2, sum |p| and sum p^2 into the device doubles out3[0..2] (zeroed by
 * the caller; several launches chain into one out3) in a fixed order — a fixed float tree per block, double partials
 * added in block order by the block that arrives last, a grid that depends on the sizes only: the same bits on every
 * run.  `partials`: device scratch of mrgcn_penalty_norm_workspace() BYTES (fully written before it is read);
 * `ticket`: a uint32 that is zero at the first call, left zero.  A tensor above 2^20 elements takes a launch of its
 * own.
 * mrgcn_adam_step_reg_multi_f32: mrgcn_adam_step_multi_f32's update of every element on
 * gg = (g + r(p)) * *grad_scale + weight_decay * p (torch's order: the penalty is clipped, the decay is not).
 * 16-byte accesses where every base is 16-byte aligned and flagged rows hold whole pieces, scalar ones otherwise. */
int64_t mrgcn_penalty_norm_workspace(void);
int mrgcn_penalty_norm_multi_f32(int32_t n_tensors, const float *const *params, const float *const *grads,
                                 const int64_t *numel, const uint8_t *const *row_flags, const int32_t *row_len, float l1,
                                 float l2, double *out3, double *partials, uint32_t *ticket, void *stream);
int mrgcn_adam_step_reg_multi_f32(int32_t n_tensors, float *const *params, const float *const *grads,
                                  const int64_t *numel, const uint8_t *const *row_flags, const int32_t *row_len,
                                  float *const *exp_avg, float *const *exp_avg_sq, const float *lr,
                                  const float *weight_decay, float l1, float l2, float beta1, float beta2, float eps,
                                  int64_t step, const float *bc_dev, const float *grad_scale, void *stream);
/* torch.optim.Adam step (node_classification.py:35-37, :193) on one tensor; the gradient is
 * multiplied by *grad_scale (device float, nullable) first, i.e. the clip is folded in. */
int mrgcn_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                        int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, const float *grad_scale, void *stream);

/* ---- link-prediction decoder (DistMult) ---------------------
 * triples: device int64 [n, 3] rows (s, p, o) indexing E (node embeddings = the encoder's
 * output) and Rel (relation embeddings, rgcn.py:40-47 `relations`). */
/* scores[t] = sum_h E[s,h] Rel[p,h] E[o,h] — score_distmult_bc with the 1-D index tensors
 * train_model passes (tasks/link_prediction.py:266-275, :645-665) */
int mrgcn_distmult_score_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                             const int64_t *triples, int64_t n, float *scores, void *stream);
/* its backward: dE / dRel (nullable) are ACCUMULATED into (zero them first) */
int mrgcn_distmult_score_bwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR,
                                 int32_t H, const int64_t *triples, int64_t n, const float *dscores,
                                 float *dE, int64_t lddE, float *dRel, int64_t lddR, void *stream);
/* the same gradients from triples visited in sorted order: order_s / order_p / order_o are device
 * int64 permutations of 0..n-1 that sort the triples by subject / predicate / object (any order
 * within ties).  Runs of equal targets are summed in registers, so the float atomics of the
 * scatter form (which collide on the few hundred relation rows) shrink by the run length.
 * dE needs order_s and order_o, dRel needs order_p; both are ACCUMULATED into. */
/* ... and those three permutations (any may be NULL): stable radix sorts of the subject / predicate / object columns
 * over the bits ids below num_nodes / num_relations can have (replaces three torch.argsort calls of the run loop's
 * autograd: a merge sort of ~30 launches per column).  workspace: mrgcn_distmult_orders_workspace(n) bytes. */
/* out[i] = pi(i) for i < k, pi a bijection of [0, n) keyed by the device word *seed_dev (a Feistel network with cycle
 * walking): k distinct pseudo-random indices below n in one launch — the corrupted facts of the device-side negative
 * sampler (tasks/link_prediction.py sample_negatives_device; torch.randperm(n)[:k] sorts n keys). */
int mrgcn_random_subset_i64(int64_t n, int64_t k, const int64_t *seed_dev, int64_t *out, void *stream);
/* The in-batch corruption of train_model (tasks/link_prediction.py:239-263) in one launch: out[k] (k < ncorrupt), rows
 * (s, p, o), is a copy of fact pi(k) — ncorrupt DISTINCT facts of the n given, pi keyed by *seed_dev as above — with
 * its head (k < nhead) or its tail replaced by nodes[u], u uniform in [0, n_nodes) (`nodes`: the batch's node set). */
int mrgcn_corrupt_triples_i64(const int64_t *facts, int64_t n, const int64_t *nodes, int64_t n_nodes,
                              const int64_t *seed_dev, int64_t ncorrupt, int64_t nhead, int64_t *out, void *stream);
int64_t mrgcn_distmult_orders_workspace(int64_t n);
int mrgcn_distmult_orders(const int64_t *triples, int64_t n, int64_t num_nodes, int64_t num_relations,
                          int64_t *order_s, int64_t *order_p, int64_t *order_o, void *workspace,
                          int64_t workspace_bytes, void *stream);
/* the same three permutations for a SMALL triple set (the corrupted facts drawn anew every epoch) by a counting sort:
 * a histogram pass, one scan block per column, a fill pass — four launches where the radix sort takes ~25
 * launch-bound ones.  Ties in no particular order.  workspace: mrgcn_distmult_orders_counting_workspace bytes. */
int64_t mrgcn_distmult_orders_counting_workspace(int64_t num_nodes, int64_t num_relations);
int mrgcn_distmult_orders_counting(const int64_t *triples, int64_t n, int64_t num_nodes, int64_t num_relations,
                                   int64_t *order_s, int64_t *order_p, int64_t *order_o, void *workspace,
                                   int64_t workspace_bytes, void *stream);
int mrgcn_distmult_score_bwd_sorted_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR,
                                        int32_t H, const int64_t *triples, int64_t n,
                                        const float *dscores, const int64_t *order_s,
                                        const int64_t *order_p, const int64_t *order_o, float *dE,
                                        int64_t lddE, float *dRel, int64_t lddR, void *stream);
/* nn.BCEWithLogitsLoss() (link_prediction.py:57, :550-554): *loss = mean; dx (nullable) its
 * gradient w.r.t. x */
int mrgcn_bce_logits_f32(const float *x, const float *y, int64_t n, float *loss, float *dx,
                         void *stream);
/* Deterministic twins for torch.use_deterministic_algorithms(True): the same results, bit for bit on every run.
 * _score_bwd_det: dE / dRel (nullable) ACCUMULATED into, every row by one owner per pass, no float atomics.
 *   n <= 4096: one block sorts the columns itself (orders ignored, may be NULL).  Larger n: order_s / _p / _o must be
 *   STABLE sorts of the columns (SortedTriples, mrgcn_distmult_orders; not the counting sort); runs that cross a
 *   wave's span meet in a slab and are added in wave order.  workspace: mrgcn_distmult_bwd_det_workspace(n, H) bytes.
 * _bce_logits_det: *loss WRITTEN (block partials added in block order; one block for n <= 8192); workspace:
 *   mrgcn_bce_logits_det_workspace(n) bytes, unread for small n. */
int64_t mrgcn_distmult_bwd_det_workspace(int64_t n, int32_t H);
int mrgcn_distmult_score_bwd_det_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                     const int64_t *triples, int64_t n, const float *dscores, const int64_t *order_s,
                                     const int64_t *order_p, const int64_t *order_o, float *dE, int64_t lddE,
                                     float *dRel, int64_t lddR, void *workspace, int64_t workspace_bytes,
                                     void *stream);
int64_t mrgcn_bce_logits_det_workspace(int64_t n);
int mrgcn_bce_logits_det_f32(const float *x, const float *y, int64_t n, float *loss, float *dx, void *workspace,
                             int64_t workspace_bytes, void *stream);
/* compute_ranks_fast (link_prediction.py:593-643): ranks[0:nf] tail-corruption, ranks[nf:2nf]
 * head-corruption rank of every fact against all num_nodes candidates;
 * rank = #greater + round_half_even((#ties-1)/2) + 1.  Filtered ranks: per fact a sorted list
 * of candidate nodes to ignore (the -inf entries of filter_scores_, :667-689) in CSR form,
 * tail_* for tail corruption and head_* for head corruption; all four NULL = raw ranks.
 * Scores are never stored.  workspace: device, >= mrgcn_distmult_ranks_workspace() bytes. */
int64_t mrgcn_distmult_ranks_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_distmult_ranks(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel,
                         int64_t ldR, int32_t H, const int64_t *triples, int64_t num_facts,
                         const int64_t *tail_ptr, const int32_t *tail_idx, const int64_t *head_ptr,
                         const int32_t *head_idx, void *workspace, int64_t workspace_bytes,
                         int64_t *ranks, void *stream);
/* Raw AND filtered ranks from one scoring pass: what test_model (link_prediction.py:394-408) gets from two calls of
 * compute_ranks_fast (:593-643), filtered = False and True, over the same [facts, nodes] scores.  ranks_raw / ranks_flt
 * [2 nf] are what mrgcn_distmult_ranks writes without / with the lists, bit for bit (one shared score body); all four
 * lists NULL: raw ranks only, ranks_flt may be NULL and stays unwritten.  One call stands for one call per PART of the
 * facts (test_model's batches, each filtered by truedicts of its own facts): every fact owns its ptr range, and
 * part_ptr [num_parts + 1] (device, rising, part_ptr[0] = 0; NULL: one part) names the parts, because the reference
 * leaves the facts at positions >= num_nodes of a call unscored (:611-617) and the position meant is the one inside
 * the fact's part.  Any num_facts: the scoring grid is launched in slices of slice_facts facts (0: the default,
 * mrgcn_distmult_ranks_both_slice(); at most 524280, rounded up to whole tiles of 8).  workspace: device,
 * >= mrgcn_distmult_ranks_both_workspace() bytes (Et [H, N], truth [nf], scored [nf], counts [8 nf]). */
int64_t mrgcn_distmult_ranks_both_slice(void);
int64_t mrgcn_distmult_ranks_both_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_distmult_ranks_both(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                              const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                              const int64_t *part_ptr, int64_t num_parts, int64_t slice_facts, void *workspace,
                              int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt, void *stream);
/* test_model's metrics (link_prediction.py:403-419) of a rank vector [2 nf] (tail ranks, then head ranks): part p owns
 * ranks [p0, p1) and nf + [p0, p1), p0 = part_ptr[p], p1 = part_ptr[p + 1] (NULL: one part); out4 = the mean over the
 * parts of the parts' mean(1 / rank), mean(rank <= 1), mean(rank <= 3), mean(rank <= 10), summed in float64 in a fixed
 * order without atomics and rounded once to float32; score_out (nullable) = (float)(1 - mrr), the score train_model
 * records (:363).  The caller guarantees 0 = part_ptr[0] < part_ptr[1] < ... < part_ptr[num_parts] = num_facts (parts
 * are not empty: an empty one would add nothing and still count in the mean); nothing on the device checks it, but
 * bounds outside [0, num_facts] are clamped, so no read leaves `ranks`.  Equal inputs give equal bits. */
int mrgcn_rank_metrics(const int64_t *ranks, int64_t num_facts, const int64_t *part_ptr, int64_t num_parts, float *out4,
                       float *score_out, void *stream);
/* Top-k completion of (s, p, ?) / (?, p, o) queries: what a user of the reference reads off the [facts, nodes] score
 * matrix of compute_ranks_fast (link_prediction.py:593-643; scores :645-665) with a sort.  queries: device int64
 * [nq, 2] rows (anchor node, relation); head == 0: candidates fill the tail slot, score = sum_h (E[s,h] Rel[p,h])
 * E[c,h]; head == 1: the head slot, sum_h (E[c,h] Rel[p,h]) E[o,h] - float32, sequential over h, uncontracted: the rank
 * kernel's scores bit for bit (one shared body).  Row q of out_idx / out_score [nq, k]: the k best candidates, score
 * descending, equal scores (-0 == +0) by ascending node id; candidates in excl_idx[excl_ptr[q] : excl_ptr[q+1]]
 * (sorted per query; both arrays or neither) never appear; a row with fewer than k candidates ends in (-1, -inf).
 * A pure function of its inputs (no atomics); embeddings must be finite (NaN: undefined).  1 <= k <= 256.  The score
 * matrix is never stored: workspace = H N floats + nq * k * ceil(N / 256) 64-bit keys,
 * mrgcn_distmult_topk_workspace() bytes (-1 for bad arguments).  No host synchronisation; capturable. */
int64_t mrgcn_distmult_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k);
int mrgcn_distmult_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                        const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *excl_ptr,
                        const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                        int64_t *out_idx, float *out_score, void *stream);

/* ComplEx beside DistMult (Trouillon et al., "Complex Embeddings for Simple Link Prediction", ICML 2016, eq. 11; the
 * reference has DistMult only): score = Re sum_k e_s[k] r[k] conj(e_o[k]) over K = H / 2 complex numbers, a row's first
 * K columns the real parts and its last K the imaginary parts.  H must be even.  Same triple layout as the DistMult
 * entries.
 * _score: lanes over k, a fixed shuffle tree per triple; a pure function of its inputs (equal inputs, equal bits), held to float64 by a
 *   tolerance.
 * _score_bwd: dE / dRel (nullable) ACCUMULATED into.  With g = dscores and a row x = (xr | xi):
 *     dE[s] += g (rr or + ri oi | rr oi - ri or)   dE[o] += g (sr rr - si ri | si rr + sr ri)
 *     dRel[p] += g (sr or + si oi | sr oi - si or)
 *   order_s / _p / _o: STABLE sorts of the triples by column (SortedTriples, mrgcn_distmult_orders; with the counting
 *   sort's the sums are right but their order, and so their last bits, may change from run to run).  Runs of equal
 *   targets are summed in registers along the orders; every row has one owner per pass, runs that cross a wave's span
 *   meet in a slab and are added in wave order: no float atomics, equal bits on every run.  workspace:
 *   mrgcn_complex_bwd_workspace(n, H) bytes (-1 for an odd H).
 * _ranks_both / _topk: mrgcn_distmult_ranks_both's and mrgcn_distmult_topk's contracts word for word, with the
 *   candidate score sum_h q[h] E[c,h], sequential over h = 0 .. H-1 in float32, uncontracted, where for k < K
 *     tail side (anchor s)   q[k] = sr rr - si ri    q[K+k] = si rr + sr ri
 *     head side (anchor o)   q[k] = rr or + ri oi    q[K+k] = rr oi - ri or
 *   each product rounded, then the sum or difference rounded once.  The two sides round differently, so the ranks keep
 *   the fact's own score per side (truth [2 nf] in the workspace).  One score body serves both entries. */
int mrgcn_complex_score_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                            const int64_t *triples, int64_t n, float *scores, void *stream);
int64_t mrgcn_complex_bwd_workspace(int64_t n, int32_t H);
int mrgcn_complex_score_bwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                const int64_t *triples, int64_t n, const float *dscores, const int64_t *order_s,
                                const int64_t *order_p, const int64_t *order_o, float *dE, int64_t lddE, float *dRel,
                                int64_t lddR, void *workspace, int64_t workspace_bytes, void *stream);
int64_t mrgcn_complex_ranks_both_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_complex_ranks_both(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                             const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                             const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                             const int64_t *part_ptr, int64_t num_parts, int64_t slice_facts, void *workspace,
                             int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt, void *stream);
int64_t mrgcn_complex_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k);
int mrgcn_complex_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                       const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *excl_ptr,
                       const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                       int64_t *out_idx, float *out_score, void *stream);

/* ---- type-constrained ranks and top-k (csrc/lp_typed.hip, csrc/distmult_topk.hip; Krompass et al., ISWC 2015) ------
 * Candidates per relation and side instead of every node: cand_ptr (int64 [2 R + 1]) / cand_idx (int32, each list
 * ascending, duplicate free, ids in [0, num_nodes)) as in mrgcn_negatives_draw_typed_i64 — slot 2 p the tails of
 * relation p, slot 2 p + 1 its heads.  The host groups the facts (queries) by relation: order (int64 [n]) lists their
 * indices relation by relation, tile_ptr (int64 [num_tiles + 1], rising from 0 to n) cuts that sequence into tiles of
 * at most 8 facts OF ONE RELATION, tile_rel (int32 [num_tiles]) names each tile's relation.  A block takes one work item
 * of `work` (int32 [num_work, 2]) and scores one tile against 256 positions of its slot; candidate scores are
 * mrgcn_distmult_ranks_both's / mrgcn_complex_ranks_both's bit for bit (one shared body, called with the gathered id).
 * All arrays are device memory; what the host built is trusted (tiles and items outside their ranges are skipped).
 *
 * _typed_ranks: work item {2 tile + side, candidate tile} for every tile, side (0 tail, 1 head) and candidate tile
 *   below ceil(slot length / 256).  ranks_raw / ranks_flt [2 nf]: tail ranks, then head ranks, in the order of
 *   `triples` (NOT the grouped order); rank = #greater + round_half_even((#ties - 1) / 2) + 1 counted over the slot's
 *   candidates — the fact's own answer must be one of them —, for ranks_flt without the candidates of the fact's filter
 *   list (tail_* / head_* as in mrgcn_distmult_ranks_both, indexed by the fact's position in `triples`; all four NULL:
 *   raw ranks only).  EVERY fact is scored: the reference's rule that facts at positions >= num_nodes of a call stay
 *   unscored (link_prediction.py:611-617) is compute_ranks_fast's and is not carried over; there is no part_ptr.
 *   workspace: mrgcn_*_typed_ranks_workspace() bytes (Et [H, N], truth [nf] — [2 nf] for ComplEx —, counts [8 nf]).
 * _typed_topk: mrgcn_distmult_topk's contract (queries [nq, 2], head, exclusions, k, result order, (-1, -inf) tails)
 *   over the nodes of the query relation's slot on the asked side; work item {tile, candidate tile}; q_tiles (int32
 *   [nq]) = ceil(slot length / 256) of each query (0: an empty slot, a row of (-1, -inf)); max_slot = the longest slot
 *   among the queries'.  Rows come back in the order of `queries`; excl_ptr is indexed by it too.  workspace = H N
 *   floats (the transposed table the gather reads) + nq * k * max(1, ceil(max_slot / 256)) 64-bit keys: the tile lists
 *   are sized by the longest slot, not by num_nodes.  No host synchronisation; capturable; pure functions of their
 *   inputs (the counts are integer atomics: any order, one sum). */
int64_t mrgcn_distmult_typed_ranks_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_distmult_typed_ranks(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                               const int64_t *triples, int64_t num_facts, const int64_t *order,
                               const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                               int64_t num_work, const int64_t *cand_ptr, const int32_t *cand_idx,
                               const int64_t *tail_ptr, const int32_t *tail_idx, const int64_t *head_ptr,
                               const int32_t *head_idx, void *workspace, int64_t workspace_bytes, int64_t *ranks_raw,
                               int64_t *ranks_flt, void *stream);
int64_t mrgcn_complex_typed_ranks_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_complex_typed_ranks(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *order,
                              const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                              int64_t num_work, const int64_t *cand_ptr, const int32_t *cand_idx,
                              const int64_t *tail_ptr, const int32_t *tail_idx, const int64_t *head_ptr,
                              const int32_t *head_idx, void *workspace, int64_t workspace_bytes, int64_t *ranks_raw,
                              int64_t *ranks_flt, void *stream);
int64_t mrgcn_distmult_typed_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k,
                                            int64_t max_slot);
int mrgcn_distmult_typed_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *order,
                              const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                              int64_t num_work, const int32_t *q_tiles, const int64_t *cand_ptr,
                              const int32_t *cand_idx, int64_t max_slot, const int64_t *excl_ptr,
                              const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                              int64_t *out_idx, float *out_score, void *stream);
int64_t mrgcn_complex_typed_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k,
                                           int64_t max_slot);
int mrgcn_complex_typed_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                             const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *order,
                             const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                             int64_t num_work, const int32_t *q_tiles, const int64_t *cand_ptr,
                             const int32_t *cand_idx, int64_t max_slot, const int64_t *excl_ptr,
                             const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                             int64_t *out_idx, float *out_score, void *stream);

/* Graph-capturable Adam (torch.optim.Adam(capturable=True) semantics): the step counter and the
 * bias corrections live in device memory, so a captured epoch replays with the right step.
 * mrgcn_adam_bias_f32: ++*step_dev; bc_dev[0] = 1 - beta1^step, bc_dev[1] = sqrt(1 - beta2^step).
 * mrgcn_adam_step_dev_f32: mrgcn_adam_step_f32 reading the corrections from bc_dev. */
/* mrgcn_adam_step_f32 / _dev_f32 (weight_decay = 0) on a parameter of `nrows` rows of `rowlen` floats
 * (the node-major basis table: nrows = N, rowlen = B*F; float4 accesses when rowlen % 4 == 0) whose gradient was produced
 * row-sparse (mrgcn_basis_mix_bwd_f32 with node_cur): rows with row_ever = 0 and row_cur = 0 are not
 * touched (g = m = v = 0: Adam's update is the identity), rows with row_ever = 1, row_cur = 0 are
 * updated with g = 0 without reading grad, rows with row_cur = 1 take grad and are marked in row_ever
 * (caller keeps row_ever across steps, zero-initialised).  `bc_dev` nullable (then `step` >= 1 is used). */
int mrgcn_adam_step_rows_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                             int64_t nrows, int32_t rowlen, const uint8_t *row_cur, uint8_t *row_ever,
                             float lr, float beta1, float beta2, float eps, int64_t step,
                             const float *bc_dev, const float *grad_scale, void *stream);
/* mrgcn_adam_step_f32 / _dev_f32 (weight_decay = 0) on the rows index[0 .. n_index) of a parameter of rows of `rowlen`
 * floats, the gradient of row index[c] in row c of a COMPACT gradient (`grad`: [n_index, ld_grad]); every other row is
 * left alone.  For the literal (R*N) x F operand of a featureless layer without bases (graph.py:69-75: weight_I is the
 * operand of torch.mm(A, .)): the autograd of that product (SparseAddmmBackward) puts gradient on the rows that are
 * columns of A only — the plan's compact columns (MRGCN_ARR_ULCOL), for every label set — so the other rows keep zero
 * moments and never move.  `index` holds distinct rows; rowlen, ld_grad multiples of 4; 16-byte aligned arrays. */
int mrgcn_adam_step_index_rows_f32(float *param, const float *grad, int64_t ld_grad, float *exp_avg,
                                   float *exp_avg_sq, const int32_t *index, int64_t n_index, int32_t rowlen, float lr,
                                   float beta1, float beta2, float eps, int64_t step, const float *bc_dev,
                                   const float *grad_scale, void *stream);
/* The same update with the gradient formed on the fly: the backward called mrgcn_basis_mix_bwd_f32 with dV = NULL
 * (flags, dcomp and ||dV||^2 only) and this call rebuilds every live node's block from its dM rows,
 *     dV[j][b][f] = sum_{live c of j} comp[r_c][b] * dM[c][f]        (the sums mrgcn_basis_mix_bwd_f32 forms, bit for bit),
 * inside the Adam pass: the gradient tensor of the node table is never written nor read.  `comp` must hold the
 * coefficients the backward saw (a snapshot when the optimizer updates them first).  Shapes:
 * mrgcn_adam_rows_fused_supported (B <= 64, F <= 16, B*F % 4 == 0, R*B*4 <= 64 KB). */
int32_t mrgcn_adam_rows_fused_supported(const mrgcn_plan_t *plan, int32_t B, int32_t F);
int mrgcn_adam_step_rows_fused_f32(const mrgcn_plan_t *plan, const float *dM, int64_t ldM, const uint8_t *col_live,
                                   const float *comp, int32_t B, int32_t F, float *param, float *exp_avg,
                                   float *exp_avg_sq, const uint8_t *row_cur, uint8_t *row_ever, float lr,
                                   float beta1, float beta2, float eps, int64_t step, const float *bc_dev,
                                   const float *grad_scale, void *stream);
int mrgcn_adam_bias_f32(int64_t *step_dev, float beta1, float beta2, float *bc_dev, void *stream);
int mrgcn_adam_step_dev_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                            int64_t n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, const float *bc_dev, const float *grad_scale,
                            void *stream);

/* ---- modality encoders: the dense step in front of the graph path ----------------------
 * Fused literal MLP + gate + masked scatter (mrgcn/models/perceptron.py:6-46 with p_dropout = 0 or in eval
 * mode; mrgcn/models/mrgcn.py:285-303):
 *     XF[rows[i], offset : offset + dims[L]] = gate[0] * MLP(X[i, 0:dims[0]]),   MLP = L x (Linear -> ReLU)
 * dims: HOST array of L + 1 widths (1..16); W / b: HOST arrays of L DEVICE pointers, W[l] is
 * [dims[l+1]][dims[l]] (nn.Linear layout), b[l] nullable; rows: nullable int64 [n] (NULL = row i).
 * The backward ACCUMULATES into dW[l] / db[l] / dgate (caller zeroes them). */
int32_t mrgcn_mlp_fused_supported(int32_t L, const int32_t *dims);
int mrgcn_mlp_gate_scatter_fwd_f32(int32_t L, const int32_t *dims, const float *const *W, const float *const *b,
                                   const float *X, int64_t ldx, int64_t n, const float *gate,
                                   const int64_t *rows, float *XF, int64_t ldxf, int32_t offset, void *stream);
int mrgcn_mlp_gate_scatter_bwd_f32(int32_t L, const int32_t *dims, const float *const *W, const float *const *b,
                                   const float *X, int64_t ldx, int64_t n, const float *gate,
                                   const int64_t *rows, const float *dXF, int64_t ldxf, int32_t offset,
                                   float *const *dW, float *const *db, float *dgate, void *stream);
/* Dense product on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32), the building block of the
 * `pre_fc -> ReLU -> fc` heads (mrgcn/models/imagecnn.py:31-41, transformer.py:29-38) and of the TCNN
 * (temporal_cnn.py:6-156):   C = epilogue(alpha * op(A) . op(B)),  epilogue: + bias[N], ReLU, * (mask > 0).
 *   amode 0: A[m*lda + k]   1: A[k*lda + m]   2: Conv1d im2col of x[b][ci][t] (m = b*Tout + t, k = ci*KW + kw)
 *         3: the transpose of mode 2 (m = ci*KW + kw, k = b*Tout + t)
 *   bmode 0: B[k*ldb + n]   1: B[n*ldb + k]   2: y[b][n][t] read as [k = b*Tout + t][n]
 *   cmode 0: C[m*ldc + n]   2: y[b][n][t], m = b*Tout + t
 *   conv_geom (HOST, modes 2 / 3): {Cin, Tin, KW, pad, Tout, Cout}.  mask: nullable, addressed like C.
 * Products with few output tiles and a long reduction (the convolutions' dW) split K over the grid: C (dense,
 * ldc == N) is zeroed and the partial tiles are added with float atomics — the result is exact to the last bits only
 * up to the order of those adds. */
int mrgcn_gemm_f32(int32_t amode, int32_t bmode, int32_t cmode, int32_t M, int32_t N, int32_t K, const float *A,
                   int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, const float *bias,
                   int32_t relu, const float *mask, float alpha, const int32_t *conv_geom, void *stream);
/* The same product on the bf16 matrix cores (the bf16 pipeline, BASELINE config 3): operands and result stay fp32 in
 * memory; tiles are rounded to bf16 (nearest even) as they are staged, v_mfma_f32_16x16x32_bf16, fp32 accumulation.
 * Shapes outside the tiled form's limits run the exact fp32 element-loader kernel. */
int mrgcn_gemm_bf16mm_f32(int32_t amode, int32_t bmode, int32_t cmode, int32_t M, int32_t N, int32_t K, const float *A,
                          int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, const float *bias,
                          int32_t relu, const float *mask, float alpha, const int32_t *conv_geom, void *stream);
/* out[n] = sum_m X[m*ld + n]  (bias gradients) */
int mrgcn_colsum_f32(const float *X, int64_t ld, int32_t M, int32_t N, float *out, void *stream);

/* The elementwise half of a TCNN block (temporal_cnn.py:6-156: Conv1d -> BatchNorm1d -> ReLU [-> MaxPool1d(k, k) |
 * AdaptiveMaxPool1d(n)]) in one pass over the convolution's output x [B][C][T]:
 *     y[b][c][to] = max_{t in window(to)} relu(gamma[c] (x[b][c][t] - mean[c]) / sqrt(var[c] + eps) + beta[c])
 * pool_kind 0: none (Tout = T), 1: MaxPool1d(pool_arg, stride pool_arg), 2: AdaptiveMaxPool1d(pool_arg).
 * training != 0: mean / var (biased) are the batch statistics, computed and written by the call; otherwise they are
 * read (running statistics).  argmax [B][C][Tout] (needed when pooled) keeps the winning position for the backward.
 * Backward: dz is a [B][C][T] workspace that only adaptive pooling uses (overlapping windows; NULL otherwise);
 * dgamma / dbeta are written; dx = d loss / d x.
 * workspace: mrgcn_bn_workspace_bytes(C) bytes (fp64 partial sums of the per-channel reductions; forward: training only). */
int32_t mrgcn_pool_out_len(int32_t pool_kind, int32_t pool_arg, int32_t T);
size_t mrgcn_bn_workspace_bytes(int32_t C);
int mrgcn_bn_relu_pool_fwd_f32(const float *x, int32_t B, int32_t C, int32_t T, const float *gamma,
                               const float *beta, float eps, int32_t training, float *mean, float *var,
                               int32_t pool_kind, int32_t pool_arg, float *y, int32_t *argmax, void *workspace,
                               void *stream);
/* nn.BatchNorm1d's running statistics after a training-mode forward over n = B * T values per channel:
 * running = (1 - momentum) running + momentum stat, the (biased) batch variance scaled by n / (n - 1). */
int mrgcn_bn_running_stats_f32(const float *mean, const float *var, int32_t C, int64_t n, float momentum,
                               float *running_mean, float *running_var, void *stream);
/* out[c] = sum over (b, t) of x[b][c][t] — the bias gradient of a Conv1d (torch: dy.sum(dim=(0, 2))); fp64 sums per
 * block, one float atomic per block into the zeroed out. */
int mrgcn_channel_sum_f32(const float *x, int32_t B, int32_t C, int32_t T, float *out, void *stream);
int mrgcn_bn_relu_pool_bwd_f32(const float *x, const float *y, const float *dy, const int32_t *argmax, int32_t B,
                               int32_t C, int32_t T, const float *gamma, const float *mean, const float *var,
                               float eps, int32_t training, int32_t pool_kind, int32_t pool_arg, float *dz,
                               float *dx, float *dgamma, float *dbeta, void *workspace, void *stream);
/* the same, and dx_chan_sum[c] (nullable) = sum over (b, t) of dx[b][c][t]: the bias gradient of the Conv1d in front of
 * the block, taken inside the pass that writes dx (float atomics, one per (b, c) row) instead of another pass over it */
int mrgcn_bn_relu_pool_bwd_sum_f32(const float *x, const float *y, const float *dy, const int32_t *argmax, int32_t B,
                               int32_t C, int32_t T, const float *gamma, const float *mean, const float *var,
                               float eps, int32_t training, int32_t pool_kind, int32_t pool_arg, float *dz,
                               float *dx, float *dgamma, float *dbeta, float *dx_chan_sum, void *workspace, void *stream);

/* ---- mini-batch frontier on the resident CSR of the stacked adjacency ---------------------
 * Replaces, per layer of a batch, the host loops of mrgcn/data/batch.py:185-263 (`A[sample_idx]`,
 * getNeighboursSparse :233-249, getAdjacencyNodeColumnIdx :251-256 + sliceSparseCOO :258-270).  indptr / indices:
 * int64 CSR of A (N x R*N) in HBM; sample: int64 [n_sample] row ids.  No allocation inside: the caller provides the
 * workspace and — after reading the two sizes row_off[n_sample] (entries) and node_pos[num_nodes] (neighbours) —
 * the outputs.
 *   count: row_off [n_sample+1] exclusive scan of the rows' lengths; node_pos [num_nodes+1] exclusive scan of
 *          "node j is the source node of some entry of these rows".
 *   emit : COO of the slice in the order A[sample].nonzero() has (row-major, stored column order): out_row = position
 *          in `sample`, out_col = global column, out_val (nullable) = the stored value as float32 or truncated to
 *          int8 (the reference's boundary cast); out_col_sliced (nullable) = r * n_neighbours + node_pos[j]: the
 *          column sliceSparseCOO gives the entry; neighbours (nullable) [n_neighbours] ascending node ids.
 *          (A slice without entries writes nothing: its output pointers are not looked at.) */
size_t mrgcn_frontier_workspace_bytes(int64_t num_nodes, int64_t n_sample);
int mrgcn_frontier_count(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, const int64_t *sample,
                         int64_t n_sample, int64_t *row_off, int32_t *node_pos, void *workspace,
                         size_t workspace_bytes, void *stream);
int mrgcn_frontier_emit(const int64_t *indptr, const int64_t *indices, const float *data, int64_t num_nodes,
                        const int64_t *sample, int64_t n_sample, const int64_t *row_off, const int32_t *node_pos,
                        int64_t n_neighbours, int32_t value_dtype, int64_t *out_row, int64_t *out_col,
                        void *out_val, int64_t *out_col_sliced, int64_t *neighbours, void *stream);

/* ---- literal encodings of a mini-batch on the device (reference mrgcn/data/batch.py:272-316 mksubset, :25-68 pad_ /
 * to_dense_, data/utils.py:109-152) -----------------------------------------------------------------------------------
 * Every encoding set is resident in HBM; per batch the caller runs `rows` for all sets at once, reads its stats back
 * ONCE, allocates, then gathers.  Nothing allocates inside; no atomics anywhere (bitwise deterministic outputs).
 *   rows        : for every set (one block each; descriptors passed by value, 32 per launch) the members the batch's
 *                 nodes carry.  out_pos[set, i] = ascending batch positions p with member_of_node[nodes[p]] >= 0;
 *                 out_member[set, i] = the selected members in ascending member order (the reference's
 *                 np.in1d(nodes_idx, common)); both [num_sets, n_nodes] int64, the first count entries of a row valid.
 *                 stats [num_sets + 1, 4] int64: per set (count, max seq_length, max width, max extent) of the selected
 *                 members, then (node ids outside [0, num_nodes): > 0 if any, 0, 0, 0).  An unordered set (node ids
 *                 not ascending in member order) needs member_flags, one int32 per member, private to the call.
 *   gather_rows : dst[i, :] = src[clamp(index[i]), :] for `count` rows of `row_bytes`, moved in pieces of `unit` bytes
 *                 (1, 2, 4, 8 or 16; must divide row_bytes and both pointers); 32 gathers per launch.
 *   tokens      : out [k, L] int64 (16-byte aligned): member members[i]'s tokens tokens[offsets[m] .. offsets[m+1])
 *                 left-aligned in row i, pad_symbol beyond its length and where a token is -1.  tokens holds one
 *                 readable entry past the last member.  Members longer than L are the caller's error to raise.
 *   csr_dense   : out [k, C, L] float32 (16-byte aligned): row r of member members[i] is the CSR row
 *                 row_ptr[m * (C + 1) + r] .. row_ptr[m * (C + 1) + r + 1] of (values, columns) with sorted, distinct
 *                 columns; element (i, r, t) = the entry of column t or 0.  Every element is stored exactly once.
 *                 values / columns hold one readable entry past the last entry. */
typedef struct {
  const int32_t *member_of_node; /* [num_nodes] member row of every node, -1: none */
  const int64_t *seq_lengths;    /* [max(members, 1)] */
  const int64_t *widths;         /* [max(members, 1)] length along the padded axis, or NULL (0) */
  const int64_t *extents;        /* [max(members, 1)] 1 + the largest used position, or NULL (0) */
  int32_t *member_flags;         /* [members] workspace of an unordered set, or NULL */
  int64_t members;
  int32_t ordered;               /* node ids ascend in member order: the batch order is the member order */
  int32_t reserved;
} mrgcn_literal_set;
typedef struct {
  const void *src;
  void *dst;
  const int64_t *index; /* [count] rows of src */
  int64_t count;
  int64_t row_bytes;
  int64_t src_rows;
  int32_t unit;
  int32_t reserved;
} mrgcn_literal_gather;
int mrgcn_literal_rows(const mrgcn_literal_set *sets, int32_t num_sets, int64_t num_nodes, const int64_t *nodes,
                       int64_t n_nodes, int64_t *out_member, int64_t *out_pos, int64_t *stats, void *stream);
int mrgcn_literal_gather_rows(const mrgcn_literal_gather *gathers, int32_t num_gathers, void *stream);
int mrgcn_literal_tokens(const int64_t *tokens, const int64_t *offsets, const int64_t *members, int64_t k, int64_t L,
                         int64_t pad_symbol, int64_t *out, void *stream);
int mrgcn_literal_csr_dense(const float *values, const int32_t *columns, const int64_t *row_ptr,
                            const int64_t *members, int64_t k, int64_t C, int64_t L, float *out, void *stream);

/* ---- node dropout on the device (mrgcn/models/rgcn.py:78-84) -----------------------------------
 * The node masks of one step: masks[l * ld + i], l < layers, i < n, is 0 when node i of layer (layer0 + l) is dropped
 * and `keep_value` (the caller's fp32 1 / (1 - p)) otherwise.  The draw is Philox4x32-10: the four nodes 4g .. 4g+3
 * take the four output words of counter (g, layer0 + l, position lo, position hi) under key (seed lo, seed hi), and a
 * node is dropped when its word is below `threshold` = floor(p * 2^32) (0: nobody, 2^32: everybody) — a mask depends
 * on (seed, position, layer, node) only, never on the launch.  `state_dev` is two int64 in DEVICE memory, {seed,
 * position}, read by the draw; with `advance` a one-thread launch behind the draw adds one to the position, in stream
 * order — a captured step therefore draws new masks at every replay.  `masks` on a 16-byte base, n <= 2^32, and
 * ld % 4 == 0 when layers > 1.  (mrgcn_amd/host.py: node_dropout_mask is the bit-exact host mirror.) */
int mrgcn_node_dropout_draw_f32(float *masks, int64_t ld, int64_t n, int32_t layers, int32_t layer0,
                                int64_t threshold, float keep_value, int64_t *state_dev, int32_t advance,
                                void *stream);
/* Y[r, 0:F] *= m[r] in place, r < rows, on rows with leading dimension ld; columns F .. ld of a row are left as
 * they are.  16-byte accesses when ld % 4 == 0 or ld == F (and a 16-byte base). */
int mrgcn_row_scale_f32(float *Y, int64_t ld, int64_t rows, int32_t F, const float *m, void *stream);
/* The backward twin on the row-live form: out[r, 0:F] = m[r] * dY[r, 0:F] for the rows with row_flags[r] != 0 (NULL:
 * all rows); the other rows of dY are not read, and their rows of `out` are zeroed (`zero_dead`) or, without it, hold
 * nothing a reader may rely on: each is left unwritten or zeroed, whichever the 16-byte store it shares with a live
 * row makes cheaper (a gradient whose consumer goes by the same flags).  out may be dY. */
int mrgcn_row_scale_live_f32(const float *dY, int64_t ld_dY, int64_t rows, int32_t F, const float *m,
                             const uint8_t *row_flags, int32_t zero_dead, float *out, int64_t ld_out, void *stream);

/* ---- edge dropout on the device (csrc/edge_dropout.hip; Schlichtkrull et al. 2018, §5) --------------------------
 * Rewrites the three value arrays of the overlay `child` from its parent's.  Entry (row i, source node j, relation r)
 * takes word x of the Philox4x32-10 block of counter (i, j, r | layer << 24, position lo) under key (seed lo,
 * seed hi ^ position hi ^ 0x45444745): below floor(rates[r] * 2^32) the entry is dropped and holds 0.0f, otherwise it
 * holds a * keep_r in one fp32 multiply, keep_r = 1.0f / (1.0f - rates[r]) (`rescale` = 0: keep_r = 1).  `rates`: num_relations
 * floats in DEVICE memory, each in [0, 1) (rate 0 leaves the parent's bits).  `state_dev`: the int64 pair {seed, position}
 * in device memory; with `advance` the one-thread launch of node dropout moves the position behind the draw (the last
 * layer's draw of a step).  The result depends on (seed, position, layer, i, j, r, rates[r]) only — never on the grid or
 * on which of the three orders an entry is met in.  Stream ordered, allocation free, capturable.  Refused: a plan that
 * is no overlay, num_relations >= 2^24, layer outside 0 .. 255.  (mrgcn_amd/host.py: edge_dropout_values is the host
 * mirror.) */
int mrgcn_edge_dropout_draw_f32(mrgcn_plan_t *child, const float *rates, int32_t rescale, int64_t *state_dev,
                                int32_t layer, int32_t advance, void *stream);

/* ---- keyed, filtered negatives for the link-prediction decoder (csrc/lp_negatives.hip) ----------------------------
 * The reference corrupts 20 % of a batch's facts with nodes of the batch and never checks a draw against the known
 * facts (mrgcn/tasks/link_prediction.py:247-264; mrgcn_corrupt_triples_i64 above is that scheme).  Here every fact
 * i < n gets `rate` negatives, negative j of fact i in row k = i * rate + j of `out` ([n * rate, 3]): a copy of the
 * fact whose head or tail is replaced by a candidate.  `side`: 0 = bit 0 of word z of attempt 0's block decides (set:
 * the head), 1 = tails only, 2 = heads only.  Attempt a = 0 .. MRGCN_NEG_MAX_ATTEMPTS - 1 takes the Philox4x32-10 block
 * of counter (k lo 32, (k >> 32) | (a << 24), position lo, position hi) under key (seed lo, seed hi ^ 0x4E454753), forms
 * h = x << 32 | y and picks candidate c = (h * n_cand) >> 64: cand[c], or c itself when `cand` is NULL.  The attempt is
 * refused when the pick equals the end it replaces, and — with `known_keys`, n_known ascending keys — when the key of the
 * corrupted triple is among them: key(s, p, o) = (s * num_relations + p) * num_nodes + o on GLOBAL ids, an id of `facts`
 * / `cand` being mapped through `to_global` when that is given (a batch's local ids).  The first accepted attempt is
 * written and unresolved[k] (nullable, [n * rate]) = 0; when all are refused the last draw stands and unresolved[k] = 1.
 * `state` is two int64 in DEVICE memory, {seed, position}, read by the draw; a one-thread launch behind it adds one to
 * the position in stream order, so a captured call draws new negatives at every replay.  One thread per negative, no
 * atomics: the result depends on the arguments and the state only.  n * rate < 2^56 (and < 2^39: one grid),
 * num_nodes * num_relations * num_nodes < 2^63; the ids in facts / cand / to_global are the caller's to keep in range.
 * (mrgcn_amd/host.py: negatives_draw is the bit-exact host mirror.) */
#define MRGCN_NEG_MAX_ATTEMPTS 8
int mrgcn_negatives_draw_i64(const int64_t *facts, int64_t n, int32_t rate, const int64_t *cand, int64_t n_cand,
                             const int64_t *to_global, const int64_t *known_keys, int64_t n_known, int64_t num_nodes,
                             int64_t num_relations, int32_t side, int64_t *state, int64_t *out, uint8_t *unresolved,
                             void *stream);
/* The type-constrained draw (Krompass, Baier, Tresp, "Type-Constrained Representation Learning in Knowledge Graphs",
 * ISWC 2015): mrgcn_negatives_draw_i64's contract word for word — the same counter, key and tag, the same side bit from
 * attempt 0's word z, the same refusals, flags and state —, with the candidates of the fact's relation p and the drawn
 * side in place of (cand, n_cand): cand_ptr (int64 [2 num_relations + 1], rising) and cand_idx (int32, every list
 * ascending and duplicate free) are a CSR over 2 num_relations slots, slot 2 p the relation's tail candidates (its
 * range), slot 2 p + 1 its head candidates (its domain).  The pick is cand_idx[cand_ptr[slot] + ((h * len) >> 64)], len
 * the slot's length: with every slot 0 .. num_nodes - 1 the output equals mrgcn_negatives_draw_i64's (cand NULL, n_cand
 * = num_nodes) bit for bit.  A slot whose only node is the end it replaces is refused at all attempts: the draw stands
 * and the negative is flagged.  An empty slot (or a relation outside [0, num_relations)) reads nothing: the fact's own
 * end stands, flagged; the caller keeps such facts out (tasks.link_prediction.NegativeSampler raises).  The lists hold
 * GLOBAL ids: there is no to_global.  (mrgcn_amd/host.py: negatives_draw(typed=...) is the bit-exact host mirror.) */
int mrgcn_negatives_draw_typed_i64(const int64_t *facts, int64_t n, int32_t rate, const int64_t *cand_ptr,
                                   const int32_t *cand_idx, const int64_t *known_keys, int64_t n_known,
                                   int64_t num_nodes, int64_t num_relations, int32_t side, int64_t *state, int64_t *out,
                                   uint8_t *unresolved, void *stream);

/* ---- grouped DistMult loss over a fact's keyed negatives (csrc/distmult_group.hip) --------------------------------
 * The decoder of mrgcn/tasks/link_prediction.py:645-665 (scores) and :550-554 (loss) for triples in the layout of
 * mrgcn_negatives_draw_i64's sampler: rows [0, n) the facts, row n + i * rate + j negative j of fact i, which has fact
 * i's predicate and one of its ends.  A negative whose column 0 differs from the fact's subject counts as
 * head-corrupted, any other as tail-corrupted (so a negative equal to its fact is a tail negative with the fact's own
 * object).  A wave owns a group: the fact's three rows are read once, one row per negative.
 * _supported: 1 when the group kernels take the shape — rows of whole 16-byte pieces (H % 4 == 0, H <= 256, ldE / ldR
 *   multiples of 4, 16-byte aligned bases), ids and n * (1 + rate) below 2^31 —, else 0 (the caller scores the flat
 *   triples instead).
 * _fwd: scores [n (1 + rate)] (bit for bit mrgcn_distmult_score_f32's on the same rows), dscores = dloss / dscore in
 *   the same layout and *loss WRITTEN: block partials added in a fixed order, no float atomic.  loss_kind
 *   MRGCN_GROUP_LOSS_BCE: BCEWithLogitsLoss(pos_weight), mean over all n (1 + rate) scores — term
 *   (1 - y) x + (1 + (w - 1) y) (log1p(exp(-|x|)) + max(-x, 0)), gradient ((1 + (w - 1) y) sigmoid(x) - w y) / count.
 *   MRGCN_GROUP_LOSS_SOFTMAX: the mean over facts of -log softmax of the fact's score among its 1 + rate scores
 *   (pos_weight unread).  workspace: mrgcn_distmult_group_fwd_workspace() bytes.
 * _bwd: dE / dRel += the gradients for dscores times *upstream (a float in DEVICE memory: no host read).  Without the
 *   orders (all three NULL) everything is added by row atomics (mini-batches).  With the three orders of the FACTS by
 *   subject / predicate / object (SortedTriples) the group pass stores three rows per fact to scratch, which are summed
 *   along the orders, and the negatives' own rows are summed along a radix sort by their changed end over the bits of
 *   num_nodes - 1; workspace then: 16-byte aligned, mrgcn_distmult_group_bwd_workspace(n, rate, H) bytes (-1 for sizes
 *   it does not take).  Float atomics at run ends: not bit-reproducible.  No host synchronisation; capturable. */
#define MRGCN_GROUP_LOSS_BCE 0
#define MRGCN_GROUP_LOSS_SOFTMAX 1
int32_t mrgcn_distmult_group_supported(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                       int64_t num_nodes, int64_t num_relations, int64_t n, int32_t rate);
int64_t mrgcn_distmult_group_fwd_workspace(void);
int mrgcn_distmult_group_fwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                 const int64_t *triples, int64_t n, int32_t rate, int32_t loss_kind, float pos_weight,
                                 float *scores, float *dscores, float *loss, void *workspace, int64_t workspace_bytes,
                                 void *stream);
int64_t mrgcn_distmult_group_bwd_workspace(int64_t n, int32_t rate, int32_t H);
int mrgcn_distmult_group_bwd_f32(const float *E, int64_t ldE, const float *Rel, int64_t ldR, int32_t H,
                                 const int64_t *triples, int64_t n, int32_t rate, const float *dscores,
                                 const float *upstream, int64_t num_nodes, const int64_t *order_s,
                                 const int64_t *order_p, const int64_t *order_o, float *dE, int64_t lddE, float *dRel,
                                 int64_t lddR, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- 1-vs-all softmax decoder on the matrix cores (csrc/lp_all.hip) -----------------------------------------------
 * Every query vector Q[q] scored against ALL rows of the candidate table E under a softmax cross-entropy:
 * x[q][c] = Q[q] . E[c], loss = (1/m) sum_q (log sum_c exp x[q][c] - x[q][target[q]]) — the objective of Kadlec, Bajgar,
 * Kleindienst ("Knowledge Base Completion: Baselines Strike Back", 2017), Lacroix, Usunier, Obozinski ("Canonical
 * Tensor Decomposition for Knowledge Base Completion", ICML 2018) and Ruffinelli, Broscheit, Gemulla ("You CAN Teach an
 * Old Dog New Tricks! On Training Knowledge Graph Embeddings", ICLR 2020); the reference has the sampled BCE only
 * (mrgcn/tasks/link_prediction.py:645-665, :550-554), so the papers stand where a reference call site would.  The
 * unit does not know the scorer: the caller builds the query vectors (tasks/link_prediction.py: pair_vectors).  The
 * [m, N] score matrix is never stored; all three kernels compute 64 x 64 score tiles with v_mfma_f32_16x16x4_f32
 * (exact fp32).  Q [m, H] and E [N, H] are float32 with row strides ldQ / ldE; target int64 [m], 0 <= target < N (not
 * checked here).
 * _supported: 1 when the kernels take the shape — H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31, ldQ / ldE >= H and
 *   multiples of 4, 16-byte aligned bases —, else 0 (the caller materialises the scores instead).
 * _chunk: the candidates per forward chunk: with fewer than 256 query tiles of 64 the forward cuts the candidates
 *   into chunks of this many over gridDim.y and merges the chunks' (max, sum) pairs in chunk order.
 * _workspace: the bytes _fwd needs (-1 for sizes it does not take); _bwd needs none.
 * _fwd: lse [2 m]: lse[q] = log sum_c exp x[q][c] by an online max / sum, rounded to float32 from the float64 it is
 *   merged in, and lse[m + q] what that rounding left (the backward subtracts both: exp(x - lse) then does not carry
 *   half an ulp of lse); xt [m] = x[q][target[q]] from the same tile arithmetic (lse - xt >= 0 in bits when N == 1);
 *   *loss WRITTEN: lse - xt summed as float64 in a fixed order, divided by m and rounded once.
 * _bwd: lse as _fwd wrote it ([2 m]); with G[q][c] = (exp(x[q][c] - lse[q]) - [c == target[q]]) * *gl / m (gl: a float in DEVICE memory, no host
 *   read), dQ = G . E and dE = G^T . Q are WRITTEN (every output row has one owning block; nothing is added); either
 *   may be NULL and its kernel is skipped.  Both recompute the scores.
 * No float atomics: equal inputs give equal bits.  Stream ordered, no allocation, capturable. */
int32_t mrgcn_lp_all_supported(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N,
                               int32_t H);
int64_t mrgcn_lp_all_chunk(void);
int64_t mrgcn_lp_all_workspace(int64_t m, int64_t N, int32_t H);
int mrgcn_lp_all_fwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                         const int64_t *target, float *lse, float *xt, float *loss, void *workspace,
                         int64_t workspace_bytes, void *stream);
int mrgcn_lp_all_bwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                         const int64_t *target, const float *lse, const float *gl, float *dQ, int64_t lddQ, float *dE,
                         int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- KvsAll decoder: multi-hot BCE against all candidates, label smoothed (csrc/lp_kvsall.hip) ---------------------
 * Every DISTINCT query vector Q[q] scored against ALL rows of the candidate table E under a binary cross-entropy whose
 * target marks all known answers of the query: x[q][c] = Q[q] . E[c], Y'[q][c] = (1 - eps) [c in ans(q)] + eps / N,
 * loss = the mean over the m N scores of bce_with_logits(x, Y') — the "1-N scoring" of Dettmers, Minervini, Stenetorp,
 * Riedel ("Convolutional 2D Knowledge Graph Embeddings", AAAI 2018) with the label smoothing of Szegedy et al.
 * ("Rethinking the Inception Architecture for Computer Vision", CVPR 2016); the reference has the sampled BCE only
 * (mrgcn/tasks/link_prediction.py:645-665, :550-554), so the papers stand where a reference call site would.  The unit
 * does not know the scorer (tasks/link_prediction.py: pair_vectors builds Q).  The [m, N] scores are never stored and
 * no label enters the dense kernels (the 64 x 64 MFMA tiles of csrc/lp_all.hip):
 *   sum_c bce = sum_c softplus(x) - (eps / N) sum_c x - (1 - eps) sum_{c in ans(q)} x,
 *   d / dx    = sigmoid(x) - eps / N - (1 - eps) [c in ans(q)],
 * the last term of each taken along the lists of the nnz (query, answer) pairs.  Q [m, H] and E [N, H] are float32 with row
 * strides ldQ / ldE.  ans_ptr int64 [m + 1] / ans_idx int32 [nnz]: the answers of query q are
 * ans_idx[ans_ptr[q] .. ans_ptr[q + 1]), ascending, 0 <= answer < N (not checked here); an empty list is legal.
 * cand_ptr int64 [N + 1] / cand_qry int32 [nnz]: the transposed lists — the queries that have candidate c as an answer,
 * ascending.
 * _supported: mrgcn_lp_all_supported's rule; _workspace: the bytes _fwd needs (-1 for sizes it does not take); _bwd
 *   needs none.
 * _fwd: per_query [m] (may be NULL) = sum_c bce of the query, *loss WRITTEN: the per-query sums added as float64 in a
 *   fixed order, divided by m N and rounded once.  The softplus is max(x, 0) + log1p(exp(-|x|)).
 * _bwd: with G[q][c] = (sigmoid(x[q][c]) - eps / N) * *gl / (m N) (gl: a float in DEVICE memory, no host read),
 *   less (1 - eps) * *gl / (m N) on the listed pairs (in the gradient tile itself, as eps (1 - 1 / N) - sigmoid(-x):
 *   along ans_* for dQ, along cand_* for dE), dQ = G . E and dE = G^T . Q are WRITTEN (every output row has one owning block;
 *   nothing is added).  dQ / dE may be NULL (skipped; cand_* may then be NULL with dE, ans_* with dQ); lddQ / lddE
 *   >= H.
 * label_smoothing outside [0, 1) is an argument error.  No float atomics: equal inputs give equal bits.  Stream
 * ordered, no allocation, capturable. */
int32_t mrgcn_lp_kvsall_supported(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N,
                                  int32_t H);
int64_t mrgcn_lp_kvsall_workspace(int64_t m, int64_t N, int32_t H);
int mrgcn_lp_kvsall_fwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                            const int64_t *ans_ptr, const int32_t *ans_idx, double label_smoothing, float *per_query,
                            float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int mrgcn_lp_kvsall_bwd_f32(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H,
                            const int64_t *ans_ptr, const int32_t *ans_idx, const int64_t *cand_ptr,
                            const int32_t *cand_qry, double label_smoothing, const float *gl, float *dQ, int64_t lddQ,
                            float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- bf16 matrix-core arithmetic for the two all-candidates decoders (csrc/lp_tile.hpp: the bf16 tile) -------------
 * The _bf16 entries are the _f32 entries above with the scores and the second product on v_mfma_f32_16x16x32_bf16.
 * With ~ = rounded to bf16, nearest even:  x[q][c] = Q~[q] . E~[c], the products (exact in fp32) summed in fp32;
 * everything after the scores — the online (max, sum), lse and its remainder, softplus, the float64 merges, the loss —
 * is the _f32 entries' code, unchanged; the gradient tile G is formed in fp32 as there and rounded to bf16 ONCE, as it
 * becomes the operand of dQ = G~ . E~ and dE = G~^T . Q~ (fp32 sums, fp32 outputs): the gradient of the loss as
 * computed, the operands' rounding passed straight through.
 * Q [m, H] and E [N, H] are bf16 TABLES (raw uint16_t rows; mrgcn_cast_rows_bf16 with ldDst = Hp makes them, once per
 * forward): row strides ldQ / ldE in elements with ld % 32 == 0 and ld >= Hp = 32 ceil(H / 32), 16-byte aligned bases,
 * ZEROS in [H, Hp) (not checked: what stands there enters every score).  H % 4 == 0, 4 <= H <= 256, 1 <= m, N < 2^31;
 * outputs are float with lddQ / lddE >= H.  _supported_bf16 is that rule (1 / 0).  The workspaces are those of the
 * _f32 entries (mrgcn_lp_all_workspace, mrgcn_lp_kvsall_workspace), lse / xt / per_query / loss / gl as there.  One
 * owning block per output row, no float atomics: equal inputs give equal bits.  Stream ordered, no allocation,
 * capturable. */
int32_t mrgcn_lp_all_supported_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE,
                                    int64_t N, int32_t H);
int mrgcn_lp_all_fwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                          int32_t H, const int64_t *target, float *lse, float *xt, float *loss, void *workspace,
                          int64_t workspace_bytes, void *stream);
int mrgcn_lp_all_bwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                          int32_t H, const int64_t *target, const float *lse, const float *gl, float *dQ, int64_t lddQ,
                          float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream);
int32_t mrgcn_lp_kvsall_supported_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE,
                                       int64_t N, int32_t H);
int mrgcn_lp_kvsall_fwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                             int32_t H, const int64_t *ans_ptr, const int32_t *ans_idx, double label_smoothing,
                             float *per_query, float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int mrgcn_lp_kvsall_bwd_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                             int32_t H, const int64_t *ans_ptr, const int32_t *ans_idx, const int64_t *cand_ptr,
                             const int32_t *cand_qry, double label_smoothing, const float *gl, float *dQ, int64_t lddQ,
                             float *dE, int64_t lddE, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- block-diagonal relation transform (csrc/block_xform.hip) ------------------------------------------------------
 * Schlichtkrull et al. 2018, "Modeling Relational Data with Graph Convolutional Networks", eq. 4:
 * W_r = blockdiag(Q_r[0], ..., Q_r[NB-1]), NB blocks of ki x fo = (K / NB) x (F / NB); input columns b ki .. b ki + ki - 1
 * feed output columns b fo .. b fo + fo - 1 only.  W: [R][NB][ki][fo].  Per compact column c = (j_c, r_c), f = b fo + q:
 *     Out[o(c), f] = sum_{k < ki} X[j_c, b ki + k] . W[r_c, b, k, q]
 * with o(c) = c or MPOS[c] (`operand_order` != 0) and the whole padded row written (zeros in [F, ldOut), nothing else),
 * as mrgcn_rel_transform_fwd_f32 does.  The sum runs over k rising from +0, every product and every sum rounded to
 * float32 on its own (no fused multiply-add): the result is one statement of float32 operations, equal to its numpy
 * mirror (mrgcn_amd.host.block_transform32) bit for bit.
 * Backward from dM [ncols, ldM] in plain compact order (the TRANSPOSED view's output); either output nullable:
 *     dX[j, b ki + k] = sum_{c in NPTR[j] .. NPTR[j+1]} sum_{q < fo} W[r_c, b, k, q] . dM[c, b fo + q]
 *                       (a node's columns in four consecutive runs, each added with c rising and q rising inside it, the
 *                       four partial rows added in run order; every row written, zeros for a node without a column)
 *     dW[r, b, k, q]  = sum_{c : r_c = r} X[j_c, b ki + k] . dM[c, b fo + q]
 *                       (units of 256 columns of RPERM inside one (band, relation) group write partial slabs of K fo
 *                       floats to the workspace, a second launch adds a relation's slabs in a fixed order; a relation
 *                       without columns gets zeros)
 * No float atomics: equal inputs give equal bits on every run.  X is not read when dW is NULL, W not when dX is NULL.
 * Limits (_supported): NB divides K and F, 1 <= ki, fo <= 64, K, F <= 256, K fo 4 <= 64 KB, fewer than 65536
 * relations; the calls also need ldX >= K, ldOut >= F, ldM >= F, lddX >= K.  A shape outside them, or a workspace
 * smaller than _bwd_workspace(...) floats, is MRGCN_ERR_INVALID. */
int32_t mrgcn_block_transform_supported(const mrgcn_plan_t *plan, int32_t K, int32_t F, int32_t NB);
int mrgcn_block_transform_fwd_f32(const mrgcn_plan_t *plan, const float *X, int64_t ldX, int32_t K, const float *W,
                                  int32_t NB, int32_t F, float *Out, int64_t ldOut, int32_t operand_order,
                                  void *stream);
int64_t mrgcn_block_transform_bwd_workspace(const mrgcn_plan_t *plan, int32_t K, int32_t F, int32_t NB,
                                            int32_t need_dX, int32_t need_dW); /* floats */
int mrgcn_block_transform_bwd_f32(const mrgcn_plan_t *plan, const float *dM, int64_t ldM, const float *X, int64_t ldX,
                                  int32_t K, const float *W, int32_t NB, int32_t F, float *dX, int64_t lddX, float *dW,
                                  float *workspace, int64_t workspace_floats, void *stream);

/* ---- validation and early stopping inside a replayed epoch (csrc/early_stop.hip) ---------------------------------
 * Evaluation of a label set: loss_out = mean cross-entropy of the rows logits[idx[i], :C] (max-subtracted
 * log-sum-exp, as mrgcn_softmax_xent_rows_f32), correct_out = how many of those rows have their arg-max at target[i]
 * (of equal values the lowest class wins, as Tensor.max(dim=1)), labels_out (nullable, [n]) = the arg-max of each.
 * No gradient is written.  All sums run in a fixed order without float atomics: equal inputs give equal bits.
 * n <= mrgcn_xent_eval_single_block_rows() takes one block and no workspace (NULL); more rows leave block partials
 * in `workspace` (mrgcn_xent_eval_workspace() bytes, 16-byte aligned) and a second launch adds them in block order.
 * idx may repeat rows; ld >= C. */
int64_t mrgcn_xent_eval_workspace(void);
int64_t mrgcn_xent_eval_single_block_rows(void);
int mrgcn_xent_eval_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx, const int64_t *target,
                             int64_t n, float *loss_out, int64_t *correct_out, int64_t *labels_out, void *workspace,
                             void *stream);
/* The state of tasks/utils.py::EarlyStop on the device.  Start: best_score = -1, records = best_record = 0,
 * delay / patience as constructed, stop = improved = 0. */
typedef struct {
  double best_score;   /* < 0: none yet */
  int64_t records;     /* records taken, the swallowed ones of `delay` included */
  int64_t best_record; /* which record (1 = the first) set best_score; 0 = none */
  int32_t delay;       /* records still to swallow */
  int32_t patience;
  int32_t stop;        /* latched: once set, later records change nothing */
  int32_t improved;    /* 1 iff THIS record set best_score (the flag mrgcn_snapshot_if reads) */
} mrgcn_early_stop_state;
/* One row of a float [rows, 4] ring on the device: values[k] (device floats, NULL = -1) go to row (records % rows)
 * of `ring` before the record is counted, unless `stop` is set already.  A host struct, read at the call. */
typedef struct {
  const float *values[4];
  float *ring;
  int64_t rows;
} mrgcn_metrics_row;
/* EarlyStop.record (tasks/utils.py:64-81) by one thread: the first `delay` records are swallowed; the next one sets
 * best_score and spends no patience; every later one spends one, and (double)*score + tolerance < best_score sets
 * best_score and gives patience_default back; stop = 1 when patience <= 0 after that. */
int mrgcn_early_stop_record(mrgcn_early_stop_state *state, const float *score, double tolerance,
                            int32_t patience_default, const mrgcn_metrics_row *metrics_row, void *stream);
/* mrgcn_early_stop_record (tasks/utils.py:64-81; link_prediction.py:362-364) with a row of any width: the `width`
 * contiguous device floats at `row` go to row (records % rows) of the float [rows, width] device `ring` before the
 * record is counted, unless `stop` is set already; the bookkeeping is that of mrgcn_early_stop_record. */
int mrgcn_early_stop_record_row(mrgcn_early_stop_state *state, const float *score, double tolerance,
                                int32_t patience_default, const float *row, int32_t width, float *ring, int64_t rows,
                                void *stream);
/* Copies every entry of a device table when *flag != 0 (flag NULL: always); restore != 0 copies dst -> src instead.
 * Any size and alignment.  first_block: the entries' running block count, an entry taking
 * ceil(bytes / mrgcn_snapshot_block_bytes()) blocks; n_blocks: the total. */
typedef struct {
  const void *src;
  void *dst;
  int64_t bytes;
  int64_t first_block;
} mrgcn_copy_entry;
int64_t mrgcn_snapshot_block_bytes(void);
int mrgcn_snapshot_if(const int32_t *flag, const mrgcn_copy_entry *table, int32_t n_entries, int64_t n_blocks,
                      int32_t restore, void *stream);

/* ---- mini-batch node classification: one loss launch per batch, the epoch's means (csrc/nc_batches.hip) -----------
 * Everything a training batch of node_classification.py:158-201 needs from its logits, in one pass over the rows
 * logits[idx[i], :C]: `loss` = their mean cross-entropy (float64 sum in a fixed order, rounded once); `drows`
 * (nullable: an evaluation batch, :229-256) = the compact gradient rows [n, C], bit for bit what
 * mrgcn_softmax_xent_rows_f32 writes (mrgcn_softmax_xent_bwd_* consume them unchanged); `correct` = how many rows have
 * their arg-max at target[i] and `labels` (nullable, [n]) the arg-max of each, by the rules of
 * mrgcn_xent_eval_rows_f32: strict >, so the lowest class wins ties, and a target outside [0, C) poisons the loss
 * (NaN) and reads nothing; `slot` (nullable) = two floats, {loss, (float)correct / (float)n}.
 * n <= mrgcn_xent_train_eval_single_block_rows() is ONE launch and needs no workspace (NULL); more rows leave
 * per-block parts in `workspace` (mrgcn_xent_train_eval_workspace() bytes, 16-byte aligned) that a second, one-thread
 * launch adds in block order.  No atomics: equal inputs give equal bits.  idx may repeat rows; ld >= C. */
int64_t mrgcn_xent_train_eval_workspace(void);
int64_t mrgcn_xent_train_eval_single_block_rows(void);
int mrgcn_xent_train_eval_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx,
                                   const int64_t *target, int64_t n, float *loss, float *drows, int64_t *correct,
                                   int64_t *labels, float *slot, void *workspace, void *stream);
/* The epoch's row of node_classification.py:203-204,:253-254 from the batches' slots ({loss, acc} pairs as the launch
 * above writes them, contiguous [n, 2]): row4 = {mean train loss, mean train acc, mean valid loss, mean valid acc},
 * each the float64 sum of its slots IN SLOT ORDER divided by the count and rounded once to float32 — unweighted means
 * over batches, as np.mean of the reference's lists.  n_valid == 0 (valid_slots may be NULL) writes -1 for both
 * validation values.  One thread; n_train > 0. */
int mrgcn_batch_means_f32(const float *train_slots, int64_t n_train, const float *valid_slots, int64_t n_valid,
                          float *row4, void *stream);

/* ---- mini-batch link prediction: one batch's ranks and metrics, the epoch's means (csrc/lp_batches.hip) -----------
 * test_model of ONE batch (link_prediction.py:375-422 around compute_ranks_fast :593-643 and filter_scores_ :667-689):
 * the batch's facts (int64 [num_facts, 3], batch-local ids, num_facts >= 1) ranked against the batch's own table
 * E [num_nodes, H], raw and — with the four arrays of the filter lists, all or none — filtered, from ONE pass over
 * the candidate scores.  ranks_raw / ranks_flt (nullable, int64 [2 num_facts]: tail ranks, then head ranks) are bit
 * for bit what mrgcn_distmult_ranks writes without / with the lists: the same float32 score body (sequential over h,
 * nothing contracted), the rule rank = greater + round_half_even((ties - 1) / 2) + 1, and the reference's quirk that
 * facts at positions >= num_nodes stay unscored (:611-625: truth 0, every candidate ties).  slot [8] = raw mrr, hits@1,
 * hits@3, hits@10, then the same four filtered (-1 each without lists, as test_model reports them, :383-389), each
 * half what mrgcn_rank_metrics gives for that rank vector with one part (:403-407): a float64 sum in that kernel's
 * order, rounded once.  Three launches (transpose + true scores; a block owns eight facts across all candidate tiles,
 * counts as integers in LDS, and writes its own ranks; one wave per rank type for the metrics), stream ordered, no
 * host memory, capturable, no float atomics: equal inputs give equal bits.  `workspace`: caller owned, 8-byte
 * aligned, mrgcn_distmult_batch_eval_workspace(num_nodes, H, num_facts) bytes (-1 for sizes it does not take). */
int64_t mrgcn_distmult_batch_eval_workspace(int64_t num_nodes, int32_t H, int64_t num_facts);
int mrgcn_distmult_batch_eval(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                              const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                              void *workspace, int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt,
                              float *slot, void *stream);
/* The epoch's row of the mini-batch loop from the batches' slots: row17[0] = np.mean(loss_lst) (:331) over the
 * n_loss contiguous floats of loss_slots; row17[1:9] / row17[9:17] = per column the unweighted mean over the n_train /
 * n_valid batches of their [n, 8] slots as mrgcn_distmult_batch_eval writes them (test_model :416-419; a column of -1
 * stays -1, as np.mean of the reference's list of -1).  Each value is the float64 sum of its slots IN SLOT ORDER
 * divided by the count and rounded once to float32; one thread.  score_out (nullable) = (float)(1 - mean validation
 * raw mrr), the score train_model records (:363), taken from the float64 mean.  A count of 0 (its pointer may be
 * NULL) leaves that set's columns — and, for n_valid, score_out — unwritten. */
int mrgcn_lp_batch_means_f32(const float *loss_slots, int64_t n_loss, const float *train_slots, int64_t n_train,
                             const float *valid_slots, int64_t n_valid, float *row17, float *score_out, void *stream);

/* ---- timing helpers (HIP events on the caller's stream; used by bench.py) ------ */
int mrgcn_event_create(void **event);
int mrgcn_event_destroy(void *event);
int mrgcn_event_record(void *event, void *stream);
int mrgcn_event_elapsed_ms(void *start, void *stop, float *h_ms); /* synchronises on stop */

#ifdef __cplusplus
}
#endif
#endif /* MRGCN_HIP_H */
