/*
 * sn_spmm.h — C-ABI of the MI355X-native Surface-Network sparse-operator layer.
 *
 * This is the drop-in boundary for the ONE hot path of jiangzhongshi/SurfaceNetworks:
 * the sparse-operator x dense-feature product inside the Lap/Dirac ResNet block and the
 * operator-format plumbing around it.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference checkout, file:line).
 *
 * Conventions (all entry points)
 *   - Every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`.
 *   - The library never allocates, frees or synchronises: the caller owns inputs, outputs
 *     and workspaces (reference: launchers allocate with values.new(), sparse_bmm.py:53).
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous and stream-ordered
 *     (reference: launch on torch.cuda.current_stream(), sparse_bmm.py:59, batch_csr.py:56).
 *   - No per-operator or per-shape caches (the reference keeps module-level kernel / handle caches, sparse_bmm_func.py:20-21,
 *     sparse_bmm.py:26,63 — deliberately not kept); re-entrant; safe from several host threads on different streams.
 *     The ONLY process-global state: (a) environment switches, read ONCE per process — the complete list, asserted against the
 *     sources by tests/test_boundary.py::test_environment_switches_are_the_documented_ones:
 *       library  SN_GEMM_VARIANT      0 = the fp32-MFMA kernels (gemm_rows_k, wgrad_mfma_k): the ONE A/B baseline of the Linear
 *                                     kernels (exact fp32 products, no fused epilogues); anything else / unset = the shipped kernels
 *       package  SN_PAIR_FUSED        0 = dense-correspondence loss on the materialised score matrix (baseline of sn_pair_fused_*)
 *                SN_STRICT            1 = raise where a shape falls back to a library GEMM / an unfused composition
 *                SN_DEBUG_VALIDATE    1 = sn_validate_csr_i32 on every operator built from CSR arrays
 *                SN_RESIDENT          0 = utils_pt's batching functions take the reference's host path (no resident cache)
 *                SN_RESIDENT_MAX_GB   HBM budget of that cache (default 96)
 *                SN_DP_FORCE_CPU      1 = dp.init_distributed ignores the GPU (CPU gloo tests)
 *                SN_PLANS             0 = every block launches its kernels one by one from Python (no launch plans, plans.py)
 *                SN_PLAN_GRAPHS       0 = a plan run always walks its launch list (no graph launch at repeating addresses)
 *     SWITCHES: SN_GEMM_VARIANT SN_PAIR_FUSED SN_STRICT SN_DEBUG_VALIDATE SN_RESIDENT SN_RESIDENT_MAX_GB SN_DP_FORCE_CPU SN_PLANS SN_PLAN_GRAPHS
 *     (b) the opt-in per-launch timing facility sn_timing_* below (a mutex-guarded list, off by default).  Neither affects
 *     results.  The Python layer adds process-wide DEFAULTS with the same property: functional.set_dirac_format /
 *     set_laplacian_format (kernel form; one operator can choose for itself, SparseOperator.format) and set_bn_sync (opt-in
 *     global BatchNorm statistics).
 *   - Return value: 0 = success; negative = SN_E_* invalid argument; positive = hipError_t of the
 *     failed launch.  sn_status_string() renders either.
 *   - Indices are int32 (the reference uses int64, utils_pt.py:62, sparse_bmm.cu:17); an operator
 *     whose nnz or row/col count does not fit int32 is rejected with SN_E_RANGE.
 *   - Every output element is written (no reliance on zero-initialised outputs), including rows
 *     with no entries — the reference kernel silently mis-handles interior empty rows
 *     (batch_csr.cu:35-41) and that defect is NOT reproduced.
 *
 * Row addressing of the dense operands ("group" layout)
 *   A dense operand with N columns is addressed as
 *        row r  ->  base + (r / group) * ld + (r % group) * N          (floats)
 *   group = 1 : ordinary row-major matrix with leading dimension ld >= N.
 *   group = 4 : the quaternion view of the Dirac path.  The reference views v:(B,V,C) as
 *               (B*V*4, C/4) (utils_pt.py:201,213): the 4 rows of one vertex/face are C = 4N
 *               contiguous floats.  With ld = 4N this is the same contiguous matrix; with ld = 2C
 *               the operand lives inside one half of the (B,Nodes,2C) concat buffer that feeds
 *               BatchNorm+Linear (utils_pt.py:204,216), so SpMM can read from / write into that
 *               buffer directly and torch.cat disappears.
 */
#ifndef SN_SPMM_H_
#define SN_SPMM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_ABI_VERSION 1

/* negative status codes (positive codes are hipError_t values) */
#define SN_OK            0
#define SN_E_NULL       -1   /* a required pointer is NULL                                   */
#define SN_E_SHAPE      -2   /* negative / inconsistent dimension                            */
#define SN_E_RANGE      -3   /* dimension or nnz does not fit the int32 index type           */
#define SN_E_LD         -4   /* leading dimension / group layout invalid for N               */
#define SN_E_ALIGN      -5   /* reserved: pointer/ld alignment required by a kernel variant  */
#define SN_E_WORKSPACE  -6   /* workspace too small                                          */
#define SN_E_UNSUPPORTED -7  /* e.g. BSR4 requested for M or K not a multiple of 4           */

int         sn_abi_version(void);
const char *sn_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Y = A · X      A: M x K in CSR (int32 rowptr[M+1], colind[nnz], fp32 vals[nnz]), fp32 throughout.
 *
 * Replaces: SparseBMM.__call__(values, col_ind, col_ptr, size, dense)   src/utils/cuda/sparse_bmm.py:28-61
 *           and its kernel                                               src/utils/cuda/sparse_bmm.cu:16-61
 *           and the ATen call sites  torch.mm(L, x) / torch.mm(Di, x) / torch.mm(DiA, x)
 *                                                                         src/utils/utils_pt.py:167,176,202,214
 * The batched (B,R,K) operator of the reference is the block-diagonal 2-D operator with
 * M = B*R, K = B*Kb (col_ptr there already holds global nnz offsets, sparse_bmm.cu:36-37).
 * The same entry point computes the backward  grad_X = Aᵀ · grad_Y  when given the CSR of Aᵀ
 * (sparse_bmm_func.py:66-70); no gradient w.r.t. the operator exists (sparse_bmm_func.py:72).
 *
 * X: K rows, Y: M rows, both N columns, addressed with (ld, group) as described above.
 * Any N >= 1 is accepted; N in {16,32,64,128} with 16-byte aligned bases/ld take the
 * vectorised wave64 kernels.  X and Y must not alias.
 * ------------------------------------------------------------------------------------------ */
int sn_spmm_csr_f32(const int32_t *rowptr, const int32_t *colind, const float *vals,
                    int64_t M, int64_t K, int64_t nnz,
                    const float *X, int64_t ldx, int32_t x_group,
                    int32_t N,
                    float *Y, int64_t ldy, int32_t y_group,
                    void *stream);

/* sn_spmm_csr_stats_f32: sn_spmm_csr_f32 for N = 128, y_group = 1 (the Laplacian product on 128-channel rows,
 * torch.mm(L, x) at src/utils/utils_pt.py:167,176) that ALSO leaves the BatchNorm statistics of its output:
 * stats_part[sn_spmm_q3_stats_blocks()][2][128] fp64 partial column sums / sums of squares, to be combined by
 * sn_colstats_merge_f64 — the statistics pass over the propagated half of [x | L x] (utils_pt.py:168-169,177-178:
 * torch.cat + BatchNorm1d) disappears.  workspace: sn_spmm_csr_stats_workspace_bytes(M). Y is bit-identical to sn_spmm_csr_f32. */
size_t sn_spmm_csr_stats_workspace_bytes(int64_t M);
int sn_spmm_csr_stats_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K, int64_t nnz,
                          const float *X, int64_t ldx, int32_t x_group, int32_t N, float *Y, int64_t ldy, int32_t y_group,
                          double *stats_part, void *workspace, size_t workspace_bytes, void *stream);

/* Same product with A stored as 4x4-block BSR (block rows Mb = M/4, block cols Kb = K/4,
 * bvals holds 16 floats per block, row-major inside the block).  This is the packed form of the
 * quaternionic Dirac operators: every 4x4 block of Di is -Q(0,e)/(2 Af) (src/utils/mesh.py:28-33,55-58).
 * Results are bit-identical to sn_spmm_csr_f32 on the same operator for finite X (the explicit
 * zeros of a block contribute fma(0,x,acc) == acc). N must be a multiple of 4. */
int sn_spmm_bsr4_f32(const int32_t *b_rowptr, const int32_t *b_colind, const float *b_vals,
                     int64_t Mb, int64_t Kb, int64_t nblocks,
                     const float *X, int64_t ldx, int32_t x_group,
                     int32_t N,
                     float *Y, int64_t ldy, int32_t y_group,
                     void *stream);

/* Quaternion-packed Dirac operators ("Q3").  Every 4x4 block of Di, DiA and their transposes is the matrix of a
 * multiplication by a pure quaternion (src/utils/mesh.py:28-33: Q(0,e); :55-58: -Q/(2 Af) and its transpose times Af/Av),
 *     M(p) = [[0, p1, p2, p3], [-p1, 0, p3, -p2], [-p2, -p3, 0, p1], [-p3, p2, -p1, 0]],
 * i.e. three floats.  q_blk holds one 16-byte record (p1, p2, p3, block column as int32 bits) per block, b_rowptr is the
 * BSR4 block-row pointer.  The operator stream is 16 instead of 68 bytes per block; results are bit-identical to
 * sn_spmm_bsr4_f32 / sn_spmm_csr_f32 for finite X (same k-ascending FMA order; zeros contribute fma(0,x,acc) = acc).
 * sn_bsr4_to_q3_f32 packs a BSR4 operator and sets *not_quaternion (device int32) to 1 if any block is not exactly M(p):
 * the caller then keeps the BSR4 form.  sn_blockdiag_concat_i32 assembles pooled Q3 operators with vals_per_entry = 4
 * (the column offset is applied inside the record; colind arguments are unused). */
int sn_spmm_q3_f32(const int32_t *b_rowptr, const float *q_blk, int64_t Mb, int64_t Kb, int64_t nblocks,
                   const float *X, int64_t ldx, int32_t x_group, int32_t N,
                   float *Y, int64_t ldy, int32_t y_group, void *stream);
/* sn_spmm_q3_stats_f32: sn_spmm_q3_f32 for N = 32 or 16, y_group = 4 (the (rows/4, 4N) view of a 128- / 64-channel tensor) that ALSO
 * leaves the BatchNorm statistics of its output: stats_part[sn_spmm_q3_stats_blocks()][2][4N] fp64 partial column sums /
 * sums of squares (per channel c = N*component + column), to be combined by sn_colstats_merge_f64 — the statistics pass over
 * the propagated half of a stage's concat buffer (utils_pt.py:204-205,216-217: torch.cat + BatchNorm1d) disappears.
 * Each workgroup's fp32 partial of its 32 output rows goes through `workspace` (sn_spmm_q3_stats_workspace_bytes(Mb)) and is
 * added up in fp64 in a fixed order (deterministic).  Y is bit-identical to sn_spmm_q3_f32. */
size_t sn_spmm_q3_stats_workspace_bytes(int64_t Mb);
int32_t sn_spmm_q3_stats_blocks(void);
int sn_spmm_q3_stats_f32(const int32_t *b_rowptr, const float *q_blk, int64_t Mb, int64_t Kb, int64_t nblocks, const float *X,
                         int64_t ldx, int32_t x_group, int32_t N, float *Y, int64_t ldy, int32_t y_group, double *stats_part,
                         void *workspace, size_t workspace_bytes, void *stream);
int sn_spmm_q3_elubwd_f32(const int32_t *b_rowptr, const float *q_blk, int64_t Mb, int64_t Kb, int64_t nblocks,
                          const float *X, int64_t ldx, int32_t x_group, int32_t N,
                          const float *E, int64_t lde, const float *G, int64_t ldg,
                          float *Y, int64_t ldy, int32_t y_group, void *stream);
/* The same product, which also leaves an upper bound of max |Y| for the two-piece weight gradient that reads Y as its dy
 * operand (sn_wgrad_*_bounded_f32): y_absmax — device, sn_spmm_q3_absmax_blocks(Mb, N) floats, one maximum per workgroup;
 * the consumer takes the maximum of all of them.  No atomics, nothing to zero beforehand; deterministic. */
int64_t sn_spmm_q3_absmax_blocks(int64_t Mb, int32_t N);
int sn_spmm_q3_elubwd_absmax_f32(const int32_t *b_rowptr, const float *q_blk, int64_t Mb, int64_t Kb, int64_t nblocks,
                                 const float *X, int64_t ldx, int32_t x_group, int32_t N, const float *E, int64_t lde,
                                 const float *G, int64_t ldg, float *Y, int64_t ldy, int32_t y_group, float *y_absmax,
                                 void *stream);
/* The same product for a RAW G: the bare product p that sn_linear_dgrad_elu_rawlow_f32 left in place of the finished input
 * gradient of the stage whose activated operand is E.  The store finishes it with E in registers, in the operation order of
 * that GEMM's own epilogue (bit-identical to the two-kernel result):
 *     g = v + v·min(E, 0),  v = p + ((E - center[c])·B[c] + Cc[c]),      Y = (A·X) ∘ elu'(E) + g
 * center / B / Cc: device, 4·N floats each, indexed by channel c = N·component + column (16-byte aligned).
 * sn_spmm_q3_tail_supported(N, y_group): N = 32 | 16 and group-4 rows; anything else is SN_E_UNSUPPORTED — finish G first with
 * sn_elu_tail_finish_f32 (G <- g in place on a (rows x C) matrix, channel = column: C % 4 = 0, 16-byte aligned) and run the
 * plain fused product.  y_absmax may be NULL. */
int32_t sn_spmm_q3_tail_supported(int32_t N, int32_t y_group);
int sn_spmm_q3_elubwd_tail_absmax_f32(const int32_t *b_rowptr, const float *q_blk, int64_t Mb, int64_t Kb, int64_t nblocks,
                                      const float *X, int64_t ldx, int32_t x_group, int32_t N, const float *E, int64_t lde,
                                      const float *G, int64_t ldg, const float *center, const float *B, const float *Cc,
                                      float *Y, int64_t ldy, int32_t y_group, float *y_absmax, void *stream);
int sn_elu_tail_finish_f32(float *g, int64_t ldg, const float *E, int64_t lde, const float *center, const float *B,
                           const float *Cc, int64_t rows, int32_t C, void *stream);
int sn_bsr4_to_q3_f32(const int32_t *b_colind, const float *b_vals, int64_t nblocks, float *q_blk,
                      int32_t *not_quaternion, void *stream);

/* The same two products with the backward of the ELU that precedes the propagation fused into the store:
 *     Y = (A·X) ∘ elu'(E) + G,      elu'(·) taken from the activation OUTPUT E: 1 where E > 0, E + 1 elsewhere
 * — with A = Lᵀ / Diᵀ / DiAᵀ this is the gradient that autograd assembles from the sparse product's backward
 * (src/utils/cuda/sparse_bmm_func.py:60-71), ELUBackward (F.elu at src/utils/utils_pt.py:161,171,193,208) and the sum of
 * the other branches' gradients (G), without the two intermediate arrays.  E and G have Y's shape and row grouping
 * (y_group) with their own leading dimensions; G may be NULL.  N in {16,32,64,128}, 16-byte aligned operands. */
int sn_spmm_csr_elubwd_f32(const int32_t *rowptr, const int32_t *colind, const float *vals,
                           int64_t M, int64_t K, int64_t nnz,
                           const float *X, int64_t ldx, int32_t x_group,
                           int32_t N,
                           const float *E, int64_t lde, const float *G, int64_t ldg,
                           float *Y, int64_t ldy, int32_t y_group,
                           void *stream);
int sn_spmm_bsr4_elubwd_f32(const int32_t *b_rowptr, const int32_t *b_colind, const float *b_vals,
                            int64_t Mb, int64_t Kb, int64_t nblocks,
                            const float *X, int64_t ldx, int32_t x_group,
                            int32_t N,
                            const float *E, int64_t lde, const float *G, int64_t ldg,
                            float *Y, int64_t ldy, int32_t y_group,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Sorted COO -> CSR.
 *
 * Replaces: BatchCSR.__call__(indices, size) -> (col_ind, col_ptr)      src/utils/cuda/batch_csr.py:28-59
 *           and its kernel                                               src/utils/cuda/batch_csr.cu:13-47
 *           plus the implicit COO->CSR inside ATen's sparse addmm behind utils_pt.py:167,176,202,214.
 *
 * idx_batch may be NULL (2-D operator, B = 1).  For a 3-D batched operator (B, R, Kb) — the output
 * of sparse_cat (utils_pt.py:21-39) — the result is the block-diagonal CSR with
 *      global row = b*R + r  (M = B*R rows),   global col = b*Kb + c.
 * Indices are the int64 rows of a torch COO `_indices()` tensor; entries must be sorted by
 * (batch,row[,col]) — i.e. coalesced, as the reference requires (batch_csr.cu comment, :13).
 * rowptr (M+1 entries) is computed by binary search per row, so interior empty rows are correct.
 * ------------------------------------------------------------------------------------------ */
int sn_coo_to_csr_i32(const int64_t *idx_batch, const int64_t *idx_row, const int64_t *idx_col,
                      int64_t nnz, int64_t B, int64_t R, int64_t Kb,
                      int32_t *rowptr, int32_t *colind,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * CSR of Aᵀ from CSR of A (deterministic: entries of each output row ordered by column).
 *
 * Replaces: matrix1.transpose(2,1).coalesce() + batch_csr on every backward
 *                                                                         src/utils/cuda/sparse_bmm_func.py:66-67
 * Done ONCE per operator here and kept resident next to A.
 * workspace: sn_csr_transpose_workspace_bytes(M, K, nnz) bytes of device scratch.
 * ------------------------------------------------------------------------------------------ */
size_t sn_csr_transpose_workspace_bytes(int64_t M, int64_t K, int64_t nnz);
int sn_csr_transpose_f32(const int32_t *rowptr, const int32_t *colind, const float *vals,
                         int64_t M, int64_t K, int64_t nnz,
                         int32_t *t_rowptr, int32_t *t_colind, float *t_vals,
                         void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * CSR -> BSR4 (4x4 blocks).  Two phases because the caller owns the allocation:
 *   1. sn_bsr4_count: b_rowptr[Mb+1] <- exclusive scan of the number of distinct 4-wide block
 *      columns touched by each group of 4 rows; the caller reads b_rowptr[Mb] (= nblocks).
 *   2. sn_bsr4_fill : b_colind[nblocks], b_vals[16*nblocks] (zero-filled where A has no entry).
 * Column indices inside each CSR row must be sorted ascending (coalesced operator).
 * workspace for count: sn_scan_workspace_bytes(Mb + 1).
 * ------------------------------------------------------------------------------------------ */
size_t sn_scan_workspace_bytes(int64_t n);
int sn_bsr4_count(const int32_t *rowptr, const int32_t *colind, int64_t M, int64_t K,
                  int32_t *b_rowptr, void *workspace, size_t workspace_bytes, void *stream);
int sn_bsr4_fill(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K,
                 const int32_t *b_rowptr, int32_t *b_colind, float *b_vals, void *stream);

/* ------------------------------------------------------------------------------------------
 * CSR -> RB4 ("row-blocked", 4x1 blocks) and the RB4 product — the packed form of the Laplacian-type operators
 * (torch.mm(L, x) with ~7 entries per row, src/utils/utils_pt.py:167,176; L from src/utils/mesh.py:102-112 and
 * src/utils/graph.py:40-66).  Rows 4b .. 4b+3 share one sorted list of the columns any of them touches; every listed
 * column carries four coefficients (zero where a row lacks it).  Four consecutive mesh rows reach ~16 distinct columns with
 * ~28 entries, so the product gathers each X row once per 4-row group instead of once per row.
 *   sn_rb4_count: b_ptr[Mb+1] <- exclusive scan of the listed-column counts, Mb = ceil(M/4) (rows past M are empty);
 *                 workspace sn_scan_workspace_bytes(Mb + 1).  The total b_ptr[Mb] never exceeds nnz, so the caller can
 *                 size b_col / b_val by nnz without reading it back.
 *   sn_rb4_fill : b_col[total] (ascending inside a group), b_val[4*total] (16-byte aligned).
 *   sn_spmm_rb4_f32 / _elubwd_f32 / _stats_f32: Y = A X on plain row-major operands (group = 1), N in {64, 128}; same
 *                 epilogue / statistics semantics as the CSR entry points; `capacity` = allocated length of b_col.
 * Results are bit-identical to sn_spmm_csr_f32 for finite X (same k-ascending FMA order per row; a zero coefficient
 * contributes fma(0, x, acc) = acc; a non-finite X entry reaches all 4 rows of a group that lists its column).
 * ------------------------------------------------------------------------------------------ */
int sn_rb4_count(const int32_t *rowptr, const int32_t *colind, int64_t M, int64_t K, int32_t *b_ptr,
                 void *workspace, size_t workspace_bytes, void *stream);
int sn_rb4_fill(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K,
                const int32_t *b_ptr, int32_t *b_col, float *b_val, void *stream);
int sn_spmm_rb4_f32(const int32_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t M, int64_t K, int64_t capacity,
                    const float *X, int64_t ldx, int32_t N, float *Y, int64_t ldy, void *stream);
int sn_spmm_rb4_elubwd_f32(const int32_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t M, int64_t K,
                           int64_t capacity, const float *X, int64_t ldx, int32_t N, const float *E, int64_t lde,
                           const float *G, int64_t ldg, float *Y, int64_t ldy, void *stream);
/* ... and max |Y| per wave into y_absmax[sn_spmm_rb4_absmax_blocks(M, N)] floats (every entry written): the bound the two-piece
 * weight gradient of the layer below needs for its dy operand (sn_wgrad_bounded_f32) — the fused backward of a Laplacian stage
 * (SparseBMMFunc.backward + ELUBackward, sparse_bmm_func.py:60-71) writes exactly that operand. */
int64_t sn_spmm_rb4_absmax_blocks(int64_t M, int32_t N);
int sn_spmm_rb4_elubwd_absmax_f32(const int32_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t M, int64_t K,
                                  int64_t capacity, const float *X, int64_t ldx, int32_t N, const float *E, int64_t lde,
                                  const float *G, int64_t ldg, float *Y, int64_t ldy, float *y_absmax, void *stream);
size_t sn_spmm_rb4_stats_workspace_bytes(int64_t M);
int sn_spmm_rb4_stats_f32(const int32_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t M, int64_t K,
                          int64_t capacity, const float *X, int64_t ldx, int32_t N, float *Y, int64_t ldy,
                          double *stats_part, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sliding-window ("ring") product for BANDED SQUARE CSR operators — the Laplacian products torch.mm(L, x) at 64 / 128
 * channels (src/utils/utils_pt.py:167,176) on batches that fill the chip; same arguments, epilogue and statistics semantics
 * as sn_spmm_csr_f32 / _elubwd_f32 / _stats_f32 with group = 1, straight from the CSR arrays (no derived form).
 * A persistent workgroup walks a strip of rows and keeps the X rows within +-sn_spmm_csr_ring_half_window() of the current
 * rows in an LDS ring: every X line and every entry is requested once per 64-column slice, by LDS-DMA.  Columns outside
 * the window are gathered from global memory (correct for ANY operator, fast for banded ones): callers decide with
 * sn_csr_band_i32, which leaves max |column - row|, the longest row and the number of rows with an entry outside the window
 * in band_longest_outside[0..2] (device memory); an operator with a row whose columns do not ascend strictly reports
 * INT32_MAX as its longest row (the ring kernel bounds a row by its first and last entry: such an operator must not take it).
 * Requirements: M == K, N in {64, 128}, columns ascending inside each row; SN_E_UNSUPPORTED otherwise.
 * Results are bit-identical to sn_spmm_csr_f32 (same k-ascending FMA order per row).
 * ------------------------------------------------------------------------------------------ */
int sn_spmm_csr_ring_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K, int64_t nnz,
                         const float *X, int64_t ldx, int32_t N, float *Y, int64_t ldy, void *stream);
int sn_spmm_csr_ring_elubwd_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K,
                                int64_t nnz, const float *X, int64_t ldx, int32_t N, const float *E, int64_t lde, const float *G,
                                int64_t ldg, float *Y, int64_t ldy, void *stream);
/* ... and max |Y| per compute wave into y_absmax[sn_spmm_csr_ring_absmax_blocks(M, N)] floats (every entry written; as
 * sn_spmm_rb4_elubwd_absmax_f32).  An operator without entries is not taken (SN_E_UNSUPPORTED). */
int64_t sn_spmm_csr_ring_absmax_blocks(int64_t M, int32_t N);
int sn_spmm_csr_ring_elubwd_absmax_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K,
                                       int64_t nnz, const float *X, int64_t ldx, int32_t N, const float *E, int64_t lde,
                                       const float *G, int64_t ldg, float *Y, int64_t ldy, float *y_absmax, void *stream);
size_t sn_spmm_csr_ring_stats_workspace_bytes(int64_t M);
int sn_spmm_csr_ring_stats_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K, int64_t nnz,
                               const float *X, int64_t ldx, int32_t N, float *Y, int64_t ldy, double *stats_part, void *workspace,
                               size_t workspace_bytes, void *stream);
int32_t sn_spmm_csr_ring_half_window(void);
int sn_csr_band_i32(const int32_t *rowptr, const int32_t *colind, int64_t M, int64_t K, int32_t *band_longest_outside, void *stream);

/* ------------------------------------------------------------------------------------------
 * Block-diagonal batch assembly from a device-resident pool of per-mesh operators.
 *
 * Replaces: sparse_diag_cat(tensors, size0, size1)                       src/utils/utils_pt.py:41-53
 *           (index shift i*[size0;size1], concat, coalesce() sort on the host every step) and the
 *           per-sample sp_sparse_to_pt_sparse conversions               src/utils/utils_pt.py:56-69,
 *           src/as_rigid_as_possible/main.py:161-162,174-175.
 *
 * The pool holds every mesh's operator once (CSR with vals_per_entry = 1, or BSR4 with 16), rowptr
 * local to the mesh (starting at 0).  desc is a (B x 4) int64 table, one row per selected mesh:
 *      desc[b] = { offset of the mesh's rowptr in pool_rowptr,
 *                  offset of the mesh's first entry in pool_colind (vals: x vals_per_entry),
 *                  number of rows of the mesh (<= size0),
 *                  offset of the mesh's first entry in the OUTPUT (exclusive prefix of entry counts) }
 * Output: out_rowptr[B*size0 + 1], out_colind[total], out_vals[total*vals_per_entry] with
 * row = b*size0 + r and col = b*size1 + c; rows beyond a mesh's own count are empty (the padding to
 * the batch maximum of the reference).  `total` = number of entries of the whole batch.
 * ------------------------------------------------------------------------------------------ */
int sn_blockdiag_concat_i32(const int32_t *pool_rowptr, const int32_t *pool_colind, const float *pool_vals,
                            const int64_t *desc, int64_t B, int64_t size0, int64_t size1,
                            int64_t total, int32_t vals_per_entry,
                            int32_t *out_rowptr, int32_t *out_colind, float *out_vals,
                            void *stream);

/* Ragged (packed) form of the same assembly — what the reference cannot express: sparse_diag_cat pads every block to
 * (size0, size1) = the batch maximum (src/utils/utils_pt.py:48-52; src/as_rigid_as_possible/main.py:172-185 computes the
 * maxima), so half of a 1k..20k-vertex batch is padding.  Here mesh b owns the output rows [desc[b][4], desc[b+1][4])
 * (the last mesh up to total_rows), the first desc[b][2] of which carry its entries, and its column indices are shifted by
 * desc[b][5].  With both offsets = exclusive prefix sums of the meshes' own row / column counts the batch has no padding
 * at all: the dense operands are the concatenation of the meshes' rows.  (desc[b][4] = b*size0, desc[b][5] = b*size1
 * reproduces sn_blockdiag_concat_i32.)
 *      desc[b] = { rowptr offset in the pool, entry offset in the pool, rows with entries,
 *                  entry offset in the output, first output row, column shift }          (B x 6) int64
 * desc[b][4] must be ascending with desc[0][4] = 0.  Output: out_rowptr[total_rows + 1], out_colind[total],
 * out_vals[total * vals_per_entry]; total_cols only enters the int32 range check. */
int sn_blockdiag_concat_ragged_i32(const int32_t *pool_rowptr, const int32_t *pool_colind, const float *pool_vals,
                                   const int64_t *desc, int64_t B, int64_t total_rows, int64_t total_cols,
                                   int64_t total, int32_t vals_per_entry,
                                   int32_t *out_rowptr, int32_t *out_colind, float *out_vals,
                                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Debug validation of a CSR operator on the device.  The reference kernels index without any bounds check
 * (src/utils/cuda/sparse_bmm.cu:16-61, batch_csr.cu:13-47) and so do the product kernels here (an out-of-range column is
 * an out-of-bounds gather); this entry point is the opt-in check.  *flags (device int32) receives a bit set:
 *   1 rowptr[0] != 0 | 2 rowptr not non-decreasing | 4 rowptr[M] != nnz | 8 column index outside [0, K) |
 *   16 column indices of a row not strictly ascending (operator not coalesced) | 32 non-finite value (vals may be NULL).
 * 0 = the operator is well formed.  The Python layer runs it on every operator it builds when SN_DEBUG_VALIDATE=1 and
 * raises (status SN_E_RANGE semantics) — see surfacenetworks_amd/operators.py.
 * ------------------------------------------------------------------------------------------ */
int sn_validate_csr_i32(const int32_t *rowptr, const int32_t *colind, const float *vals, int64_t M, int64_t K, int64_t nnz,
                        int32_t *flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused elementwise helpers of the residual blocks (each replaces separate ATen passes).
 *
 * sn_elu_into_f32: dst[r, 0:C] = elu(src[r, 0:C]) for `rows` rows; src stride lds, dst stride ldd.
 *   Replaces F.elu (utils_pt.py:161,171,195,208) + the first operand copy of torch.cat
 *   (utils_pt.py:168,177,204,216): ELU is written straight into the first half of the concat buffer.
 * sn_elu_bwd_acc_f32: gsrc[r,c] (+)= (gdst[r,c] + gdst2[r,c]) * (out[r,c] > 0 ? 1 : out[r,c] + 1) + gadd[r,c], out = elu
 *   value.  gdst2 and gadd may be NULL.  The activated tensor feeds both the concat buffer and the SpMM (two gradients
 *   meet before the ELU derivative) and the un-activated tensor also feeds the residual path (gadd, after it);
 *   accumulate != 0 additionally adds into gsrc.
 * ------------------------------------------------------------------------------------------ */
int sn_elu_into_f32(const float *src, int64_t lds, float *dst, int64_t ldd,
                    int64_t rows, int32_t C, void *stream);
int sn_elu_bwd_acc_f32(const float *gdst, int64_t ldg, const float *gdst2, int64_t ldg2, const float *gadd, int64_t ldga,
                       const float *out, int64_t ldo, float *gsrc, int64_t ldgs, int64_t rows, int32_t C,
                       int32_t accumulate, void *stream);


/* ------------------------------------------------------------------------------------------
 * BatchNorm("pre") + Linear of GraphConv1x1 (src/utils/utils_pt.py:83-99) without materialising the
 * normalised tensor.  With s = gamma*invstd, t = beta - mean*s the layer is  y = x·(W·diag(s))ᵀ + (b + W·t),
 * so the forward needs only per-channel statistics of x; the backward needs G = dyᵀ·x and colsum(dy), from
 * which every BatchNorm reduction follows algebraically (sum dz = colsum(dy)·W, sum dz*x = sum_j W∘G).
 *
 * sn_colstats_f32 : out[0:C] = column sums, out[C:2C] = column sums of squares of x (rows x C, row stride ld),
 *                   accumulated in fp64, two deterministic stages.  Replaces the statistics pass of
 *                   nn.BatchNorm1d (train mode) and the bias-gradient reduction.
 * sn_wgrad_f32    : G (J x C, row-major, fp32) = dyᵀ·(x - center) with dy (rows x J, stride lddy), x (rows x C, stride
 *                   ldx), center[C] optional (NULL = 0; BatchNorm passes the batch mean so that no cancellation
 *                   between dyᵀ·x and mean·colsum(dy) is left to fp32):
 *                   split-K over row slabs on the fp32 MFMA (v_mfma_f32_32x32x2_f32), partial tiles reduced in a
 *                   fixed order.  J <= 128 and a multiple of 4, C in {128, 256}.  dysum (optional, J doubles) receives the
 *                   column sums of dy — the bias gradient and the input of sn_bn_bwd_coeffs_f32 — accumulated by the
 *                   same pass over dy, so no separate reduction kernel is needed.
 *                   Replaces the weight-gradient GEMM of nn.Linear for tall-skinny operands (K = rows ~ 1e5..1e6).
 * sn_affine_cols_acc_f32 : dx[r,c] += (x[r,c] - center[c])*B[c] + Cc[c]  (the elementwise tail of BatchNorm
 *                   backward, fused; center may be NULL).
 * ------------------------------------------------------------------------------------------ */
size_t sn_colstats_workspace_bytes(int64_t rows, int32_t C);
int sn_colstats_f32(const float *x, int64_t ld, int64_t rows, int32_t C, double *out,
                    void *workspace, size_t workspace_bytes, void *stream);
/* sn_colstats_into_f32 : the same statistics written as ONE HALF of a wider vector: sums at out[out_off + c], sums of
 *                   squares at out[out_ld + out_off + c] (out_ld = full width).
 * sn_colstats_merge_f64 : the other half, from the per-workgroup partials ([nblk][2][C] fp64, nblk =
 *                   sn_linear_fwd_stats_blocks(rows)) that sn_linear_fwd_f32 / sn_linear_fwd_segbias_f32 leave when asked for
 *                   the column statistics of their ELU output (elu_stats_part): the statistics pass of the next stage then
 *                   reads only the propagated half of its concat buffer. */
int sn_colstats_into_f32(const float *x, int64_t ld, int64_t rows, int32_t C, double *out, int64_t out_ld, int64_t out_off,
                         void *workspace, size_t workspace_bytes, void *stream);
int sn_colstats_merge_f64(const double *part, int32_t nblk, int32_t C, double *out, int64_t out_ld, int64_t out_off,
                          void *stream);
/* sn_colstats_merge2_f64 : both halves at once — out (2 x (C_lo + C_hi) fp64, [sums | squares]) from the partials of the two
 * producers ([nblk_lo][2][ld_lo] and [nblk_hi][2][ld_hi], of which the first C_lo / C_hi channels count: ld = C for a
 * producer's own layout, 128 for the forward GEMM of a 64-output layer); the same sums, bit for bit, as two
 * sn_colstats_merge_f64 calls on packed partials. */
int sn_colstats_merge2_f64(const double *part_lo, int32_t nblk_lo, int32_t C_lo, int32_t ld_lo, const double *part_hi,
                           int32_t nblk_hi, int32_t C_hi, int32_t ld_hi, double *out, void *stream);
int32_t sn_linear_fwd_stats_blocks(int64_t rows);
size_t sn_wgrad_workspace_bytes(int64_t rows, int32_t J, int32_t C);
int sn_wgrad_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                 int32_t J, int32_t C, float *G, double *dysum, void *workspace, size_t workspace_bytes, void *stream);
/* sn_wgrad_seg_f32: the same weight gradient for a batch of rows / rows_per_seg meshes, with the row slabs aligned to mesh
 * boundaries so that the pass also yields the PER-MESH column sums of dy, seg_dysum (nseg x J, fp32) — what the half-width
 * global-average stage needs (it replaces a sn_segment_colsum_f32 pass over dy).  dysum and seg_dysum are required; rows
 * must be a multiple of rows_per_seg.  Split-bf16 kernels only (SN_E_UNSUPPORTED with SN_GEMM_VARIANT=0). */
size_t sn_wgrad_seg_workspace_bytes(int64_t rows, int64_t rows_per_seg, int32_t J, int32_t C);
int sn_wgrad_seg_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                     int64_t rows_per_seg, int32_t J, int32_t C, float *G, double *dysum, float *seg_dysum, void *workspace,
                     size_t workspace_bytes, void *stream);
/* sn_wgrad_slabs_f32: the same for RAGGED meshes (packed batches, no padding rows — the reference pads every mesh to the
 * batch maximum, src/as_rigid_as_possible/main.py:172-185): the caller supplies the row slabs, slab b = rows
 * [slab_off[b], slab_off[b+1]) (device int64[nslab + 1], consecutive, none crossing a mesh boundary) and the slabs of every
 * mesh, [seg_slab_ptr[m], seg_slab_ptr[m+1]) (device int64[nseg + 1]); seg_dysum is (nseg x J).  Workspace:
 * nslab * 128 * (C + 1) floats.  16-bit matrix-pipe kernel only (SN_E_UNSUPPORTED with SN_GEMM_VARIANT=0). */
int sn_wgrad_slabs_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                       const int64_t *slab_off, int32_t nslab, const int64_t *seg_slab_ptr, int32_t nseg, int32_t J, int32_t C,
                       float *G, double *dysum, float *seg_dysum, void *workspace, size_t workspace_bytes, void *stream);
/* sn_wgrad_*_bounded_f32: the three weight gradients above on TWO fp16 pieces per operand (three exact partial products
 * instead of the six of the three-piece bf16 split: half the matrix work; measured -20 % per launch, round 4).  fp16 has
 * five exponent bits, and the contraction runs over the rows, so the powers of two that bring the operands into range must be
 * constant along a column and known before the first row is read.  The caller supplies the bounds they follow from:
 *   dybound   device, n_dybound floats whose maximum is >= max |dy| over the whole operand — the per-workgroup maxima left by
 *             the kernel that produced dy (sn_linear_dgrad_elu_absmax_f32, sn_linear_dgrad_eluseg_absmax_f32,
 *             sn_spmm_q3_elubwd_absmax_f32), or one number from any other source; the kernel takes their maximum itself;
 *   xinvstd   device, C floats: BatchNorm's inverse standard deviations 1 / sqrt(var + eps) of x's columns about `center`
 *             (the biased batch variance, src/utils/utils_pt.py:83-99 nn.BatchNorm1d), over stat_rows >= rows rows that include
 *             every row of x:  |x[r][c] - center[c]| <= sqrt(stat_rows) / xinvstd[c]  holds for every row, rigorously.
 * Both operands are scaled so that their bound lands in [2^14, 2^15) (nothing can overflow); an element keeps 22 significant
 * bits down to 2^-17 of its operand's bound and 2^-25 of the scaled unit (2^-39 of the bound) in absolute terms below that
 * (one accumulator, the low pieces unscaled); results leave multiplied by the exact inverse scales.  Eval-mode BatchNorm (running statistics) offers no such bound: use the unbounded forms.
 * Same arguments, workspace and status codes as the forms above; SN_E_SHAPE when stat_rows < rows, SN_E_NULL without bounds. */
int sn_wgrad_bounded_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                         int32_t J, int32_t C, float *G, double *dysum, void *workspace, size_t workspace_bytes,
                         const float *dybound, int64_t n_dybound, const float *xinvstd, int64_t stat_rows, void *stream);
int sn_wgrad_seg_bounded_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                             int64_t rows_per_seg, int32_t J, int32_t C, float *G, double *dysum, float *seg_dysum,
                             void *workspace, size_t workspace_bytes, const float *dybound, int64_t n_dybound,
                             const float *xinvstd, int64_t stat_rows, void *stream);
int sn_wgrad_slabs_bounded_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, const float *center, int64_t rows,
                               const int64_t *slab_off, int32_t nslab, const int64_t *seg_slab_ptr, int32_t nseg, int32_t J,
                               int32_t C, float *G, double *dysum, float *seg_dysum, void *workspace, size_t workspace_bytes,
                               const float *dybound, int64_t n_dybound, const float *xinvstd, int64_t stat_rows, void *stream);
/* sn_wgrad_thin_f32: weight and bias gradient of a Linear with 1..8 input channels — the models' first layer,
 * GraphConv1x1(6 | 3 -> C, batch_norm=None) (src/as_rigid_as_possible/models.py:113, src/utils/utils_pt.py:99) — on
 * rows ~ 1e5..1e6:  G (J x C, row-major, fp32) = dy^T x,  db (J, optional) = colsum(dy).  One pass over dy; fp32
 * accumulation over <= 64 rows per thread, fp64 above; two deterministic stages.  J % 4 == 0 and J/4 must divide 256
 * (SN_E_UNSUPPORTED otherwise).  Replaces the weight-gradient GEMM + the bias reduction of nn.Linear's backward. */
size_t sn_wgrad_thin_workspace_bytes(int64_t rows, int32_t J, int32_t C);
int sn_wgrad_thin_f32(const float *dy, int64_t lddy, const float *x, int64_t ldx, int64_t rows, int32_t J, int32_t C,
                      float *G, float *db, void *workspace, size_t workspace_bytes, void *stream);
/* Masked smooth-L1 training loss of the ARAP harness (src/as_rigid_as_possible/main.py:225-226:
 * `outputs * mask`, F.smooth_l1_loss(size_average=False) / batch_size), forward and backward as one pass each:
 *   loss  = scale * sum_{r,c} l(out[r,c]*rowmask[r] - target[r,c]),  l(d) = d*d/2 if |d| < 1 else |d| - 1/2   (fp64 sums)
 *   gout  = gloss[0]*scale * rowmask[r] * clamp(out[r,c]*rowmask[r] - target[r,c], -1, 1)
 * rowmask (rows floats) may be NULL (= all ones); gloss is a DEVICE scalar (the gradient of the loss value). */
size_t sn_masked_smooth_l1_workspace_bytes(int64_t rows, int32_t C);
int sn_masked_smooth_l1_fwd_f32(const float *out, int64_t ldo, const float *target, int64_t ldt, const float *rowmask,
                                int64_t rows, int32_t C, double scale, float *loss, void *workspace, size_t workspace_bytes,
                                void *stream);
int sn_masked_smooth_l1_bwd_f32(const float *out, int64_t ldo, const float *target, int64_t ldt, const float *rowmask,
                                int64_t rows, int32_t C, double scale, const float *gloss, float *gout, int64_t ldg,
                                void *stream);
/* Loss and gradient in one pass over out and target (a training step reads them once instead of twice):
 *   sn_masked_smooth_l1_fwdg_f32 : the loss of sn_masked_smooth_l1_fwd_f32 — the same grid, items and order of the sum, so the
 *                   same bits — and gout as sn_masked_smooth_l1_bwd_f32 writes it for gloss[0] == 1 (the same expression, so the
 *                   same bits).  Where out and target allow 16-byte items, gout must too (SN_E_ALIGN otherwise).
 *   sn_masked_smooth_l1_bwdg_f32 : sn_masked_smooth_l1_bwd_f32 over a gout that sn_masked_smooth_l1_fwdg_f32 filled for the same
 *                   operands: gout is kept when gloss[0] == 1 — tested on the device, gloss may be written by a captured graph —
 *                   and recomputed from out and target otherwise.  Same result as sn_masked_smooth_l1_bwd_f32 for every gloss. */
int sn_masked_smooth_l1_fwdg_f32(const float *out, int64_t ldo, const float *target, int64_t ldt, const float *rowmask,
                                 int64_t rows, int32_t C, double scale, float *loss, float *gout, int64_t ldg, void *workspace,
                                 size_t workspace_bytes, void *stream);
int sn_masked_smooth_l1_bwdg_f32(const float *out, int64_t ldo, const float *target, int64_t ldt, const float *rowmask,
                                 int64_t rows, int32_t C, double scale, const float *gloss, float *gout, int64_t ldg,
                                 void *stream);
/* ---- Normal prediction ----------------------------------------------------------------------------------------------------
 * Squared-cosine loss, mean angle deviation and the loss gradient of the normal-prediction driver in one pass over the rows.
 * Replaces: src/normal_predict/train_4_normal.py:113-123 (loss_fun, mean_angle_deviation: F.normalize, the inner product,
 * masked_select and mean, each twice, and their backward passes).  Per row r, all fp32:
 *   o = y[r, 0:3] (+ frame[r, 0:3] if a frame is given)
 *   n = max(sqrt(o·o), 1e-12)        u = o / n          c = u·t[r]
 *   l = 1 - c·c                      a = acos(min(|c|, 1))
 *   S = { r : rowmask[r] != 0 }   (rowmask NULL: all rows)
 *   loss = sum_S l / |S|           mad = sum_S a / |S|       (fp64 sums, a fixed order: the same bits every run)
 *   g[r] = (gloss/|S|) · (-2c) · (t - c·u) / n      for r in S with sqrt(o·o) >= 1e-12
 *   g[r] = (gloss/|S|) · (-2c) · t / 1e-12          for r in S below that
 *   g[r] = 0 exactly                                 for r outside S
 * A row outside S is never read: NaN there reaches neither the sums nor g (torch autograd turns 0 · NaN into NaN).  |S| = 0:
 * loss and mad are NaN, as torch's empty mean, and g is all zero.
 * y and g: rows of 3 floats with a pitch (ldy, ldg) of 3 or 4 floats (SN_E_SHAPE otherwise); a pitch-4 operand that is 16-byte
 * aligned moves as one 16-byte word per row — the fourth float of EVERY row must be addressable.  The fourth column of a
 * pitch-4 g is written 0, 16-byte aligned or not.  target: (rows, 3), ldt >= 3.  frame: NULL or a (rows, 3) view, ldf >= 3.  All 4-byte aligned (SN_E_ALIGN).
 * out: 3 floats on the device — loss, mad and |S| (the number the gradient entries divide by).
 *   sn_normal_cosine_fwd_f32   loss and mad only (evaluation).
 *   sn_normal_cosine_fwdg_f32  the same sums in the same order — the same bits — and g for gloss == 1.  g needs 1/|S| before
 *                   its first row is stored, so with a rowmask |S| is counted by a small launch AHEAD of the pass (4 bytes per
 *                   row); without one it is `rows`.
 *   sn_normal_cosine_bwd_f32   g for the DEVICE scalar gloss from the operands again; count = out + 2 of a forward call.
 *   sn_normal_cosine_bwdg_f32  the same over a g that sn_normal_cosine_fwdg_f32 filled for the same operands: kept when
 *                   gloss[0] == 1 (tested on the device), recomputed otherwise; the same bits as sn_normal_cosine_bwd_f32.
 * No atomics, no memset, nothing that synchronises: every entry can be captured into a hipGraph.
 * sn_normal_cosine_grid_rows: the rows one sweep of the forward grid covers (more rows: every thread walks on). */
int64_t sn_normal_cosine_grid_rows(void);
size_t sn_normal_cosine_workspace_bytes(int64_t rows);
int sn_normal_cosine_fwd_f32(const float *y, int64_t ldy, const float *frame, int64_t ldf, const float *target, int64_t ldt,
                             const float *rowmask, int64_t rows, float *out, void *workspace, size_t workspace_bytes,
                             void *stream);
int sn_normal_cosine_fwdg_f32(const float *y, int64_t ldy, const float *frame, int64_t ldf, const float *target, int64_t ldt,
                              const float *rowmask, int64_t rows, float *out, float *gout, int64_t ldg, void *workspace,
                              size_t workspace_bytes, void *stream);
int sn_normal_cosine_bwd_f32(const float *y, int64_t ldy, const float *frame, int64_t ldf, const float *target, int64_t ldt,
                             const float *rowmask, int64_t rows, const float *count, const float *gloss, float *gout,
                             int64_t ldg, void *stream);
int sn_normal_cosine_bwdg_f32(const float *y, int64_t ldy, const float *frame, int64_t ldf, const float *target, int64_t ldt,
                              const float *rowmask, int64_t rows, const float *count, const float *gloss, float *gout,
                              int64_t ldg, void *stream);
/* ---- Sibling-pair pooling ---------------------------------------------------------------------------------------------------
 * The two parameter-free pooling operations of the cascade model (cascade.LapCascade) and their backward passes, over the node
 * axis of a hierarchy whose siblings are neighbours: fine rows 2 j and 2 j + 1 are the children of coarse row j.
 * Replaces: src/normal_predict/models.py:568-576 (EfficientCascade._Pooling: MaxPool1d(2, stride=2) and
 * F.interpolate(scale_factor=2) between two transposes) and the in-place skip `x += down_series[-i]` of models.py:597.
 * Operands are row-major fp32 matrices of C >= 1 columns with leading dimensions >= C (SN_E_SHAPE otherwise): `pairs` coarse rows,
 * 2 * pairs fine rows.  A (B, V, C) batch with even V is the matrix of B * V fine rows: no pair crosses a sample.
 *   sn_pool_max2_fwd_f32     y[j, c] = second ? x[2 j + 1, c] : x[2 j, c],   second = x[2 j + 1, c] > x[2 j, c] or x[2 j + 1, c] is NaN
 *                            — torch's MaxPool1d choice: a tie keeps the first, (NaN, v) keeps the first (the NaN), (v, NaN) and
 *                            (NaN, NaN) take the second.  The chosen element is copied: its bits, a NaN's payload included.
 *   sn_pool_max2_bwd_f32     gx[2 j + s, c] = g[j, c] for the chosen s, 0 for the other; the choice is made again from x (no index
 *                            tensor is kept).  Every element of gx is written.
 *   sn_unpool2_add_fwd_f32   y[2 j + s, c] = x[j, c] + skip[2 j + s, c],  s = 0, 1: nearest-neighbour upsampling and the skip
 *                            connection in one pass, one fp32 add per element.  No operand may alias an output.
 *   sn_unpool2_bwd_f32       gx[j, c] = g[2 j, c] + g[2 j + 1, c]   (the gradient of skip is g itself: no kernel)
 * C a multiple of 4 with 16-byte aligned bases and leading dimensions that are multiples of 4 moves 16 bytes per lane; anything
 * else one float.  One item per thread and a grid-stride loop past INT_MAX workgroups; no atomics, no memset, nothing that
 * synchronises: every entry can be captured into a hipGraph. */
int sn_pool_max2_fwd_f32(const float *x, int64_t ldx, int64_t pairs, int32_t C, float *y, int64_t ldy, void *stream);
int sn_pool_max2_bwd_f32(const float *x, int64_t ldx, const float *g, int64_t ldg, int64_t pairs, int32_t C, float *gx,
                         int64_t ldgx, void *stream);
int sn_unpool2_add_fwd_f32(const float *x, int64_t ldx, const float *skip, int64_t lds, int64_t pairs, int32_t C, float *y,
                           int64_t ldy, void *stream);
int sn_unpool2_bwd_f32(const float *g, int64_t ldg, int64_t pairs, int32_t C, float *gx, int64_t ldgx, void *stream);
/* ---- Graph attention ----------------------------------------------------------------------------------------------------------
 * The propagation rule of the graph-attention block (attention.GatResNet2, attention.LapGatModel): the weights of the product are
 * computed from the features, per stored entry and per call, with a softmax over each row.  The reference names the block
 * (`pygat.GatResNet2`, src/normal_predict/models.py:85-124) and contains no code for it, and its driver runs it on a dense N x N
 * adjacency only: the definition below is this project's own (pattern-only attention, no dropout); the statement in torch
 * operations is attention.attn_propagate_reference.
 *   A      square CSR operator of R rows, int32.  Only rowptr and colind are read: the values never are.  A stored explicit zero is
 *          an entry like any other.  Column indices must lie in 0 .. R-1 (the kernels do not check, like the products).
 *   e      (R, C) fp32;  H heads, slice k = channels [k C / H, (k + 1) C / H);  a (2, C) fp32, contiguous: row 0 scores a row as a
 *          source, row 1 as a destination;  SN_ATTN_SLOPE = 0.2.
 *   s[j, k]     = sum over slice k of a[0, c] e[j, c]          s[i, H + k] likewise with a[1]                  (s: R x 2H)
 *   u_ij^k      = leaky_relu(s[i, H + k] + s[j, k], SN_ATTN_SLOPE)             for every stored entry (i, j)
 *   alpha_ij^k  = exp(u_ij^k - m_i^k) / z_i^k,   m_i^k = max over row i of u,   z_i^k = sum over row i of exp(u - m)
 *   p[i, slice k] = sum over row i of alpha_ij^k e[j, slice k]
 * A row without a stored entry gives p[i, :] = 0 (and m = z = 0) and sends no gradient anywhere.  The maximum is subtracted before
 * every exponential.  A NaN logit makes the head's slice of that row NaN, as the torch statement does.
 * Supported: C % 4 == 0, 4 <= C <= SN_ATTN_MAX_CHANNELS, C % H == 0, (C / H) % 4 == 0 (sn_attn_supported says 1; SN_E_UNSUPPORTED
 * otherwise); M == K (SN_E_SHAPE otherwise); dense operands with 16-byte aligned bases and leading dimensions that are multiples
 * of 4 and >= C (SN_E_ALIGN / SN_E_LD).  Nothing of size nnz is stored anywhere; no atomics, no memset, nothing that synchronises:
 * two runs give the same bits and every entry can be captured into a hipGraph.
 *   sn_attn_elu_scores_f32     e = elu(x) (the library's ELU, as sn_elu_into_f32) written with leading dimension lde — the first half
 *                              of a stage's (R, 2C) concat buffer — and s from the same registers: one streaming pass.
 *   sn_attn_propagate_fwd_f32  p (leading dimension ldp: the second half of the concat buffer), m and z ((R, H) each, kept for the
 *                              backward pass).  Row-wise over A: a first sweep over a row's column indices takes the maximum from s
 *                              alone, a second one accumulates exp and the weighted rows.
 *   sn_attn_propagate_bwd_f32  g: the gradient of p.  dx = de, or with ge (the gradient of the e half of the concat buffer, may be
 *                              NULL)  dx = (de + ge) * elu'(e)  — the gradient of x;  da (2, C).  With D_i^k = <g[i, k], p[i, k]> and
 *                              dpre_ij = alpha_ij (<g[i, k], e[j, k]> - D_i^k) * (1 where the logit's argument is > 0, else the slope):
 *                                pass 1, rows of A:    ds[i, H + k] = sum_j dpre_ij
 *                                pass 2, rows of A^T:  ds[j, k] = sum_i dpre_ij,   de[j, slice k] = sum_i alpha_ij g[i, slice k]
 *                                                      + ds[j, k] a[0] + ds[j, H + k] a[1]        (alpha recomputed from s, m, z)
 *                                da = column sums of ds (x) e: one partial per workgroup of pass 2, added in a fixed order in float64.
 *                              t_rowptr / t_colind: the CSR pattern of A^T.  workspace: sn_attn_propagate_bwd_workspace_bytes(R, C, H),
 *                              else SN_E_WORKSPACE.  dx must not overlap an input. */
#define SN_ATTN_MAX_CHANNELS 256
#define SN_ATTN_SLOPE        0.2
int32_t sn_attn_supported(int32_t C, int32_t H);
int sn_attn_elu_scores_f32(const float *x, int64_t ldx, const float *a, int64_t R, int32_t C, int32_t H, float *e, int64_t lde,
                           float *s, void *stream);
int sn_attn_propagate_fwd_f32(const int32_t *rowptr, const int32_t *colind, int64_t M, int64_t K, int64_t nnz, const float *e,
                              int64_t lde, const float *s, int32_t C, int32_t H, float *p, int64_t ldp, float *m, float *z,
                              void *stream);
size_t sn_attn_propagate_bwd_workspace_bytes(int64_t R, int32_t C, int32_t H);
int sn_attn_propagate_bwd_f32(const int32_t *rowptr, const int32_t *colind, const int32_t *t_rowptr, const int32_t *t_colind,
                              int64_t M, int64_t K, int64_t nnz, const float *g, int64_t ldg, const float *ge, int64_t ldge,
                              const float *e, int64_t lde, const float *p, int64_t ldp, const float *s, const float *m,
                              const float *z, const float *a, int32_t C, int32_t H, float *dx, int64_t lddx, float *da,
                              void *workspace, size_t workspace_bytes, void *stream);
/* ---- Mesh hierarchy -------------------------------------------------------------------------------------------------------------
 * One coarsening step of the hierarchy the cascade model's per-level operators come from (operators.mesh_hierarchy; the numpy
 * statement is mesh_ops.mesh_hierarchy).  The reference names the coarsening of Defferrard et al. 2017 ("the specific construction
 * of permuted nodes", src/normal_predict/models.py:591) and contains no code for it: this is the project's own definition.
 * L: square CSR, fp32, columns ascending inside a row.  All arithmetic fp32, no contraction, divisions correctly rounded.
 *   score     for a stored off-diagonal entry  s_ij = fl(|L_ij| / |L_ii|) + fl(|L_ji| / |L_jj|),  L_ji the stored entry or 0;
 *             s_ij = 0 where either diagonal entry is 0 or absent.  s_ij and s_ji have the same bits (the add commutes).  For
 *             L = M^-1 C the mass cancels: w_ij (1 / d_i + 1 / d_j), the normalised cut of Graclus.
 *   matching  in a round every unmatched i proposes to the unmatched neighbour j with the largest s_ij > 0, ties to the smallest j;
 *             mutual proposals become pairs; rounds repeat until one makes no pair; what is left are singletons.  Every round
 *             with an eligible edge makes a pair (the smallest endpoint among the globally best edges and its choice are mutual).
 *             A round past max_rounds that would still make a pair makes none and raises SN_HIER_NOT_FINISHED.
 *   weights   r_i = m_i / (m_i + m_mate(i)) and msum_i = fl(m_i + m_mate(i)) for a matched i, r_i = 1 and msum_i = m_i for a
 *             singleton; mass NULL: every m_i = 1.
 * The rest of a level is built from these by the caller: clusters numbered by the rank of their smallest member, P (n x n_c, ones)
 * and R (n_c x n, the r of a cluster's members in ascending order), and the coarse operator R (L P) with sn_csr_spgemm_f32 and its
 * summation order, i.e.  L_c[c, d] = fl(fl(r_a t_ad) + fl(r_b t_bd)),  t_id = the sequential sum of L_ij over parent(j) = d in
 * ascending j, exact zeros dropped: the aggregation Galerkin operator M_c^-1 P^T M L P.
 * sn_mesh_match_f32: ONE workgroup of SN_HIER_THREADS threads walks the operator; the rounds run inside the kernel, propose and
 * accept separated by barriers, no host read-back.  mate[n]: partner or -1; r[n], msum[n]; out[2] = {rounds that made pairs,
 * status word}.  A column index outside 0 .. n-1 raises SN_HIER_BAD_COLUMN and nothing is matched.
 * workspace: sn_mesh_match_workspace_bytes(n, nnz). */
#define SN_HIER_NOT_FINISHED  1
#define SN_HIER_BAD_COLUMN    2
#define SN_HIER_THREADS       1024
size_t sn_mesh_match_workspace_bytes(int64_t n, int64_t nnz);
int sn_mesh_match_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, const float *mass, int64_t n, int64_t nnz,
                      int32_t max_rounds, int32_t *mate, float *r, float *msum, int32_t *out, void *workspace,
                      size_t workspace_bytes, void *stream);
/* sn_gather_segments_f32: batch assembly of dense per-sample windows (the ARAP sampler's inputs / targets,
 * src/as_rigid_as_possible/main.py:126-152): out[(i*rows_per_item + r)*len + c] = src[base[i] + r*row_stride + c],
 * i < nitems, r < rows_per_item, c < len; base is a DEVICE array of element offsets into the resident dataset. */
int sn_gather_segments_f32(const float *src, const int64_t *base, int64_t nitems, int64_t rows_per_item, int64_t row_stride,
                           int32_t len, float *out, void *stream);
/* ... straight into a PACKED batch (no padded intermediate, no boolean-mask gather): item i supplies its first
 * item_off[i+1] - item_off[i] rows, written to output rows item_off[i] ..; item_off: int64[nitems + 1] on the device,
 * total_rows = item_off[nitems] (known to the caller, who built the table). */
int sn_gather_segments_ragged_f32(const float *src, const int64_t *base, const int64_t *item_off, int64_t nitems,
                                  int64_t total_rows, int64_t row_stride, int32_t len, float *out, void *stream);
/* sn_pair_argmin_f32: target of the dense-correspondence loss (src/dense_correspondence/main.py:236-237,
 * `_, GAB = torch.min(GA[:, liA[lB]] + GB[liB[lA], :], dim=1)`):  out[r] = argmin_j ( GA[r*ldA + pa[j]] + GB[pb[r]*ldB + j] ),
 * r < NA, j < NB, with pa = liA[lB] (NB entries) and pb = liB[lA] (NA entries) as DEVICE int64 arrays; the two gathered
 * NA x NB matrices are never materialised.  fp32 sum as in the reference; ties go to the lowest j, a NaN wins (torch.min).
 * GA has colsA valid columns per row (rows up to 60 KB are staged in LDS, wider ones gathered from global memory); the
 * caller guarantees 0 <= pa[j] < colsA and that pb[r] indexes a row of GB. */
int sn_pair_argmin_f32(const float *GA, int64_t ldA, int64_t colsA, const int64_t *pa, const float *GB, int64_t ldB,
                       const int64_t *pb, int64_t NA, int64_t NB, int64_t *out, void *stream);
/* sn_pair_ce_fwd_f32 / sn_pair_ce_bwd_f32: the cross entropy of the dense-correspondence loss on the score matrix
 * (src/dense_correspondence/main.py:238-239, `F.cross_entropy(outputs[0, :NA, :NB], GAB)`; replaces log_softmax, nll_loss,
 * their backward passes and the zero padding of the slice's gradient).  Forward: lse[r] = log sum_j<NB exp(S[r][j]) and
 * rowloss[r] = lse[r] - S[r][target[r]] for r < NA (the loss is their mean; the caller sums NA floats).  Backward:
 * dS[r][j] = (*gloss / NA) * (softmax(S[r][:NB])[j] - [j == target[r]]) for r < NA, j < NB and 0 for the rest of the
 * rows x cols matrix (the padding of the batch); gloss is a DEVICE scalar.  fp32 throughout, max-subtracted like torch's.
 * 0 <= target[r] < NB is the caller's guarantee (not checked on the device). */
int sn_pair_ce_fwd_f32(const float *S, int64_t ld, const int64_t *target, int64_t NA, int64_t NB, float *lse, float *rowloss,
                       void *stream);
int sn_pair_ce_bwd_f32(const float *S, int64_t ld, const int64_t *target, const float *lse, const float *gloss, int64_t NA,
                       int64_t NB, int64_t rows, int64_t cols, float *dS, int64_t ldd, void *stream);
/* sn_pair_fused_fwd_f32 / sn_pair_fused_bwd_f32: the same loss computed FROM THE TOWER FEATURES, the score matrix never
 * written (replaces `torch.bmm(FA, FB.transpose(1, 2))`, src/dense_correspondence/models.py:203, together with the cross
 * entropy of main.py:238-239 and both their backward passes).  FA: rowsA x K, FB: rowsB x K row-major fp32 (K <= 128; the
 * towers emit 120), the first NA / NB rows are scored, the rest is the padding of the batch.  Scores are formed tile by tile
 * on the bf16 matrix pipe from three-piece truncation splits of the features (six exact partial products per term, fp32
 * accumulation: fp32-accurate, not bit-equal to an fp32 FMA chain) and reduced on the spot.
 *   forward : lse[r], rowloss[r] (r < NA) as sn_pair_ce_fwd_f32; the split features are left in `workspace`
 *             (sn_pair_fused_workspace_bytes(rowsA, rowsB) bytes, 16-byte aligned) for the backward pass.
 *   backward: dFA[r][k] = (*gloss / NA) sum_j (softmax(S[r])[j] - [j == target[r]]) FB[j][k] and
 *             dFB[j][k] = (*gloss / NA) sum_r (...) FA[r][k]; rows >= NA / NB of dFA / dFB are set to 0.  Reads the workspace
 *             the forward call filled (same rowsA, rowsB, K) and its lse.  Fixed summation order: run-to-run identical.
 * 0 <= target[r] < NB is the caller's guarantee. */
size_t sn_pair_fused_workspace_bytes(int64_t rowsA, int64_t rowsB);
int sn_pair_fused_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *target, int64_t NA,
                          int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, float *lse, float *rowloss, void *workspace,
                          size_t workspace_bytes, void *stream);
int sn_pair_fused_bwd_f32(const int64_t *target, const float *lse, const float *gloss, int64_t NA, int64_t NB, int64_t rowsA,
                          int64_t rowsB, int32_t K, float *dFA, int64_t ldda, float *dFB, int64_t lddb, void *workspace,
                          size_t workspace_bytes, void *stream);
/* sn_pair_soft_* / sn_pair_sl1_*: the other two losses of the FAUST driver FROM THE TOWER FEATURES — the soft-target cross
 * entropy `cel` (loss_fun_cross_entropy, src/dense_correspondence/main.py:216-227) and the smooth-L1 `sl1` (loss_fun_sl1 with
 * aggregate_batch_G, main.py:197-214) — replacing bmm(FA, FB^T) (models.py:203), the two gathered matrices
 * GA[:, liA[lB]] and GB[liB[lA], :], their sum, softmin / log_softmax / smooth_l1 and all their backward passes.  Neither the
 * scores nor any other NA x NB temporary is written.  Arithmetic and workspace of sn_pair_fused_*.
 * The geodesic sum is read in LABEL ORDER: geo is a DEVICE array of two device pointers {HA, HB}, row-major fp32 with leading
 * dimensions ldgA, ldgB >= NB, and G[u][v] = HA[u][v] + HB[u][v] (fp32 + fp32) for u < NA, v < NB.  Row u of G belongs to
 * row mapA[u] of FA and column v to row mapB[v] of FB (int64 permutations of [0, NA) / [0, NB) on the device; NULL =
 * identity); rows of FA / FB past NA / NB are the padding of the batch and keep their place.  With label / label_inv
 * mutually inverse, H = G_frame[label_inv][:, label_inv] and map = label_inv reproduce main.py:200-201 / 219-220.
 *   soft fwd: stats[u] = log sum_v exp(S[u][v]), stats[NA + u] = min_v G[u][v] - log sum_v exp(min - G[u][v]) (so that
 *             softmin(G[u])[v] = exp(stats[NA + u] - G[u][v])), rowloss[u] = stats[u] - sum_v softmin(G[u])[v] S[u][v], u < NA,
 *             v < NB; the loss is the SUM of rowloss (main.py:225 sums, it does not average).
 *   soft bwd: dS = *gloss (softmax(S[u]) - softmin(G[u])) inside the corner, 0 outside; dFA = dS·FB, dFB = dS^T·FA written to
 *             rows mapA[u] / mapB[v]; rows >= NA / NB are set to 0.
 *   sl1 fwd : rowloss[u] (fp64, u < rowsA) = sum_{v < rowsB} l(S[u][v] - FullG[u][v]), FullG = G in the corner and 0 in the
 *             padding (main.py:206-210), l(d) = d^2/2 for |d| < 1, |d| - 1/2 otherwise; the loss is sum / (rowsA rowsB).
 *   sl1 bwd : dS = *gloss clamp(S - FullG, -1, 1) / (rowsA rowsB) over the whole rectangle: padding rows of dFA / dFB are
 *             in general not 0.
 * The backward calls read the workspace their forward call filled (sn_pair_loss_workspace_bytes, 16-byte aligned) with the
 * same maps and geo.  Fixed summation order: run-to-run identical.  gloss is a DEVICE scalar. */
size_t sn_pair_loss_workspace_bytes(int64_t rowsA, int64_t rowsB);
int sn_pair_soft_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *mapA, const int64_t *mapB,
                         const float *const *geo, int64_t ldgA, int64_t ldgB, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB,
                         int32_t K, float *stats, float *rowloss, void *workspace, size_t workspace_bytes, void *stream);
int sn_pair_soft_bwd_f32(const int64_t *mapA, const int64_t *mapB, const float *const *geo, int64_t ldgA, int64_t ldgB,
                         const float *stats, const float *gloss, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K,
                         float *dFA, int64_t ldda, float *dFB, int64_t lddb, void *workspace, size_t workspace_bytes, void *stream);
int sn_pair_sl1_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *mapA, const int64_t *mapB,
                        const float *const *geo, int64_t ldgA, int64_t ldgB, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB,
                        int32_t K, double *rowloss, void *workspace, size_t workspace_bytes, void *stream);
int sn_pair_sl1_bwd_f32(const int64_t *mapA, const int64_t *mapB, const float *const *geo, int64_t ldgA, int64_t ldgB,
                        const float *gloss, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, float *dFA, int64_t ldda,
                        float *dFB, int64_t lddb, void *workspace, size_t workspace_bytes, void *stream);
/* sn_pair_match_f32: what the trained network PREDICTS, from the tower features — for every vertex of shape A the vertex of
 * shape B with the largest score and, optionally, the reverse and the geodesic error of the match.  Replaces
 * `torch.bmm(FA, FB.transpose(1, 2))` (src/dense_correspondence/models.py:203) followed by a row maximum (and a column
 * maximum, and a gather from the geodesic matrix): the scores are formed tile by tile as in sn_pair_fused_fwd_f32 (the same
 * two-piece products per element, plain vertex order; the per-matrix scale is taken over the scored rows only, where that
 * entry point takes it over all rowsA / rowsB) and reduced on the spot; no NA x NB temporary is written.
 *   colA[r] = argmax_{j < NB} S[r][j], bestA[r] = that score, r < NA; rowB[j] = argmax_{r < NA} S[r][j], bestB[j], j < NB
 *   (rowB and bestB may be NULL together: the second direction is then not computed).  A strictly larger score wins and on
 *   equal scores the smaller index (numpy.argmax); a NaN score never wins, and every index lies inside the corner whatever
 *   the features hold.  Only the scored rows are read: the padding of the batch (rows >= NA / NB) cannot move a result.
 *   errA[r] = geoB[truthA[r] * ldgB + colA[r]] for 0 <= truthA[r] < NB, NaN otherwise: geoB is row-major fp32 with at least NB
 *   rows and ldgB >= NB, truthA (int64[NA]) the vertex of B that row r of A truly corresponds to; geoB, truthA and errA are all
 *   NULL or all set.
 * workspace: sn_pair_match_workspace_bytes(rowsA, rowsB) bytes, 16-byte aligned (the split features and the per-range
 * partials; smaller than sn_pair_fused_workspace_bytes: no transposed copies, no gradient partials).  Run-to-run identical. */
size_t sn_pair_match_workspace_bytes(int64_t rowsA, int64_t rowsB);
int sn_pair_match_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, int64_t NA, int64_t NB, int64_t rowsA,
                      int64_t rowsB, int32_t K, int64_t *colA, float *bestA, int64_t *rowB, float *bestB, const float *geoB,
                      int64_t ldgB, const int64_t *truthA, float *errA, void *workspace, size_t workspace_bytes, void *stream);
/* sn_linear_thin_fwd_f32: forward of that first layer, y = x·W^T + bias (x: rows x C, C <= 8; W: J x C), and optionally
 * elu(y) into y_elu (the first half of the next block's concat buffer; replaces the F.elu of utils_pt.py:161,195).  y or
 * y_elu may be NULL (not both).  Ascending-k fp32 FMA chain on top of the bias. */
int sn_linear_thin_fwd_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *bias, int64_t rows,
                           int32_t C, int32_t J, float *y, int64_t ldy, float *y_elu, int64_t lde, void *stream);
int sn_affine_cols_acc_f32(float *dx, int64_t lddx, const float *x, int64_t ldx, const float *center, const float *B,
                           const float *Cc, int64_t rows, int32_t C, void *stream);
/* sn_affine_cols_elu_bwd_f32: the same tail for a layer whose operand x is itself the output of an ELU (the models' last
 * layer, `conv2(F.elu(v))`, src/as_rigid_as_possible/models.py:149-150), continued through that activation in the same
 * pass:  dx[r,c] = (dx[r,c] + (x[r,c]-center[c])*B[c] + Cc[c]) * (x[r,c] > 0 ? 1 : x[r,c] + 1).  B = Cc = NULL: no
 * BatchNorm tail (eval mode).  Replaces the tail pass + ELUBackward. */
int sn_affine_cols_elu_bwd_f32(float *dx, int64_t lddx, const float *x, int64_t ldx, const float *center, const float *B,
                               const float *Cc, int64_t rows, int32_t C, void *stream);

/* Small coefficient kernels of the folded BatchNorm+Linear (they replace ~40 tiny elementwise launches per layer):
 * sn_bn_fold_f32 : from the column statistics (stats = [sums | sums of squares], fp64, `rows` rows) or, when
 *   training == 0, from running_mean / running_var, compute mean[C], invstd[C], s = gamma*invstd, t = beta - mean*s,
 *   Wf = W·diag(s) (J x C), bf = b + W·t; in training mode also update running_mean / running_var in place with
 *   `momentum` and the unbiased variance, as nn.BatchNorm1d does, and add 1 to *num_batches_tracked (may be NULL).
 *   b may be NULL.
 * sn_bn_bwd_coeffs_f32 : from Gc = dyᵀ·(x - mean) (J x C), the column sums of dy (fp64, first J entries of `dystats`),
 *   W, s, invstd, mean, beta: dW = s∘Gc + colsum(dy) ⊗ beta, db = colsum(dy), dgamma = invstd ∘ sum_j W∘Gc,
 *   dbeta = colsum(dy)·W, and the coefficients of the elementwise tail Bc = -s∘invstd∘dgamma/rows, Cc = -s∘dbeta/rows. */
int sn_bn_fold_f32(const double *stats, int64_t rows, const float *gamma, const float *beta, const float *W,
                   const float *b, int32_t J, int32_t C, double eps, double momentum, int32_t training,
                   float *running_mean, float *running_var, float *mean, float *invstd, float *s, float *t,
                   float *Wf, float *bf, int64_t *num_batches_tracked, void *stream);
/* sn_colstats_partial_f32 : the statistics pass over x WITHOUT its final reduction — partial[sn_colstats_blocks(rows)][2][C]
 * fp64, the producer format of sn_colstats_merge_f64.
 * sn_wgrad_bounded_enabled / sn_gemm_variant : what the process-wide baseline switch SN_GEMM_VARIANT resolved to (read once):
 * 1 / 2 with the shipped 16-bit matrix-pipe kernels, 0 / 0 with the fp32-MFMA A/B baseline — launchers ask the library
 * instead of parsing the environment themselves. */
int32_t sn_wgrad_bounded_enabled(void);
int32_t sn_gemm_variant(void);
int32_t sn_colstats_blocks(int64_t rows);
int sn_colstats_partial_f32(const float *x, int64_t ld, int64_t rows, int32_t C, double *partial, void *stream);
int sn_bn_bwd_coeffs_f32(const float *Gc, const double *dystats, const float *W, const float *s, const float *invstd,
                         const float *beta, int64_t rows, int32_t J, int32_t C, float *dW, float *db, float *dgamma,
                         float *dbeta, float *Bc, float *Cc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Global-average block helpers (AvgResNet2, src/utils/utils_pt.py:222-243; global_average :120-122).
 * A batch is nseg meshes of rows_per_seg (padded) rows each; mask[r] in {0,1} marks real vertices (may be NULL = all).
 *
 * sn_segment_colsum_f32 : out[seg, c] = sum over the rows r of mesh seg of mask[r] * x[r, c]   (fp64 accumulation,
 *                         two deterministic stages).  Replaces (x * mask).sum(1).
 * sn_bcast_rows_f32     : dst[r, c] = src[seg(r), c]  — writes the per-mesh mean into the second half of the concat
 *                         buffer (expand_as + contiguous + torch.cat in the reference).
 * sn_elu_bwd_bcast_f32  : gsrc[r,c] = (gdst[r,c] + mask[r] * bias[seg(r), c]) * elu'(out[r,c]) + gadd[r,c]: ELU backward
 *                         with the gradient of the mean path folded in (gadd: optional residual-path gradient).
 *
 * Half-width form of a global-average stage.  The second half of its concat buffer [e | mean(e) broadcast] is a per-mesh
 * constant, so the stage needs only e: the BatchNorm statistics of the second half, its share of the Linear product (a
 * per-mesh bias), of the weight gradient and of the input gradient are nseg x C algebra on the per-mesh mean m:
 * sn_avg_fwd_prep_f32   : m = segsum * inv_count;  stats (2 x 2C fp64, the layout sn_bn_fold_f32 reads) = [stats1 |
 *                         rows_per_seg * sum_mesh m, rows_per_seg * sum_mesh m^2]  (stats1 = sn_colstats_f32 of e).
 * sn_avg_stats_f32      : the two above in ONE pass over e (per-mesh masked sums, and sums / sums of squares of all rows,
 *                         fp64): m and stats as sn_avg_fwd_prep_f32 would produce them from sn_segment_colsum_f32 +
 *                         sn_colstats_f32.
 * sn_seg_affine_f32     : out[g, j] = bias[j] + sum_c A[g, c] * W[j, c]  — the per-mesh bias  m·Wf[:, C:]^T + bf  consumed
 *                         by sn_linear_fwd_segbias_f32.
 * sn_avg_bwd_gc_f32     : Gc (J x 2C) = [ G1 | sum_mesh seg_dy[mesh]^T (m[mesh] - mu2) ]  (G1 = sn_wgrad_f32 of the first
 *                         half, seg_dy = sn_segment_colsum_f32 of dy): the operand of sn_bn_bwd_coeffs_f32.
 * sn_avg_bwd_segvec_f32 : v[mesh, c] = inv_count[mesh] * ( seg_dy[mesh]·Wf2[:, c] + rows_per_seg * ((m[mesh,c] - mu2[c]) *
 *                         B2[c] + C2[c]) ): gradient of the mean path, added per row (times the row mask) inside
 *                         sn_linear_dgrad_eluseg_f32.
 * sn_bn_fold_seg_f32    : sn_bn_fold_f32 (training mode) of the stage's 2C-wide layer AND sn_seg_affine_f32 in one launch: the
 *                         workgroup that folds output row j also forms segbias[g, j] = bf[j] + m[g]·Wf[j, C:] (same operands,
 *                         same order: the same numbers).  C = the layer's full width (2 x channels of e), <= 256.
 * sn_avg_bn_bwd_f32     : sn_avg_bwd_gc_f32 + sn_bn_bwd_coeffs_f32 + sn_avg_bwd_segvec_f32 in one launch — all three are per
 *                         channel, so the workgroup of 32 channels runs them for its own; bit-identical.  G1 (J x C), dystats,
 *                         seg_dy (nseg x J) from sn_wgrad_seg_f32 / sn_wgrad_slabs_f32; segoff != NULL: ragged meshes (their
 *                         row counts from the offsets) instead of rows_per_seg.  J <= 128, C % 32 == 0.
 * ------------------------------------------------------------------------------------------ */
int sn_bn_fold_seg_f32(const double *stats, int64_t rows, const float *gamma, const float *beta, const float *W, const float *b,
                       int32_t J, int32_t C, double eps, double momentum, float *running_mean, float *running_var, float *mean,
                       float *invstd, float *s, float *t, float *Wf, float *bf, int64_t *num_batches_tracked, const float *seg_mean,
                       int64_t nseg, float *segbias, void *stream);
int sn_avg_bn_bwd_f32(const float *G1, const double *dystats, const float *seg_dy, const float *seg_mean, const float *mu2,
                      const float *W, const float *s, const float *invstd, const float *beta, int64_t rows, int32_t J, int32_t C,
                      int64_t nseg, const float *Wf2, int64_t ldw, const float *inv_count, int64_t rows_per_seg, const int64_t *segoff,
                      float *dW, float *db, float *dgamma, float *dbeta, float *Bc, float *Cc, float *segvec, void *stream);
/* Ragged forms for PACKED batches (meshes of different sizes, no padding): the rows of mesh g are cut into tiles of at most
 * 256 rows; tiles is an (ntiles x 3) int64 device table {mesh, first row, rows}, tiles of one mesh consecutive,
 * seg_tile_ptr[nseg + 1] the first tile of every mesh.
 * sn_segment_colsum_ragged_f32 : out[g, c] = scale[g] * sum over the rows r of mesh g of x[r, c]  (fp64, two deterministic
 *                                stages; scale may be NULL).  With scale = 1 / vertex count: global_average on a packed batch.
 * sn_bcast_rows_ragged_f32     : dst[r, :] = src[mesh(r), :]. */
/* sn_avg_prep_ragged_f32        : BatchNorm statistics (2 x 2C fp64, the layout sn_bn_fold_f32 reads) of [e | per-mesh mean
 *                                broadcast] on a packed batch: first half from the statistics partials ([nblk][2][C] fp64) of the
 *                                kernel that wrote e, second half  sum_g len_g m_g,  sum_g len_g m_g^2  from the means and the
 *                                row offsets segoff[nseg + 1]. */
int sn_avg_prep_ragged_f32(const float *seg_mean, const int64_t *segoff, int64_t nseg, int32_t C, const double *stats_part,
                           int32_t nblk, double *stats, void *stream);
size_t sn_segment_colsum_ragged_workspace_bytes(int64_t ntiles, int32_t C);
int sn_segment_colsum_ragged_f32(const float *x, int64_t ld, const int64_t *tiles, int64_t ntiles, const int64_t *seg_tile_ptr,
                                 int64_t nseg, int32_t C, const float *scale, float *out, void *workspace,
                                 size_t workspace_bytes, void *stream);
int sn_bcast_rows_ragged_f32(const float *src, const int64_t *tiles, int64_t ntiles, float *dst, int64_t ldd, int32_t C,
                             void *stream);
size_t sn_segment_colsum_workspace_bytes(int64_t rows_per_seg, int64_t nseg, int32_t C);
int sn_segment_colsum_f32(const float *x, int64_t ld, const float *mask, int64_t rows_per_seg, int64_t nseg, int32_t C,
                          float *out, void *workspace, size_t workspace_bytes, void *stream);
int sn_bcast_rows_f32(const float *src, float *dst, int64_t ldd, int64_t rows_per_seg, int64_t nseg, int32_t C,
                      void *stream);
int sn_elu_bwd_bcast_f32(const float *gdst, int64_t ldg, const float *out, int64_t ldo, const float *bias,
                         const float *mask, const float *gadd, int64_t ldga, float *gsrc, int64_t ldgs,
                         int64_t rows_per_seg, int64_t nseg, int32_t C, void *stream);
int sn_avg_fwd_prep_f32(const float *segsum, const float *inv_count, int64_t nseg, int32_t C, int64_t rows_per_seg,
                        const double *stats1, float *m, double *stats, void *stream);
size_t sn_avg_stats_workspace_bytes(int64_t rows_per_seg, int64_t nseg, int32_t C);
int sn_avg_stats_f32(const float *e, int64_t ld, const float *mask, const float *inv_count, int64_t rows_per_seg, int64_t nseg,
                     int32_t C, float *m, double *stats, void *workspace, size_t workspace_bytes, void *stream);
int sn_seg_affine_f32(const float *A, int64_t nseg, int32_t K, const float *W, int64_t ldw, const float *bias, int32_t J,
                      float *out, void *stream);
int sn_avg_bwd_gc_f32(const float *G1, const float *seg_dy, const float *m, const float *mu2, int64_t nseg, int32_t J,
                      int32_t C, float *Gc, void *stream);
int sn_avg_bwd_segvec_f32(const float *seg_dy, const float *Wf2, int64_t ldw, const float *m, const float *mu2,
                          const float *B2, const float *C2, const float *inv_count, int64_t rows_per_seg, int64_t nseg,
                          int32_t J, int32_t C, float *out, void *stream);
/* ... for ragged meshes: mesh g has segoff[g+1] - segoff[g] rows (device int64[nseg + 1]) in place of rows_per_seg */
int sn_avg_bwd_segvec_ragged_f32(const float *seg_dy, const float *Wf2, int64_t ldw, const float *m, const float *mu2,
                                 const float *B2, const float *C2, const float *inv_count, const int64_t *segoff, int64_t nseg,
                                 int32_t J, int32_t C, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Device-side construction of the quaternionic Dirac operators from a triangle mesh.
 *
 * Replaces: mesh.dirac(V, F)                      src/utils/mesh.py:35-64  (dense O(F·V) numpy builder, 8 s at V=1000)
 *           with mesh.dist / mesh.area            src/utils/mesh.py:17-26, 67-80
 *           and Q = quaternion_matrix             src/utils/mesh.py:28-33
 * All geometry is evaluated in fp64 with the reference's operation order (no FMA contraction) and rounded to fp32 at
 * the end, exactly like `D.astype('float32')` in the reference's preprocessing (add_laplacian.py:61-65).
 *
 * Inputs : V (nV x 3, fp32 — the dtype the reference stores in its datasets), F (nF x 3, int32).
 * Outputs: four operators in BSR4 (4x4 blocks, explicit zeros):
 *            Di   (4nF x 4nV): block row = face, 3 blocks, block columns ascending
 *            DiA  (4nV x 4nF): block row = vertex, one block per incident face, block columns ascending
 *            DiT = Diᵀ (structure of DiA), DiAT = DiAᵀ (structure of Di)   — for the backward products
 *          di_rowptr[nF+1], di_colind[3nF], di_vals[48nF], diat_vals[48nF];
 *          dia_rowptr[nV+1], dia_colind[3nF], dia_vals[48nF], dit_vals[48nF]   (DiT shares DiA's index arrays,
 *          DiAT shares Di's).  Faces must reference three distinct vertices.
 * workspace: sn_dirac_workspace_bytes(nV, nF).
 * ------------------------------------------------------------------------------------------ */
size_t sn_dirac_workspace_bytes(int64_t nV, int64_t nF);
int sn_dirac_bsr4_from_mesh(const float *V, const int32_t *F, int64_t nV, int64_t nF,
                            int32_t *di_rowptr, int32_t *di_colind, float *di_vals, float *diat_vals,
                            int32_t *dia_rowptr, int32_t *dia_colind, float *dia_vals, float *dit_vals,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Profiling aid (off by default; the library's only global state, mutex-guarded).  While enabled every SpMM launch
 * (sn_spmm_csr_f32 / sn_spmm_bsr4_f32 and their _elubwd forms) is issued with hipExtLaunchKernelGGL so that the KERNEL's own start and stop are
 * stamped into two events: durations carry no marker / kernel-boundary overhead and agree with rocprofv3's kernel trace.
 * sn_timing_drain waits for the recorded launches, writes up to `capacity` durations (ms) and 5 int64 per record
 * {kind (bit 0: 0 csr, 1 blocked; bit 5: RB4 (4x1 row blocks); bit 3: the blocked form is Q3; bit 4: the launch also left column statistics (sn_spmm_q3_stats_f32); bit 1: fused ELU-backward epilogue, E read; bit 2: G read
 *  too), M, K,
 *  nnz (csr) | nblocks (bsr4), N}, and clears the list.  The Linear-layer launchers (forward, input gradient, weight gradient)
 * record themselves the same way: kind 0x100 / 0x200 / 0x400 + a variant number, then rows, input width, operand bytes, output
 * width.  sn_timing_enable(1): everything; (2): the sparse products only (an event pair costs a launch ~2 us of GPU time); (0): off.
 * ------------------------------------------------------------------------------------------ */
int     sn_timing_enable(int32_t on);
int64_t sn_timing_count(void);
int     sn_timing_drain(double *ms, int64_t *meta, int64_t capacity, int64_t *written);

/* ------------------------------------------------------------------------------------------
 * Device-side construction of the mass-normalised cotangent Laplacian  L = A^-1 (D - W)  in CSR.
 *
 * Replaces: mesh.dist / mesh.area / mesh.cotangent_weights     src/utils/mesh.py:17-26, 67-80, 102-112
 *           graph.laplacian(W, normalized=False)               src/utils/graph.py:40-49
 *           L = A * L                                           src/mesh_mnist/add_laplacian.py:47-48
 * fp64 in the reference's operation order (W[i,j] += (-l_ij^2 + l_jk^2 + l_ki^2)/(8a + 1e-6) per face, A[i] += a/3/4
 * twice per incident face in face order, d = column sums of W in ascending row order), rounded to fp32 at the end.
 * Two phases (the caller owns the allocation): phase 0 writes rowptr[nV+1] (row i holds its distinct neighbours with a
 * non-zero weight plus the diagonal); the caller reads rowptr[nV] = nnz, allocates colind/vals, and calls phase 1.
 * A vertex may have at most SN_LAP_MAX_DEGREE incident faces (else SN_E_UNSUPPORTED is reported through *status_flag).
 * workspace: sn_laplacian_workspace_bytes(nV, nF) — must be the same buffer for both phases.
 * ------------------------------------------------------------------------------------------ */
#define SN_LAP_MAX_DEGREE 24
size_t sn_laplacian_workspace_bytes(int64_t nV, int64_t nF);
int sn_laplacian_csr_from_mesh(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase,
                               int32_t *rowptr, int32_t *colind, float *vals, int32_t *status_flag,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Geodesic distance matrices: all-pairs shortest paths along the edges of a graph (a mesh's vertex adjacency).
 *
 * Replaces: nothing computed by the reference — it loads `dist_mat` from its .npz frames (src/dense_correspondence/main.py:65-104);
 *           this is the one input of the dense-correspondence job that could not be produced from (V, F).
 *
 * Definition.  Graph: vertices 0..n-1 in CSR, int32 rowptr/colind, fp32 weights w >= 0; self-loops and explicit zeros allowed.
 *   Row v lists the edges INTO v: a stored entry (v, u) is the edge u -> v (the sweep pulls along its row).  A mesh's graph
 *   stores both directions with bit-identical weights.
 *   Mesh edge weight of a stored entry (i, j): d = V[i] - V[j] in fp64 from the fp32 coordinates,
 *   w = (float) sqrt((dx*dx + dy*dy) + dz*dz), every product and sum rounded on its own (no fused multiply-add) — numpy's value.
 *   D[s][s] = 0; D[s][v] = the minimum over all edge paths s -> ... -> v of the length accumulated in fp32 from the source
 *   outward, fl(fl(fl(0 + w1) + w2) + ...); +inf where there is no path.  fp32 addition of a non-negative number is monotone,
 *   so this is what a textbook Dijkstra adding in fp32 returns, and equally the unique fixed point of
 *   d[v] = min(d[v], min_u fl(d[u] + w_uv)) from d = inf, d[s] = 0 under ANY relaxation order: results are bit-reproducible.
 *   D is not exactly symmetric (the reverse path accumulates in the other order); the symmetric matrix is min(D, D^T).
 *
 * sn_edge_lengths_csr_f32 : w[e] for every stored entry of an n x n CSR pattern (a column outside 0..n-1 gets +inf).  On the
 *                           pattern of sn_laplacian_csr_from_mesh this is the vertex adjacency with a zero self-loop per row.
 * sn_graph_apsp_f32       : rows src_begin .. src_begin+src_count-1 of D:  out[(s - src_begin) * ldo + v].  One workgroup holds
 *                           the distance vectors of S consecutive sources in LDS (S = sn_graph_apsp_group(n): the largest of
 *                           8, 4, 2, 1 with S * n <= sn_graph_apsp_max_vertices()) and sweeps them to the fixed point, at most n
 *                           sweeps whatever the arrays hold.  *unreached (may be NULL) is OR-ed with 1 when a written row holds
 *                           +inf; the caller clears it.  colind == w == NULL declares a graph without entries.
 *                           n > sn_graph_apsp_max_vertices(): SN_E_UNSUPPORTED, nothing is launched (there is no fallback).
 *                           src_begin + src_count > n: SN_E_SHAPE;  ldo < n: SN_E_LD.
 * sn_graph_apsp_sweeps_f32: the same, and sweeps[g] (may be NULL) = the number of sweeps workgroup g ran (measurement).
 * sn_graph_apsp_threads   : threads per workgroup for n vertices (1024 / 512 / 256 when the LDS holds one / two / more workgroups).
 * sn_symmetrize_min_f32   : G[i][j] = G[j][i] = min(G[i][j], G[j][i]) in place, any n, any ld >= n, no second matrix.
 * ------------------------------------------------------------------------------------------ */
int sn_edge_lengths_csr_f32(const float *V, const int32_t *rowptr, const int32_t *colind, int64_t n, float *w, void *stream);
int64_t sn_graph_apsp_max_vertices(void);
int32_t sn_graph_apsp_group(int64_t n);
int32_t sn_graph_apsp_threads(int64_t n);
int sn_graph_apsp_f32(const int32_t *rowptr, const int32_t *colind, const float *w, int64_t n, int64_t src_begin,
                      int64_t src_count, float *out, int64_t ldo, int32_t *unreached, void *stream);
int sn_graph_apsp_sweeps_f32(const int32_t *rowptr, const int32_t *colind, const float *w, int64_t n, int64_t src_begin,
                             int64_t src_count, float *out, int64_t ldo, int32_t *unreached, int32_t *sweeps, void *stream);
int sn_symmetrize_min_f32(float *G, int64_t n, int64_t ld, void *stream);

/* ------------------------------------------------------------------------------------------
 * Geodesic distance matrices that cross triangles: first-order Eikonal sweeps on a triangle mesh (the Hopf-Lax form of the
 * fast-marching / fast-iterative update, after Bornemann & Rasch).  A vertex pulls from the opposite edge of each incident
 * triangle, not only from its neighbours; the edge paths above are the special case lambda = 0 or 1.
 *
 * Definition.  A corner is a face (i, j, k) seen from one of its vertices: (v; a, b), the other two vertices in face order —
 *   (i; j, k), (j; k, i), (k; i, j).  A face with an index outside 0..nV-1 or with two equal indices contributes no corner and
 *   raises the builder's flag.  Per-corner constants, P = the fp32 coordinates widened to fp64, every product and sum rounded
 *   on its own (no fused multiply-add), three-term sums as (x + y) + z:
 *     e = P_a - P_b,  c = sqrt(e.e),  q = P_b - P_v,  s_b = (q.e) / c,  h = sqrt((q x e).(q x e)) / c   (the cross-product
 *     form, not q.q - s_b^2),  l_a, l_b = the fp32 edge weights of (v, a) and (v, b) by the formula above: bit-identical to
 *     what sn_edge_lengths_csr_f32 returns.  In the plane of the triangle with the line through a and b as an axis, v's foot is
 *     the origin, b lies at s_b, a at s_b + c, and v at height h.
 *   Update of d[v] from one corner, d_a and d_b the stored fp32 values:
 *     cand = min(fl32(d_a + l_a), fl32(d_b + l_b));
 *     in fp64, Delta = d_a - d_b; only if c > 0, h > 0 and |Delta| < c (a NaN or infinite Delta fails this, as intended):
 *       r = sqrt((c - Delta) * (c + Delta));  if s_b * r <= -(h * Delta) <= (s_b + c) * r:
 *       t = d_b + (h * r - s_b * Delta) / c,  cand = min(cand, (float) t).
 *     t is min over lambda in [0, 1] of d_b + lambda * Delta + |P_b + lambda * e - P_v| when the minimiser is interior; the
 *     update is monotone and non-expansive in (d_a, d_b) and needs no causality test.
 *   D[s][.] = the fixed point of d[v] = min(d[v], min over the corners of v of cand) reached from d = +inf, d[s] = 0; only
 *   strict decreases are accepted.  Because the edge candidates are the edge kernel's own fp32 sums and fp32 addition is
 *   monotone, D_triangles <= D_edges elementwise and EXACTLY (sn_graph_apsp_f32 on the same mesh).  Unlike the edge paths the
 *   value is not bit-reproducible across relaxation orders: the fp64 evaluation is monotone only up to its rounding, so two
 *   orders may differ by a few fp32 ulps.  First order: the error against the true surface distance falls with the mesh
 *   width; obtuse triangles are not unfolded (the scheme stays valid there, only less accurate).  Not exact polyhedral
 *   geodesics.
 *
 * Corner table: CSR by vertex.  cptr[nV + 1] int32, then per corner one record of SN_MESH_CORNER_BYTES = 40 bytes:
 *   int32 a, b; float l_a, l_b; double c, s_b, h.  The order of the corners of a vertex is not deterministic (atomic cursor);
 *   the minimum does not depend on it.
 *
 * sn_mesh_corners_f32        : cptr and the records from (V, F) on the device: count, scan, fill; `corners` holds 3 * nF
 *                              records, the first cptr[nV] of them are written.  *status_flag (may be NULL) is cleared, then set
 *                              to 1 when a face was dropped.  workspace: sn_mesh_corners_workspace_bytes(nV), else SN_E_WORKSPACE.
 * sn_mesh_geodesics_f32      : rows src_begin .. src_begin+src_count-1 of D, out[(s - src_begin) * ldo + v]; dispatch, LDS
 *                              layout and limits of sn_graph_apsp_f32 (sn_graph_apsp_group / _threads / _max_vertices).  At
 *                              most n sweeps.  A corner whose a or b lies outside 0..n-1 is skipped.  *flags (may be NULL;
 *                              the caller clears it) is OR-ed with 1 when a written row holds +inf and with 2 when the n-th
 *                              sweep of a workgroup still changed something (not converged).  corners == NULL declares a
 *                              table without corners.  Status codes as sn_graph_apsp_f32.
 * sn_mesh_geodesics_sweeps_f32: the same, and sweeps[g] (may be NULL) = the number of sweeps workgroup g ran.
 * ------------------------------------------------------------------------------------------ */
#define SN_MESH_CORNER_BYTES 40
size_t sn_mesh_corners_workspace_bytes(int64_t nV);
int sn_mesh_corners_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t *cptr, void *corners,
                        int32_t *status_flag, void *workspace, size_t workspace_bytes, void *stream);
int sn_mesh_geodesics_f32(const int32_t *cptr, const void *corners, int64_t n, int64_t src_begin, int64_t src_count,
                          float *out, int64_t ldo, int32_t *flags, void *stream);
int sn_mesh_geodesics_sweeps_f32(const int32_t *cptr, const void *corners, int64_t n, int64_t src_begin, int64_t src_count,
                                 float *out, int64_t ldo, int32_t *flags, int32_t *sweeps, void *stream);

/* ------------------------------------------------------------------------------------------
 * Intrinsic Delaunay Laplacian: edge flips from (V, F) on the device, then L = A^-1 (D - W) on the flipped triangulation.
 *
 * Replaces: mesh.intrinsic_laplacian(V, F)   src/dense_correspondence/main.py:87, src/normal_predict/sampler.py:68 — the
 *           reference imports an unpublished module for it.  Scaling and sign of that matrix are unknown: this is the
 *           project's A^-1 (D - W) on the intrinsic Delaunay triangulation (Bobenko & Springborn 2007; the flip algorithm
 *           of Fisher et al. 2006), NOT a reproduction of it.
 *
 * Input.  V fp32 (nV, 3), F int32 (nF, 3): manifold, consistently oriented, possibly with boundary.  Refusals through the
 *   status word (nothing is flipped then): SN_IDT_BAD_FACE a face with an index outside 0..nV-1 or a repeated index;
 *   SN_IDT_NON_MANIFOLD an edge with more than two faces; SN_IDT_ORIENTATION an edge whose two faces traverse it in the same
 *   direction.
 * State.  Faces F' (nF, 3); fp64 side lengths l' (nF, 3), l'[f] = (|v0 v1|, |v1 v2|, |v2 v0|); glue map G (nF, 3) of face-side
 *   codes 3 g + t, -1 on the boundary.  A Delta-complex, not a simplicial complex: after flips two faces may share two edges,
 *   a face may have a self-edge (both ends the same vertex), one vertex pair may carry several edges — everything is keyed by
 *   face sides, never by vertex pairs.  Start: F' = F, l' in fp64 from the fp32 coordinates as sqrt((dx*dx + dy*dy) + dz*dz), G
 *   from F.
 * Delaunay test of an interior side (f, s) glued to (g, t), f != g: a = the shared length, b, c the other two sides of a face,
 *   cot = ((b*b + c*c) - a*a) / (4 A), A = sqrt(h (h-a) (h-b) (h-c)), h = ((a + b) + c) / 2 in fp64.  The side is
 *   non-Delaunay iff cot_f + cot_g < SN_IDT_THRESHOLD = -1e-12 (part of the definition; the sums are dimensionless).  A face
 *   whose Heron radicand is <= 0 is degenerate: its sides are never flipped and SN_IDT_DEGENERATE is set when one is tested.
 *   A side glued to another side of its own face is always Delaunay and is never flipped.
 * Flip.  Both faces rotated so that the shared side is side 0, f = (i, j, k), g = (j, i, m):  f = (k, i, m) with lengths
 *   (l_ki, l_im, l_km), g = (m, j, k) with (l_mj, l_jk, l_km).  l_km from the planar layout i = (0, 0), j = (a, 0):
 *   x_k = ((a*a + l_ki*l_ki) - l_jk*l_jk) / (2a), y_k = sqrt(max((l_ki - x_k)(l_ki + x_k), 0)) >= 0, likewise x_m from
 *   (l_im, l_mj) and y_m <= 0, l_km = sqrt(dx*dx + dy*dy).  Sides 2 of the new faces are glued to each other; the four outer
 *   sides keep their partners — a partner that is itself one of the four old outer sides is remapped first (the
 *   Delta-complex case).
 * Result.  The fixed point: no interior side is non-Delaunay; unique in connectivity unless four vertices are cocircular,
 *   whatever the flip order.  A round is two launches (kernel boundaries are the only cross-workgroup ordering): idt_claim_k —
 *   every non-Delaunay side with 3f+s < 3g+t writes its 64-bit word (0xFFFFF - round, a 12-bit hash of (side code, round),
 *   side code) by integer atomic min into a claim word of f, of g and of the up to four faces across their outer sides;
 *   idt_flip_k — a side that holds all its claims flips, and nobody else reads or writes those faces in that round.  The
 *   words of a round are distinct (the code is in them), so the smallest one always wins: every round with work makes
 *   progress, the schedule is a function of the input alone and two runs are bit-identical.  The hash shuffles the priority
 *   per round; the bare code leaves chains of waiting sides along the face numbering (1569 rounds instead of 27 on a
 *   6890-vertex torus).  Rounds past convergence are no-ops.  max_rounds <= 2^20, else SN_E_RANGE.
 *   SN_IDT_NOT_CONVERGED: round max_rounds - 1 still found a non-Delaunay side.
 * Laplacian of (F', l'), this project's convention: a = Heron area with the 1e-6 floor; for every face and every ordered
 *   pair (p, q, r) of its corners (the six permutations in lexicographic order), i = F'[p], j = F'[q]:
 *     W[i, j] += ((-l_pq^2 + l_qr^2) + l_rp^2) / (8a + 1e-6),  d[i] += ((-l_pq^2 + l_rp^2) + l_qr^2) / (8a + 1e-6)  (the
 *     mirror term W[j, i]: d = column sums of W),  A[i] += a / 3 / 4;  a pair with i == j (a self-edge) adds its mass only:
 *     W[i, i] cancels in D - W.  L[i, j] = (0 - W[i, j]) / (A[i] + 1e-9), L[i, i] = d[i] / (A[i] + 1e-9), fp64, rounded once
 *     to fp32.  Pattern: every vertex pair joined by at least one intrinsic edge plus the whole diagonal, stored whatever the
 *     value (nothing is dropped for being zero: the pattern does not depend on rounding), columns ascending.  Every sum runs
 *     serially over its contributions sorted by (face, permutation): no floating-point atomics.  No SN_LAP_MAX_DEGREE limit.
 *
 * sn_mesh_glue_i32          : G (3 nF) from F through a by-vertex bucket of sides; *status is cleared, then OR-ed with the
 *                             refusal bits.  V and l both non-NULL: also the start lengths l (3 nF fp64); both NULL: glue only.
 *                             A refused face gets G = -1 and l = 0.  workspace: sn_mesh_glue_workspace_bytes(nV, nF).
 * sn_mesh_idt_rounds_f64    : rounds round_begin .. round_begin + round_count - 1 of at most max_rounds on (F', l', G) in
 *                             place.  counters (2 * max_rounds int32, caller-owned): counters[2r] = non-Delaunay sides found
 *                             in round r, counters[2r + 1] = flips done; this call clears its own rounds' pairs first.  The
 *                             kernels return at once when *status holds a refusal bit.  workspace:
 *                             sn_mesh_idt_workspace_bytes(nF), the same buffer for every call of one run (round 0 resets it).
 *                             A caller enqueues rounds in chunks and reads the counters once per chunk; a round that found
 *                             nothing is the fixed point.
 * sn_mesh_idt_laplacian_f32 : three phases on one workspace (sn_mesh_idt_laplacian_workspace_bytes(nV, nF)), N =
 *                             sn_mesh_idt_laplacian_items(nV, nF) = 12 nF + nV.  phase 0 writes keys[N] (int64, one per
 *                             contribution; INT64_MAX = none) — the caller sorts them ascending and keeps the permutation
 *                             (order[t] = source index of sorted position t).  phase 1 (count), keys = the SORTED keys: writes
 *                             rowptr[nV + 1]; the caller reads rowptr[nV] = nnz and allocates.  phase 2 (fill): colind, vals.
 *                             A face of F' with an index outside 0..nV-1 contributes nothing and sets SN_IDT_BAD_FACE
 *                             (status may be NULL).  SN_E_RANGE when nV^2 * 16 max(nF, 1) does not fit the int64 key.
 * ------------------------------------------------------------------------------------------ */
#define SN_IDT_BAD_FACE       1
#define SN_IDT_NOT_CONVERGED  2
#define SN_IDT_DEGENERATE     4
#define SN_IDT_NON_MANIFOLD   8
#define SN_IDT_ORIENTATION    16
#define SN_IDT_THRESHOLD      (-1e-12)
size_t sn_mesh_glue_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_glue_i32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t *G, double *l, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream);
size_t sn_mesh_idt_workspace_bytes(int64_t nF);
int sn_mesh_idt_rounds_f64(int32_t *Fp, double *lp, int32_t *G, int64_t nF, int32_t round_begin, int32_t round_count,
                           int32_t max_rounds, int32_t *counters, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream);
int64_t sn_mesh_idt_laplacian_items(int64_t nV, int64_t nF);
size_t sn_mesh_idt_laplacian_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_idt_laplacian_f32(const int32_t *Fp, const double *lp, int64_t nV, int64_t nF, int32_t phase, int64_t *keys,
                              const int64_t *order, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh clean-up: connected components, the largest one, and compaction of what is kept.
 *
 * Replaces: igl.facet_components + scipy.stats.mode + igl.slice + igl.remove_unreferenced
 *           src/dense_correspondence/largest_component.py:28-47 (an off-line libigl script; nothing of it is on the device).
 *
 * Definition.  F int32 (nF, 3) over the vertices 0..nV-1.  A face is BAD when one of its indices lies outside 0..nV-1 or two
 *   of its indices are equal: its flabel is -1, it joins nothing, it is never kept, and *status |= SN_CC_BAD_FACE.  Every
 *   other face is good.  Non-manifold and inconsistently oriented input is welcome (unlike sn_mesh_glue_i32).
 *   SN_CC_VERTEX: two vertices are joined when a good face holds both.  vlabel[v] = the smallest vertex id of v's class; a
 *     vertex no good face uses is a class of its own, vlabel[v] = v.  flabel[f] = vlabel[F[f][0]].  Labels are vertex ids:
 *     count has nV entries.
 *   SN_CC_EDGE (igl.facet_components): two good faces are joined when each has a side on the same unordered vertex pair,
 *     whatever the orientation and however many faces lie on that edge; faces that touch in one vertex only are not joined.
 *     flabel[f] = the smallest face id of f's class.  Labels are face ids: count has nF entries.  vlabel may be NULL and is
 *     not written.
 *   count[l] = the number of good faces with label l (0 for an id that is no label).
 *   summary[0..2] = {number of labels with at least one face, the winning label, its face count}: the winner has the largest
 *     count, the smallest label on a tie — in edge mode the component that contains the lowest face index, scipy.stats.mode's
 *     choice among the reference's first-face-ordered ids.  Without a good face summary = {0, -1, 0}.
 *   All of it is a function of the partition alone: whatever order the threads run in, two runs are bit-identical.
 * Method.  A concurrent union-find over parent[] (the label array itself): a link is one atomicCAS(&parent[hi], hi, lo) between
 *   two roots, the larger under the smaller, so chains strictly decrease and a root is the minimum of its class; find halves
 *   paths with plain stores (only non-roots are rewritten, only roots are CAS targets).  Lock-free: a pass is repeated only
 *   because another thread's link succeeded.  Every loop is bounded by the node count (a chain has at most n nodes, a class is
 *   linked at most n times); a bound that is hit — it cannot be, short of memory written from outside — sets SN_CC_INTERNAL
 *   instead of spinning, and the labels are then not to be used.  Edge mode buckets every side under its lower vertex (count,
 *   scan, fill, as the glue builder) and joins a side's face to the face of the first side of the bucket with the same upper
 *   vertex; the bucket order picks the centre of that star, not the partition.  Every index read from F is range-checked
 *   before it addresses anything.  Histogram: integer atomicAdd; winner: one 64-bit atomicMax per wave over
 *   (count << 32) | (0x7fffffff - label).
 *
 * sn_mesh_components_i32 : vlabel[nV] (vertex mode), flabel[nF], count[nV or nF], summary[3] and *status (cleared first) as
 *                          defined above.  workspace: sn_mesh_components_workspace_bytes(nV, nF, mode), else SN_E_WORKSPACE.
 *                          Another mode: SN_E_SHAPE.  nV + 1 or 3 nF past int32: SN_E_RANGE.  Does not synchronise.
 * sn_mesh_label_mask_i32 : keep[f] = (flabel[f] == *label && *label >= 0), label read on the device: the keep mask of the
 *                          winner (label = summary + 1) without a round trip to the host.
 * sn_mesh_compact_i32    : igl.slice + igl.remove_unreferenced.  Face f stays when keep[f] != 0 and f is good.  Outputs sized
 *                          by the caller for the worst case, the used prefix as sizes[0..1] = {nV', nF'} says:
 *                          I[nV] old -> new vertex id, -1 for a vertex no staying face uses;  J[nV'] new -> old, ascending
 *                          (kept vertices keep their relative order);  Fsrc[nF'] the original index of every staying face,
 *                          ascending;  Fnew[nF'][3] = I[F[Fsrc]];  Vnew[nV'][3] = V[J] bit for bit when V and Vnew are given
 *                          (both or neither).  Marks are idempotent stores of 1, the positions two exclusive int32 scans
 *                          (nF + 1 and nV + 1 entries, any number of scan tiles).  workspace:
 *                          sn_mesh_compact_workspace_bytes(nV, nF), else SN_E_WORKSPACE.  Does not synchronise.
 * ------------------------------------------------------------------------------------------ */
#define SN_CC_EDGE      0
#define SN_CC_VERTEX    1
#define SN_CC_BAD_FACE  1
#define SN_CC_INTERNAL  2
size_t sn_mesh_components_workspace_bytes(int64_t nV, int64_t nF, int32_t mode);
int sn_mesh_components_i32(const int32_t *F, int64_t nV, int64_t nF, int32_t mode, int32_t *vlabel, int32_t *flabel,
                           int32_t *count, int32_t *summary, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream);
int sn_mesh_label_mask_i32(const int32_t *flabel, int64_t nF, const int32_t *label, int32_t *keep, void *stream);
size_t sn_mesh_compact_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_compact_i32(const float *V, const int32_t *F, const int32_t *keep, int64_t nV, int64_t nF, int32_t *I, int32_t *J,
                        int32_t *Fsrc, int32_t *Fnew, float *Vnew, int32_t *sizes, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh repair: weld duplicate vertices, drop duplicate faces, orient every component consistently.
 *
 * Replaces: igl.remove_duplicate_vertices, igl.bfs_orient and the face filter of fix_degen
 *           src/normal_predict/fix_degenerate.py (pyigl on the host; nothing of it is on the device).
 * This is the project's own definition in libigl's conventions, not libigl's bits.  Host statement: mesh_ops.repair_mesh
 * (weld_vertices, unique_faces, orient_faces), vectorised numpy that is not the device algorithm; the device is compared to it
 * bit for bit.  V fp32 (nV, 3), F int32 (nF, 3).
 *
 * Definition.
 *   1. Weld key.  tol == 0: the key of a vertex is its three fp32 coordinates compared AS VALUES, so -0.0 and +0.0 are one key.
 *      tol > 0: the key is rint((double)x / tol) per coordinate — fp64 division, round-half-even — as int64.  A vertex is
 *      UNWELDABLE when a coordinate is not finite or, with tol > 0, a quotient lies outside +-2^62 (an infinite quotient
 *      included).  An unweldable vertex is welded to nothing, and every face that uses one is a bad face
 *      (SN_REPAIR_NONFINITE).  tol > 0 IS A GRID, NOT A BALL: the cells are the cubes [(k - 1/2) tol, (k + 1/2) tol] around the
 *      lattice points k tol.  Two points 0.2 tol apart on either side of a cell border stay apart; two points 0.9 tol apart
 *      inside one cell weld.  No vertex moves: a tolerance only decides who is one class.
 *   2. Weld.  Vertices with equal keys are a class, its representative rep[v] is the smallest vertex id of the class
 *      (rep[v] = v for an unweldable vertex).  F is rewritten through rep; in the rewritten F an unweldable vertex is written
 *      as -1, so that every later step sees its faces as bad, and an index outside 0..nV-1 stays what it is.  The coordinates
 *      of a representative are kept bit for bit (a -0.0 stays -0.0).  With weld == 0 rep[v] = v, and only a non-finite
 *      coordinate makes a vertex unweldable.
 *   3. Bad and duplicate faces.  A face is BAD when it has an index outside 0..nV-1, an unweldable vertex or, after welding, a
 *      repeated index (SN_REPAIR_BAD_FACE); it is never kept.  Two good faces over the same UNORDERED vertex triple are
 *      duplicates, whatever their winding: the smallest face id stays (keep = 1), the others are dropped.  With unique == 0
 *      every good face stays.  counts = {bad faces, duplicate faces, degenerate faces}: a kept face is DEGENERATE when the fp64
 *      squared double-area |(b - a) x (c - a)|^2 — differences of the fp32 coordinates widened to fp64, cross product
 *      (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx), (cx cx + cy cy) + cz cz, no contraction — is exactly 0: a cap or a needle
 *      on three distinct vertices.  Such a face is COUNTED AND KEPT: flipping it away (fix_degen_face_with_flip) changes
 *      connectivity in an order-dependent way and is not done here, nor is orient_outward.
 *   4. Orientation.  Among the kept faces an edge (unordered vertex pair) carried by exactly two faces is a LINK; an edge with
 *      one face, or with three and more, links nothing, and the edges with three and more are counted (nonmanifold edges,
 *      SN_REPAIR_NONMANIFOLD).  The classes of faces under links are the orientation classes; label[f] = the smallest face id
 *      of f's class, -1 for a face that is not kept.  In each class the smallest face id keeps its winding and every other
 *      face gets the winding that makes each link traversed in opposite directions by its two faces: flip[f] = 1 turns
 *      (a, b, c) into (a, c, b).  When no such winding exists (a Moebius band) every face of the class is left as it came
 *      (flip = 0), the class is counted and SN_REPAIR_NONORIENTABLE is set.  counts = {nonmanifold edges, classes without a
 *      consistent winding, classes}.
 *   5. Compaction: sn_mesh_compact_i32 on the oriented faces with the keep mask of step 3.
 *   All of it is a function of the input alone: whatever order the threads run in, two runs are bit-identical.
 * Method.  Steps 2 and 3 use one scheme: an open-addressing table of ids with at least 2 n slots.  A slot is claimed by
 *   atomicCAS(empty -> id) and holds ids of one key from then on; a probe compares its key with the key of the id in the slot,
 *   moves on when they differ and does atomicMin(slot, id) when they agree.  Slots are never emptied, so a class meets in one
 *   slot and a second launch reads its minimum from there: k coincident vertices cost k atomics, not k^2 comparisons.  Step 4
 *   is the union-find of the clean-up section over the faces with the parity to the parent in bit 0 of the word: a link is
 *   atomicCAS(&w[hi], hi << 1, (lo << 1) | p) between two roots, larger under smaller; path halving stores (grandparent,
 *   composed parity) with a plain 32-bit store, and since the parity between a node and an ancestor is fixed by the links made,
 *   every word a reader meets is a valid pair.  Two faces of one link that reach one root with the wrong relative parity flag
 *   that root; a later launch carries the flag to the final root.  The root is the smallest face id and parity 0 means "as it
 *   came", which is the definition.  Lock-free, every loop bounded as in the clean-up section (SN_REPAIR_INTERNAL, results then
 *   not to be used); the packed parity needs nF < 2^30.  Links are found in the side buckets of SN_CC_EDGE built over the kept
 *   faces: a side walks the bucket of its lower vertex, so the cost grows with the square of the number of kept sides that
 *   share one lower vertex (6 on a regular mesh).  Shared words are read and written with relaxed device-scope atomics.
 *
 * sn_mesh_weld_f32         : rep[nV], Fw[nF][3], counts[1] = {vertices with rep[v] != v}, *status (cleared first).  tol < 0 or
 *                            not finite: SN_E_SHAPE.  nV > 2^30 or 3 nF past int32: SN_E_RANGE.  workspace:
 *                            sn_mesh_weld_workspace_bytes(nV), else SN_E_WORKSPACE.  Does not synchronise.
 * sn_mesh_unique_faces_i32 : keep[nF], counts[3], *status (cleared first) of step 3 for the welded F.  V may be NULL: the
 *                            degenerate count is then 0.  workspace: sn_mesh_unique_faces_workspace_bytes(nF).
 * sn_mesh_orient_i32       : flip[nF], label[nF], counts[3], *status (cleared first) of step 4 for the faces with keep[f] != 0
 *                            (a bad face among them is skipped and sets SN_REPAIR_BAD_FACE);  Fout[nF][3] (may be NULL, must
 *                            not be F) = F with the flagged faces turned.  nF >= 2^30: SN_E_RANGE.  workspace:
 *                            sn_mesh_orient_workspace_bytes(nV, nF).  Does not synchronise.
 * None of the three allocates; every fill and copy is a kernel of this library.
 * ------------------------------------------------------------------------------------------ */
#define SN_REPAIR_BAD_FACE       1
#define SN_REPAIR_NONFINITE      2
#define SN_REPAIR_NONORIENTABLE  4
#define SN_REPAIR_NONMANIFOLD    8
#define SN_REPAIR_INTERNAL       16
size_t sn_mesh_weld_workspace_bytes(int64_t nV);
int sn_mesh_weld_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, double tol, int32_t weld, int32_t *rep, int32_t *Fw,
                     int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t sn_mesh_unique_faces_workspace_bytes(int64_t nF);
int sn_mesh_unique_faces_i32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t unique, int32_t *keep,
                             int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t sn_mesh_orient_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_orient_i32(const int32_t *F, const int32_t *keep, int64_t nV, int64_t nF, int32_t *flip, int32_t *label, int32_t *Fout,
                       int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Lattice Delaunay and the Mesh-MNIST maker: images to triangle meshes on the device.
 *
 * Replaces: run()                   src/mesh_mnist/create_data.py:62-99 (a multiprocessing.Pool over 70 000 images)
 *           bilinear_interpolation  src/mesh_mnist/create_data.py:28-36
 *           Grid.poisson            src/mesh_mnist/poisson_disc.py (Bridson's sampling with Python's random)
 *           scipy.spatial.Delaunay  (Qhull on the host)
 * This is the project's own definition on an INTEGER LATTICE, not a reproduction of Python's random stream nor of Qhull's choice
 * among cocircular diagonals.  Host statements: mesh_ops.delaunay_2d, poisson_disc, lattice_intensity, mesh_digits — Python-int
 * arithmetic that is not the device algorithm; the device is compared to them bit for bit.  No transcendental function and no
 * floating-point predicate anywhere.
 *
 * Lattice.  A point is a pair of int32 coordinates with |x|, |y| < 2^24.  orient(a, b, c) = (bx - ax)(cy - ay) - (by - ay)(cx - ax)
 *   fits int64.  incircle(a, b, c, d) = the 3 x 3 determinant of the rows (px - dx, py - dy, (px - dx)^2 + (py - dy)^2), p = a, b,
 *   c; it needs at most 104 bits and is evaluated in __int128.  It is > 0 iff d lies strictly inside the circle through the
 *   counter-clockwise a, b, c.  Float input is snapped by the caller with rint(P / quantum).
 *
 * Delaunay (sn_delaunay2d_i32).  The result is a triangulation of the convex hull of the set: every triangle counter-clockwise
 *   with orient > 0; a point on a hull edge is a boundary vertex (no zero-area triangle exists); no point lies strictly inside the
 *   circle of any triangle.  nF = 2 n - 2 - b, b the number of boundary vertices.  Faces are CANONICAL: each rotated so that its
 *   smallest input index comes first, the faces sorted lexicographically; rows nF .. 2 Nmax - 1 of F are -1.  cocircular = the
 *   number of interior edges of the result whose incircle value is exactly 0: with 0 the triangulation is unique; otherwise the
 *   result is one of the valid ones, a function of the input alone (two runs are bit-identical).
 *   Refusals, per set (nF = 0, the other sets are not affected), the first that applies:
 *     count > SN_DELAUNAY_MAX_POINTS or count > Nmax  SN_DT_TOO_LARGE;   a coordinate with |c| >= 2^24  SN_DT_RANGE;
 *     count < 3  SN_DT_DEGENERATE;   two equal points  SN_DT_DUPLICATE;   all points on one line  SN_DT_DEGENERATE;
 *     a bad edge is left after max_rounds flip rounds  SN_DT_NOT_CONVERGED.  SN_DT_INTERNAL: a loop bound of the sweep was hit
 *     (never for a valid input).
 *   Method.  One workgroup per set, everything in LDS (50 KiB: 1024 points as 64-bit sort keys, 2048 faces and their adjacency as
 *   int16, one claim word per face; a batch with Nmax <= 512 runs the same code at half the capacity and half the LDS).  Bitonic sort by (x, y).  One lane sweeps: the collinear prefix p0 .. p(k-1) is fanned from
 *   the first point pk off their line, then each later point — strictly outside the hull so far, since it is the largest — walks
 *   the hull ring from its predecessor in both directions while orient(a, b, p) < 0 and caps every edge it sees with a triangle
 *   (at most hull-size steps).  Then Lawson flips in claim-then-flip rounds: an interior edge with incircle > 0 does atomicMin of
 *   its id 3 f + s on the claim words of its two faces and their four outer neighbours, and flips in the second half of the round
 *   iff it holds all six, so the flips of one round touch disjoint faces and the smallest bad edge always flips; every flip
 *   strictly improves the triangulation, so the rounds end, and the schedule does not depend on thread timing.  The canonical
 *   keys (three 10-bit indices) are sorted and stored with vector stores.  counts[b] = {flips, cocircular, rounds, boundary}.
 *
 * Poisson-disc sampling (sn_poisson_disc_i32).  Q = 2^16 lattice units per pixel.  The domain is the open rectangle
 *   (0, W Q) x (0, H Q); R = round(r Q) (the caller's); cell = isqrt(R^2 / 2), so a cell holds at most one sample and a sample
 *   closer than R lies within +-2 cells; gw = ceil(W Q / cell), gh = ceil(H Q / cell), gw gh <= SN_DELAUNAY_MAX_POINTS (else
 *   SN_E_UNSUPPORTED); W Q, H Q < 2^24 and 4 <= R, 4 R < 2^31 (else SN_E_RANGE / SN_E_SHAPE).
 *   Random numbers are counter-based: draw(step, cand, retry, purpose) = h4, where h0 = seed and
 *   h(i+1) = mix64(h(i) + 0x9E3779B97F4A7C15 + w(i)) modulo 2^64 for w = (image index, attempt, step, cand << 16 | retry << 8 |
 *   purpose), mix64 the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
 *   z ^= z >> 31).  An integer below m is ((draw >> 32) m) >> 32; the bias of multiply-shift is part of the definition.
 *   Step 0: the first sample is (1 + below(W Q - 1), 1 + below(H Q - 1)) from purposes 0 and 1 (cand = retry = 0).
 *   Step s >= 1, while the active list is not empty: j = below(active count) from purpose 2 picks the active sample a.  Candidate
 *   c = 0 .. 29: for retry t = 0 .. 31, dx = below(4 R) - 2 R (purpose 3), dy likewise (purpose 4), until R^2 <= dx^2 + dy^2 <
 *   4 R^2; a candidate whose 32 draws all fail is invalid.  A candidate a + (dx, dy) is valid when it lies inside the open
 *   rectangle and its squared distance to every sample in the 5 x 5 cells around its own is >= R^2.  The valid candidate with the
 *   LOWEST index becomes the next sample and joins the active list at its end (so lanes test the 30 in parallel and give the
 *   sequential result); with none, a is retired: active[j] = the last active sample, the list shrinks by one.
 *   At most one sample per cell and one retirement per sample: the loop runs at most 2 gw gh steps.  P holds the samples in the
 *   order they were made (rows past count are 0), steps[b] the number of steps taken.
 *
 * Maker (sn_mesh_digits_u8).  images (B, rows, cols) uint8; the domain is W = cols - 1 by H = rows - 1 pixels.  For attempt = 0,
 *   1, .. max_attempts - 1 (max_attempts <= SN_MESHDIGITS_MAX_ATTEMPTS): sample image image_base + b with that attempt number,
 *   refuse the sample when it has fewer than min_points points (101 is the reference's "> 100"; at least 3), triangulate, refuse
 *   it when the triangulation has a status or when any triangle has orient <= min_det.  SN_MESHDIGITS_MIN_DET = floor(0.02 2^32)
 *   states the reference's flat-area test, area <= 1e-2 pixel^2 (orient = 2 area Q^2).  The reference also tests the area of the
 *   triangle in 3-D; a triangle is never smaller than its projection, so the flat test implies it and the 3-D area is not
 *   computed.  The first sample that is not refused is the mesh and attempts[b] its attempt number; when all are refused the
 *   image gets SN_DT_REJECTED, count = nF = 0 and attempts[b] = max_attempts.
 *   Intensity at (x, y), bilinear with the reference's indexing (create_data.py:28-36; the first coordinate runs along the
 *   columns, the second up the rows): iu = x >> 16, fu = x & 0xFFFF, iv = y >> 16, fv = y & 0xFFFF, f00 = I[rows-1-iv][iu], f01 =
 *   I[rows-1-iv][iu+1], f10 = I[rows-2-iv][iu], f11 = I[rows-2-iv][iu+1]; sum = f00 (Q-fv)(Q-fu) + f01 (Q-fv) fu + f10 fv (Q-fu)
 *   + f11 fv fu in int64; z = (float)((double)sum / (255 2^32)).  V = ((float)x 2^-16, (float)y 2^-16, z), exact in fp32.
 *   Outputs, padded to Nmax >= gw gh: P (B, Nmax, 2), count, V (B, Nmax, 3) (rows past count are 0), F (B, 2 Nmax, 3), nF,
 *   status, attempts, counts (B, 4) as sn_delaunay2d_i32's.  One workgroup per image.  Samples are at least R apart, so discs
 *   of radius R / 2 around them are disjoint inside the domain grown by R / 2: n <= 4 (W Q + R)(H Q + R) / (3 R^2) (pi > 3).  When
 *   that bound is at most 512 — it is 481 for MNIST's 27 x 27 pixels at r = 1.5 — the image's state is sized for 512 points and
 *   takes 32 KiB of LDS, otherwise for 1024 points and 62 KiB; the results do not depend on which.
 * None of the three allocates or synchronises; every loop is bounded by the input size.
 * ------------------------------------------------------------------------------------------ */
#define SN_DELAUNAY_MAX_POINTS      1024
#define SN_MESHDIGITS_MAX_ATTEMPTS  8
#define SN_MESHDIGITS_MIN_DET       85899345
#define SN_DT_DEGENERATE     1
#define SN_DT_DUPLICATE      2
#define SN_DT_RANGE          4
#define SN_DT_TOO_LARGE      8
#define SN_DT_NOT_CONVERGED  16
#define SN_DT_REJECTED       32
#define SN_DT_INTERNAL       64
int64_t sn_delaunay2d_max_points(void);
int sn_delaunay2d_i32(const int32_t *P, const int32_t *count, int64_t B, int64_t Nmax, int32_t max_rounds, int32_t *F, int32_t *nF,
                      int32_t *status, int32_t *counts, void *stream);
int64_t sn_poisson_disc_cells(int64_t W, int64_t H, int64_t R);     /* gw gh, or a negative SN_E_* */
int sn_poisson_disc_i32(uint64_t seed, int64_t image_base, int32_t attempt, int64_t W, int64_t H, int64_t R, int64_t B, int64_t Nmax,
                        int32_t *P, int32_t *count, int32_t *steps, void *stream);
int sn_mesh_digits_u8(const uint8_t *images, int64_t B, int32_t rows, int32_t cols, uint64_t seed, int64_t image_base, int64_t R,
                      int32_t min_points, int64_t min_det, int32_t max_attempts, int32_t max_rounds, int64_t Nmax, int32_t *P,
                      int32_t *count, float *V, int32_t *F, int32_t *nF, int32_t *status, int32_t *attempts, int32_t *counts,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh descriptors: per-vertex normals, mass, Gaussian and mean curvature, and the libigl-convention Laplacian M^-1 C.
 *
 * Replaces: compute_normals, area, laplacian_and_mass, compute_laplacian, gaussian_curvature, hacky_compute_laplacian
 *           src/utils/geom_utils.py (all through pyigl), feeding src/normal_predict/sampler.py:21-91.
 * These are this project's own definitions in libigl's conventions, not its bits.  Host statement: mesh_ops.vertex_descriptors,
 * mesh_ops.libigl_laplacian.
 *
 * Arithmetic.  P = the fp32 coordinates widened to fp64.  Every product and sum is rounded on its own (no fused multiply-add);
 *   a three-term sum is (x + y) + z;  u x w = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x);  u.w = (u_x w_x +
 *   u_y w_y) + u_z w_z.  A sum "over the faces of a vertex" runs over its incident faces that are neither bad nor flat, in
 *   ascending face index, from +0.0.  Outputs are rounded to fp32 at the end.
 * Face f = (i, j, k).  BAD: an index outside 0..nV-1 or two equal indices; contributes nothing, SN_DESC_BAD_FACE, face outputs 0.
 *   n_f = (P_j - P_i) x (P_k - P_i), dbl_f = sqrt(n_f.n_f), a_f = dbl_f / 2.  FLAT: !(dbl_f > 0) (zero or NaN); contributes
 *   nothing to any vertex sum nor to the Laplacian's pattern, SN_DESC_FLAT_FACE, face outputs a_f = 0, nhat_f = 0.  Otherwise
 *   nhat_f = n_f / dbl_f componentwise.  All three corners use the same n_f, dbl_f (from the first vertex).
 * Corner (v; a, b), a and b the other two vertices in face order (the corner table of sn_mesh_corners_f32):
 *   u = P_a - P_v, w = P_b - P_v, d_v = u.w, theta_v = atan2(dbl_f, d_v), cot_v = d_v / dbl_f.
 *   The face is OBTUSE when d_i < 0 or d_j < 0 or d_k < 0.
 * Vertex v:
 *   N_area = sum n_f;  N_uniform = sum nhat_f;  N_angle = sum theta_v nhat_f (the scalar times each component).  Each is then
 *     divided componentwise by sqrt(N.N); a length that is not > 0 gives (0, 0, 0) and SN_DESC_NO_NORMAL (an isolated vertex;
 *     raised for the normals that were asked for).
 *   M_bary = sum a_f / 3.
 *   M_voronoi = sum of one term per corner (Meyer's mixed cells, libigl's MASSMATRIX_TYPE_VORONOI): obtuse face and d_v < 0:
 *     a_f / 2;  obtuse face otherwise: a_f / 4;  else ((u.u) cot_b + (w.w) cot_a) / 8.
 *   K = 2 pi - sum theta_v, the raw angle defect (at boundary vertices too, as igl.gaussian_curvature), 2 pi the fp64 constant.
 *   dP = sum ((0.5 cot_b) u + (0.5 cot_a) w), componentwise: the cotangent Laplacian applied to the positions (the edge v-a lies
 *     opposite b).
 *   H = s sqrt(dP.dP) / (2 M_voronoi), s = -1 when dP.N_area > 0 (N_area before its division) and +1 otherwise; H = 0 when
 *     M_voronoi is not > 0.  A sphere of radius r with outward faces has H = +1/r.
 * Only + - * / sqrt and one atan2 per corner: everything but K and N_angle equals the host statement bit for bit.
 *
 * sn_mesh_descriptors_f32 : face_area[nF], face_normal[nF][3], n_area / n_uniform / n_angle [nV][3], mass_bary / mass_voronoi /
 *     gauss (K) / mean (H) [nV].  Any output pointer may be NULL and is then not computed.  *status is cleared, then OR-ed.
 *     No limit on the number of faces at a vertex: one thread per vertex streams over its incidence list (codes 3 f + c of the
 *     good faces, counted, scanned, filled with an atomic cursor and sorted, so the order of the sums is fixed: two runs are
 *     bit-identical).  workspace: sn_mesh_descriptors_workspace_bytes(nV, nF), else SN_E_WORKSPACE.  Negative nV or nF:
 *     SN_E_SHAPE.  nV + 1 or 3 nF past int32: SN_E_RANGE.  Does not synchronise.
 *
 * sn_mesh_cot_laplacian_f32 : L = M^-1 C in CSR, libigl's igl.cotmatrix scaled by the inverse mass matrix.
 *     C_vj = the sum of 0.5 cot at the corner opposite the edge v-j, over the faces of v that contain j, ascending face order.
 *     Stored entry (v, j) = C_vj / M_v; diagonal = (0 - sum_j C_vj) / M_v, j ascending; M = M_bary (SN_DESC_MASS_BARYCENTRIC) or
 *     M_voronoi (SN_DESC_MASS_VORONOI) in fp64, before any rounding.  Pattern: every distinct neighbour plus the diagonal, columns
 *     ascending; an exactly zero C_vj is KEPT (sn_laplacian_csr_from_mesh drops it).  A vertex without mass has a NaN diagonal.
 *     clamp != 0: an entry whose fp32 value is not finite or exceeds 1e10 in magnitude becomes (float) hack and SN_DESC_CLAMPED
 *     is set (geom_utils.py:209-211).  -2 L(barycentric) is sn_laplacian_csr_from_mesh's A^-1 (D - W) without its two epsilons.
 *     Two phases as sn_laplacian_csr_from_mesh (phase 0: rowptr and *status, cleared first; the caller reads rowptr[nV] and the
 *     status, allocates, calls phase 1 with the same workspace, which ORs SN_DESC_CLAMPED into *status).  A vertex with more
 *     than SN_LAP_MAX_DEGREE incident good faces sets SN_DESC_DEGREE in phase 0: the caller launches nothing further.
 *
 * sn_mesh_cot_pencil_f64 : the same sums left in fp64 and undivided, the pencil (S, M) of the "Spectral" section below.
 *     rowptr / colind: the pattern of sn_mesh_cot_laplacian_f32 (every neighbour plus the diagonal, columns ascending, exact
 *     zeros kept).  S[nnz] fp64: S_vj = 0 - C_vj off the diagonal, S_vv = sum_j C_vj over ascending j from +0.0.  mass[nV]: fp64
 *     M_voronoi, unrounded.  C_vj and C_jv sum the same corners (the two that lie opposite the edge v-j) in the same ascending
 *     face order, so S equals its transpose BIT FOR BIT.  The same two phases, the same workspace (its size is
 *     sn_mesh_cot_laplacian_workspace_bytes(nV, nF), else SN_E_WORKSPACE) and the same status bits (phase 1 writes colind, S and
 *     mass and adds no bit).  Host statement: mesh_ops.cot_pencil.
 * ------------------------------------------------------------------------------------------ */
#define SN_DESC_BAD_FACE   1
#define SN_DESC_FLAT_FACE  2
#define SN_DESC_NO_NORMAL  4
#define SN_DESC_CLAMPED    8
#define SN_DESC_DEGREE     16
#define SN_DESC_MASS_BARYCENTRIC 0
#define SN_DESC_MASS_VORONOI     1
size_t sn_mesh_descriptors_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_descriptors_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, float *face_area, float *face_normal,
                            float *n_area, float *n_uniform, float *n_angle, float *mass_bary, float *mass_voronoi,
                            float *gauss, float *mean, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t sn_mesh_cot_laplacian_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_cot_laplacian_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase, int32_t mass, int32_t clamp,
                              double hack, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status, void *workspace,
                              size_t workspace_bytes, void *stream);
int sn_mesh_cot_pencil_f64(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase, int32_t *rowptr, int32_t *colind,
                           double *S, double *mass, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Principal curvatures: k1 >= k2 and their directions from a quadric fitted over the k-ring patch of every vertex.
 *
 * Replaces: igl.principal_curvature in compute_curv4 src/utils/geom_utils.py:390-405 (an un-vendored pyigl fork, on the host, one
 *           mesh at a time), the 'curv4': 4 input of src/normal_predict/train_4_normal.py:126.
 * This is this project's own definition in libigl's conventions (igl::principal_curvature with its defaults: k-ring patch,
 * projection-plane check, averaged normal, quadric z = a x^2 + b x y + c y^2 + d x + e y), not its bits: no igl was at hand to
 * compare with, so nothing here claims agreement with it beyond the conventions.  Host statement: mesh_ops.principal_curvatures.
 *
 * Arithmetic.  As "Mesh descriptors": P = the fp32 coordinates widened to fp64, every product and sum rounded on its own, (x + y) + z,
 *   u.w = (u_x w_x + u_y w_y) + u_z w_z, u x w as there, sums from +0.0; outputs rounded to fp32 at the end.  Only + - * / sqrt and
 *   comparisons occur, so the device equals the host statement bit for bit.  A vertex takes the first failure it meets in the
 *   order of this text, gets that one bit, and stops.
 * Vertex normals.  n_x = N_area / sqrt(N_area.N_area) of "Mesh descriptors" in fp64, before its rounding; (0, 0, 0) where that
 *   length is not > 0.  Computed once per vertex into the workspace.
 * Ring.  Two vertices are neighbours when a face that is not BAD holds both (a FLAT face still connects).  S_0 = {v}, S_(i+1) = S_i
 *   and the neighbours of its members, S = S_radius, radius >= 1.  More than SN_CURV_MAX_RING members: SN_CURV_OVERFLOW, and
 *   ring_size = SN_CURV_MAX_RING + 1.
 * Projection-plane check.  n_v = (0, 0, 0): SN_CURV_NO_NORMAL (an isolated vertex, or one with flat faces only).
 *   S' = {x in S : n_x.n_v > 0}; if SN_CURV_MIN_POINTS <= |S'| < |S| then S = S'.  ring_size = |S|.  |S| < SN_CURV_MIN_POINTS:
 *   SN_CURV_FEW_POINTS.
 * Order.  S is a set.  Every sum below runs over its members in ascending vertex id; the order in which the search found them
 *   reaches no arithmetic.
 * Fit normal.  m = sum n_x, then divided componentwise by l = sqrt(m.m).  l not > 0: SN_CURV_DEGENERATE (all four causes share
 *   the bit; they are tested in this order: l, the frame, h, the pivots).
 * Frame.  For a neighbour a of v (a member of S_1 other than v, whether or not the check kept it): c = P_a - P_v,
 *   t = c - (c.m) m componentwise (c_x - (c.m) m_x).  The a of smallest id with sqrt(t.t) > 0 is taken: e1 = t / sqrt(t.t),
 *   e2 = m x e1.  None: SN_CURV_DEGENERATE.
 * Local coordinates.  c = P_x - P_v for x in S (v included, a zero row).  h = sqrt(the largest c.c), found by `if (c.c > best)`
 *   from 0.  h not > 0: SN_CURV_DEGENERATE.  xi = (c.e1) / h, eta = (c.e2) / h, zeta = (c.m) / h.
 * Normal equations.  r = (xi xi, xi eta, eta eta, xi, eta).  G_ab = sum r_a r_b (a <= b, 15 sums, mirrored), g_a = sum zeta r_a.
 *   Cholesky G = L L^T without pivoting, column j = 0..4: d = G_jj, then d = d - L_jk L_jk for k = 0..j-1; a pivot that is not
 *   d > SN_CURV_PIVOT_FLOOR G_jj: SN_CURV_DEGENERATE; L_jj = sqrt(d); for i = j+1..4: x = G_ij, x = x - L_ik L_jk for k = 0..j-1,
 *   L_ij = x / L_jj.  Forward: y_i = (g_i minus L_ik y_k, k = 0..i-1, one after the other) / L_ii, i = 0..4.  Backward:
 *   q_i = (y_i minus L_ki q_k, k = i+1..4, one after the other) / L_ii, i = 4..0.  (a, b, c, d, e) = (q_0 / h, q_1 / h, q_2 / h,
 *   q_3, q_4).  (On well-shaped patches the smallest L_jj is 0.4-1.2 with this scaling: the floor does not touch them.)
 * Fundamental forms.  E = 1 + d d, F = d e, G = 1 + e e, w = sqrt((1 + d d) + e e), L = (2 a) / w, M = b / w, N = (2 c) / w,
 *   den = E G - F F, s11 = (L G - M F) / den, s12 = (M E - L F) / den, s22 = (N E - M F) / den: the symmetric matrix libigl forms.
 * Eigenvalues.  tr2 = (s11 + s22) / 2, df = s11 - s22, disc = df df + 4 (s12 s12), rt = sqrt(disc) / 2.  The curvatures are the
 *   negated eigenvalues: k1 = rt - tr2, k2 = (0 - tr2) - rt, so k1 >= k2 and a plane has k1 = k2 = +0.0.  A sphere of radius r with
 *   outward faces has k1 = k2 = +1/r, the sign of H in "Mesh descriptors".
 * Directions.  For d1: lambda = tr2 - rt; for d2: lambda = tr2 + rt.  If |s11 - lambda| >= |s22 - lambda| then (u1, u2) =
 *   (s12, lambda - s11), else (lambda - s22, s12) — orthogonal to the row of S - lambda I with the larger diagonal entry.  If u1 < 0,
 *   or u1 = 0 and u2 < 0, both are negated.  D = u1 e1 + u2 e2 componentwise, divided by sqrt(D.D).  Where disc is not > 0 (an
 *   umbilic) or that length is not > 0: d1 = e1, d2 = e2.  Both lie in the plane perpendicular to m, the averaged normal, which is
 *   not n_v.
 * Failures.  A vertex that fails gets NaN (0x7FC00000) in every output that was asked for, ring_size as stated, and its bit OR-ed
 *   into *status; its neighbours are unaffected.  A BAD face sets SN_DESC_BAD_FACE; FLAT faces raise nothing here.
 *
 * sn_mesh_principal_curvature_f32 : k1, k2 [nV] fp32, d1, d2 [nV][3] fp32, ring_size [nV] int32; any of them may be NULL and is
 *     then not written.  *status is cleared, then OR-ed.  One wavefront per vertex: the patch is a list of ids in LDS beside an
 *     open-addressing table, grown level by level, filtered, sorted (bitonic), and only then summed, serially.  Batches are one
 *     disjoint mesh with offset faces.  workspace: sn_mesh_curvature_workspace_bytes(nV, nF), else SN_E_WORKSPACE.  Negative nV
 *     or nF, radius < 1: SN_E_SHAPE.  nV + 1 or 3 nF past int32: SN_E_RANGE.  Does not synchronise; two runs are bit-identical.
 * ------------------------------------------------------------------------------------------ */
#define SN_CURV_FEW_POINTS   32
#define SN_CURV_NO_NORMAL    64
#define SN_CURV_OVERFLOW     128
#define SN_CURV_DEGENERATE   1024
#define SN_CURV_MAX_RING     1024
#define SN_CURV_MIN_POINTS   6
#define SN_CURV_PIVOT_FLOOR  1e-12
size_t sn_mesh_curvature_workspace_bytes(int64_t nV, int64_t nF);
int sn_mesh_principal_curvature_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t radius, float *k1, float *k2,
                                    float *d1, float *d2, int32_t *ring_size, int32_t *status, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Spectral: the lowest eigenpairs of the cotangent pencil and the wave kernel signature, on the device.
 *
 * Replaces: compute_wks src/utils/geom_utils.py:407-440 (scipy.sparse.linalg.eigsh(-L, M=Am, sigma=-1e-5, k=300), a shift-invert
 *           Lanczos with a sparse LU on the host, then the WKS sums), the 'wks': 100 input of src/normal_predict/train_4_normal.py:126.
 * Host statement: mesh_ops.cot_pencil, spectral_start, cheb_filter_step, laplacian_eigenpairs, wks_weights, wks_contract,
 *           wave_kernel_signature.  The three kernels below equal their numpy statements bit for bit (fp64, no contraction, only
 *           + - * / and conversions); the solver as a whole (operators.laplacian_eigenpairs) takes the statement's steps with
 *           the statement's parameters and differs from it in the rounding order of the library QR, eigh and dense products.
 *
 * Problem.  S phi = lambda diag(Am) phi for the k lowest lambda of every mesh of a block-diagonal batch; voff[B + 1] (int32,
 *   ascending, voff[0] = 0, voff[B] = n) holds the first row of every mesh.
 *   1. Mass: Am = max(M_voronoi, 1e-8), then Am /= sum(Am) per mesh (compute_wks:415-416).  A clipped vertex: SN_EIG_CLIPPED_MASS.
 *   2. Standard form: A = D S D, D = Am^-1/2, A_ij = (D_i S_ij) D_j: S's pattern, symmetric.
 *   3. Upper bound: b = max_i sum_j |A_ij| per mesh (Gershgorin); S is positive semidefinite, so the spectrum lies in [0, b].
 *   4. Start block: m = min(n_b, k + guard) columns (the smallest mesh decides for the batch), sn_spectral_start_f64, orthonormalised (QR).
 *   5. Outer iteration, at most max_outer times: Rayleigh-Ritz (H = X^T A X, symmetrised, eigh, X and A X rotated), residuals
 *      r_i = |A x_i - theta_i x_i|_2, converged when r_i <= tol b for all i < k; else a Chebyshev filter of degree deg on [a, b],
 *      a = theta_{m-1}, scaled at a0 = theta_0 (Zhou & Saad): e = (b - a) / 2, c = (b + a) / 2, sigma_1 = e / (a0 - c),
 *      Y_1 = (sigma_1 / e) (A X - c X), sigma_{j+1} = 1 / (2 / sigma_1 - sigma_j),
 *      Y_{j+1} = (2 sigma_{j+1} / e) (A Y_j - c Y_j) - sigma_j sigma_{j+1} Y_{j-1}: deg calls of sn_cheb_filter_step_f64 with
 *      per-mesh scalars, then QR again.  A mesh that has converged is left alone (alpha = 0, beta = -1 hands X through).
 *   6. Result: values theta_i and vectors phi = D x (phi^T diag(Am) phi = I).  Not converged: SN_EIG_NOT_CONVERGED.
 *   The SN_EIG_* bits share the status word with the pencil's SN_DESC_* bits.
 *
 * sn_spectral_start_f64 : X[i, c] = (double)(h >> 11) * 2^-53 - 0.5, h = mix64(mix64(seed + G + r) + G + c) modulo 2^64, r the
 *     row's number inside its mesh, G = 0x9E3779B97F4A7C15, mix64 the splitmix64 finaliser of the Mesh-MNIST maker: a fixed
 *     function of (seed, row in mesh, column), so a mesh starts from the same block alone and in a batch.  X: (n, m) row-major.
 *
 * sn_cheb_filter_step_f64 : Z[i, c] = (alpha_b * ((sum_j A_ij Y[j, c]) - shift_b * Y[i, c])) - beta_b * X[i, c] for every row i
 *     and column c < m, b the mesh of row i.  A: fp64 CSR (rowptr[n + 1], colind, vals; int32); X, Y, Z: (n, m) row-major fp64,
 *     m >= 1 of any value (no alignment or width is assumed); alpha, beta, shift: [B] fp64 in DEVICE memory, so the steps of a
 *     filter need no host synchronisation.  The row sum is serial over the stored entries in ascending position from +0.0, every
 *     product and sum rounded on its own.  A X = the step with alpha = 1, beta = 0, shift = 0.  Z may BE X (every element of X
 *     is read only by the thread that writes it); Z must not overlap Y, nor X in part: SN_E_SHAPE.  Lanes run over columns (a
 *     gather of Y[j, :] is contiguous); one wave takes up to 256 columns of one row, or 64 / W rows when m <= W < 64.
 *     A stored column outside 0..n-1 is passed over.  Does not synchronise; two runs are bit-identical.
 *
 * sn_wks_f64 : out[v, i] = (sum_k phi[v, k]^2 W[b, k, i]) / C[b, i], b the mesh of vertex v: phi (nV, k), W (B, k, N), C (B, N)
 *     fp64 row-major; the square is formed on load, the sum is serial over ascending k from +0.0, the division is in the store.
 *     out: (nV, N) fp64, or fp32 (out_f32 != 0: the quotient rounded once).  W and C are compute_wks:423-438 on the values:
 *     E = sorted |values|, logE = log(max(E, 1e-6)), ee = linspace(logE[1], max(logE) / 1.02, N), sigma = 6 (ee[1] - ee[0]),
 *     W_ki = exp(-(ee_i - logE_k)^2 / (2 sigma^2)), C_i = sum_k W_ki — a few kilobytes, made by the caller.
 *
 * All three: B < 1, m < 1, k < 1, N < 1 or a negative size: SN_E_SHAPE.  n or B past int32: SN_E_RANGE.
 * ------------------------------------------------------------------------------------------ */
#define SN_EIG_NOT_CONVERGED 256
#define SN_EIG_CLIPPED_MASS  512
int sn_spectral_start_f64(uint64_t seed, const int32_t *voff, int64_t B, int64_t n, int64_t m, double *X, void *stream);
int sn_cheb_filter_step_f64(const int32_t *rowptr, const int32_t *colind, const double *vals, const int32_t *voff, int64_t B, int64_t n,
                            int64_t m, const double *alpha, const double *beta, const double *shift, const double *X, const double *Y,
                            double *Z, void *stream);
int sn_wks_f64(const double *phi, const int32_t *voff, int64_t B, int64_t nV, int64_t k, int64_t N, const double *W, const double *Cn,
               int32_t out_f32, void *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * ARAP deformation: as-rigid-as-possible sequences from a rest mesh and moving handles, on the device.
 *
 * Replaces: nothing in the reference's tree — its data_plus/ sequences were made off-line with libigl and downloaded, and neither the
 *           generator nor its parameters are there.  This is the textbook spokes-only algorithm (Sorkine & Alexa 2007), alternating
 *           local and global steps, with this project's weights: NOT a reproduction of those files.
 * Host statement: mesh_ops.arap_weights, arap_rotations, arap_rhs, arap_cg, arap_deform (numpy); the device equals it bit for bit.
 * Everything is fp64 without contraction; only + - * / sqrt and comparisons are used, so numpy reproduces every rounding.
 *
 * Input.  Rest mesh V0 fp32 (nV, 3), widened to fp64 (P0); F int32 (nF, 3); handles int32 (nH): distinct, in range, at least one per
 *   mesh; H fp32 (T, nH, 3), the handle positions of every frame; iters >= 1, tol, max_cg <= SN_ARAP_MAX_CG.  A batch is a disjoint
 *   union: V0, F, handles index the union, voff[B + 1] and hoff[B + 1] (int32, ascending) cut vertices and handles into meshes, and
 *   every entry of a row stays inside its mesh.  One mesh has at most sn_arap_max_vertices() vertices (its search direction lives in
 *   the LDS of one compute unit).
 * Weights.  w_ij = W[i, j] of the cotangent weights of the Laplacian section above on the rest mesh (Heron area with the 1e-6 floor,
 *   denominator 8a + 1e-6): lengths l = sqrt((dx*dx + dy*dy) + dz*dz) in the face's own order (|v0 v1|, |v1 v2|, |v2 v0|),
 *   h = ((l0 + l1) + l2) / 2, a = sqrt(((h (h-l0)) (h-l1)) (h-l2)) or 1e-6 when the radicand is <= 0; for the ordered corner triple
 *   (p, q, r) the contribution to W[F[p], F[q]] is ((-l_pq^2 + l_qr^2) + l_rp^2) / (8a + 1e-6).  The pattern is the vertex adjacency
 *   (no diagonal); a value is kept whatever it is, negative and zero included; columns ascend.  An entry is the serial sum, from its
 *   first contribution on, over its contributions sorted by (face, permutation) — the rule of sn_mesh_idt_laplacian_f32.  W[i, j] and
 *   W[j, i] differ in their last bits (the three squares are added in another order); row i uses W[i, .].  d_i = the serial sum of
 *   w_ij from +0.0 in ascending column order.  A face with an index outside 0..nV-1 or a repeated index contributes nothing
 *   (SN_ARAP_BAD_FACE); a vertex with more than SN_LAP_MAX_DEGREE incident good faces gets an empty row (SN_ARAP_DEGREE).
 * Frame t = 0 .. T-1.  The rows of handles are set to H[t]; the free rows start from frame t-1's result, from P0 for t = 0.  Then
 *   iters times a local and a global step.
 * Local step.  S_i = sum over ascending j of w_ij e_ij e'_ij^T, e_ij = P0_i - P0_j, e'_ij = x_i - x_j, accumulated from +0.0 as
 *   S[a][b] = S[a][b] + (w e[a]) e'[b].  R_i = the proper rotation maximising tr(R S_i):
 *     G = S^T S, G[a][b] = (S[0][a] S[0][b] + S[1][a] S[1][b]) + S[2][a] S[2][b];  V = I;  SN_ARAP_JACOBI_SWEEPS sweeps over the pairs
 *     (p, q) = (0,1), (0,2), (1,2), r the third index; a pair with G_pq == 0 is skipped, else theta = (G_qq - G_pp) / (2 G_pq),
 *     t = 1 / (|theta| + sqrt(theta theta + 1)) negated when theta < 0, c = 1 / sqrt(t t + 1), s = t c;  G_pp -= t G_pq,
 *     G_qq += t G_pq, (G_rp, G_rq) = (c G_rp - s G_rq, s G_rp + c G_rq), G_pq = 0, and every row k of V:
 *     (V_kp, V_kq) = (c V_kp - s V_kq, s V_kp + c V_kq), all from the old values.  The diagonal and the columns of V are sorted by
 *     the exchanges (0,1), (1,2), (0,1), each done when lambda_a < lambda_b.  v1, v2 = the first two columns, v3 = v1 x v2;
 *     a1 = S v1, a2 = S v2 with (S v)[r] = (S[r][0] v[0] + S[r][1] v[1]) + S[r][2] v[2];  n1 = a1.a1, u1 = a1 / sqrt(n1);
 *     a2' = a2 - (u1.a2) u1, n2 = a2'.a2', u2 = a2' / sqrt(n2), u3 = u1 x u2;  R[a][b] = (v1[a] u1[b] + v2[a] u2[b]) + v3[a] u3[b].
 *     Dot products are (x x + y y) + z z, cross products (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x).  The third
 *     singular value is never divided by: a flat cloth (rank 2) is exact, a reflection turns the weakest direction.  Unless n1 > 0
 *     and n2 > SN_ARAP_RANK_EPS n1 (rank below 2): R_i = I and SN_ARAP_DEGENERATE.
 * Global step.  b_i = sum over ascending j of ((w_ij 0.5) ((R_i + R_j) e_ij)) from +0.0, the matrix-vector product as above.
 *   Solve  d_i x_i - sum_j w_ij x_j = b_i  on the free rows, the handle rows held:  rhs_i = b_i plus, over the handle columns in
 *   ascending order, w_ij x_j;  (A y)_i = d_i y_i - (sum over the FREE columns, ascending, from +0.0, of w_ij y_j).
 *   Jacobi-preconditioned CG, the three coordinate columns sharing the matrix product, each with its own alpha and beta:
 *     r = rhs - A x, z = r / d, p = z;  rz = <r z>, rr = <r r>, bb = <rhs rhs>;  a column is CONVERGED when sqrt(rr) <= tol sqrt(bb),
 *     tested here and after every update, and stays so: it is FROZEN (x, r, p of that column are not touched again — an all-zero
 *     column, a flat cloth moving in its plane, never divides 0 by 0).
 *     Iteration, at most max_cg of them, none when every column is converged:  pAp = <p A p>;  a column that is not converged and
 *     has not pAp > 0 ends the solve with SN_ARAP_BREAKDOWN;  alpha = rz / pAp;  x = x + alpha p, r = r - alpha (A p);  z = r / d;
 *     rz' = <r z>, rr = <r r>;  convergence test;  beta = rz' / rz;  p = z + beta p and rz = rz' on the columns still running.
 *     max_cg iterations done and a column left: SN_ARAP_NOT_CONVERGED.
 *   <u v>, per column, over the free rows i (local index in the mesh): lane i mod SN_ARAP_THREADS adds its rows serially in ascending
 *     order from +0.0;  then a halving tree inside every group of 64 consecutive lanes (lane l += lane l + s, s = 32 .. 1);  then a
 *     halving tree over the 16 group sums (s = 8 .. 1).
 *   A free row without d_i > 0 sets SN_ARAP_BREAKDOWN for the mesh: no step runs in any frame and every R is I.  After a breakdown
 *     inside a solve the free rows go back to the values they had when the frame began and the frame's remaining steps are skipped
 *     (their counts are 0).  This is what a component without a handle or a broken mesh ends in, if it does not simply fail to converge.
 * Output per frame: the positions rounded once to fp32;  the CG iteration count of every global step;  the energy
 *   sum_i sum_j w_ij |e'_ij - R_i e_ij|^2 after the last step, with the R of the last local step: per row serially over ascending j
 *   from +0.0, each term w ((dx dx + dy dy) + dz dz), rows by the reduction above over ALL rows of the mesh.
 *
 * sn_arap_weights_f64 : rowptr[nV + 1], colind, w (sized for 6 nF entries by the caller, rowptr[nV] used), d[nV], *status (cleared
 *                       first).  The by-vertex buckets are those of the other mesh builders (bucket_count_k / bucket_fill_k /
 *                       sn_internal_scan_i32).  workspace: sn_arap_weights_workspace_bytes(nV, nF).  Does not synchronise.
 * sn_arap_frames_f64  : frames frame_begin .. frame_begin + frame_count - 1 of T, one workgroup of SN_ARAP_THREADS threads per mesh,
 *                       the local step, the right-hand side and the whole CG of a frame inside it; no workgroup waits for another,
 *                       every loop is bounded by an argument, and every exit from the CG loop is decided from values all threads
 *                       read after a barrier.  p (3 fp64 per vertex) is in LDS; x, r, A p, R and the frame's start values are in
 *                       the workspace, each row read and written by its owner thread alone except x and R, which neighbours read
 *                       after a barrier.  max_mesh_vertices: an upper bound of the meshes' sizes, > sn_arap_max_vertices() is
 *                       SN_E_UNSUPPORTED; a mesh larger than the bound is skipped (frames = V0, SN_ARAP_TOO_LARGE).  The state
 *                       between calls is the workspace (sn_arap_frames_workspace_bytes(nV)): a caller enqueues frames in chunks
 *                       with the same workspace, frame_begin == 0 initialises it and clears status.  frames (T, nV, 3) fp32,
 *                       cg_iters (B, T, iters) int32, energy (B, T) fp64, status (B) int32.  R_first (nV, 9) and rhs_first (nV, 3)
 *                       fp64 (both or neither): R and b of the first local step of frame 0, written by the call that holds it.
 * ------------------------------------------------------------------------------------------ */
#define SN_ARAP_NOT_CONVERGED  1
#define SN_ARAP_BREAKDOWN      2
#define SN_ARAP_DEGENERATE     4
#define SN_ARAP_BAD_FACE       8
#define SN_ARAP_DEGREE         16
#define SN_ARAP_TOO_LARGE      32
#define SN_ARAP_THREADS        1024
#define SN_ARAP_JACOBI_SWEEPS  6
#define SN_ARAP_RANK_EPS       1e-20
#define SN_ARAP_MAX_CG         65536
int64_t sn_arap_max_vertices(void);
size_t sn_arap_weights_workspace_bytes(int64_t nV, int64_t nF);
int sn_arap_weights_f64(const float *V0, const int32_t *F, int64_t nV, int64_t nF, int32_t *rowptr, int32_t *colind, double *w,
                        double *d, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t sn_arap_frames_workspace_bytes(int64_t nV);
int sn_arap_frames_f64(const float *V0, const int32_t *rowptr, const int32_t *colind, const double *w, const double *d,
                       const int32_t *voff, const int32_t *hoff, const int32_t *handles, const float *H, int64_t B, int64_t nV,
                       int64_t nH, int64_t T, int64_t max_mesh_vertices, int32_t frame_begin, int32_t frame_count, int32_t iters,
                       double tol, int32_t max_cg, float *frames, int32_t *cg_iters, double *energy, int32_t *status,
                       double *R_first, double *rhs_first, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sparse x sparse CSR products and the symmetric diagonal scaling: the operators of the 'amp' tower.
 *
 * Replaces: L = Dsq.dot(L).dot(Dsq); twice L = Dsq.dot(L).dot(Dsq), L = L.dot(L)     src/dense_correspondence/main.py:72-83
 *           scipy's csr_matmat behind every one of those dots (the diagonal ones included).
 *
 * Definition of the product C = A B.  A is M x K, B is K x N, int32 CSR with fp32 values, columns strictly ascending inside a
 *   row, explicit zeros allowed.  The structural pattern of row i is the union of the rows j of B over the stored (i, j) of A.
 *   c_ik = fl(...fl(fl(0 + fl(a_ij1 b_j1k)) + fl(a_ij2 b_j2k))...),  j1 < j2 < ... the entries of A's row i in ascending column
 *   order, only those j with (j, k) stored in B taking part.  Every product and every sum is rounded on its own (no fused
 *   multiply-add, no fast-math), no floating-point atomics: two runs give identical bits.  Output columns ascend.  An entry whose
 *   sum is exactly zero is dropped, as scipy drops it; the structural arrays (every entry kept) are a result of their own.
 *   On an A with ascending columns this is scipy's csr_matmat value bit for bit; scipy's OUTPUT rows are unsorted, so a product
 *   that takes an unsorted scipy result as its left operand sums in another order (LABNOTES.md#spgemm has the bound).
 *
 * sn_csr_spgemm_f32, three phases on one workspace (sn_csr_spgemm_workspace_bytes(M)); the caller owns every allocation:
 *   phase 0 (structural count)  clears *status, writes s_rowptr[M + 1]; the caller reads s_rowptr[M] and allocates s_colind, s_vals.
 *   phase 1 (fill + count)      writes s_colind, s_vals (the structural result) and rowptr[M + 1] of the entries != 0; the caller
 *                               reads rowptr[M]: equal to s_rowptr[M], the structural arrays are the result, else it allocates.
 *   phase 2 (compaction)        colind, vals: the entries != 0 in order.
 *   One workgroup per result row: the candidate columns are marked as bits of an LDS bitmap over the row's column window
 *   (atomicOr on bits is order-independent), a popcount prefix numbers them in ascending order, each thread then owns result
 *   entries, walks A's row in order and finds k in B's row j by binary search.
 *   *status bits: SN_SPGEMM_BAD_COLUMN  a column of A outside 0..K-1 or of B outside 0..N-1: it contributes nothing, nothing is
 *                                       read out of bounds;
 *                 SN_SPGEMM_TOO_WIDE    a result row whose candidates span more than sn_csr_spgemm_max_window() =
 *                                       SN_SPGEMM_MAX_WINDOW columns (last - first + 1; the bitmap is 16 KiB of LDS);
 *                 SN_SPGEMM_TOO_LARGE   the structural entries do not fit the int32 row pointers.
 *   With one of the last two set the call is unsupported and NOTHING is written (s_rowptr included; later phases return at
 *   once).  There is no host fallback.  No limit on the length of a row of A, B or C.
 *
 * sn_csr_inv_sqrt_degree_f32 : d[i] = (float)(1.0 / sqrt((double)(rowptr[i+1] - rowptr[i] - 1))), fp64 as numpy computes it.
 *                              Clears *status; a row with fewer than two entries sets SN_CSR_NO_OFFDIAGONAL (the host divides
 *                              by zero there; d[i] is then inf or nan).
 * sn_csr_scale_sym_f32       : out_ij = fl(fl(d_i a_ij) d_j) of a square M x M matrix, what the two diagonal products of the
 *                              reference give.  phase 0 clears *status, writes s_vals (on A's pattern) and rowptr[M + 1] of the
 *                              results != 0; phase 1 compacts (a_rowptr, a_colind, s_vals) into (rowptr, colind, vals) — not
 *                              needed when rowptr[M] == a_rowptr[M].  A column outside 0..M-1 gives 0 and sets
 *                              SN_SPGEMM_BAD_COLUMN.  workspace: sn_csr_spgemm_workspace_bytes(M).
 * ------------------------------------------------------------------------------------------ */
#define SN_SPGEMM_MAX_WINDOW   131072
#define SN_SPGEMM_BAD_COLUMN   1
#define SN_SPGEMM_TOO_WIDE     2
#define SN_SPGEMM_TOO_LARGE    4
#define SN_CSR_NO_OFFDIAGONAL  8
int64_t sn_csr_spgemm_max_window(void);
size_t sn_csr_spgemm_workspace_bytes(int64_t M);
int sn_csr_spgemm_f32(const int32_t *a_rowptr, const int32_t *a_colind, const float *a_vals, const int32_t *b_rowptr,
                      const int32_t *b_colind, const float *b_vals, int64_t M, int64_t K, int64_t N, int32_t phase,
                      int32_t *s_rowptr, int32_t *s_colind, float *s_vals, int32_t *rowptr, int32_t *colind, float *vals,
                      int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int sn_csr_inv_sqrt_degree_f32(const int32_t *rowptr, int64_t M, float *d, int32_t *status, void *stream);
int sn_csr_scale_sym_f32(const int32_t *a_rowptr, const int32_t *a_colind, const float *a_vals, const float *d, int64_t M,
                         int32_t phase, float *s_vals, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Row-streaming fp32 GEMMs of the per-node Linear layers with the weights held in registers
 * (v_mfma_f32_32x32x2_f32; the operands are tall-skinny: rows ~ 1e5..1e6, K and N in {128, 256}).
 *
 * sn_linear_fwd_f32 : y[r, j] = sum_k x[r,k] * W[j,k] + bias[j] (+ residual[r,j]);  optionally also
 *                     y_elu[r, j] = elu(y[r, j]) written to a second destination (e.g. the concat buffer of the next
 *                     stage).  W is (J x K) row-major — the BN-folded weight W·diag(s) of sn_bn_fold_f32.
 *                     Replaces nn.Linear (src/utils/utils_pt.py:89,99) + the residual add (utils_pt.py:180,220) + the
 *                     F.elu that follows (utils_pt.py:171,208).
 * sn_linear_dgrad_f32 : dx[r, c] = sum_j dy[r,j] * W[j,c]  (+ (x[r,c] - center[c]) * B[c] + Cc[c]  when B != NULL):
 *                     input gradient of the folded BatchNorm+Linear with the BatchNorm tail fused in the epilogue
 *                     (replaces the dgrad GEMM + sn_affine_cols_acc_f32).  W is (J x C) row-major.
 * sn_linear_dgrad_elu_f32 : the same input gradient when x is the concat buffer [elu(u) | P·elu(u)] of a residual stage
 *                     (C = 2·C/2 columns): the first C/2 columns continue through the activation in the epilogue,
 *                         gact[r, c] = dx[r, c] * elu'(x[r, c]) + gadd[r, c]      (c < C/2; gadd may be NULL),
 *                     and only the last C/2 columns are written, to dx_hi (rows x C/2) — the operand of the transposed
 *                     sparse product.  B (the BatchNorm tail) is required.  Split-bf16 kernels only
 *                     (SN_E_UNSUPPORTED with SN_GEMM_VARIANT=0: the caller composes the unfused calls).
 * sn_linear_fwd_segbias_f32 : the forward with a PER-MESH bias, y[r, :] = x[r]·W^T + segbias[r / rows_per_seg, :]
 *                     (+ residual) — the half-width global-average stage; y may be NULL when only y_elu is wanted (also
 *                     accepted by sn_linear_fwd_f32).  rows_per_seg >= 32.  Split-bf16 kernels only.
 * sn_linear_dgrad_eluseg_f32 : input gradient through the activation for ALL C columns with a per-mesh vector added before
 *                     the derivative:  gact[r, c] = (dy[r]·W[:, c] + (x[r,c] - center[c]) B[c] + Cc[c] + rowmask[r] *
 *                     segvec[r / rows_per_seg, c]) * elu'(x[r, c]) + gadd[r, c]   (rowmask, gadd may be NULL).
 * sn_linear_dgrad_eluseg_f32 also takes segvec = NULL (then rowmask must be NULL and rows_per_seg is ignored): every column
 * through the activation without a per-mesh vector — the backward of conv(F.elu(v)), the models' last layer.
 * Supported: K in {128, 256} for the forward; C in {128, 256} for the input gradient; J = 128 or, with the split kernels
 * (SN_GEMM_VARIANT != 0), any multiple of 4 up to 128 — the last layer has 120 outputs (models.py:148-150): weights,
 * bias, residual and dy columns past J are never read and nothing is stored past column J of y / y_elu; all leading
 * dimensions multiples of 4 floats, below 2^24 floats (a lane's byte offset inside a 32-row tile is kept in 32 bits),
 * and 16-byte aligned bases (else SN_E_UNSUPPORTED / SN_E_ALIGN: the caller falls back to a library GEMM).
 * The kernels address every streamed matrix through a raw buffer window that ends with its last row: nothing before the
 * first or past the last row of a view, and no column outside it, is read or written (strided views inside larger
 * buffers are safe; tests/test_dense_gpu.py::test_linear_kernels_stay_inside_their_views).
 * elu_stats_part holds sn_linear_fwd_stats_blocks(rows) blocks — the largest grid any forward kernel uses; a kernel with a
 * smaller grid writes zeros into the blocks past its own, so the merge may always read all of them.
 * The launchers pick a kernel form by operand size; two read-only queries say which, so that tests straddle the real
 * thresholds instead of repeating them:
 * sn_linear_small_rows : operands of at most this many rows take the one-pass weight prologue (every Linear entry point).
 * sn_linear_fwd_form   : the form sn_linear_fwd_tiles_f32 launches for these arguments (has_*: the pointer is non-NULL) —
 *                     0 the fp32-MFMA A/B baseline (SN_GEMM_VARIANT=0), 1 split, small operand, 2 split, large operand
 *                     (two-pass weight prologue), 3 the eight-wave forward kernel.  Arguments the launcher would refuse
 *                     are not checked here.
 * ------------------------------------------------------------------------------------------ */
int64_t sn_linear_small_rows(void);
int32_t sn_linear_fwd_form(int64_t rows, int32_t K, int32_t J, int32_t has_residual, int32_t has_y, int32_t has_elu,
                           int32_t has_tile_sums);
int sn_linear_fwd_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                      const float *residual, int64_t ldr, float *y, int64_t ldy, float *y_elu, int64_t lde,
                      int64_t rows, int32_t K, int32_t J, double *elu_stats_part /* NULL | [stats_blocks][2][128] */,
                      void *stream);
int sn_linear_dgrad_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                        const float *center, const float *B, const float *Cc, float *dx, int64_t lddx,
                        int64_t rows, int32_t J, int32_t C, void *stream);
int sn_linear_dgrad_elu_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                            const float *center, const float *B, const float *Cc, float *dx_hi, int64_t lddx,
                            float *gact, int64_t ldga, const float *gadd, int64_t ldgadd,
                            int64_t rows, int32_t J, int32_t C, void *stream);
/* The same launch, which also leaves an upper bound of max |gact| — gact is the dy operand of the layer below, and the
 * two-piece weight gradient (sn_wgrad_*_bounded_f32) needs that bound before it reads the first row.  gact_absmax: device,
 * sn_linear_dgrad_absmax_blocks() floats, one maximum per workgroup (entries past the grid zeroed): the consumer takes the
 * maximum of all of them.  No atomics, no zero-fill before the launch; deterministic.  NULL: as the plain entry point. */
int32_t sn_linear_dgrad_absmax_blocks(void);
int sn_linear_dgrad_elu_absmax_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                                   const float *center, const float *B, const float *Cc, float *dx_hi, int64_t lddx,
                                   float *gact, int64_t ldga, const float *gadd, int64_t ldgadd,
                                   int64_t rows, int32_t J, int32_t C, float *gact_absmax, void *stream);
/* The "raw low half" form: dx_hi as above; columns below C/2 leave as the bare product graw = dy·W[:, :C/2] — no BatchNorm
 * tail, no activation derivative, no maximum — and x[:, :C/2] is NOT READ (the side window starts at column C/2).  The one
 * consumer of that gradient, a transposed product whose epilogue streams the same elu(.) anyway, finishes it
 * (sn_spmm_q3_elubwd_tail_absmax_f32, or sn_elu_tail_finish_f32 in place).  center / B / Cc: the full C-wide vectors (only
 * their high halves are read).  Same shapes, alignment rules and error codes as sn_linear_dgrad_elu_f32. */
int sn_linear_dgrad_elu_rawlow_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                                   const float *center, const float *B, const float *Cc, float *dx_hi, int64_t lddx,
                                   float *graw, int64_t ldgr, int64_t rows, int32_t J, int32_t C, void *stream);
int sn_linear_fwd_segbias_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *segbias,
                              int64_t rows_per_seg, const float *residual, int64_t ldr, float *y, int64_t ldy,
                              float *y_elu, int64_t lde, int64_t rows, int32_t K, int32_t J, double *elu_stats_part,
                              void *stream);
int sn_linear_dgrad_eluseg_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                               const float *center, const float *B, const float *Cc, const float *segvec,
                               int64_t rows_per_seg, const float *rowmask, float *gact, int64_t ldga, const float *gadd,
                               int64_t ldgadd, int64_t rows, int32_t J, int32_t C, void *stream);
/* sn_linear_fwd_tiles_f32 / sn_linear_fwd_segbias_tiles_f32: the two forward launches above, which also leave the column sums of
 * the ACTIVATED output per 32-row tile: tile_sums[(rows + 31) / 32][128] floats (every tile written; J = 128, with y_elu and
 * elu_stats_part).  The half-width global-average stage that consumes y_elu (AvgResNet2, src/utils/utils_pt.py:230-243) then needs
 * no statistics pass over it: sn_avg_stats_from_tiles_f32 forms the per-mesh masked sums from the tiles inside each mesh (rows
 * of tiles shared by two meshes, and of tiles that hold a masked-out row, are read from e) and the BatchNorm sums from the
 * statistics partials — the outputs of sn_avg_stats_f32 (m: nseg x C, stats: 2 x 2C fp64) without reading e
 * (165 MB per stage at the ARAP batch).  workspace: nseg * C floats.  C = 128. */
int sn_linear_fwd_tiles_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *bias, const float *residual,
                            int64_t ldr, float *y, int64_t ldy, float *y_elu, int64_t lde, int64_t rows, int32_t K, int32_t J,
                            double *elu_stats_part, float *tile_sums, void *stream);
/* sn_linear_fwd_frame_f32: the plain forward launch (y only) of a layer whose J outputs are J/3 frames of 3 coordinates — the ARAP
 * models' last layer, 40 predicted frames (src/as_rigid_as_possible/models.py:105,152: `x + inputs[:, :, -3:].repeat(1, 1, 40)`):
 *   y[r][3t + c] = (x·Wᵀ + bias)[r][3t + c] + frame[r·ldf + c],   c < 3, t < J/3
 * with the product and bias formed exactly as sn_linear_fwd_tiles_f32 forms them and the frame value added by one further fp32
 * addition: the same bits as that launch followed by a broadcast add over its result, without the second pass over y.  J a
 * multiple of 12 (J <= 128), K in {128, 256}; frame needs 4-byte alignment only (ldf >= 3: e.g. the last three columns of the
 * (rows, 6) input); only its three addressed columns of rows < `rows` are read.  16-bit matrix-pipe kernels only:
 * sn_linear_fwd_frame_supported says whether this process has them for a K -> J layer (SN_E_UNSUPPORTED otherwise). */
int32_t sn_linear_fwd_frame_supported(int32_t K, int32_t J);
int sn_linear_fwd_frame_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *bias, const float *frame,
                            int64_t ldf, float *y, int64_t ldy, int64_t rows, int32_t K, int32_t J, void *stream);
int sn_linear_fwd_segbias_tiles_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *segbias,
                                    int64_t rows_per_seg, const float *residual, int64_t ldr, float *y, int64_t ldy, float *y_elu,
                                    int64_t lde, int64_t rows, int32_t K, int32_t J, double *elu_stats_part, float *tile_sums,
                                    void *stream);
int sn_avg_stats_from_tiles_f32(const float *tile_sums, const double *stats_part, int32_t nblk, const float *e, int64_t ld,
                                const float *mask, const float *inv_count, int64_t rows_per_seg, int64_t nseg, int32_t C,
                                float *m, double *stats, float *workspace, void *stream);
/* ... and for RAGGED meshes (mesh g = rows [segoff[g], segoff[g+1]), inv_count[g] = 1 / its row count, no mask): the per-mesh means
 * and the statistics of [e | mean broadcast] without a pass over e; sn_linear_fwd_segbias_ragged_tiles_f32 is the ragged
 * per-mesh-bias launch that leaves the tile sums. */
int sn_avg_stats_from_tiles_ragged_f32(const float *tile_sums, const double *stats_part, int32_t nblk, const float *e, int64_t ld,
                                       const int64_t *segoff, const float *inv_count, int64_t nseg, int32_t C, float *m,
                                       double *stats, float *workspace, void *stream);
int sn_linear_fwd_segbias_ragged_tiles_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *segbias,
                                           const int64_t *segoff, int32_t nseg, const float *residual, int64_t ldr, float *y,
                                           int64_t ldy, float *y_elu, int64_t lde, int64_t rows, int32_t K, int32_t J,
                                           double *elu_stats_part, float *tile_sums, void *stream);
/* The two per-mesh-vector kernels for RAGGED meshes (packed batches): mesh g owns rows [segoff[g], segoff[g+1]) (device
 * int64[nseg + 1], segoff[0] = 0, segoff[nseg] = rows, every mesh at least 32 rows — the caller's responsibility: a device
 * array is not validated here); no row mask (a packed batch has no padding rows). */
int sn_linear_fwd_segbias_ragged_f32(const float *x, int64_t ldx, const float *W, int64_t ldw, const float *segbias,
                                     const int64_t *segoff, int32_t nseg, const float *residual, int64_t ldr, float *y,
                                     int64_t ldy, float *y_elu, int64_t lde, int64_t rows, int32_t K, int32_t J,
                                     double *elu_stats_part, void *stream);
int sn_linear_dgrad_eluseg_ragged_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                                      const float *center, const float *B, const float *Cc, const float *segvec,
                                      const int64_t *segoff, int32_t nseg, float *gact, int64_t ldga, const float *gadd,
                                      int64_t ldgadd, int64_t rows, int32_t J, int32_t C, void *stream);
/* ... and with the bound of |gact| for the two-piece weight gradient of the layer below (see sn_linear_dgrad_elu_absmax_f32:
 * gact_absmax holds sn_linear_dgrad_absmax_blocks() floats, one maximum per workgroup). */
int sn_linear_dgrad_eluseg_absmax_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x, int64_t ldx,
                                      const float *center, const float *B, const float *Cc, const float *segvec,
                                      int64_t rows_per_seg, const float *rowmask, float *gact, int64_t ldga, const float *gadd,
                                      int64_t ldgadd, int64_t rows, int32_t J, int32_t C, float *gact_absmax, void *stream);
int sn_linear_dgrad_eluseg_ragged_absmax_f32(const float *dy, int64_t lddy, const float *W, int64_t ldw, const float *x,
                                             int64_t ldx, const float *center, const float *B, const float *Cc,
                                             const float *segvec, const int64_t *segoff, int32_t nseg, float *gact, int64_t ldga,
                                             const float *gadd, int64_t ldgadd, int64_t rows, int32_t J, int32_t C,
                                             float *gact_absmax, void *stream);

/* ---- launch plans: one host call enqueues a whole residual block ------------------------------------------------------------
 * Replaces, per block, the Python dispatch the reference pays per op: LapResNet2 / DirResNet2 / AvgResNet2.forward
 * (src/utils/utils_pt.py:159-180, 191-220, 230-243) and their autograd backward are sequences of torch ops launched one by one
 * from the interpreter inside the training loops (src/as_rigid_as_possible/main.py:217-232, src/mesh_mnist/main.py:151-167,
 * src/dense_correspondence/main.py:310-327), which cannot be graph-captured by an unmodified driver.
 *
 * A plan is a HOST object holding the launch list of one block direction: entries of this header (by index into the table
 * sn_plan_lookup searches) with their scalar arguments, pointer arguments as (slot, byte offset).  The caller supplies the
 * slots' base addresses per run — slot 0/1 by convention the block's two workspace arenas (ONE allocation each, sized once per
 * shape by the caller), the rest the tensors the block reads or writes — and sn_plan_run calls the recorded entry points in
 * order on `stream`: the same launchers, kernels and grids as calling them one by one, bit-identical results.  The library
 * still never allocates device memory, synchronises or keeps per-shape state: plans are created, owned and destroyed by the
 * caller, immutable while running, usable from several threads / streams at once.
 *   kind[i]: 0 integer (ival), 1 floating point (dval), 2 pointer = slot_base[slot[i]] + ival[i], 3 NULL pointer, 4 the stream
 *   (last argument of every entry point).  sn_plan_add_call checks every kind against the parameter type of the entry point
 *   (SN_E_UNSUPPORTED on a mismatch, SN_E_SHAPE on a wrong argument count).
 *   sn_plan_add_memset / sn_plan_add_copy: a byte fill / a device-to-device copy of a 2-D region (rows x width_bytes, pitches in
 *   bytes; rows = 1: flat) — what torch.zeros / Tensor.copy_ do between the reference's ops.
 *   sn_plan_run: 0, or the status of the first failing entry (its index in *failed_node, else -1); SN_E_NULL when a slot a
 *   recorded pointer refers to is handed over as 0. */
typedef struct sn_plan sn_plan;
int sn_plan_create(sn_plan **out);
int sn_plan_destroy(sn_plan *plan);
int32_t sn_plan_lookup(const char *entry_point_name);
int32_t sn_plan_entry_count(void);
const char *sn_plan_entry_name(int32_t fn);
const char *sn_plan_entry_signature(int32_t fn);        /* one char per parameter: p pointer, i integer, d floating point */
int64_t sn_plan_length(const sn_plan *plan);
int sn_plan_add_call(sn_plan *plan, int32_t fn, int32_t nargs, const int32_t *kind, const int32_t *slot, const int64_t *ival,
                     const double *dval);
int sn_plan_add_memset(sn_plan *plan, int32_t slot, int64_t offset, int32_t byte_value, int64_t pitch, int64_t width_bytes,
                       int64_t rows);
int sn_plan_add_copy(sn_plan *plan, int32_t dst_slot, int64_t dst_offset, int64_t dst_pitch, int32_t src_slot, int64_t src_offset,
                     int64_t src_pitch, int64_t width_bytes, int64_t rows);
int sn_plan_run(const sn_plan *plan, const uint64_t *slot_base, int32_t nslots, void *stream, int32_t *failed_node);

/* A plan at FIXED slot addresses as one graph launch.  In a training loop the addresses of a plan run repeat from step to step (the
 * framework's caching allocator hands the same blocks to the same sequence of requests); sn_plan_instantiate captures the launch
 * list at those addresses into an executable hipGraph (kernel nodes only; on a private stream, thread-local capture mode, nothing
 * runs), sn_plan_exec_launch enqueues it on `stream` with ONE hipGraphLaunch — or walks the list like sn_plan_run when `stream` is
 * itself being captured by the caller or the per-launch timer is on (plan and addresses are passed for that).  Same kernels, same
 * arguments, same order: bit-identical to sn_plan_run.  The object is the caller's (keyed by the addresses it was made for, valid
 * while the memory behind them is), holds no device memory; SN_E_UNSUPPORTED while the timer is on. */
typedef struct sn_plan_exec sn_plan_exec;
int sn_plan_instantiate(const sn_plan *plan, const uint64_t *slot_base, int32_t nslots, sn_plan_exec **out, int32_t *failed_node);
int sn_plan_exec_launch(const sn_plan_exec *exec, const sn_plan *plan, const uint64_t *slot_base, int32_t nslots, void *stream,
                        int32_t *failed_node);
int sn_plan_exec_destroy(sn_plan_exec *exec);

#ifdef __cplusplus
}
#endif
#endif /* SN_SPMM_H_ */
