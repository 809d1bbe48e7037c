// sn_attention.hip — graph attention on the pattern of a mesh operator (gfx950, fp32).  The definition is the section "Graph
// attention" of sn_spmm.h; the statement in torch operations is attention.attn_propagate_reference.
//
// One lane layout for every kernel: C / 4 lanes per row with one float4 of the row each (lane `sub` holds channels 4 sub .. 4 sub + 3),
// 64 / (C / 4) rows side by side in a wave, four waves per workgroup.  Head k owns the C / (4 H) consecutive lanes of a row that
// hold its slice, so a per-head dot product is a sum over those lanes (head_sum: DPP inside a row of 16 lanes, two shuffles beyond)
// and every lane of a head holds the head's scalars itself — logits, maximum, normaliser are computed redundantly per lane, never
// exchanged.  A wave owns `iters` consecutive passes of rows; its rows walk their entries in predicated batches of KB with all row
// gathers of a batch in flight, as the generic CSR product does (sn_kernels.hip, spmm_csr_rows_body), so a long row costs a wave
// what it costs there.  The "values" of the product are a few flops from s[R, 2H], which is small enough to stay in cache.
//
// No atomics, no memset, nothing that synchronises: every sum has one owner and a fixed order, so two runs give the same bits, and
// every entry point can be captured into a hipGraph.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
constexpr int kWaves = kWG / 64;
constexpr int KB = 8;                    // row gathers in flight per lane
constexpr float kSlope = 0.2f;           // SN_ATTN_SLOPE
constexpr int kMaxIters = 64;            // passes of rows per wave, at most
constexpr int kBwdBlocks = 1024;         // workgroups of the transposed pass, at most: one (2, C) partial of da each
constexpr int kRedCols = 16, kRedSlices = 16;      // da_reduce_k: 16 columns x 16 slices of the partials per workgroup

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 ld4(const float *p) { return *reinterpret_cast<const f4 *>(p); }
__device__ __forceinline__ f4 ld4_nt(const float *p) { return __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p)); }
__device__ __forceinline__ void st4(float *p, f4 v) { *reinterpret_cast<f4 *>(p) = v; }
__device__ __forceinline__ void st4_nt(float *p, f4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(p)); }
__device__ __forceinline__ f4 fma4(float a, f4 x, f4 acc) {
  acc.x = __builtin_fmaf(a, x.x, acc.x);
  acc.y = __builtin_fmaf(a, x.y, acc.y);
  acc.z = __builtin_fmaf(a, x.z, acc.z);
  acc.w = __builtin_fmaf(a, x.w, acc.w);
  return acc;
}
__device__ __forceinline__ float dot4(f4 a, f4 b) {
  return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }      // (sn_kernels.hip: the library's ELU)
__device__ __forceinline__ float lrelu(float x) { return x > 0.f ? x : x * kSlope; }
__device__ __forceinline__ float lrelu_d(float x) { return x > 0.f ? 1.f : kSlope; }

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Where a lane stands: row slot `grp` of the wave, float4 `sub` of the row, head `head`; lanes past the last whole row idle.
struct Lane {
  int lpr, rpw, lh, H;       // lanes per row, rows per wave pass, lanes per head, heads
  int wave, lane, grp, sub, head;
  bool active, writer;       // writer: the first lane of its head (stores the head's scalars)
  __device__ Lane(int C, int H_) {
    lpr = C >> 2;
    rpw = 64 / lpr;
    H = H_;
    lh = lpr / H;
    wave = threadIdx.x >> 6;
    lane = threadIdx.x & 63;
    grp = lane / lpr;
    sub = lane - grp * lpr;
    head = sub / lh;
    active = grp < rpw;
    writer = active && sub == head * lh;
  }
  // the sum of v over the lanes of this lane's head, in every one of them.  The heads of a row are aligned runs of lh lanes, so for
  // a power of two the butterfly stays inside the head: xor 1 and xor 2 as quad permutes, then the mirror of a half row (lane l of
  // 8 <-> 7 - l: the other quad) and of a row (l of 16 <-> 15 - l: the other half), each adding two operands that already hold
  // the sums of their own sides; 32 and 64 lanes through the shuffle unit.  Both partners of a step add the same two numbers, so the
  // lanes of a head end with the same bits.  Any other head width: every lane adds the head's lanes in ascending order.
  __device__ __forceinline__ float head_sum(float v) const {
    if ((lh & (lh - 1)) == 0) {
      if (lh >= 2) v += dpp<0xB1>(v);        // quad_perm:[1,0,3,2]
      if (lh >= 4) v += dpp<0x4E>(v);        // quad_perm:[2,3,0,1]
      if (lh >= 8) v += dpp<0x141>(v);       // row_half_mirror
      if (lh >= 16) v += dpp<0x140>(v);      // row_mirror
      if (lh >= 32) v += __shfl_xor(v, 16);
      if (lh >= 64) v += __shfl_xor(v, 32);
      return v;
    }
    const int first = lane - (sub - head * lh);
    float t = 0.f;
    for (int q = 0; q < lh; ++q) t += __shfl(v, first + q);
    return t;
  }
};

// the column indices of entries k .. k + KB - 1 of a row that ends at ke; slots past the end repeat the last entry (a valid address)
__device__ __forceinline__ void batch_cols(const int *__restrict__ colind, int k, int ke, int (&c)[KB]) {
#pragma unroll
  for (int j = 0; j < KB; ++j) c[j] = colind[k + j < ke ? k + j : ke - 1];
}

// ---- e = elu(x) into the concat buffer, s = the per-head scores of e ------------------------------------------------------------
__global__ __launch_bounds__(kWG) void attn_elu_scores_k(const float *__restrict__ x, int64_t ldx, const float *__restrict__ a,
                                                         int64_t R, int C, int H, float *__restrict__ e, int64_t lde,
                                                         float *__restrict__ s) {
  const Lane L(C, H);
  if (!L.active) return;
  const f4 a0 = ld4(a + L.sub * 4), a1 = ld4(a + C + L.sub * 4);
  const int64_t stride = (int64_t)gridDim.x * kWaves * L.rpw;
  for (int64_t r = ((int64_t)blockIdx.x * kWaves + L.wave) * L.rpw + L.grp; r < R; r += stride) {
    f4 v = ld4_nt(x + r * ldx + L.sub * 4);
    v.x = elu1(v.x); v.y = elu1(v.y); v.z = elu1(v.z); v.w = elu1(v.w);
    st4(e + r * lde + L.sub * 4, v);                       // (read again by the gathers of the pass that follows: a plain store)
    const float d0 = L.head_sum(dot4(a0, v)), d1 = L.head_sum(dot4(a1, v));
    if (L.writer) {
      s[r * 2 * H + L.head] = d0;
      s[r * 2 * H + H + L.head] = d1;
    }
  }
}

// ---- forward: p = softmax-weighted sum of the gathered rows -------------------------------------------------------------------------
__global__ __launch_bounds__(kWG) void attn_fwd_k(const int *__restrict__ rowptr, const int *__restrict__ colind, int64_t R,
                                                  const float *__restrict__ e, int64_t lde, const float *__restrict__ s, int C, int H,
                                                  int iters, float *__restrict__ p, int64_t ldp, float *__restrict__ m_out,
                                                  float *__restrict__ z_out) {
  const Lane L(C, H);
  if (!L.active) return;
  const float *eb = e + L.sub * 4;
  const float *sb = s + L.head;
  const int64_t r0 = ((int64_t)blockIdx.x * kWaves + L.wave) * L.rpw * iters;
  for (int it = 0; it < iters; ++it) {
    const int64_t r = r0 + (int64_t)it * L.rpw + L.grp;
    if (r >= R) return;
    const int kb = rowptr[r], ke = rowptr[r + 1];
    const float sd = sb[r * 2 * H + H];
    float m = -INFINITY, z = 0.f;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    if (kb < ke) {
      // The first batch — the whole row on a mesh — is loaded once: its indices and logits serve both sweeps, and its row gathers
      // are in flight while the maximum is taken.  (A repeated last entry changes no maximum.)
      int c0[KB];
      float u0[KB];
      f4 x0[KB];
      batch_cols(colind, kb, ke, c0);
#pragma unroll
      for (int j = 0; j < KB; ++j) u0[j] = sb[(int64_t)c0[j] * 2 * H];
#pragma unroll
      for (int j = 0; j < KB; ++j) x0[j] = ld4(eb + (int64_t)c0[j] * lde);
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        u0[j] = lrelu(sd + u0[j]);
        m = fmaxf(m, u0[j]);
      }
      // first sweep over the rest of a longer row: the maximum from the scores alone
      for (int k = kb + KB; k < ke; k += KB) {
        int c[KB];
        float ss[KB];
        batch_cols(colind, k, ke, c);
#pragma unroll
        for (int j = 0; j < KB; ++j) ss[j] = sb[(int64_t)c[j] * 2 * H];
#pragma unroll
        for (int j = 0; j < KB; ++j) m = fmaxf(m, lrelu(sd + ss[j]));
      }
      // second sweep: the normaliser and the weighted rows, entries in ascending order
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (kb + j < ke) {
          const float w = expf(u0[j] - m);
          z += w;
          acc = fma4(w, x0[j], acc);
        }
      }
      for (int k = kb + KB; k < ke; k += KB) {
        int c[KB];
        float ss[KB];
        f4 xr[KB];
        batch_cols(colind, k, ke, c);
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          xr[j] = ld4(eb + (int64_t)c[j] * lde);
          ss[j] = sb[(int64_t)c[j] * 2 * H];
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          if (k + j < ke) {
            const float w = expf(lrelu(sd + ss[j]) - m);
            z += w;
            acc = fma4(w, xr[j], acc);
          }
        }
      }
    }
    f4 out = {0.f, 0.f, 0.f, 0.f};
    if (ke > kb) out = f4{acc.x / z, acc.y / z, acc.z / z, acc.w / z};
    st4_nt(p + r * ldp + L.sub * 4, out);
    if (L.writer) {
      m_out[r * H + L.head] = ke > kb ? m : 0.f;
      z_out[r * H + L.head] = ke > kb ? z : 0.f;
    }
  }
}

// ---- backward, pass 1: rows of A.  ds_dst and the per-row record q = {s_dst, m, 1 / z, D} the transposed pass gathers ---------------
__global__ __launch_bounds__(kWG) void attn_bwd_rows_k(const int *__restrict__ rowptr, const int *__restrict__ colind, int64_t R,
                                                       const float *__restrict__ g, int64_t ldg, const float *__restrict__ e,
                                                       int64_t lde, const float *__restrict__ p, int64_t ldp,
                                                       const float *__restrict__ s, const float *__restrict__ m_in,
                                                       const float *__restrict__ z_in, int C, int H, int iters,
                                                       float *__restrict__ q, float *__restrict__ dsd) {
  const Lane L(C, H);
  if (!L.active) return;
  const float *eb = e + L.sub * 4;
  const float *sb = s + L.head;
  const int64_t r0 = ((int64_t)blockIdx.x * kWaves + L.wave) * L.rpw * iters;
  for (int it = 0; it < iters; ++it) {
    const int64_t r = r0 + (int64_t)it * L.rpw + L.grp;
    if (r >= R) return;
    const int kb = rowptr[r], ke = rowptr[r + 1];
    const f4 gr = ld4_nt(g + r * ldg + L.sub * 4);
    const float D = L.head_sum(dot4(gr, ld4_nt(p + r * ldp + L.sub * 4)));
    const float sd = sb[r * 2 * H + H];
    const float m = m_in[r * H + L.head];
    const float rz = ke > kb ? 1.f / z_in[r * H + L.head] : 0.f;
    float acc = 0.f;
    for (int k = kb; k < ke; k += KB) {
      int c[KB];
      float ss[KB], da[KB];
      f4 xr[KB];
      batch_cols(colind, k, ke, c);
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        xr[j] = ld4(eb + (int64_t)c[j] * lde);
        ss[j] = sb[(int64_t)c[j] * 2 * H];
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) da[j] = L.head_sum(dot4(gr, xr[j]));
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (k + j < ke) {
          const float pre = sd + ss[j];
          const float alpha = expf(lrelu(pre) - m) * rz;
          acc += alpha * (da[j] - D) * lrelu_d(pre);
        }
      }
    }
    if (L.writer) {
      dsd[r * H + L.head] = acc;
      st4(q + (r * H + L.head) * 4, f4{sd, m, rz, D});
    }
  }
}

// ---- backward, pass 2: rows of A^T.  Row j keeps e[j] and gathers g[i] and q[i]; writes dx[j] and the workgroup's share of da -----
__global__ __launch_bounds__(kWG) void attn_bwd_cols_k(const int *__restrict__ t_rowptr, const int *__restrict__ t_colind, int64_t R,
                                                       const float *__restrict__ g, int64_t ldg, const float *__restrict__ ge,
                                                       int64_t ldge, const float *__restrict__ e, int64_t lde,
                                                       const float *__restrict__ s, const float *__restrict__ q,
                                                       const float *__restrict__ dsd, const float *__restrict__ a, int C, int H,
                                                       int iters, float *__restrict__ dx, int64_t lddx, float *__restrict__ part) {
  __shared__ float s_da[kWaves][64][8];
  const Lane L(C, H);
  f4 da0 = {0.f, 0.f, 0.f, 0.f}, da1 = da0;
  if (L.active) {
    const f4 a0 = ld4(a + L.sub * 4), a1 = ld4(a + C + L.sub * 4);
    const float *gb = g + L.sub * 4;
    const int64_t r0 = ((int64_t)blockIdx.x * kWaves + L.wave) * L.rpw * iters;
    for (int it = 0; it < iters; ++it) {
      const int64_t r = r0 + (int64_t)it * L.rpw + L.grp;
      if (r >= R) break;
      const int kb = t_rowptr[r], ke = t_rowptr[r + 1];
      const f4 er = ld4(e + r * lde + L.sub * 4);
      const float ss = s[r * 2 * H + L.head];
      float dss = 0.f;
      f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k = kb; k < ke; k += KB) {
        int c[KB];
        float da[KB];
        f4 gi[KB], qi[KB];
        batch_cols(t_colind, k, ke, c);
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          gi[j] = ld4(gb + (int64_t)c[j] * ldg);
          qi[j] = ld4(q + ((int64_t)c[j] * H + L.head) * 4);
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) da[j] = L.head_sum(dot4(gi[j], er));
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          if (k + j < ke) {
            const float pre = qi[j].x + ss;
            const float alpha = expf(lrelu(pre) - qi[j].y) * qi[j].z;
            dss += alpha * (da[j] - qi[j].w) * lrelu_d(pre);
            acc = fma4(alpha, gi[j], acc);
          }
        }
      }
      const float dd = dsd[r * H + L.head];
      f4 de = fma4(dd, a1, fma4(dss, a0, acc));
      if (ge) {                                           // the gradient of the elu half and elu' through the activation output
        de += ld4_nt(ge + r * ldge + L.sub * 4);
        de = f4{de.x * (er.x > 0.f ? 1.f : er.x + 1.f), de.y * (er.y > 0.f ? 1.f : er.y + 1.f),
                de.z * (er.z > 0.f ? 1.f : er.z + 1.f), de.w * (er.w > 0.f ? 1.f : er.w + 1.f)};
      }
      st4_nt(dx + r * lddx + L.sub * 4, de);
      da0 = fma4(dss, er, da0);
      da1 = fma4(dd, er, da1);
    }
  }
  // the workgroup's (2, C) share of da: every lane's sums over its rows, then waves and row slots in ascending order
  float *mine = s_da[threadIdx.x >> 6][threadIdx.x & 63];
  st4(mine, da0);
  st4(mine + 4, da1);
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * C; o += kWG) {
    const int which = o >= C, col = o - which * C;
    const int sub = col >> 2, comp = (col & 3) + 4 * which;
    float t = 0.f;
    for (int w = 0; w < kWaves; ++w)
      for (int gslot = 0; gslot < L.rpw; ++gslot) t += s_da[w][gslot * L.lpr + sub][comp];
    part[(int64_t)blockIdx.x * 2 * C + o] = t;
  }
}

// da[o] = the sum over the workgroups' partials, o < 2 C: slice q of a column adds partials q, q + 16, ... in float64, then the
// slices are added in ascending order
__global__ __launch_bounds__(kRedCols *kRedSlices) void attn_da_reduce_k(const float *__restrict__ part, int nblocks, int C2,
                                                                         float *__restrict__ da) {
  __shared__ double s_sum[kRedSlices][kRedCols];
  const int col = threadIdx.x % kRedCols, slice = threadIdx.x / kRedCols;
  const int o = blockIdx.x * kRedCols + col;
  double t = 0.0;
  if (o < C2)
    for (int b = slice; b < nblocks; b += kRedSlices) t += (double)part[(int64_t)b * C2 + o];
  s_sum[slice][col] = t;
  __syncthreads();
  if (slice == 0 && o < C2) {
    double tot = 0.0;
    for (int q = 0; q < kRedSlices; ++q) tot += s_sum[q][col];
    da[o] = (float)tot;
  }
}

inline bool supported(int32_t C, int32_t H) {
  return C >= 4 && C <= SN_ATTN_MAX_CHANNELS && C % 4 == 0 && H >= 1 && C % H == 0 && (C / H) % 4 == 0;
}
inline bool aligned16(const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ld % 4 == 0; }

// passes of rows per wave and the workgroups that take R rows at `rpw` rows per wave pass, at most `cap` workgroups where the
// passes allow it (a function of the shapes alone: the partition decides the order of the sums)
inline void partition(int64_t R, int rpw, int64_t cap, int *iters, unsigned *blocks) {
  const int64_t per_pass = (int64_t)kWaves * rpw;
  int64_t it = (R + per_pass * cap - 1) / (per_pass * cap);
  it = it < 1 ? 1 : it > kMaxIters ? kMaxIters : it;
  int64_t b = (R + per_pass * it - 1) / (per_pass * it);
  *iters = (int)it;
  *blocks = (unsigned)(b < 1 ? 1 : b);
}

// what the two propagate entries check of the operator and the widths
inline int check_operator(int64_t M, int64_t K, int64_t nnz, int32_t C, int32_t H) {
  if (M < 0 || K < 0 || nnz < 0 || M != K) return SN_E_SHAPE;
  if (M >= INT32_MAX || nnz > INT32_MAX) return SN_E_RANGE;
  if (!supported(C, H)) return SN_E_UNSUPPORTED;
  return SN_OK;
}

struct BwdWorkspace {
  float *q, *dsd, *part;
  size_t bytes;
  BwdWorkspace(void *base, int64_t R, int32_t C, int32_t H, unsigned blocks) {
    SnCarver carve(base);
    q = carve.take<float>((size_t)R * H * 4);
    dsd = carve.take<float>((size_t)R * H);
    part = carve.take<float>((size_t)blocks * 2 * C);
    bytes = carve.bytes;
  }
};

}  // namespace

extern "C" {

int32_t sn_attn_supported(int32_t C, int32_t H) { return supported(C, H) ? 1 : 0; }

int sn_attn_elu_scores_f32(const float *x, int64_t ldx, const float *a, int64_t R, int32_t C, int32_t H, float *e, int64_t lde,
                           float *s, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (R < 0) return SN_E_SHAPE;
  if (!supported(C, H)) return SN_E_UNSUPPORTED;
  if (ldx < C || lde < C) return SN_E_LD;
  if (R >= INT32_MAX) return SN_E_RANGE;
  if (R == 0) return SN_OK;
  if (!x || !a || !e || !s) return SN_E_NULL;
  if (!aligned16(x, ldx) || !aligned16(e, lde) || !aligned16(a, C)) return SN_E_ALIGN;
  const int rpw = 64 / (C / 4);
  hipLaunchKernelGGL(attn_elu_scores_k, dim3(grid_for(R, kWaves * rpw, 65535 * 4)), dim3(kWG), 0, static_cast<hipStream_t>(stream), x,
                     ldx, a, R, (int)C, (int)H, e, lde, s);
  return launch_status();
}

int sn_attn_propagate_fwd_f32(const int32_t *rowptr, const int32_t *colind, int64_t M, int64_t K, int64_t nnz, const float *e,
                              int64_t lde, const float *s, int32_t C, int32_t H, float *p, int64_t ldp, float *m, float *z,
                              void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (const int st = check_operator(M, K, nnz, C, H)) return st;
  if (lde < C || ldp < C) return SN_E_LD;
  if (M == 0) return SN_OK;
  if (!rowptr || (nnz && !colind) || !e || !s || !p || !m || !z) return SN_E_NULL;
  if (!aligned16(e, lde) || !aligned16(p, ldp)) return SN_E_ALIGN;
  int iters;
  unsigned blocks;
  partition(M, 64 / (C / 4), 8192, &iters, &blocks);
  hipLaunchKernelGGL(attn_fwd_k, dim3(blocks), dim3(kWG), 0, static_cast<hipStream_t>(stream), rowptr, colind, M, e, lde, s, (int)C,
                     (int)H, iters, p, ldp, m, z);
  return launch_status();
}

size_t sn_attn_propagate_bwd_workspace_bytes(int64_t R, int32_t C, int32_t H) {
  if (R < 0 || !supported(C, H)) return 0;
  int iters;
  unsigned blocks;
  partition(R, 64 / (C / 4), kBwdBlocks, &iters, &blocks);
  return BwdWorkspace(nullptr, R, C, H, blocks).bytes;
}

int sn_attn_propagate_bwd_f32(const int32_t *rowptr, const int32_t *colind, const int32_t *t_rowptr, const int32_t *t_colind,
                              int64_t M, int64_t K, int64_t nnz, const float *g, int64_t ldg, const float *ge, int64_t ldge,
                              const float *e, int64_t lde, const float *p, int64_t ldp, const float *s, const float *m,
                              const float *z, const float *a, int32_t C, int32_t H, float *dx, int64_t lddx, float *da,
                              void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (const int st = check_operator(M, K, nnz, C, H)) return st;
  if (ldg < C || (ge && ldge < C) || lde < C || ldp < C || lddx < C) return SN_E_LD;
  if (!da) return SN_E_NULL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rpw = 64 / (C / 4);
  int iters1, iters2;
  unsigned blocks1, blocks2;
  partition(M, rpw, 8192, &iters1, &blocks1);
  partition(M, rpw, kBwdBlocks, &iters2, &blocks2);
  if (M == 0) {                                  // no row: da = 0 from a reduction over no partial
    hipLaunchKernelGGL(attn_da_reduce_k, dim3((2 * C + kRedCols - 1) / kRedCols), dim3(kRedCols * kRedSlices), 0, st, nullptr, 0,
                       2 * (int)C, da);
    return launch_status();
  }
  if (!rowptr || !t_rowptr || (nnz && (!colind || !t_colind)) || !g || !e || !p || !s || !m || !z || !a || !dx) return SN_E_NULL;
  if (!aligned16(g, ldg) || (ge && !aligned16(ge, ldge)) || !aligned16(e, lde) || !aligned16(p, ldp) || !aligned16(dx, lddx) ||
      !aligned16(a, C) || !aligned16(workspace, 4))
    return SN_E_ALIGN;
  const BwdWorkspace ws(workspace, M, C, H, blocks2);
  if (!workspace || workspace_bytes < ws.bytes) return SN_E_WORKSPACE;
  hipLaunchKernelGGL(attn_bwd_rows_k, dim3(blocks1), dim3(kWG), 0, st, rowptr, colind, M, g, ldg, e, lde, p, ldp, s, m, z, (int)C,
                     (int)H, iters1, ws.q, ws.dsd);
  hipLaunchKernelGGL(attn_bwd_cols_k, dim3(blocks2), dim3(kWG), 0, st, t_rowptr, t_colind, M, g, ldg, ge, ldge, e, lde, s, ws.q,
                     ws.dsd, a, (int)C, (int)H, iters2, dx, lddx, ws.part);
  hipLaunchKernelGGL(attn_da_reduce_k, dim3((2 * C + kRedCols - 1) / kRedCols), dim3(kRedCols * kRedSlices), 0, st, ws.part,
                     (int)blocks2, 2 * (int)C, da);
  return launch_status();
}

}  // extern "C"
