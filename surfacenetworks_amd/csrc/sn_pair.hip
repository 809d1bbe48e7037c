// sn_pair.hip — the three dense-correspondence losses computed from the tower features, WITHOUT the score matrix (gfx950):
// `dcel` (hard argmin target, sn_pair_fused_*), `cel` (soft target, sn_pair_soft_*) and `sl1` (smooth-L1, sn_pair_sl1_*); and
// what the trained network PREDICTS, from the same streamed score tiles: the arg-max of every row and of every column
// (sn_pair_match_f32).
// src/dense_correspondence/models.py:203 bmm(FA, FB^T) followed by one of main.py:197-240: the 7000 x 7000 scores are formed
// tile by tile on the fp16 matrix pipe and reduced on the spot; forward and backward never write them.
// (The losses on a materialised score matrix, pair_argmin* and pair_ce_*, are in sn_dense.hip.)
//
// Arithmetic: the two-piece fp16 split of the Linear kernels (sn_gemm.hip).  x·up = h + l with h = rn16(x·up),
// l = rn16(x·up - h) holds 22+ significant bits, `up` an exact power of two taken from the MATRIX's absolute maximum (so it
// factors out of every contraction); a product is the three partial products l·h + h·l + h·h, each exact in the fp32
// accumulator of v_mfma_f32_32x32x16_f16 (the dropped l·l is below 2^-24 of the term).  Elements more than 2^16 below the
// matrix maximum lose low-order bits of l: an ABSOLUTE error below 2^-39 of the maximum, nothing next to the fp32 rounding of
// a 120-term sum.  The factor P of the gradient, in [-1, 1] for all three losses, is split the same way after scaling by 2^14.
//
// Layout: every operand is stored in MFMA FRAGMENT ORDER, 32 rows (a "tile") at a time — [tile][k-step][piece][lane][8 halfs],
// lane (i, kh) holding row i's elements 8 kh .. 8 kh + 7 of the k-step — so that one wave-wide LDS-DMA instruction moves 1 KiB
// of contiguous global memory into 1 KiB of LDS that ds_read_b128 then reads without bank conflicts: no transposition, no
// address arithmetic per element.  R holds the features for the score product (contraction over the feature index), T holds
// them transposed for the gradient product (contraction over the streamed rows, in the order the accumulator of the score
// tile hands them over: pair_perm).
//
//   pair_maxabs_k      absolute maximum of both feature matrices -> the two scales
//   pair_split_k       F -> R, T of both sides (cel / sl1: rows taken through a map, "label order" below)
//   pair_fwd_k<Loss>   a workgroup owns 128 rows of A (4 waves x 32, fragments in registers) and streams a RANGE of B's tiles
//                      through a double-buffered LDS stage; the tile is computed TRANSPOSED (lane = row of A), so the
//                      reductions of a row stay inside a lane; the row's share per range -> pair_*combine_k
//   pair_grad_k<Loss>  both gradients in one launch: a workgroup owns 128 rows of one side and streams a range of the other
//                      side's tiles (R and T); scores recomputed, P split in registers — the accumulator layout of the
//                      transposed tile IS the operand layout of the second product — dOwn += P·Other; partial sums per range
//   pair_reduce_k      sums the ranges in fixed order, applies gloss and the scales, scatters the rows through the map,
//                      zero-fills the padding rows
// Loss = PairHard | PairSoft | PairSl1: what differs between the losses, and nothing else (see "The loss policies").
// PairMatch is a fourth, forward-only policy of pair_fwd_k (row arg-max; pair_match_combine_k folds the ranges).

#include <algorithm>
#include <limits.h>

#include "sn_dense_common.h"

namespace {

constexpr int kPairKP = 128;                       // padded feature count (K <= 128)
constexpr int kPairTile = 32 * kPairKP * 2;        // halfs of one tile of R (or T): 8 (or 4 x 2) k-steps x 2 pieces x 64 lanes x 8
constexpr int kPairChunk = 512;                    // halfs per DMA instruction (64 lanes x 16 B)
constexpr int kPairMaxLseSplits = 8, kPairMaxGradSplits = 4;
constexpr int kPairHeader = 256;                   // bytes: [0] max|FA| bits, [1] max|FB| bits

template <int N_>
__device__ __forceinline__ void pair_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}
// up = 2^(14 - E), down = 2^(E - 14) for an absolute maximum m = f·2^E, f in [0.5, 1)
__device__ __forceinline__ void pair_scales(unsigned mbits, float &up, float &down) {
  int e = (int)((mbits >> 23) & 0xffu) - 126;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);       // zero / denormal / non-finite matrices: any finite scale will do
  up = __uint_as_float((unsigned)(127 + 14 - e) << 23);
  down = __uint_as_float((unsigned)(127 - 14 + e) << 23);
}

__global__ __launch_bounds__(kWG) void pair_maxabs_k(const float *__restrict__ FA, int64_t lda, int rowsA, const float *__restrict__ FB,
                                                     int64_t ldb, int rowsB, int K, unsigned *__restrict__ header) {
  const float *F = blockIdx.y ? FB : FA;
  const int64_t ld = blockIdx.y ? ldb : lda;
  const int64_t total = (int64_t)(blockIdx.y ? rowsB : rowsA) * K;
  unsigned m = 0;
  for (int64_t id = (int64_t)blockIdx.x * kWG + threadIdx.x; id < total; id += (int64_t)gridDim.x * kWG) {
    const unsigned b = __float_as_uint(F[id / K * ld + id % K]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned q = (unsigned)__shfl_xor((int)m, o);
    m = q > m ? q : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(header + blockIdx.y, m);
}

// one thread per (row, 4 features) of a side (blockIdx.y): rows [0, npad), feature quads [0, 32)
// MAP: position `row` of R / T takes row map[row] of F for row < nmap (a permutation of [0, nmap)), row `row` itself past it
// WITH_T = false: R only (forward-only users; TA / TB are not touched)
template <bool MAP, bool WITH_T = true>
__global__ __launch_bounds__(kWG) void pair_split_k(const float *__restrict__ FA, int64_t lda, int rowsA, int npadA, unsigned short *__restrict__ RA,
                                                    unsigned short *__restrict__ TA, const float *__restrict__ FB, int64_t ldb, int rowsB,
                                                    int npadB, unsigned short *__restrict__ RB, unsigned short *__restrict__ TB, int K,
                                                    const unsigned *__restrict__ header, const int64_t *__restrict__ mapA, int nmapA,
                                                    const int64_t *__restrict__ mapB, int nmapB) {
  const bool sb = blockIdx.y != 0;
  const float *F = sb ? FB : FA;
  const int64_t ld = sb ? ldb : lda;
  const int n = sb ? rowsB : rowsA, npad = sb ? npadB : npadA;
  unsigned short *R = sb ? RB : RA, *T = sb ? TB : TA;
  const int64_t id = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (id >= (int64_t)npad * 32) return;
  float up, down;
  pair_scales(header[sb ? 1 : 0], up, down);
  const int row = (int)(id >> 5), kq = (int)(id & 31) * 4;
  int64_t src = row;
  if (MAP) {
    const int64_t *map = sb ? mapB : mapA;
    if (map && row < (sb ? nmapB : nmapA)) src = map[row];
  }
  _Float16 h[4], l[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float v = ((row < n && kq + c < K) ? F[src * ld + kq + c] : 0.f) * up;
    h[c] = (_Float16)v;
    l[c] = (_Float16)(v - (float)h[c]);
  }
  const int t = row >> 5, i = row & 31;
  {  // R: [t][ks][p][kh*32 + i][j], k = 16 ks + 8 kh + j
    const int ks = kq >> 4, kh = (kq >> 3) & 1, j = kq & 7;
    _Float16 *r = reinterpret_cast<_Float16 *>(R) + (size_t)t * kPairTile + ((size_t)(ks * 2) * 64 + kh * 32 + i) * 8 + j;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      r[c] = h[c];
      r[512 + c] = l[c];
    }
  }
  if constexpr (WITH_T) {  // T: [t][f][s2][p][kh*32 + kfl][j], feature 32 f + kfl, streamed row 16 s2 + 8 (j >> 2) + 4 kh + (j & 3)  (pair_perm)
    const int s2 = i >> 4, r16 = i & 15, kh = (r16 >> 2) & 1, j = 4 * (r16 >> 3) + (r16 & 3);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int kf = kq + c, f = kf >> 5, kfl = kf & 31;
      _Float16 *q = reinterpret_cast<_Float16 *>(T) + (size_t)t * kPairTile + ((size_t)((f * 2 + s2) * 2) * 64 + kh * 32 + kfl) * 8 + j;
      q[0] = h[c];
      q[512] = l[c];
    }
  }
}

// the wave's share (chunks wave, wave + 4, ...) of NCH 1 KiB chunks from global memory into the LDS stage
template <int NCH>
__device__ __forceinline__ void pair_stage(const unsigned short *__restrict__ src, unsigned short *dst, int wave, int lane) {
#pragma unroll
  for (int q = 0; q < NCH / 4; ++q) {
    const int c = wave + 4 * q;
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const u4 *>(src + (size_t)c * kPairChunk) + lane, dst + c * kPairChunk, 16, 0, 0);
  }
}

// transposed score tile from the staged R tile: D[i][n] = sum_k Other[i][k] · Own[n][k]   (lane & 31 = n; element e <-> streamed
// row i = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)); two accumulators (even / odd k-steps) halve the dependent chain
__device__ __forceinline__ f16v pair_tile(const u4 (&own)[8][2], const unsigned short *st, int lane) {
  const u4 *s4 = reinterpret_cast<const u4 *>(st) + lane;
  f16v a0, a1;
#pragma unroll
  for (int e = 0; e < 16; ++e) a0[e] = a1[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ks += 2) {
    const u4 h0 = s4[(ks * 2) * 64], l0 = s4[(ks * 2 + 1) * 64], h1 = s4[(ks * 2 + 2) * 64], l1 = s4[(ks * 2 + 3) * 64];
    a0 = mfma_f16(l0, own[ks][0], a0);
    a1 = mfma_f16(l1, own[ks + 1][0], a1);
    a0 = mfma_f16(h0, own[ks][1], a0);
    a1 = mfma_f16(h1, own[ks + 1][1], a1);
    a0 = mfma_f16(h0, own[ks][0], a0);
    a1 = mfma_f16(h1, own[ks + 1][0], a1);
  }
  return a0 + a1;
}

__device__ __forceinline__ void pair_load_own(u4 (&own)[8][2], const unsigned short *__restrict__ R, int tile, int lane) {
  const u4 *g = reinterpret_cast<const u4 *>(R + (size_t)tile * kPairTile) + lane;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    own[ks][0] = g[(ks * 2) * 64];
    own[ks][1] = g[(ks * 2 + 1) * 64];
  }
}


// ------------------------------------------------------------------------------------------------
// Label order: the geodesics of `cel` (loss_fun_cross_entropy, main.py:216-227) and `sl1` (loss_fun_sl1 + aggregate_batch_G,
// main.py:197-214).  Both compare S = FA·FB^T with G[r][j] = GA[r][liA[lB[j]]] + GB[liB[lA[r]]][j] ELEMENT BY ELEMENT, so G is
// read in the 32 x 32 tiles of the score kernels.  In the vertex numbering that is a gather of scattered columns; with label /
// label_inv mutually inverse it is (HA + HB)[lA[r]][lB[j]], H = G_frame[label_inv][:, label_inv] built once per frame.  So the
// kernels run in LABEL ORDER: row u of the tile grid is vertex mapA[u] = liA[u] of shape A, column v vertex mapB[v] of shape
// B, both matrices are read as contiguous row segments, and the only permutation left is on the feature rows (pair_split_k
// on the way in, pair_reduce_k on the way out).  Every sum runs over all (r, j) or all j of a row: the numbering changes the
// order of summation and nothing else.  The two base addresses come from a DEVICE table: a captured step replays on another
// pair by rewriting 16 bytes, not by copying 2 x 190 MB into static buffers.
// ------------------------------------------------------------------------------------------------
// what a loss reads besides the features; members a loss does not use are null / 0
struct PairIn {
  const float *const *base;      // cel, sl1: device table {HA, HB}
  int64_t ldA, ldB;
  int NA, NB;                    // the scored corner: the rows that have stats / targets, the part of G that exists
  const float *stats;            // dcel: lse[NA]; cel: lse[NA] | dmin[NA]  (gradient only)
  const int64_t *target;         // dcel: [NA]
};
__device__ __forceinline__ bool pair_geo_vec(const float *ga, const float *gb, const PairIn &G) {
  return (((reinterpret_cast<uintptr_t>(ga) | reinterpret_cast<uintptr_t>(gb)) & 15) == 0) && (G.ldA % 4) == 0 && (G.ldB % 4) == 0;
}
// columns c .. c + 3 (c a multiple of 4) of a row; 0 past ncols
__device__ __forceinline__ f4 pair_geo4(const float *__restrict__ row, int c, int ncols, bool vec) {
  if (vec && c + 3 < ncols) return *reinterpret_cast<const f4 *>(row + c);
  f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = c + e < ncols ? row[c + e] : 0.f;
  return v;
}
// G for the 16 elements of a transposed tile whose OWN rows are rows of G (lane's row u fixed, streamed columns c0 + ...):
// element e <-> column c0 + (e & 3) + 8 (e >> 2), c0 = 32 t + 4 kh
__device__ __forceinline__ void pair_geo_own_row(float (&g)[16], const float *rowa, const float *rowb, bool row_ok, int c0, int ncols, bool vec) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f4 a = f4{0.f, 0.f, 0.f, 0.f}, b = a;
    if (row_ok && c0 + 8 * q < ncols) {
      a = pair_geo4(rowa, c0 + 8 * q, ncols, vec);
      b = pair_geo4(rowb, c0 + 8 * q, ncols, vec);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) g[4 * q + c] = a[c] + b[c];
  }
}
// ... whose own rows are COLUMNS of G (lane's column v fixed, streamed rows u0 + ...)
__device__ __forceinline__ void pair_geo_own_col(float (&g)[16], const float *ga, const float *gb, const PairIn &G, bool col_ok, int v, int u0) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int u = u0 + (e & 3) + 8 * (e >> 2);
    g[e] = (col_ok && u < G.NA) ? ga[(int64_t)u * G.ldA + v] + gb[(int64_t)u * G.ldB + v] : 0.f;
  }
}
__device__ __forceinline__ float pair_sl1(float d) {
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

struct PairGradSide {
  const unsigned short *Rown, *Roth, *Toth;
  float *part;             // [splits][npad_own][128]
  int Nown, Noth, npad_own, nblk, splits;
};

// ------------------------------------------------------------------------------------------------
// The loss policies: structs of inlined static functions and constants, nothing chosen at run time.
//   kGeo, kAuxLoads, kMean   geodesics read?; LDS-DMA loads per issue() of pair_grad_k besides the 8 of the R and T tiles;
//                            gradient scaled by gloss / scale (true) or gloss · scale (false)
//   Fwd, fwd_init / _tile / _store   a lane's running state in pair_fwd_k; its update from the 16 scores acc[e]·sAB of a tile
//                            (element e <-> column c0 + pair_col(e) < cols, gv their geodesics); half-wave fold and store
//   grad_own, grad_aux, grad_p   the two values (v0, v1) a row of A carries — read directly where the workgroup owns rows of A,
//                            streamed through the wave's 256-byte auxiliary slot (lanes 0..31 v0, 32..63 v1 of rows 32 t + n)
//                            where it owns rows of B — and P of one element from (s, v0, v1, gv, its column `col`)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pair_col(int e) { return (e & 3) + 8 * (e >> 2); }

// `dcel`: rowloss[u] = lse_S[u] - S[u][target[u]];  P = softmax(S) - onehot(target)
struct PairHard {
  static constexpr bool kGeo = false;
  static constexpr int kAuxLoads = 1;
  static constexpr bool kMean = true;
  struct Fwd { float m, l, tl; int tgt; };
  static __device__ __forceinline__ Fwd fwd_init(const PairIn &G, int u, int rows) {
    return Fwd{-INFINITY, 0.f, 0.f, u < rows ? (int)G.target[u] : -1};
  }
  static __device__ __forceinline__ void fwd_tile(Fwd &st, const f16v &acc, float sAB, int c0, int cols, float (&)[16]) {
    float sv[16], tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = c0 + pair_col(e);
      const float s = acc[e] * sAB;
      sv[e] = i < cols ? s : -INFINITY;
      st.tl += i == st.tgt ? s : 0.f;
      tmax = fmaxf(tmax, sv[e]);
    }
    if (tmax > -INFINITY) {
      const float mn = fmaxf(st.m, tmax);
      float add = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) add += __expf(sv[e] - mn);          // (exp(-inf) = 0 for the columns past NB)
      st.l = st.l * __expf(st.m - mn) + add;
      st.m = mn;
    }
  }
  // part[split][row][4] = (max, sum, target logit, -)
  static __device__ __forceinline__ void fwd_store(const Fwd &st, bool write, size_t slot, float *part, float *) {
    const float m2 = __shfl_xor(st.m, 32), l2 = __shfl_xor(st.l, 32), t2 = __shfl_xor(st.tl, 32);
    const float mn = fmaxf(st.m, m2);
    const float l = (st.m > -INFINITY ? st.l * __expf(st.m - mn) : 0.f) + (m2 > -INFINITY ? l2 * __expf(m2 - mn) : 0.f);
    if (write) *reinterpret_cast<f4 *>(part + slot * 4) = f4{mn, l, st.tl + t2, 0.f};
  }
  // v1 is the target's BIT PATTERN (low word of the int64 entry; -1 is a NaN pattern): move and compare it, never compute on it
  static __device__ __forceinline__ void grad_own(float &v0, float &v1, const PairIn &G, int u, bool ok) {
    v0 = ok ? G.stats[u] : 0.f;
    v1 = __int_as_float(ok ? (int)G.target[u] : -1);
  }
  static __device__ __forceinline__ const void *grad_aux(const PairIn &G, int i, int kh) {
    return kh ? static_cast<const void *>(G.target + i) : static_cast<const void *>(G.stats + i);
  }
  static __device__ __forceinline__ float grad_p(float s, float lse, float tgt, float, int col) {
    return __expf(s - lse) - (__float_as_int(tgt) == col ? 1.f : 0.f);
  }
};

// `cel`: the soft-max statistics of S and an online soft-min of G (row minimum, sum exp(-(G - min)), the same weighted by S)
// over the NA x NB corner;  P = exp(S - lse[u]) - exp(dmin[u] - G)
struct PairSoft {
  static constexpr bool kGeo = true;
  static constexpr int kAuxLoads = 1;
  static constexpr bool kMean = false;
  struct Fwd { float m, l, gm, gl, gts; };
  static __device__ __forceinline__ Fwd fwd_init(const PairIn &, int, int) { return Fwd{-INFINITY, 0.f, INFINITY, 0.f, 0.f}; }
  static __device__ __forceinline__ void fwd_tile(Fwd &st, const f16v &acc, float sAB, int c0, int cols, float (&gv)[16]) {
    float sv[16], tmax = -INFINITY, tmin = INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = c0 + pair_col(e);
      sv[e] = acc[e] * sAB;
      if (i >= cols) gv[e] = INFINITY;
      tmax = fmaxf(tmax, i < cols ? sv[e] : -INFINITY);
      tmin = fminf(tmin, gv[e]);
    }
    if (tmax > -INFINITY) {                        // (the lane holds at least one column of the corner)
      const float mn = fmaxf(st.m, tmax), gn = fminf(st.gm, tmin);
      float add = 0.f, gadd = 0.f, gsadd = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = c0 + pair_col(e);
        add += i < cols ? __expf(sv[e] - mn) : 0.f;
        const float w = __expf(gn - gv[e]);        // (exp(-inf) = 0 for the columns past NB)
        gadd += w;
        gsadd += w * sv[e];
      }
      st.l = st.l * __expf(st.m - mn) + add;
      st.m = mn;
      const float sc = __expf(gn - st.gm);         // (first tile: exp(-inf) = 0 times 0)
      st.gl = st.gl * sc + gadd;
      st.gts = st.gts * sc + gsadd;
      st.gm = gn;
    }
  }
  // part[split][row][4] = (max, sum, -, -), part2[split][row][4] = (min G, sum exp(-(G - min)), sum exp(-(G - min)) S, -)
  static __device__ __forceinline__ void fwd_store(const Fwd &st, bool write, size_t slot, float *part, float *part2) {
    const float m2 = __shfl_xor(st.m, 32), l2 = __shfl_xor(st.l, 32);
    const float gm2 = __shfl_xor(st.gm, 32), gl2 = __shfl_xor(st.gl, 32), gts2 = __shfl_xor(st.gts, 32);
    const float mn = fmaxf(st.m, m2), gn = fminf(st.gm, gm2);
    const float l = (st.m > -INFINITY ? st.l * __expf(st.m - mn) : 0.f) + (m2 > -INFINITY ? l2 * __expf(m2 - mn) : 0.f);
    const float c1 = st.gm < INFINITY ? __expf(gn - st.gm) : 0.f, c2 = gm2 < INFINITY ? __expf(gn - gm2) : 0.f;
    if (write) {
      // (a sum of two products: WHICH one is fused into the addition is the compiler's choice under -ffp-contract=fast and
      //  moves the last bit, so it is spelled out — the other half-wave's product is rounded, this one's is not)
      *reinterpret_cast<f4 *>(part + slot * 4) = f4{mn, l, 0.f, 0.f};
      *reinterpret_cast<f4 *>(part2 + slot * 4) = f4{gn, __fmaf_rn(st.gl, c1, gl2 * c2), __fmaf_rn(st.gts, c1, gts2 * c2), 0.f};
    }
  }
  static __device__ __forceinline__ void grad_own(float &v0, float &v1, const PairIn &G, int u, bool ok) {
    v0 = ok ? G.stats[u] : 0.f;
    v1 = ok ? G.stats[G.NA + u] : 0.f;
  }
  static __device__ __forceinline__ const void *grad_aux(const PairIn &G, int i, int kh) { return G.stats + (kh ? G.NA : 0) + i; }
  static __device__ __forceinline__ float grad_p(float s, float lse, float dmin, float gv, int) {
    return __expf(s - lse) - __expf(dmin - gv);
  }
};

// `sl1`: the row's share of sum l(S - FullG) over the WHOLE rows x cols rectangle (gv = 0 outside the corner: FullG), in
// fp64 across tiles;  P = clamp(S - FullG, -1, 1)
struct PairSl1 {
  static constexpr bool kGeo = true;
  static constexpr int kAuxLoads = 0;
  static constexpr bool kMean = false;
  struct Fwd { double sum; };
  static __device__ __forceinline__ Fwd fwd_init(const PairIn &, int, int) { return Fwd{0.0}; }
  static __device__ __forceinline__ void fwd_tile(Fwd &st, const f16v &acc, float sAB, int c0, int cols, float (&gv)[16]) {
    float ts = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float d = acc[e] * sAB - gv[e];
      ts += c0 + pair_col(e) < cols ? pair_sl1(d) : 0.f;
    }
    st.sum += (double)ts;
  }
  // part (as doubles)[split][row]
  static __device__ __forceinline__ void fwd_store(const Fwd &st, bool write, size_t slot, float *part, float *) {
    const double v = st.sum + __shfl_xor(st.sum, 32);
    if (write) reinterpret_cast<double *>(part)[slot] = v;
  }
  static __device__ __forceinline__ void grad_own(float &v0, float &v1, const PairIn &, int, bool) { v0 = v1 = 0.f; }
  static __device__ __forceinline__ float grad_p(float s, float, float, float gv, int) { return fminf(fmaxf(s - gv, -1.f), 1.f); }
};

// the prediction: (best, col) = the largest score of the row and the streamed column it came from.  A strictly larger score
// wins, on equal scores the smaller column: numpy.argmax on the score row.  Forward only: no gradient members, so neither
// pair_grad_k nor pair_reduce_k is instantiated for it.  A NaN score never wins; col starts at 0, so it is always a column
// of the corner whatever the features hold.
struct PairMatch {
  static constexpr bool kGeo = false;
  struct Fwd { float best; int col; };
  static __device__ __forceinline__ bool better(float s, int c, float best, int col) { return s > best || (s == best && c < col); }
  static __device__ __forceinline__ Fwd fwd_init(const PairIn &, int, int) { return Fwd{-INFINITY, 0}; }
  static __device__ __forceinline__ void fwd_tile(Fwd &st, const f16v &acc, float sAB, int c0, int cols, float (&)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {                   // (pair_col ascends with e: inside a lane `>` alone is the tie rule)
      const int i = c0 + pair_col(e);
      const float s = acc[e] * sAB;
      if (i < cols && s > st.best) {
        st.best = s;
        st.col = i;
      }
    }
  }
  // part[split][row][4] = (best, column as a BIT PATTERN, -, -): moved and compared as an integer, never computed on.
  // The two half-waves hold disjoint, interleaved columns of the same row.
  static __device__ __forceinline__ void fwd_store(const Fwd &st, bool write, size_t slot, float *part, float *) {
    const float b2 = __shfl_xor(st.best, 32);
    const int c2 = __shfl_xor(st.col, 32);
    const bool other = better(b2, c2, st.best, st.col);
    if (write) *reinterpret_cast<f4 *>(part + slot * 4) = f4{other ? b2 : st.best, __int_as_float(other ? c2 : st.col), 0.f, 0.f};
  }
};

// grid (ceil(tiles_rows / 4), splits): rows x cols is the NA x NB corner (hard, soft, match) or the whole rectangle (sl1)
template <class Loss>
__global__ __launch_bounds__(kWG, 2) void pair_fwd_k(const unsigned short *__restrict__ RA, const unsigned short *__restrict__ RB, PairIn G,
                                                     int rows, int cols, int npadA, const unsigned *__restrict__ header,
                                                     float *__restrict__ part, float *__restrict__ part2) {
  __shared__ __attribute__((aligned(16))) unsigned short stage[2][kPairTile];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = lane & 31, kh = lane >> 5;
  const int tilesA = (rows + 31) / 32, tilesB = (cols + 31) / 32;
  const int mytile = blockIdx.x * 4 + wave;
  const int u = mytile * 32 + n;
  u4 own[8][2];
  pair_load_own(own, RA, mytile < tilesA ? mytile : tilesA - 1, lane);
  float upA, downA, upB, downB;
  pair_scales(header[0], upA, downA);
  pair_scales(header[1], upB, downB);
  const float sAB = downA * downB;
  const float *rowa = nullptr, *rowb = nullptr;
  bool vec = false, row_geo = false;
  if constexpr (Loss::kGeo) {
    const float *ga = G.base[0], *gb = G.base[1];
    vec = pair_geo_vec(ga, gb, G);
    row_geo = u < G.NA;
    rowa = ga + (int64_t)(row_geo ? u : 0) * G.ldA;
    rowb = gb + (int64_t)(row_geo ? u : 0) * G.ldB;
  }
  const int per = (tilesB + (int)gridDim.y - 1) / (int)gridDim.y;
  const int t0 = blockIdx.y * per, t1 = min(tilesB, t0 + per);
  typename Loss::Fwd st = Loss::fwd_init(G, u, rows);
  pair_wait_vmcnt<0>();                              // (own fragments, target: out of the way of the counted stage loads)
  if (t0 < t1) pair_stage<16>(RB + (size_t)t0 * kPairTile, stage[0], wave, lane);
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    if (t + 1 < t1) {
      pair_stage<16>(RB + (size_t)(t + 1) * kPairTile, stage[buf ^ 1], wave, lane);
      pair_wait_vmcnt<4>();                          // (a wave's share of a tile: 16 chunks / 4 waves)
    } else {
      pair_wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();                    // every wave's share of tile t has landed
    float gv[16];                                    // (issued before the products: the loads land while the matrix pipe works)
    if constexpr (Loss::kGeo) pair_geo_own_row(gv, rowa, rowb, row_geo, t * 32 + 4 * kh, G.NB, vec);
    const f16v acc = pair_tile(own, stage[buf], lane);
    Loss::fwd_tile(st, acc, sAB, t * 32 + 4 * kh, cols, gv);
    __builtin_amdgcn_s_barrier();                    // all waves are done with stage[buf] before tile t + 2 lands in it
  }
  Loss::fwd_store(st, kh == 0 && u < rows, (size_t)blockIdx.y * npadA + u, part, part2);
}

__global__ __launch_bounds__(kWG) void pair_combine_k(const float *__restrict__ part, int splits, int npadA, int NA, float *__restrict__ lse,
                                                      float *__restrict__ rowloss) {
  const int r = blockIdx.x * kWG + threadIdx.x;
  if (r >= NA) return;
  float mm = -INFINITY;
  for (int s = 0; s < splits; ++s) mm = fmaxf(mm, part[((size_t)s * npadA + r) * 4]);
  float ll = 0.f, tt = 0.f;
  for (int s = 0; s < splits; ++s) {
    const f4 v = *reinterpret_cast<const f4 *>(part + ((size_t)s * npadA + r) * 4);
    ll += v.x > -INFINITY ? v.y * __expf(v.x - mm) : 0.f;
    tt += v.z;
  }
  const float ls = mm + __logf(ll);
  lse[r] = ls;
  rowloss[r] = ls - tt;
}

// stats[r] = lse_S[r], stats[NA + r] = min_G[r] - log sum_j exp(-(G[r][j] - min_G[r]))  (softmin(G[r])[j] = exp(stats[NA + r] - G[r][j]))
__global__ __launch_bounds__(kWG) void pair_soft_combine_k(const float *__restrict__ part, const float *__restrict__ part2, int splits, int npadA,
                                                           int NA, float *__restrict__ stats, float *__restrict__ rowloss) {
  const int r = blockIdx.x * kWG + threadIdx.x;
  if (r >= NA) return;
  float mm = -INFINITY, gmm = INFINITY;
  for (int s = 0; s < splits; ++s) {
    mm = fmaxf(mm, part[((size_t)s * npadA + r) * 4]);
    gmm = fminf(gmm, part2[((size_t)s * npadA + r) * 4]);
  }
  float ll = 0.f, gl = 0.f, gts = 0.f;
  for (int s = 0; s < splits; ++s) {
    const f4 v = *reinterpret_cast<const f4 *>(part + ((size_t)s * npadA + r) * 4);
    const f4 w = *reinterpret_cast<const f4 *>(part2 + ((size_t)s * npadA + r) * 4);
    ll += v.x > -INFINITY ? v.y * expf(v.x - mm) : 0.f;
    const float c = w.x < INFINITY ? expf(gmm - w.x) : 0.f;
    gl += w.y * c;
    gts += w.z * c;
  }
  const float ls = mm + logf(ll);
  stats[r] = ls;
  stats[NA + r] = gmm - logf(gl);
  rowloss[r] = ls - gts / gl;
}
__global__ __launch_bounds__(kWG) void pair_sl1_combine_k(const double *__restrict__ part, int splits, int npadA, int rows, double *__restrict__ rowloss) {
  const int r = blockIdx.x * kWG + threadIdx.x;
  if (r >= rows) return;
  double v = 0.0;
  for (int s = 0; s < splits; ++s) v += part[(size_t)s * npadA + r];
  rowloss[r] = v;
}

// the winner over the ranges, in range order, by PairMatch::better (an empty range holds (-inf, 0), and column 0 belongs to
// range 0, so it never displaces one); err[r] = geo[truth[r]][col[r]] when geo is given, NaN where truth[r] is not a row of
// it: N scattered reads
__global__ __launch_bounds__(kWG) void pair_match_combine_k(const float *__restrict__ part, int splits, int npad, int N, int ncols,
                                                            int64_t *__restrict__ col, float *__restrict__ best,
                                                            const float *__restrict__ geo, int64_t ldg,
                                                            const int64_t *__restrict__ truth, float *__restrict__ err) {
  const int r = blockIdx.x * kWG + threadIdx.x;
  if (r >= N) return;
  f4 w = *reinterpret_cast<const f4 *>(part + (size_t)r * 4);
  for (int s = 1; s < splits; ++s) {
    const f4 v = *reinterpret_cast<const f4 *>(part + ((size_t)s * npad + r) * 4);
    if (PairMatch::better(v.x, __float_as_int(v.y), w.x, __float_as_int(w.y))) w = v;
  }
  const int c = __float_as_int(w.y);
  col[r] = c;
  best[r] = w.x;
  if (geo) {
    const int64_t t = truth[r];
    err[r] = (t >= 0 && t < ncols) ? geo[t * ldg + c] : __uint_as_float(0x7fc00000u);
  }
}

// grid: side A's nblk x splits workgroups, then side B's.  Own rows n of side A carry (v0, v1) themselves; for side B (own
// rows are COLUMNS of the score matrix) they belong to the streamed rows and come through the stage.
template <class Loss>
__global__ __launch_bounds__(kWG, 2) void pair_grad_k(PairGradSide A, PairGradSide B, PairIn G,
                                                      const unsigned *__restrict__ header) {
  extern __shared__ __attribute__((aligned(16))) unsigned short gstage[];      // 2 x (R tile | T tile | 4 x 256 B auxiliary)
  constexpr int kStage = 2 * kPairTile + 4 * 128;                              // halfs
  const bool ownA = blockIdx.x < (unsigned)(A.nblk * A.splits);
  const PairGradSide &S = ownA ? A : B;
  const int bid = ownA ? blockIdx.x : blockIdx.x - A.nblk * A.splits;
  const int blk = bid % S.nblk, split = bid / S.nblk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = lane & 31, kh = lane >> 5;
  const int tiles_own = (S.Nown + 31) / 32, tiles_oth = (S.Noth + 31) / 32;
  const int mytile = blk * 4 + wave;
  const int n0 = mytile * 32;
  const bool own_ok = n0 + n < S.Nown;
  u4 own[8][2];
  pair_load_own(own, S.Rown, mytile < tiles_own ? mytile : tiles_own - 1, lane);
  float upA, downA, upB, downB;
  pair_scales(header[0], upA, downA);
  pair_scales(header[1], upB, downB);
  const float sAB = downA * downB;
  const float *ga = nullptr, *gb = nullptr, *rowa = nullptr, *rowb = nullptr;
  bool vec = false, own_geo = false;
  if constexpr (Loss::kGeo) {
    ga = G.base[0];
    gb = G.base[1];
    vec = pair_geo_vec(ga, gb, G);
    own_geo = n0 + n < (ownA ? G.NA : G.NB);       // my own row / column lies inside the corner
    rowa = ga + (int64_t)((ownA && own_geo) ? n0 + n : 0) * G.ldA;
    rowb = gb + (int64_t)((ownA && own_geo) ? n0 + n : 0) * G.ldB;
  }
  float my0, my1;
  Loss::grad_own(my0, my1, G, n0 + n, ownA && own_ok);
  const int per = (tiles_oth + S.splits - 1) / S.splits;
  const int t0 = split * per, t1 = min(tiles_oth, t0 + per);
  f16v g[4];                                   // dOwn[n][32 f + (e&3) + 8 (e>>2) + 4 kh], f = 0..3
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int e = 0; e < 16; ++e) g[f][e] = 0.f;
  auto issue = [&](int t, int buf) {             // 8 + Loss::kAuxLoads loads per wave
    unsigned short *st = gstage + buf * kStage;
    pair_stage<16>(S.Roth + (size_t)t * kPairTile, st, wave, lane);
    pair_stage<16>(S.Toth + (size_t)t * kPairTile, st + kPairTile, wave, lane);
    if constexpr (Loss::kAuxLoads) {             // a private copy per wave
      const void *src = Loss::grad_aux(G, min(t * 32 + n, G.NA - 1), kh);
      __builtin_amdgcn_global_load_lds(static_cast<const unsigned *>(src), st + 2 * kPairTile + wave * 128, 4, 0, 0);
    }
  };
  pair_wait_vmcnt<0>();
  if (t0 < t1) issue(t0, 0);
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    if (t + 1 < t1) {
      issue(t + 1, buf ^ 1);
      pair_wait_vmcnt<8 + Loss::kAuxLoads>();
    } else {
      pair_wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    const unsigned short *st = gstage + buf * kStage;
    float gv[16];                                    // element 8 s2 + 4 jq + c <-> streamed row 16 s2 + 8 jq + 4 kh + c of the tile
    if constexpr (!Loss::kGeo) {
#pragma unroll
      for (int e = 0; e < 16; ++e) gv[e] = 0.f;
    } else {
      if (ownA) pair_geo_own_row(gv, rowa, rowb, own_geo, t * 32 + 4 * kh, G.NB, vec);
      else pair_geo_own_col(gv, ga, gb, G, own_geo, n0 + n, t * 32 + 4 * kh);
    }
    const f16v acc = pair_tile(own, st, lane);
    const float *aux = reinterpret_cast<const float *>(st + 2 * kPairTile + wave * 128);
    // P (times 2^14) for my own row and the 16 streamed rows this lane holds, as two fp16 pieces: slot (s2, j) = element 8 s2 + j
    u4 PH[2], PL[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float pv[8];
#pragma unroll
      for (int jq = 0; jq < 2; ++jq) {
        const int il = 16 * s2 + 8 * jq + 4 * kh;                       // streamed rows il .. il + 3 of the tile (elements 8 s2 + 4 jq + 0..3)
        f4 v0 = f4{my0, my0, my0, my0}, v1 = f4{my1, my1, my1, my1};
        if (Loss::kAuxLoads && !ownA) {
          v0 = *reinterpret_cast<const f4 *>(aux + il);
          v1 = *reinterpret_cast<const f4 *>(aux + 32 + il);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = 8 * s2 + 4 * jq + c;
          const int i = t * 32 + il + c;                                // streamed (other) row
          const float p = Loss::grad_p(acc[e] * sAB, v0[c], v1[c], gv[e], ownA ? i : n0 + n);
          pv[4 * jq + c] = (own_ok && i < S.Noth) ? p * 16384.f : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const h2v h = __builtin_convertvector(f2v{pv[2 * q], pv[2 * q + 1]}, h2v);
        const h2v lo = __builtin_convertvector(f2v{pv[2 * q] - (float)h.x, pv[2 * q + 1] - (float)h.y}, h2v);
        PH[s2][q] = __builtin_bit_cast(unsigned, h);
        PL[s2][q] = __builtin_bit_cast(unsigned, lo);
      }
    }
    // dOwn[n][kf] += sum_i P[n][i] Other[i][kf]: D2[kf][n], operand A = T tile (feature-major, pair_perm order), operand B = P
    const u4 *t4 = reinterpret_cast<const u4 *>(st + kPairTile) + lane;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u4 th[4], tl_[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        th[f] = t4[((f * 2 + s2) * 2) * 64];
        tl_[f] = t4[((f * 2 + s2) * 2 + 1) * 64];
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) g[f] = mfma_f16(tl_[f], PH[s2], g[f]);
#pragma unroll
      for (int f = 0; f < 4; ++f) g[f] = mfma_f16(th[f], PL[s2], g[f]);
#pragma unroll
      for (int f = 0; f < 4; ++f) g[f] = mfma_f16(th[f], PH[s2], g[f]);
    }
    __builtin_amdgcn_s_barrier();
  }
  if (mytile < tiles_own) {
    float *p = S.part + ((size_t)split * S.npad_own + n0 + n) * kPairKP;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f4 *>(p + 32 * f + 8 * q + 4 * kh) = f4{g[f][4 * q], g[f][4 * q + 1], g[f][4 * q + 2], g[f][4 * q + 3]};
  }
}

// dOwn[map[r]][k] = gloss (/ or ·) scale · 2^-14 down_other · sum_splits part[s][r][k] for r < Nown (label order; map = identity
// past nmap or where there is no map), 0 for the rows past Nown; one thread per (row, 4 features) of a side (blockIdx.y).
// MEAN: gloss / scale, the hard-target loss's division by NA (gloss · (1 / NA) rounds differently); else gloss · scale.
template <bool MEAN>
__global__ __launch_bounds__(kWG) void pair_reduce_k(PairGradSide A, PairGradSide B, float *__restrict__ dFA, int64_t ldda, int rowsA,
                                                     float *__restrict__ dFB, int64_t lddb, int rowsB, int K,
                                                     const float *__restrict__ gloss, const unsigned *__restrict__ header, float scale,
                                                     const int64_t *__restrict__ mapA, int nmapA, const int64_t *__restrict__ mapB, int nmapB) {
  const bool sb = blockIdx.y != 0;
  const PairGradSide &S = sb ? B : A;
  float *d = sb ? dFB : dFA;
  const int64_t ldd = sb ? lddb : ldda;
  const int rows = sb ? rowsB : rowsA;
  const int64_t *map = sb ? mapB : mapA;
  const int nmap = sb ? nmapB : nmapA;
  const int64_t id = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const int r = (int)(id >> 5), k = (int)(id & 31) * 4;
  if (r >= rows || k >= K) return;
  f4 v = f4{0.f, 0.f, 0.f, 0.f};
  if (r < S.Nown) {
    for (int s = 0; s < S.splits; ++s) v += *reinterpret_cast<const f4 *>(S.part + ((size_t)s * S.npad_own + r) * kPairKP + k);
    float up, down;
    pair_scales(header[sb ? 0 : 1], up, down);      // the OTHER side's features were scaled up
    v *= (MEAN ? gloss[0] / scale : gloss[0] * scale) * (1.f / 16384.f) * down;
  }
  const int64_t dst = (map && r < nmap) ? map[r] : r;
  float *o = d + dst * ldd + k;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (k + c < K) o[c] = v[c];
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

struct PairWs {
  int pa, pb;
  unsigned *header;
  unsigned short *RA, *TA, *RB, *TB;
  float *lse_part, *gradA, *gradB;
  float *part2;                  // the soft-min partials of `cel`: past `bytes`, inside `loss_bytes`
  size_t bytes, loss_bytes;      // sn_pair_fused_workspace_bytes, sn_pair_loss_workspace_bytes
};
PairWs pair_ws(void *workspace, int64_t rowsA, int64_t rowsB) {
  PairWs w;
  w.pa = (int)((rowsA + 31) / 32 * 32);
  w.pb = (int)((rowsB + 31) / 32 * 32);
  char *p = static_cast<char *>(workspace);
  w.header = reinterpret_cast<unsigned *>(p);
  p += kPairHeader;
  const size_t fa = (size_t)w.pa * kPairKP * 2 * sizeof(unsigned short), fb = (size_t)w.pb * kPairKP * 2 * sizeof(unsigned short);
  w.RA = reinterpret_cast<unsigned short *>(p); p += fa;
  w.TA = reinterpret_cast<unsigned short *>(p); p += fa;
  w.RB = reinterpret_cast<unsigned short *>(p); p += fb;
  w.TB = reinterpret_cast<unsigned short *>(p); p += fb;
  w.lse_part = reinterpret_cast<float *>(p); p += (size_t)kPairMaxLseSplits * w.pa * 4 * sizeof(float);
  w.gradA = reinterpret_cast<float *>(p); p += (size_t)kPairMaxGradSplits * w.pa * kPairKP * sizeof(float);
  w.gradB = reinterpret_cast<float *>(p); p += (size_t)kPairMaxGradSplits * w.pb * kPairKP * sizeof(float);
  w.bytes = (size_t)(p - static_cast<char *>(workspace));
  w.part2 = reinterpret_cast<float *>(p); p += (size_t)kPairMaxLseSplits * w.pa * 4 * sizeof(float);
  w.loss_bytes = (size_t)(p - static_cast<char *>(workspace));
  return w;
}

// sn_pair_match_f32: header | RA | RB | partials of the rows of A | partials of the rows of B — no T, no gradient partials.
// `ab` scores the rows of A against the streamed rows of B; `ba` is the same memory with the sides exchanged.
struct PairMatchWs {
  PairWs ab, ba;
  size_t bytes;
};
PairMatchWs pair_match_ws(void *workspace, int64_t rowsA, int64_t rowsB) {
  PairWs w{};
  w.pa = (int)((rowsA + 31) / 32 * 32);
  w.pb = (int)((rowsB + 31) / 32 * 32);
  char *p = static_cast<char *>(workspace);
  w.header = reinterpret_cast<unsigned *>(p);
  p += kPairHeader;
  w.RA = reinterpret_cast<unsigned short *>(p); p += (size_t)w.pa * kPairKP * 2 * sizeof(unsigned short);
  w.RB = reinterpret_cast<unsigned short *>(p); p += (size_t)w.pb * kPairKP * 2 * sizeof(unsigned short);
  w.lse_part = reinterpret_cast<float *>(p); p += (size_t)kPairMaxLseSplits * w.pa * 4 * sizeof(float);
  PairWs x = w;
  x.pa = w.pb; x.pb = w.pa;
  x.RA = w.RB; x.RB = w.RA;
  x.lse_part = reinterpret_cast<float *>(p); p += (size_t)kPairMaxLseSplits * w.pb * 4 * sizeof(float);
  return PairMatchWs{w, x, (size_t)(p - static_cast<char *>(workspace))};
}

// the checks `cel` and `sl1` share
int pair_loss_check(int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, int64_t ldgA, int64_t ldgB) {
  if (NA < 1 || NB < 1 || rowsA < NA || rowsB < NB || K < 1 || ldgA < NB || ldgB < NB) return SN_E_SHAPE;
  if (K > kPairKP) return SN_E_UNSUPPORTED;
  if (rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return SN_E_RANGE;
  return SN_OK;
}

// features -> fragment order in the workspace: header fill, absolute maxima, split (MAP, the losses in label order: rows
// [0, NA) / [0, NB) taken through the maps, where there are any)
template <bool MAP, bool WITH_T = true>
int pair_split(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *mapA, const int64_t *mapB, int64_t NA,
               int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, const PairWs &w, hipStream_t s) {
  hipError_t e = sn_internal_fill(w.header, 0, kPairHeader, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pair_maxabs_k, dim3((unsigned)std::min<int64_t>(1024, (std::max(rowsA, rowsB) * K + 4 * kWG - 1) / (4 * kWG)), 2), dim3(kWG), 0, s, FA, lda, (int)rowsA, FB, ldb, (int)rowsB, (int)K, w.header);
  const int64_t quads = (int64_t)std::max(w.pa, w.pb) * 32;
  hipLaunchKernelGGL((pair_split_k<MAP, WITH_T>), dim3((unsigned)((quads + kWG - 1) / kWG), 2), dim3(kWG), 0, s, FA, lda, (int)rowsA, w.pa, w.RA, w.TA, FB,
                     ldb, (int)rowsB, w.pb, w.RB, w.TB, (int)K, w.header, mapA, (int)NA, mapB, (int)NB);
  return SN_OK;
}

// the forward kernel over rows x cols; returns the number of ranges per row block (the combine kernels' `splits`)
// (w.part2 lies past a workspace sized by sn_pair_fused_workspace_bytes: only PairSoft::fwd_store writes through it, `dcel` never)
template <class Loss>
int pair_fwd_launch(PairIn G, int64_t rows, int64_t cols, const PairWs &w, hipStream_t s) {
  const int tilesA = (int)((rows + 31) / 32), tilesB = (int)((cols + 31) / 32);
  const int nblk = (tilesA + 3) / 4;
  const int splits = std::max(1, std::min({kPairMaxLseSplits, 512 / nblk, tilesB}));
  hipLaunchKernelGGL((pair_fwd_k<Loss>), dim3((unsigned)nblk, (unsigned)splits), dim3(kWG), 0, s, w.RA, w.RB, G, (int)rows, (int)cols, w.pa,
                     w.header, w.lse_part, w.part2);
  return splits;
}

// both gradients over Nrows x Ncols and their reduction into dFA / dFB (rowsA / rowsB rows; `scale` as Loss::kMean says)
template <class Loss>
int pair_bwd_launch(PairIn G, const int64_t *mapA, const int64_t *mapB, const float *gloss, int64_t Nrows, int64_t Ncols,
                    int64_t rowsA, int64_t rowsB, int32_t K, float scale, float *dFA, int64_t ldda, float *dFB, int64_t lddb,
                    const PairWs &w, hipStream_t s) {
  const int tilesA = (int)((Nrows + 31) / 32), tilesB = (int)((Ncols + 31) / 32);
  PairGradSide A{w.RA, w.RB, w.TB, w.gradA, (int)Nrows, (int)Ncols, w.pa, (tilesA + 3) / 4, 1};
  PairGradSide B{w.RB, w.RA, w.TA, w.gradB, (int)Ncols, (int)Nrows, w.pb, (tilesB + 3) / 4, 1};
  const int want = std::max(1, 512 / (A.nblk + B.nblk));
  A.splits = std::max(1, std::min({kPairMaxGradSplits, want, tilesB}));
  B.splits = std::max(1, std::min({kPairMaxGradSplits, want, tilesA}));
  constexpr size_t lds = (size_t)2 * (2 * kPairTile + 4 * 128) * sizeof(unsigned short);
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void *>(pair_grad_k<Loss>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) return (int)attr;
  hipLaunchKernelGGL((pair_grad_k<Loss>), dim3((unsigned)(A.nblk * A.splits + B.nblk * B.splits)), dim3(kWG), lds, s, A, B, G, w.header);
  const int64_t quads = (int64_t)std::max(rowsA, rowsB) * 32;
  hipLaunchKernelGGL((pair_reduce_k<Loss::kMean>), dim3((unsigned)((quads + kWG - 1) / kWG), 2), dim3(kWG), 0, s, A, B, dFA, ldda, (int)rowsA, dFB, lddb,
                     (int)rowsB, (int)K, gloss, w.header, scale, mapA, G.NA, mapB, G.NB);
  return launch_status();
}

}  // namespace

extern "C" {

size_t sn_pair_fused_workspace_bytes(int64_t rowsA, int64_t rowsB) {
  if (rowsA < 0 || rowsB < 0 || rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return 0;
  return pair_ws(nullptr, rowsA, rowsB).bytes;
}

size_t sn_pair_loss_workspace_bytes(int64_t rowsA, int64_t rowsB) {
  if (rowsA < 0 || rowsB < 0 || rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return 0;
  return pair_ws(nullptr, rowsA, rowsB).loss_bytes;
}

int sn_pair_fused_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *target, int64_t NA, int64_t NB,
                          int64_t rowsA, int64_t rowsB, int32_t K, float *lse, float *rowloss, void *workspace,
                          size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (NA < 1 || NB < 1 || rowsA < NA || rowsB < NB || K < 1 || lda < K || ldb < K) return SN_E_SHAPE;
  if (K > kPairKP) return SN_E_UNSUPPORTED;
  if (rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return SN_E_RANGE;
  if (!FA || !FB || !target || !workspace || !lse || !rowloss) return SN_E_NULL;
  if (!aligned16(workspace)) return SN_E_ALIGN;
  if (workspace_bytes < sn_pair_fused_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairWs w = pair_ws(workspace, rowsA, rowsB);
  if (int st = pair_split<false>(FA, lda, FB, ldb, nullptr, nullptr, NA, NB, rowsA, rowsB, K, w, s)) return st;
  const int splits = pair_fwd_launch<PairHard>(PairIn{nullptr, 0, 0, (int)NA, (int)NB, nullptr, target}, NA, NB, w, s);
  hipLaunchKernelGGL(pair_combine_k, dim3((unsigned)((NA + kWG - 1) / kWG)), dim3(kWG), 0, s, w.lse_part, splits, w.pa, (int)NA, lse, rowloss);
  return launch_status();
}

int sn_pair_fused_bwd_f32(const int64_t *target, const float *lse, const float *gloss, int64_t NA, int64_t NB, int64_t rowsA,
                          int64_t rowsB, int32_t K, float *dFA, int64_t ldda, float *dFB, int64_t lddb, void *workspace,
                          size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (NA < 1 || NB < 1 || rowsA < NA || rowsB < NB || K < 1 || K > kPairKP || ldda < K || lddb < K) return SN_E_SHAPE;
  if (rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return SN_E_RANGE;
  if (!target || !lse || !gloss || !dFA || !dFB || !workspace) return SN_E_NULL;
  if (workspace_bytes < sn_pair_fused_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  return pair_bwd_launch<PairHard>(PairIn{nullptr, 0, 0, (int)NA, (int)NB, lse, target}, nullptr, nullptr, gloss, NA, NB, rowsA, rowsB, K,
                                   (float)NA, dFA, ldda, dFB, lddb, pair_ws(workspace, rowsA, rowsB), static_cast<hipStream_t>(stream));
}

int sn_pair_soft_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *mapA, const int64_t *mapB,
                         const float *const *geo, int64_t ldgA, int64_t ldgB, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB,
                         int32_t K, float *stats, float *rowloss, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (int st = pair_loss_check(NA, NB, rowsA, rowsB, K, ldgA, ldgB)) return st;
  if (lda < K || ldb < K) return SN_E_SHAPE;
  if (!FA || !FB || !geo || !workspace || !stats || !rowloss) return SN_E_NULL;
  if (!aligned16(workspace)) return SN_E_ALIGN;
  if (workspace_bytes < sn_pair_loss_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairWs w = pair_ws(workspace, rowsA, rowsB);
  if (int st = pair_split<true>(FA, lda, FB, ldb, mapA, mapB, NA, NB, rowsA, rowsB, K, w, s)) return st;
  const int splits = pair_fwd_launch<PairSoft>(PairIn{geo, ldgA, ldgB, (int)NA, (int)NB, nullptr, nullptr}, NA, NB, w, s);
  hipLaunchKernelGGL(pair_soft_combine_k, dim3((unsigned)((NA + kWG - 1) / kWG)), dim3(kWG), 0, s, w.lse_part, w.part2, splits, w.pa, (int)NA,
                     stats, rowloss);
  return launch_status();
}

int sn_pair_soft_bwd_f32(const int64_t *mapA, const int64_t *mapB, const float *const *geo, int64_t ldgA, int64_t ldgB, const float *stats,
                         const float *gloss, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, float *dFA, int64_t ldda,
                         float *dFB, int64_t lddb, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (int st = pair_loss_check(NA, NB, rowsA, rowsB, K, ldgA, ldgB)) return st;
  if (ldda < K || lddb < K) return SN_E_SHAPE;
  if (!geo || !stats || !gloss || !dFA || !dFB || !workspace) return SN_E_NULL;
  if (workspace_bytes < sn_pair_loss_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  return pair_bwd_launch<PairSoft>(PairIn{geo, ldgA, ldgB, (int)NA, (int)NB, stats, nullptr}, mapA, mapB, gloss, NA, NB,
                                   rowsA, rowsB, K, 1.f, dFA, ldda, dFB, lddb, pair_ws(workspace, rowsA, rowsB),
                                   static_cast<hipStream_t>(stream));
}

int sn_pair_sl1_fwd_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, const int64_t *mapA, const int64_t *mapB,
                        const float *const *geo, int64_t ldgA, int64_t ldgB, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB,
                        int32_t K, double *rowloss, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (int st = pair_loss_check(NA, NB, rowsA, rowsB, K, ldgA, ldgB)) return st;
  if (lda < K || ldb < K) return SN_E_SHAPE;
  if (!FA || !FB || !geo || !workspace || !rowloss) return SN_E_NULL;
  if (!aligned16(workspace)) return SN_E_ALIGN;
  if (workspace_bytes < sn_pair_loss_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairWs w = pair_ws(workspace, rowsA, rowsB);
  if (int st = pair_split<true>(FA, lda, FB, ldb, mapA, mapB, NA, NB, rowsA, rowsB, K, w, s)) return st;
  const int splits = pair_fwd_launch<PairSl1>(PairIn{geo, ldgA, ldgB, (int)NA, (int)NB, nullptr, nullptr}, rowsA, rowsB, w, s);
  hipLaunchKernelGGL(pair_sl1_combine_k, dim3((unsigned)((rowsA + kWG - 1) / kWG)), dim3(kWG), 0, s, reinterpret_cast<const double *>(w.lse_part),
                     splits, w.pa, (int)rowsA, rowloss);
  return launch_status();
}

int sn_pair_sl1_bwd_f32(const int64_t *mapA, const int64_t *mapB, const float *const *geo, int64_t ldgA, int64_t ldgB, const float *gloss,
                        int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB, int32_t K, float *dFA, int64_t ldda, float *dFB, int64_t lddb,
                        void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (int st = pair_loss_check(NA, NB, rowsA, rowsB, K, ldgA, ldgB)) return st;
  if (ldda < K || lddb < K) return SN_E_SHAPE;
  if (!geo || !gloss || !dFA || !dFB || !workspace) return SN_E_NULL;
  if (workspace_bytes < sn_pair_loss_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  const float mul = (float)(1.0 / ((double)rowsA * (double)rowsB));
  return pair_bwd_launch<PairSl1>(PairIn{geo, ldgA, ldgB, (int)NA, (int)NB, nullptr, nullptr}, mapA, mapB, gloss, rowsA, rowsB, rowsA,
                                  rowsB, K, mul, dFA, ldda, dFB, lddb, pair_ws(workspace, rowsA, rowsB), static_cast<hipStream_t>(stream));
}

size_t sn_pair_match_workspace_bytes(int64_t rowsA, int64_t rowsB) {
  if (rowsA < 0 || rowsB < 0 || rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return 0;
  return pair_match_ws(nullptr, rowsA, rowsB).bytes;
}

int sn_pair_match_f32(const float *FA, int64_t lda, const float *FB, int64_t ldb, int64_t NA, int64_t NB, int64_t rowsA, int64_t rowsB,
                      int32_t K, int64_t *colA, float *bestA, int64_t *rowB, float *bestB, const float *geoB, int64_t ldgB,
                      const int64_t *truthA, float *errA, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (NA < 1 || NB < 1 || rowsA < NA || rowsB < NB || K < 1 || lda < K || ldb < K || (geoB && ldgB < NB)) return SN_E_SHAPE;
  if (K > kPairKP) return SN_E_UNSUPPORTED;
  if (rowsA > INT_MAX - 64 || rowsB > INT_MAX - 64) return SN_E_RANGE;
  if (!FA || !FB || !colA || !bestA || !workspace || !rowB != !bestB) return SN_E_NULL;
  if (!geoB != !truthA || !geoB != !errA) return SN_E_NULL;
  if (!aligned16(workspace)) return SN_E_ALIGN;
  if (workspace_bytes < sn_pair_match_workspace_bytes(rowsA, rowsB)) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairMatchWs w = pair_match_ws(workspace, rowsA, rowsB);
  // (the scales and the split see the scored rows only: what the padding of the batch holds cannot move a prediction)
  if (int st = pair_split<false, false>(FA, lda, FB, ldb, nullptr, nullptr, NA, NB, NA, NB, K, w.ab, s)) return st;
  const PairIn none{nullptr, 0, 0, (int)NA, (int)NB, nullptr, nullptr};
  int splits = pair_fwd_launch<PairMatch>(none, NA, NB, w.ab, s);
  hipLaunchKernelGGL(pair_match_combine_k, dim3((unsigned)((NA + kWG - 1) / kWG)), dim3(kWG), 0, s, w.ab.lse_part, splits, w.ab.pa, (int)NA,
                     (int)NB, colA, bestA, geoB, ldgB, truthA, errA);
  if (rowB) {                   // the column arg-max: the same kernel with the sides exchanged
    splits = pair_fwd_launch<PairMatch>(none, NB, NA, w.ba, s);
    hipLaunchKernelGGL(pair_match_combine_k, dim3((unsigned)((NB + kWG - 1) / kWG)), dim3(kWG), 0, s, w.ba.lse_part, splits, w.ba.pa, (int)NB,
                       (int)NA, rowB, bestB, static_cast<const float *>(nullptr), (int64_t)0, static_cast<const int64_t *>(nullptr),
                       static_cast<float *>(nullptr));
  }
  return launch_status();
}

}  // extern "C"
