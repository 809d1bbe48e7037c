// sn_delaunay.hip — batched 2-D Delaunay triangulation on an integer lattice, Bridson Poisson-disc sampling in integers and the
// Mesh-MNIST maker built on the two (gfx950).  One workgroup per point set / image, all state in LDS.  Every predicate is an exact
// integer: orientation in int64, in-circle in __int128.  The definition is in include/sn_spmm.h ("Lattice Delaunay and the
// Mesh-MNIST maker"); the host statements are mesh_ops.delaunay_2d, poisson_disc and mesh_digits.
// Every loop below has a bound that follows from the input size; nothing waits on a condition without a counter.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_spmm.h"

namespace {

constexpr int kN = SN_DELAUNAY_MAX_POINTS;        // points of one set, cells of one sampler grid
constexpr int kSmall = 512;                       // capacity of the small variants (N below: 512 or 1024 points, 2 N faces)
constexpr int kWG = 256;
constexpr int kCand = 30, kRetry = 32;            // Bridson's k and the annulus retries
constexpr int64_t kBias = (int64_t)1 << 24;       // coordinates are stored biased: sort keys are unsigned
static_assert(kN <= 1024, "face keys pack three 10-bit vertex indices; faces and vertices are held as int16");

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SN_OK : (int)e;
}

// ---- state of one triangulation of at most N points: 50 KiB for N = 1024, 25 KiB for N = 512 ----------------------------------
template <int N>
struct DtState {
  static constexpr int kPoints = N, kFaces = 2 * N;
  unsigned long long key[N];   // sorted points: (x + 2^24) << 32 | (y + 2^24)
  int claim[2 * N];              // flip rounds: the smallest bad edge id that wants this face;  afterwards: the canonical face keys
  short perm[N];                // sorted position -> input index
  short fv[2 * N][3];            // face vertices (sorted positions), counter-clockwise
  short fa[2 * N][3];            // fa[f][s]: the face across side s = (fv[f][s], fv[f][s + 1]), -1 on the hull
  short hnext[N], hprev[N];     // the hull as a ring, counter-clockwise
  short hface[N];               // the face whose side v -> hnext[v] is the hull edge that starts at v
  unsigned char chk[2 * N];      // bit 0: an edge of this face may be bad in this round;  bit 1: the same for the next round
  int nf, status, flips, cocircular, rounds, bad;
};

__device__ __forceinline__ int64_t key_x(unsigned long long k) { return (int64_t)(k >> 32) - kBias; }
__device__ __forceinline__ int64_t key_y(unsigned long long k) { return (int64_t)(k & 0xffffffffull) - kBias; }

__device__ __forceinline__ int64_t orient_keys(unsigned long long a, unsigned long long b, unsigned long long c) {
  const int64_t ax = key_x(a), ay = key_y(a);
  return (key_x(b) - ax) * (key_y(c) - ay) - (key_y(b) - ay) * (key_x(c) - ax);      // |differences| < 2^25: fits
}

// sign of the in-circle determinant of differences, exact (at most 104 bits)
__device__ __forceinline__ int incircle_keys(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
  const int64_t dx = key_x(d), dy = key_y(d);
  const int64_t adx = key_x(a) - dx, ady = key_y(a) - dy, bdx = key_x(b) - dx, bdy = key_y(b) - dy;
  const int64_t cdx = key_x(c) - dx, cdy = key_y(c) - dy;
  const int64_t ad = adx * adx + ady * ady, bd = bdx * bdx + bdy * bdy, cd = cdx * cdx + cdy * cdy;
  const __int128 det = (__int128)ad * (bdx * cdy - bdy * cdx) - (__int128)bd * (adx * cdy - ady * cdx) +
                       (__int128)cd * (adx * bdy - ady * bdx);
  return det > 0 ? 1 : (det < 0 ? -1 : 0);
}

// The priority of bad edge e in a round: hashed, so that the winners of a round are spread over the mesh (an id order would
// serialise the rounds along chains of neighbours), unique through its low 13 bits, a function of (e, round) alone.
__device__ __forceinline__ int edge_priority(int e, int round) {
  unsigned h = (unsigned)e * 2654435761u + (unsigned)round * 0x9E3779B1u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  return (int)((h >> 14) << 13) | e;                       // 18 + 13 bits, e < 3 * 2048 < 2^13
}

template <class DT>
__device__ __forceinline__ int side_of(const DT &S, int f, int g) {     // the side of f that faces g (0 when none does)
  return S.fa[f][0] == g ? 0 : (S.fa[f][1] == g ? 1 : 2);
}

// Single lane: one new face (b, a, p) over the hull edge a -> b, glued to the face behind the edge.
template <class DT>
__device__ __forceinline__ int sweep_add_face(DT &S, int a, int b, int p) {
  const int t = S.nf++;
  S.fv[t][0] = (short)b; S.fv[t][1] = (short)a; S.fv[t][2] = (short)p;
  const int in = S.hface[a];
  S.fa[t][0] = (short)in; S.fa[t][1] = -1; S.fa[t][2] = -1;
  for (int s = 0; s < 3; ++s)
    if (S.fv[in][s] == a && S.fv[in][s == 2 ? 0 : s + 1] == b) S.fa[in][s] = (short)t;
  return t;
}

// The sweep over the sorted points (lane 0 only): a collinear prefix, its fan, then one point after the other from outside.
template <class DT>
__device__ void dt_sweep(DT &S, int n) {
  int k = 2;
  while (k < n && orient_keys(S.key[0], S.key[1], S.key[k]) == 0) ++k;          // at most n steps
  if (k == n) { S.status = SN_DT_DEGENERATE; return; }
  const bool left = orient_keys(S.key[0], S.key[1], S.key[k]) > 0;
  for (int i = 0; i + 1 < k; ++i) {                                              // the fan (i, i + 1, k) or (i + 1, i, k)
    const int t = S.nf++;
    S.fv[t][0] = (short)(left ? i : i + 1); S.fv[t][1] = (short)(left ? i + 1 : i); S.fv[t][2] = (short)k;
    // sides: 0 = the chain edge (hull), 1 and 2 = the spokes
    S.fa[t][0] = -1;
    S.fa[t][left ? 1 : 2] = (short)(i + 2 < k ? t + 1 : -1);                     // spoke at i + 1: shared with the next fan face
    S.fa[t][left ? 2 : 1] = (short)(i > 0 ? t - 1 : -1);                         // spoke at i: shared with the previous one
  }
  // hull ring: left: 0 -> 1 -> .. -> k-1 -> k -> 0;  right: k-1 -> .. -> 0 -> k -> k-1
  for (int i = 0; i + 1 < k; ++i) {
    const int a = left ? i : i + 1, b = left ? i + 1 : i;
    S.hnext[a] = (short)b; S.hprev[b] = (short)a; S.hface[a] = (short)i;
  }
  const int tail = left ? k - 1 : 0, head = left ? 0 : k - 1;
  S.hnext[tail] = (short)k; S.hprev[k] = (short)tail; S.hface[tail] = (short)(left ? k - 2 : 0);
  S.hnext[k] = (short)head; S.hprev[head] = (short)k; S.hface[k] = (short)(left ? 0 : k - 2);
  for (int p = k + 1; p < n; ++p) {
    // p - 1 is the largest point so far, a hull vertex that p sees; the hull edges p sees strictly are one chain through it
    const unsigned long long kp = S.key[p];
    int first = p - 1, last = p - 1;
    for (int it = 0; it < p; ++it) {                                             // the hull has at most p vertices
      const int nx = S.hnext[last];
      if (!(orient_keys(S.key[last], S.key[nx], kp) < 0)) break;
      last = nx;
    }
    for (int it = 0; it < p; ++it) {
      const int pv = S.hprev[first];
      if (!(orient_keys(S.key[pv], S.key[first], kp) < 0)) break;
      first = pv;
    }
    if (first == last) { S.status |= SN_DT_INTERNAL; return; }   // never: p lies strictly outside
    int prev_t = -1, a = first;
    for (int it = 0; it < p && a != last; ++it) {
      const int b = S.hnext[a];
      if (S.nf >= DT::kFaces) { S.status |= SN_DT_INTERNAL; return; }
      const int t = sweep_add_face(S, a, b, p);
      if (prev_t >= 0) { S.fa[t][1] = (short)prev_t; S.fa[prev_t][2] = (short)t; }   // side (a, p) of t = side (p, a) of prev_t
      if (a == first) S.hface[first] = (short)t;                                 // first -> p is side 1 of this face
      prev_t = t;
      a = b;
    }
    S.hface[p] = (short)prev_t;                                                  // p -> last is side 2 of the last face
    S.hnext[first] = (short)p; S.hprev[p] = (short)first;
    S.hnext[p] = (short)last; S.hprev[last] = (short)p;
  }
}

// bitonic sort of m = 2^k (key, perm) pairs, whole workgroup
template <class DT>
__device__ void sort_points(DT &S, int m) {
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < m; i += kWG) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = S.key[i], b = S.key[l];
          if ((a > b) == ((i & k) == 0)) {
            S.key[i] = b; S.key[l] = a;
            const short t = S.perm[i]; S.perm[i] = S.perm[l]; S.perm[l] = t;
          }
        }
      }
      __syncthreads();
    }
}

template <class DT>
__device__ void sort_claims(DT &S, int m) {
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < m; i += kWG) {
        const int l = i ^ j;
        if (l > i) {
          const int a = S.claim[i], b = S.claim[l];
          if ((a > b) == ((i & k) == 0)) { S.claim[i] = b; S.claim[l] = a; }
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int m = 2;
  while (m < n) m <<= 1;                     // n <= 2048: at most 11 steps
  return m;
}

// The triangulation of n points (xs[i * stride], ys[i * stride]); whole workgroup, uniform control flow.  On return S.status,
// S.nf, S.flips, S.cocircular, S.rounds are set; with status 0 S.fv holds the faces in sorted positions, S.perm the way back.
template <class DT>
__device__ void dt_run(DT &S, const int *xs, const int *ys, int stride, int n, int nmax, int max_rounds) {
  const int tid = threadIdx.x;
  if (tid == 0) { S.nf = 0; S.status = 0; S.flips = 0; S.cocircular = 0; S.rounds = 0; S.bad = 0; }
  __syncthreads();
  if (n > DT::kPoints || n > nmax) {
    if (tid == 0) S.status = SN_DT_TOO_LARGE;
    __syncthreads();
    return;
  }
  if (n < 0) n = 0;
  const int m = pow2_at_least(n);
  for (int i = tid; i < m; i += kWG) {
    unsigned long long k = ~0ull;
    if (i < n) {
      const int64_t x = xs[(int64_t)i * stride], y = ys[(int64_t)i * stride];
      if (x <= -kBias || x >= kBias || y <= -kBias || y >= kBias) {
        atomicOr(&S.status, SN_DT_RANGE);
        k = 0;
      } else {
        k = ((unsigned long long)(x + kBias) << 32) | (unsigned long long)(y + kBias);
      }
    }
    S.key[i] = k;
    S.perm[i] = (short)i;
  }
  __syncthreads();
  if (S.status == 0 && n < 3) {
    __syncthreads();
    if (tid == 0) S.status = SN_DT_DEGENERATE;
  }
  __syncthreads();
  if (S.status) return;
  sort_points(S, m);
  for (int i = tid; i + 1 < n; i += kWG)
    if (S.key[i] == S.key[i + 1]) atomicOr(&S.status, SN_DT_DUPLICATE);
  __syncthreads();
  if (S.status) return;
  if (tid == 0) dt_sweep(S, n);
  __syncthreads();
  if (S.status) return;
  const int nf = S.nf;
  // Lawson flips in claim-then-flip rounds.  A bad edge e = 3 f + s (f the smaller of its two faces) asks for its two faces and
  // their four outer neighbours with atomicMin of its priority; it flips when it holds all of them, so two flips of one round
  // touch disjoint faces and the bad edge of the smallest priority always flips.  An edge is looked at only when one of its
  // faces is marked: every face at first, then the faces of the edges found bad and the faces a flip rewrote — an edge changes
  // its value only when one of its faces is rewritten.  The schedule is a function of the input alone.
  for (int f = tid; f < nf; f += kWG) S.chk[f] = 2;
  __syncthreads();
  for (int round = 0; round < max_rounds; ++round) {
    for (int f = tid; f < nf; f += kWG) { S.claim[f] = INT_MAX; S.chk[f] >>= 1; }
    if (tid == 0) S.bad = 0;
    __syncthreads();
    for (int e = tid; e < 3 * nf; e += kWG) {
      const int f = e / 3, s = e - 3 * f, g = S.fa[f][s];
      if (g <= f || !((S.chk[f] | S.chk[g]) & 1)) continue;
      const int s1 = s == 2 ? 0 : s + 1, s2 = s1 == 2 ? 0 : s1 + 1;
      const int t = side_of(S, g, f), t2 = t == 0 ? 2 : t - 1;
      if (incircle_keys(S.key[S.fv[f][s]], S.key[S.fv[f][s1]], S.key[S.fv[f][s2]], S.key[S.fv[g][t2]]) <= 0) continue;
      S.bad = 1;
      S.chk[f] |= 2; S.chk[g] |= 2;                        // (every writer of this phase sets bit 1 and leaves bit 0)
      const int t1 = t == 2 ? 0 : t + 1, pr = edge_priority(e, round);
      const int nb[6] = {f, g, S.fa[f][s1], S.fa[f][s2], S.fa[g][t1], S.fa[g][t2]};
      for (int q = 0; q < 6; ++q)
        if (nb[q] >= 0) atomicMin(&S.claim[nb[q]], pr);
    }
    __syncthreads();
    if (!S.bad) break;                                     // uniform: read after the barrier, written before it
    for (int e = tid; e < 3 * nf; e += kWG) {
      const int f = e / 3, s = e - 3 * f;
      const int pr = edge_priority(e, round);
      if (S.claim[f] != pr) continue;                      // only the bad edges around f wrote their priority there
      const int g = S.fa[f][s];
      if (g <= f || S.claim[g] != pr) continue;                      // g is someone else's: it may be changing under this lane
      const int s1 = s == 2 ? 0 : s + 1, s2 = s1 == 2 ? 0 : s1 + 1;
      const int t = side_of(S, g, f), t1 = t == 2 ? 0 : t + 1, t2 = t1 == 2 ? 0 : t1 + 1;
      const int n_vw = S.fa[f][s1], n_wu = S.fa[f][s2], n_uz = S.fa[g][t1], n_zv = S.fa[g][t2];
      if ((n_vw >= 0 && S.claim[n_vw] != pr) || (n_wu >= 0 && S.claim[n_wu] != pr) ||
          (n_uz >= 0 && S.claim[n_uz] != pr) || (n_zv >= 0 && S.claim[n_zv] != pr))
        continue;
      const short u = S.fv[f][s], v = S.fv[f][s1], w = S.fv[f][s2], z = S.fv[g][t2];
      // f = (u, z, w), g = (z, v, w)
      S.fv[f][0] = u; S.fv[f][1] = z; S.fv[f][2] = w;
      S.fa[f][0] = (short)n_uz; S.fa[f][1] = (short)g; S.fa[f][2] = (short)n_wu;
      S.fv[g][0] = z; S.fv[g][1] = v; S.fv[g][2] = w;
      S.fa[g][0] = (short)n_zv; S.fa[g][1] = (short)n_vw; S.fa[g][2] = (short)f;
      if (n_uz >= 0) S.fa[n_uz][side_of(S, n_uz, g)] = (short)f;
      if (n_vw >= 0) S.fa[n_vw][side_of(S, n_vw, f)] = (short)g;
      S.chk[f] = 2; S.chk[g] = 2;
      atomicAdd(&S.flips, 1);
    }
    __syncthreads();
    if (tid == 0) S.rounds = round + 1;
  }
  __syncthreads();
  if (S.bad) {                                             // the budget ran out with a bad edge left
    __syncthreads();
    if (tid == 0) S.status = SN_DT_NOT_CONVERGED;
    __syncthreads();
    return;
  }
  for (int e = tid; e < 3 * nf; e += kWG) {
    const int f = e / 3, s = e - 3 * f, g = S.fa[f][s];
    if (g <= f) continue;
    const int s1 = s == 2 ? 0 : s + 1, s2 = s1 == 2 ? 0 : s1 + 1;
    const int t = side_of(S, g, f), t2 = t == 0 ? 2 : t - 1;
    if (incircle_keys(S.key[S.fv[f][s]], S.key[S.fv[f][s1]], S.key[S.fv[f][s2]], S.key[S.fv[g][t2]]) == 0)
      atomicAdd(&S.cocircular, 1);
  }
  __syncthreads();
}

// Canonical faces (input indices, smallest first, sorted) into F[rows][3]; rows past nf are -1.  Uses S.claim.
template <class DT>
__device__ void dt_store(DT &S, int32_t *F, int64_t rows) {
  const int tid = threadIdx.x;
  const int nf = S.status ? 0 : S.nf;
  const int m = pow2_at_least(nf);
  for (int f = tid; f < m; f += kWG) {
    int k = INT_MAX;
    if (f < nf) {
      const int a = S.perm[S.fv[f][0]], b = S.perm[S.fv[f][1]], c = S.perm[S.fv[f][2]];
      k = (a < b && a < c) ? (a << 20 | b << 10 | c) : ((b < a && b < c) ? (b << 20 | c << 10 | a) : (c << 20 | a << 10 | b));
    }
    S.claim[f] = k;
  }
  __syncthreads();
  sort_claims(S, m);
  for (int64_t i = tid; i < rows * 3; i += kWG) {
    const int f = (int)(i / 3), c = (int)(i - 3 * (int64_t)f);
    F[i] = f < nf ? ((S.claim[f] >> (20 - 10 * c)) & 1023) : -1;
  }
  __syncthreads();
}

template <int N>
__global__ void __launch_bounds__(kWG) delaunay2d_k(const int32_t *P, const int32_t *count, int64_t nmax, int max_rounds, int32_t *F,
                                                    int32_t *nF, int32_t *status, int32_t *counts) {
  __shared__ DtState<N> S;
  const int64_t b = blockIdx.x;
  const int32_t *Pb = P + b * nmax * 2;
  const int n = count ? count[b] : (int)(nmax < INT_MAX ? nmax : INT_MAX);
  dt_run(S, Pb, Pb + 1, 2, n, (int)(nmax < N ? nmax : N), max_rounds);
  dt_store(S, F + b * nmax * 6, 2 * nmax);
  if (threadIdx.x == 0) {
    const int ok = S.status == 0;
    nF[b] = ok ? S.nf : 0;
    status[b] = S.status;
    counts[4 * b + 0] = S.flips;
    counts[4 * b + 1] = ok ? S.cocircular : 0;
    counts[4 * b + 2] = S.rounds;
    counts[4 * b + 3] = ok ? 2 * n - 2 - S.nf : 0;
  }
}

// ---- Poisson-disc sampling ----------------------------------------------------------------------------------------------------
template <int N>
struct PdState {
  static constexpr int kPoints = N;
  int px[N], py[N];             // the samples in the order they were made
  short grid[kN];               // cell -> sample, -1 empty
  short active[N];
  int cx[kCand], cy[kCand];
  int n, nact, win, steps;
};

struct PdParams {
  unsigned long long seed;
  int64_t image;
  int attempt;
  int WQ, HQ;                   // the open rectangle (0, WQ) x (0, HQ)
  int R, cell, gw, gh;
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// prefix: h after (image, attempt);  draw = mix64(mix64(prefix + G + step) + G + (cand << 16 | retry << 8 | purpose))
__device__ __forceinline__ unsigned long long draw_prefix(const PdParams &p) {
  unsigned long long h = mix64(p.seed + 0x9E3779B97F4A7C15ull + (unsigned long long)p.image);
  return mix64(h + 0x9E3779B97F4A7C15ull + (unsigned long long)(long long)p.attempt);
}
__device__ __forceinline__ unsigned long long draw(unsigned long long prefix, int step, int cand, int retry, int purpose) {
  const unsigned long long h = mix64(prefix + 0x9E3779B97F4A7C15ull + (unsigned long long)step);
  return mix64(h + 0x9E3779B97F4A7C15ull + (unsigned long long)((cand << 16) | (retry << 8) | purpose));
}
__device__ __forceinline__ int below(unsigned long long d, unsigned m) { return (int)(((d >> 32) * (unsigned long long)m) >> 32); }

// Whole workgroup, uniform control flow.  Leaves S.n samples in S.px / S.py and S.steps.
template <class PD>
__device__ void pd_run(PD &S, const PdParams &p) {
  const int tid = threadIdx.x;
  const int cells = p.gw * p.gh;                      // <= kN, checked by the host entry
  const unsigned long long prefix = draw_prefix(p);
  const int64_t R2 = (int64_t)p.R * p.R;
  for (int i = tid; i < cells; i += kWG) S.grid[i] = -1;
  __syncthreads();
  if (tid == 0) {
    const int x = 1 + below(draw(prefix, 0, 0, 0, 0), (unsigned)(p.WQ - 1)), y = 1 + below(draw(prefix, 0, 0, 0, 1), (unsigned)(p.HQ - 1));
    S.px[0] = x; S.py[0] = y;
    S.grid[(y / p.cell) * p.gw + x / p.cell] = 0;
    S.active[0] = 0;
    S.n = 1; S.nact = 1; S.steps = 0;
  }
  __syncthreads();
  for (int step = 1; step <= 2 * cells; ++step) {     // one sample per cell, one retirement per sample
    const int nact = S.nact;
    if (nact == 0) break;                             // uniform: written before the last barrier
    const int j = below(draw(prefix, step, 0, 0, 2), (unsigned)nact);
    const int a = S.active[j], ax = S.px[a], ay = S.py[a];
    if (tid == 0) { S.win = kCand; S.steps = step; }
    __syncthreads();
    for (int c = tid; c < kCand; c += kWG) {             // one lane per candidate
      bool ok = false;
      int dx = 0, dy = 0;
      for (int t = 0; t < kRetry && !ok; ++t) {
        dx = below(draw(prefix, step, c, t, 3), 4u * (unsigned)p.R) - 2 * p.R;
        dy = below(draw(prefix, step, c, t, 4), 4u * (unsigned)p.R) - 2 * p.R;
        const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy;
        ok = d2 >= R2 && d2 < 4 * R2;
      }
      const int x = ax + dx, y = ay + dy;
      ok = ok && x > 0 && x < p.WQ && y > 0 && y < p.HQ;
      if (ok) {
        const int gx = x / p.cell, gy = y / p.cell;
        for (int v = -2; v <= 2 && ok; ++v)
          for (int u = -2; u <= 2 && ok; ++u) {
            const int qx = gx + u, qy = gy + v;
            if (qx < 0 || qy < 0 || qx >= p.gw || qy >= p.gh) continue;
            const int i = S.grid[qy * p.gw + qx];
            if (i < 0) continue;
            const int64_t ex = x - S.px[i], ey = y - S.py[i];
            if (ex * ex + ey * ey < R2) ok = false;
          }
      }
      if (ok) {
        S.cx[c] = x; S.cy[c] = y;
        atomicMin(&S.win, c);
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int w = S.win;
      if (w < kCand && S.n < PD::kPoints) {              // (never false: pd_capacity bounds the samples)
        const int i = S.n, x = S.cx[w], y = S.cy[w];
        S.px[i] = x; S.py[i] = y;
        S.grid[(y / p.cell) * p.gw + x / p.cell] = (short)i;
        S.active[nact] = (short)i;
        S.n = i + 1; S.nact = nact + 1;
      } else {
        S.active[j] = S.active[nact - 1];
        S.nact = nact - 1;
      }
    }
    __syncthreads();
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kWG) poisson_disc_k(PdParams p, int64_t nmax, int32_t *P, int32_t *count, int32_t *steps) {
  __shared__ PdState<kN> S;
  const int64_t b = blockIdx.x;
  p.image += b;
  pd_run(S, p);
  const int n = S.n;
  for (int64_t i = threadIdx.x; i < nmax; i += kWG) {
    P[(b * nmax + i) * 2 + 0] = i < n ? S.px[i] : 0;
    P[(b * nmax + i) * 2 + 1] = i < n ? S.py[i] : 0;
  }
  if (threadIdx.x == 0) { count[b] = n; steps[b] = S.steps; }
}

// ---- the maker: sampler, Delaunay, quality test, retries, intensity ------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(kWG) mesh_digits_k(const uint8_t *images, int rows, int cols, PdParams p, int min_points,
                                                     int64_t min_det, int max_attempts, int max_rounds, int64_t nmax, int32_t *P,
                                                     int32_t *count, float *V, int32_t *F, int32_t *nF, int32_t *status,
                                                     int32_t *attempts, int32_t *counts) {
  __shared__ DtState<N> D;
  __shared__ PdState<N> S;
  __shared__ int small;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  p.image += b;
  bool taken = false;
  int attempt = 0;
  for (; attempt < max_attempts; ++attempt) {            // at most SN_MESHDIGITS_MAX_ATTEMPTS
    p.attempt = attempt;
    pd_run(S, p);
    if (tid == 0) small = 0;
    __syncthreads();
    const int n = S.n;
    if (n < min_points) continue;                         // uniform
    dt_run(D, S.px, S.py, 1, n, (int)(nmax < N ? nmax : N), max_rounds);
    if (D.status) continue;                               // uniform: dt_run ends behind a barrier
    for (int f = tid; f < D.nf; f += kWG)
      if (orient_keys(D.key[D.fv[f][0]], D.key[D.fv[f][1]], D.key[D.fv[f][2]]) <= min_det) small = 1;
    __syncthreads();
    if (small) continue;
    taken = true;
    break;
  }
  __syncthreads();
  const int n = taken ? S.n : 0;
  if (!taken && tid == 0) D.status = SN_DT_REJECTED;
  __syncthreads();
  dt_store(D, F + b * nmax * 6, 2 * nmax);
  const uint8_t *img = images + b * (int64_t)rows * cols;
  for (int64_t i = tid; i < nmax; i += kWG) {
    int x = 0, y = 0;
    float z = 0.f;
    if (i < n) {
      x = S.px[i]; y = S.py[i];
      const int iu = x >> 16, iv = y >> 16;
      const int64_t fu = x & 0xffff, fv = y & 0xffff, Q = 65536;
      const uint8_t *r0 = img + (int64_t)(rows - 1 - iv) * cols + iu, *r1 = r0 - cols;
      const int64_t sum = r0[0] * (Q - fv) * (Q - fu) + r0[1] * (Q - fv) * fu + r1[0] * fv * (Q - fu) + r1[1] * fv * fu;
      z = (float)((double)sum / 1095216660480.0);         // 255 * 2^32: one rounding to double, one to float
    }
    int32_t *Pi = P + (b * nmax + i) * 2;
    float *Vi = V + (b * nmax + i) * 3;
    Pi[0] = x; Pi[1] = y;
    Vi[0] = (float)x * (1.0f / 65536.0f); Vi[1] = (float)y * (1.0f / 65536.0f); Vi[2] = z;
  }
  if (tid == 0) {
    count[b] = n;
    nF[b] = taken ? D.nf : 0;
    status[b] = taken ? 0 : SN_DT_REJECTED;
    attempts[b] = attempt;
    counts[4 * b + 0] = taken ? D.flips : 0;
    counts[4 * b + 1] = taken ? D.cocircular : 0;
    counts[4 * b + 2] = taken ? D.rounds : 0;
    counts[4 * b + 3] = taken ? 2 * n - 2 - D.nf : 0;
  }
}

int pd_params(uint64_t seed, int64_t image_base, int32_t attempt, int64_t W, int64_t H, int64_t R, PdParams *p) {
  if (W < 1 || H < 1 || R < 4 || attempt < 0) return SN_E_SHAPE;
  if (W * 65536 >= ((int64_t)1 << 24) || H * 65536 >= ((int64_t)1 << 24) || 4 * R >= ((int64_t)1 << 31)) return SN_E_RANGE;
  const int64_t half = R * R / 2;
  int64_t cell = 0;
  for (int bit = 30; bit >= 0; --bit) {                   // isqrt
    const int64_t c = cell | ((int64_t)1 << bit);
    if (c * c <= half) cell = c;
  }
  const int64_t gw = (W * 65536 + cell - 1) / cell, gh = (H * 65536 + cell - 1) / cell;
  if (gw * gh > SN_DELAUNAY_MAX_POINTS) return SN_E_UNSUPPORTED;
  p->seed = seed; p->image = image_base; p->attempt = attempt;
  p->WQ = (int)(W * 65536); p->HQ = (int)(H * 65536);
  p->R = (int)R; p->cell = (int)cell; p->gw = (int)gw; p->gh = (int)gh;
  return SN_OK;
}

// Samples are at least R apart, so the discs of radius R / 2 around them are disjoint and lie in the domain grown by R / 2 on every
// side: n pi R^2 / 4 <= (WQ + R)(HQ + R), and with pi > 3 n <= 4 (WQ + R)(HQ + R) / (3 R^2).  Also n <= cells.
int64_t pd_capacity(const PdParams &p) {
  const int64_t pack = 4 * ((int64_t)p.WQ + p.R) * ((int64_t)p.HQ + p.R) / (3 * (int64_t)p.R * p.R);
  const int64_t cells = (int64_t)p.gw * p.gh;
  return pack < cells ? pack : cells;
}

}  // namespace

extern "C" {

int64_t sn_delaunay2d_max_points(void) { return SN_DELAUNAY_MAX_POINTS; }

int sn_delaunay2d_i32(const int32_t *P, const int32_t *count, int64_t B, int64_t Nmax, int32_t max_rounds, int32_t *F, int32_t *nF,
                      int32_t *status, int32_t *counts, void *stream) {
  if (B < 0 || Nmax < 0 || max_rounds < 1) return SN_E_SHAPE;
  if (B == 0) return SN_OK;
  if ((!P && Nmax > 0) || (!F && Nmax > 0) || !nF || !status || !counts) return SN_E_NULL;
  if (B > INT_MAX || Nmax > (INT_MAX / 8)) return SN_E_RANGE;
  if (Nmax <= kSmall)                                     // half the LDS, twice the workgroups in flight
    hipLaunchKernelGGL(delaunay2d_k<kSmall>, dim3((unsigned)B), dim3(kWG), 0, (hipStream_t)stream, P, count, Nmax, max_rounds, F, nF,
                       status, counts);
  else
    hipLaunchKernelGGL(delaunay2d_k<kN>, dim3((unsigned)B), dim3(kWG), 0, (hipStream_t)stream, P, count, Nmax, max_rounds, F, nF, status,
                       counts);
  return launch_status();
}

int64_t sn_poisson_disc_cells(int64_t W, int64_t H, int64_t R) {
  PdParams p;
  const int st = pd_params(0, 0, 0, W, H, R, &p);
  return st == SN_OK ? (int64_t)p.gw * p.gh : (int64_t)st;
}

int sn_poisson_disc_i32(uint64_t seed, int64_t image_base, int32_t attempt, int64_t W, int64_t H, int64_t R, int64_t B, int64_t Nmax,
                        int32_t *P, int32_t *count, int32_t *steps, void *stream) {
  PdParams p;
  const int st = pd_params(seed, image_base, attempt, W, H, R, &p);
  if (st != SN_OK) return st;
  if (B < 0 || Nmax < (int64_t)p.gw * p.gh) return SN_E_SHAPE;
  if (B == 0) return SN_OK;
  if (!P || !count || !steps) return SN_E_NULL;
  if (B > INT_MAX) return SN_E_RANGE;
  hipLaunchKernelGGL(poisson_disc_k, dim3((unsigned)B), dim3(kWG), 0, (hipStream_t)stream, p, Nmax, P, count, steps);
  return launch_status();
}

int sn_mesh_digits_u8(const uint8_t *images, int64_t B, int32_t rows, int32_t cols, uint64_t seed, int64_t image_base, int64_t R,
                      int32_t min_points, int64_t min_det, int32_t max_attempts, int32_t max_rounds, int64_t Nmax, int32_t *P,
                      int32_t *count, float *V, int32_t *F, int32_t *nF, int32_t *status, int32_t *attempts, int32_t *counts,
                      void *stream) {
  if (rows < 2 || cols < 2 || max_attempts < 0 || max_attempts > SN_MESHDIGITS_MAX_ATTEMPTS || max_rounds < 1 || min_det < 0)
    return SN_E_SHAPE;
  PdParams p;
  const int st = pd_params(seed, image_base, 0, cols - 1, rows - 1, R, &p);
  if (st != SN_OK) return st;
  if (B < 0 || Nmax < (int64_t)p.gw * p.gh) return SN_E_SHAPE;
  if (B == 0) return SN_OK;
  if (!images || !P || !count || !V || !F || !nF || !status || !attempts || !counts) return SN_E_NULL;
  if (B > INT_MAX || Nmax > (INT_MAX / 8)) return SN_E_RANGE;
  if (min_points < 3) min_points = 3;
  if (pd_capacity(p) <= kSmall)                           // 32 KiB of LDS instead of 62: four workgroups on a CU instead of two
    hipLaunchKernelGGL(mesh_digits_k<kSmall>, dim3((unsigned)B), dim3(kWG), 0, (hipStream_t)stream, images, (int)rows, (int)cols, p,
                       (int)min_points, min_det, (int)max_attempts, (int)max_rounds, Nmax, P, count, V, F, nF, status, attempts, counts);
  else
    hipLaunchKernelGGL(mesh_digits_k<kN>, dim3((unsigned)B), dim3(kWG), 0, (hipStream_t)stream, images, (int)rows, (int)cols, p,
                       (int)min_points, min_det, (int)max_attempts, (int)max_rounds, Nmax, P, count, V, F, nF, status, attempts, counts);
  return launch_status();
}

}  // extern "C"
