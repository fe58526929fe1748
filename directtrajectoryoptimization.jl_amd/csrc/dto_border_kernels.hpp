// Border algebra of dto_kkt_border_factor / dto_kkt_border_solve (include/dto.h): model-independent kernels of the runtime
// library, not of the model plugin.  For every instance
//     [ K   G' ] [ v ]   [ r ]      G: nb x N border rows (nb <= 16, N = num_variables + num_constraint),  C: nb x nb
//     [ G   C  ] [ y ] = [ s ]
// is solved by the Schur complement on the border: Y = K^-1 G' and v0 = K^-1 r come from the path's own solves
// (dto_kkt_solve_multi / dto_kkt_solve), the four kernels below do the rest:
//     k_border_gram   P = G Y'              16 x 16 per instance, inner dimension N, on v_mfma_f64_16x16x4_f64
//     k_border_schur  S = sym(C) - sym(P)   Cholesky of -S (flag), LU with partial pivoting (kept), zero-pivot flag
//     k_border_rhs    y = S^-1 (s - Y r)    (G K^-1 r = Y r: K is symmetric)
//     k_border_sub    v = v0 - Y' y
// dto_kkt_border_multiply adds the border part of [K G'; G sym(C)] [v; y] to K v in one pass over the kept panel G (k_border_mul,
// k_border_mul_fin); dto_kkt_border_solve_refined is built on that product and the solve above.
// A vector of length N lives in two arrays (the variables' part and the constraint rows' part) with a leading dimension each,
// so every k range below is two segments.  Nothing is read beyond the row lengths: the callers' padding may hold anything.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dto_point_rules.hpp"

namespace dto {

constexpr int KB_MAX = 16;              // border rows of one panel
constexpr int KB_KT = 128;              // doubles of k per LDS slab
// row stride of a slab: a fragment read is slab[r][k + q] with r = lane & 15, q = lane >> 4; ds_read_b64 banks are (dword
// address) mod 64 and the two 32-lane halves are served separately, so r * LD + q must be distinct mod 32 for r < 16, q < 2 --
// LD = 2 (mod 32) makes it 2 r + q
constexpr int KB_LD = KB_KT + 2;
constexpr int KB_THREADS = 256;         // four wavefronts: each takes a quarter (32 doubles of k) of every slab
constexpr int KB_RHS_THREADS = 1024;    // k_border_rhs: one workgroup per instance
constexpr int KB_CHUNK_DEFAULT = 2048;  // doubles of k per workgroup ("bordered solves": how it was chosen)
constexpr int KB_ROW_BLOCKS = 64;       // workgroups per instance of k_border_sub (as AXPY_BLOCKS_PER_ROW)

typedef double kb_d4 __attribute__((ext_vector_type(4)));

// element k of row `row` of a vector stored as two segments
__device__ __forceinline__ double kb_seg(const double* x, int64_t ldx, const double* c, int64_t ldc, int64_t row, int64_t k, int64_t nx) {
  return k < nx ? x[row * ldx + k] : c[row * ldc + (k - nx)];
}

// P = G Y' per instance and chunk of k: grid.x = B * chunks, workgroup (b, ch) covers k in [ch * chunk, min(N, (ch + 1) * chunk))
// and writes its partial 16 x 16 (row-major: P[a][q] = sum_k G[a][k] Y[q][k]) to part[(b * chunks + ch) * 256].  No atomics: the
// partials are summed in chunk order by k_border_schur, so a result depends on the chunk length and on nothing else.
// Row j of instance b is row b * nb + j of (g_x, g_c) and of (y_x, y_c); n_c = 0 skips the second segment.  Rows nb .. 15 and
// the tail of the last slab are zeros in LDS.  Every row element is loaded once, a wavefront reading 64 consecutive doubles of
// one row per instruction; the loads of slab i + 1 are in flight while the matrix cores work on slab i.
static __global__ __launch_bounds__(KB_THREADS) void k_border_gram(int nb, int64_t n_x, int64_t n_c, int64_t chunk, int chunks,
                                                                   const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc,
                                                                   const double* y_x, int64_t ldyx, const double* y_c, int64_t ldyc,
                                                                   double* part) {
  __shared__ double sG[KB_MAX * KB_LD], sY[KB_MAX * KB_LD];
  const int64_t b = blockIdx.x / chunks;
  const int ch = (int)(blockIdx.x % chunks);
  const int64_t N = n_x + n_c;
  const int64_t k_lo = (int64_t)ch * chunk, k_hi = k_lo + chunk < N ? k_lo + chunk : N;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = t & (KB_KT - 1), half = t >> 7;   // this thread stages column `col` of rows half, half + 2, ...
  const int r = lane & 15, q = lane >> 4;
  double vg[8], vy[8];
  auto fetch = [&](int64_t k0) {
    const int64_t k = k0 + col;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = 2 * i + half;
      const bool in = row < nb && k < k_hi;
      vg[i] = in ? kb_seg(g_x, ldgx, g_c, ldgc, b * nb + row, k, n_x) : 0.0;
      vy[i] = in ? kb_seg(y_x, ldyx, y_c, ldyc, b * nb + row, k, n_x) : 0.0;
    }
  };
  kb_d4 acc = {0.0, 0.0, 0.0, 0.0};
  if (k_lo < k_hi) fetch(k_lo);
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += KB_KT) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sG[(2 * i + half) * KB_LD + col] = vg[i];
      sY[(2 * i + half) * KB_LD + col] = vy[i];
    }
    __syncthreads();   // the slab is complete before any wavefront reads fragments of it
    if (k0 + KB_KT < k_hi) fetch(k0 + KB_KT);
    const double* a = sG + r * KB_LD + wave * (KB_KT / 4) + q;
    const double* y = sY + r * KB_LD + wave * (KB_KT / 4) + q;
#pragma unroll
    for (int kk = 0; kk < KB_KT / 4; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], y[kk], acc, 0, 0, 0);
    __syncthreads();   // every fragment has been read before the slab is overwritten
  }
  // the four accumulators, added in wavefront order (C/D layout: col = lane & 15, row = (lane >> 4) + 4 j); sG is free after
  // the barrier that ended the loop
  double* red = sG;   // [4][256]
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wave * 256 + (q + 4 * j) * 16 + r] = acc[j];
  __syncthreads();
  part[((int64_t)b * chunks + ch) * 256 + t] = ((red[t] + red[256 + t]) + red[512 + t]) + red[768 + t];
}
static_assert(4 * 256 <= KB_MAX * KB_LD, "the reduction of k_border_gram reuses one slab");

// One wavefront per instance: P = sum of the partials in chunk order, S = (C + C')/2 - (P + P')/2, then lane 0: is -S positive
// definite (Cholesky attempt), LU of S with partial pivoting into lu [B][256] (row-major, stride 16: unit-lower multipliers
// below the diagonal, U on and above) and piv [B][16] (row exchanged with row k at step k); flags [2][B]: negdef, singular
// (a pivot that is zero -- or not a number -- was met; the elimination of that column is skipped).  csym [B][256], stride 16, keeps
// (C + C')/2 (zeros without c and beyond nb) for k_border_mul_fin.
// skeep (optional, [B][256], stride 16): S before the elimination, for a caller that wants its eigenvalue signs (dto_kkt_lbfgs_border).
static __global__ __launch_bounds__(64) void k_border_schur(int64_t B, int nb, int chunks, const double* part, const double* c, int64_t ldc,
                                                            double* lu, int* piv, int* flags, double* csym, double* skeep = nullptr) {
  __shared__ double P[256], S[256], L[256];
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double acc = 0.0;
    for (int ch = 0; ch < chunks; ++ch) acc += part[(b * chunks + ch) * 256 + l + 64 * e];
    P[l + 64 * e] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = l + 64 * e, a = i >> 4, q = i & 15;
    double v = 0.0, cs = 0.0;
    if (a < nb && q < nb) {
      if (c) cs = 0.5 * (c[b * ldc + a * nb + q] + c[b * ldc + q * nb + a]);
      v = cs - 0.5 * (P[a * 16 + q] + P[q * 16 + a]);
    }
    S[i] = v;
    csym[b * 256 + i] = cs;
    if (skeep) skeep[b * 256 + i] = v;
  }
  __syncthreads();
  if (l != 0) return;
  bool negdef = true, singular = false;
  for (int a = 0; a < nb && negdef; ++a)
    for (int q = 0; q <= a; ++q) {
      double acc = -S[a * 16 + q];
      for (int k = 0; k < q; ++k) acc -= L[a * 16 + k] * L[q * 16 + k];
      if (a == q) { if (!(acc > 0.0)) { negdef = false; break; } L[a * 16 + a] = sqrt(acc); }
      else L[a * 16 + q] = acc / L[q * 16 + q];
    }
  for (int k = 0; k < nb; ++k) {
    int pv = k;
    for (int i = k + 1; i < nb; ++i) if (fabs(S[i * 16 + k]) > fabs(S[pv * 16 + k])) pv = i;
    piv[b * 16 + k] = pv;
    if (pv != k)
      for (int q = 0; q < nb; ++q) { const double tmp = S[k * 16 + q]; S[k * 16 + q] = S[pv * 16 + q]; S[pv * 16 + q] = tmp; }
    const double d = S[k * 16 + k];
    if (!(fabs(d) > 0.0)) { singular = true; continue; }
    for (int i = k + 1; i < nb; ++i) {
      const double f = S[i * 16 + k] / d;
      S[i * 16 + k] = f;
      for (int q = k + 1; q < nb; ++q) S[i * 16 + q] -= f * S[k * 16 + q];
    }
  }
  for (int i = 0; i < 256; ++i) lu[b * 256 + i] = S[i];
  flags[b] = negdef ? 1 : 0;
  flags[B + b] = singular ? 1 : 0;
}

// One workgroup of sixteen wavefronts per instance (the dot products stream nb x N doubles per instance: at 256 instances one
// workgroup per compute unit has to keep the memory system busy on its own): t_j = s_j - Y_j . r for the nb rows of Y -- thread t
// adds elements t, t + 1024, ... of every row in that order, a shuffle tree inside the wavefront, the sixteen wavefront sums in
// wavefront order: the same order every run -- then thread 0 solves S y = t with the stored LU.  y goes to sol_b and to
// yw [B][16]; a singular instance gets NaN.
static __global__ __launch_bounds__(KB_RHS_THREADS) void k_border_rhs(int nb, int64_t n_x, int64_t n_c, const double* y_x, int64_t ldyx,
                                                                      const double* y_c, int64_t ldyc, const double* r_x, int64_t ldrx,
                                                                      const double* r_c, int64_t ldrc, const double* s, int64_t lds,
                                                                      const double* lu, const int* piv, const int* singular, double* sol_b,
                                                                      int64_t ldsb, double* yw) {
  __shared__ double red[KB_MAX][KB_RHS_THREADS / 64];
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t N = n_x + n_c;
  double acc[KB_MAX];
#pragma unroll
  for (int j = 0; j < KB_MAX; ++j) acc[j] = 0.0;
  for (int64_t k = t; k < N; k += KB_RHS_THREADS) {
    const double rk = kb_seg(r_x, ldrx, r_c, ldrc, b, k, n_x);
#pragma unroll
    for (int j = 0; j < KB_MAX; ++j)
      if (j < nb) acc[j] += kb_seg(y_x, ldyx, y_c, ldyc, b * nb + j, k, n_x) * rk;
  }
#pragma unroll
  for (int j = 0; j < KB_MAX; ++j) {
    double v = acc[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[j][wave] = v;
  }
  __syncthreads();   // the wavefront sums are in LDS before thread 0 reads them
  if (t != 0) return;
  double v[KB_MAX];
  const double* A = lu + b * 256;
  if (singular[b]) {
    for (int j = 0; j < nb; ++j) v[j] = __builtin_nan("");
  } else {
    for (int j = 0; j < nb; ++j) {
      double dot = 0.0;
      for (int w = 0; w < KB_RHS_THREADS / 64; ++w) dot += red[j][w];
      v[j] = s[b * lds + j] - dot;
    }
    // (the exchanges of the factorisation moved whole rows, multipliers included: all of them first, then the unit-lower solve)
    for (int k = 0; k < nb; ++k) {
      const int pv = piv[b * 16 + k];
      if (pv != k) { const double tmp = v[k]; v[k] = v[pv]; v[pv] = tmp; }
    }
    for (int k = 0; k < nb; ++k)
      for (int i = k + 1; i < nb; ++i) v[i] -= A[i * 16 + k] * v[k];
    for (int k = nb - 1; k >= 0; --k) {
      double a = v[k];
      for (int q = k + 1; q < nb; ++q) a -= A[k * 16 + q] * v[q];
      v[k] = a / A[k * 16 + k];
    }
  }
  for (int j = 0; j < nb; ++j) { sol_b[b * ldsb + j] = v[j]; yw[b * 16 + j] = v[j]; }
}

// sol = v0 - sum_j y_j Y_j (j ascending) over the N entries of every instance: grid.x = B * KB_ROW_BLOCKS, the outputs with their
// own leading dimensions, nothing written beyond the row lengths.  A NaN in y reaches every entry.
static __global__ __launch_bounds__(KB_THREADS) void k_border_sub(int nb, int64_t n_x, int64_t n_c, const double* v0, const double* y_x,
                                                                  int64_t ldyx, const double* y_c, int64_t ldyc, const double* yw,
                                                                  double* sol_x, int64_t ldsx, double* sol_c, int64_t ldsc) {
  const int64_t b = blockIdx.x / KB_ROW_BLOCKS, blk = blockIdx.x % KB_ROW_BLOCKS;
  const int64_t N = n_x + n_c;
  double y[KB_MAX];
#pragma unroll
  for (int j = 0; j < KB_MAX; ++j) y[j] = j < nb ? yw[b * 16 + j] : 0.0;
  for (int64_t k = blk * KB_THREADS + threadIdx.x; k < N; k += (int64_t)KB_ROW_BLOCKS * KB_THREADS) {
    double v = v0[b * N + k];
#pragma unroll
    for (int j = 0; j < KB_MAX; ++j)
      if (j < nb) v -= y[j] * kb_seg(y_x, ldyx, y_c, ldyc, b * nb + j, k, n_x);
    if (k < n_x) sol_x[b * ldsx + k] = v;
    else sol_c[b * ldsc + (k - n_x)] = v;
  }
}

// ---- dto_kkt_border_multiply: [out; out_b] = [K G'; G sym(C)] [v; v_b].  out arrives holding K v (k_wide_kmul); the border part is
//      ONE pass over the kept panel G, every entry loaded once and used twice:
//          out[k] += sum_j v_b[j] G[j][k]   (j ascending, the sum formed first)       t_j += G[j][k] v[k]
// grid.x = B * chunks with the chunks of dto_kkt_border_factor (k_border_gram), workgroup (b, ch) covers k in
// [ch * chunk, min(N, (ch + 1) * chunk)); n_c = 0 (no g_c at factor time) skips the constraint segment of G, v and out.  Thread t
// takes k_lo + t, k_lo + t + 256, ...: a wavefront reads 64 consecutive doubles of one row per instruction, the nb loads of one k
// are independent.  The partial t_j: thread sums in k order, a shuffle tree inside the wavefront, the four wavefront sums in
// wavefront order through LDS -> tpart[(b * chunks + ch) * 16 + j].  No atomics.  Nothing is read or written beyond the row lengths.
static __global__ __launch_bounds__(KB_THREADS) void k_border_mul(int nb, int64_t n_x, int64_t n_c, int64_t chunk, int chunks,
                                                                  const double* g_x, int64_t ldgx, const double* g_c, int64_t ldgc,
                                                                  const double* v_x, int64_t ldvx, const double* v_c, int64_t ldvc,
                                                                  const double* v_b, int64_t ldvb, double* out_x, int64_t ldox,
                                                                  double* out_c, int64_t ldoc, double* tpart) {
  __shared__ double red[KB_MAX][KB_THREADS / 64];
  const int64_t b = blockIdx.x / chunks;
  const int ch = (int)(blockIdx.x % chunks);
  const int64_t N = n_x + n_c;
  const int64_t k_lo = (int64_t)ch * chunk, k_hi = k_lo + chunk < N ? k_lo + chunk : N;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double y[KB_MAX], acc[KB_MAX];
#pragma unroll
  for (int j = 0; j < KB_MAX; ++j) {
    y[j] = j < nb ? v_b[b * ldvb + j] : 0.0;
    acc[j] = 0.0;
  }
  for (int64_t k = k_lo + t; k < k_hi; k += KB_THREADS) {
    const double vk = kb_seg(v_x, ldvx, v_c, ldvc, b, k, n_x);
    const double ok = kb_seg(out_x, ldox, out_c, ldoc, b, k, n_x);   // (K v)[k]: requested with the row loads, not after them
    double g[KB_MAX];
#pragma unroll
    for (int j = 0; j < KB_MAX; ++j) g[j] = j < nb ? kb_seg(g_x, ldgx, g_c, ldgc, b * nb + j, k, n_x) : 0.0;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KB_MAX; ++j)
      if (j < nb) {
        s += y[j] * g[j];
        acc[j] += g[j] * vk;
      }
    if (k < n_x) out_x[b * ldox + k] = ok + s;
    else out_c[b * ldoc + (k - n_x)] = ok + s;
  }
#pragma unroll
  for (int j = 0; j < KB_MAX; ++j) {
    double v = acc[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[j][wave] = v;
  }
  __syncthreads();   // the wavefront sums are in LDS before the first nb threads read them
  if (t < nb) tpart[((int64_t)b * chunks + ch) * KB_MAX + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}
static_assert(KB_THREADS / 64 == 4, "k_border_mul adds four wavefront sums");

// One wavefront per instance, lane j < nb: out_b[j] = sum of the partials t_j in chunk order, then + sym(C)[j][q] v_b[q], q ascending
// (csym [B][256], stride 16, as dto_kkt_border_factor kept it).
static __global__ __launch_bounds__(64) void k_border_mul_fin(int nb, int chunks, const double* tpart, const double* csym, const double* v_b,
                                                              int64_t ldvb, double* out_b, int64_t ldob) {
  const int64_t b = blockIdx.x;
  const int j = threadIdx.x;
  if (j >= nb) return;
  double acc = 0.0;
  for (int ch = 0; ch < chunks; ++ch) acc += tpart[(b * chunks + ch) * KB_MAX + j];
  for (int q = 0; q < nb; ++q) acc += csym[b * 256 + j * 16 + q] * v_b[b * ldvb + q];
  out_b[b * ldob + j] = acc;
}

// ---- the compact limited-memory BFGS matrix as a border (dto_kkt_lbfgs_border; dto_kkt_kernels.hpp, "limited-memory BFGS"):
//          B = sigma I - W M^-1 W',  W = [sigma S, Y],  M = [[sigma S'S, L], [L', -D]]   (L, D: strictly lower part / diagonal of S'Y)
//      so K0 - [W; 0] M^-1 [W; 0]' is the Schur complement of the bordered matrix [K0 U; U' M] with U' = the panel below.
// The panel of instance b (nb rows, nb >= 2 m: dto_kkt_lbfgs_border_rows keeps the caller's rows behind the history): rows 0 .. m-1 =
// sigma_b s_j, rows m .. 2m-1 = y_j (pair j = row b * m + j of s and y, oldest first), the rows of the pairs j >= npairs[b] zeros.
// One thread per entry of the variables' part; the constraint part is cleared by the caller.
static __global__ void k_lbfgs_panel(int64_t B, int m, int nb, int64_t Nz, const double* s, int64_t lds, const double* y, int64_t ldy,
                                     const int* npairs, const double* sigma, double* g, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * m * Nz) return;
  const int64_t row = idx / Nz, k = idx - row * Nz, b = row / m;
  const int j = (int)(row - b * m);
  const bool have = j < npairs[b];
  g[(b * nb + j) * ldg + k] = have ? sigma[b] * s[row * lds + k] : 0.0;
  g[(b * nb + m + j) * ldg + k] = have ? y[row * ldy + k] : 0.0;
}
// The caller's nr rows behind the 2 m history rows of every instance (dto_kkt_lbfgs_border_rows): row j of instance b is row
// b * nr + j of (g_x, g_c) and becomes row b * nb + (nb - nr) + j of the panel g (pitch ldg, Nz + Nc entries).  One thread per
// (instance, column): it writes its column of all nr rows, on the variable side and on the constraint side (zeros without g_c), so
// EVERY entry of those rows is written and nothing is summed.
static __global__ void k_lbfgs_rows(int64_t B, int nb, int nr, int64_t Nz, int64_t Nc, const double* g_x, int64_t ldgx, const double* g_c,
                                    int64_t ldgc, double* g, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t N = Nz + Nc;
  if (idx >= B * N) return;
  const int64_t b = idx / N, k = idx - b * N;
  for (int j = 0; j < nr; ++j) {
    const int64_t src = b * nr + j;
    const double v = k < Nz ? g_x[src * ldgx + k] : (g_c ? g_c[src * ldgc + (k - Nz)] : 0.0);
    g[(b * nb + (nb - nr) + j) * ldg + k] = v;
  }
}
// M of instance b from the Gram matrix of its panel (the partials of k_border_gram with the panel as both operands, summed in chunk
// order): P = [[sigma^2 S'S, sigma S'Y], [sigma Y'S, Y'Y]].  A pair the instance does not have gets +1 on the diagonal of the S block
// and -1 on that of the Y block: the Schur complement stays regular and keeps its inertia.  lbfgs_m_entry: entry (a, q) of M,
// a, q < 2 m, from P (stride 16).
__device__ __forceinline__ double lbfgs_m_entry(const double* P, int m, int np, double sg, int a, int q) {
  if (a < m && q < m) return (a < np && q < np) ? 0.5 * (P[a * 16 + q] + P[q * 16 + a]) / sg : (a == q ? 1.0 : 0.0);
  if (a >= m && q >= m) return a != q ? 0.0 : (a - m < np ? -P[(a - m) * 16 + a] / sg : -1.0);
  const int si = a < m ? a : q, yj = (a < m ? q : a) - m;   // the entry s_si' y_yj of L (or of L')
  return (si > yj && si < np) ? P[si * 16 + m + yj] / sg : 0.0;
}
// c [B][4 m m], row-major.
static __global__ __launch_bounds__(64) void k_lbfgs_c(int m, int chunks, const double* part, const int* npairs, const double* sigma, double* c) {
  __shared__ double P[256];
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x, nb = 2 * m, np = npairs[b];
  const double sg = sigma[b];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double acc = 0.0;
    for (int ch = 0; ch < chunks; ++ch) acc += part[(b * chunks + ch) * 256 + l + 64 * e];
    P[l + 64 * e] = acc;
  }
  __syncthreads();
  for (int i = l; i < nb * nb; i += 64) {
    const int a = i / nb, q = i - a * nb;
    c[b * nb * nb + i] = lbfgs_m_entry(P, m, np, sg, a, q);
  }
}
// The same with the caller's nr rows behind the history (dto_kkt_lbfgs_border_rows; the Gram pass ran over all nb = 2 m + nr rows of
// the panel, only its 2 m x 2 m corner is read: an entry of P is the sum over k of ONE product, so that corner has the bits it has
// without the rows): c [B][nb * nb], row-major = blkdiag(M, C) -- M top-left, the caller's cr ([B][ldcr], nr x nr row-major) bottom-right,
// zeros between.
static __global__ __launch_bounds__(64) void k_lbfgs_c_rows(int m, int nr, int chunks, const double* part, const int* npairs, const double* sigma,
                                                            const double* cr, int64_t ldcr, double* c) {
  __shared__ double P[256];
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x, nm = 2 * m, nb = nm + nr, np = npairs[b];
  const double sg = sigma[b];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double acc = 0.0;
    for (int ch = 0; ch < chunks; ++ch) acc += part[(b * chunks + ch) * 256 + l + 64 * e];
    P[l + 64 * e] = acc;
  }
  __syncthreads();
  for (int i = l; i < nb * nb; i += 64) {
    const int a = i / nb, q = i - a * nb;
    double v = 0.0;
    if (a < nm && q < nm) v = lbfgs_m_entry(P, m, np, sg, a, q);
    else if (a >= nm && q >= nm) v = cr[b * ldcr + (a - nm) * nr + (q - nm)];
    c[b * nb * nb + i] = v;
  }
}

// ---- the secant pairs of the limited-memory mode in the bordered solve loop (dto_solver.cpp: general_solve_batch with a QnHistory).
//      Instance-major, a thread owns a column, sums in a fixed order.
// grad_x L(x, lam) without bound-multiplier terms = grad f + J' lam, columns through the CSC tables of k_border_point.
__device__ __forceinline__ double qn_grad_l(int64_t b, int64_t col, int64_t nnzJ, const double* J, const double* g, int64_t Nz,
                                            const double* lam, int64_t ldl, const int* cptr, const int* ck, const int* crow) {
  double acc = g[b * Nz + col];
  for (int e = cptr[col]; e < cptr[col + 1]; ++e) acc += J[b * nnzJ + ck[e]] * lam[b * ldl + crow[e]];
  return acc;
}
// after an accepted step: s = alpha dz and gl = grad_x L(x_k, lam_{k+1}) from grad f and J of the OLD point (still in the step's
// workspace) and the NEW multipliers.  alpha[b] == 0: the instance took no step, nothing of it is written.
static __global__ void k_border_qn_save(int64_t B, int64_t Nz, int64_t nnzJ, const double* J, const double* g, const double* lam, int64_t ldl,
                                 const int* cptr, const int* ck, const int* crow, const double* dz, const double* alpha, double* s, double* gl) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, col = idx - b * Nz;
  const double al = alpha[b];
  if (al == 0.0) return;
  s[idx] = al * dz[idx];
  gl[idx] = qn_grad_l(b, col, nnzJ, J, g, Nz, lam, ldl, cptr, ck, crow);
}
// at the new point: y = grad_x L(x_{k+1}, lam_{k+1}) - gl (zero, with s, on a fixed variable), and dots [B][3] = s'y, s's, y'y:
// one workgroup of 256 per instance, thread t adds columns t, t + 256, ... in that order, a shuffle tree, the four wavefront sums in
// wavefront order.  pending[b] == 0: the instance has no saved step, nothing of it is written.
static __global__ __launch_bounds__(256) void k_border_qn_y(int64_t Nz, int64_t nnzJ, const double* J, const double* g, const double* lam, int64_t ldl,
                                                     const int* cptr, const int* ck, const int* crow, const int* fixed, const int* pending,
                                                     double* s, const double* gl, double* y, double* dots) {
  __shared__ double red[3][4];
  const int64_t b = blockIdx.x;
  if (!pending[b]) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sy = 0.0, ss = 0.0, yy = 0.0;
  for (int64_t col = t; col < Nz; col += 256) {
    const int64_t i = b * Nz + col;
    double sv = s[i], yv = 0.0;
    if (fixed[col]) { sv = 0.0; s[i] = 0.0; }
    else yv = qn_grad_l(b, col, nnzJ, J, g, Nz, lam, ldl, cptr, ck, crow) - gl[i];
    y[i] = yv;
    sy += sv * yv; ss += sv * sv; yy += yv * yv;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sy += __shfl_down(sy, off, 64); ss += __shfl_down(ss, off, 64); yy += __shfl_down(yy, off, 64); }
  if (lane == 0) { red[0][wave] = sy; red[1][wave] = ss; red[2][wave] = yy; }
  __syncthreads();
  if (t < 3) dots[b * 3 + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}
// push the pair (s, y) of the instances with slot[b] >= 0 into their histories S, Y [B][m][Nz], oldest first: slot[b] = m drops the
// oldest pair first (rows 1 .. m-1 move down, the new pair is row m-1), slot[b] < m writes row slot[b].  A thread owns a column of
// an instance, so the move needs no barrier.
static __global__ void k_border_qn_push(int64_t B, int m, int64_t Nz, const int* slot, const double* s, const double* y, double* S, double* Y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, col = idx - b * Nz;
  int k = slot[b];
  if (k < 0) return;
  double* Sb = S + b * m * Nz + col;
  double* Yb = Y + b * m * Nz + col;
  if (k >= m) {
    for (int j = 1; j < m; ++j) { Sb[(int64_t)(j - 1) * Nz] = Sb[(int64_t)j * Nz]; Yb[(int64_t)(j - 1) * Nz] = Yb[(int64_t)j * Nz]; }
    k = m - 1;
  }
  Sb[(int64_t)k * Nz] = s[idx];
  Yb[(int64_t)k * Nz] = y[idx];
}

// ---- finite variable bounds in the bordered solve loop (dto_solver.cpp: general_solve_batch): primal-dual barrier with the bound
//      multipliers eliminated, as wide_outer has it.  The per-variable pieces are wide_bar / wide_bar_step of dto_wide_kernels.hpp
//      (include that header first); lo == hi is a fixed variable and has no barrier term.
// What bordered_step is given beside the point: device pointers, z / zl / zu instance-major [B][Nz], lo / hi the problem's shared
// bounds [Nz], mu the barrier parameter per instance [B].  z == NULL: no barrier terms, the step is the plain Newton step.
struct BorderBar {
  const double *z = nullptr, *zl = nullptr, *zu = nullptr, *lo = nullptr, *hi = nullptr, *mu = nullptr;
};
enum { BORDER_BAR_APMAX = 0, BORDER_BAR_ADMAX, BORDER_BAR_LOGBAR, BORDER_BAR_DPHI, BORDER_BAR_SZMAX, BORDER_BAR_ISZMAX, BORDER_BAR_SUMZ,
       BORDER_BAR_DINF, BORDER_BAR_NSTAT };
// What the host loop needs of the bounds at the point and along the step dz, per instance (one wavefront each, lane-strided partial
// results and a fixed tree, so the same numbers at every run): the fraction-to-the-boundary steps alpha_p^max / alpha_d^max with
// tau = max(tau_min, 1 - mu), sum log(gap), the barrier part of the merit's directional derivative -mu sum dx/(x-lo) + mu sum dx/(hi-x),
// max gap z and max 1 / (gap z) (DTO_WIDE_SZMAX / ISZMAX of the tile solver: compl_at(mu) on the host for any mu), sum z_L + sum z_U,
// and the dual infeasibility over the non-fixed variables of an r_x that already holds - z_L + z_U.
static __global__ __launch_bounds__(64) void k_border_bar_stats(int64_t Nz, BorderBar bar, const double* dz, const double* rx,
                                                                const int* fixed, double tau_min, double* out) {
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
  const double mu = bar.mu[b], tau = fmax(tau_min, 1.0 - mu);
  double ap = 1.0, ad = 1.0, logb = 0.0, dphi = 0.0, szmax = 0.0, iszmax = 0.0, sumz = 0.0, dinf = 0.0;
  for (int64_t k = l; k < Nz; k += 64) {
    const int64_t i = b * Nz + k;
    const double x = bar.z[i], dx = dz[i], lo = bar.lo[k], hi = bar.hi[k], zl = bar.zl[i], zu = bar.zu[i];
    const wide::WideBar wb = wide::wide_bar(x, lo, hi, zl, zu, mu);
    logb += wb.logb; sumz += wb.sum_z; dphi -= wb.br * dx;
    szmax = fmax(szmax, wb.sz_max); iszmax = fmax(iszmax, wb.isz_max);
    wide::wide_bar_step(x, dx, lo, hi, zl, zu, mu, tau, ap, ad);
    if (!fixed[k]) dinf = fmax(dinf, fabs(rx[i]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    logb += __shfl_down(logb, off, 64); sumz += __shfl_down(sumz, off, 64); dphi += __shfl_down(dphi, off, 64);
    szmax = fmax(szmax, __shfl_down(szmax, off, 64)); iszmax = fmax(iszmax, __shfl_down(iszmax, off, 64));
    dinf = fmax(dinf, __shfl_down(dinf, off, 64));
    ap = fmin(ap, __shfl_down(ap, off, 64)); ad = fmin(ad, __shfl_down(ad, off, 64));
  }
  if (l == 0) {
    double* o = out + b * BORDER_BAR_NSTAT;
    o[BORDER_BAR_APMAX] = ap; o[BORDER_BAR_ADMAX] = ad; o[BORDER_BAR_LOGBAR] = logb; o[BORDER_BAR_DPHI] = dphi;
    o[BORDER_BAR_SZMAX] = szmax; o[BORDER_BAR_ISZMAX] = iszmax; o[BORDER_BAR_SUMZ] = sumz; o[BORDER_BAR_DINF] = dinf;
  }
}
// ---- inequality rows (c <= 0) of stage Constraints in the bordered solve loop: slacks c + s = 0, s >= 0, eliminated as the loop
//      eliminates those of inequality general rows -- s / nu on the constraint diagonal (dto_kkt_system.sigma_c), mu / nu in the
//      right-hand side, nu the row's own entry of lam.  There are about T of them per instance, so they live on the device:
// s and the step ds instance-major [B][Ns] (zero on equality rows), mask [Ns] 1 on the inequality rows, mu the barrier parameter per
// instance [B] (shared with the bounds and the general rows' slacks).  s == NULL: no such rows, every kernel takes its old branch.
struct BorderSlack {
  double *s = nullptr, *ds = nullptr;
  const int* mask = nullptr;
  const double* mu = nullptr;
  int64_t Ns = 0;
};
enum { BORDER_SLK_APMAX = 0, BORDER_SLK_ADMAX, BORDER_SLK_LOGS, BORDER_SLK_DSS, BORDER_SLK_SNUMAX, BORDER_SLK_ISNUMAX, BORDER_SLK_SUMNU,
       BORDER_SLK_NSTAT };
// the start: s = max(-c, 1e-2) and nu = 1 on the masked rows (as the general rows' slacks start), s = ds = 0 on the others
static __global__ void k_border_slack_init(int64_t B, int64_t Nc, BorderSlack sl, const double* c, double* lam) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * sl.Ns) return;
  const int64_t b = idx / sl.Ns, k = idx - b * sl.Ns;
  sl.ds[idx] = 0.0;
  if (!sl.mask[k]) { sl.s[idx] = 0.0; return; }
  sl.s[idx] = fmax(-c[b * Nc + k], 1e-2);
  lam[b * Nc + k] = 1.0;
}
// What the host loop needs of these slacks at the point and along the step dlam, per instance (one wavefront each, lane-strided
// partial results and a fixed tree): ds = (mu - s nu) / nu - (s / nu) dnu, WRITTEN to sl.ds; alpha_p^max / alpha_d^max with
// tau = max(tau_min, 1 - mu); sum log s; sum ds / s; max s nu and max 1 / (s nu) (compl_at(mu) on the host for any mu); sum nu.
static __global__ __launch_bounds__(64) void k_border_slack_stats(int64_t Nc, BorderSlack sl, const double* lam, const double* dlam,
                                                                  double tau_min, double* out) {
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
  const double mu = sl.mu[b], tau = fmax(tau_min, 1.0 - mu);
  double ap = 1.0, ad = 1.0, logs = 0.0, dss = 0.0, snumax = 0.0, isnumax = 0.0, sumnu = 0.0;
  for (int64_t k = l; k < sl.Ns; k += 64) {
    if (!sl.mask[k]) continue;
    const double s = sl.s[b * sl.Ns + k], nu = lam[b * Nc + k], dnu = dlam[b * Nc + k];
    const double ds = (mu - s * nu) / nu - (s / nu) * dnu;
    sl.ds[b * sl.Ns + k] = ds;
    if (ds < 0.0) ap = fmin(ap, -tau * s / ds);
    if (dnu < 0.0) ad = fmin(ad, -tau * nu / dnu);
    logs += log(s); dss += ds / s; sumnu += fabs(nu);
    snumax = fmax(snumax, s * nu); isnumax = fmax(isnumax, 1.0 / (s * nu));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    logs += __shfl_down(logs, off, 64); dss += __shfl_down(dss, off, 64); sumnu += __shfl_down(sumnu, off, 64);
    snumax = fmax(snumax, __shfl_down(snumax, off, 64)); isnumax = fmax(isnumax, __shfl_down(isnumax, off, 64));
    ap = fmin(ap, __shfl_down(ap, off, 64)); ad = fmin(ad, __shfl_down(ad, off, 64));
  }
  if (l == 0) {
    double* o = out + b * BORDER_SLK_NSTAT;
    o[BORDER_SLK_APMAX] = ap; o[BORDER_SLK_ADMAX] = ad; o[BORDER_SLK_LOGS] = logs; o[BORDER_SLK_DSS] = dss;
    o[BORDER_SLK_SNUMAX] = snumax; o[BORDER_SLK_ISNUMAX] = isnumax; o[BORDER_SLK_SUMNU] = sumnu;
  }
}
// The update of the multipliers with such slacks (in the place of lam += alpha dlam): on a masked row s += alpha ds and
// nu += alpha_d dnu -- the dual fraction-to-the-boundary step, not alpha -- then Ipopt's kappa_Sigma clamp of nu against the instance's
// mu and the new s; every other row moves with alpha.  One thread owns a row: it reads the old s and nu itself.  alpha == 0 (the
// instance terminated, or its mu just moved): nothing of it is written.  Grid: B * blocks_per_row blocks.
static __global__ void k_border_slack_update(int64_t Nc, BorderSlack sl, double* lam, const double* dlam, const double* alpha,
                                             const double* alpha_d, double kappa_sigma, int blocks_per_row) {
  const int64_t b = blockIdx.x / blocks_per_row;
  const int64_t blk = blockIdx.x % blocks_per_row;
  const double al = alpha[b];
  if (al == 0.0) return;
  const double ad = alpha_d[b], mu = sl.mu[b];
  for (int64_t k = blk * blockDim.x + threadIdx.x; k < Nc; k += (int64_t)blocks_per_row * blockDim.x) {
    if (k < sl.Ns && sl.mask[k]) {
      const double s = sl.s[b * sl.Ns + k] + al * sl.ds[b * sl.Ns + k];
      const double nu = lam[b * Nc + k] + ad * dlam[b * Nc + k];
      sl.s[b * sl.Ns + k] = s;
      lam[b * Nc + k] = fmax(fmin(nu, kappa_sigma * mu / s), mu / (kappa_sigma * s));
    } else {
      lam[b * Nc + k] += al * dlam[b * Nc + k];
    }
  }
}

// ---- warm start of the bordered solve loop from a caller's primal-dual point (dto_solve_batch_warm; the rules: warm_var /
//      warm_slack / shift_source of dto_point_rules.hpp).  One thread per entry, instance-major, no atomics.
// The variables: x / zl_in / zu_in are the caller's arrays with their leading dimensions (zl_in == NULL: no multipliers given,
// every one starts on the central path), lo / hi the problem's shared bounds [Nz], mu [B] the barrier parameter per instance
// (NULL without a barrier).  z [B][Nz] takes the point, zl / zu [B][Nz] the multipliers; zl == NULL when the problem has no finite
// bound: only the fixed variables move then.
static __global__ void k_border_warm_vars(int64_t B, int64_t Nz, const double* x, int64_t ldx, const double* zl_in, int64_t ldzl,
                                          const double* zu_in, int64_t ldzu, const double* lo, const double* hi, const double* mu,
                                          double bound_push, double bound_frac, double* z, double* zl, double* zu) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, k = idx - b * Nz;
  const bool have = zl != nullptr;
  const WarmVar w = warm_var(x[b * ldx + k], lo[k], hi[k], have, (have && zl_in) ? zl_in[b * ldzl + k] : 0.0,
                             (have && zl_in) ? zu_in[b * ldzu + k] : 0.0, mu ? mu[b] : 0.0, bound_push, bound_frac);
  z[idx] = w.v;
  if (have) { zl[idx] = w.zl; zu[idx] = w.zu; }
}
// The slacks of the inequality stage rows, the warm counterpart of k_border_slack_init: c [B][Nc] the constraint values at the
// start point, lam [B][Nc] already holds the caller's multipliers, s_in the caller's slacks [B][lds] (NULL: none given).  A masked
// row keeps (s, nu) when both are positive, else takes warm_slack's start; s = ds = 0 on the other rows.
static __global__ void k_border_slack_warm(int64_t B, int64_t Nc, BorderSlack sl, const double* c, double* lam, const double* s_in,
                                           int64_t lds, double bound_push) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * sl.Ns) return;
  const int64_t b = idx / sl.Ns, k = idx - b * sl.Ns;
  sl.ds[idx] = 0.0;
  if (!sl.mask[k]) { sl.s[idx] = 0.0; return; }
  const WarmSlack w = warm_slack(c[b * Nc + k], s_in ? s_in[b * lds + k] : 0.0, lam[b * Nc + k], sl.mu[b], bound_push);
  sl.s[idx] = w.s;
  lam[b * Nc + k] = w.nu;
}
// Receding horizon on a caller's arrays (dto_point_shift): k_wide_shift_knots with a leading dimension and an inner count.  `in`
// holds B * inner vectors of n entries, vector v of instance b at in + (b * inner + v) * ld (inner = 1: x, the multipliers;
// inner = 6: the secant pairs of the limited-memory history, one launch for all of them); out is compact, [B * inner][n].
static __global__ void k_point_shift(const double* in, int64_t ld, double* out, int64_t n, int64_t B, int64_t inner, int stride,
                                     int T_blocks, int last_len, int k, const int* keep) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * inner * n) return;
  const int64_t row = idx / n, j = idx - row * n;   // row = b * inner + v
  out[idx] = in[row * ld + shift_source(j, stride, T_blocks, last_len, k, keep && keep[j])];
}

// A trial point of the line search with bounds, one launch: out[2 b] = sum_k |rows[b][k] (+ shift)|, the sum of k_rows_abs_sum in
// its order, and out[2 b + 1] = sum log(gap) of the trial point x ([B][Nz]; inside the bounds by the fraction-to-the-boundary rule;
// x == NULL: no bounds, 0).  With slacks of stage rows (sl.s != NULL; then the output has three numbers per instance): rows k < sl.Ns
// get s + alpha ds added (zero on equality rows) and out[3 b + 2] = sum log(s + alpha ds) over the masked rows.
static __global__ __launch_bounds__(64) void k_border_trial(const double* rows, int64_t ld, int64_t n, const double* shift, int64_t n0,
                                                            int64_t nsh, const double* x, int64_t Nz, const double* lo, const double* hi,
                                                            double* out, BorderSlack sl = BorderSlack(), const double* alpha = nullptr) {
  const int64_t b = blockIdx.x;
  double acc = 0.0, logb = 0.0, logs = 0.0;
  if (sl.s) {
    const double al = alpha[b];
    for (int64_t i = threadIdx.x; i < n; i += 64) {
      double v = rows[b * ld + i] + ((shift && i >= n0) ? shift[b * nsh + (i - n0)] : 0.0);
      if (i < sl.Ns) {
        const double st = sl.s[b * sl.Ns + i] + al * sl.ds[b * sl.Ns + i];
        v += st;
        if (sl.mask[i]) logs += log(st);
      }
      acc += fabs(v);
    }
  } else {
    for (int64_t i = threadIdx.x; i < n; i += 64) acc += fabs(rows[b * ld + i] + ((shift && i >= n0) ? shift[b * nsh + (i - n0)] : 0.0));
  }
  for (int64_t k = threadIdx.x; x && k < Nz; k += 64) {
    const double a = lo[k], c = hi[k], v = x[b * Nz + k];
    if (a == c) continue;
    double t = 0.0;   // (per variable first, as wide_bar sums it at the iterate)
    if (a > -1e300) t += log(v - a);
    if (c < 1e300) t += log(c - v);
    logb += t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64); logb += __shfl_down(logb, off, 64);
    if (sl.s) logs += __shfl_down(logs, off, 64);   // (uniform over the wavefront)
  }
  if (threadIdx.x == 0) {
    if (sl.s) { out[3 * b] = acc; out[3 * b + 1] = logb; out[3 * b + 2] = logs; }
    else { out[2 * b] = acc; out[2 * b + 1] = logb; }
  }
}

// ---- the bordered step of the solver on the lane path, device side (dto_solver.cpp: bordered_step_device; DTO_BORDER_HOST=1
//      selects the host algebra of bordered_step_host instead).  Only the per-instance numbers the host-driven solve loop reads and
//      B flags cross PCIe; the Jacobian, the n_g + 1 right-hand sides and solutions and the border algebra stay on the device.
// General rows of the lane path's device border: the LDS arrays of k_border_solve.  A limit of its own -- KB_MAX is the rows of one
// panel of right-hand sides on the tile path -- that happens to have the same value.
constexpr int BORDER_MAX_NG = 16;

// S y = r for the n x n Schur complement of a border, in place on the caller's storage (S: n * n row-major, r: n, L: n * n scratch
// of the Cholesky factor; n <= BORDER_MAX_NG in the LDS arrays of k_border_solve, any n in the vectors of bordered_step_host).
// Returns whether S is negative definite -- Cholesky of -S, symmetrised: the inertia of the bordered matrix is then (Nz, Nc) -- and
// leaves y in r: Gaussian elimination with partial pivoting and back substitution, whatever the verdict.  An exactly zero pivot
// makes the verdict false and its unknown zero.  One statement order for the device and the host: the two borders agree to the
// last bit where their inputs do.
__host__ __device__ __forceinline__ bool border_schur_solve(int ng, double* Sm, double* rg, double* Lc) {
  bool negdef = true;
  for (int a = 0; a < ng && negdef; ++a)
    for (int q = 0; q <= a; ++q) {
      double acc = -0.5 * (Sm[a * ng + q] + Sm[q * ng + a]);
      for (int k = 0; k < q; ++k) acc -= Lc[a * ng + k] * Lc[q * ng + k];
      if (a == q) { if (!(acc > 0.0)) { negdef = false; break; } Lc[a * ng + a] = sqrt(acc); }
      else Lc[a * ng + q] = acc / Lc[q * ng + q];
    }
  for (int k = 0; k < ng; ++k) {
    int piv = k;
    for (int r = k + 1; r < ng; ++r) if (fabs(Sm[r * ng + k]) > fabs(Sm[piv * ng + k])) piv = r;
    if (piv != k) {
      for (int q = 0; q < ng; ++q) { const double t = Sm[k * ng + q]; Sm[k * ng + q] = Sm[piv * ng + q]; Sm[piv * ng + q] = t; }
      const double t = rg[k]; rg[k] = rg[piv]; rg[piv] = t;
    }
    const double d = Sm[k * ng + k];
    if (d == 0.0) { negdef = false; continue; }
    for (int r = k + 1; r < ng; ++r) {
      const double f = Sm[r * ng + k] / d;
      for (int q = k; q < ng; ++q) Sm[r * ng + q] -= f * Sm[k * ng + q];
      rg[r] -= f * rg[k];
    }
  }
  for (int k = ng - 1; k >= 0; --k) {
    double acc = rg[k];
    for (int q = k + 1; q < ng; ++q) acc -= Sm[k * ng + q] * rg[q];
    rg[k] = Sm[k * ng + k] != 0.0 ? acc / Sm[k * ng + k] : 0.0;
  }
  return negdef;
}
// r_x = grad f + J' mu column by column (entries of a column in COO order: the same sums as the host loop of round 3), the
// general rows of J as dense vectors, the first right-hand side
static __global__ void k_border_rx(int64_t B, int64_t Nz, int64_t Ns, int64_t nnzJ, const double* J, const double* g, const double* mu,
                                   int64_t ldmu, const int* cptr, const int* ck, const int* crow, double* rx, double* rhsx, double* Grow,
                                   BorderBar bar) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, col = idx - b * Nz;
  double acc = g[idx];
  for (int e = cptr[col]; e < cptr[col + 1]; ++e) {
    const double v = J[b * nnzJ + ck[e]];
    const int row = crow[e];
    acc += v * mu[b * ldmu + row];
    if (row >= Ns) Grow[((int64_t)(row - Ns) * B + b) * Nz + col] += v;   // (this thread owns column col of instance b)
  }
  if (bar.z) {
    // finite bounds: r_x with the bound multipliers, the right-hand side with the barrier gradient (this kernel runs once per point:
    // a further delta_w attempt keeps both)
    const wide::WideBar wb = wide::wide_bar(bar.z[idx], bar.lo[col], bar.hi[col], bar.zl[idx], bar.zu[idx], bar.mu[b]);
    rx[idx] = acc + wb.zdiff;
    rhsx[idx] = -(acc - wb.br);
    return;
  }
  rx[idx] = acc;
  rhsx[idx] = -acc;
}
// what the host loop needs of the point and the step, per instance: theta_1, theta_inf (rows n0 .. get their slack added), the
// dual infeasibility over the free variables, sum |lam|, grad f' dz -- five numbers instead of five vectors over PCIe
static __global__ __launch_bounds__(64) void k_border_stats(int64_t Nz, int64_t Nc, const double* c, const double* rx, const double* g,
                                                            const double* dz, const double* lam, const int* fixed, const double* shift,
                                                            int64_t n0, int64_t nsh, double* out, const double* sshift = nullptr,
                                                            int64_t nss = 0) {
  // sshift (optional, [B][nss]): the slacks of the stage rows, added to rows 0 .. nss - 1 (zero on equality rows)
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
  double th1 = 0.0, thinf = 0.0, dinf = 0.0, slam = 0.0, gd = 0.0;
  for (int64_t k = l; k < Nc; k += 64) {
    double cv = c[b * Nc + k] + ((shift && k >= n0) ? shift[b * nsh + (k - n0)] : 0.0);
    if (sshift && k < nss) cv += sshift[b * nss + k];
    const double v = fabs(cv);
    th1 += v; thinf = fmax(thinf, v); slam += fabs(lam[b * Nc + k]);
  }
  for (int64_t k = l; k < Nz; k += 64) {
    if (!fixed[k]) dinf = fmax(dinf, fabs(rx[b * Nz + k]));
    gd += g[b * Nz + k] * dz[b * Nz + k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    th1 += __shfl_down(th1, off, 64); slam += __shfl_down(slam, off, 64); gd += __shfl_down(gd, off, 64);
    thinf = fmax(thinf, __shfl_down(thinf, off, 64)); dinf = fmax(dinf, __shfl_down(dinf, off, 64));
  }
  if (l == 0) { double* o = out + b * 5; o[0] = th1; o[1] = thinf; o[2] = dinf; o[3] = slam; o[4] = gd; }
}
// per-instance delta_w on the primal diagonal; a variable with lo == hi gets a huge entry instead (its step is ~1e-16 r); with
// finite bounds (bar.z != NULL) the others get delta_w + z_L/(x-lo) + z_U/(hi-x)
static __global__ void k_border_sig(int64_t B, int64_t Nz, const double* dw, const int* fixed, int pin_fixed, double* sig, BorderBar bar) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, col = idx % Nz;
  if (bar.z && !(pin_fixed && fixed[col])) {
    sig[idx] = dw[b] + wide::wide_bar(bar.z[idx], bar.lo[col], bar.hi[col], bar.zl[idx], bar.zu[idx], bar.mu[b]).sig;
    return;
  }
  sig[idx] = (pin_fixed && fixed[col]) ? 1e16 : dw[b];
}
// sl (sl.s != NULL: slack-eliminated inequality stage rows, see BorderSlack): such a row gets -(c + mu / nu) and s / nu in sigc
// ([B][Nc], zero everywhere else), nu its entry of the multipliers
static __global__ void k_border_rhsc(int64_t B, int64_t Nc, int64_t Ns, const double* c, double* rhsc, BorderSlack sl = BorderSlack(),
                                     const double* mu = nullptr, int64_t ldmu = 0, double* sigc = nullptr) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nc) return;
  if (sl.s) {
    const int64_t b = idx / Nc, k = idx - b * Nc;
    if (k < Ns && sl.mask[k]) {
      const double nu = mu[b * ldmu + k];
      rhsc[idx] = -(c[idx] + sl.mu[b] / nu);
      sigc[idx] = sl.s[b * sl.Ns + k] / nu;
      return;
    }
    sigc[idx] = 0.0;
  }
  rhsc[idx] = (idx % Nc) < Ns ? -c[idx] : 0.0;
}
// one wavefront per instance: S = -(G Y_x + dc I), r_g = -c_g - G v0_x (lane-strided partial sums, fixed tree), then lane 0: S
// negative definite? and S drho = r_g (border_schur_solve)
static __global__ __launch_bounds__(64) void k_border_solve(int64_t B, int64_t Nz, int64_t Nc, int64_t Ns, int ng, double delta_c,
                                                            const double* Grow, const double* Yx, const double* v0x, const double* c,
                                                            const double* gdiag, const double* gshift, double* rho, int* negdef_out) {
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
  __shared__ double Sm[BORDER_MAX_NG * BORDER_MAX_NG], rg[BORDER_MAX_NG], Lc[BORDER_MAX_NG * BORDER_MAX_NG];
  auto gdot = [&](int row, const double* v) {
    const double* gr = Grow + ((int64_t)row * B + b) * Nz;
    double acc = 0.0;
    for (int64_t k = l; k < Nz; k += 64) acc += gr[k] * v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    return acc;   // lane 0
  };
  for (int a = 0; a < ng; ++a) {
    for (int q = 0; q < ng; ++q) {
      const double d = gdot(a, Yx + ((int64_t)q * B + b) * Nz);
      // slack-eliminated inequality rows (general_solve_batch): s / nu on the diagonal, mu / nu in the right-hand side
      if (l == 0) Sm[a * ng + q] = -d - (a == q ? delta_c + (gdiag ? gdiag[b * ng + a] : 0.0) : 0.0);
    }
    const double d = gdot(a, v0x + b * Nz);
    if (l == 0) rg[a] = -c[b * Nc + Ns + a] - (gshift ? gshift[b * ng + a] : 0.0) - d;
  }
  if (l != 0) return;
  const bool negdef = border_schur_solve(ng, Sm, rg, Lc);
  for (int q = 0; q < ng; ++q) rho[b * ng + q] = rg[q];
  negdef_out[b] = negdef ? 1 : 0;
}
// v = v0 - Y drho; the multipliers of the general rows are drho
static __global__ void k_border_apply(int64_t B, int64_t Nz, int64_t Nc, int64_t Ns, int ng, const double* v0x, const double* v0c,
                                      const double* Yx, const double* Yc, const double* rho, double* dx, int64_t lddx, double* dmu,
                                      int64_t lddmu, double* hdx, double* hdm) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * (Nz + Nc)) return;
  const int64_t b = idx / (Nz + Nc), k = idx - b * (Nz + Nc);
  if (k < Nz) {
    double v = v0x[b * Nz + k];
    for (int q = 0; q < ng; ++q) v -= Yx[((int64_t)q * B + b) * Nz + k] * rho[b * ng + q];
    dx[b * lddx + k] = v;
    hdx[b * Nz + k] = v;
  } else {
    const int64_t r = k - Nz;
    double v;
    if (r < Ns) {
      v = v0c[b * Nc + r];
      for (int q = 0; q < ng; ++q) v -= Yc[((int64_t)q * B + b) * Nc + r] * rho[b * ng + q];
    } else {
      v = rho[b * ng + (r - Ns)];
    }
    dmu[b * lddmu + r] = v;
    hdm[b * Nc + r] = v;
  }
}

// ---- the bordered step of the solver on the tile path (dto_solver.cpp: bordered_step_tile): everything dto_kkt_border_factor /
//      dto_kkt_border_solve are given, from the derivatives at the point.  One thread per (instance, column) -- a thread owns
//      column `col` of instance b in r_x, rhs_x and all ng panel rows, so nothing is summed across threads:
//          r_x = grad f + J' mu (entries of a column in COO order, as k_border_rx),  rhs_x = -r_x
//          panel row b * ng + j = row j of the general rows' Jacobian, Nz entries, EVERY one written (zeros included)
//      and, on the first threads of the same grid (B * Ns < B * Nz: a dynamics row per state),
//          rhs_c = -c on the Ns stage-part rows (pitch Nc),  rhs_b = -(c_g + gshift),  C = -(delta_c + gdiag) I as [B][ng * ng]
//      pin (with fixed[col]): the variable keeps its value -- its column of the panel and its entry of rhs_x are zero (the factor
//      holds 1e16 on its diagonal).  J is indexed through the CSC tables of the constant pattern
//      (cptr [Nz + 1], ck: position in the COO value array, crow: 0-based row).
//      bar (bar.z != NULL: finite variable bounds, see BorderBar below): r_x gets - z_L + z_U and rhs_x the barrier gradient,
//          rhs_x = -(grad f + J' mu - mu_b/(x-lo) + mu_b/(hi-x)); this kernel runs at every delta_w attempt, so the terms are here.
static __global__ void k_border_point(int64_t B, int64_t Nz, int64_t Nc, int64_t Ns, int ng, int64_t nnzJ, const double* J, const double* g,
                                      const double* c, const double* mu, int64_t ldmu, const int* cptr, const int* ck, const int* crow,
                                      const int* fixed, int pin, double delta_c, const double* gdiag, const double* gshift, double* rx,
                                      double* rhsx, double* panel, double* rhsc, double* rhsb, double* cblk, BorderBar bar) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < B * Ns) {
    const int64_t b = idx / Ns, k = idx - b * Ns;
    rhsc[b * Nc + k] = -c[b * Nc + k];
  }
  if (idx < B * ng * ng) {
    const int64_t b = idx / (ng * ng);
    const int e = (int)(idx - b * ng * ng), a = e / ng, q = e - a * ng;
    cblk[idx] = a == q ? -(delta_c + (gdiag ? gdiag[b * ng + a] : 0.0)) : 0.0;
    if (q == 0) rhsb[b * ng + a] = -(c[b * Nc + Ns + a] + (gshift ? gshift[b * ng + a] : 0.0));
  }
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, col = idx - b * Nz;
  const bool pinned = pin && fixed[col];
  double* prow = panel + b * ng * Nz + col;
  for (int j = 0; j < ng; ++j) prow[(int64_t)j * Nz] = 0.0;
  double acc = g[idx];
  for (int e = cptr[col]; e < cptr[col + 1]; ++e) {
    const double v = J[b * nnzJ + ck[e]];
    const int row = crow[e];
    acc += v * mu[b * ldmu + row];
    if (row >= Ns && !pinned) prow[(int64_t)(row - Ns) * Nz] += v;
  }
  if (bar.z) {
    const wide::WideBar wb = wide::wide_bar(bar.z[idx], bar.lo[col], bar.hi[col], bar.zl[idx], bar.zu[idx], bar.mu[b]);
    rx[idx] = acc + wb.zdiff;
    rhsx[idx] = pinned ? 0.0 : -(acc - wb.br);
    return;
  }
  rx[idx] = acc;
  rhsx[idx] = pinned ? 0.0 : -acc;
}

// the step of a pinned variable (1e16 on its diagonal, zero right-hand side: what is left is the 1e-16-sized answer to its couplings) is
// exactly zero
static __global__ void k_border_unpin(int64_t B, int64_t Nz, const int* fixed, double* dx, int64_t lddx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Nz) return;
  const int64_t b = idx / Nz, k = idx - b * Nz;
  if (fixed[k]) dx[b * lddx + k] = 0.0;
}

// resid[b] = NaN for the instances whose Schur complement is singular (their solution is NaN in every entry; the maximum of
// k_rows_maxabs ignores NaN)
static __global__ void k_border_resid_singular(int64_t B, const int* singular, double* resid) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && singular[b]) resid[b] = __builtin_nan("");
}

}  // namespace dto
