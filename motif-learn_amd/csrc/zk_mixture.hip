// zk_mixture.hip -- the Gaussian mixture on the resident moment matrix (zk_rows.h):
//   gmm_lbs(X, n)      reference clustering/_clustering_functions.py:25-33 (sklearn GaussianMixture(n, type).fit(X).predict(X))
// the E step and the weighted second moments of the M step, each on the vector pipe and on the matrix cores, and the one-hot
// responsibilities of the k-means initialisation; zk_rows_gram is the M-step Gram code with unit weights.
#include "zk_rows.h"

namespace {

// ---- Gaussian mixture E step (sklearn/mixture/_gaussian_mixture.py _estimate_log_gaussian_prob + _base.py
// _estimate_log_prob_resp): per component y = x P - mu P with P the upper-triangular Cholesky factor of the precision
// ([k][D][DP] row-major, DP = D rounded up to ZK_EW, zeros below the diagonal and in the padding; b = mu P as [k][DP]),
// lp_c = (-0.5 (D log 2pi + |y|^2) + logdet_c) + logw_c; log-sum-exp over components; resp (k, N) = exp(lp - lse);
// label = first argmax; part[block] = sum of lse over the block's rows -----------------------------------------------------
#ifndef ZK_EW
#define ZK_EW 16  // columns of y per pass of the E step (8: 4.2 ms, 16: 2.9 ms per 4 M x 45 rows at k = 6)
#endif
#define ZK_LGKM_WAIT()                \
  __builtin_amdgcn_s_waitcnt(0xC07F); \
  __builtin_amdgcn_sched_barrier(0)

// (Tried: the product y = x P on the matrix cores -- v_mfma_f64_16x16x4_f64 runs at 77 TFLOP/s from vector registers,
//  tools/micro_mfma64.hip, against the 28-48 of SGPR-fed v_fma_f64 -- with wave = 16-row block, A from the LDS tile, B = the
//  factor from memory: correct on every test, but 3.4 ms against 2.1: every lane fetches its own element of the factor, 512 B
//  per MFMA, 19 TB through L1 / L2 per pass over 4 M rows, where a scalar operand is fetched once per wave and used by 64 lanes x
//  16 FMAs.  Reusing B across row blocks needs a different split of the work; not pursued.
//  Also tried: two rows per lane (128-row tiles) so that every scalar operand feeds two FMAs: 2.03 against 2.08 ms -- the
//  halved occupancy takes back what the halved scalar traffic gives.)
// ZK_EWAVES waves share a tile (every wave holds the same 64 rows, lane = row): the (component, column block) pairs are dealt
// to the waves by cost on the host (`plan`: per wave a count and its (c, j0) pairs), each wave adds the squared norm of a
// block into slot (block mod ZK_EWAVES) of an LDS table [ZK_EWAVES][k][64], and after a barrier every wave adds a component's
// slots in slot order -- redundant but cheap arithmetic -- for the log-sum-exp; the stores of the responsibilities are split
// by component.  (The slot follows the block, not the wave that computed it: which wave did a block must not show in the sum, or
// two identical components get log probabilities that differ in the last bit and the tie between them goes to either index.
// A slot takes one block (D <= 64: a plain store) or two (an LDS atomic add onto the zeroed slot: a + b is b + a, so the order
// in which the two waves arrive does not show either).)
#ifndef ZK_EWAVES
#define ZK_EWAVES 4
#endif
static_assert((ZK_EWAVES & (ZK_EWAVES - 1)) == 0 && ZK_EW * 2 * ZK_EWAVES >= 128, "a slot takes at most two column blocks");
__global__ __launch_bounds__(64 * ZK_EWAVES) void estep_kernel(const double* __restrict__ X, long long N, int D, int DP,
                                                               const double* __restrict__ P, const double* __restrict__ B,
                                                               const double* __restrict__ cst /* [k][2]: logdet, logw */,
                                                               const int* __restrict__ plan, int plan_stride, double dlog2pi, int k,
                                                               double* __restrict__ resp, int32_t* __restrict__ labels,
                                                               double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* tile = lds;                  // [64][D]
  double* sqw = lds + TILE * D;        // [ZK_EWAVES][k][64]
  const bool shared_slots = DP / ZK_EW > ZK_EWAVES;  // two blocks per slot (D <= 127 < ZK_EW * 2 * ZK_EWAVES)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* mine = sqw + (long long)wave * k * 64;
  const ZK_CONST int* my_plan = (const ZK_CONST int*)plan + wave * plan_stride;
  const int n_mine = my_plan[0];
  const int n_gran = 32 * D;
  double lse_sum = 0.0;
  for (long long t = blockIdx.x; t * TILE < N; t += gridDim.x) {
    __syncthreads();  // the previous tile and tables are no longer read
    if ((t + 1) * TILE <= N) {
      const char* src = (const char*)(X + t * TILE * D);
      for (int q = wave; q * 64 < n_gran; q += ZK_EWAVES) {
        const int g = q * 64 + lane;
        if (g < n_gran) __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR(src + (long long)g * 16), ZK_LDS_PTR((char*)tile + q * 1024), 16, 0, 2);
      }
    } else {
      const long long base = t * TILE * D, total = N * D;
      for (int q = wave; q < D; q += ZK_EWAVES) {
        const long long e = base + (long long)q * TILE + lane;
        tile[q * TILE + lane] = e < total ? X[e] : 0.0;
      }
    }
    for (int c = 0; c < k; ++c) mine[c * 64 + lane] = 0.0;  // wave w clears slot w
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const double* row = tile + lane * D;
    for (int p = 0; p < n_mine; ++p) {
      const int c = my_plan[1 + 2 * p], j0 = my_plan[2 + 2 * p];
      const ZK_CONST double* pc = zk_const(P) + (long long)c * D * DP;
      const ZK_CONST double* bc = zk_const(B) + (long long)c * DP;
      // ZK_EW columns of y at a time; row i of the factor (ZK_EW wave-uniform doubles) and x_i are requested one step ahead
      // of their FMAs (the scalar-operand pipelining of zk_sep.h: wait for this step's operands, request the next, compute).
      // The prefetch past the last row reads the next component's first row / the table that follows: in bounds.
      double a[ZK_EW], Pn[ZK_EW];
      const ZK_CONST double* pr = pc + j0;
#pragma unroll
      for (int jj = 0; jj < ZK_EW; ++jj) a[jj] = -bc[j0 + jj], Pn[jj] = pr[jj];
      double xn = row[0];
      const int imax = j0 + ZK_EW < D ? j0 + ZK_EW : D;
#define ZK_ESTEP(NEXT)                                                                    \
  {                                                                                       \
    ZK_LGKM_WAIT();                                                                       \
    const double x = xn;                                                                  \
    double Pc[ZK_EW];                                                                     \
    _Pragma("unroll") for (int jj = 0; jj < ZK_EW; ++jj) Pc[jj] = Pn[jj];                 \
    xn = row[i + (NEXT)];                                                                 \
    _Pragma("unroll") for (int jj = 0; jj < ZK_EW; ++jj) Pn[jj] = pr[(NEXT)*DP + jj];     \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    _Pragma("unroll") for (int jj = 0; jj < ZK_EW; ++jj) a[jj] = __builtin_fma(x, Pc[jj], a[jj]); \
  }
      int i = 0;
      for (; i + 3 < imax; i += 4) {
        ZK_ESTEP(1)
        ZK_ESTEP(2)
        ZK_ESTEP(3)
        ZK_ESTEP(4)
        pr += 4 * DP;
      }
      for (; i < imax; ++i) {
        ZK_ESTEP(1)
        pr += DP;
      }
#undef ZK_ESTEP
      ZK_LGKM_WAIT();
      double sq = 0.0;
#pragma unroll
      for (int jj = 0; jj < ZK_EW; ++jj) sq = __builtin_fma(a[jj], a[jj], sq);
      // every (c, j0) pair is in exactly one wave's plan
      double* slot = sqw + ((long long)((j0 / ZK_EW) & (ZK_EWAVES - 1)) * k + c) * 64 + lane;
      if (shared_slots) (void)__hip_atomic_fetch_add(slot, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else *slot = sq;
    }
    __syncthreads();
    // weighted log probabilities of the 64 rows (every wave), log-sum-exp, outputs split by component / wave
    double best = -std::numeric_limits<double>::infinity();
    int bl = 0;
    for (int c = 0; c < k; ++c) {
      double sq = 0.0;
#pragma unroll
      for (int w = 0; w < ZK_EWAVES; ++w) sq += sqw[((long long)w * k + c) * 64 + lane];
      const ZK_CONST double* cc = zk_const(cst) + 2 * c;
      const double v = (-0.5 * (dlog2pi + sq) + cc[0]) + cc[1];
      if (v > best) best = v, bl = c;
    }
    double s = 0.0;
    for (int c = 0; c < k; ++c) {
      double sq = 0.0;
#pragma unroll
      for (int w = 0; w < ZK_EWAVES; ++w) sq += sqw[((long long)w * k + c) * 64 + lane];
      const ZK_CONST double* cc = zk_const(cst) + 2 * c;
      s += exp(((-0.5 * (dlog2pi + sq) + cc[0]) + cc[1]) - best);
    }
    const double lse = log(s) + best;
    const long long r = t * TILE + lane;
    if (r < N) {
      if (wave == 0) {
        lse_sum += lse;
        if (labels) labels[r] = bl;
      }
      if (resp)
        for (int c = wave; c < k; c += ZK_EWAVES) {
          double sq = 0.0;
#pragma unroll
          for (int w = 0; w < ZK_EWAVES; ++w) sq += sqw[((long long)w * k + c) * 64 + lane];
          const ZK_CONST double* cc = zk_const(cst) + 2 * c;
          __builtin_nontemporal_store(exp(((-0.5 * (dlog2pi + sq) + cc[0]) + cc[1]) - lse), resp + (long long)c * N + r);
        }
    }
  }
  if (wave == 0) {
    const double tot = wave_sum(lse_sum);
    if (lane == 0) part[blockIdx.x] = tot;
  }
}

// ---- E step on the matrix cores (round 3): y = x P_c as  (16 rows x D) . (D x 16-column blocks of the factor) -------------------
// Round 2's attempt above lost because every lane fetched its own element of the factor from global memory.  Here the factors
// of ALL components sit in LDS for the life of the workgroup, already in the MFMA operand order --
//   tabP[c][bj][s][lane] = P_c[4 s + (lane >> 4)][16 bj + (lane & 15)],  s < 4 (bj + 1)   (upper triangle; zeros elsewhere)
// (24 steps x 512 B = 12 KiB per component at D <= 48) -- so a B operand is one conflict-free ds_read_b64, and the eight waves
// of a workgroup (two per SIMD, one workgroup per CU) stream their OWN 16-row blocks of the matrix: the block is DMA'd into a
// wave-private 16 x D buffer, its A operands A[i][k] = x_{row i}[4 s + k] are pulled into registers once (all components and
// column blocks reuse them), and the DMA of the wave's next block is issued straight away -- no barrier after the table load.
// Per (component, column block): one accumulator chain (initialised with -mu P, so the result is y), then sq += y^2; per
// component a 16-lane row reduction (DPP) and four lanes park the four row sums in a wave-private table; the epilogue runs with
// lane = (row, slot): slot s takes the exponentials of the components c = s (mod 4).
// FULL: every piece of the upper triangle ('full' / 'tied' factors); else only the four diagonal pieces of a column block
// ('diag' / 'spherical' factors: the host looks at the factors it was given).
template <int NB, bool FULL, int NW>
__global__ __launch_bounds__(64 * NW) void estep_mfma_kernel(const double* __restrict__ X, long long N, int D, const double* __restrict__ tabP,
                                                            const double* __restrict__ tabB /* [k][NB][16]: -mu P */,
                                                            const double* __restrict__ cst, double dlog2pi, int k,
                                                            double* __restrict__ resp, int32_t* __restrict__ labels,
                                                            double* __restrict__ part) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  constexpr int NS = 4 * NB;                  // feature steps of a row block
  constexpr int PSTEPS = 2 * NB * (NB + 1);   // operand pieces per component
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int li = lane & 15, kr = lane >> 4;
  double* const ptab = lds;                                   // [k][PSTEPS][64]
  double* const btab = ptab + (long long)k * PSTEPS * 64;     // [k][NB][16]
  double* const mine = btab + k * NB * 16 + wave * (16 * D + 4 + 16 * 8);  // this wave's row block [16][D] (+ pad), then sq [8 slots][16]
  double* const sqt = mine + 16 * D + 4;
  {  // the factor table: one cooperative copy
    const long long n = (long long)k * PSTEPS * 64 + k * NB * 16;
    for (long long e = threadIdx.x; e < n; e += 64 * NW) lds[e] = e < (long long)k * PSTEPS * 64 ? tabP[e] : tabB[e - (long long)k * PSTEPS * 64];
  }
  const long long n_blocks = (N + 15) / 16, stride = (long long)gridDim.x * NW;
  long long b = (long long)blockIdx.x * NW + wave;
  const int n_gran = 8 * D;  // 16-byte granules of a block
  auto issue = [&](long long bb) {
    if ((bb + 1) * 16 > N) return;  // the ragged last block is copied with ordinary loads
    const char* src = (const char*)(X + bb * 16 * D);
    for (int q = 0; q * 64 < n_gran; ++q) {
      const int g = q * 64 + lane;
      if (g < n_gran) __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR(src + (long long)g * 16), ZK_LDS_PTR((char*)mine + q * 1024), 16, 0, 2);
    }
  };
  if (b < n_blocks) issue(b);
  __syncthreads();  // the table is in place (the only barrier)
  const ZK_CONST double* cc = zk_const(cst);
  double lse_sum = 0.0;
  for (; b < n_blocks; b += stride) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((b + 1) * 16 > N) {
      const long long base = b * 16 * D, total = N * D;
      for (int e = lane; e < 16 * D; e += 64) mine[e] = base + e < total ? X[base + e] : 0.0;
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    double a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int f = 4 * s + kr;
      a[s] = mine[li * D + (f < D ? f : 0)];
      if (f >= D) a[s] = 0.0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the block is in registers: its buffer can take the next one
    if (b + stride < n_blocks) issue(b + stride);
    for (int c = 0; c < k; ++c) {
      const double* __restrict__ pc = ptab + ((long long)c * PSTEPS) * 64 + lane;
      double sq[4] = {0.0, 0.0, 0.0, 0.0};
      v4d acc[NB];  // the NB chains back to back, their results read afterwards: one wait for the matrix pipe per component
#pragma unroll
      for (int bj = 0; bj < NB; ++bj) {
        const double nb = btab[(c * NB + bj) * 16 + li];
        acc[bj] = v4d{nb, nb, nb, nb};
        const double* __restrict__ pb = pc + (2 * bj * (bj + 1)) * 64;  // pieces of the column blocks before bj: 4 (1 + .. + bj)
#pragma unroll
        for (int s = FULL ? 0 : 4 * bj; s < 4 * (bj + 1); ++s) acc[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], pb[s * 64], acc[bj], 0, 0, 0);
      }
#pragma unroll
      for (int bj = 0; bj < NB; ++bj)
#pragma unroll
        for (int q = 0; q < 4; ++q) sq[q] = __builtin_fma(acc[bj][q], acc[bj][q], sq[q]);
      // sum over the 16 columns a lane group holds (rows kr + 4 q), halving the number of values a lane carries at each of the
      // first two steps: lane pairs (xor 1) split q {0, 1} | {2, 3}, pairs of pairs (xor 2) split again, then two row
      // rotations (by 4 and 8 lanes) -- 5 additions instead of 16; lane li ends with the whole sum of q = 2 (li & 1) + ((li >> 1) & 1)
      {
        const bool hi1 = li & 1, hi2 = li & 2;
        const double keep0 = hi1 ? sq[2] : sq[0], keep1 = hi1 ? sq[3] : sq[1];      // what this lane goes on with
        const double give0 = hi1 ? sq[0] : sq[2], give1 = hi1 ? sq[1] : sq[3];      // what its partner goes on with
        const double a0 = keep0 + zk_dpp_f64<0xB1>(give0), a1 = keep1 + zk_dpp_f64<0xB1>(give1);
        const double keep = hi2 ? a1 : a0, give = hi2 ? a0 : a1;
        double t = keep + zk_dpp_f64<0x4E>(give);
        t += zk_dpp_f64<0x124>(t);  // row_ror:4 and :8 -- the other three quads' lanes with the same li & 3
        t += zk_dpp_f64<0x128>(t);
        if (li < 4) sqt[c * 16 + kr + 4 * (2 * (li & 1) + (li >> 1))] = t;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- epilogue: lane = (row li, slot kr) ---------------------------------------------------------------------------------
    double best = -std::numeric_limits<double>::infinity();
    int bl = 0;
    for (int c = 0; c < k; ++c) {
      const double v = (-0.5 * (dlog2pi + sqt[c * 16 + li]) + cc[2 * c]) + cc[2 * c + 1];
      if (v > best) best = v, bl = c;
    }
    double ssum = 0.0, e0 = 0.0, e1 = 0.0;  // this slot's (at most two: k <= 8) exponentials
    for (int c = kr, n = 0; c < k; c += 4, ++n) {
      const double e = exp(((-0.5 * (dlog2pi + sqt[c * 16 + li]) + cc[2 * c]) + cc[2 * c + 1]) - best);
      ssum += e;
      if (n == 0) e0 = e;
      else e1 = e;
    }
    ssum += __shfl_xor(ssum, 16, 64);
    ssum += __shfl_xor(ssum, 32, 64);
    const double lse = log(ssum) + best;
    const double inv = 1.0 / ssum;  // resp_c = exp(v_c - lse) = exp(v_c - best) / sum
    const long long r = b * 16 + li;
    if (r < N) {
      if (kr == 0) {
        lse_sum += lse;
        if (labels) labels[r] = bl;
      }
      if (resp) {
        if (kr < k) __builtin_nontemporal_store(e0 * inv, resp + (long long)kr * N + r);
        if (kr + 4 < k) __builtin_nontemporal_store(e1 * inv, resp + (long long)(kr + 4) * N + r);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // sqt is read before the next block's sums overwrite it
  }
  // one partial sum per workgroup (waves in order)
  const double tot = wave_sum(lse_sum);
  __syncthreads();
  if (lane == 0) lds[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < NW; ++w) t += lds[w];
    part[blockIdx.x] = t;
  }
}

// resp[c][r] = (labels[r] == c)
__global__ __launch_bounds__(256) void onehot_kernel(const int32_t* __restrict__ labels, long long N, int k, double* __restrict__ resp) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int l = labels[r];
  for (int c = 0; c < k; ++c) resp[(long long)c * N + r] = l == c ? 1.0 : 0.0;
}

// part[block][group][c] = sum over the group's rows of w_cr [x_r - shift | 1]^T [x_r - shift | 1]  (D+1 x D+1; upper triangle
// written, mirrored) for C consecutive planes w_c of the responsibilities (unit weights when w is null).  The (4T x 4T)-padded
// matrix is cut into 4 x 4 register tiles; only the T (T + 1) / 2 tiles of the upper triangle are computed, one per thread, and
// the threads of a workgroup form G groups of that many that share the LDS-staged 64-row tile and take every G-th row of it.
// C components per pass share the staging of the tile and the LDS reads of its rows (the kernel is bound by those, not by the
// FMAs): one component per pass 0.59 ms each on 4 M x 45, three per pass: see profiles/r02_cluster_kernel_stats.csv.
template <int C>
__global__ __launch_bounds__(1024) void wgram_kernel(const double* __restrict__ X, long long N, int D, int T, int G,
                                                     const double* __restrict__ shift, const double* __restrict__ w,
                                                     double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double tile[];  // [64][4T + 4] then [C][64] weights
  const int P = 4 * T + 4, n_ut = T * (T + 1) / 2;  // + 4: a pitch of 4T doubles puts every other row on the same LDS banks
  double* wt = tile + 64 * P;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int g = tid / n_ut, u = tid - g * n_ut;
  const bool worker = g < G;
  int ti = 0, rem = u;
  while (rem >= T - ti) rem -= T - ti, ++ti;
  const int tj = ti + rem;
  double acc[C][4][4];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[c][a][b] = 0.0;
  // columns D .. P-1 never change: the constant 1, then zero padding
  for (int e = tid; e < 64 * (P - D); e += nthreads) {
    const int r = e / (P - D), c = D + e - r * (P - D);
    tile[r * P + c] = c == D ? 1.0 : 0.0;
  }
  const long long total = N * D;
  const int adv_r = nthreads / D, adv_c = nthreads - adv_r * D;
  for (long long r0 = (long long)blockIdx.x * 64; r0 < N; r0 += (long long)gridDim.x * 64) {
    __syncthreads();
    {  // the tile's 64 * D contiguous doubles, eight coalesced loads in flight per thread
      int r = tid / D, c = tid - r * D;
      const long long base = r0 * D;
      for (int e0 = tid; e0 < 64 * D; e0 += 8 * nthreads) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int e = e0 + q * nthreads;
          v[q] = e < 64 * D && base + e < total ? __builtin_nontemporal_load(X + base + e) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (e0 + q * nthreads < 64 * D) tile[r * P + c] = v[q] - shift[c];
          r += adv_r, c += adv_c;
          if (c >= D) c -= D, ++r;
        }
      }
    }
    for (int e = tid; e < 64 * C; e += nthreads) {
      const int c = e >> 6, r = e & 63;
      wt[e] = r0 + r < N ? (w ? w[(long long)c * N + r0 + r] : 1.0) : 0.0;
    }
    __syncthreads();
    if (worker) {
#pragma unroll 2
      for (int r = g; r < 64; r += G) {
        const double* row = tile + r * P;
        double xi[4], xj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = row[4 * ti + a], xj[a] = row[4 * tj + a];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double wr = wt[c * 64 + r];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double xw = xi[a] * wr;
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[c][a][b] = __builtin_fma(xw, xj[b], acc[c][a][b]);
          }
        }
      }
    }
  }
  if (worker) {
    const int D1 = D + 1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double* out = part + (((long long)blockIdx.x * G + g) * C + c) * D1 * D1;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = 4 * ti + a, j = 4 * tj + b;
          if (i < D1 && j < D1 && i <= j) {
            out[i * D1 + j] = acc[c][a][b];
            if (i != j) out[j * D1 + i] = acc[c][a][b];
          }
        }
    }
  }
}

// The same sums on the matrix cores (D + 1 <= 48, i.e. the 45 moments of n_max 8 and below): S_c = sum_r w_cr z_r z_r^T is a
// symmetric rank-N update -- GEMM-shaped work -- and v_mfma_f64_16x16x4_f64 takes both of its operands straight from LDS: one
// double per lane per operand for 2 048 flops, where the register-tiled kernel above reads eight doubles per 32 flops and is
// bound by those reads.  All components of a call (KC <= 8) are done in ONE pass over the matrix.
//   A wave owns ONE of the six 16 x 16 blocks (bi <= bj) of the 48 x 48-padded upper triangle for the whole kernel, with KC
//   accumulators (4 doubles per lane each), and walks every n-th 64-row tile.  It fetches what IT needs of a tile itself -- the
//   16 columns of block column bi (and of bj) as two 8-KiB planes [64 rows][16 doubles], and the KC x 64 weights -- with the
//   LDS-DMA engine into a slab of its own: no workgroup barrier exists (a wave only reads LDS bytes it DMA'd itself), every wave
//   does the same work, and while one wave of a SIMD waits for its tile the other one's MFMAs run.  (A column block is fetched
//   by three or four waves: L2 traffic, HBM still sees the matrix once.)
//   k dimension = rows: step s uses rows 4s .. 4s + 3: A[i][k] = z_{4s+k}[16 bi + i], B[k][j] = w_c[4s+k] z_{4s+k}[16 bj + j]
//   (lane l: i = j = l & 15, k = l >> 4; tools/micro_mfma64.hip verified the layout).  A plane's row pitch of 128 B puts the
//   four rows of a step on disjoint halves of the LDS banks.
//   Measured, six components of 4 M x 45: register-tiled kernel 2.84 ms (two passes of three); this kernel 1.38 ms
//   (53 TFLOP/s of MFMA work).
//   What bounds it: SQ_VALU_MFMA_BUSY_CYCLES = 0.70 of the kernel's SIMD cycles at a measured 2.35 GHz -- and the same 0.70 in
//   three differently organised versions (barrier per tile pair; this one; this one with 32-row stages double-buffered per
//   wave: 1.43 / 1.38 / 1.48 ms for six components).  On this chip the float64 MFMA and the float64 vector pipe have the
//   same peak (78.6 TFLOP/s) and evidently do not overlap: the ~14 vector instructions a step needs beside its KC MFMAs (the
//   weight products, the shift, address updates) take their share of the same cycles.
template <int KC>
__global__ __launch_bounds__(256, 2) void wgram_mfma_kernel(const double* __restrict__ X, long long N, int D, int sets,
                                                            const double* __restrict__ shift, const double* __restrict__ w,
                                                            double* __restrict__ part) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  constexpr int SLAB = 2 * TILE * 16 + KC * TILE;  // doubles per wave: plane A, plane Z, weights
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long gw = (long long)blockIdx.x * 4 + wv;  // global wave index: set = gw / 6 walks tiles set, set + sets, ...
  const int blk = (int)(gw % 6);
  const long long set = gw / 6;
  if (set >= sets) return;  // (no barrier in this kernel)
  const int bi = blk < 3 ? 0 : blk < 5 ? 1 : 2, bj = blk < 3 ? blk : blk < 5 ? blk - 2 : 2;
  double* const pa = lds + wv * SLAB;
  double* const pz = bi == bj ? pa : pa + TILE * 16;
  double* const pw = pa + 2 * TILE * 16;
  const int ci = 16 * bi + (lane & 15), cj = 16 * bj + (lane & 15), kr = lane >> 4;
  const bool in_i = ci < D, in_j = cj < D;
  const double one_i = ci == D ? 1.0 : 0.0, one_j = cj == D ? 1.0 : 0.0;  // the constant column of [x | 1], then zero padding
  const double si = in_i ? shift[ci] : 0.0, sj = in_j ? shift[cj] : 0.0;
  v4d acc[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) acc[c] = v4d{0.0, 0.0, 0.0, 0.0};

  const long long n_tiles = (N + TILE - 1) / TILE;
  // DMA addressing of a plane: position p = q * 64 + lane (q = 0 .. 7) is granule g = p & 7 (two columns) of row p >> 3; a
  // granule is fetched when its first column exists (its second one may be the next row's first element: never used).  The
  // last tile goes through ordinary loads (rows past the end as zeros; and a DMA of its last row could read past the matrix).
  const int g = lane & 7, rq = lane >> 3;
  const bool ga = 16 * bi + 2 * g < D, gz = 16 * bj + 2 * g < D;
  for (long long t = set; t < n_tiles; t += sets) {
    const long long r0 = t * TILE;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slab is no longer read
    if (t + 1 < n_tiles) {
      const char* rowp = (const char*)(X + (r0 + rq) * D);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const char* src = rowp + (long long)q * 8 * D * 8;
        if (ga) __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR(src + (16 * bi + 2 * g) * 8), ZK_LDS_PTR((char*)pa + q * 1024), 16, 0, 0);
        if (bi != bj && gz)
          __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR(src + (16 * bj + 2 * g) * 8), ZK_LDS_PTR((char*)pz + q * 1024), 16, 0, 0);
      }
      if (w) {
#pragma unroll
        for (int q = 0; q * 64 < KC * 32; ++q) {
          const int p = q * 64 + lane;  // granule p of the [KC][64] weights: component p / 32, rows 2 (p % 32)
          if (p < KC * 32)
            __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR((const char*)(w + (long long)(p >> 5) * N + r0) + (p & 31) * 16),
                                             ZK_LDS_PTR((char*)pw + q * 1024), 16, 0, 0);
        }
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) pw[c * TILE + lane] = 1.0;
      }
    } else {
      for (int e = lane; e < TILE * 16; e += 64) {
        const long long r = r0 + (e >> 4);
        const int c1 = 16 * bi + (e & 15), c2 = 16 * bj + (e & 15);
        pa[e] = r < N && c1 < D ? X[r * D + c1] : 0.0;
        if (bi != bj) pz[e] = r < N && c2 < D ? X[r * D + c2] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) pw[c * TILE + lane] = r0 + lane < N ? (w ? w[(long long)c * N + r0 + lane] : 1.0) : 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    // operands of step s + 1 are read while the MFMAs of step s run (branch-free: the constant columns are selected afterwards).
    // (Round 3 also tried one accumulator chain per component -- the fast form of tools/micro_mfma64_occ.hip -- with the tile's 16
    //  operand pairs kept in registers: 1.41 ms against 1.39 for six components; the weight products, not the chain order, are
    //  what the MFMAs wait for here.)
    const double* ta = pa + kr * 16 + (lane & 15);
    const double* tz = pz + kr * 16 + (lane & 15);
    const double* wt = pw + kr;
    double a_n = ta[0], z_n = tz[0], w_n[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) w_n[c] = wt[c * TILE];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double a = in_i ? a_n - si : one_i;
      const double z = bi == bj ? a : (in_j ? z_n - sj : one_j);
      double wz[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) wz[c] = w_n[c] * z;
      if (s + 1 < 16) {
        a_n = ta[(s + 1) * 64];
        z_n = tz[(s + 1) * 64];
#pragma unroll
        for (int c = 0; c < KC; ++c) w_n[c] = wt[c * TILE + (s + 1) * 4];
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wz[c], acc[c], 0, 0, 0);
    }
  }
  // this wave's partial block: part[set][blk][c][16 x 16] (row (lane >> 4) + 4 q, column lane & 15)
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    double* out = part + (((long long)set * 6 + blk) * KC + c) * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(kr + 4 * q) * 16 + (lane & 15)] = acc[c][q];
  }
}

// out[j] = (mu P)_j of one component, negated on request, in the order of numpy.dot(mu, prec_chol) (P is upper triangular)
void mean_times_factor(const double* mu, const double* pc, int D, bool negate, double* out) {
  for (int j = 0; j < D; ++j) {
    double s = 0.0;
    for (int i = 0; i <= j; ++i) s += mu[i] * pc[(size_t)i * D + j];
    out[j] = negate ? -s : s;
  }
}

// what an E step writes: one partial sum per workgroup, the responsibilities (k, N) when asked for, and the labels
int estep_outputs(zk_rows* m, int grid, int k, int want_resp) {
  int rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)grid * sizeof(double));
  if (rc || (want_resp && (rc = zk_ensure(&m->d_resp, &m->resp_bytes, (size_t)k * m->N * sizeof(double))))) return rc;
  return zk_rows_need_labels(m, false);
}

// E step on the vector pipe (estep_kernel): any D and k.  (This path records no profile events: zk_rows_last_kernel_ms
// keeps the time of the last profiled pass.)
int estep_valu(zk_rows* m, const double* prec_chol, const double* means, const double* log_det, const double* log_w, int k,
               int want_resp, double* lse_sum_out) {
  const int D = m->D, DP = (D + ZK_EW - 1) / ZK_EW * ZK_EW, n_blk = DP / ZK_EW;
  // the (component, column block) pairs, dealt to the waves: longest first, each to the least loaded wave
  const int plan_stride = 1 + 2 * k * n_blk;
  std::vector<int> plan((size_t)ZK_EWAVES * plan_stride, 0);
  {
    long long load[ZK_EWAVES] = {0};
    for (int jb = n_blk - 1; jb >= 0; --jb)
      for (int c = 0; c < k; ++c) {
        int w = 0;
        for (int v = 1; v < ZK_EWAVES; ++v)
          if (load[v] < load[w]) w = v;
        int* mine = plan.data() + (size_t)w * plan_stride;
        mine[1 + 2 * mine[0]] = c;
        mine[2 + 2 * mine[0]] = jb * ZK_EW;
        ++mine[0];
        load[w] += std::min(D, (jb + 1) * ZK_EW) + 4;
      }
  }
  const size_t plan_doubles = (plan.size() * sizeof(int) + 7) / 8;
  std::vector<double>& h = m->h_buf;
  h.assign((size_t)k * D * DP + (size_t)k * DP + 2 * (size_t)k + plan_doubles, 0.0);
  double* P = h.data();
  double* B = P + (size_t)k * D * DP;
  double* C = B + (size_t)k * DP;
  memcpy(C + 2 * (size_t)k, plan.data(), plan.size() * sizeof(int));
  for (int c = 0; c < k; ++c) {
    const double* pc = prec_chol + (size_t)c * D * D;
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) P[((size_t)c * D + i) * DP + j] = pc[(size_t)i * D + j];
    mean_times_factor(means + (size_t)c * D, pc, D, false, B + (size_t)c * DP);
    C[2 * c] = log_det[c];
    C[2 * c + 1] = log_w[c];
  }
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  const size_t lds = (size_t)TILE * D * sizeof(double) + (size_t)ZK_EWAVES * k * 64 * sizeof(double);
  if ((rc = zk_check_lds(lds))) return rc;
  int per_cu = (int)std::min<size_t>((160 * 1024) / (lds + 512), (size_t)(32 / ZK_EWAVES));
  per_cu = std::max(1, per_cu);
  const int grid = (int)std::min<long long>((m->N + TILE - 1) / TILE, (long long)per_cu * m->n_cu);
  if ((rc = estep_outputs(m, grid, k, want_resp))) return rc;
  const double* tab = (const double*)m->d_tab;
  const double* d_cst = tab + (size_t)k * D * DP + (size_t)k * DP;
  rc = zk_launch_lds(estep_kernel, m, dim3(grid), dim3(64 * ZK_EWAVES), lds, m->X, (long long)m->N, D, DP, tab, tab + (size_t)k * D * DP,
                     d_cst, (const int*)(d_cst + 2 * (size_t)k), plan_stride, (double)D * std::log(2.0 * M_PI), k,
                     want_resp ? (double*)m->d_resp : nullptr, m->d_labels, (double*)m->d_part);
  return rc ? rc : zk_reduce_to_host(m, grid, 1, lse_sum_out);
}

// E step on the matrix cores (estep_mfma_kernel; D <= 48, k <= 8: the factors of all components fit the LDS of a CU beside the
// waves' row blocks)
int estep_mfma(zk_rows* m, const double* prec_chol, const double* means, const double* log_det, const double* log_w, int k,
               int want_resp, double* lse_sum_out) {
  const int D = m->D, NB = (D + 15) / 16, psteps = 2 * NB * (NB + 1);
  bool diag = true;  // only the diagonal pieces hold anything: 'diag' / 'spherical' factors
  for (int c = 0; c < k && diag; ++c)
    for (int i = 0; i < D && diag; ++i)
      for (int j = i; j < D; ++j)
        if (prec_chol[((size_t)c * D + i) * D + j] != 0.0 && i / 16 != j / 16) {
          diag = false;
          break;
        }
  std::vector<double>& h = m->h_buf;
  h.assign((size_t)k * psteps * 64 + (size_t)k * NB * 16 + 2 * (size_t)k, 0.0);
  double* TP = h.data();
  double* TB = TP + (size_t)k * psteps * 64;
  double* TC = TB + (size_t)k * NB * 16;
  for (int c = 0; c < k; ++c) {
    const double* pc = prec_chol + (size_t)c * D * D;
    for (int bj = 0; bj < NB; ++bj)
      for (int s = 0; s < 4 * (bj + 1); ++s)
        for (int l = 0; l < 64; ++l) {
          const int i = 4 * s + (l >> 4), j = 16 * bj + (l & 15);
          TP[((size_t)c * psteps + 2 * bj * (bj + 1) + s) * 64 + l] = i < D && j < D && i <= j ? pc[(size_t)i * D + j] : 0.0;
        }
    mean_times_factor(means + (size_t)c * D, pc, D, true, TB + (size_t)c * NB * 16);
    TC[2 * c] = log_det[c];
    TC[2 * c + 1] = log_w[c];
  }
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  // twelve waves per workgroup (three per SIMD) while the factors and the waves' row blocks fit a CU's LDS, else eight: the
  // chains are 4 / 8 / 12 MFMAs long, and short dependent chains gain from a third wave (tools/micro_mfma64_chain.hip)
  const size_t lds_tab = ((size_t)k * psteps * 64 + (size_t)k * NB * 16) * sizeof(double);
  const size_t lds_wave = ((size_t)16 * D + 4 + 128) * sizeof(double);
  const int nw = lds_tab + 12 * lds_wave <= 160 * 1024 ? 12 : 8;
  const size_t lds = lds_tab + nw * lds_wave;
  if ((rc = zk_check_lds(lds))) return rc;
  const long long n_blocks = (m->N + 15) / 16;
  const int grid = (int)std::min<long long>((n_blocks + nw - 1) / nw, (long long)m->n_cu);
  if ((rc = estep_outputs(m, grid, k, want_resp))) return rc;
  const double* tab = (const double*)m->d_tab;
  const double* d_tb = tab + (size_t)k * psteps * 64;
  const double* d_tc = d_tb + (size_t)k * NB * 16;
  rc = zk_with_int<1, 2, 3>(NB, [&](auto nb) {
    return zk_with_int<0, 1>(diag ? 0 : 1, [&](auto full) {
      return zk_with_int<8, 12>(nw, [&](auto nwv) {
        return zk_launch_profiled(estep_mfma_kernel<nb, (full != 0), nwv>, m, dim3(grid), dim3(64 * nwv), lds, m->X, (long long)m->N, D,
                                  tab, d_tb, d_tc, (double)D * std::log(2.0 * M_PI), k, want_resp ? (double*)m->d_resp : nullptr,
                                  m->d_labels, (double*)m->d_part);
      });
    });
  });
  if (rc || (rc = zk_reduce_to_host(m, grid, 1, lse_sum_out))) return rc;
  return zk_rows_prof_read(m);
}

}  // namespace

// E step with the upper-triangular precision Cholesky factors prec_chol (k, D, D), means (k, D), log-determinants and log
// weights (k each).  Writes the responsibilities (k, N) and the labels (first argmax) on the device;
// lse_sum_out = sum_r logsumexp_c(weighted log prob).
extern "C" int zk_gmm_estep(zk_rows* m, const double* prec_chol, const double* means, const double* log_det, const double* log_w, int k,
                            int want_resp, double* lse_sum_out) {
  if (!m || !prec_chol || !means || !log_det || !log_w || !lse_sum_out) return zk_fail(ZK_E_BADARG, "null pointer");
  if (k < 1 || k > 64) return zk_fail(ZK_E_BADARG, "1 to 64 mixture components");
  ZK_ON_DEVICE(m->device);
  // matrix-core form unless ZK_ESTEP_VALU asks for the scalar-operand kernel (A/B runs)
  if ((m->D + 15) / 16 <= 3 && k <= 8 && m->D >= 2 && !zk_switch_on(ZK_ESTEP_VALU))
    return estep_mfma(m, prec_chol, means, log_det, log_w, k, want_resp, lse_sum_out);
  return estep_valu(m, prec_chol, means, log_det, log_w, k, want_resp, lse_sum_out);
}

// responsibilities = one-hot of the current labels (the k-means initialisation of the mixture)
extern "C" int zk_gmm_resp_from_labels(zk_rows* m, int k) {
  if (!m || k < 1 || k > 64) return zk_fail(ZK_E_BADARG, "bad arguments");
  if (!m->d_labels) return zk_fail(ZK_E_BADARG, "no labels yet");
  ZK_ON_DEVICE(m->device);
  int rc = zk_ensure(&m->d_resp, &m->resp_bytes, (size_t)k * m->N * sizeof(double));
  if (rc) return rc;
  return zk_launch_lds(onehot_kernel, m, dim3((unsigned)((m->N + 255) / 256)), dim3(256), 0, (const int32_t*)m->d_labels, (long long)m->N,
                       k, (double*)m->d_resp);
}

// sum_r w_cr [x_r - shift | 1]^T [x_r - shift | 1] for `count` (1 to 3) consecutive planes of the responsibilities starting at
// w_dev, or with unit weights (w_dev null, count 1); gram_out (count, D+1, D+1)
static int rows_gram(zk_rows* m, const double* w_dev, int count, const double* shift, double* gram_out) {
  const int D = m->D, D1 = D + 1, T = (D1 + 3) / 4, n_ut = T * (T + 1) / 2;
  m->h_buf.assign(shift, shift + D);
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  const bool no_mfma = zk_switch_on(ZK_WGRAM_VALU);  // A/B runs: the register-tiled kernel
  if (D1 <= 48 && D >= 2 && !no_mfma) {
    // matrix-core form: every component of the call in one pass; `sets` groups of six waves (one per block of the triangle),
    // each set walking its share of the tiles
    const size_t lds = (size_t)4 * (2 * TILE * 16 + count * TILE) * sizeof(double);
    const long long n_tiles = (m->N + TILE - 1) / TILE;
    const long long sets = std::max<long long>(1, std::min<long long>(n_tiles, (long long)m->n_cu * 8 / 6));
    const long long waves = sets * 6, blocks = (waves + 3) / 4;
    const int n = 6 * count * 256;
    if ((rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)sets * n * sizeof(double)))) return rc;
    rc = zk_with_int<1, 2, 3, 4, 5, 6, 7, 8>(count, [&](auto cc) {
      return zk_launch_profiled(wgram_mfma_kernel<cc>, m, dim3((unsigned)blocks), dim3(256), lds, m->X, (long long)m->N, D, (int)sets,
                                (const double*)m->d_tab, w_dev, (double*)m->d_part);
    });
    if (rc) return rc;
    // fixed-order sum over the sets, then the six blocks are put in place (upper triangle mirrored; inside a diagonal block
    // only i <= j is taken: its two halves differ in the last bit)
    std::vector<double> blocks_sum((size_t)n);
    if ((rc = zk_reduce_to_host(m, (int)sets, n, blocks_sum.data()))) return rc;
    static const int BI[6] = {0, 0, 0, 1, 1, 2}, BJ[6] = {0, 1, 2, 1, 2, 2};
    for (int b = 0; b < 6; ++b)
      for (int c = 0; c < count; ++c) {
        const double* src = blocks_sum.data() + ((size_t)b * count + c) * 256;
        double* dst = gram_out + (size_t)c * D1 * D1;
        for (int i = 0; i < 16; ++i)
          for (int j = 0; j < 16; ++j) {
            const int gi = 16 * BI[b] + i, gj = 16 * BJ[b] + j;
            if (gi < D1 && gj < D1 && gi <= gj) dst[gi * D1 + gj] = dst[gj * D1 + gi] = src[i * 16 + j];
          }
      }
    return zk_rows_prof_read(m);
  }
  if (count > 3) return zk_fail(ZK_E_BADARG, "more than 3 components per pass need D <= 47");
  const int threads = std::max(256, (n_ut + 63) & ~63);
  const int G = std::min(threads / n_ut, 16);
  const size_t lds = ((size_t)64 * (4 * T + 4) + 64 * count) * sizeof(double);
  int per_cu = (int)std::min<size_t>((160 * 1024) / (lds + 512), (size_t)(2048 / threads));
  per_cu = std::max(1, std::min(per_cu, count > 1 ? 4 : 6));
  long long blocks = std::min<long long>((m->N + 63) / 64, (long long)per_cu * m->n_cu);
  if ((rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)blocks * G * count * D1 * D1 * sizeof(double)))) return rc;
  rc = zk_with_int<1, 2, 3>(count, [&](auto cc) {
    return zk_launch_profiled(wgram_kernel<cc>, m, dim3((unsigned)blocks), dim3(threads), lds, m->X, (long long)m->N, D, T, G,
                              (const double*)m->d_tab, w_dev, (double*)m->d_part);
  });
  if (rc || (rc = zk_reduce_to_host(m, (int)(blocks * G), count * D1 * D1, gram_out))) return rc;
  return zk_rows_prof_read(m);
}

// M-step sums about `shift` (D) of `count` (1 to 3) consecutive components starting at c: gram_out (count, D+1, D+1), each
// sum_r resp[c][r] [x_r - shift | 1]^T [x_r - shift | 1] -- second moments, first moments in the last row / column, the
// component's weight in the corner.
extern "C" int zk_gmm_moments(zk_rows* m, int c, int count, const double* shift, double* gram_out) {
  if (!m || !shift || !gram_out) return zk_fail(ZK_E_BADARG, "null pointer");
  if (count < 1 || count > 8 || (count > 3 && m && m->D > 47)) return zk_fail(ZK_E_BADARG, "1 to 8 components per pass (1 to 3 with more than 47 features)");
  if (!m->d_resp || c < 0 || (size_t)(c + count) * m->N * sizeof(double) > m->resp_bytes) return zk_fail(ZK_E_BADARG, "no such component");
  ZK_ON_DEVICE(m->device);
  return rows_gram(m, (const double*)m->d_resp + (size_t)c * m->N, count, shift, gram_out);
}

// The same sums with unit weights: everything a covariance needs (pca), in a fixed summation order.
extern "C" int zk_rows_gram(zk_rows* m, const double* shift, double* gram_out) {
  if (!m || !shift || !gram_out) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(m->device);
  return rows_gram(m, nullptr, 1, shift, gram_out);
}
