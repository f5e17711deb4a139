// zk_eels.hip -- device side of mtflearn.eels (reference eels/_baseline_correction.py): the baseline of every spectrum of a
// spectrum image.
//
//   layout    energy-major (L, N): channel c of spectrum n at [c * N + n] -- (E, H, W), the reference's EELSData layout.  An
//             operand is (outer, L, inner); outer == 1 is that layout as it stands, anything else goes through swap_axes on
//             the way in (widened to float64) and on the way out.
//   mapping   one spectrum per lane; the 64 lanes of a wave hold 64 adjacent spectra, so every access to a channel plane is
//             one 512-byte float64 segment.  A lane reads and writes its own column only: no atomics, and a spectrum's
//             numbers depend neither on its neighbours nor on the chunking.
//
//   snip      v = log(log(sqrt(y + 1) + 1) + 1); niter Jacobi passes v'[e] = min(v[e], (v[e + pp] + v[e - pp]) / 2) on
//             pp <= e < L - pp between two planes (one launch per pass, a pass with 2 pp >= L is skipped: it changes
//             nothing); baseline = (exp(exp(v) - 1) - 1)^2 - 1.
//   pls       (W + lam D^T D) z = W y with D the order-K differences, K = 1 .. 3: a symmetric positive definite band of
//             half-bandwidth K.  eels_pls_kernel<K, MODE> runs the WHOLE reweighting loop of a spectrum in one launch:
//               forward   right-looking band LDL^T fused with the forward substitution: only the pending updates of the
//                         next K columns (K (K + 1) / 2 values) and of the next K right-hand sides live in registers; the K
//                         multipliers and the scaled right-hand side of each channel go to K + 1 float64 scratch planes.
//                         The penalty band lam D^T D (L x (K + 1), built on the host, the same for every lane) is read with
//                         wave-uniform loads.  The weights of the sweep are formed on the fly: 1 (first sweep), the ALS /
//                         airPLS rule on y and the previous z (read back from the output plane), the arPLS weight plane, or
//                         the caller's weights (plain Whittaker).
//               backward  reads the planes in reverse, writes z, and accumulates the statistics of the negative residuals in
//                         registers (airPLS: sum and max; arPLS: Welford mean / variance).
//               arPLS     a third sweep forms the new weights from the finished statistics, accumulates |w - wt|^2 and
//                         |w|^2 and stores wt to the weight plane.
//             A lane that has met its stop rule stops storing; a wave leaves when its 64 lanes are done.
//   latency   the recurrence is a serial chain (one float64 reciprocal per channel); the loads do not depend on it, so both
//             sweeps load the operands of the next ZK_EELS_PF channels before they walk the current ZK_EELS_PF.
//   chunking  N is cut so that the scratch planes stay under the cap (zk_eels_set_chunk, default 1 GiB).
#include <math.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>
#include <vector>

#include "zk_internal.h"
#include "zk_scratch.h"

#ifndef ZK_EELS_PF
#define ZK_EELS_PF 8  // channels loaded ahead of the chain (tools/time_eels.py, profiles/eels.txt)
#endif

namespace {

constexpr int PF = ZK_EELS_PF;
constexpr size_t DEFAULT_CAP = (size_t)1 << 30;
zk_device_bytes g_cap;  // zk_eels_set_chunk: scratch cap per device; 0: DEFAULT_CAP

// ---------------------------------------------------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------------------------------------------------

// (X, Y) -> (Y, X), widened to float64
template <typename T>
__global__ __launch_bounds__(256) void transpose_widen_kernel(const T* __restrict__ in, double* __restrict__ out, long long X, long long Y) {
  __shared__ double tile[64][65];
  const long long by = (long long)blockIdx.x * 64, bx = (long long)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const long long x = bx + r, y = by + tx;
    if (x < X && y < Y) tile[r][tx] = (double)in[x * Y + y];
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const long long y = by + r, x = bx + tx;
    if (x < X && y < Y) out[y * X + x] = tile[tx][r];
  }
}

// (X, Y, B) -> (Y, X, B), widened to float64; lanes along b, then x
template <typename T>
__global__ __launch_bounds__(256) void swap_axes_kernel(const T* __restrict__ in, double* __restrict__ out, long long X, long long Y,
                                                        long long B) {
  const long long total = X * Y * B;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long b = i % B, x = (i / B) % X, y = i / (B * X);
    out[i] = (double)in[(x * Y + y) * B + b];
  }
}

template <typename T>
int swap_axes(const T* in, double* out, long long X, long long Y, long long B, hipStream_t s) {
  if (B == 1) {
    const long long by = (Y + 63) / 64, bx = (X + 63) / 64;
    if (bx > 65535) {  // grid.y is 16 bits wide: the plain form
      hipLaunchKernelGGL(swap_axes_kernel<T>, dim3(std::min<unsigned>(blocks_of(X * Y, 256), 65536)), dim3(256), 0, s, in, out, X, Y, B);
    } else {
      hipLaunchKernelGGL(transpose_widen_kernel<T>, dim3((unsigned)by, (unsigned)bx), dim3(256), 0, s, in, out, X, Y);
    }
  } else {
    hipLaunchKernelGGL(swap_axes_kernel<T>, dim3(std::min<unsigned>(blocks_of(X * Y * B, 256), 65536)), dim3(256), 0, s, in, out, X, Y, B);
  }
  ZK_HIP(hipGetLastError());
  return 0;
}

// A 256-thread block of the plane kernels covers 64 spectra of 4 channels; the channel blocks are strided over grid.y.
struct plane_grid {
  dim3 grid;
  plane_grid(int L, int n) : grid(blocks_of(n, 64), std::min<unsigned>(blocks_of(L, 4), 65535)) {}
};

// out[c * os + n] = f(in[c * is + n]): the widening copy of a chunk (SNIP false) or SNIP's forward transform
template <typename T, bool SNIP>
__global__ __launch_bounds__(256) void load_plane_kernel(const T* __restrict__ in, long long is, double* __restrict__ out, long long os,
                                                         int L, int n) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  if (col >= n) return;
  for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < L; c += gridDim.y * 4) {
    double v = (double)in[(long long)c * is + col];
    if (SNIP) v = log(log(sqrt(v + 1.0) + 1.0) + 1.0);
    out[(long long)c * os + col] = v;
  }
}

__global__ __launch_bounds__(256) void snip_pass_kernel(const double* __restrict__ in, double* __restrict__ out, long long vs, int L, int n,
                                                        int pp) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  if (col >= n) return;
  for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < L; c += gridDim.y * 4) {
    double v = in[(long long)c * vs + col];
    if (c >= pp && c < L - pp) {
      const double r = (in[(long long)(c + pp) * vs + col] + in[(long long)(c - pp) * vs + col]) * 0.5;
      v = r < v ? r : v;
    }
    out[(long long)c * vs + col] = v;
  }
}

__global__ __launch_bounds__(256) void snip_inverse_kernel(const double* __restrict__ in, long long vs, double* __restrict__ out,
                                                           long long os, int L, int n) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  if (col >= n) return;
  for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < L; c += gridDim.y * 4) {
    const double t = exp(exp(in[(long long)c * vs + col]) - 1.0) - 1.0;
    out[(long long)c * os + col] = t * t - 1.0;
  }
}

// signal = data - baseline, both in the caller's layout
template <typename T>
__global__ __launch_bounds__(256) void signal_kernel(const T* __restrict__ data, const double* __restrict__ base, double* __restrict__ sig,
                                                     long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) sig[i] = (double)data[i] - base[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// penalised least squares
// ---------------------------------------------------------------------------------------------------------------------

struct pls_args {
  const double* y;     // (L, .) spectra of the chunk, channel stride ys
  long long ys;
  const double* w;     // ZK_EELS_WHITTAKER: weight of (c, col) at w[c * ws + col * wl]
  long long ws;
  int wl;
  const double* band;  // (L, K + 1): band[c][q] = (lam D^T D)[c + q][c]
  double* fac;         // K + 1 planes (L, fs): the multipliers l[1 .. K], then the scaled right-hand side
  long long fs;
  double* wt;          // ZK_EELS_ARPLS: (L, fs) weights
  double* z;           // (L, .) baselines, channel stride zs
  long long zs;
  int32_t* iters;      // (n) solves per spectrum, or null
  int L, n;
  double p;            // ALS: p; arPLS: ratio
  int itermax;
};

template <int K, int MODE>
__global__ __launch_bounds__(64) void eels_pls_kernel(const pls_args a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const long long col = live ? g : a.n - 1;  // a lane past the end walks the last column and stores nothing
  const int L = a.L;
  const long long ys = a.ys, zs = a.zs, fs = a.fs;
  const long long plane = (long long)L * fs;
  const double* __restrict__ y = a.y + col;
  const double* __restrict__ band = a.band;
  const double* wsrc = MODE == ZK_EELS_WHITTAKER ? a.w + col * a.wl : nullptr;
  double* z = a.z + col;
  double* fac = a.fac + col;
  double* wt = MODE == ZK_EELS_ARPLS ? a.wt + col : nullptr;
  bool run = live;
  int count = 0;
  double sumabs = 0.0, dssn = 1.0, dmax = 0.0;  // airPLS

  for (int it = 0; it < a.itermax; ++it) {
    if (__builtin_amdgcn_ballot_w64(run) == 0) break;
    const bool first = it == 0;

    // ------------------------------------------------------------------------------------------------ forward
    double pend[K][K + 1], rhs[K];  // pend[p][q]: what the columns walked so far subtract from A[c + p + q][c + p]
#pragma unroll
    for (int p = 0; p < K; ++p) {
      rhs[p] = 0.0;
#pragma unroll
      for (int q = 0; q <= K; ++q) pend[p][q] = 0.0;
    }
    const double w_edge = MODE == ZK_EELS_AIRPLS && !first ? exp(((double)it * dmax) / dssn) : 1.0;
    auto load_fwd = [&](int c0, double(&yo)[PF], double(&xo)[PF]) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const long long c = c0 + j < L ? c0 + j : L - 1;
        yo[j] = y[c * ys];
        if (MODE == ZK_EELS_WHITTAKER) xo[j] = wsrc[c * a.ws];
        else if (first) xo[j] = 1.0;
        else if (MODE == ZK_EELS_ARPLS) xo[j] = wt[c * fs];
        else xo[j] = z[c * zs];
      }
    };
    double yb[PF], xb[PF];
    load_fwd(0, yb, xb);
    for (int c0 = 0; c0 < L; c0 += PF) {
      double yn[PF], xn[PF];
      load_fwd(c0 + PF, yn, xn);
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int c = c0 + j;
        if (c < L) {
          const double yv = yb[j], x = xb[j];
          double w;
          if (MODE == ZK_EELS_WHITTAKER || (MODE == ZK_EELS_ARPLS && !first)) {
            w = x;
          } else if (first) {
            w = 1.0;
          } else if (MODE == ZK_EELS_ALS) {
            w = yv > x ? a.p : (yv < x ? 1.0 - a.p : 0.0);
          } else {
            const double d = yv - x;
            w = d < 0.0 ? exp(((double)it * fabs(d)) / dssn) : 0.0;
            if (c == 0 || c == L - 1) w = w_edge;
          }
          if (MODE == ZK_EELS_AIRPLS && first) sumabs += fabs(yv);
          const double* __restrict__ bc = band + (long long)c * (K + 1);
          double cc[K + 1];
          cc[0] = (bc[0] + w) - pend[0][0];
#pragma unroll
          for (int q = 1; q <= K; ++q) cc[q] = bc[q] - pend[0][q];
          const double inv = 1.0 / cc[0];
          double l[K + 1];
#pragma unroll
          for (int m = 1; m <= K; ++m) l[m] = cc[m] * inv;
          const double yi = w * yv - rhs[0];
#pragma unroll
          for (int p = 1; p <= K; ++p) {
#pragma unroll
            for (int q = 0; q <= K; ++q) {
              const double old = p < K ? pend[p < K ? p : 0][q] : 0.0;
              pend[p - 1][q] = q <= K - p ? old + l[p] * cc[p + q <= K ? p + q : K] : 0.0;
            }
            rhs[p - 1] = (p < K ? rhs[p < K ? p : 0] : 0.0) + l[p] * yi;
          }
          if (run) {
#pragma unroll
            for (int m = 1; m <= K; ++m) fac[(m - 1) * plane + c * fs] = l[m];
            fac[K * plane + c * fs] = yi * inv;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        yb[j] = yn[j];
        xb[j] = xn[j];
      }
    }

    // ------------------------------------------------------------------------------------------------ backward
    constexpr bool STATS = MODE == ZK_EELS_ARPLS || MODE == ZK_EELS_AIRPLS;
    double zn[K];  // z[c + 1 .. c + K]; 0 past the end (the multipliers are 0 there as well)
#pragma unroll
    for (int m = 0; m < K; ++m) zn[m] = 0.0;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;                            // arPLS: Welford over the negative residuals
    double dsum = 0.0, dtop = -std::numeric_limits<double>::infinity();  // airPLS: their sum and their maximum
    auto load_bwd = [&](int c0, double(&fo)[PF][K + 1], double(&yo)[PF]) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const long long c = c0 + j < L ? (c0 + j >= 0 ? c0 + j : 0) : L - 1;
#pragma unroll
        for (int m = 0; m <= K; ++m) fo[j][m] = fac[m * plane + c * fs];
        yo[j] = STATS ? y[c * ys] : 0.0;
      }
    };
    double fb[PF][K + 1], yc[PF];
    const int top = ((L - 1) / PF) * PF;
    load_bwd(top, fb, yc);
    for (int c0 = top; c0 >= 0; c0 -= PF) {
      double fn[PF][K + 1], yn[PF];
      load_bwd(c0 - PF, fn, yn);
#pragma unroll
      for (int j = PF - 1; j >= 0; --j) {
        const int c = c0 + j;
        if (c < L) {
          double zc = fb[j][K];
#pragma unroll
          for (int m = 1; m <= K; ++m) zc -= fb[j][m - 1] * zn[m - 1];
#pragma unroll
          for (int m = K - 1; m >= 1; --m) zn[m] = zn[m - 1];
          zn[0] = zc;
          if (run) z[c * zs] = zc;
          if (STATS) {
            const double d = yc[j] - zc;
            if (d < 0.0) {
              if (MODE == ZK_EELS_ARPLS) {
                cnt += 1.0;
                const double delta = d - mean;
                mean += delta / cnt;
                m2 += delta * (d - mean);
              } else {
                dsum += d;
                dtop = d > dtop ? d : dtop;
              }
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        yc[j] = yn[j];
#pragma unroll
        for (int m = 0; m <= K; ++m) fb[j][m] = fn[j][m];
      }
    }

    // ------------------------------------------------------------------------------------------------ stop rules
    if (run) count = it + 1;
    if (MODE == ZK_EELS_ARPLS) {
      const double sd = sqrt(m2 / cnt), thr = 2.0 * sd - mean;
      double num = 0.0, den = 0.0;
#pragma unroll 4
      for (int c = 0; c < L; ++c) {
        const double d = y[c * ys] - z[c * zs];
        const double wn = 1.0 / (1.0 + exp((2.0 * (d - thr)) / sd));
        const double wo = first ? 1.0 : wt[c * fs];
        num += (wo - wn) * (wo - wn);
        den += wo * wo;
        if (run) wt[c * fs] = wn;
      }
      if (sqrt(num) / sqrt(den) < a.p) run = false;
    } else if (MODE == ZK_EELS_AIRPLS) {
      dssn = fabs(dsum);
      dmax = dtop;
      if (dssn < 0.001 * sumabs) run = false;
    }
  }
  if (live && a.iters) a.iters[g] = count;
}

template <int K>
int launch_pls_k(int mode, const pls_args& a, hipStream_t s) {
  const dim3 grid(blocks_of(a.n, 64)), block(64);
  switch (mode) {
    case ZK_EELS_WHITTAKER: hipLaunchKernelGGL((eels_pls_kernel<K, ZK_EELS_WHITTAKER>), grid, block, 0, s, a); break;
    case ZK_EELS_ALS: hipLaunchKernelGGL((eels_pls_kernel<K, ZK_EELS_ALS>), grid, block, 0, s, a); break;
    case ZK_EELS_ARPLS: hipLaunchKernelGGL((eels_pls_kernel<K, ZK_EELS_ARPLS>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((eels_pls_kernel<K, ZK_EELS_AIRPLS>), grid, block, 0, s, a); break;
  }
  ZK_HIP(hipGetLastError());
  return 0;
}

int launch_pls(int order, int mode, const pls_args& a, hipStream_t s) {
  return order == 1 ? launch_pls_k<1>(mode, a, s) : order == 2 ? launch_pls_k<2>(mode, a, s) : launch_pls_k<3>(mode, a, s);
}

// lam D^T D of the order-k differences as (L, k + 1): band[c][q] = entry (c + q, c); integers times lam, the reference's entries
std::vector<double> penalty_band(int L, int k, double lam) {
  double coef[4] = {0, 0, 0, 0};  // row of D: (-1)^(k - j) C(k, j)
  const int binom[4][4] = {{1, 0, 0, 0}, {1, 1, 0, 0}, {1, 2, 1, 0}, {1, 3, 3, 1}};
  for (int j = 0; j <= k; ++j) coef[j] = ((k - j) & 1 ? -1.0 : 1.0) * binom[k][j];
  std::vector<double> band((size_t)L * (k + 1), 0.0);
  for (int c = 0; c < L; ++c)
    for (int q = 0; q <= k && c + q < L; ++q) {
      double sum = 0.0;
      for (int r = std::max(0, c + q - k); r <= std::min(c, L - k - 1); ++r) sum += coef[c - r] * coef[c + q - r];
      band[(size_t)c * (k + 1) + q] = lam * sum;
    }
  return band;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

struct eels_job {
  bool snip = false;
  int mode = 0, order = 2, itermax = 1;  // snip: itermax = niter
  double lam = 0.0, param = 0.0;
  const double* weights = nullptr;       // device; WHITTAKER only
  int weights_per_spectrum = 0;
};

int check_shape(const char* who, const void* data, int dtype, int64_t outer, int64_t length, int64_t inner, const void* baseline) {
  const std::string name(who);
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, name + ": dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (outer < 1 || inner < 1 || length < 1) return zk_fail(ZK_E_BADARG, name + ": outer, length and inner must be positive");
  if (length >= ((int64_t)1 << 24) || outer >= ((int64_t)1 << 31) || inner >= ((int64_t)1 << 31) || outer * inner >= ((int64_t)1 << 31) ||
      outer * inner * length >= ((int64_t)1 << 40))
    return zk_fail(ZK_E_BADARG, name + ": needs length < 2^24, outer * inner < 2^31 and fewer than 2^40 samples");
  if (!data || !baseline) return zk_fail(ZK_E_BADARG, name + ": null pointer");
  return 0;
}

int check_job(const eels_job& j, int64_t length, bool has_weights) {
  if (j.snip) {
    if (j.itermax < 0) return zk_fail(ZK_E_BADARG, "eels_snip: niter must be >= 0");
    return 0;
  }
  if (j.mode < ZK_EELS_WHITTAKER || j.mode > ZK_EELS_AIRPLS) return zk_fail(ZK_E_BADARG, "eels_pls: mode must be one of ZK_EELS_*");
  if (j.order < 1 || j.order > 3) return zk_fail(ZK_E_BADARG, "eels_pls: the difference order must be 1, 2 or 3");
  if ((j.mode == ZK_EELS_ALS || j.mode == ZK_EELS_ARPLS) && j.order != 2) return zk_fail(ZK_E_BADARG, "eels_pls: ALS and arPLS use second differences");
  if (length < j.order + 1) return zk_fail(ZK_E_BADARG, "eels_pls: a spectrum needs at least order + 1 channels");
  if (!(j.lam > 0.0) || !std::isfinite(j.lam)) return zk_fail(ZK_E_BADARG, "eels_pls: lam must be positive and finite");
  if (j.itermax < 1) return zk_fail(ZK_E_BADARG, "eels_pls: needs at least one iteration");
  if (j.mode == ZK_EELS_ALS && !(j.param > 0.0 && j.param < 1.0)) return zk_fail(ZK_E_BADARG, "eels_pls: p must lie in (0, 1)");
  if (j.mode == ZK_EELS_ARPLS && !(j.param > 0.0)) return zk_fail(ZK_E_BADARG, "eels_pls: ratio must be positive");
  if ((j.mode == ZK_EELS_WHITTAKER) != has_weights) return zk_fail(ZK_E_BADARG, "eels_pls: weights go with ZK_EELS_WHITTAKER, and only with it");
  return 0;
}

// spectra per chunk: the largest multiple of 64 whose scratch planes stay under the device's cap
int64_t chunk_columns(int device, int64_t L, int planes, int64_t N) {
  const size_t cap = g_cap.get(device, DEFAULT_CAP);
  int64_t nc = (int64_t)(cap / ((size_t)L * 8 * (size_t)planes)) / 64 * 64;
  nc = std::max<int64_t>(nc, 64);
  return std::min<int64_t>(nc, (N + 63) / 64 * 64);
}

template <typename T>
int run_typed(int device, const eels_job& j, const void* data_v, int64_t A, int64_t L64, int64_t B, double* baseline, double* signal,
              int32_t* iters, hipStream_t s) {
  const T* data = (const T*)data_v;
  const int64_t N = A * B;
  const int L = (int)L64;
  const bool native = A == 1;
  int rc;
  // ---- the (L, N) views of input and output
  dev_buf d_in, d_out, d_w;
  const double* y64 = nullptr;  // the spectra as float64 (L, N), where they exist in that form
  if (!native) {
    if ((rc = d_in.alloc((size_t)L * N * 8)) || (rc = d_out.alloc((size_t)L * N * 8)) || (rc = swap_axes<T>(data, d_in.as<double>(), A, L, B, s)))
      return rc;
    y64 = d_in.as<double>();
  } else if (std::is_same<T, double>::value) {
    y64 = (const double*)data_v;
  }
  double* z = native ? baseline : d_out.as<double>();

  if (j.snip) {
    const int64_t nc_max = chunk_columns(device, L, 2, N);
    dev_buf d_v;
    if ((rc = d_v.alloc((size_t)2 * L * nc_max * 8))) return rc;
    double* v[2] = {d_v.as<double>(), d_v.as<double>() + (size_t)L * nc_max};
    for (int64_t n0 = 0; n0 < N; n0 += nc_max) {
      const int nc = (int)std::min<int64_t>(nc_max, N - n0);
      const plane_grid pg(L, nc);
      if (y64) hipLaunchKernelGGL((load_plane_kernel<double, true>), pg.grid, dim3(256), 0, s, y64 + n0, (long long)N, v[0], (long long)nc_max, L, nc);
      else hipLaunchKernelGGL((load_plane_kernel<T, true>), pg.grid, dim3(256), 0, s, data + n0, (long long)N, v[0], (long long)nc_max, L, nc);
      ZK_HIP(hipGetLastError());
      int cur = 0;
      for (int pp = 1; pp <= j.itermax && 2 * (int64_t)pp < L; ++pp, cur ^= 1) {
        hipLaunchKernelGGL(snip_pass_kernel, pg.grid, dim3(256), 0, s, v[cur], v[cur ^ 1], (long long)nc_max, L, nc, pp);
        ZK_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(snip_inverse_kernel, pg.grid, dim3(256), 0, s, v[cur], (long long)nc_max, z + n0, (long long)N, L, nc);
      ZK_HIP(hipGetLastError());
    }
  } else {
    const int K = j.order;
    const bool widen = !y64;
    const int planes = K + 1 + (j.mode == ZK_EELS_ARPLS ? 1 : 0) + (widen ? 1 : 0);
    const int64_t nc_max = chunk_columns(device, L, planes, N);
    const size_t plane = (size_t)L * nc_max;
    dev_buf d_scratch, d_band;
    const std::vector<double> band = penalty_band(L, K, j.lam);  // lives until the synchronisation below
    if ((rc = d_scratch.alloc(plane * planes * 8)) || (rc = d_band.alloc(band.size() * 8))) return rc;
    ZK_HIP(hipMemcpyAsync(d_band.p, band.data(), band.size() * 8, hipMemcpyHostToDevice, s));
    const double* w = j.weights;
    if (w && j.weights_per_spectrum && !native) {
      if ((rc = d_w.alloc((size_t)L * N * 8)) || (rc = swap_axes<double>(w, d_w.as<double>(), A, L, B, s))) return rc;
      w = d_w.as<double>();
    }
    double* fac = d_scratch.as<double>();
    double* wt = j.mode == ZK_EELS_ARPLS ? fac + plane * (K + 1) : nullptr;
    double* ybuf = widen ? fac + plane * (planes - 1) : nullptr;
    for (int64_t n0 = 0; n0 < N; n0 += nc_max) {
      const int nc = (int)std::min<int64_t>(nc_max, N - n0);
      pls_args a;
      if (widen) {
        hipLaunchKernelGGL((load_plane_kernel<T, false>), plane_grid(L, nc).grid, dim3(256), 0, s, data + n0, (long long)N, ybuf, (long long)nc_max, L, nc);
        ZK_HIP(hipGetLastError());
        a.y = ybuf;
        a.ys = nc_max;
      } else {
        a.y = y64 + n0;
        a.ys = N;
      }
      a.w = w ? (j.weights_per_spectrum ? w + n0 : w) : nullptr;
      a.ws = j.weights_per_spectrum ? N : 1;
      a.wl = j.weights_per_spectrum ? 1 : 0;
      a.band = d_band.as<double>();
      a.fac = fac;
      a.fs = nc_max;
      a.wt = wt;
      a.z = z + n0;
      a.zs = N;
      a.iters = iters ? iters + n0 : nullptr;
      a.L = L;
      a.n = nc;
      a.p = j.param;
      a.itermax = j.itermax;
      if ((rc = launch_pls(K, j.mode, a, s))) return rc;
    }
  }
  if (!native && (rc = swap_axes<double>(z, baseline, L, A, B, s))) return rc;
  if (signal) {
    const long long total = (long long)A * L * B;
    hipLaunchKernelGGL(signal_kernel<T>, dim3(std::min<unsigned>(blocks_of(total, 256), 65536)), dim3(256), 0, s, data, baseline, signal, total);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(s));  // the scratch is freed on return
  return 0;
}

int run_dev(int device, const eels_job& j, const void* data, int dtype, int64_t A, int64_t L, int64_t B, double* baseline, double* signal,
            int32_t* iters, hipStream_t s) {
  return zk_with_elem(dtype, [&](auto e) { return run_typed<typename decltype(e)::type>(device, j, data, A, L, B, baseline, signal, iters, s); });
}

// the host-buffer form: the cube goes up, baseline (signal, iteration counts) come down
int run_host(int device, eels_job j, const void* data, int dtype, int64_t A, int64_t L, int64_t B, const double* weights_host, double* baseline,
             double* signal, int32_t* iters) {
  const size_t total = (size_t)A * L * B, in_bytes = total * zk_elem_size(dtype), out_bytes = total * 8, it_bytes = (size_t)A * B * 4,
               w_bytes = (j.weights_per_spectrum ? total : (size_t)L) * 8;
  dev_buf d_data, d_base, d_sig, d_it, d_w;          // d_sig, d_it and d_w stay null for what the caller left out
  int rc;
  if ((rc = d_data.upload(data, in_bytes)) || (rc = d_base.alloc(out_bytes)) || (signal && (rc = d_sig.alloc(out_bytes))) ||
      (iters && (rc = d_it.alloc(it_bytes))) || (rc = d_w.upload(weights_host, w_bytes)))
    return rc;
  j.weights = d_w.as<double>();
  if ((rc = run_dev(device, j, d_data.p, dtype, A, L, B, d_base.as<double>(), d_sig.as<double>(), d_it.as<int32_t>(), (hipStream_t)0)) ||
      (rc = d_base.download(baseline, out_bytes)) || (rc = d_sig.download(signal, out_bytes)))
    return rc;
  return d_it.download(iters, it_bytes);
}

eels_job snip_job(int niter) {
  eels_job j;
  j.snip = true;
  j.itermax = niter;
  return j;
}

eels_job pls_job(int mode, int order, double lam, double param, int itermax, const double* weights, int weights_per_spectrum) {
  eels_job j;
  j.mode = mode;
  j.order = order;
  j.lam = lam;
  j.param = param;
  j.itermax = mode == ZK_EELS_WHITTAKER ? 1 : itermax;
  j.weights = weights;
  j.weights_per_spectrum = weights_per_spectrum != 0;
  return j;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_eels_set_chunk(int device, int64_t scratch_bytes) {
  return g_cap.set(device, scratch_bytes, "bad arguments");
}

extern "C" int zk_eels_snip(int device, const void* data_host, int dtype, int64_t outer, int64_t length, int64_t inner, int niter,
                            double* baseline_host, double* signal_host) {
  const eels_job j = snip_job(niter);
  int rc = check_shape("eels_snip", data_host, dtype, outer, length, inner, baseline_host);
  if (rc || (rc = check_job(j, length, false)) || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  return run_host(device, j, data_host, dtype, outer, length, inner, nullptr, baseline_host, signal_host, nullptr);
}

extern "C" int zk_eels_snip_dev(int device, const void* data_dev, int dtype, int64_t outer, int64_t length, int64_t inner, int niter,
                                double* baseline_dev, double* signal_dev, void* hip_stream) {
  const eels_job j = snip_job(niter);
  int rc = check_shape("eels_snip", data_dev, dtype, outer, length, inner, baseline_dev);
  if (rc || (rc = check_job(j, length, false)) || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  return run_dev(device, j, data_dev, dtype, outer, length, inner, baseline_dev, signal_dev, nullptr, (hipStream_t)hip_stream);
}

extern "C" int zk_eels_pls(int device, const void* data_host, int dtype, int64_t outer, int64_t length, int64_t inner, int mode, int order,
                           double lam, double param, int itermax, const double* weights_host, int weights_per_spectrum,
                           double* baseline_host, double* signal_host, int32_t* iterations_host) {
  const eels_job j = pls_job(mode, order, lam, param, itermax, nullptr, weights_per_spectrum);
  int rc = check_shape("eels_pls", data_host, dtype, outer, length, inner, baseline_host);
  if (rc || (rc = check_job(j, length, weights_host != nullptr)) || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  return run_host(device, j, data_host, dtype, outer, length, inner, weights_host, baseline_host, signal_host, iterations_host);
}

extern "C" int zk_eels_pls_dev(int device, const void* data_dev, int dtype, int64_t outer, int64_t length, int64_t inner, int mode, int order,
                               double lam, double param, int itermax, const double* weights_dev, int weights_per_spectrum,
                               double* baseline_dev, double* signal_dev, int32_t* iterations_dev, void* hip_stream) {
  const eels_job j = pls_job(mode, order, lam, param, itermax, weights_dev, weights_per_spectrum);
  int rc = check_shape("eels_pls", data_dev, dtype, outer, length, inner, baseline_dev);
  if (rc || (rc = check_job(j, length, weights_dev != nullptr)) || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  return run_dev(device, j, data_dev, dtype, outer, length, inner, baseline_dev, signal_dev, iterations_dev, (hipStream_t)hip_stream);
}
