// zk_denoise.hip -- device side of mtflearn.denoise (reference denoise/_denoise_svd.py, _denoise_svd_memory_view.py): patch-SVD
// and patch-PCA denoising as operators of the implicit window matrix of a resident frame.
//
// A is the (N, D) matrix whose row w = a * nj + b is the ph x pw window of the frame at origin (ii[a], jj[b]), D = ph * pw,
// N = ni * nj; ii and jj are ascending origin lists from the caller (the reference's grid has an irregular last step).  A is
// never formed: every kernel walks the windows in the frame.  Pixels are widened to float64 as they are read; all arithmetic
// is float64.
//
//   apply        Y (N, l) = (A - 1 mu^T) Q.  One window per lane, ZK_DN_LC columns of Q per pass (grid.y); Q and mu are
//                wave-uniform (scalar loads), the lanes of a wave read windows one grid step apart.
//   apply_t      Z (D, l) = A^T Y.  One pixel of the window per lane, the windows cut into chunks (grid.x); every chunk sums
//                its windows in order into a partial (chunks, D, l), a second kernel adds the partials in chunk order.
//   moments      dense grid: mu (D) and C (D, D) = (A - 1 mu^T)^T (A - 1 mu^T) / (N - 1), by the structure of the dense
//                window matrix: with J = frame - g (g the frame's mean: any constant is exact, this one keeps the products
//                small), entry [(a, b), (c, d)] of A^T A is the sum of J[y, x] J[y + c - a, x + d - b] over the
//                (H - ph + 1) x (W - pw + 1) rectangle at (a, b).  One workgroup per offset (c - a, d - b) makes the products
//                of one frame row per wave, sums the columns every rectangle shares once and adds each rectangle's own border
//                columns to it; rows are collapsed the same way.  Sums only, no sliding subtraction: about 2 ph pw H W
//                products in all against 2 N D^2 of the plain product.
//   reconstruct  out (H, W) = overlap-add of the windows Y[w, :] V + mu (or of an explicit (N, ph, pw) batch) over the number
//                of windows on each pixel.  A gather: every output pixel adds the windows over it, rows then columns of the
//                grid ascending (the order of the reference's loop); a pixel under no window is 0 / 0 = NaN.
//
// No atomics anywhere and every reduction in a fixed order: two runs give the same bits.
#include <math.h>

#include <algorithm>
#include <vector>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int ZK_DN_LC = 16;        // columns of Q / Y per pass of apply and apply_t
constexpr int ZK_DN_CHUNKS = 512;   // most window chunks of apply_t
constexpr int ZK_DN_MAX_P = 48;     // largest patch edge of the moments kernel (its border tables stay within 64 KiB of LDS)

// the window grid of one call: origins checked on the host, then resident
struct grid_desc {
  int H, W, ph, pw, ni, nj;
  const int* ii;  // device
  const int* jj;
};

// ---------------------------------------------------------------------------------------------------------------------
// apply: Y = (A - 1 mu^T) Q
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void windows_apply_kernel(const T* __restrict__ img, grid_desc g, const double* __restrict__ Q, int l,
                                                            const double* __restrict__ mu, double* __restrict__ Y) {
  const long long n = (long long)g.ni * g.nj;
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int l0 = blockIdx.y * ZK_DN_LC;
  const int lc = min(ZK_DN_LC, l - l0);
  const int a = (int)(w / g.nj), b = (int)(w - (long long)a * g.nj);
  const T* src = img + (long long)g.ii[a] * g.W + g.jj[b];
  double acc[ZK_DN_LC];
#pragma unroll
  for (int j = 0; j < ZK_DN_LC; ++j) acc[j] = 0.0;
  for (int dy = 0; dy < g.ph; ++dy) {
    const T* row = src + (long long)dy * g.W;
    for (int dx = 0; dx < g.pw; ++dx) {
      const int d = dy * g.pw + dx;
      double v = (double)row[dx];
      if (mu) v -= mu[d];
      const double* q = Q + (long long)d * l + l0;
      if (lc == ZK_DN_LC) {
#pragma unroll
        for (int j = 0; j < ZK_DN_LC; ++j) acc[j] = fma(v, q[j], acc[j]);
      } else {
#pragma unroll
        for (int j = 0; j < ZK_DN_LC; ++j)
          if (j < lc) acc[j] = fma(v, q[j], acc[j]);
      }
    }
  }
  double* y = Y + w * l + l0;
#pragma unroll
  for (int j = 0; j < ZK_DN_LC; ++j)
    if (j < lc) y[j] = acc[j];
}

// ---------------------------------------------------------------------------------------------------------------------
// apply_t: Z = A^T Y
// ---------------------------------------------------------------------------------------------------------------------
// part[chunk][d][l]: the windows [chunk * per_chunk, ...) in order
template <typename T>
__global__ __launch_bounds__(256) void windows_apply_t_kernel(const T* __restrict__ img, grid_desc g, const double* __restrict__ Y, int l,
                                                              long long per_chunk, double* __restrict__ part) {
  const int D = g.ph * g.pw;
  const int d = blockIdx.y * 256 + threadIdx.x;
  const int l0 = blockIdx.z * ZK_DN_LC;
  const int lc = min(ZK_DN_LC, l - l0);
  const long long n = (long long)g.ni * g.nj;
  const long long w0 = (long long)blockIdx.x * per_chunk;
  const long long w1 = min(n, w0 + per_chunk);
  const bool live = d < D;
  const int dd = live ? d : 0;
  const int dy = dd / g.pw, dx = dd - dy * g.pw;
  const T* src = img + (long long)dy * g.W + dx;
  double acc[ZK_DN_LC];
#pragma unroll
  for (int j = 0; j < ZK_DN_LC; ++j) acc[j] = 0.0;
  int a = (int)(w0 / g.nj), b = (int)(w0 - (long long)a * g.nj);
  for (long long w = w0; w < w1; ++w) {
    const double v = (double)src[(long long)g.ii[a] * g.W + g.jj[b]];
    const double* y = Y + w * l + l0;
    if (lc == ZK_DN_LC) {
#pragma unroll
      for (int j = 0; j < ZK_DN_LC; ++j) acc[j] = fma(v, y[j], acc[j]);
    } else {
#pragma unroll
      for (int j = 0; j < ZK_DN_LC; ++j)
        if (j < lc) acc[j] = fma(v, y[j], acc[j]);
    }
    if (++b == g.nj) {
      b = 0;
      ++a;
    }
  }
  if (!live) return;
  double* out = part + ((long long)blockIdx.x * D + d) * l + l0;
#pragma unroll
  for (int j = 0; j < ZK_DN_LC; ++j)
    if (j < lc) out[j] = acc[j];
}

__global__ __launch_bounds__(256) void chunk_sum_kernel(const double* __restrict__ part, int chunks, long long n, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = part[e];
  for (int c = 1; c < chunks; ++c) s += part[(long long)c * n + e];
  out[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// moments of the dense grid
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// 256 partial sums of the frame, strided: part[b] in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void frame_sum_kernel(const T* __restrict__ img, long long n, double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += (double)img[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// g[0] = sum(part) / n
__global__ __launch_bounds__(64) void frame_mean_kernel(const double* __restrict__ part, int parts, long long n, double* __restrict__ g) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < parts; ++i) s += part[i];
    g[0] = s / (double)n;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void centre_kernel(const T* __restrict__ img, const double* __restrict__ g, double* __restrict__ J, long long n) {
  const double m = g[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) J[i] = (double)img[i] - m;
}

// Lines of an axis of extent n under dense windows of edge p (nw = n - p + 1 origins): the lines p - 1 <= t < nw lie in every
// window span [o, o + nw) and are summed once ("core"); every other line is kept on its own, at lone_index().
__device__ __forceinline__ bool is_core(int t, int p, int nw) { return t >= p - 1 && t < nw; }
__device__ __forceinline__ int lone_index(int t, int p, int nw) { return t < p - 1 ? t : (p - 1) + (t - max(nw, p - 1)); }
__device__ __forceinline__ int lone_line(int i, int p, int nw) { return i < p - 1 ? i : max(nw, p - 1) + (i - (p - 1)); }
__host__ __device__ __forceinline__ int lone_count(int n, int p) { return (p - 1) + (n - (n - p + 1 > p - 1 ? n - p + 1 : p - 1)); }

// blockIdx = (v + pw - 1, u): S[u][v][a][b] = sum over y in [a, a + nh), x in [b, b + nw) of J[y][x] J[y + u][x + v] for
// 0 <= a < ph - u and the b with 0 <= b + v < pw; blockIdx.y == ph: the plain box sums of J over N (the window means of J).
// LDS: lone[n_lone_rows][pw], core[4][pw], cols[4][n_lone_cols].
__global__ __launch_bounds__(256) void moments_offset_kernel(const double* __restrict__ J, int H, int W, int ph, int pw,
                                                             double* __restrict__ S, double* __restrict__ mean) {
  extern __shared__ __align__(16) unsigned char dn_lds[];
  const int nh = H - ph + 1, nw = W - pw + 1;
  const int n_lr = lone_count(H, ph), n_lc = lone_count(W, pw);
  double* lone = (double*)dn_lds;
  double* core = lone + (size_t)n_lr * pw;
  double* cols = core + 4 * pw;
  const bool plain = (int)blockIdx.y == ph;
  const int u = plain ? 0 : (int)blockIdx.y;
  const int v = plain ? 0 : (int)blockIdx.x - (pw - 1);
  if (plain ? blockIdx.x != 0 : (u == 0 && v < 0)) return;  // the lower half comes from the upper by symmetry
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < n_lr * pw; i += 256) lone[i] = 0.0;
  __syncthreads();
  double* my_cols = cols + (size_t)wave * n_lc;
  double k_core = 0.0;  // lane b < pw: the core rows of this wave
  for (int y = wave; y < H - u; y += 4) {
    const double* r0 = J + (long long)y * W;
    const double* r1 = J + (long long)(y + u) * W + v;
    double c = 0.0;
    for (int x = lane; x < W; x += 64) {
      double p = r0[x];
      if (!plain) p = (x + v >= 0 && x + v < W) ? p * r1[x] : 0.0;
      if (is_core(x, pw, nw)) c += p;
      else my_cols[lone_index(x, pw, nw)] = p;
    }
    c = wave_sum(c);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < pw) {
      double gsum = c;
      for (int i = 0; i < n_lc; ++i) {
        const int x = lone_line(i, pw, nw);
        if (x >= lane && x < lane + nw) gsum += my_cols[i];
      }
      if (is_core(y, ph, nh)) k_core += gsum;
      else lone[(size_t)lone_index(y, ph, nh) * pw + lane] = gsum;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane < pw) core[wave * pw + lane] = k_core;
  __syncthreads();
  const double n_windows = (double)nh * (double)nw;
  for (int t = threadIdx.x; t < (ph - u) * pw; t += 256) {
    const int a = t / pw, b = t - a * pw;
    if (b + v < 0 || b + v >= pw) continue;
    double s = ((core[b] + core[pw + b]) + core[2 * pw + b]) + core[3 * pw + b];
    for (int i = 0; i < n_lr; ++i) {
      const int y = lone_line(i, ph, nh);
      if (y >= a && y < a + nh) s += lone[(size_t)i * pw + b];
    }
    if (plain) mean[a * pw + b] = s / n_windows;
    else S[(((size_t)u * (2 * pw - 1) + (v + pw - 1)) * ph + a) * pw + b] = s;
  }
}

// C[i][j] = (S - N m_i m_j) / max(N - 1, 1) with m the window means of J; mu = m + g
__global__ __launch_bounds__(256) void moments_finish_kernel(const double* __restrict__ S, const double* __restrict__ mean,
                                                             const double* __restrict__ g, int ph, int pw, double n_windows,
                                                             double* __restrict__ mu, double* __restrict__ C) {
#pragma clang fp contract(off)  // s - N m_i m_j with the product rounded: exactly 0 for a single window, as the plain form gives
  const int D = ph * pw;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)D * D) return;
  int i = (int)(e / D), j = (int)(e - (long long)i * D);
  if (j == 0) mu[i] = mean[i] + g[0];
  if (j < i) {
    const int t = i;
    i = j;
    j = t;
  }
  const int a = i / pw, b = i - a * pw, c = j / pw, d = j - c * pw;  // c > a, or c == a and d >= b
  const int u = c - a, v = d - b;
  const double s = S[(((size_t)u * (2 * pw - 1) + (v + pw - 1)) * ph + a) * pw + b];
  const double denom = n_windows > 1.0 ? n_windows - 1.0 : 1.0;
  C[e] = (s - n_windows * mean[i] * mean[j]) / denom;
}

// ---------------------------------------------------------------------------------------------------------------------
// reconstruct
// ---------------------------------------------------------------------------------------------------------------------
// rows[y] / cols[x]: first and last grid index over the line (last < first: none)
__global__ __launch_bounds__(256) void windows_reconstruct_kernel(grid_desc g, const int2* __restrict__ rows, const int2* __restrict__ cols,
                                                                  const double* __restrict__ Y, int k, const double* __restrict__ V,
                                                                  const double* __restrict__ mu, double* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= g.W || y >= g.H) return;
  const int D = g.ph * g.pw;
  const int2 ra = rows[y], rb = cols[x];
  double sum = 0.0;
  for (int a = ra.x; a <= ra.y; ++a) {
    const int dy = y - g.ii[a];
    for (int b = rb.x; b <= rb.y; ++b) {
      const int d = dy * g.pw + (x - g.jj[b]);
      const long long w = (long long)a * g.nj + b;
      double t;
      if (V) {
        const double* yw = Y + w * k;
        t = 0.0;
        for (int j = 0; j < k; ++j) t = fma(yw[j], V[(long long)j * D + d], t);
      } else {
        t = Y[w * D + d];
      }
      if (mu) t += mu[d];
      sum += t;
    }
  }
  const double cover = (double)max(ra.y - ra.x + 1, 0) * (double)max(rb.y - rb.x + 1, 0);
  out[(long long)y * g.W + x] = sum / cover;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int check_frame(int dtype, int64_t H, int64_t W, int64_t ph, int64_t pw) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (H <= 0 || W <= 0 || H * W >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "bad image shape (needs 0 < height * width < 2^31)");
  if (ph < 1 || pw < 1 || ph > H || pw > W) return zk_fail(ZK_E_BADARG, "the patch must be at least 1 x 1 and fit the image");
  if (ph * pw > ((int64_t)1 << 23)) return zk_fail(ZK_E_BADARG, "patch too large");
  if (H > 4 * 65535) return zk_fail(ZK_E_BADARG, "height must be at most 262140 (the overlap-add covers four rows per block)");
  return 0;
}

int check_origins(const int32_t* o, int64_t n, int64_t extent, int64_t patch, const char* what) {
  if (!o || n < 1 || n > extent) return zk_fail(ZK_E_BADARG, std::string(what) + ": need between 1 and (image extent) origins");
  for (int64_t i = 0; i < n; ++i) {
    if (o[i] < 0 || o[i] + patch > extent) return zk_fail(ZK_E_BADARG, std::string(what) + ": a window leaves the image");
    if (i && o[i] <= o[i - 1]) return zk_fail(ZK_E_BADARG, std::string(what) + ": origins must be strictly ascending");
  }
  return 0;
}

// device copies of the origin lists (and, for the gather, of the grid range over every line)
struct grid_tables {
  dev_buf d_ii, d_jj, d_rows, d_cols;
  grid_desc g;
  int upload(int64_t H, int64_t W, int64_t ph, int64_t pw, const int32_t* ii, int64_t ni, const int32_t* jj, int64_t nj, bool ranges,
             hipStream_t s) {
    int rc;
    if ((rc = check_origins(ii, ni, H, ph, "row origins")) || (rc = check_origins(jj, nj, W, pw, "column origins"))) return rc;
    if (ni * nj >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "too many windows (needs fewer than 2^31)");
    if ((rc = d_ii.alloc((size_t)ni * 4)) || (rc = d_jj.alloc((size_t)nj * 4))) return rc;
    ZK_HIP(hipMemcpyAsync(d_ii.p, ii, (size_t)ni * 4, hipMemcpyHostToDevice, s));
    ZK_HIP(hipMemcpyAsync(d_jj.p, jj, (size_t)nj * 4, hipMemcpyHostToDevice, s));
    g = grid_desc{(int)H, (int)W, (int)ph, (int)pw, (int)ni, (int)nj, d_ii.as<int>(), d_jj.as<int>()};
    if (ranges) {
      line_ranges(ii, ni, H, ph, h_rows);
      line_ranges(jj, nj, W, pw, h_cols);
      if ((rc = d_rows.alloc((size_t)H * 8)) || (rc = d_cols.alloc((size_t)W * 8))) return rc;
      ZK_HIP(hipMemcpyAsync(d_rows.p, h_rows.data(), (size_t)H * 8, hipMemcpyHostToDevice, s));
      ZK_HIP(hipMemcpyAsync(d_cols.p, h_cols.data(), (size_t)W * 8, hipMemcpyHostToDevice, s));
    }
    ZK_HIP(hipStreamSynchronize(s));  // the host lists are the caller's (and ours): read before we return
    return 0;
  }

 private:
  std::vector<int2> h_rows, h_cols;
  static void line_ranges(const int32_t* o, int64_t n, int64_t extent, int64_t patch, std::vector<int2>& out) {
    out.resize((size_t)extent);
    int64_t lo = 0, hi = -1;  // origins are ascending: both ends only move forward
    for (int64_t t = 0; t < extent; ++t) {
      while (hi + 1 < n && o[hi + 1] <= t) ++hi;
      while (lo < n && o[lo] + patch <= t) ++lo;
      out[(size_t)t] = make_int2((int)lo, (int)hi);
    }
  }
};

template <typename T>
int apply_typed(const void* img, const grid_desc& g, const double* Q, int l, const double* mu, double* Y, hipStream_t s) {
  const long long n = (long long)g.ni * g.nj;
  hipLaunchKernelGGL(windows_apply_kernel<T>, dim3(blocks_of(n, 256), blocks_of(l, ZK_DN_LC)), dim3(256), 0, s, (const T*)img, g, Q, l, mu, Y);
  ZK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int apply_t_typed(const void* img, const grid_desc& g, const double* Y, int l, double* Z, hipStream_t s) {
  const long long n = (long long)g.ni * g.nj;
  const long long D = (long long)g.ph * g.pw;
  // partials of at most 64 MiB
  const long long chunks_cap = std::max<long long>(1, std::min<long long>(ZK_DN_CHUNKS, ((long long)8 << 20) / (D * l)));
  const long long per_chunk = (n + chunks_cap - 1) / chunks_cap;
  const int chunks = (int)((n + per_chunk - 1) / per_chunk);
  dev_buf part;
  int rc;
  if ((rc = part.alloc((size_t)chunks * D * l * 8))) return rc;
  hipLaunchKernelGGL(windows_apply_t_kernel<T>, dim3(chunks, blocks_of(D, 256), blocks_of(l, ZK_DN_LC)), dim3(256), 0, s, (const T*)img, g,
                     Y, l, per_chunk, part.as<double>());
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(chunk_sum_kernel, dim3(blocks_of(D * l, 256)), dim3(256), 0, s, part.as<double>(), chunks, D * l, Z);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));  // the partials are freed on return
  return 0;
}

template <typename T>
int moments_typed(const void* img, int H, int W, int ph, int pw, double* mu, double* C, hipStream_t s) {
  const long long n = (long long)H * W;
  const int D = ph * pw;
  const int parts = 256;
  const size_t s_count = (size_t)ph * (2 * pw - 1) * D;
  dev_buf d_part, d_g, d_J, d_S, d_mean;
  int rc;
  if ((rc = d_part.alloc(parts * 8)) || (rc = d_g.alloc(8)) || (rc = d_J.alloc((size_t)n * 8)) || (rc = d_S.alloc(s_count * 8)) ||
      (rc = d_mean.alloc((size_t)D * 8)))
    return rc;
  hipLaunchKernelGGL(frame_sum_kernel<T>, dim3(parts), dim3(256), 0, s, (const T*)img, n, d_part.as<double>());
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(frame_mean_kernel, dim3(1), dim3(64), 0, s, d_part.as<double>(), parts, n, d_g.as<double>());
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(centre_kernel<T>, dim3(std::min<unsigned>(blocks_of(n, 256), 2048)), dim3(256), 0, s, (const T*)img, d_g.as<double>(),
                     d_J.as<double>(), n);
  ZK_HIP(hipGetLastError());
  const size_t lds = ((size_t)lone_count(H, ph) * pw + 4 * (size_t)pw + 4 * (size_t)lone_count(W, pw)) * 8;  // <= 40 KiB at 48 x 48
  hipLaunchKernelGGL(moments_offset_kernel, dim3(2 * pw - 1, ph + 1), dim3(256), lds, s, d_J.as<double>(), H, W, ph, pw, d_S.as<double>(),
                     d_mean.as<double>());
  ZK_HIP(hipGetLastError());
  const double n_windows = (double)(H - ph + 1) * (double)(W - pw + 1);
  hipLaunchKernelGGL(moments_finish_kernel, dim3(blocks_of((long long)D * D, 256)), dim3(256), 0, s, d_S.as<double>(), d_mean.as<double>(),
                     d_g.as<double>(), ph, pw, n_windows, mu, C);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));  // the scratch is freed on return
  return 0;
}

int apply_any(int dtype, const void* img, const grid_desc& g, const double* Q, int l, const double* mu, double* Y, hipStream_t s) {
  return zk_with_elem(dtype, [&](auto e) { return apply_typed<typename decltype(e)::type>(img, g, Q, l, mu, Y, s); });
}
int apply_t_any(int dtype, const void* img, const grid_desc& g, const double* Y, int l, double* Z, hipStream_t s) {
  return zk_with_elem(dtype, [&](auto e) { return apply_t_typed<typename decltype(e)::type>(img, g, Y, l, Z, s); });
}
int moments_any(int dtype, const void* img, int H, int W, int ph, int pw, double* mu, double* C, hipStream_t s) {
  return zk_with_elem(dtype, [&](auto e) { return moments_typed<typename decltype(e)::type>(img, H, W, ph, pw, mu, C, s); });
}

int check_columns(int64_t l) {
  if (l < 1 || l > 4096) return zk_fail(ZK_E_BADARG, "the number of columns must be in [1, 4096]");
  return 0;
}

// device-resident forms -------------------------------------------------------------------------------------------------
int apply_dev(int device, const void* img, int dtype, int64_t H, int64_t W, int64_t ph, int64_t pw, const int32_t* ii, int64_t ni,
              const int32_t* jj, int64_t nj, const double* Q, int64_t l, const double* mu, double* Y, hipStream_t s) {
  int rc = check_frame(dtype, H, W, ph, pw);
  if (rc || (rc = check_columns(l))) return rc;
  if (!img || !Q || !Y) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(device);
  grid_tables t;
  if ((rc = t.upload(H, W, ph, pw, ii, ni, jj, nj, false, s)) || (rc = apply_any(dtype, img, t.g, Q, (int)l, mu, Y, s))) return rc;
  ZK_HIP(hipStreamSynchronize(s));  // the origin lists are freed on return
  return 0;
}

int apply_t_dev(int device, const void* img, int dtype, int64_t H, int64_t W, int64_t ph, int64_t pw, const int32_t* ii, int64_t ni,
                const int32_t* jj, int64_t nj, const double* Y, int64_t l, double* Z, hipStream_t s) {
  int rc = check_frame(dtype, H, W, ph, pw);
  if (rc || (rc = check_columns(l))) return rc;
  if (!img || !Y || !Z) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(device);
  grid_tables t;
  if ((rc = t.upload(H, W, ph, pw, ii, ni, jj, nj, false, s))) return rc;
  return apply_t_any(dtype, img, t.g, Y, (int)l, Z, s);
}

int moments_dev(int device, const void* img, int dtype, int64_t H, int64_t W, int64_t ph, int64_t pw, double* mu, double* C, hipStream_t s) {
  int rc = check_frame(dtype, H, W, ph, pw);
  if (rc) return rc;
  if (ph > ZK_DN_MAX_P || pw > ZK_DN_MAX_P) return zk_fail(ZK_E_BADARG, "the moments kernel takes patches of at most 48 x 48");
  if (!img || !mu || !C) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(device);
  return moments_any(dtype, img, (int)H, (int)W, (int)ph, (int)pw, mu, C, s);
}

int reconstruct_dev(int device, int64_t H, int64_t W, int64_t ph, int64_t pw, const int32_t* ii, int64_t ni, const int32_t* jj, int64_t nj,
                    const double* Y, int64_t k, const double* V, const double* mu, double* out, hipStream_t s) {
  int rc = check_frame(ZK_F64, H, W, ph, pw);
  if (rc) return rc;
  if (V && (rc = check_columns(k))) return rc;
  if (!Y || !out) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(device);
  grid_tables t;
  if ((rc = t.upload(H, W, ph, pw, ii, ni, jj, nj, true, s))) return rc;
  hipLaunchKernelGGL(windows_reconstruct_kernel, dim3(blocks_of(W, 64), blocks_of(H, 4)), dim3(256), 0, s, t.g, t.d_rows.as<int2>(),
                     t.d_cols.as<int2>(), Y, (int)k, V, mu, out);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));  // the tables are freed on return
  return 0;
}

}  // namespace

// the host-buffer forms below: operands up (dev_buf::upload; an absent mean or V stays a null pointer), one device call, result down

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_windows_apply_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                    int64_t patch_w, const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins,
                                    int64_t n_cols, const double* Q_dev, int64_t n_columns, const double* mean_dev, double* Y_dev,
                                    void* hip_stream) {
  return apply_dev(device, image_dev, dtype, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Q_dev, n_columns,
                   mean_dev, Y_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_windows_apply(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                int64_t patch_w, const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols,
                                const double* Q_host, int64_t n_columns, const double* mean_host, double* Y_host) {
  int rc = check_frame(dtype, height, width, patch_h, patch_w);
  if (rc || (rc = check_columns(n_columns))) return rc;
  if (!image_host || !Q_host || !Y_host || n_rows < 1 || n_cols < 1) return zk_fail(ZK_E_BADARG, "null pointer or empty grid");
  ZK_ON_DEVICE(device);
  const size_t D = (size_t)patch_h * patch_w, N = (size_t)n_rows * n_cols;
  const size_t img_bytes = (size_t)height * width * zk_elem_size(dtype), q_bytes = D * n_columns * 8, mu_bytes = D * 8, y_bytes = N * n_columns * 8;
  dev_buf img, Q, mu, Y;
  if ((rc = img.upload(image_host, img_bytes)) || (rc = Q.upload(Q_host, q_bytes)) || (rc = mu.upload(mean_host, mu_bytes)) ||
      (rc = Y.alloc(y_bytes)))
    return rc;
  if ((rc = apply_dev(device, img.p, dtype, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Q.as<double>(),
                      n_columns, mu.as<double>(), Y.as<double>(), (hipStream_t)0)))
    return rc;
  return Y.download(Y_host, y_bytes);
}

extern "C" int zk_windows_apply_t_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                      int64_t patch_w, const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins,
                                      int64_t n_cols, const double* Y_dev, int64_t n_columns, double* Z_dev, void* hip_stream) {
  return apply_t_dev(device, image_dev, dtype, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Y_dev, n_columns,
                     Z_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_windows_apply_t(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                  int64_t patch_w, const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols,
                                  const double* Y_host, int64_t n_columns, double* Z_host) {
  int rc = check_frame(dtype, height, width, patch_h, patch_w);
  if (rc || (rc = check_columns(n_columns))) return rc;
  if (!image_host || !Y_host || !Z_host || n_rows < 1 || n_cols < 1) return zk_fail(ZK_E_BADARG, "null pointer or empty grid");
  ZK_ON_DEVICE(device);
  const size_t D = (size_t)patch_h * patch_w, N = (size_t)n_rows * n_cols;
  const size_t img_bytes = (size_t)height * width * zk_elem_size(dtype), y_bytes = N * n_columns * 8, z_bytes = D * n_columns * 8;
  dev_buf img, Y, Z;
  if ((rc = img.upload(image_host, img_bytes)) || (rc = Y.upload(Y_host, y_bytes)) || (rc = Z.alloc(z_bytes))) return rc;
  if ((rc = apply_t_dev(device, img.p, dtype, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Y.as<double>(),
                        n_columns, Z.as<double>(), (hipStream_t)0)))
    return rc;
  return Z.download(Z_host, z_bytes);
}

extern "C" int zk_windows_moments_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                      int64_t patch_w, double* mean_dev, double* cov_dev, void* hip_stream) {
  return moments_dev(device, image_dev, dtype, height, width, patch_h, patch_w, mean_dev, cov_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_windows_moments(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h,
                                  int64_t patch_w, double* mean_host, double* cov_host) {
  int rc = check_frame(dtype, height, width, patch_h, patch_w);
  if (rc) return rc;
  if (!image_host || !mean_host || !cov_host) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(device);
  const size_t D = (size_t)patch_h * patch_w;
  const size_t img_bytes = (size_t)height * width * zk_elem_size(dtype), mu_bytes = D * 8, c_bytes = D * D * 8;
  dev_buf img, mu, C;
  if ((rc = img.upload(image_host, img_bytes)) || (rc = mu.alloc(mu_bytes)) || (rc = C.alloc(c_bytes))) return rc;
  if ((rc = moments_dev(device, img.p, dtype, height, width, patch_h, patch_w, mu.as<double>(), C.as<double>(), (hipStream_t)0))) return rc;
  if ((rc = mu.download(mean_host, mu_bytes))) return rc;
  return C.download(cov_host, c_bytes);
}

extern "C" int zk_windows_reconstruct_dev(int device, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                                          const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols,
                                          const double* Y_dev, int64_t n_components, const double* V_dev, const double* mean_dev,
                                          double* out_dev, void* hip_stream) {
  return reconstruct_dev(device, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Y_dev, n_components, V_dev,
                         mean_dev, out_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_windows_reconstruct(int device, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                                      const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols,
                                      const double* Y_host, int64_t n_components, const double* V_host, const double* mean_host,
                                      double* out_host) {
  int rc = check_frame(ZK_F64, height, width, patch_h, patch_w);
  if (rc) return rc;
  if (V_host && (rc = check_columns(n_components))) return rc;
  if (!Y_host || !out_host || n_rows < 1 || n_cols < 1) return zk_fail(ZK_E_BADARG, "null pointer or empty grid");
  ZK_ON_DEVICE(device);
  const size_t D = (size_t)patch_h * patch_w, N = (size_t)n_rows * n_cols;
  const size_t y_bytes = N * (V_host ? (size_t)n_components : D) * 8, v_bytes = (size_t)n_components * D * 8, mu_bytes = D * 8,
               out_bytes = (size_t)height * width * 8;
  dev_buf Y, V, mu, out;
  if ((rc = Y.upload(Y_host, y_bytes)) || (rc = V.upload(V_host, v_bytes)) || (rc = mu.upload(mean_host, mu_bytes)) ||
      (rc = out.alloc(out_bytes)))
    return rc;
  if ((rc = reconstruct_dev(device, height, width, patch_h, patch_w, row_origins, n_rows, col_origins, n_cols, Y.as<double>(), n_components,
                            V.as<double>(), mu.as<double>(), out.as<double>(), (hipStream_t)0)))
    return rc;
  return out.download(out_host, out_bytes);
}
