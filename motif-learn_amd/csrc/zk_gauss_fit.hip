// zk_gauss_fit.hip -- least-squares fits of a 2-D Gaussian to the size x size window of every key point: the contract of
// include/zernike_hip.h, section "Gaussian fits of key points" (Levenberg-Marquardt with Marquardt's scaling on the precision-matrix
// form f = g + A exp(-(a dx^2 + 2 b dx dy + c dy^2) / 2), or its circular case b = 0, c = a).  A file of its own beside
// zk_com_refine.hip; no reference counterpart, so nothing here restates NumPy operation by operation and the unit is built with the
// library's default flags (products and sums may fuse).
//
// One launch, ONE WAVE PER POINT (a workgroup of 64 lanes), the whole iteration on chip, no global scratch, no floating-point
// atomics.  The window is read from the frame once, widened to float64 and kept in VGPRs: pixel i = row * size + col belongs to
// lane i % 64, slot i / 64, so a lane holds PPL = 1, 2, 4, 8 or 16 pixels (size <= 8, 11, 16, 22, 32).  The mask and the lanes
// past the window are a per-pixel predicate: such a slot adds exact zeros.  Every evaluation of a parameter vector computes exp,
// the residual and the Jacobian row of the lane's pixels and accumulates the upper triangle of J^T J, J^T r and rss in the lane
// (36 sums at 7 parameters, 21 at 5), slot after slot.  The lanes' sums are joined in a fixed order by a REDUCE-SCATTER: the sums
// are padded to a multiple of 8 (40 / 24); the exchanges with lanes ^32, ^16 and ^8 each halve what a lane carries (a lane keeps
// the half its lane bit selects and adds the partner's copy of it), the exchanges with lanes ^4, ^2, ^1 are plain butterflies on
// the remaining eighth: 50 64-bit shuffles at 7 parameters where the plain butterfly takes 216.  Lanes 0, 8, .. 56 then hold the
// eight finished eighths and write them to one of two LDS slots of 40 doubles; every lane reads what it needs from there (one
// address per read: a broadcast).  The accepted point's sums stay in one slot while a trial fills the other, so accepting is a
// flip of the slot index.  The damped normal equations are solved by Cholesky redundantly in every lane from those LDS values:
// the data are the same in all 64 lanes, so the accept / reject decision and every branch of the loop are wave-uniform by
// construction, and a rejected trial (not finite, not positive definite, centre out of the window) skips its evaluation in all
// lanes at once.  The tree depends on size alone: two runs, and the corner and point entry points, agree bit for bit.
//
// A window that leaves the frame raises the error flag and writes nothing.  In point mode the corner is rint(point) - size / 2.
// LDS: 640 bytes a wave.  Registers and what binds the kernel: DESIGN.md, "Gaussian fits of key points".
#include <math.h>

#include "zk_point_window.h"

namespace {

constexpr int MIN_SIZE = 3, MAX_SIZE = 32;           // the side of a window
constexpr int MAX_ITER_LIMIT = 10000;
constexpr double LAMBDA_START = 1e-3, LAMBDA_MIN = 1e-12, LAMBDA_MAX = 1e12;
constexpr int FITTED = 1 << 16;                      // pos: col | row << 8 | FITTED
constexpr int SLOT = 40;                             // doubles of one LDS slot: the padded sums of the elliptical model

template <int NP>
struct layout {
  static constexpr int TRI = NP * (NP + 1) / 2;      // J^T J, upper triangle by rows
  static constexpr int RHS = TRI;                    // J^T r
  static constexpr int RSS = TRI + NP;
  static constexpr int NS = TRI + NP + 1;
  static constexpr int PAD = (NS + 7) / 8 * 8;
  __host__ __device__ static constexpr int tri(int i, int j) { return i * NP - i * (i - 1) / 2 + (j - i); }   // i <= j
};

// One reduce-scatter stage: N values a lane -> N / 2; the lane whose bit `d` is set keeps the upper half.
template <int N>
__device__ inline void scatter_stage(double* a, int d, int lane) {
  const bool upper = (lane & d) != 0;
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const double keep = upper ? a[j + N / 2] : a[j], send = upper ? a[j] : a[j + N / 2];
    a[j] = keep + __shfl_xor(send, d, 64);
  }
}

// The lanes' PAD sums joined in the fixed order; `slot` (PAD doubles of LDS) holds them afterwards, for every lane to read.
template <int PAD>
__device__ inline void wave_sums(double (&a)[PAD], double* slot) {
  const int lane = threadIdx.x;
  scatter_stage<PAD>(a, 32, lane);
  scatter_stage<PAD / 2>(a, 16, lane);
  scatter_stage<PAD / 4>(a, 8, lane);
#pragma unroll
  for (int d = 4; d > 0; d >>= 1)
#pragma unroll
    for (int j = 0; j < PAD / 8; ++j) a[j] += __shfl_xor(a[j], d, 64);
  __syncthreads();                                   // whoever still reads this slot from two evaluations ago
  if ((lane & 7) == 0)
#pragma unroll
    for (int j = 0; j < PAD / 8; ++j) slot[(lane >> 3) * (PAD / 8) + j] = a[j];
  __syncthreads();
}

// J^T J, J^T r and rss of the parameters p over the lane's pixels, joined over the wave into `slot`.
// p = (A, x0, y0, a, b, c, g) at NP = 7, (A, x0, y0, a, g) at NP = 5.
template <int NP, int PPL>
__device__ inline void evaluate(const double (&pix)[PPL], const int (&pos)[PPL], const double (&p)[NP], double* slot) {
  using L = layout<NP>;
  double acc[L::PAD];
#pragma unroll
  for (int j = 0; j < L::PAD; ++j) acc[j] = 0;
  const double A = p[0], a = p[3], b = NP == 7 ? p[4] : 0.0, c = NP == 7 ? p[5] : p[3], g = p[NP - 1];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const bool on = (pos[k] & FITTED) != 0;
    const double dx = (double)(pos[k] & 255) - p[1], dy = (double)((pos[k] >> 8) & 255) - p[2];
    const double q = a * dx * dx + 2.0 * b * dx * dy + c * dy * dy;
    const double e = on ? exp(-0.5 * q) : 0.0, ae = A * e;
    const double r = on ? pix[k] - (g + ae) : 0.0;
    double jac[NP];
    jac[0] = e;
    jac[1] = ae * (a * dx + b * dy);
    jac[2] = ae * (b * dx + c * dy);
    if (NP == 7) {
      jac[3] = -0.5 * ae * dx * dx;
      jac[4] = -ae * dx * dy;
      jac[5] = -0.5 * ae * dy * dy;
    } else {
      jac[3] = -0.5 * ae * (dx * dx + dy * dy);
    }
    jac[NP - 1] = on ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
      for (int j = i; j < NP; ++j) acc[L::tri(i, j)] += jac[i] * jac[j];
      acc[L::RHS + i] += jac[i] * r;
    }
    acc[L::RSS] += r * r;
  }
  wave_sums<L::PAD>(acc, slot);
}

// (J^T J + lambda diag(J^T J)) delta = J^T r by Cholesky, from the sums in `slot`.  False when a pivot is not positive.
template <int NP>
__device__ inline bool solve(const double* slot, double lambda, double (&delta)[NP]) {
  using L = layout<NP>;
  double f[NP][NP];                                  // the lower factor; f[i][i] holds 1 / pivot
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    double d = slot[L::tri(j, j)];
    d = d + lambda * d;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= f[j][k] * f[j][k];
    ok = ok && d > 0;                                // false for a NaN
    const double root = sqrt(d), inv = 1.0 / root;
    f[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < NP; ++i) {
      double s = slot[L::tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= f[i][k] * f[j][k];
      f[i][j] = s * inv;
    }
  }
  if (!ok) return false;
  double y[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double s = slot[L::RHS + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= f[i][k] * y[k];
    y[i] = s * f[i][i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < NP; ++k) s -= f[k][i] * delta[k];
    delta[i] = s * f[i][i];
  }
  return true;
}

// A trial is looked at only when it is finite, positive definite and its centre lies in [-0.5, size - 0.5] on both axes.
template <int NP>
__device__ inline bool admissible(const double (&p)[NP], int size) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < NP; ++k) ok = ok && isfinite(p[k]);
  const double a = p[3], b = NP == 7 ? p[4] : 0.0, c = NP == 7 ? p[5] : p[3], top = (double)size - 0.5;
  return ok && a > 0 && c > 0 && a * c - b * b > 0 && p[1] >= -0.5 && p[1] <= top && p[2] >= -0.5 && p[2] <= top;
}

template <typename T, int NP, int PPL>
__global__ __launch_bounds__(64) void gauss_fit_kernel(const T* __restrict__ img, long long H, long long W, const void* __restrict__ pts,
                                                       int pts_dtype, int size, int disk, double sigma0, double tol, int max_iter,
                                                       double* __restrict__ params, int* __restrict__ iterations,
                                                       int* __restrict__ status, int* __restrict__ flag) {
  using L = layout<NP>;
  __shared__ double sums[2][SLOT];
  const int lane = threadIdx.x, area = size * size;
  const long long n = blockIdx.x;
  // the corner of the window: uniform over the wave, so every exit below is taken by all lanes
  const point_window at = window_at(pts, pts_dtype, n, size, H, W);
  if (!at.inside) {
    if (lane == 0) atomicOr(flag, ERR_WINDOW);
    return;
  }
  const long long x0 = at.x0, y0 = at.y0;
  double pix[PPL], lo = INFINITY, hi = -INFINITY;
  int pos[PPL];
  bool bad = false;
  const int radius = size / 2;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int i = lane + 64 * k, row = i / size, col = i - row * size;
    bool on = i < area;
    if (disk) on = on && (row - radius) * (row - radius) + (col - radius) * (col - radius) <= radius * radius;
    pos[k] = on ? (col | row << 8 | FITTED) : 0;
    pix[k] = on ? (double)img[(y0 + row) * W + x0 + col] : 0.0;
    if (on) {
      bad = bad || !isfinite(pix[k]);
      lo = fmin(lo, pix[k]);
      hi = fmax(hi, pix[k]);
    }
  }
  double* out = params + 8 * n;
  if (__any(bad)) {                                  // status 3: a fitted pixel is NaN or inf
    if (lane < 8) out[lane] = NAN;
    if (lane == 0) {
      iterations[n] = 0;
      status[n] = ZK_GAUSS_NOT_FINITE;
    }
    return;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, d, 64));
    hi = fmax(hi, __shfl_xor(hi, d, 64));
  }
  double p[NP], trial[NP], delta[NP];
  trial[0] = hi - lo;
  trial[1] = trial[2] = (double)(size / 2);
  trial[3] = 1.0 / (sigma0 * sigma0);
  if (NP == 7) {
    trial[4] = 0.0;
    trial[5] = trial[3];
  }
  trial[NP - 1] = lo;
#pragma unroll
  for (int k = 0; k < NP; ++k) p[k] = trial[k], delta[k] = 0;
  double lambda = LAMBDA_START, rss = 0;
  int cur = 1, it = 0, state = ZK_GAUSS_MAX_ITER;
  bool have = false, ok = true;
  if (lo == hi) {                                    // no variation: the start is the answer (rss 0), status 2
    state = ZK_GAUSS_STALLED;
  } else {
    for (;;) {
      if (ok) {
        evaluate<NP, PPL>(pix, pos, trial, sums[cur ^ 1]);
        ok = !have || sums[cur ^ 1][L::RSS] <= rss;    // false for a NaN
      }
      if (ok) {
        cur ^= 1;
        rss = sums[cur][L::RSS];
        bool small = have;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          p[k] = trial[k];
          small = small && fabs(delta[k]) <= tol * (fabs(p[k]) + 1.0);
        }
        if (have) lambda = fmax(lambda / 10.0, LAMBDA_MIN);
        have = true;
        if (small) {
          state = ZK_GAUSS_CONVERGED;
          break;
        }
      } else {
        lambda *= 10.0;
        if (lambda > LAMBDA_MAX) {
          state = ZK_GAUSS_STALLED;
          break;
        }
      }
      if (it == max_iter) break;                     // state is ZK_GAUSS_MAX_ITER
      ++it;
      ok = solve<NP>(sums[cur], lambda, delta);
#pragma unroll
      for (int k = 0; k < NP; ++k) trial[k] = p[k] + delta[k];
      ok = ok && admissible<NP>(trial, size);
    }
  }
  if (lane == 0) {
    const double a = p[3], b = NP == 7 ? p[4] : 0.0, c = NP == 7 ? p[5] : p[3];
    const double mean = 0.5 * (a + c), half = 0.5 * (a - c), l2 = mean + sqrt(half * half + b * b), l1 = (a * c - b * b) / l2;
    out[0] = (double)x0 + p[1];
    out[1] = (double)y0 + p[2];
    out[2] = p[0];
    out[3] = 1.0 / sqrt(NP == 7 ? l1 : a);               // the circular model: both widths are 1 / sqrt(a), the same bits
    out[4] = 1.0 / sqrt(NP == 7 ? l2 : a);
    out[5] = NP == 7 ? 0.5 * atan2(0.0 - 2.0 * b, c - a) : 0.0;
    out[6] = p[NP - 1];
    out[7] = rss;
    iterations[n] = it;
    status[n] = state;
  }
}

int fitted_pixels(int size, int mask) {
  if (mask == ZK_GAUSS_BOX) return size * size;
  const int r = size / 2;
  int count = 0;
  for (int row = 0; row < size; ++row)
    for (int col = 0; col < size; ++col) count += (row - r) * (row - r) + (col - r) * (col - r) <= r * r;
  return count;
}

int check_fit(const char* who, const void* img, int dtype, int64_t H, int64_t W, const void* pts, int64_t n, int64_t size, int model,
              int mask, double sigma0, double tol, int64_t max_iter, const void* params, const void* iterations, const void* status) {
  int rc;
  if ((rc = check_frame(who, img, dtype, H, W, n))) return rc;
  const std::string name(who);
  if (size < MIN_SIZE || size > MAX_SIZE) return zk_fail(ZK_E_BADARG, name + ": needs 3 <= size <= 32");
  if (model != ZK_GAUSS_CIRCULAR && model != ZK_GAUSS_ELLIPTICAL) return zk_fail(ZK_E_BADARG, name + ": unknown model");
  if (mask != ZK_GAUSS_BOX && mask != ZK_GAUSS_DISK) return zk_fail(ZK_E_BADARG, name + ": unknown mask");
  if (mask == ZK_GAUSS_DISK && size % 2 == 0) return zk_fail(ZK_E_BADARG, name + ": the disk mask needs an odd size");
  if (fitted_pixels((int)size, mask) <= (model == ZK_GAUSS_ELLIPTICAL ? 7 : 5))
    return zk_fail(ZK_E_BADARG, name + ": the window has no more fitted pixels than the model has parameters");
  if (!(sigma0 > 0) || !isfinite(sigma0)) return zk_fail(ZK_E_BADARG, name + ": sigma0 must be positive and finite");
  if (!(tol >= 0) || !isfinite(tol)) return zk_fail(ZK_E_BADARG, name + ": tol must be finite and not negative");
  if (max_iter < 1 || max_iter > MAX_ITER_LIMIT) return zk_fail(ZK_E_BADARG, name + ": needs 1 <= max_iter <= 10000");
  return check_pointers(who, n, pts && params && iterations && status);
}

struct fit_args {
  const void* img;
  int64_t H, W;
  const void* pts;
  int pts_dtype;
  int64_t n;
  int size, mask;
  double sigma0, tol;
  int max_iter;
  double* params;
  int *iterations, *status, *flag;
  hipStream_t s;
};

template <typename T, int NP, int PPL>
int fit_launch(const fit_args& a) {
  hipLaunchKernelGGL((gauss_fit_kernel<T, NP, PPL>), dim3((unsigned)a.n), dim3(64), 0, a.s, (const T*)a.img, (long long)a.H, (long long)a.W,
                     a.pts, a.pts_dtype, a.size, a.mask == ZK_GAUSS_DISK, a.sigma0, a.tol, a.max_iter, a.params, a.iterations, a.status,
                     a.flag);
  ZK_HIP(hipGetLastError());
  return 0;
}

template <typename T, int NP>
int fit_by_size(const fit_args& a) {
  const int area = a.size * a.size;                  // pixels a lane: the window spread over 64 lanes
  if (area <= 64) return fit_launch<T, NP, 1>(a);
  if (area <= 128) return fit_launch<T, NP, 2>(a);
  if (area <= 256) return fit_launch<T, NP, 4>(a);
  if (area <= 512) return fit_launch<T, NP, 8>(a);
  return fit_launch<T, NP, 16>(a);
}

int fit_call(const char* who, int dtype, int model, fit_args a) {
  if (a.n == 0) return 0;
  int rc, flags;
  dev_flag flag;
  if ((rc = flag.arm(a.s))) return rc;
  a.flag = flag.word();
  if (model == ZK_GAUSS_ELLIPTICAL)
    rc = dtype == ZK_F32 ? fit_by_size<float, 7>(a) : fit_by_size<double, 7>(a);
  else
    rc = dtype == ZK_F32 ? fit_by_size<float, 5>(a) : fit_by_size<double, 5>(a);
  if (rc || (rc = flag.read(a.s, &flags))) return rc;
  return flags & ERR_WINDOW ? window_fail(who) : 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_gauss_fit_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const void* points_dev,
                                       int points_dtype, int64_t n, int64_t size, int model, int mask, double sigma0, double tol,
                                       int64_t max_iter, double* params_dev, int32_t* iterations_dev, int32_t* status_dev,
                                       void* hip_stream) {
  int rc = check_fit("gauss_fit_points", image_dev, image_dtype, H, W, points_dev, n, size, model, mask, sigma0, tol, max_iter, params_dev,
                     iterations_dev, status_dev);
  if (rc) return rc;
  if (points_dtype != ZK_I32 && points_dtype != ZK_F64) return zk_fail(ZK_E_BADARG, "gauss_fit_points: points are ZK_F64 or ZK_I32");
  ZK_ON_DEVICE(device);
  return fit_call("gauss_fit_points", image_dtype, model,
                  fit_args{image_dev, H, W, points_dev, points_dtype, n, (int)size, mask, sigma0, tol, (int)max_iter, params_dev, iterations_dev,
                           status_dev, nullptr, (hipStream_t)hip_stream});
}

extern "C" int zk_gauss_fit(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* corners_host, int64_t n,
                            int64_t size, int model, int mask, double sigma0, double tol, int64_t max_iter, double* params_out,
                            int32_t* iterations_out, int32_t* status_out) {
  int rc = check_fit("gauss_fit", image_host, image_dtype, H, W, corners_host, n, size, model, mask, sigma0, tol, max_iter, params_out,
                     iterations_out, status_out);
  if (rc) return rc;
  if (!corners_inside(corners_host, n, size, H, W)) return window_fail("gauss_fit");   // before anything is launched
  if (n == 0) return 0;
  ZK_ON_DEVICE(device);
  const size_t count = (size_t)n;
  const size_t img_bytes = zk_elem_size(image_dtype) * (size_t)H * (size_t)W, corner_bytes = sizeof(int32_t) * 2 * count,
               par_bytes = sizeof(double) * 8 * count, int_bytes = sizeof(int32_t) * count;
  dev_buf d_img, d_corners, d_par, d_it, d_status;
  if ((rc = d_img.upload(image_host, img_bytes)) || (rc = d_corners.upload(corners_host, corner_bytes)) || (rc = d_par.alloc(par_bytes)) ||
      (rc = d_it.alloc(int_bytes)) || (rc = d_status.alloc(int_bytes)) ||
      (rc = fit_call("gauss_fit", image_dtype, model,
                     fit_args{d_img.p, H, W, d_corners.p, CORNERS, n, (int)size, mask, sigma0, tol, (int)max_iter, d_par.as<double>(),
                              d_it.as<int>(), d_status.as<int>(), nullptr, (hipStream_t)0})) ||
      (rc = d_par.download(params_out, par_bytes)) || (rc = d_it.download(iterations_out, int_bytes)))
    return rc;
  return d_status.download(status_out, int_bytes);
}
