// zk_window_size.hip -- device side of the Fourier window-size estimators and the angular spectrum average (reference
// features/_window_size.py: compute_autocorrelation, get_characteristic_length, get_characteristic_length_fft;
// features/_fft_related.py: fft_power_spectrum, angular_average), each batched over a stack of B frames (B, H, W).
//
//   magnitude     magnitude_reduce_kernel writes |z| (or |z| / (H W) after the inverse transform, or log(|z| + 1)) at the
//                 fft-shifted position and, in the same pass, reduces each frame to its FIRST maximum in C order (numpy.argmax:
//                 the first NaN, else the larger value, else the smaller index) and to its min / max (warp_polar's clip rule).
//                 A block covers RED_PER_BLOCK consecutive outputs of one frame and leaves one partial; finalize_kernel (one
//                 block per frame) turns the partials into the centre table (B, 2) and the min / max table the polar profile
//                 of zk_pickers.hip reads.  The autocorrelation route runs the same reduction over its real map.
//   1-D tails     one workgroup per frame, the cut profile line[0:i] in LDS:
//                 fft_tail_kernel    SNIP in the reference's operation order (v = log(log(sqrt(y + 1) + 1) + 1); niter Jacobi
//                                    sweeps v[e] = min(v[e], (v[e + pp] + v[e - pp]) / 2) on pp <= e < n - pp between two LDS
//                                    arrays; bg = (exp(exp(v) - 1) - 1)^2 - 1), y1 = y - bg, the running mean of `size` samples
//                                    with reflected edges (scipy.ndimage.uniform_filter1d, mode 'reflect', origin 0: samples
//                                    e - size / 2 .. e + size - size / 2 - 1) and its first maximum.
//                 peak_tail_kernel   the first peak of scipy.signal.find_peaks without conditions (_local_maxima_1d): a sample
//                                    above its left neighbour whose plateau ends in a lower sample; the plateau's midpoint
//                                    (left + right) / 2.  -1 when there is none.
//   angular       angular_kernel: every pixel goes to the bin with edges[i] <= theta < edges[i + 1] of the HOST's
//                 numpy.linspace(0, 360, num_bins + 1) (binary search in the table; a theta of 360.0 falls in no bin), theta =
//                 degrees(atan2(dy, dx)) mod 360 in float64.  The eight directions on which a pixel can sit exactly on an edge
//                 (dy == 0, dx == 0, |dx| == |dy|: the multiples of 45 degrees) take their exact values instead of atan2's
//                 last bit; the circular mask is dx^2 + dy^2 <= min(cy, cx)^2 in integers.  A lane walks ANG_RUN consecutive
//                 pixels and adds a run that shares a bin once; per-bin float64 sums and counts go through a per-workgroup LDS
//                 table (up to ANG_LDS_BINS bins) flushed once per workgroup, or straight to global atomics above that.  Counts
//                 are exact; sums depend on the order of the atomics in their last bits.
#include <math.h>

#include <algorithm>
#include <vector>

#include "zk_internal.h"
#include "zk_pickers.h"
#include "zk_scratch.h"

namespace {

constexpr int RED_PER_BLOCK = 4096;  // outputs per 256-thread block of the magnitude / reduction pass
constexpr int ANG_RUN = 16;          // consecutive pixels per lane of the angular reduction
constexpr int ANG_LDS_BINS = 4096;   // 48 KiB of LDS: float64 sums and 32-bit counts
constexpr int TAIL_MAX = 8192;       // samples of a cut profile the tail kernels hold twice in LDS (128 KiB)

struct partial {
  double v;
  long long idx;  // flat index in the frame; -1: none
  double lo, hi;
};

// does (av, ai) come before (bv, bi) under numpy.argmax?
__device__ __forceinline__ bool first_max(double av, long long ai, double bv, long long bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}

// the block's first maximum (and min / max) to thread 0
__device__ __forceinline__ void block_first_max(double& v, long long& idx, double& lo, double& hi) {
  __shared__ double v_s[256], lo_s[256], hi_s[256];
  __shared__ long long i_s[256];
  const int t = threadIdx.x;
  v_s[t] = v;
  i_s[t] = idx;
  lo_s[t] = lo;
  hi_s[t] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      if (first_max(v_s[t + o], i_s[t + o], v_s[t], i_s[t])) {
        v_s[t] = v_s[t + o];
        i_s[t] = i_s[t + o];
      }
      lo_s[t] = fmin(lo_s[t], lo_s[t + o]);
      hi_s[t] = fmax(hi_s[t], hi_s[t + o]);
    }
    __syncthreads();
  }
  v = v_s[0];
  idx = i_s[0];
  lo = lo_s[0];
  hi = hi_s[0];
  __syncthreads();
}

// frames (optionally standardised with stats[2 b], stats[2 b + 1]) as a complex field
template <typename T>
__global__ __launch_bounds__(256) void load_kernel(const T* __restrict__ in, const double* __restrict__ stats, long long per,
                                                   cplx* __restrict__ out, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  double v = (double)in[t];
  if (stats) {
    const long long b = t / per;
    v = (v - stats[2 * b]) / stats[2 * b + 1];
  }
  out[t].x = v;
  out[t].y = 0.0;
}

__global__ __launch_bounds__(256) void square_kernel(cplx* __restrict__ z, long long total) {  // F conj(F)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const double re = z[t].x, im = z[t].y;
  z[t].x = re * re + im * im;
  z[t].y = 0.0;
}

// z != null: out[b][i][j] = f(|scale z[b][(i - H/2) mod H][(j - W/2) mod W]|) (numpy.fft.fftshift), f = log(. + 1) with
// use_log; z == null: the values are out's own (reduction only).  Either way parts[b][block] = the block's first maximum and
// min / max.  Grid (blocks per frame, B).
__global__ __launch_bounds__(256) void magnitude_reduce_kernel(const cplx* __restrict__ z, int H, int W, double scale, int use_log,
                                                               double* __restrict__ out, partial* __restrict__ parts) {
  const long long per = (long long)H * W;
  const int b = blockIdx.y;
  const long long first = (long long)blockIdx.x * RED_PER_BLOCK;
  const long long last = first + RED_PER_BLOCK < per ? first + RED_PER_BLOCK : per;
  double best = 0.0, lo = INFINITY, hi = -INFINITY;
  long long at = -1;
  for (long long t = first + threadIdx.x; t < last; t += 256) {
    double v;
    if (z) {
      const int i = (int)(t / W), j = (int)(t - (long long)i * W);
      const cplx c = z[b * per + (long long)((i - H / 2 + H) % H) * W + (j - W / 2 + W) % W];
      v = hypot(c.x * scale, c.y * scale);
      if (use_log) v = log(v + 1.0);
      out[b * per + t] = v;
    } else {
      v = out[b * per + t];
    }
    if (first_max(v, t, best, at)) {
      best = v;
      at = t;
    }
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  block_first_max(best, at, lo, hi);
  if (threadIdx.x == 0) parts[(long long)b * gridDim.x + blockIdx.x] = partial{best, at, lo, hi};
}

// partials of frame b -> its centre (row, col) and its min / max
__global__ __launch_bounds__(256) void finalize_kernel(const partial* __restrict__ parts, int n_parts, int W, int32_t* __restrict__ centres,
                                                       double* __restrict__ mm) {
  const int b = blockIdx.x;
  double best = 0.0, lo = INFINITY, hi = -INFINITY;
  long long at = -1;
  for (int k = threadIdx.x; k < n_parts; k += 256) {
    const partial p = parts[(long long)b * n_parts + k];
    if (first_max(p.v, p.idx, best, at)) {
      best = p.v;
      at = p.idx;
    }
    lo = fmin(lo, p.lo);
    hi = fmax(hi, p.hi);
  }
  block_first_max(best, at, lo, hi);
  if (threadIdx.x == 0) {
    centres[2 * b] = (int32_t)(at / W);
    centres[2 * b + 1] = (int32_t)(at % W);
    mm[2 * b] = lo;
    mm[2 * b + 1] = hi;
  }
}

// index of the first maximum of v[0 .. n) (n >= 1) over the block
__device__ __forceinline__ int block_argmax(const double* v, int n) {
  double best = 0.0, lo = 0.0, hi = 0.0;
  long long at = -1;
  for (int e = threadIdx.x; e < n; e += 256)
    if (first_max(v[e], e, best, at)) {
      best = v[e];
      at = e;
    }
  block_first_max(best, at, lo, hi);
  return (int)at;
}

__global__ __launch_bounds__(256) void fft_tail_kernel(const double* __restrict__ prof, int R, const int32_t* __restrict__ centres,
                                                       int niter, int size, double* __restrict__ y2_out, int32_t* __restrict__ ind_out) {
  extern __shared__ double lds[];
  const int b = blockIdx.x;
  const int n = centres[2 * b] < R ? centres[2 * b] : R;
  const double* y = prof + (long long)b * R;
  if (n <= 0) {  // an empty profile has no argmax
    if (threadIdx.x == 0) ind_out[b] = -1;
    return;
  }
  double* cur = lds;
  double* nxt = lds + n;
  for (int e = threadIdx.x; e < n; e += 256) cur[e] = log(log(sqrt(y[e] + 1.0) + 1.0) + 1.0);
  __syncthreads();
  for (int pp = 1; pp <= niter && 2 * pp < n; ++pp) {  // a sweep with 2 pp >= n changes nothing
    for (int e = threadIdx.x; e < n; e += 256) {
      double v = cur[e];
      if (e >= pp && e < n - pp) {
        const double r = (cur[e + pp] + cur[e - pp]) * 0.5;
        v = r < v ? r : v;
      }
      nxt[e] = v;
    }
    __syncthreads();
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int e = threadIdx.x; e < n; e += 256) {
    const double t = exp(exp(cur[e]) - 1.0) - 1.0;
    nxt[e] = y[e] - (t * t - 1.0);
  }
  __syncthreads();
  const int period = 2 * n;
  for (int e = threadIdx.x; e < n; e += 256) {
    double s = 0.0;
    for (int k = 0; k < size; ++k) {
      int q = (e + k - size / 2) % period;  // half-sample mirror, repeated: d c b a | a b c d | d c b a
      if (q < 0) q += period;
      if (q >= n) q = period - 1 - q;
      s += nxt[q];
    }
    cur[e] = s / (double)size;
    if (y2_out) y2_out[(long long)b * R + e] = cur[e];
  }
  __syncthreads();
  const int at = block_argmax(cur, n);
  if (threadIdx.x == 0) ind_out[b] = at;
}

__global__ __launch_bounds__(256) void peak_tail_kernel(const double* __restrict__ prof, int R, const int32_t* __restrict__ centres,
                                                        int32_t* __restrict__ peak_out) {
  extern __shared__ double lds[];
  __shared__ int first;
  const int b = blockIdx.x;
  const int n = centres[2 * b] < R ? centres[2 * b] : R;
  const double* y = prof + (long long)b * R;
  if (threadIdx.x == 0) first = 0x7fffffff;
  for (int e = threadIdx.x; e < n; e += 256) lds[e] = y[e];
  __syncthreads();
  for (int e = 1 + threadIdx.x; e < n - 1; e += 256) {
    if (!(lds[e - 1] < lds[e])) continue;
    int ahead = e + 1;
    while (ahead < n - 1 && lds[ahead] == lds[e]) ++ahead;
    if (lds[ahead] < lds[e]) atomicMin(&first, (e + ahead - 1) / 2);
  }
  __syncthreads();
  if (threadIdx.x == 0) peak_out[b] = first == 0x7fffffff ? -1 : first;
}

// numpy: degrees(arctan2(dy, dx)) % 360 for integer offsets
__device__ __forceinline__ double angle_degrees(int dy, int dx) {
  if (dy == 0) return dx >= 0 ? 0.0 : 180.0;
  if (dx == 0) return dy > 0 ? 90.0 : 270.0;
  if (dx == dy) return dx > 0 ? 45.0 : 225.0;
  if (dx == -dy) return dx < 0 ? 135.0 : 315.0;
  const double t = atan2((double)dy, (double)dx) * (180.0 / M_PI);
  double m = fmod(t, 360.0);
  if (m != 0.0) {
    if (m < 0.0) m += 360.0;
  } else {
    m = 0.0;
  }
  return m;
}

template <bool USE_LDS>
__global__ __launch_bounds__(256) void angular_kernel(const double* __restrict__ data, int H, int W, const double* __restrict__ edges, int nb,
                                                      int use_mask, double* __restrict__ sums, unsigned long long* __restrict__ counts) {
  __shared__ double s_sum[USE_LDS ? ANG_LDS_BINS : 1];
  __shared__ unsigned int s_cnt[USE_LDS ? ANG_LDS_BINS : 1];
  const int b = blockIdx.y;
  const long long per = (long long)H * W;
  const int cy = H / 2, cx = W / 2;
  const long long rmax = cy < cx ? cy : cx, rmax2 = rmax * rmax;
  if (USE_LDS) {
    for (int i = threadIdx.x; i < nb; i += 256) {
      s_sum[i] = 0.0;
      s_cnt[i] = 0u;
    }
    __syncthreads();
  }
  double* g_sum = sums + (long long)b * nb;
  unsigned long long* g_cnt = counts + (long long)b * nb;
  int bin_run = -1;
  double acc = 0.0;
  unsigned int cnt = 0;
  auto flush = [&]() {
    if (bin_run < 0 || cnt == 0) return;
    if (USE_LDS) {
      atomicAdd(&s_sum[bin_run], acc);
      atomicAdd(&s_cnt[bin_run], cnt);
    } else {
      atomicAdd(&g_sum[bin_run], acc);
      atomicAdd(&g_cnt[bin_run], (unsigned long long)cnt);
    }
  };
  const long long t0 = ((long long)blockIdx.x * 256 + threadIdx.x) * ANG_RUN;
  for (int k = 0; k < ANG_RUN; ++k) {
    const long long t = t0 + k;
    if (t >= per) break;
    const int yy = (int)(t / W), xx = (int)(t - (long long)yy * W);
    const int dy = yy - cy, dx = xx - cx;
    if (use_mask && (long long)dx * dx + (long long)dy * dy > rmax2) continue;
    const double theta = angle_degrees(dy, dx);
    int lo = 0, hi = nb;  // the largest i in [0, nb] with edges[i] <= theta (edges[0] = 0 <= theta)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (edges[mid] <= theta) lo = mid;
      else hi = mid - 1;
    }
    if (lo >= nb || !(edges[lo] <= theta)) continue;  // theta == 360.0 (or NaN) lies in no bin
    if (lo != bin_run) {
      flush();
      bin_run = lo;
      acc = 0.0;
      cnt = 0;
    }
    acc += data[b * per + t];
    ++cnt;
  }
  flush();
  if (USE_LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256)
      if (s_cnt[i]) {
        atomicAdd(&g_sum[i], s_sum[i]);
        atomicAdd(&g_cnt[i], (unsigned long long)s_cnt[i]);
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

int check_stack(const char* who, const void* p, int dtype, int64_t B, int64_t H, int64_t W) {
  const std::string name(who);
  if (dtype != ZK_F32 && dtype != ZK_F64) return zk_fail(ZK_E_BADARG, name + ": dtype must be ZK_F32 or ZK_F64");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 16384 || W > 16384 || B * H >= ((int64_t)1 << 31))
    return zk_fail(ZK_E_BADARG, name + ": needs 1 .. 65535 frames of at most 16384 x 16384 and fewer than 2^31 rows in all");
  if (!p) return zk_fail(ZK_E_BADARG, name + ": null pointer");
  return 0;
}

inline int parts_per_frame(int64_t H, int64_t W) { return (int)((H * W + RED_PER_BLOCK - 1) / RED_PER_BLOCK); }

// the frames of a stack as windows of the (B H, W) image they form
int frame_origins(dev_buf& d_org, int64_t B, int64_t H) {
  std::vector<int32_t> org((size_t)2 * B, 0);
  for (int64_t b = 0; b < B; ++b) org[(size_t)2 * b] = (int32_t)(b * H);
  return d_org.upload(org.data(), (size_t)B * 8);
}

// mean / std of every frame on the device; a constant frame is the reference's ValueError
int frame_stats(const void* d_img, int dtype, int64_t B, int64_t H, int64_t W, const int32_t* d_org, double* d_stats) {
  int rc = zk_window_stats_dev(d_img, dtype, W, d_org, (int)B, (int)H, (int)W, d_stats);
  if (rc) return rc;
  std::vector<double> st((size_t)2 * B);
  ZK_HIP(hipMemcpy(st.data(), d_stats, st.size() * 8, hipMemcpyDeviceToHost));
  for (int64_t b = 0; b < B; ++b)
    if (!(st[(size_t)2 * b + 1] > 0.0)) return zk_fail(ZK_E_BADARG, "Standard deviation is zero, can't standardize the image.");
  return 0;
}

// d_map (B, H, W) = |fftshift(fft2(frame))| (log(. + 1) with use_log), or with `autocorr` |fftshift(ifft2(F conj F))| of the
// frames standardised with d_stats (null: as they are); d_parts (B, parts_per_frame): the partials of the reduction
int magnitude_maps(const void* d_img, int dtype, const double* d_stats, int64_t B, int64_t H, int64_t W, int autocorr, int use_log,
                   double* d_map, partial* d_parts) {
  int rc;
  const long long per = (long long)H * W;
  const int n_parts = parts_per_frame(H, W);
  int chunk = (int)std::max<long long>(1, ((long long)1 << 30) / (per * 16));  // at most ~1 GiB of complex field
  chunk = (int)std::min<int64_t>(chunk, B);
  dev_buf d_z;
  if ((rc = d_z.alloc((size_t)chunk * per * 16))) return rc;
  zk_fft_plan plan, plan_tail;
  if ((rc = plan.make((int)H, (int)W, chunk))) return rc;
  const size_t es = zk_elem_size(dtype);
  for (int64_t first = 0; first < B; first += chunk) {
    const int nb = (int)std::min<int64_t>(chunk, B - first);
    zk_fft_plan* use = &plan;
    if (nb != chunk) {
      if ((rc = plan_tail.make((int)H, (int)W, nb))) return rc;
      use = &plan_tail;
    }
    const long long total = (long long)nb * per;
    const void* src = (const char*)d_img + (size_t)first * per * es;
    const double* st = d_stats ? d_stats + 2 * first : nullptr;
    if (dtype == ZK_F32)
      hipLaunchKernelGGL(load_kernel<float>, dim3(blocks_of(total)), dim3(256), 0, 0, (const float*)src, st, per, d_z.as<cplx>(), total);
    else
      hipLaunchKernelGGL(load_kernel<double>, dim3(blocks_of(total)), dim3(256), 0, 0, (const double*)src, st, per, d_z.as<cplx>(), total);
    ZK_HIP(hipGetLastError());
    ZK_FFT(zk_fft.ExecZ2Z(use->h, d_z.as<cplx>(), d_z.as<cplx>(), HIPFFT_FORWARD));
    if (autocorr) {
      hipLaunchKernelGGL(square_kernel, dim3(blocks_of(total)), dim3(256), 0, 0, d_z.as<cplx>(), total);
      ZK_HIP(hipGetLastError());
      ZK_FFT(zk_fft.ExecZ2Z(use->h, d_z.as<cplx>(), d_z.as<cplx>(), HIPFFT_BACKWARD));
    }
    hipLaunchKernelGGL(magnitude_reduce_kernel, dim3(n_parts, nb), dim3(256), 0, 0, d_z.as<cplx>(), (int)H, (int)W,
                       autocorr ? 1.0 / (double)per : 1.0, use_log, d_map + (size_t)first * per, d_parts + (size_t)first * n_parts);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipDeviceSynchronize());  // the field is freed on return
  return 0;
}

struct profile_stage {
  dev_buf centres, mm, prof;
  std::vector<int32_t> centres_host;
  int R = 0, n_max = 0;  // radii of a profile; longest cut profile of the stack
};

// partials -> centres and min / max -> the mean polar profiles about them, cut at the centre's row
int cut_profiles(profile_stage& ps, const double* d_map, const partial* d_parts, int64_t B, int64_t H, int64_t W) {
  int rc;
  ps.R = (int)zk_polar_radii(H, W);
  if ((rc = ps.centres.alloc((size_t)B * 8)) || (rc = ps.mm.alloc((size_t)B * 16)) || (rc = ps.prof.alloc((size_t)B * ps.R * 8))) return rc;
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)B), dim3(256), 0, 0, d_parts, parts_per_frame(H, W), (int)W, ps.centres.as<int32_t>(),
                     ps.mm.as<double>());
  ZK_HIP(hipGetLastError());
  if ((rc = zk_polar_profile_dev(d_map, (int)B, (int)H, (int)W, ps.centres.as<int32_t>(), 1, 0, ps.mm.as<double>(), ps.prof.as<double>())))
    return rc;
  ps.centres_host.resize((size_t)2 * B);
  ZK_HIP(hipMemcpy(ps.centres_host.data(), ps.centres.p, (size_t)B * 8, hipMemcpyDeviceToHost));
  ps.n_max = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int32_t ci = ps.centres_host[(size_t)2 * b], cj = ps.centres_host[(size_t)2 * b + 1];
    if (ci < 0 || ci >= H || cj < 0 || cj >= W) return zk_fail(ZK_E_BADARG, "window size: a frame has no maximum");
    ps.n_max = std::max(ps.n_max, std::min((int)ci, ps.R));
  }
  if (ps.n_max > TAIL_MAX) return zk_fail(ZK_E_BADARG, "window size: a cut profile longer than 8192 samples");
  return 0;
}

template <class K>
int tail_lds(K kernel, size_t bytes) {
  if (bytes > 65536) ZK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}

int download_profiles(const profile_stage& ps, int64_t B, int32_t* centres_host, double* profiles_host) {
  if (centres_host) std::copy(ps.centres_host.begin(), ps.centres_host.end(), centres_host);
  return ps.prof.download(profiles_host, (size_t)B * ps.R * 8);
}

int shifted_map(const char* who, int device, const void* images_host, int dtype, int64_t B, int64_t H, int64_t W, int autocorr,
                int standardize, int use_log, double* out_host) {
  int rc = check_stack(who, images_host, dtype, B, H, W);
  if (rc) return rc;
  if (!out_host) return zk_fail(ZK_E_BADARG, std::string(who) + ": null pointer");
  if ((rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  const size_t n = (size_t)B * H * W, map_bytes = n * 8;
  dev_buf d_img, d_org, d_stats, d_map, d_parts;
  if ((rc = d_img.upload(images_host, n * zk_elem_size(dtype))) || (rc = d_map.alloc(map_bytes)) ||
      (rc = d_parts.alloc((size_t)B * parts_per_frame(H, W) * sizeof(partial))))
    return rc;
  if (standardize && ((rc = frame_origins(d_org, B, H)) || (rc = d_stats.alloc((size_t)B * 16)) ||
                      (rc = frame_stats(d_img.p, dtype, B, H, W, d_org.as<int32_t>(), d_stats.as<double>()))))
    return rc;
  if ((rc = magnitude_maps(d_img.p, dtype, d_stats.as<double>(), B, H, W, autocorr, use_log, d_map.as<double>(), d_parts.as<partial>())))
    return rc;
  return d_map.download(out_host, map_bytes);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_circular_autocorr(int device, const void* images_host, int dtype, int64_t batch, int64_t H, int64_t W, int standardize,
                                    double* out_host) {
  return shifted_map("circular_autocorr", device, images_host, dtype, batch, H, W, 1, standardize, 0, out_host);
}

extern "C" int zk_shifted_magnitude(int device, const void* images_host, int dtype, int64_t batch, int64_t H, int64_t W, int use_log,
                                    double* out_host) {
  return shifted_map("shifted_magnitude", device, images_host, dtype, batch, H, W, 0, 0, use_log, out_host);
}

extern "C" int zk_char_length_fft(int device, const void* images_host, int dtype, int64_t B, int64_t H, int64_t W, int niter, int size,
                                  int use_log, int32_t* centres_host, double* profiles_host, double* smoothed_host, int32_t* ind_host) {
  int rc = check_stack("char_length_fft", images_host, dtype, B, H, W);
  if (rc) return rc;
  if (!ind_host) return zk_fail(ZK_E_BADARG, "char_length_fft: null pointer");
  if (niter < 0 || size < 1 || size > (1 << 20)) return zk_fail(ZK_E_BADARG, "char_length_fft: niter must be >= 0 and size in 1 .. 2^20");
  if ((rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  const size_t n = (size_t)B * H * W, ind_bytes = (size_t)B * 4;
  dev_buf d_img, d_map, d_parts, d_y2, d_ind;
  profile_stage ps;
  if ((rc = d_img.upload(images_host, n * zk_elem_size(dtype))) || (rc = d_map.alloc(n * 8)) ||
      (rc = d_parts.alloc((size_t)B * parts_per_frame(H, W) * sizeof(partial))) || (rc = d_ind.alloc(ind_bytes)) ||
      (rc = magnitude_maps(d_img.p, dtype, nullptr, B, H, W, 0, use_log, d_map.as<double>(), d_parts.as<partial>())) ||
      (rc = cut_profiles(ps, d_map.as<double>(), d_parts.as<partial>(), B, H, W)))
    return rc;
  const size_t y2_bytes = (size_t)B * ps.R * 8;
  if (smoothed_host) {                               // without it d_y2 stays null, which the kernel takes as "not wanted"
    if ((rc = d_y2.alloc(y2_bytes))) return rc;
    ZK_HIP(hipMemset(d_y2.p, 0, y2_bytes));
  }
  const size_t lds = (size_t)2 * std::max(ps.n_max, 1) * 8;
  if ((rc = tail_lds(fft_tail_kernel, lds))) return rc;
  hipLaunchKernelGGL(fft_tail_kernel, dim3((unsigned)B), dim3(256), lds, 0, ps.prof.as<double>(), ps.R, ps.centres.as<int32_t>(), niter, size,
                     d_y2.as<double>(), d_ind.as<int32_t>());
  ZK_HIP(hipGetLastError());
  if ((rc = d_ind.download(ind_host, ind_bytes)) || (rc = d_y2.download(smoothed_host, y2_bytes))) return rc;
  return download_profiles(ps, B, centres_host, profiles_host);
}

extern "C" int zk_char_length(int device, const void* images_host, int dtype, int64_t B, int64_t H, int64_t W, int standardize,
                              int32_t* centres_host, double* profiles_host, int32_t* peaks_host) {
  int rc = check_stack("char_length", images_host, dtype, B, H, W);
  if (rc) return rc;
  if (!peaks_host) return zk_fail(ZK_E_BADARG, "char_length: null pointer");
  if ((rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  const size_t n = (size_t)B * H * W, peak_bytes = (size_t)B * 4;
  const int n_parts = parts_per_frame(H, W);
  dev_buf d_img, d_org, d_stats, d_map, d_parts, d_peak;
  profile_stage ps;
  if ((rc = d_img.upload(images_host, n * zk_elem_size(dtype))) || (rc = d_map.alloc(n * 8)) ||
      (rc = d_parts.alloc((size_t)B * n_parts * sizeof(partial))) || (rc = d_peak.alloc(peak_bytes)) || (rc = frame_origins(d_org, B, H)))
    return rc;
  if (standardize && ((rc = d_stats.alloc((size_t)B * 16)) ||
                      (rc = frame_stats(d_img.p, dtype, B, H, W, d_org.as<int32_t>(), d_stats.as<double>()))))
    return rc;
  // scipy.signal.correlate(image, image, 'same', 'fft') of every frame: the windows of zk_autocorr_mean, one map each
  if ((rc = zk_autocorr_same_dev(d_img.p, dtype, W, d_org.as<int32_t>(), (int)B, (int)H, (int)W, d_stats.as<double>(), d_map.as<double>(), 1)))
    return rc;
  hipLaunchKernelGGL(magnitude_reduce_kernel, dim3(n_parts, (unsigned)B), dim3(256), 0, 0, (const cplx*)nullptr, (int)H, (int)W, 1.0, 0,
                     d_map.as<double>(), d_parts.as<partial>());
  ZK_HIP(hipGetLastError());
  if ((rc = cut_profiles(ps, d_map.as<double>(), d_parts.as<partial>(), B, H, W))) return rc;
  const size_t lds = (size_t)std::max(ps.n_max, 1) * 8;
  if ((rc = tail_lds(peak_tail_kernel, lds))) return rc;
  hipLaunchKernelGGL(peak_tail_kernel, dim3((unsigned)B), dim3(256), lds, 0, ps.prof.as<double>(), ps.R, ps.centres.as<int32_t>(),
                     d_peak.as<int32_t>());
  ZK_HIP(hipGetLastError());
  if ((rc = d_peak.download(peaks_host, peak_bytes))) return rc;
  return download_profiles(ps, B, centres_host, profiles_host);
}

extern "C" int zk_angular_average(int device, const double* spectra_host, int64_t B, int64_t H, int64_t W, const double* edges_host,
                                  int64_t num_bins, int use_mask, double* sums_host, int64_t* counts_host) {
  int rc = check_stack("angular_average", spectra_host, ZK_F64, B, H, W);
  if (rc) return rc;
  if (!edges_host || !sums_host || !counts_host) return zk_fail(ZK_E_BADARG, "angular_average: null pointer");
  if (num_bins < 1 || num_bins > (1 << 24)) return zk_fail(ZK_E_BADARG, "angular_average: needs 1 .. 2^24 bins");
  for (int64_t i = 0; i < num_bins; ++i)
    if (!(edges_host[i] < edges_host[i + 1])) return zk_fail(ZK_E_BADARG, "angular_average: the bin edges must increase");
  ZK_ON_DEVICE(device);
  const size_t n = (size_t)B * H * W, nb = (size_t)num_bins, bins_bytes = B * nb * 8;  // sums and counts alike
  dev_buf d_in, d_edges, d_sum, d_cnt;
  if ((rc = d_in.upload(spectra_host, n * 8)) || (rc = d_edges.upload(edges_host, (nb + 1) * 8)) || (rc = d_sum.alloc(bins_bytes)) ||
      (rc = d_cnt.alloc(bins_bytes)))
    return rc;
  ZK_HIP(hipMemset(d_sum.p, 0, bins_bytes));
  ZK_HIP(hipMemset(d_cnt.p, 0, bins_bytes));
  const dim3 grid(blocks_of((long long)H * W, 256 * ANG_RUN), (unsigned)B);
  if (num_bins <= ANG_LDS_BINS)
    hipLaunchKernelGGL(angular_kernel<true>, grid, dim3(256), 0, 0, d_in.as<double>(), (int)H, (int)W, d_edges.as<double>(), (int)num_bins,
                       use_mask, d_sum.as<double>(), d_cnt.as<unsigned long long>());
  else
    hipLaunchKernelGGL(angular_kernel<false>, grid, dim3(256), 0, 0, d_in.as<double>(), (int)H, (int)W, d_edges.as<double>(), (int)num_bins,
                       use_mask, d_sum.as<double>(), d_cnt.as<unsigned long long>());
  ZK_HIP(hipGetLastError());
  if ((rc = d_sum.download(sums_host, bins_bytes))) return rc;
  return d_cnt.download(counts_host, bins_bytes);
}
