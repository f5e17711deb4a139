// zk_strain.hip -- geometric phase analysis (Hytch, Snoeck, Kilaas, Ultramicroscopy 74, 131 (1998)): the strain and rotation
// maps of every frame of a (B, H, W) stack from the phases of two Bragg spots.  No reference counterpart: the reference
// package has nothing on strain.  The contract is written out in include/zernike_hip.h.
//
//   widen_kernel          frame * (wy[y] * wx[x]) as a complex float64 field (zk_frames.h, the kernel of the registration);
//                         hipFFT transforms it in place (plans of zk_pickers.h): F.
//   mask_kernel           one read of F writes F M_1 and F M_2, M_k the Gaussian of width sigma around g_k on the wrapped
//                         frequency grid; one batched inverse transform then covers the 2 n planes of a run: H_k (H W).
//   ref_parts_kernel      the four phase gradients dP_k/dr_a summed over the reference rectangle, one partial per 4096 of its
//                         pixels and a fixed tree inside the block; ref_fold_kernel folds a frame's partials with the same
//                         tree, divides once: m[k][a], and G = g + m / (2 pi).  No atomics.  Without a rectangle the fold
//                         runs over no partials: m = 0 and G = g, so the strain kernel has one form.
//   strain_kernel         one pixel per lane along the rows: the 5-point stencil of both planes (read through L2: a lane's
//                         left and right neighbours are its wave's own loads, the rows above and below are another wave's
//                         lines, and the arithmetic -- four atan2 and a hypot per plane -- outweighs them), minus m, through
//                         inv(G) formed by the lane from m in device memory: exx, eyy, exy, rotation, both amplitudes and,
//                         when asked, both display phases and the planes themselves.
//
// The phase gradient is arg(H[r + 1] conj(H[r - 1]) c2) / 2 inside and arg(H[r'] conj(H[r' - 1]) c1) at the two edges, with
// c1 = exp(-2 pi i g), c2 = exp(-4 pi i g) per axis from the host: nothing is unwrapped and nothing grows with y or x.
//
// Frames go in runs whose three complex fields stay under RUN_BYTES (zk_gpa_set_run_bytes: another budget); no kernel looks
// across frames, so a frame's numbers do not depend on the run length.
#include <algorithm>
#include <cmath>

#include "zk_frames.h"

namespace {

constexpr int RED_PER_BLOCK = 4096;                // reference pixels per 256-thread block of the reduction
constexpr size_t RUN_BYTES = (size_t)1 << 30;      // the spectrum and the two planes of one run
constexpr int MAX_RUN = 32767;                     // 2 n planes are the y extent of a grid

// what the kernels know about a call; [k]: the Bragg vector, [a]: 0 = y, 1 = x
struct gpa_par {
  double g[2][2];
  cplx c1[2][2], c2[2][2];                         // exp(-2 pi i g[k][a]), exp(-4 pi i g[k][a])
  double two_s2;                                   // 2 sigma^2
  int H, W;
  int y0, y1, x0, x1;                              // the reference rectangle, half open; y1 == y0: none
};

// F (n, H W) -> FM (n, 2, H W): FM[b][k] = F[b] M_k
__global__ __launch_bounds__(256) void mask_kernel(const cplx* __restrict__ F, cplx* __restrict__ FM, gpa_par p, long long per) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= per) return;
  const long long b = blockIdx.y;
  const int ky = (int)(t / p.W), kx = (int)(t - (long long)ky * p.W);
  const double fy = (double)wrapped_lag(ky, p.H) * (1.0 / (double)p.H);  // numpy.fft.fftfreq: k times 1 / n
  const double fx = (double)wrapped_lag(kx, p.W) * (1.0 / (double)p.W);
  const cplx f = F[b * per + t];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double dy = fy - p.g[k][0], dx = fx - p.g[k][1];
    dy -= rint(dy);
    dx -= rint(dx);
    const double m = exp(-(dy * dy + dx * dx) / p.two_s2);
    cplx o;
    o.x = f.x * m;
    o.y = f.y * m;
    FM[(2 * b + k) * per + t] = o;
  }
}

// arg(a conj(b) c)
__device__ __forceinline__ double arg3(cplx a, cplx b, cplx c) {
  const double zr = a.x * b.x + a.y * b.y, zi = a.y * b.x - a.x * b.y;
  return atan2(zr * c.y + zi * c.x, zr * c.x - zi * c.y);
}

// the phase gradient of plane P along one axis at sample `at`, the i-th of n (n >= 2) samples `step` apart
__device__ __forceinline__ double phase_gradient(const cplx* __restrict__ P, long long at, long long step, int i, int n, cplx c1, cplx c2) {
  if (i == 0) return arg3(P[at + step], P[at], c1);
  if (i == n - 1) return arg3(P[at], P[at - step], c1);
  return 0.5 * arg3(P[at + step], P[at - step], c2);
}

// d[2 k + a] = dP_k/dr_a at (y, x) of the frame whose planes are P0 and P0 + per
__device__ __forceinline__ void gradients(const cplx* __restrict__ P0, long long per, const gpa_par& p, int y, int x, double d[4]) {
  const long long at = (long long)y * p.W + x;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const cplx* __restrict__ P = P0 + k * per;
    d[2 * k] = phase_gradient(P, at, p.W, y, p.H, p.c1[k][0], p.c2[k][0]);
    d[2 * k + 1] = phase_gradient(P, at, 1, x, p.W, p.c1[k][1], p.c2[k][1]);
  }
}

// the block's four sums to thread 0: a fixed tree of 8 levels
__device__ __forceinline__ void block_sum4(double s[4]) {
  __shared__ double s_s[4][256];
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) s_s[i][t] = s[i];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_s[i][t] += s_s[i][t + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = s_s[i][0];
}

// Grid (partials per frame, n): parts (n, gridDim.x, 4), the sums of the four gradients over RED_PER_BLOCK pixels of the rectangle
__global__ __launch_bounds__(256) void ref_parts_kernel(const cplx* __restrict__ Hk, gpa_par p, long long per, double* __restrict__ parts) {
  const long long b = blockIdx.y;
  const int rw = p.x1 - p.x0;
  const long long roi = (long long)(p.y1 - p.y0) * rw;
  const long long first = (long long)blockIdx.x * RED_PER_BLOCK;
  const long long last = first + RED_PER_BLOCK < roi ? first + RED_PER_BLOCK : roi;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long q = first + threadIdx.x; q < last; q += 256) {
    const int ry = (int)(q / rw), rx = (int)(q - (long long)ry * rw);
    double d[4];
    gradients(Hk + 2 * b * per, per, p, p.y0 + ry, p.x0 + rx, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += d[i];
  }
  block_sum4(s);
  if (threadIdx.x < 4) parts[(b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = s[threadIdx.x];
}

// Grid (n): m (n, 4) = the partials' sum / roi (roi 0: no rectangle, m = 0) and G (n, 4) = g + m / (2 pi)
__global__ __launch_bounds__(256) void ref_fold_kernel(const double* __restrict__ parts, int n_parts, long long roi, gpa_par p,
                                                       double* __restrict__ m, double* __restrict__ G) {
  const long long b = blockIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < n_parts; k += 256) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += parts[(b * n_parts + k) * 4 + i];
  }
  block_sum4(s);
  const int i = threadIdx.x;
  if (i < 4) {
    const double mean = roi ? s[i] / (double)roi : 0.0;
    m[b * 4 + i] = mean;
    G[b * 4 + i] = p.g[i >> 1][i & 1] + mean / (2.0 * M_PI);
  }
}

// Grid (blocks per frame, n).  maps: exx, eyy, exy, rotation of the run, `map_pitch` doubles apart, each (n, H W); amp, phase
// and planes (n, 2, H W); phase and planes may be null.  scale = 1 / (H W): the inverse transform's.
__global__ __launch_bounds__(256) void strain_kernel(const cplx* __restrict__ Hk, const double* __restrict__ m, gpa_par p, long long per,
                                                     double scale, double* __restrict__ maps, long long map_pitch, double* __restrict__ amp,
                                                     double* __restrict__ phase, cplx* __restrict__ planes) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= per) return;
  const long long b = blockIdx.y;
  const int y = (int)(t / p.W), x = (int)(t - (long long)y * p.W);
  const cplx* __restrict__ P0 = Hk + 2 * b * per;
  double d[4], G[4];
  gradients(P0, per, p, y, x, d);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double mean = m[b * 4 + i];
    d[i] -= mean;
    G[i] = p.g[i >> 1][i & 1] + mean / (2.0 * M_PI);
  }
  // inv(G)[j][k] of G[k][a] = G[2 k + a]; e[j][a] = -(1 / 2 pi) sum_k inv(G)[j][k] dP_k/dr_a
  const double det = G[0] * G[3] - G[1] * G[2];
  const double i00 = G[3] / det, i01 = -G[1] / det, i10 = -G[2] / det, i11 = G[0] / det;
  const double f = -1.0 / (2.0 * M_PI);
  const double eyy = f * (i00 * d[0] + i01 * d[2]), eyx = f * (i00 * d[1] + i01 * d[3]);
  const double exy = f * (i10 * d[0] + i11 * d[2]), exx = f * (i10 * d[1] + i11 * d[3]);
  double* __restrict__ out = maps + b * per + t;
  out[0] = exx;
  out[map_pitch] = eyy;
  out[2 * map_pitch] = 0.5 * (exy + eyx);
  out[3 * map_pitch] = 0.5 * (eyx - exy);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const cplx h = P0[k * per + t];
    const long long o = (2 * b + k) * per + t;
    amp[o] = hypot(h.x, h.y) * scale;
    if (planes) {
      cplx v;
      v.x = h.x * scale;
      v.y = h.y * scale;
      planes[o] = v;
    }
    if (phase) {
      double c = p.g[k][0] * (double)y + p.g[k][1] * (double)x, sn, cs;
      c -= floor(c);
      sincos(2.0 * M_PI * c, &sn, &cs);
      phase[o] = atan2(h.y * cs - h.x * sn, h.x * cs + h.y * sn);  // arg(h exp(-2 pi i c))
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
zk_device_bytes g_run_bytes;  // zk_gpa_set_run_bytes; 0: RUN_BYTES

struct job {
  int dtype;
  int64_t B, H, W;
  int window;
  gpa_par par;
  size_t per() const { return (size_t)H * W; }
  long long roi() const { return (long long)(par.y1 - par.y0) * (par.x1 - par.x0); }
};

cplx unit(double turns) {
  cplx e;
  e.x = cos(2.0 * M_PI * turns);
  e.y = sin(2.0 * M_PI * turns);
  return e;
}

// everything but the device and the output pointers; fills j
int check_job(job& j, const void* stack, int dtype, int64_t B, int64_t H, int64_t W, const double* g, double sigma, int window, const int64_t* ref,
              const void* maps, const void* amp, const void* g_out) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "gpa: dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (B < 1 || B >= ((int64_t)1 << 31) || H < 4 || W < 4 || H > 16384 || W > 16384)
    return zk_fail(ZK_E_BADARG, "gpa: needs 1 .. 2^31 - 1 frames of 4 x 4 .. 16384 x 16384 samples");
  if (window != ZK_GPA_WINDOW_NONE && window != ZK_GPA_WINDOW_HANN) return zk_fail(ZK_E_BADARG, "gpa: window must be one of ZK_GPA_WINDOW_*");
  if (!stack || !g || !maps || !amp || !g_out) return zk_fail(ZK_E_BADARG, "gpa: null pointer");
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(g[i]) || fabs(g[i]) > 0.5) return zk_fail(ZK_E_BADARG, "gpa: the components of g must be finite and within 0.5 cycles per pixel");
  const double n0 = hypot(g[0], g[1]), n1 = hypot(g[2], g[3]);
  if (n0 == 0.0 || n1 == 0.0 || fabs(g[0] * g[3] - g[1] * g[2]) <= 1e-6 * n0 * n1)
    return zk_fail(ZK_E_BADARG, "gpa: the rows of g must be non-zero and not collinear");
  if (!std::isfinite(sigma) || sigma <= 0.0) return zk_fail(ZK_E_BADARG, "gpa: sigma must be finite and positive");
  if (ref && (ref[0] < 0 || ref[1] <= ref[0] || ref[1] > H || ref[2] < 0 || ref[3] <= ref[2] || ref[3] > W))
    return zk_fail(ZK_E_BADARG, "gpa: the reference rectangle (y0, y1, x0, x1) must be non-empty and inside the frame");
  j.dtype = dtype;
  j.B = B;
  j.H = H;
  j.W = W;
  j.window = window;
  gpa_par& p = j.par;
  for (int k = 0; k < 2; ++k)
    for (int a = 0; a < 2; ++a) {
      p.g[k][a] = g[2 * k + a];
      p.c1[k][a] = unit(-g[2 * k + a]);
      p.c2[k][a] = unit(-2.0 * g[2 * k + a]);
    }
  p.two_s2 = 2.0 * sigma * sigma;
  p.H = (int)H;
  p.W = (int)W;
  p.y0 = ref ? (int)ref[0] : 0;
  p.y1 = ref ? (int)ref[1] : 0;
  p.x0 = ref ? (int)ref[2] : 0;
  p.x1 = ref ? (int)ref[3] : 0;
  return 0;
}

inline int parts_of(long long n) { return (int)((n + RED_PER_BLOCK - 1) / RED_PER_BLOCK); }

int run_length(const job& j, int device) {
  const int64_t n = std::max<int64_t>(1, (int64_t)(g_run_bytes.get(device, RUN_BYTES) / (j.per() * 48)));
  return (int)std::min<int64_t>(std::min<int64_t>(n, j.B), MAX_RUN);
}

// everything a call keeps on the device: the spectra of a run, its 2 n planes, the partial sums and m
struct state {
  int chunk = 0, n_parts = 0;
  dev_buf field, planes, win, parts, mean;
  stream_plan fwd, fwd_tail, inv, inv_tail;
  hipStream_t s = nullptr;
};

int prepare(state& st, const job& j, int device, hipStream_t s) {
  int rc;
  const int H = (int)j.H, W = (int)j.W;
  const size_t per = j.per();
  st.s = s;
  st.chunk = run_length(j, device);
  st.n_parts = parts_of(j.roi());
  const size_t n = (size_t)st.chunk;
  if ((rc = st.field.alloc(n * per * 16)) || (rc = st.planes.alloc(2 * n * per * 16)) || (rc = st.win.alloc((size_t)(H + W) * 8)) ||
      (rc = st.parts.alloc(n * st.n_parts * 32)) || (rc = st.mean.alloc(n * 32)))
    return rc;
  if ((rc = st.fwd.make(H, W, st.chunk, s)) || (rc = st.inv.make(H, W, 2 * st.chunk, s))) return rc;
  hipLaunchKernelGGL(window_table_kernel, dim3(blocks_of(H + W)), dim3(256), 0, s, st.win.as<double>(), H, W, j.window == ZK_GPA_WINDOW_HANN ? 1 : 0);
  ZK_HIP(hipGetLastError());
  return 0;
}

// n <= st.chunk frames at frames_dev; runs follow each other in order on st.s.  maps: the run's rows of the four maps,
// map_pitch doubles apart; amp, phase, planes (n, 2, H W) and g_out (n, 4): the run's rows.
int run_frames(state& st, const job& j, const void* frames_dev, int n, double* maps, long long map_pitch, double* amp, double* g_out, double* phase,
               cplx* planes) {
  int rc;
  const int H = (int)j.H, W = (int)j.W;
  const long long per = (long long)j.per();
  hipStream_t s = st.s;
  cplx* F = st.field.as<cplx>();
  cplx* Hk = st.planes.as<cplx>();
  stream_plan *fwd = &st.fwd, *inv = &st.inv;
  if (n != st.chunk) {
    if ((rc = st.fwd_tail.make(H, W, n, s)) || (rc = st.inv_tail.make(H, W, 2 * n, s))) return rc;
    fwd = &st.fwd_tail;
    inv = &st.inv_tail;
  }
  if ((rc = launch_widen(j.dtype, frames_dev, st.win.as<double>(), H, W, F, (long long)n * per, s))) return rc;
  ZK_FFT(zk_fft.ExecZ2Z(fwd->p.h, F, F, HIPFFT_FORWARD));
  hipLaunchKernelGGL(mask_kernel, dim3(blocks_of(per), n), dim3(256), 0, s, F, Hk, j.par, per);
  ZK_HIP(hipGetLastError());
  ZK_FFT(zk_fft.ExecZ2Z(inv->p.h, Hk, Hk, HIPFFT_BACKWARD));
  if (st.n_parts) {
    hipLaunchKernelGGL(ref_parts_kernel, dim3(st.n_parts, n), dim3(256), 0, s, Hk, j.par, per, st.parts.as<double>());
    ZK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(ref_fold_kernel, dim3(n), dim3(256), 0, s, st.parts.as<double>(), st.n_parts, j.roi(), j.par, st.mean.as<double>(), g_out);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(strain_kernel, dim3(blocks_of(per), n), dim3(256), 0, s, Hk, st.mean.as<double>(), j.par, per, 1.0 / (double)per, maps, map_pitch,
                     amp, phase, planes);
  ZK_HIP(hipGetLastError());
  return 0;
}

zk_device_stage g_host[ZK_DEVICE_TABLE];  // the staging of the host entry point (zk_ring.h)

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_gpa_set_run_bytes(int device, int64_t bytes) {
  return g_run_bytes.set(device, bytes, "gpa_set_run_bytes: bytes must be >= 0 (0: the default)");
}

extern "C" int zk_gpa_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, const double* g, double sigma, int window,
                          const int64_t* reference, double* maps_dev, double* amp_dev, double* g_out_dev, double* phase_dev, void* planes_dev,
                          void* hip_stream) {
  job j;
  int rc = check_job(j, stack_dev, dtype, B, H, W, g, sigma, window, reference, maps_dev, amp_dev, g_out_dev);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE)) || (rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t per = j.per(), frame_bytes = per * zk_elem_size(dtype);
  state st;
  rc = prepare(st, j, device, s);
  for (int64_t first = 0; first < B && !rc; first += st.chunk) {
    const int n = (int)std::min<int64_t>(st.chunk, B - first);
    rc = run_frames(st, j, (const char*)stack_dev + (size_t)first * frame_bytes, n, maps_dev + (size_t)first * per, (long long)B * (long long)per,
                    amp_dev + 2 * (size_t)first * per, g_out_dev + 4 * first, phase_dev ? phase_dev + 2 * (size_t)first * per : nullptr,
                    planes_dev ? (cplx*)planes_dev + 2 * (size_t)first * per : nullptr);
  }
  const hipError_t e = hipStreamSynchronize(s);  // the fields are freed on return, whatever happened
  if (rc) return rc;
  ZK_HIP(e);
  return 0;
}

extern "C" int zk_gpa(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, const double* g, double sigma, int window,
                      const int64_t* reference, double* maps_host, double* amp_host, double* g_out_host, double* phase_host, void* planes_host) {
  job j;
  int rc = check_job(j, stack_host, dtype, B, H, W, g, sigma, window, reference, maps_host, amp_host, g_out_host);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE)) || (rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  std::lock_guard<std::mutex> guard(g_host[device].lock);
  zk_stage* h = &g_host[device].stage;
  if ((rc = zk_stage_create(h))) return rc;
  zk_ring* r = &h->ring;
  const size_t per = j.per(), in_unit = per * zk_elem_size(dtype);
  // a frame's share of a slot's output, in doubles per pixel: four maps, two amplitudes, two phases, two complex planes
  const size_t amp_at = 4, phase_at = 6, planes_at = phase_at + (phase_host ? 2 : 0), out_doubles = planes_at + (planes_host ? 4 : 0);
  dev_buf d_g;  // G of every frame
  if ((rc = d_g.alloc((size_t)B * 32))) return rc;
  state st;
  rc = prepare(st, j, device, h->stream);
  if (!rc) {
    const zk_chunks ch{B, st.chunk, (B + st.chunk - 1) / st.chunk};
    const size_t run = (size_t)ch.chunk * per;  // doubles of one map of a full run
    rc = zk_ring_run(
        r, h->stream, ch.n_chunks,
        [&](int64_t c, int slot) -> int {
          int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, run * out_doubles * 8);
          if (!e) e = zk_ring_up(r, h->stream, c, slot, r->d_in[slot], (const char*)stack_host + (size_t)ch.first(c) * in_unit, (size_t)ch.count(c) * in_unit);
          if (e) return e;
          double* out = (double*)r->d_out[slot];
          return run_frames(st, j, r->d_in[slot], (int)ch.count(c), out, (long long)run, out + amp_at * run, d_g.as<double>() + 4 * ch.first(c),
                            phase_host ? out + phase_at * run : nullptr, planes_host ? (cplx*)(out + planes_at * run) : nullptr);
        },
        [&](int64_t c, int slot) -> int {
          const size_t n = (size_t)ch.count(c) * per, f = (size_t)ch.first(c) * per;
          const double* out = (const double*)r->d_out[slot];
          for (size_t q = 0; q < 4; ++q)
            ZK_HIP(hipMemcpyAsync(maps_host + q * (size_t)B * per + f, out + q * run, n * 8, hipMemcpyDeviceToHost, r->s_out));
          ZK_HIP(hipMemcpyAsync(amp_host + 2 * f, out + amp_at * run, 2 * n * 8, hipMemcpyDeviceToHost, r->s_out));
          if (phase_host) ZK_HIP(hipMemcpyAsync(phase_host + 2 * f, out + phase_at * run, 2 * n * 8, hipMemcpyDeviceToHost, r->s_out));
          if (planes_host) ZK_HIP(hipMemcpyAsync((double*)planes_host + 4 * f, out + planes_at * run, 4 * n * 8, hipMemcpyDeviceToHost, r->s_out));
          return 0;
        });
  } else {
    (void)hipStreamSynchronize(h->stream);
  }
  zk_stage_trim(h, ZK_STAGE_KEEP_STACKS);
  if (rc) return rc;  // zk_ring_run has drained every stream: the fields may go
  return d_g.download(g_out_host, (size_t)B * 32);
}
