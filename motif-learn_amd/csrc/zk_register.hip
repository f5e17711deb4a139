// zk_register.hip -- stack registration: the rigid sub-pixel drift of every frame of a (B, H, W) stack against a reference
// frame (Guizar-Sicairos, Thurman, Fienup, Opt. Lett. 33, 156 (2008)), and the ordered float64 mean of a stack.  No reference
// counterpart: the reference package has no registration.  The contract is written out in include/zernike_hip.h.
//
//   widen_kernel          frame * (wy[y] * wx[x]) as a complex float64 field (the window table is 1 or the periodic Hann window,
//                         window_table_kernel; both in zk_frames.h, shared with zk_strain.hip); hipFFT transforms it in place
//                         (plans of zk_pickers.h).
//   cross_power_kernel    P = R conj(F) into a second field, R the reference's spectrum (slot 0) or the frame before; with the
//                         phase normalisation it leaves max|P| per block, frame_max_kernel folds them per frame and
//                         phase_kernel divides by max(|P|, 100 eps max|P|).
//   argmax_parts_kernel   the first maximum (larger value, else smaller flat index) of real(ifft2(P)) / (H W) over the lags with
//                         |wrapped lag| <= max_shift, one partial per 4096 samples and a fixed tree inside the block;
//                         coarse_kernel folds a frame's partials with the same tree: the coarse lag (y0, x0).
//   twiddle_kernel        Ey (S, H) and Ex (W, S) of every frame: exp(2 pi i k (y0 u + j - off) / (u n)) with the integer product
//                         reduced modulo u n first, so the phase keeps every bit whatever the size of k y.
//   product_kernel        C = A B of complex float64 matrices, batched: 64 x 64 outputs per workgroup, 4 x 4 per lane, slices of
//                         16 through LDS (the A slice transposed, pitch 65: the stores of a slice and the 128-bit reads of a
//                         row spread over the banks); rows, columns and depth past the edge are zero in LDS and not stored.
//                         Once as T = Ey P (S, W), once as real(T Ex) / (H W) (S, S), where only the real part is accumulated.
//                         A lane sums its k in ascending order: no atomics, two runs agree bit for bit.
//   fine_kernel           the first maximum of C in row-major order -> shift = y0 + (j - off) / u and peak.
//   mean_kernel           out[p] = (sum over b ascending of stack[b, p]) / B in float64, one pixel per lane.
//
// Frames go in runs whose two complex fields stay under 1 GiB; a frame's numbers do not depend on the run length.
#include <math.h>

#include <algorithm>

#include "zk_frames.h"

namespace {

constexpr int RED_PER_BLOCK = 4096;                    // samples per 256-thread block of the reductions
constexpr int GT = 64;                                 // rows and columns of a workgroup's output tile
constexpr int GK = 16;                                 // depth of an LDS slice
constexpr int GA_PITCH = GT + 1;                       // complex numbers between the k rows of the transposed A slice
constexpr size_t FIELD_BYTES = (size_t)1 << 30;        // the two complex fields of one run
constexpr size_t TABLE_BYTES = (size_t)1 << 30;        // twiddle tables, T and C of one run
constexpr size_t MEAN_BUDGET = (size_t)256 << 20;      // input + output of one chunk of zk_stack_mean

struct partial {
  double v;
  long long idx;  // flat index in the frame; -1: none
};

// does (av, ai) come before (bv, bi)?  The larger value, else the smaller index; non-finite values are not defined.
__device__ __forceinline__ bool first_max(double av, long long ai, double bv, long long bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  if (av != bv) return av > bv;
  return ai < bi;
}

// the block's first maximum to every thread: a fixed tree of 8 levels
__device__ __forceinline__ void block_first_max(double& v, long long& idx) {
  __shared__ double v_s[256];
  __shared__ long long i_s[256];
  const int t = threadIdx.x;
  v_s[t] = v;
  i_s[t] = idx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o && first_max(v_s[t + o], i_s[t + o], v_s[t], i_s[t])) {
      v_s[t] = v_s[t + o];
      i_s[t] = i_s[t + o];
    }
    __syncthreads();
  }
  v = v_s[0];
  idx = i_s[0];
  __syncthreads();
}

__device__ __forceinline__ double block_max(double v) {
  __shared__ double m_s[256];
  const int t = threadIdx.x;
  m_s[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) m_s[t] = fmax(m_s[t], m_s[t + o]);
    __syncthreads();
  }
  v = m_s[0];
  __syncthreads();
  return v;
}

// field: slot 0 and the n frames of the run behind it.  P[b] = field[r] conj(field[b + 1]), r = 0 or (previous) b.
// Grid (blocks per frame, n); part_max (n, gridDim.x) when the phase normalisation wants max|P|.
__global__ __launch_bounds__(256) void cross_power_kernel(const cplx* __restrict__ field, int previous, cplx* __restrict__ P, long long per,
                                                          double* __restrict__ part_max) {
  const int b = blockIdx.y;
  const cplx* __restrict__ R = field + (previous ? (long long)b * per : 0);
  const cplx* __restrict__ F = field + (long long)(b + 1) * per;
  const long long first = (long long)blockIdx.x * RED_PER_BLOCK;
  const long long last = first + RED_PER_BLOCK < per ? first + RED_PER_BLOCK : per;
  double m = 0.0;
  for (long long t = first + threadIdx.x; t < last; t += 256) {
    const cplx r = R[t], f = F[t];
    cplx p;
    p.x = r.x * f.x + r.y * f.y;
    p.y = r.y * f.x - r.x * f.y;
    P[b * per + t] = p;
    if (part_max) m = fmax(m, hypot(p.x, p.y));
  }
  if (part_max) {
    m = block_max(m);
    if (threadIdx.x == 0) part_max[(long long)b * gridDim.x + blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(256) void frame_max_kernel(const double* __restrict__ part_max, int n_parts, double* __restrict__ frame_max) {
  const int b = blockIdx.x;
  double m = 0.0;
  for (int k = threadIdx.x; k < n_parts; k += 256) m = fmax(m, part_max[(long long)b * n_parts + k]);
  m = block_max(m);
  if (threadIdx.x == 0) frame_max[b] = m;
}

__global__ __launch_bounds__(256) void phase_kernel(cplx* __restrict__ P, long long per, const double* __restrict__ frame_max) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= per) return;
  const int b = blockIdx.y;
  cplx p = P[b * per + t];
  const double d = fmax(hypot(p.x, p.y), 100.0 * 2.220446049250313e-16 * frame_max[b]);
  p.x /= d;
  p.y /= d;
  P[b * per + t] = p;
}

// value t of frame b is vals[(b per + t) stride] * scale (stride 2: the real parts of a complex field).  rows x cols is the
// frame; max_shift >= 0 keeps the samples whose wrapped lags are within it on both axes.  plane_out (n, per): the values.
__global__ __launch_bounds__(256) void argmax_parts_kernel(const double* __restrict__ vals, int stride, double scale, int rows, int cols,
                                                           long long max_shift, partial* __restrict__ parts, double* __restrict__ plane_out) {
  const long long per = (long long)rows * cols;
  const int b = blockIdx.y;
  const long long first = (long long)blockIdx.x * RED_PER_BLOCK;
  const long long last = first + RED_PER_BLOCK < per ? first + RED_PER_BLOCK : per;
  double best = 0.0;
  long long at = -1;
  for (long long t = first + threadIdx.x; t < last; t += 256) {
    const double v = vals[(b * per + t) * stride] * scale;
    if (plane_out) plane_out[b * per + t] = v;
    if (max_shift >= 0) {
      const int y = (int)(t / cols), x = (int)(t - (long long)y * cols);
      if (abs(wrapped_lag(y, rows)) > max_shift || abs(wrapped_lag(x, cols)) > max_shift) continue;
    }
    if (first_max(v, t, best, at)) {
      best = v;
      at = t;
    }
  }
  block_first_max(best, at);
  if (threadIdx.x == 0) parts[(long long)b * gridDim.x + blockIdx.x] = partial{best, at};
}

__device__ __forceinline__ void fold_parts(const partial* __restrict__ parts, int n_parts, double& best, long long& at) {
  best = 0.0;
  at = -1;
  for (int k = threadIdx.x; k < n_parts; k += 256) {
    const partial p = parts[(long long)blockIdx.x * n_parts + k];
    if (first_max(p.v, p.idx, best, at)) {
      best = p.v;
      at = p.idx;
    }
  }
  block_first_max(best, at);
}

// partials of frame b -> its coarse lag (y0, x0); with `last` that is the answer
__global__ __launch_bounds__(256) void coarse_kernel(const partial* __restrict__ parts, int n_parts, int H, int W, int32_t* __restrict__ coarse,
                                                     int last, double* __restrict__ shifts, double* __restrict__ peak) {
  double best;
  long long at;
  fold_parts(parts, n_parts, best, at);
  if (threadIdx.x) return;
  const int b = blockIdx.x;
  if (at < 0) at = 0;  // lag 0 is inside every mask: only non-finite data comes here
  const int ly = wrapped_lag((int)(at / W), H), lx = wrapped_lag((int)(at % W), W);
  coarse[2 * b] = ly;
  coarse[2 * b + 1] = lx;
  if (last) {
    shifts[2 * b] = (double)ly;
    shifts[2 * b + 1] = (double)lx;
    peak[b] = best;
  }
}

// partials of the upsampled plane (S, S) of frame b -> shift = coarse + (j - off) / u, the oracle's own float64 expression
__global__ __launch_bounds__(256) void fine_kernel(const partial* __restrict__ parts, int n_parts, int S, int off, int u,
                                                   const int32_t* __restrict__ coarse, double* __restrict__ shifts, double* __restrict__ peak) {
  double best;
  long long at;
  fold_parts(parts, n_parts, best, at);
  if (threadIdx.x) return;
  const int b = blockIdx.x;
  if (at < 0) at = 0;
  const int j = (int)(at / S), i = (int)(at % S);
  shifts[2 * b] = (double)coarse[2 * b] + (double)(j - off) / (double)u;
  shifts[2 * b + 1] = (double)coarse[2 * b + 1] + (double)(i - off) / (double)u;
  peak[b] = best;
}

// exp(2 pi i k q / m) for integers: k q is reduced modulo m (to |r| <= m / 2) before it meets 2 pi / m
__device__ __forceinline__ cplx unit_root(long long k, long long q, long long m) {
  long long r = (k * q) % m;
  if (2 * r > m) r -= m;
  if (2 * r < -m) r += m;
  cplx e;
  sincos(2.0 * M_PI * (double)r / (double)m, &e.y, &e.x);
  return e;
}

// Ey (n, S, H): Ey[b][j][k] = exp(2 pi i ys[j] fftfreq(H)[k]), ys[j] = y0 + (j - off) / u; Ex (n, W, S) likewise, transposed
__global__ __launch_bounds__(256) void twiddle_kernel(const int32_t* __restrict__ coarse, int H, int W, int S, int off, int u,
                                                      cplx* __restrict__ Ey, cplx* __restrict__ Ex) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ny = (long long)S * H, nx = (long long)W * S;
  if (t >= ny + nx) return;
  const int b = blockIdx.y;
  if (t < ny) {
    const int j = (int)(t / H), k = (int)(t - (long long)j * H);
    Ey[b * ny + t] = unit_root(wrapped_lag(k, H), (long long)coarse[2 * b] * u + (j - off), (long long)u * H);
  } else {
    const long long e = t - ny;
    const int k = (int)(e / S), i = (int)(e - (long long)k * S);
    Ex[b * nx + e] = unit_root(wrapped_lag(k, W), (long long)coarse[2 * b + 1] * u + (i - off), (long long)u * W);
  }
}

// out[z] (M, N) = scale * A[z] (M, K) B[z] (K, N), row-major and dense; REAL_OUT: only the real part, as float64.
// Grid (ceil(N / 64), ceil(M / 64), batch).  Lane (tx, ty) owns rows ty + 16 r and columns tx + 16 c, r, c < 4.
template <bool REAL_OUT>
__global__ __launch_bounds__(256) void product_kernel(const cplx* __restrict__ A, const cplx* __restrict__ Bm, void* __restrict__ out_v, int M,
                                                      int N, int K, double scale) {
  __shared__ cplx a_s[GK * GA_PITCH];  // [k][row]
  __shared__ cplx b_s[GK * GT];        // [k][column]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long z = blockIdx.z;
  const int row0 = blockIdx.y * GT, col0 = blockIdx.x * GT;
  const cplx* __restrict__ Az = A + z * M * K;
  const cplx* __restrict__ Bz = Bm + z * K * N;
  double re[4][4], im[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) re[r][c] = im[r][c] = 0.0;

  for (int k0 = 0; k0 < K; k0 += GK) {
    if (k0) __syncthreads();  // every lane is done with the slice before
#pragma unroll
    for (int e = tid; e < GT * GK; e += 256) {
      const int r = e / GK, k = e - r * GK;  // 16 consecutive k of a row: 256 B
      cplx v = {0.0, 0.0};
      if (row0 + r < M && k0 + k < K) v = Az[(long long)(row0 + r) * K + k0 + k];
      a_s[k * GA_PITCH + r] = v;
    }
#pragma unroll
    for (int e = tid; e < GK * GT; e += 256) {
      const int k = e / GT, c = e - k * GT;
      cplx v = {0.0, 0.0};
      if (k0 + k < K && col0 + c < N) v = Bz[(long long)(k0 + k) * N + col0 + c];
      b_s[k * GT + c] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < GK; ++k) {
      cplx a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = a_s[k * GA_PITCH + ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = b_s[k * GT + tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          re[r][c] = fma(a[r].x, b[c].x, re[r][c]);
          re[r][c] = fma(-a[r].y, b[c].y, re[r][c]);
          if (!REAL_OUT) {
            im[r][c] = fma(a[r].x, b[c].y, im[r][c]);
            im[r][c] = fma(a[r].y, b[c].x, im[r][c]);
          }
        }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + ty + 16 * r;
    if (row >= M) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = col0 + tx + 16 * c;
      if (col >= N) continue;
      const long long o = (z * M + row) * N + col;
      if (REAL_OUT) {
        ((double*)out_v)[o] = re[r][c] * scale;
      } else {
        cplx v;
        v.x = re[r][c] * scale;
        v.y = im[r][c] * scale;
        ((cplx*)out_v)[o] = v;
      }
    }
  }
}

// out[t] = (in[0][t] + in[1][t] + ... in ascending order) / B for t < count; `pitch` samples between the frames
template <typename T>
__global__ __launch_bounds__(256) void mean_kernel(const T* __restrict__ in, long long B, long long pitch, long long count,
                                                   double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  double s = 0.0;
  for (long long b = 0; b < B; ++b) s += (double)in[b * pitch + t];
  out[t] = s / (double)B;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct job {
  int dtype;
  int64_t B, H, W;
  int ref_mode;
  int64_t ref_index;
  int ref_dtype, upsample;
  int64_t max_shift;
  int normalization, window;
  size_t per() const { return (size_t)H * W; }
  int S() const { return (3 * upsample + 1) / 2; }  // ceil(1.5 upsample)
  int off() const { return S() / 2; }
  size_t up_per() const { return upsample > 1 ? (size_t)S() * S() : 0; }
};

int check_job(const job& j, const void* stack, const void* ref, const void* shifts, const void* peak) {
  if (!zk_is_elem(j.dtype)) return zk_fail(ZK_E_BADARG, "register_shifts: dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (j.B < 1 || j.B >= ((int64_t)1 << 31) || j.H < 2 || j.W < 2 || j.H > 16384 || j.W > 16384)
    return zk_fail(ZK_E_BADARG, "register_shifts: needs 1 .. 2^31 - 1 frames of 2 x 2 .. 16384 x 16384 samples");
  if (j.upsample < 1 || j.upsample > 1000) return zk_fail(ZK_E_BADARG, "register_shifts: upsample must be in 1 .. 1000");
  if (j.max_shift < -1) return zk_fail(ZK_E_BADARG, "register_shifts: max_shift must be >= 0, or -1 for every lag");
  if (j.normalization != ZK_REGISTER_NORM_NONE && j.normalization != ZK_REGISTER_NORM_PHASE)
    return zk_fail(ZK_E_BADARG, "register_shifts: normalization must be one of ZK_REGISTER_NORM_*");
  if (j.window != ZK_REGISTER_WINDOW_NONE && j.window != ZK_REGISTER_WINDOW_HANN)
    return zk_fail(ZK_E_BADARG, "register_shifts: window must be one of ZK_REGISTER_WINDOW_*");
  if (j.ref_mode == ZK_REGISTER_REF_INDEX) {
    if (j.ref_index < 0 || j.ref_index >= j.B) return zk_fail(ZK_E_BADARG, "register_shifts: the reference index is outside the stack");
  } else if (j.ref_mode == ZK_REGISTER_REF_FRAME) {
    if (!ref) return zk_fail(ZK_E_BADARG, "register_shifts: null pointer");
    if (!zk_is_elem(j.ref_dtype)) return zk_fail(ZK_E_BADARG, "register_shifts: ref_dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  } else if (j.ref_mode != ZK_REGISTER_REF_PREVIOUS) {
    return zk_fail(ZK_E_BADARG, "register_shifts: ref_mode must be one of ZK_REGISTER_REF_*");
  }
  if (!stack || !shifts || !peak) return zk_fail(ZK_E_BADARG, "register_shifts: null pointer");
  return 0;
}

inline int parts_of(size_t n) { return (int)((n + RED_PER_BLOCK - 1) / RED_PER_BLOCK); }

// everything a call keeps on the device: slot 0 of `field` is the reference's spectrum (or the spectrum of the frame before the
// run), slots 1 .. chunk the run's frames -- their spectra, then their correlation planes; `power` is P
struct state {
  int chunk = 0, n_parts = 0, up_parts = 0;
  dev_buf field, power, win, parts, part_max, frame_max, coarse, ey, ex, t, c;
  stream_plan plan, plan_tail, plan_one;
  hipStream_t s = nullptr;
};

int run_length(const job& j) {
  int64_t n = std::max<int64_t>(1, (int64_t)(FIELD_BYTES / (j.per() * 32)));
  if (j.upsample > 1) {
    const size_t tables = ((size_t)j.S() * (j.H + 2 * j.W) * 2 + j.up_per()) * 8;
    n = std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)(TABLE_BYTES / tables)));
  }
  return (int)std::min<int64_t>(std::min<int64_t>(n, j.B), 65535);
}

// ref_dev: the reference frame on the device (not for ZK_REGISTER_REF_PREVIOUS)
int prepare(state& st, const job& j, const void* ref_dev, int ref_dtype, hipStream_t s) {
  int rc;
  const int H = (int)j.H, W = (int)j.W, S = j.S();
  const size_t per = j.per();
  st.s = s;
  st.chunk = run_length(j);
  st.n_parts = parts_of(per);
  st.up_parts = parts_of(j.up_per());
  const size_t n = (size_t)st.chunk;
  if ((rc = st.field.alloc((n + 1) * per * 16)) || (rc = st.power.alloc(n * per * 16)) || (rc = st.win.alloc((size_t)(H + W) * 8)) ||
      (rc = st.parts.alloc(n * std::max(st.n_parts, st.up_parts) * sizeof(partial))) || (rc = st.coarse.alloc(n * 8)))
    return rc;
  if (j.normalization == ZK_REGISTER_NORM_PHASE && ((rc = st.part_max.alloc(n * st.n_parts * 8)) || (rc = st.frame_max.alloc(n * 8)))) return rc;
  if (j.upsample > 1 && ((rc = st.ey.alloc(n * S * H * 16)) || (rc = st.ex.alloc(n * W * S * 16)) || (rc = st.t.alloc(n * S * W * 16)) ||
                         (rc = st.c.alloc(n * j.up_per() * 8))))
    return rc;
  if ((rc = st.plan.make(H, W, st.chunk, s))) return rc;
  hipLaunchKernelGGL(window_table_kernel, dim3(blocks_of(H + W)), dim3(256), 0, s, st.win.as<double>(), H, W,
                     j.window == ZK_REGISTER_WINDOW_HANN ? 1 : 0);
  ZK_HIP(hipGetLastError());
  if (j.ref_mode == ZK_REGISTER_REF_PREVIOUS) return 0;
  if ((rc = launch_widen(ref_dtype, ref_dev, st.win.as<double>(), H, W, st.field.as<cplx>(), (long long)per, s))) return rc;
  stream_plan* one = &st.plan;
  if (st.chunk != 1) {
    if ((rc = st.plan_one.make(H, W, 1, s))) return rc;
    one = &st.plan_one;
  }
  ZK_FFT(zk_fft.ExecZ2Z(one->p.h, st.field.as<cplx>(), st.field.as<cplx>(), HIPFFT_FORWARD));
  return 0;
}

// frames [first, first + n) of the stack, n <= st.chunk, at frames_dev; runs follow each other in order on st.s.
// shifts (n, 2) and peak (n) are the run's rows; corr (n, H, W) and up (n, S, S) are optional.
int run_frames(state& st, const job& j, const void* frames_dev, int64_t first, int n, double* shifts, double* peak, double* corr, double* up) {
  int rc;
  const int H = (int)j.H, W = (int)j.W, S = j.S(), u = j.upsample;
  const long long per = (long long)j.per();
  const bool previous = j.ref_mode == ZK_REGISTER_REF_PREVIOUS, phase = j.normalization == ZK_REGISTER_NORM_PHASE;
  hipStream_t s = st.s;
  cplx* slot0 = st.field.as<cplx>();
  cplx* frames = slot0 + per;
  cplx* P = st.power.as<cplx>();
  stream_plan* plan = &st.plan;
  if (n != st.chunk) {
    if (n == 1 && st.plan_one.bound) {
      plan = &st.plan_one;
    } else {
      if ((rc = st.plan_tail.make(H, W, n, s))) return rc;
      plan = &st.plan_tail;
    }
  }
  if ((rc = launch_widen(j.dtype, frames_dev, st.win.as<double>(), H, W, frames, (long long)n * per, s))) return rc;
  ZK_FFT(zk_fft.ExecZ2Z(plan->p.h, frames, frames, HIPFFT_FORWARD));
  if (previous && first == 0) ZK_HIP(hipMemcpyAsync(slot0, frames, (size_t)per * 16, hipMemcpyDeviceToDevice, s));  // frame 0 meets itself
  hipLaunchKernelGGL(cross_power_kernel, dim3(st.n_parts, n), dim3(256), 0, s, slot0, previous ? 1 : 0, P, per,
                     phase ? st.part_max.as<double>() : nullptr);
  ZK_HIP(hipGetLastError());
  if (previous) ZK_HIP(hipMemcpyAsync(slot0, frames + (long long)(n - 1) * per, (size_t)per * 16, hipMemcpyDeviceToDevice, s));
  if (phase) {
    hipLaunchKernelGGL(frame_max_kernel, dim3(n), dim3(256), 0, s, st.part_max.as<double>(), st.n_parts, st.frame_max.as<double>());
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(phase_kernel, dim3(blocks_of(per), n), dim3(256), 0, s, P, per, st.frame_max.as<double>());
    ZK_HIP(hipGetLastError());
  }
  ZK_FFT(zk_fft.ExecZ2Z(plan->p.h, P, frames, HIPFFT_BACKWARD));  // P stays for the upsampled transform
  hipLaunchKernelGGL(argmax_parts_kernel, dim3(st.n_parts, n), dim3(256), 0, s, (const double*)frames, 2, 1.0 / (double)per, H, W,
                     (long long)j.max_shift, st.parts.as<partial>(), corr);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(coarse_kernel, dim3(n), dim3(256), 0, s, st.parts.as<partial>(), st.n_parts, H, W, st.coarse.as<int32_t>(), u == 1 ? 1 : 0,
                     shifts, peak);
  ZK_HIP(hipGetLastError());
  if (u == 1) return 0;
  double* C = up ? up : st.c.as<double>();
  hipLaunchKernelGGL(twiddle_kernel, dim3(blocks_of((long long)S * (H + W)), n), dim3(256), 0, s, st.coarse.as<int32_t>(), H, W, S, j.off(), u,
                     st.ey.as<cplx>(), st.ex.as<cplx>());
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(product_kernel<false>, dim3(blocks_of(W, GT), blocks_of(S, GT), n), dim3(256), 0, s, st.ey.as<cplx>(), P, st.t.p, S, W, H, 1.0);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(product_kernel<true>, dim3(blocks_of(S, GT), blocks_of(S, GT), n), dim3(256), 0, s, st.t.as<cplx>(), st.ex.as<cplx>(), (void*)C,
                     S, S, W, 1.0 / (double)per);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(argmax_parts_kernel, dim3(st.up_parts, n), dim3(256), 0, s, (const double*)C, 1, 1.0, S, S, (long long)-1, st.parts.as<partial>(),
                     (double*)nullptr);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fine_kernel, dim3(n), dim3(256), 0, s, st.parts.as<partial>(), st.up_parts, S, j.off(), u, st.coarse.as<int32_t>(), shifts, peak);
  ZK_HIP(hipGetLastError());
  return 0;
}

int launch_mean(int dtype, const void* in, int64_t B, long long pitch, long long count, double* out, hipStream_t s) {
  zk_with_elem(dtype, [&](auto e) {
    using T = typename decltype(e)::type;
    hipLaunchKernelGGL(mean_kernel<T>, dim3(blocks_of(count)), dim3(256), 0, s, (const T*)in, (long long)B, pitch, count, out);
  });
  ZK_HIP(hipGetLastError());
  return 0;
}

int check_mean(const void* stack, int dtype, int64_t B, int64_t H, int64_t W, const void* out) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "stack_mean: dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (B < 1 || H < 1 || W < 1 || H > ((int64_t)1 << 21) || W > ((int64_t)1 << 21) || B >= ((int64_t)1 << 31) || B * H * W >= ((int64_t)1 << 40))
    return zk_fail(ZK_E_BADARG, "stack_mean: needs B, H, W positive, H, W <= 2^21, B < 2^31 and fewer than 2^40 samples");
  if (!stack || !out) return zk_fail(ZK_E_BADARG, "stack_mean: null pointer");
  return 0;
}

zk_device_stage g_host[ZK_DEVICE_TABLE];  // the staging of the host entry points (zk_ring.h)

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_register_shifts_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, int ref_mode,
                                      int64_t ref_index, const void* ref_dev, int ref_dtype, int upsample, int64_t max_shift, int normalization,
                                      int window, double* shifts_dev, double* peak_dev, double* corr_dev, double* up_dev, void* hip_stream) {
  const job j{dtype, B, H, W, ref_mode, ref_index, ref_dtype, upsample, max_shift, normalization, window};
  int rc = check_job(j, stack_dev, ref_dev, shifts_dev, peak_dev);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE)) || (rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t frame_bytes = j.per() * zk_elem_size(dtype);
  const bool by_index = ref_mode == ZK_REGISTER_REF_INDEX;
  state st;
  if ((rc = prepare(st, j, by_index ? (const char*)stack_dev + (size_t)ref_index * frame_bytes : ref_dev, by_index ? dtype : ref_dtype, s))) return rc;
  for (int64_t first = 0; first < B && !rc; first += st.chunk) {
    const int n = (int)std::min<int64_t>(st.chunk, B - first);
    rc = run_frames(st, j, (const char*)stack_dev + (size_t)first * frame_bytes, first, n, shifts_dev + 2 * first, peak_dev + first,
                    corr_dev ? corr_dev + (size_t)first * j.per() : nullptr, up_dev ? up_dev + (size_t)first * j.up_per() : nullptr);
  }
  const hipError_t e = hipStreamSynchronize(s);  // the fields are freed on return, whatever happened
  if (rc) return rc;
  ZK_HIP(e);
  return 0;
}

extern "C" int zk_register_shifts(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, int ref_mode, int64_t ref_index,
                                  const void* ref_host, int ref_dtype, int upsample, int64_t max_shift, int normalization, int window,
                                  double* shifts_host, double* peak_host, double* corr_host, double* up_host) {
  const job j{dtype, B, H, W, ref_mode, ref_index, ref_dtype, upsample, max_shift, normalization, window};
  int rc = check_job(j, stack_host, ref_host, shifts_host, peak_host);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE)) || (rc = zk_fft_load())) return rc;
  ZK_ON_DEVICE(device);
  std::lock_guard<std::mutex> guard(g_host[device].lock);
  zk_stage* h = &g_host[device].stage;
  if ((rc = zk_stage_create(h))) return rc;
  zk_ring* r = &h->ring;
  const size_t per = j.per(), up_per = j.up_per(), in_unit = per * zk_elem_size(dtype);
  const bool by_index = ref_mode == ZK_REGISTER_REF_INDEX;
  const size_t shift_bytes = (size_t)B * 16, peak_bytes = (size_t)B * 8, ref_bytes = per * zk_elem_size(by_index ? dtype : ref_dtype);
  // the reference frame: one of the stack's, the caller's, or none (every frame against the one before it)
  const void* ref_src = ref_mode == ZK_REGISTER_REF_PREVIOUS ? nullptr : by_index ? (const char*)stack_host + (size_t)ref_index * in_unit : ref_host;
  dev_buf d_ref, d_res;                              // d_res: the shifts, then the peaks
  if ((rc = d_res.alloc(shift_bytes + peak_bytes)) || (rc = d_ref.upload(ref_src, ref_bytes))) return rc;
  state st;
  rc = prepare(st, j, d_ref.p, by_index ? dtype : ref_dtype, h->stream);
  if (!rc) {
    double* d_shifts = d_res.as<double>();
    double* d_peak = d_shifts + 2 * B;
    const zk_chunks ch{B, st.chunk, (B + st.chunk - 1) / st.chunk};
    const size_t corr_unit = corr_host ? per * 8 : 0, up_unit = up_host ? up_per * 8 : 0;
    rc = zk_ring_run(
        r, h->stream, ch.n_chunks,
        [&](int64_t c, int slot) -> int {
          int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, (size_t)ch.chunk * (corr_unit + up_unit));
          if (!e) e = zk_ring_up(r, h->stream, c, slot, r->d_in[slot], (const char*)stack_host + (size_t)ch.first(c) * in_unit, (size_t)ch.count(c) * in_unit);
          if (e) return e;
          double* d_corr = corr_unit ? (double*)r->d_out[slot] : nullptr;
          double* d_up = up_unit ? (double*)r->d_out[slot] + (corr_unit ? (size_t)ch.chunk * per : 0) : nullptr;
          return run_frames(st, j, r->d_in[slot], ch.first(c), (int)ch.count(c), d_shifts + 2 * ch.first(c), d_peak + ch.first(c), d_corr, d_up);
        },
        [&](int64_t c, int slot) -> int {
          const size_t n = (size_t)ch.count(c), f = (size_t)ch.first(c);
          if (corr_unit) ZK_HIP(hipMemcpyAsync(corr_host + f * per, r->d_out[slot], n * corr_unit, hipMemcpyDeviceToHost, r->s_out));
          if (up_unit)
            ZK_HIP(hipMemcpyAsync(up_host + f * up_per, (double*)r->d_out[slot] + (corr_unit ? (size_t)ch.chunk * per : 0), n * up_unit,
                                  hipMemcpyDeviceToHost, r->s_out));
          return 0;
        });
  } else {
    (void)hipStreamSynchronize(h->stream);
  }
  zk_stage_trim(h, ZK_STAGE_KEEP_STACKS);
  if (rc) return rc;  // zk_ring_run has drained every stream: the fields may go
  if ((rc = d_res.download(shifts_host, shift_bytes))) return rc;
  ZK_HIP(hipMemcpy(peak_host, d_res.as<double>() + 2 * B, peak_bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int zk_stack_mean_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, double* out_dev, void* hip_stream) {
  int rc = check_mean(stack_dev, dtype, B, H, W, out_dev);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  return launch_mean(dtype, stack_dev, B, (long long)H * W, (long long)H * W, out_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_stack_mean(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, double* out_host) {
  int rc = check_mean(stack_host, dtype, B, H, W, out_host);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  std::lock_guard<std::mutex> guard(g_host[device].lock);
  zk_stage* h = &g_host[device].stage;
  if ((rc = zk_stage_create(h))) return rc;
  zk_ring* r = &h->ring;
  const size_t es = zk_elem_size(dtype);
  const int64_t per = H * W;
  const zk_chunks ch = zk_chunk_plan(MEAN_BUDGET, (size_t)B * es + 8, 256, per);  // chunks of pixels, every frame's share of each
  rc = zk_ring_run(
      r, h->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * B * es, (size_t)ch.chunk * 8);
        if (!e)
          e = zk_ring_up_2d(r, h->stream, c, slot, r->d_in[slot], (size_t)ch.chunk * es, (const char*)stack_host + (size_t)ch.first(c) * es,
                            (size_t)per * es, (size_t)ch.count(c) * es, (size_t)B);
        return e ? e : launch_mean(dtype, r->d_in[slot], B, (long long)ch.chunk, (long long)ch.count(c), (double*)r->d_out[slot], h->stream);
      },
      [&](int64_t c, int slot) -> int { return zk_ring_down(r, slot, out_host + ch.first(c), (size_t)ch.count(c) * 8); });
  zk_stage_trim(h, ZK_STAGE_KEEP_STACKS);
  return rc;
}
