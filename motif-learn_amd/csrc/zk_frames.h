// zk_frames.h -- what zk_register.hip shares with zk_strain.hip (not part of the public ABI): a stack of real frames widened
// and windowed into a complex float64 field, and a cached hipFFT plan bound to a stream for the length of a call.  (Both units
// stage their host-buffer entry points through zk_ring.h.)
#pragma once

#include <math.h>

#include "zk_pickers.h"
#include "zk_ring.h"
#include "zk_scratch.h"

namespace {

// numpy.fft.fftfreq(n, 1 / n)[k]
__device__ __forceinline__ int wrapped_lag(int k, int n) { return k <= (n - 1) / 2 ? k : k - n; }

// win[0 .. H) = wy, win[H .. H + W) = wx
__global__ __launch_bounds__(256) void window_table_kernel(double* __restrict__ win, int H, int W, int hann) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= H + W) return;
  const int n = t < H ? H : W, i = t < H ? t : t - H;
  win[t] = hann ? 0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)n) : 1.0;
}

template <typename T>
__global__ __launch_bounds__(256) void widen_kernel(const T* __restrict__ in, const double* __restrict__ win, int H, int W,
                                                    cplx* __restrict__ out, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long p = t % ((long long)H * W);
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  out[t].x = (double)in[t] * (win[y] * win[H + x]);
  out[t].y = 0.0;
}

int launch_widen(int dtype, const void* in, const double* win, int H, int W, cplx* out, long long total, hipStream_t s) {
  zk_with_elem(dtype, [&](auto e) {
    using T = typename decltype(e)::type;
    hipLaunchKernelGGL(widen_kernel<T>, dim3(blocks_of(total)), dim3(256), 0, s, (const T*)in, win, H, W, out, total);
  });
  ZK_HIP(hipGetLastError());
  return 0;
}

// a cached plan bound to a stream for the length of a call; it goes back to the cache on the default stream, as the other
// units expect to find it
struct stream_plan {
  zk_fft_plan p;
  bool bound = false;
  ~stream_plan() {
    if (bound) (void)zk_fft.SetStream(p.h, nullptr);
  }
  int make(int ny, int nx, int batch, hipStream_t s) {
    const int rc = p.make(ny, nx, batch);
    if (rc) return rc;
    bound = true;
    ZK_FFT(zk_fft.SetStream(p.h, s));
    return 0;
  }
};

}  // namespace
