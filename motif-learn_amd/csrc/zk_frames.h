// zk_frames.h -- what zk_register.hip shares with zk_strain.hip (not part of the public ABI): a stack of real frames widened
// and windowed into a complex float64 field, a cached hipFFT plan bound to a stream for the length of a call, and the staging
// state of a unit's host-buffer entry points.
#pragma once

#include <math.h>

#include <mutex>

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
  const dim3 grid(blocks_of(total)), block(256);
  switch (dtype) {
    case ZK_F32: hipLaunchKernelGGL(widen_kernel<float>, grid, block, 0, s, (const float*)in, win, H, W, out, total); break;
    case ZK_F64: hipLaunchKernelGGL(widen_kernel<double>, grid, block, 0, s, (const double*)in, win, H, W, out, total); break;
    case ZK_U8: hipLaunchKernelGGL(widen_kernel<uint8_t>, grid, block, 0, s, (const uint8_t*)in, win, H, W, out, total); break;
    case ZK_U16: hipLaunchKernelGGL(widen_kernel<uint16_t>, grid, block, 0, s, (const uint16_t*)in, win, H, W, out, total); break;
    default: hipLaunchKernelGGL(widen_kernel<int16_t>, grid, block, 0, s, (const int16_t*)in, win, H, W, out, total); break;
  }
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

bool known_dtype(int d) { return d >= ZK_F32 && d <= ZK_I16; }

int check_device(int device) {
  const int ndev = zk_device_count();
  if (ndev < 0) return ndev;
  if (ndev == 0) return zk_fail(ZK_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev || device >= 64) return zk_fail(ZK_E_BADARG, "device index out of range");
  return 0;
}

// the staging of a unit's host entry points: one ring and one stream per device, made at the first call and kept
struct host_state {
  std::mutex lock;
  bool made = false;
  zk_ring ring;
  hipStream_t stream = nullptr;
};

int host_state_make(host_state* h) {
  if (h->made) return 0;
  ZK_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const int rc = zk_ring_create(&h->ring);
  if (rc) {
    zk_ring_destroy(&h->ring);
    (void)hipStreamDestroy(h->stream);
    h->stream = nullptr;
    return rc;
  }
  h->made = true;
  return 0;
}

}  // namespace
