// zk_pickers.h -- what zk_pickers.hip shares with zk_window_size.hip (not part of the public ABI): hipFFT bound at run time,
// the cache of batched 2-D plans, and the device-pointer forms of the two picker stages the window-size estimators reuse.
#pragma once

#include <hipfft/hipfft.h>  // types and prototypes only; nothing here links against libhipfft

#include "zk_internal.h"

struct zk_fft_api {
  void* handle = nullptr;
  decltype(&hipfftPlanMany) PlanMany = nullptr;
  decltype(&hipfftExecZ2Z) ExecZ2Z = nullptr;
  decltype(&hipfftSetStream) SetStream = nullptr;
  decltype(&hipfftDestroy) Destroy = nullptr;
};
extern zk_fft_api zk_fft;  // filled by zk_fft_load()
int zk_fft_load();         // 0, or ZK_E_FFT when libhipfft cannot be loaded

#define ZK_FFT(call)                                                                         \
  do {                                                                                       \
    const hipfftResult zk_f_ = (call);                                                       \
    if (zk_f_ != HIPFFT_SUCCESS) return zk_fail(ZK_E_FFT, std::string(#call) + " failed with hipfftResult " + std::to_string((int)zk_f_)); \
  } while (0)

// A batched (ny, nx) complex float64 plan checked out of the cache (zk_pickers.hip); it goes back when its holder dies.
struct zk_fft_cached {
  int device, ny, nx, batch;
  hipfftHandle h;
};
struct zk_fft_plan {
  hipfftHandle h = 0;
  bool live = false;
  zk_fft_cached key = {};
  ~zk_fft_plan();
  int make(int ny, int nx, int batch);
};

typedef hipfftDoubleComplex cplx;

// scipy.signal.correlate(p, p, 'same', 'fft') of n windows (wh x ww, origins (y, x) on the device) of a device image of row
// length W, each standardised with stats[2 b], stats[2 b + 1] (mean, std; null: as it is).  per_window 0: out (wh, ww) +=
// the mean of the maps (the caller zeroes it); 1: out (n, wh, ww) = the maps.  Zero lag at [wh / 2, ww / 2].
int zk_autocorr_same_dev(const void* d_img, int dtype, int64_t W, const int32_t* d_org, int n_windows, int wh, int ww,
                         const double* d_stats, double* d_out, int per_window);
// mean and population standard deviation of n windows -> stats (n, 2) on the device
int zk_window_stats_dev(const void* d_img, int dtype, int64_t W, const int32_t* d_org, int n_windows, int wh, int ww, double* d_stats);
// the polar profile of zk_polar_profile on device operands: centres (B, 2) int32 (row, col) per map, mm (B, 2) the maps'
// min / max, out (B, R).  cut 1: map b keeps radii below min(centre row, R), the rest of its row is 0.
int zk_polar_profile_dev(const double* d_data, int B, int h, int w, const int32_t* d_centres, int cut, int method,
                         const double* d_mm, double* d_out);
