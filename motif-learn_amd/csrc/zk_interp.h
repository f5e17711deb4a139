// zk_interp.h -- the interpolation primitives of zk_resample.hip, kept apart so that another kernel can sample an image at
// real coordinates the way scipy.ndimage.map_coordinates does: the boundary rules as index folds on the extended signal, the
// B-spline tap weights of orders 0, 1 and 3, and one segment of the cubic prefilter.  Everything is float64 and usable from
// host code as well (a CPU build of these functions is how they were compared with SciPy before any kernel ran).
#pragma once

#include <math.h>

#include "zk_internal.h"

#define ZK_HD static __host__ __device__ __forceinline__

// the modes of zk_scan_resample (include/zernike_hip.h: ZK_RESAMPLE_*)
enum zk_extend { ZK_EXT_REFLECT = 0, ZK_EXT_MIRROR = 1, ZK_EXT_NEAREST = 2, ZK_EXT_GRID_WRAP = 3, ZK_EXT_GRID_CONSTANT = 4, ZK_EXT_CONSTANT = 5 };

#define ZK_SPLINE_POLE (-0.26794919243112270647)  // sqrt(3) - 2
#define ZK_SPLINE_GAIN 6.0                        // (1 - pole) (1 - 1 / pole)
#define ZK_SPLINE_WARMUP 32                       // |pole|^32 = 5e-19: below one float64 ulp of the sum it truncates

// Index i of the signal extended by `mode` -> index into its n samples, or -1 where the extension is the constant 0
// (ZK_EXT_GRID_CONSTANT).  The modulo form: right for an index any number of periods away.  ZK_EXT_CONSTANT clamps -- its
// samples outside [0, n - 1] are refused as a whole by the caller, and the taps of one inside that leave it have weight 0.
ZK_HD long long zk_fold_index(long long i, long long n, int mode) {
  if ((unsigned long long)i < (unsigned long long)n) return i;
  switch (mode) {
    case ZK_EXT_REFLECT: {  // d c b a | a b c d | d c b a: period 2 n
      const long long p = 2 * n;
      long long m = i % p;
      if (m < 0) m += p;
      return m < n ? m : p - 1 - m;
    }
    case ZK_EXT_MIRROR: {  // d c b | a b c d | c b a: period 2 n - 2
      if (n == 1) return 0;
      const long long p = 2 * n - 2;
      long long m = i % p;
      if (m < 0) m += p;
      return m < n ? m : p - m;
    }
    case ZK_EXT_GRID_WRAP: {
      const long long m = i % n;
      return m < 0 ? m + n : m;
    }
    case ZK_EXT_GRID_CONSTANT: return -1;
    default: return i < 0 ? 0 : n - 1;  // ZK_EXT_NEAREST, ZK_EXT_CONSTANT
  }
}

// Coordinate c of a line of n samples -> the equivalent coordinate map_coordinates evaluates at (ni_interpolation.c,
// map_coordinate): inside the line it is c itself, outside it is brought back by whole periods of the mode's extension (to
// within one sample of the line; the taps are folded afterwards).  Mathematically the interpolant of the extended signal has
// the same value at both; the weights are formed from the mapped coordinate because its rounding (2e-14 where a small negative
// coordinate is wrapped to n - |c|) is part of the reference's result.  ZK_EXT_GRID_CONSTANT and ZK_EXT_CONSTANT keep c.  |c| is
// clamped to 1e12 first, so that every quotient and tap index below is representable whatever the shift.
ZK_HD double zk_map_coordinate(double c, long long n, int mode) {
  c = fmin(fmax(c, -1e12), 1e12);
  const double len = (double)n;
  if (!(c < 0.0) && !(c > len - 1.0)) return c;
  if (mode == ZK_EXT_GRID_CONSTANT || mode == ZK_EXT_CONSTANT) return c;
  if (mode == ZK_EXT_NEAREST) return c < 0.0 ? 0.0 : len - 1.0;
  if (n <= 1) return 0.0;
  if (mode == ZK_EXT_MIRROR) {
    const double p = (double)(2 * n - 2);
    if (c < 0.0) {
      c = p * (double)(long long)(-c / p) + c;
      return c <= 1.0 - len ? c + p : -c;
    }
    c -= p * (double)(long long)(c / p);
    return c >= len ? p - c : c;
  }
  if (mode == ZK_EXT_REFLECT) {
    const double p = (double)(2 * n);
    if (c < 0.0) {
      if (c < -p) c = p * (double)(long long)(-c / p) + c;
      return c < -len ? c + p : (c > -1e-15 ? 1e-15 : -c) - 1.0;
    }
    c -= p * (double)(long long)(c / p);
    return c >= len ? p - c - 1.0 : c;
  }
  // ZK_EXT_GRID_WRAP
  if (c < 0.0) return c + len * (double)((long long)((-1.0 - c) / len) + 1);
  c -= len * (double)(long long)((c + 1.0) / len);
  return c < 0.0 ? c + len : c;
}

// First tap and the order + 1 weights of the B-spline of `order` (0, 1 or 3) at the mapped coordinate c: SciPy's expressions
// (ni_splines.c), the last weight being one minus the others.  The taps are then folded by zk_fold_index, which keeps every
// address inside the line.
ZK_HD long long zk_spline_taps(double c, int order, double* w) {
  if (order == 0) {
    w[0] = 1.0;
    return (long long)floor(c + 0.5);
  }
  const double fl = floor(c), y = c - fl, z = 1.0 - y;
  if (order == 1) {
    w[0] = 1.0 - y;
    w[1] = 1.0 - w[0];
    return (long long)fl;
  }
  w[0] = z * z * z / 6.0;
  w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[3] = ((1.0 - w[0]) - w[1]) - w[2];
  return (long long)fl - 1;
}

// Cubic B-spline coefficients of samples [a, b) of one line of the extended signal.  raw(i) is ZK_SPLINE_GAIN times the sample
// at ANY index i of the extension (the caller folds); put(i, v) / get(i) store and re-read inside [a, b).
//   causal      c+[i] = raw(i) + pole c+[i - 1], started ZK_SPLINE_WARMUP samples before a
//   anticausal  c[b - 1] = pole / (pole^2 - 1) (c+[b - 1] + sum_{j >= 1} pole^j raw(b - 1 + j)),  c[i] = pole (c[i + 1] - c+[i])
// which is the exact two-sided filter of the infinite extension up to the truncated tails, whatever the boundary rule and
// however short the line: a segment's numbers do not depend on where its neighbours were cut.
template <class Raw, class Put, class Get>
ZK_HD void zk_spline3_segment(long long a, long long b, Raw raw, Put put, Get get) {
  const double zp = ZK_SPLINE_POLE;
  double cp = 0.0;
  for (long long i = a - ZK_SPLINE_WARMUP; i < a; ++i) cp = raw(i) + zp * cp;
  for (long long i = a; i < b; ++i) {
    cp = raw(i) + zp * cp;
    put(i, cp);
  }
  double t = 0.0;
  for (int j = ZK_SPLINE_WARMUP; j >= 1; --j) t = zp * (t + raw(b - 1 + j));
  double cm = (zp / (zp * zp - 1.0)) * (cp + t);
  put(b - 1, cm);
  for (long long i = b - 2; i >= a; --i) {
    cm = zp * (cm - get(i));
    put(i, cm);
  }
}
