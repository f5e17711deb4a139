// zk_point_window.h -- what the kernels that work on one window (or box) of a frame per key point share: refine_points
// (zk_refine.hip), com_refine (zk_com_refine.hip) and the Gaussian fits (zk_gauss_fit.hip).  The single owner of:
//
//   corner       window_at: from the rows of `pts` to the corner (x0, y0) of point n's size x size window, the point itself as two
//                doubles (com_refine adds it back to the centroid) and whether the window lies inside the frame.  The rows are
//                  CORNERS   int32 window corners, taken as they are;
//                  ZK_I32    int32 points: the corner is x - size / 2 in integers, no limit on x;
//                  ZK_F64    float64 points: r = rint(x) (ties to even), |r| < POINT_LIMIT (false for a NaN), (long long)r - size / 2.
//                com_refine used to send ZK_I32 points through the float64 route and so refused coordinates of 2^30 and above
//                even where the window lay inside a frame that wide; it takes the integer route of the fits now.  A frame narrower
//                than 2^30 sees no difference: such a point's window leaves it on either route.
//   flag         ERR_WINDOW, the bit a kernel raises for a window that leaves the frame, and window_fail, the refusal it becomes.
//   host checks  check_frame (float frame, 0 < H, W < 2^31, n < 2^24), check_pointers and corners_inside, the host's form of the
//                inside test, which the host-array entry points apply before anything is launched.
//   staging      none of its own: a host-array entry point takes its frame and int32 rows up with dev_buf::upload, allocates
//                its results and brings them down with dev_buf::download (zk_scratch.h: pageable memory, no ring -- these calls
//                are not the hot path).  A null result pointer is an output the caller does not want.
//
// This header is compiled under each includer's flags: zk_refine.o and zk_com_refine.o are built with -ffp-contract=off,
// zk_gauss_fit.o is not.  The device code here is rint, fabs, compares, conversions and integer arithmetic only: nothing of the
// shape a * b + c that contraction could fuse.  Keep it so; com_refine's (centroid - size / 2.0) + point stays in its own file.
// Everything has internal linkage: each object keeps its own copy.
#pragma once

#include <math.h>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int CORNERS = -1;                          // pts_dtype: the rows are int32 window corners
constexpr double POINT_LIMIT = 1073741824.0;         // |rint(point)| below 2^30: the corner is an int
enum { ERR_WINDOW = 1 };

struct point_window {
  long long x0, y0;                                  // the corner
  double px, py;                                     // the point (0 for CORNERS)
  bool inside;
};

__device__ inline point_window window_at(const void* __restrict__ pts, int pts_dtype, long long n, int size, long long H, long long W) {
  point_window w = {0, 0, 0.0, 0.0, true};
  if (pts_dtype == CORNERS || pts_dtype == ZK_I32) {
    const int x = ((const int*)pts)[2 * n], y = ((const int*)pts)[2 * n + 1];
    w.x0 = x;
    w.y0 = y;
    if (pts_dtype == ZK_I32) {
      w.px = (double)x;
      w.py = (double)y;
      w.x0 -= size / 2;
      w.y0 -= size / 2;
    }
  } else {
    w.px = ((const double*)pts)[2 * n];
    w.py = ((const double*)pts)[2 * n + 1];
    const double rx = rint(w.px), ry = rint(w.py);
    w.inside = fabs(rx) < POINT_LIMIT && fabs(ry) < POINT_LIMIT;             // false for a NaN
    w.x0 = w.inside ? (long long)rx - size / 2 : 0;
    w.y0 = w.inside ? (long long)ry - size / 2 : 0;
  }
  w.inside = w.inside && w.x0 >= 0 && w.y0 >= 0 && w.x0 + size <= W && w.y0 + size <= H;
  return w;
}

const char* const WINDOW_MESSAGE = ": a window leaves the frame (every corner needs 0 <= x0 <= W - size, 0 <= y0 <= H - size)";

inline int window_fail(const char* who) { return zk_fail(ZK_E_BADARG, std::string(who) + WINDOW_MESSAGE); }

inline bool corners_inside(const int32_t* corners, int64_t n, int64_t size, int64_t H, int64_t W) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t x0 = corners[2 * i], y0 = corners[2 * i + 1];
    if (x0 < 0 || y0 < 0 || x0 + size > W || y0 + size > H) return false;
  }
  return true;
}

// the refusals every entry point opens with; what it checks of its own follows, and check_pointers comes last
inline int check_frame(const char* who, const void* img, int dtype, int64_t H, int64_t W, int64_t n) {
  const std::string name(who);
  if (dtype != ZK_F32 && dtype != ZK_F64) return zk_fail(ZK_E_BADARG, name + ": the frame must be ZK_F32 or ZK_F64 (a float frame)");
  if (H <= 0 || W <= 0 || H > ((int64_t)1 << 31) - 1 || W > ((int64_t)1 << 31) - 1 || !img)
    return zk_fail(ZK_E_BADARG, name + ": needs a frame with 0 < H, W < 2^31");
  if (n < 0 || n >= ((int64_t)1 << 24)) return zk_fail(ZK_E_BADARG, name + ": needs 0 <= n_points < 2^24");
  return 0;
}

inline int check_pointers(const char* who, int64_t n, bool all_given) {
  return n && !all_given ? zk_fail(ZK_E_BADARG, std::string(who) + ": null pointer") : 0;
}

}  // namespace
