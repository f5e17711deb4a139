// zk_voronoi.hip -- device side of the reference's graph/vnn.py: the Voronoi neighbours of a point set, and the bonds
// vnn_graph keeps of them.  Points (N, 2) go in; directed index pairs (and, for the plain neighbour list, the ridge and edge
// length of each) come out, sorted.  No triangulation is built: every point clips its own cell.
//
//   points       converted to float64 (ZK_F64 as they are, ZK_I32 widened exactly); a NaN or inf raises the error flag.
//                One point alone has no rows (its corner points would coincide with it).
//   frame        one workgroup: centre = (sum x, sum y) / N and v0 = max |p - centre| over both coordinates, each a strided
//                sequential sum / max per lane and a fixed tree over the 1024 lanes (no floating-point atomics).  The four
//                corner points are centre + (-+v, -+v), v = v0 (1 + pad), with the indices N .. N + 3, as add_corner_points
//                appends them.
//   bins         the point grid of zk_point_grid.h over the square centre -+ v0.
//   cells        one lane per point, in bin order.  The cell is a convex polygon in coordinates RELATIVE to the point, each
//                vertex with the index of the neighbour whose bisector made the edge that leaves it.  It starts as a square
//                that contains the cell (below), is clipped by the four corners, then by the points of the bins in rings of
//                growing Chebyshev distance r around the point's own bin; a candidate q clips with x . q <= |q|^2 / 2.  A
//                point cuts off a vertex v exactly when it lies inside the circle around v through the cell's own point (the
//                security radius: within 2 |v|), and every point lies in the grid's rectangle, so the search stops at the
//                first ring where, for every vertex, the part of that circle inside the rectangle lies within the rings
//                already searched: the cell is then exact against all points, and a border cell, whose far vertices lie
//                outside the rectangle, does not search the whole grid.  At the end every vertex is computed again from the
//                two bisectors that meet in it (a 2 x 2 solve in relative coordinates), so its rounding does not depend on
//                the clipping order or on the starting square.
//   rows         the lane walks its polygon: ridge length L = hypot of the edge, edge length L1 = hypot(q).  A ridge of length
//                exactly zero is no neighbour.  Mode ZK_VORONOI_NEIGHBOURS keeps every real neighbour; mode ZK_VORONOI_GRAPH
//                sums L over the entries (corners included) with L1 < dmax and keeps the real ones among them with
//                L / sum >= threshold.
//   output       per-lane counts are scanned, the rows compacted into keys (i << 32) | j (graph mode: both orientations),
//                radix-sorted, and in graph mode deduplicated: the sorted, symmetrised pair list.
//
// The starting square.  Let s = 1 + pad, the points lie in |p - centre| <= v0 per coordinate and the corners at v = s v0.
// A point z of a cell with z_x - centre_x = X > v has |z_y - centre_y| <= v (else the corner on its side is closer than any
// point), so its distance to that corner is at most sqrt((X - v)^2 + v^2), while its own point is at least X - v0 away:
// (X - v0)^2 <= (X - v)^2 + v^2, that is X <= (2 v^2 - v0^2) / (2 (v - v0)) = v (2 s^2 - 1) / (2 pad s), 11.48 v at
// pad = 0.05; the same on every side.  The square has that half-side times 17/16, centred on the centre.  A larger one
// would only cost precision in the clipped vertices that steer the search.
//
// Vertex storage.  A cell may have up to CAP = 32 vertices (a lattice cell has 3 .. 8).  A polygon that would pass the cap
// raises the error flag and nothing is written past it: that is a point with more than 32 Voronoi neighbours, or one with
// nearly as many, because clips come in bin order, not by distance, and the polygon may pass its final size on the way.  The polygon is indexed by run-time values, so in
// registers it would be spilled to scratch (640 B a lane: at 8 waves per SIMD 1.3 MB per CU, far past the 32 KiB L1, so every
// clip would go to L2 and beyond).  It lives in LDS instead: x and y as float64, the index as int32, laid out [vertex][lane],
// so the bank of an access depends on the lane alone and lanes never conflict whatever vertex each one is at.  A workgroup
// is one wave: 64 lanes x 32 vertices x 20 B = 40 KiB, four workgroups (one wave per SIMD) in the 160 KiB of a CU.  The
// kernel is a chain of dependent clips per lane with divergent trip counts; what binds it has not been measured.
//
// Memory.  The count phase stages CAP rows per point: 128 B a point of neighbour indices, and in neighbour mode 512 B more
// of lengths (640 B a point: 58 MB at 90 k points, 43 GB at the 2^26 limit of the interface), freed when it returns.
//
// Only integer atomics (the error flag); the order of every sum is fixed: two runs agree byte for byte.
#include <math.h>

#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "zk_internal.h"
#include "zk_point_grid.h"
#include "zk_scratch.h"

namespace {

typedef unsigned long long u64;

constexpr int CAP = 32;                              // vertices of one cell
constexpr int CELL_LANES = 64;                       // one wave per workgroup of the cell kernel
constexpr double SLACK = 1e-9;                       // relative margin of the search's stopping test, far past any rounding in it

enum { ERR_COINCIDENT = 2, ERR_CAP = 4, ERR_OPEN = 8, ERR_ROUNDING = 16 };

// what the count phase leaves for the fill phase
struct voronoi_state {
  int device = 0, mode = 0;
  int64_t M = 0;
  dev_buf ijs, ridge, edge;                          // int64 (M, 2), float64 (M), float64 (M)
};

// centre, corners, grid and starting square of one call (device memory, written by frame_kernel)
struct frame_info {
  double cx, cy;                                     // centre
  double v0, v;                                      // max |p - centre|, v0 (1 + pad)
  zk_grid_frame grid;                                // the bins, over centre -+ v0
  double half;                                       // half-side of the starting square
};

// one cell's polygon: vertex t at x[t * stride], y[t * stride], id[t * stride]
struct poly_ref {
  double* x;
  double* y;
  int* id;
  int stride;
};

// Clips the polygon of n vertices with x . q <= |q|^2 / 2 in place (Sutherland-Hodgman; the write index never passes
// the vertex read next, which is held in registers).  Returns the new vertex count, -1 when it would pass CAP, -2 when
// nothing is left, -3 when the vertices outside the half-plane are not one run around the polygon: it is then convex only up
// to rounding (three nearly collinear vertices, as nearly coincident points make them), and neither the count nor the
// in-place order would hold.  Every store is guarded by the cap as well.
__device__ inline int clip_cell(poly_ref p, int n, double qx, double qy, int qid) {
  const double hq = 0.5 * (qx * qx + qy * qy);
  const int s = p.stride;
  int outside = 0, runs = 0;
  bool before = p.x[(n - 1) * s] * qx + p.y[(n - 1) * s] * qy - hq > 0;
  for (int k = 0; k < n; ++k) {
    const bool out = p.x[k * s] * qx + p.y[k * s] * qy - hq > 0;
    outside += out ? 1 : 0;
    runs += (out && !before) ? 1 : 0;
    before = out;
  }
  if (outside == 0) return n;
  if (outside == n) return -2;
  if (runs != 1) return -3;
  if (n - outside + 2 > CAP) return -1;
  const double fx = p.x[0], fy = p.y[0];
  const int fid = p.id[0];
  double cx = fx, cy = fy, cd = cx * qx + cy * qy - hq;
  int cid = fid, o = 0;
  for (int k = 0; k < n; ++k) {
    const bool last = k + 1 == n;
    const double nx = last ? fx : p.x[(k + 1) * s], ny = last ? fy : p.y[(k + 1) * s];
    const int nid = last ? fid : p.id[(k + 1) * s];
    const double nd = nx * qx + ny * qy - hq;
    const bool cin = !(cd > 0), nin = !(nd > 0);
    if (cin) {
      if (o >= CAP) return -1;
      p.x[o * s] = cx;
      p.y[o * s] = cy;
      p.id[o * s] = cid;
      ++o;
    }
    if (cin != nin) {
      const double t = cd / (cd - nd);
      const double ix = cx + t * (nx - cx), iy = cy + t * (ny - cy);
      if (o >= CAP) return -1;
      p.x[o * s] = ix;
      p.y[o * s] = iy;
      p.id[o * s] = cin ? qid : cid;                 // leaving the cell: the new edge starts here; entering: the old edge goes on
      ++o;
    }
    cx = nx;
    cy = ny;
    cd = nd;
    cid = nid;
  }
  return o;
}

// the grid's rectangle (every point lies in it) and the box of the bins already searched, relative to the cell's point
struct search_box {
  double gxlo, gxhi, gylo, gyhi, qxlo, qxhi, qylo, qyhi;
};

// Can a point outside the searched box still cut the polygon?  A point q cuts off vertex v exactly when it lies inside the
// circle around v through the cell's own point (|q - v| < |v|), so the search is over when, for every vertex, the part of
// that circle inside the grid's rectangle lies in the box.  The part is bounded by its extent in y over the rectangle's x
// range and its extent in x over the rectangle's y range; radii are taken SLACK larger.
__device__ inline bool can_be_cut(poly_ref p, int nv, const search_box& b) {
  for (int t = 0; t < nv; ++t) {
    const double vx = p.x[t * p.stride], vy = p.y[t * p.stride], r2 = (vx * vx + vy * vy) * (1 + SLACK);
    const double dx = fmax(fmax(b.gxlo - vx, vx - b.gxhi), 0.0), dy = fmax(fmax(b.gylo - vy, vy - b.gyhi), 0.0);
    if (dx * dx + dy * dy >= r2) continue;           // the circle does not reach the rectangle
    const double ry = sqrt(r2 - dx * dx), rx = sqrt(r2 - dy * dy);
    if (fmax(vx - rx, b.gxlo) < b.qxlo || fmin(vx + rx, b.gxhi) > b.qxhi || fmax(vy - ry, b.gylo) < b.qylo ||
        fmin(vy + ry, b.gyhi) > b.qyhi)
      return true;
  }
  return false;
}

// what a cell is built from
struct cell_input {
  const double2* pts;                                // the points in the caller's order
  const double2* spts;                               // the points in bin order
  const int* sidx;                                   // their indices
  const int* bin_start;                              // g * g + 1 entries
  long long n;
};

// position of neighbour `id` relative to (px, py): a point, or corner id - n in the order (-,-) (+,-) (+,+) (-,+)
__device__ inline void relative_of(const cell_input& in, const frame_info& f, int id, double px, double py, double* qx,
                                            double* qy) {
  if (id < in.n) {
    *qx = in.pts[id].x - px;
    *qy = in.pts[id].y - py;
  } else {
    const int c = id - (int)in.n;
    *qx = ((c == 1 || c == 2) ? f.v : -f.v) + f.cx - px;
    *qy = (c >= 2 ? f.v : -f.v) + f.cy - py;
  }
}

// clips with the points of the sorted range [lo, hi); returns the vertex count or a negative code
__device__ inline int clip_range(const cell_input& in, poly_ref p, int nv, int lo, int hi, int self, double px, double py,
                                          int* err) {
  for (int m = lo; m < hi && nv > 0; ++m) {
    const int j = in.sidx[m];
    if (j == self) continue;
    const double qx = in.spts[m].x - px, qy = in.spts[m].y - py;
    if (qx == 0 && qy == 0) {
      *err |= ERR_COINCIDENT;
      continue;
    }
    nv = clip_cell(p, nv, qx, qy, j);
  }
  return nv;
}

// The cell of sorted point k in p; returns its vertex count, or 0 with bits set in *err.
__device__ inline int build_cell(const cell_input& in, const frame_info& f, long long k, poly_ref p, int* err) {
  const zk_grid_frame& gf = f.grid;
  const int s = p.stride, self = in.sidx[k], g = gf.g;
  const double px = in.spts[k].x, py = in.spts[k].y;
  // the starting square, counter-clockwise, no neighbour behind its edges
  const double mx = f.cx - px, my = f.cy - py;
  for (int t = 0; t < 4; ++t) {
    p.x[t * s] = mx + ((t == 1 || t == 2) ? f.half : -f.half);
    p.y[t * s] = my + (t >= 2 ? f.half : -f.half);
    p.id[t * s] = -1;
  }
  int nv = 4;
  for (int c = 0; c < 4 && nv > 0; ++c) {
    double qx, qy;
    relative_of(in, f, (int)in.n + c, px, py, &qx, &qy);
    nv = clip_cell(p, nv, qx, qy, (int)in.n + c);
  }
  const int bx = gf.bin_x(px), by = gf.bin_y(py);
  int reach = bx > g - 1 - bx ? bx : g - 1 - bx;
  reach = by > reach ? by : reach;
  reach = g - 1 - by > reach ? g - 1 - by : reach;
  for (int r = 0; r <= reach && nv > 0; ++r) {
    if (r > 0) {                                     // the points not yet seen lie outside the box of the rings before r
      const double e = SLACK * gf.h * g;
      const search_box b = {gf.x0 - px - e, gf.x0 + gf.h * g - px + e, gf.y0 - py - e, gf.y0 + gf.h * g - py + e,
                            gf.x0 + gf.h * (bx - r + 1) - px + e, gf.x0 + gf.h * (bx + r) - px - e,
                            gf.y0 + gf.h * (by - r + 1) - py + e, gf.y0 + gf.h * (by + r) - py - e};
      if (!can_be_cut(p, nv, b)) break;
    }
    const int xlo = bx - r > 0 ? bx - r : 0, xhi = bx + r < g - 1 ? bx + r : g - 1;
    if (by - r >= 0) nv = clip_range(in, p, nv, in.bin_start[(by - r) * g + xlo], in.bin_start[(by - r) * g + xhi + 1], self, px, py, err);
    if (r > 0 && by + r <= g - 1 && nv > 0)
      nv = clip_range(in, p, nv, in.bin_start[(by + r) * g + xlo], in.bin_start[(by + r) * g + xhi + 1], self, px, py, err);
    const int ylo = by - r + 1 > 0 ? by - r + 1 : 0, yhi = by + r - 1 < g - 1 ? by + r - 1 : g - 1;
    for (int y = ylo; y <= yhi && nv > 0; ++y) {
      if (bx - r >= 0) nv = clip_range(in, p, nv, in.bin_start[y * g + bx - r], in.bin_start[y * g + bx - r + 1], self, px, py, err);
      if (bx + r <= g - 1 && nv > 0)
        nv = clip_range(in, p, nv, in.bin_start[y * g + bx + r], in.bin_start[y * g + bx + r + 1], self, px, py, err);
    }
  }
  if (nv <= 0) {
    *err |= nv == -1 ? ERR_CAP : (nv == -3 ? ERR_ROUNDING : ERR_OPEN);
    return 0;
  }
  if (*err) return 0;
  // every vertex again from the two bisectors that meet in it: the one entering (the edge of the vertex before) and the one leaving
  int prev = p.id[(nv - 1) * s];
  for (int t = 0; t < nv; ++t) {
    const int cur = p.id[t * s];
    if (cur < 0) {
      *err |= ERR_OPEN;                              // an edge of the starting square survived: it did not contain the cell
      return 0;
    }
    double ax, ay, bx2, by2;
    relative_of(in, f, prev, px, py, &ax, &ay);
    relative_of(in, f, cur, px, py, &bx2, &by2);
    const double ha = 0.5 * (ax * ax + ay * ay), hb = 0.5 * (bx2 * bx2 + by2 * by2), det = ax * by2 - ay * bx2;
    if (det != 0) {
      p.x[t * s] = (ha * by2 - hb * ay) / det;
      p.y[t * s] = (ax * hb - bx2 * ha) / det;
    }
    prev = cur;
  }
  return nv;
}

// The rows of a finished cell: for vertex t the neighbour id[t], its ridge length and its edge length.  Returns the number of
// rows kept by `mode` and writes them through put(row, j, L, L1).
template <class Put>
__device__ inline int cell_rows(const cell_input& in, const frame_info& f, long long k, poly_ref p, int nv, int mode, double dmax,
                                         double threshold, Put put) {
  const int s = p.stride;
  const double px = in.spts[k].x, py = in.spts[k].y;
  double sum = 0;
  if (mode == ZK_VORONOI_GRAPH)
    for (int t = 0; t < nv; ++t) {
      const int u = t + 1 == nv ? 0 : t + 1;
      double qx, qy;
      relative_of(in, f, p.id[t * s], px, py, &qx, &qy);
      if (hypot(qx, qy) < dmax) sum += hypot(p.x[u * s] - p.x[t * s], p.y[u * s] - p.y[t * s]);
    }
  int rows = 0;
  for (int t = 0; t < nv; ++t) {
    const int u = t + 1 == nv ? 0 : t + 1, j = p.id[t * s];
    if (j >= in.n) continue;
    double qx, qy;
    relative_of(in, f, j, px, py, &qx, &qy);
    const double len = hypot(p.x[u * s] - p.x[t * s], p.y[u * s] - p.y[t * s]), l1 = hypot(qx, qy);
    if (!(len > 0)) continue;
    if (mode == ZK_VORONOI_GRAPH && !(l1 < dmax && len / sum >= threshold)) continue;
    put(rows, j, len, l1);
    ++rows;
  }
  return rows;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------

// one workgroup: centre, v0, corners' v, grid and starting square
__global__ __launch_bounds__(1024) void frame_kernel(const double2* __restrict__ pts, long long n, double pad, int g,
                                                     frame_info* __restrict__ out, int* __restrict__ flag) {
  __shared__ double sa[1024];
  __shared__ double sb[1024];
  const int t = threadIdx.x;
  double a = 0, b = 0;
  for (long long i = t; i < n; i += 1024) {
    a += pts[i].x;
    b += pts[i].y;
  }
  sa[t] = a;
  sb[t] = b;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d) {
      sa[t] += sa[t + d];
      sb[t] += sb[t + d];
    }
    __syncthreads();
  }
  const double cx = sa[0] / (double)n, cy = sb[0] / (double)n;
  __syncthreads();
  a = 0;
  for (long long i = t; i < n; i += 1024) a = fmax(a, fmax(fabs(pts[i].x - cx), fabs(pts[i].y - cy)));
  sa[t] = a;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d) sa[t] = fmax(sa[t], sa[t + d]);
    __syncthreads();
  }
  if (t == 0) {
    frame_info f;
    const double s = 1 + pad;
    f.cx = cx;
    f.cy = cy;
    f.v0 = sa[0];
    f.v = f.v0 * s;
    f.grid.x0 = cx - f.v0;
    f.grid.y0 = cy - f.v0;
    f.grid.h = f.v0 > 0 ? 2 * f.v0 / (double)g : 1.0;
    f.grid.g = g;
    f.half = f.v * ((2 * s * s - 1) / (2 * pad * s)) * (17.0 / 16.0);
    *out = f;
    // finite points whose sum or whose starting square overflows (coordinates near 1e308) are refused like non-finite ones
    if (!(fabs(cx) + fabs(cy) + f.half <= 1.7976931348623157e308)) atomicOr(flag, ERR_NONFINITE);
  }
}

// One lane per sorted point.  Its rows go to stage_*[row * n + k] (coalesced over the lanes), their number to cnt[k];
// cnt has n + 1 entries, the last 0: its scan ends in the total.
__global__ __launch_bounds__(CELL_LANES) void cell_kernel(cell_input in, const frame_info* __restrict__ fi, int mode, double dmax,
                                                          double threshold, int* __restrict__ cnt, int* __restrict__ stage_j,
                                                          double* __restrict__ stage_l, double* __restrict__ stage_l1,
                                                          int* __restrict__ flag) {
  __shared__ double lx[CAP * CELL_LANES];
  __shared__ double ly[CAP * CELL_LANES];
  __shared__ int lid[CAP * CELL_LANES];
  const long long k = (long long)blockIdx.x * CELL_LANES + threadIdx.x;
  if (k > in.n) return;
  if (k == in.n) {
    cnt[k] = 0;
    return;
  }
  int rows = 0;
  if (!(*flag & ERR_NONFINITE)) {                    // set before this launch; with a NaN no search would ever stop
    const frame_info f = *fi;
    const poly_ref p = {lx + threadIdx.x, ly + threadIdx.x, lid + threadIdx.x, CELL_LANES};
    int err = 0;
    const int nv = build_cell(in, f, k, p, &err);
    if (err) atomicOr(flag, err);
    if (nv > 0) {
      const long long n = in.n;
      rows = cell_rows(in, f, k, p, nv, mode, dmax, threshold, [=](int row, int j, double len, double l1) {
        stage_j[(long long)row * n + k] = j;
        if (stage_l) {
          stage_l[(long long)row * n + k] = len;
          stage_l1[(long long)row * n + k] = l1;
        }
      });
    }
  }
  cnt[k] = rows;
}

// keys[off[k] + row] = (i << 32) | j of every staged row (graph mode: total more keys (j << 32) | i behind them); pos = its place
__global__ __launch_bounds__(256) void compact_kernel(const int* __restrict__ cnt, const int* __restrict__ off, const int* __restrict__ sidx,
                                                      const int* __restrict__ stage_j, long long n, long long total, int mode,
                                                      u64* __restrict__ keys, int* __restrict__ pos) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const u64 i = (u64)sidx[k];
  const long long o = off[k];
  for (int row = 0; row < cnt[k]; ++row) {
    const u64 j = (u64)stage_j[(long long)row * n + k];
    keys[o + row] = (i << 32) | j;
    if (mode == ZK_VORONOI_GRAPH) keys[total + o + row] = (j << 32) | i;
    else pos[o + row] = (int)((long long)row * n + k);
  }
}

__global__ __launch_bounds__(256) void unpack_kernel(const u64* __restrict__ keys, const int* __restrict__ pos, const double* __restrict__ stage_l,
                                                     const double* __restrict__ stage_l1, long long m, long long* __restrict__ ijs,
                                                     double* __restrict__ ridge, double* __restrict__ edge) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  ijs[2 * e] = (long long)(keys[e] >> 32);
  ijs[2 * e + 1] = (long long)(keys[e] & 0xffffffffull);
  if (pos) {
    ridge[e] = stage_l[pos[e]];
    edge[e] = stage_l1[pos[e]];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the launch sequence
// ---------------------------------------------------------------------------------------------------------------------

int fail_flags(int flags) {
  if (flags & ERR_NONFINITE)
    return zk_fail(ZK_E_BADARG, "voronoi_cells: a point is not finite (or the coordinates are so large that their sum or the corner points overflow)");
  if (flags & ERR_COINCIDENT) return zk_fail(ZK_E_BADARG, "voronoi_cells: two points coincide");
  if (flags & ERR_CAP)
    return zk_fail(ZK_E_BADARG, "voronoi_cells: a cell needs more than 32 vertices: a point with more than 32 Voronoi neighbours, or with nearly "
                                "as many (cells are clipped in bin order and may pass their final size on the way)");
  if (flags & ERR_ROUNDING)
    return zk_fail(ZK_E_BADARG, "voronoi_cells: a cell is convex only up to rounding (nearly coincident points?)");
  return zk_fail(ZK_E_BADARG, "voronoi_cells: a cell was not closed by the corner points (is pad too small for float64?)");
}

int voronoi_count(voronoi_state* st, const void* points, int dtype, int64_t n, double pad, int mode, double dmax, double threshold,
                  hipStream_t s) {
  if (n == 0) return 0;
  int rc;
  temp_store tmp;
  const int g = grid_side(n);
  const bool lengths = mode == ZK_VORONOI_NEIGHBOURS;

  point_grid grid;
  dev_buf d_pts, d_small, d_frame, d_cnt, d_off, d_sj, d_sl, d_sl1;
  if ((rc = d_pts.alloc(sizeof(double2) * (size_t)n)) || (rc = d_small.alloc(64)) || (rc = d_frame.alloc(sizeof(frame_info))) ||
      (rc = d_cnt.alloc(sizeof(int) * (size_t)(n + 1))) || (rc = d_off.alloc(sizeof(int) * (size_t)(n + 1))) ||
      (rc = d_sj.alloc(sizeof(int) * CAP * (size_t)n)) || (lengths && ((rc = d_sl.alloc(sizeof(double) * CAP * (size_t)n)) ||
                                                                      (rc = d_sl1.alloc(sizeof(double) * CAP * (size_t)n)))))
    return rc;
  int* d_flag = d_small.as<int>();                   // [0] error flags, [1] unique keys (graph mode)
  ZK_HIP(hipMemsetAsync(d_small.p, 0, 64, s));
  hipLaunchKernelGGL(load_points_kernel, dim3(blocks_of(n)), dim3(256), 0, s, points, dtype, (long long)n, d_pts.as<double2>(), d_flag);
  if (n == 1) {                                      // the four corner points coincide with the point: no diagram, no rows
    int flags = 0;
    ZK_HIP(hipMemcpyAsync(&flags, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return flags ? fail_flags(flags) : 0;
  }
  hipLaunchKernelGGL(frame_kernel, dim3(1), dim3(1024), 0, s, d_pts.as<double2>(), (long long)n, pad, g, d_frame.as<frame_info>(), d_flag);
  if ((rc = build_point_grid(&grid, tmp, d_pts.as<double2>(), n, g, &d_frame.as<frame_info>()->grid, s))) return rc;
  const cell_input in = {d_pts.as<double2>(), grid.spts, grid.sidx, grid.bin_start, (long long)n};
  hipLaunchKernelGGL(cell_kernel, dim3((unsigned)((n + 1 + CELL_LANES - 1) / CELL_LANES)), dim3(CELL_LANES), 0, s, in,
                     d_frame.as<frame_info>(), mode, dmax, threshold, d_cnt.as<int>(), d_sj.as<int>(), d_sl.as<double>(), d_sl1.as<double>(),
                     d_flag);
  ZK_HIP(hipGetLastError());
  if ((rc = exclusive_sum<int>(tmp, d_cnt.as<int>(), d_off.as<int>(), (size_t)(n + 1), s))) return rc;

  // the error flags and the number of rows cross to the host: the rows size the sort
  int flags = 0, total = 0;
  ZK_HIP(hipMemcpyAsync(&flags, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipMemcpyAsync(&total, d_off.as<int>() + n, sizeof(int), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  if (flags) return fail_flags(flags);
  if (total == 0) return 0;

  const long long keys_n = lengths ? total : 2 * (long long)total;
  dev_buf d_rk, d_rp;
  if ((rc = d_rk.alloc(sizeof(u64) * 2 * (size_t)keys_n)) || (lengths && (rc = d_rp.alloc(sizeof(int) * 2 * (size_t)keys_n)))) return rc;
  u64 *r_in = d_rk.as<u64>(), *r_out = r_in + keys_n;
  int *p_in = d_rp.as<int>(), *p_out = lengths ? p_in + keys_n : nullptr;   // row positions: neighbour mode only
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(n)), dim3(256), 0, s, d_cnt.as<int>(), d_off.as<int>(), grid.sidx, d_sj.as<int>(),
                     (long long)n, (long long)total, mode, r_in, p_in);
  ZK_HIP(hipGetLastError());
  long long m = keys_n;
  const u64* sorted = r_out;
  if (lengths) {
    if ((rc = zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::radix_sort_pairs(p, b, r_in, r_out, p_in, p_out, (size_t)keys_n, 0, 64, s); })))
      return rc;
  } else {
    if ((rc = zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::radix_sort_keys(p, b, r_in, r_out, (size_t)keys_n, 0, 64, s); })) ||
        (rc = zk_prim(tmp, [&](void* p, size_t& b) {
           return rocprim::unique(p, b, r_out, r_in, (unsigned int*)(d_flag + 1), (size_t)keys_n, rocprim::equal_to<u64>(), s);
         })))
      return rc;
    int unique_n = 0;
    ZK_HIP(hipMemcpyAsync(&unique_n, d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    if (unique_n < 0 || unique_n > keys_n) return zk_fail(ZK_E_BADARG, "voronoi_cells: bad unique pair count");
    m = unique_n;
    sorted = r_in;
  }
  if ((rc = st->ijs.alloc(sizeof(long long) * 2 * (size_t)m)) ||
      (lengths && ((rc = st->ridge.alloc(sizeof(double) * (size_t)m)) || (rc = st->edge.alloc(sizeof(double) * (size_t)m)))))
    return rc;
  hipLaunchKernelGGL(unpack_kernel, dim3(blocks_of(m)), dim3(256), 0, s, sorted, lengths ? p_out : (const int*)nullptr, d_sl.as<double>(),
                     d_sl1.as<double>(), m, st->ijs.as<long long>(), st->ridge.as<double>(), st->edge.as<double>());
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));                   // the working buffers go with this call
  st->M = m;
  return 0;
}

// copies what the count phase left to the caller's arrays (device or host memory, by `kind`)
int voronoi_fill(const voronoi_state* st, int64_t* ijs, double* ridge, double* edge, hipMemcpyKind kind, hipStream_t s) {
  if (ijs && st->M) ZK_HIP(hipMemcpyAsync(ijs, st->ijs.p, sizeof(int64_t) * 2 * (size_t)st->M, kind, s));
  if (ridge && st->M && st->ridge.p) ZK_HIP(hipMemcpyAsync(ridge, st->ridge.p, sizeof(double) * (size_t)st->M, kind, s));
  if (edge && st->M && st->edge.p) ZK_HIP(hipMemcpyAsync(edge, st->edge.p, sizeof(double) * (size_t)st->M, kind, s));
  ZK_HIP(hipStreamSynchronize(s));                   // the state is freed next
  return 0;
}

int check_voronoi(const void* points, int dtype, int64_t n, double pad, int mode, double dmax, double threshold, void** state,
                  const int64_t* counts) {
  if (!state) return zk_fail(ZK_E_BADARG, "voronoi_cells: null state pointer");
  if (*state) return 0;                              // fill phase: the inputs are not read again
  if (!counts) return zk_fail(ZK_E_BADARG, "voronoi_cells: the count phase needs counts_host");
  if (n < 0 || n + 4 >= ((int64_t)1 << 31) / CAP) return zk_fail(ZK_E_BADARG, "voronoi_cells: needs 0 <= n_points < 2^26 - 4");
  if (n && !points) return zk_fail(ZK_E_BADARG, "voronoi_cells: null pointer");
  if (dtype != ZK_F64 && dtype != ZK_I32) return zk_fail(ZK_E_BADARG, "voronoi_cells: points are ZK_F64 or ZK_I32");
  if (!(pad > 0) || !(pad <= 1.7976931348623157e308)) return zk_fail(ZK_E_BADARG, "voronoi_cells: pad must be positive and finite");
  if (mode != ZK_VORONOI_NEIGHBOURS && mode != ZK_VORONOI_GRAPH) return zk_fail(ZK_E_BADARG, "voronoi_cells: unknown mode");
  if (mode == ZK_VORONOI_GRAPH && (!(dmax > 0) || !(threshold > 0)))
    return zk_fail(ZK_E_BADARG, "voronoi_cells: the graph needs dmax > 0 and threshold > 0");
  return 0;
}

// both phases on resident points; `kind` says where the fill phase's arrays live
int voronoi_call(int device, const void* points, int dtype, int64_t n, double pad, int mode, double dmax, double threshold, void** state,
                 int64_t* counts, int64_t* ijs, double* ridge, double* edge, hipMemcpyKind kind, hipStream_t s) {
  if (!*state) {
    voronoi_state* st = new (std::nothrow) voronoi_state;
    if (!st) return zk_fail(ZK_E_BADARG, "voronoi_cells: out of host memory");
    st->device = device;
    st->mode = mode;
    const int rc = voronoi_count(st, points, dtype, n, pad, mode, dmax, threshold, s);
    if (rc) {
      delete st;
      return rc;
    }
    counts[0] = st->M;
    *state = st;
    return 0;
  }
  voronoi_state* st = (voronoi_state*)*state;
  const int rc = voronoi_fill(st, ijs, ridge, edge, kind, s);
  delete st;
  *state = nullptr;
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_voronoi_cells_dev(int device, const void* points_dev, int points_dtype, int64_t n_points, double pad, int mode, double dmax,
                                    double threshold, void** state, int64_t* counts_host, int64_t* ijs_dev, double* ridge_dev,
                                    double* edge_dev, void* hip_stream) {
  int rc = check_voronoi(points_dev, points_dtype, n_points, pad, mode, dmax, threshold, state, counts_host);
  if (rc) return rc;
  ZK_ON_DEVICE(*state ? ((voronoi_state*)*state)->device : device);
  return voronoi_call(device, points_dev, points_dtype, n_points, pad, mode, dmax, threshold, state, counts_host, ijs_dev, ridge_dev, edge_dev,
                      hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
}

extern "C" int zk_voronoi_cells(int device, const void* points_host, int points_dtype, int64_t n_points, double pad, int mode, double dmax,
                                double threshold, void** state, int64_t* counts_host, int64_t* ijs_host, double* ridge_host,
                                double* edge_host) {
  int rc = check_voronoi(points_host, points_dtype, n_points, pad, mode, dmax, threshold, state, counts_host);
  if (rc) return rc;
  if (!*state && points_dtype == ZK_F64)             // the values are checked before anything is launched
    for (int64_t k = 0; k < 2 * n_points; ++k)
      if (!(fabs(((const double*)points_host)[k]) <= 1.7976931348623157e308)) return zk_fail(ZK_E_BADARG, "voronoi_cells: a point is not finite");
  ZK_ON_DEVICE(*state ? ((voronoi_state*)*state)->device : device);
  const size_t pts_bytes = (points_dtype == ZK_I32 ? sizeof(int32_t) : sizeof(double)) * 2 * (size_t)n_points;
  dev_buf d_pts;
  if (!*state && n_points && (rc = d_pts.upload(points_host, pts_bytes))) return rc;
  return voronoi_call(device, d_pts.p, points_dtype, n_points, pad, mode, dmax, threshold, state, counts_host, ijs_host, ridge_host, edge_host,
                      hipMemcpyDeviceToHost, (hipStream_t)0);
}
