// zk_align.hip -- rotation alignment of Zernike-moment rows to templates, and the per-row rotation that goes with it (no
// reference counterpart: the reference has only the scalar-angle zmoments.rotate and never searches the angle).
//
//   rows      (N, P)  float64, row-major real moments with labels (n, m); the label set is PAIRED: every (n, m > 0) comes with
//                     (n, -m).  Pair k = (n, |m|) has the complex value z_k = x_{n,+m} + i x_{n,-m} (zmoments.to_complex).
//   templates (T, P)  float64 in the same real form, T <= 64; select (P) keeps or drops whole pairs (s_k = 0 / 1).
//
//   c_m      = sum over the pairs with |m_k| = m of  s_k z_k conj(t_k)
//   f(theta) = sum_m Re(c_m exp(-i m theta)) = c_0 + sum_{m >= 1} (Re c_m cos(m theta) + Im c_m sin(m theta))
//            = <rotate(z, theta), t> over the selected real moments; |rotate(z, theta) - t|^2 = |z|^2 + |t|^2 - 2 f(theta).
//
// zk_align_kernel<NM, TB>: one row per lane.  TB templates share a pass: their c_m (2 NM TB float64 VGPRs) are built from one
// read of the row (pairs sorted by m, so every register index is static; pair indices and template values are wave-uniform),
// then ONE pass over the (n_theta, 2 NM) cos / sin table -- wave-uniform as well -- serves the TB grid scans (first maximum,
// NumPy's argmax rule).  Refinement: `newton` steps on f' from the grid maximum theta_0, a step only where f'' < 0, every
// iterate clamped to theta_0 +- one grid step; the result is wrapped into [0, period) and f is evaluated there once more, and
// it is kept only if that value is >= the grid maximum (else theta_0 with the grid value): score >= max over the grid always.
// cos / sin(m theta) off the grid come from one sincos and the angle-addition recurrence (error ~ m ulp, inside the rounding
// of the sum).  best: first argmin_t fma(-2, score, |t|^2) or first argmax_t score * (1 / |t|), the T values given by the host.
// NM is the kernel's largest m (the selected set's largest |m| rounded up to an instance; the table is zero-padded), TB = 4
// up to NM 12, 2 up to 24, 1 at 40.  No atomics; a row's results do not depend on the launch geometry or on the chunking.
//
// zk_rotate_rows_kernel: (a, b) -> (a cos m theta + b sin m theta, b cos m theta - a sin m theta) per pair with the row's own
// angle, one sincos per (row, m); m = 0 columns are copied.  A lane reads a pair before it writes it: in place is allowed.
//
// The rows are read per lane at stride P (as zk_maps_rows_kernel does: the strided accesses are served by the caches; the
// arithmetic per element read is 2 n_theta FMAs and more).
//
// zk_align_planes_kernel<NM, TB>: the same search for the plane layout of the dense path, one pixel per lane.
//   planes    (P, .)  float64, moment j of pixel i at planes[j * plane_stride + i]: the 64 lanes of a wave read one contiguous
//                     512-byte run per moment plane.  All offsets are 64-bit.
//   outputs           plane-major, so that the stores coalesce: angle, score (T, .) with out_plane_stride between templates,
//                     best (.) int32 and norm2 (.) = sum_j s_j x_j^2 over the selected real moments -- one fma chain in
//                     ascending column order -- which turns score into a distance (norm2 + |t|^2 - 2 score) or a cosine
//                     (score / sqrt(norm2 |t|^2)).  Any output may be NULL.
// Both kernels instantiate ONE body (align_body) on an operand accessor: the c_m build in pair order, the table pass, the Newton
// steps, the wrap, the re-evaluation and the best rule are the same operations in the same order, so a pixel gets the bits its
// row would get.  Same NM / TB instances, same limits, same register budget (2 NM TB float64 accumulators, no scratch).
//
// zk_frame_align(_dev): frame -> maps.  The plan's dense transform (whatever zk_transform_frame_dev resolves) writes a band of
// rows into the plan's scratch matrix (P, band, W), the planes kernel turns the band into its part of the maps, band after
// band on one stream: the (P, H, W) moments never exist.  A band holds at most 1 GiB of moments (zk_align_set_band_bytes: less),
// at least one row, whole multiples of 8 rows where it can (a block of the dense kernels).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <optional>

#include "zk_ring.h"

// Nothing in this unit is contracted by the compiler: every fused multiply-add is written as __builtin_fma, every other
// operation rounds on its own, so the rows and the planes kernel (one body, two operand layouts) give one pixel the same bits.
#pragma clang fp contract(off)

#define ZK_ALIGN_MAX_M 40
#define ZK_ALIGN_MAX_T 64
#define ZK_ALIGN_MAX_THETA 4096
#define ZK_ALIGN_MAX_NEWTON 16
#define ZK_ALIGN_TABLES 8   // device trig tables kept per device, one per distinct (kernel NM, n_theta, symmetry, values)
#define ZK_ALIGN_SLOTS 4    // per-call operand blobs in flight per device (pair lists, templates, key values)
#define ZK_ALIGN_STARTS (ZK_ALIGN_MAX_M + 4)  // int32 words of the m-bucket offsets in a blob (8-byte multiple)

namespace {

constexpr double D2R_HI = 0x1.1df46a2529d39p-6, D2R_LO = 0x1.5c1d8becdd291p-62;  // pi / 180 = HI + LO
constexpr double R2D = 57.29577951308232;

// theta in degrees -> radians, one rounding of the exact product
__device__ __forceinline__ double to_radians(double deg) { return __builtin_fma(deg, D2R_HI, deg * D2R_LO); }

// f, f', f'' (per radian) at `deg` from the c_m of one template; DERIV false: f only
template <int NM, bool DERIV>
__device__ __forceinline__ void align_eval(const double c0, const double (&cr)[NM], const double (&ci)[NM], double deg, double& f,
                                           double& f1, double& f2) {
  double s1, c1;
  sincos(to_radians(deg), &s1, &c1);
  double cm = c1, sm = s1, fa = c0, fb = 0.0, g = 0.0, h = 0.0;
#pragma unroll
  for (int m = 1; m <= NM; ++m) {
    const double p = __builtin_fma(cr[m - 1], cm, ci[m - 1] * sm);
    if (m & 1) fa += p; else fb += p;
    if (DERIV) {
      const double q = __builtin_fma(ci[m - 1], cm, -(cr[m - 1] * sm));
      g = __builtin_fma((double)m, q, g);
      h = __builtin_fma((double)(m * m), p, h);
    }
    const double cn = __builtin_fma(cm, c1, -(sm * s1)), sn = __builtin_fma(sm, c1, cm * s1);
    cm = cn;
    sm = sn;
  }
  f = fa + fb;
  f1 = g;
  f2 = -h;
}

// What a launch reads besides the operand: the pair lists (bucket m is [starts[m], starts[m + 1])), the templates in pair form,
// the key values, the grid and its table -- all wave-uniform -- and, for norm2, the selected columns in ascending order.
struct align_params {
  const int32_t *starts, *ia, *ib, *cols;
  const double *tmpl, *keyval, *theta, *trig;
  int K, T, n_theta, newton, key, n_cols;
  double step_deg, period;
};

// The two operand layouts of the shared body.  at(j): moment j of the lane's unit; out(t): where its value for template t goes.
struct rows_access {  // (N, P) rows -> (N, T) outputs
  const double* __restrict__ row;
  long long r;
  int T;
  __device__ __forceinline__ double at(int j) const { return row[j]; }
  __device__ __forceinline__ size_t out(int t) const { return (size_t)(r * T + t); }
};
struct planes_access {  // (P, .) planes `stride` apart -> (T, .) planes `out_stride` apart
  const double* __restrict__ px;  // plane 0 at the lane's pixel
  size_t stride, out_stride;
  long long i;
  __device__ __forceinline__ double at(int j) const { return px[(size_t)j * stride]; }
  __device__ __forceinline__ size_t out(int t) const { return (size_t)t * out_stride + (size_t)i; }
};

// Everything after the load, for both kernels.  Every multiply-add below is an explicit fma and every other operation is rounded
// on its own (contraction is off for this unit, see the top): the two instantiations run the same operations in the same order.
template <int NM, int TB, class A>
__device__ __forceinline__ void align_body(const A& x, bool live, long long unit, const align_params& q, double* __restrict__ angle,
                                           double* __restrict__ score, int32_t* __restrict__ best, double* __restrict__ norm2) {
  const int T = q.T, K = q.K;
  double best_val = 0.0;
  int best_t = 0;
  for (int t0 = 0; t0 < T; t0 += TB) {
    const double* tp[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) tp[u] = q.tmpl + (size_t)(t0 + u < T ? t0 + u : T - 1) * K * 2;  // past T: the last one again, not written
    double c0[TB], cr[TB][NM], ci[TB][NM];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      c0[u] = 0.0;
#pragma unroll
      for (int m = 0; m < NM; ++m) cr[u][m] = ci[u][m] = 0.0;
    }
    for (int k = q.starts[0]; k < q.starts[1]; ++k) {
      const double a = x.at(q.ia[k]);
#pragma unroll
      for (int u = 0; u < TB; ++u) c0[u] = __builtin_fma(a, tp[u][2 * k], c0[u]);
    }
#pragma unroll
    for (int m = 1; m <= NM; ++m)
      for (int k = q.starts[m]; k < q.starts[m + 1]; ++k) {
        const double a = x.at(q.ia[k]), b = x.at(q.ib[k]);
#pragma unroll
        for (int u = 0; u < TB; ++u) {
          const double tr = tp[u][2 * k], ti = tp[u][2 * k + 1];  // z conj(t) = (a tr + b ti) + i (b tr - a ti)
          cr[u][m - 1] = __builtin_fma(a, tr, __builtin_fma(b, ti, cr[u][m - 1]));
          ci[u][m - 1] = __builtin_fma(b, tr, __builtin_fma(-a, ti, ci[u][m - 1]));
        }
      }

    // ---- the grid: one pass over the table for the TB templates
    double fmax[TB];
    int jmax[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      fmax[u] = 0.0;
      jmax[u] = 0;
    }
    for (int j = 0; j < q.n_theta; ++j) {
      const double* __restrict__ tj = q.trig + (size_t)j * (2 * NM);
      double fc[TB], fs[TB];
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        fc[u] = c0[u];
        fs[u] = 0.0;
      }
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const double cs = tj[m], sn = tj[NM + m];
#pragma unroll
        for (int u = 0; u < TB; ++u) {
          fc[u] = __builtin_fma(cr[u][m], cs, fc[u]);
          fs[u] = __builtin_fma(ci[u][m], sn, fs[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        const double f = fc[u] + fs[u];
        if (j == 0 || f > fmax[u]) {
          fmax[u] = f;
          jmax[u] = j;
        }
      }
    }

    // ---- refinement and the outputs
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      const int t = t0 + u;
      const double th0 = q.theta[jmax[u]];
      double ang = th0, sc = fmax[u];
      if (q.newton > 0) {
        const double lo = th0 - q.step_deg, hi = th0 + q.step_deg;
        double th = th0;
        for (int it = 0; it < q.newton; ++it) {
          double f, f1, f2;
          align_eval<NM, true>(c0[u], cr[u], ci[u], th, f, f1, f2);
          if (f2 < 0.0) {
            const double next = __builtin_fma(-(f1 / f2), R2D, th);  // th - (f1 / f2) R2D, one rounding
            th = next < lo ? lo : next > hi ? hi : next == next ? next : th;
          }
        }
        if (th < 0.0) th += q.period;
        if (th >= q.period) th -= q.period;
        double f, f1, f2;
        align_eval<NM, false>(c0[u], cr[u], ci[u], th, f, f1, f2);
        if (f >= fmax[u]) {
          ang = th;
          sc = f;
        }
      }
      if (t < T) {
        if (live && angle) angle[x.out(t)] = ang;
        if (live && score) score[x.out(t)] = sc;
        const double val = q.key == 0 ? __builtin_fma(-2.0, sc, q.keyval[t]) : sc * q.keyval[t];
        if (t == 0 || (q.key == 0 ? val < best_val : val > best_val)) {
          best_val = val;
          best_t = t;
        }
      }
    }
  }
  if (live && best) best[unit] = best_t;
  if (norm2) {  // sum_j s_j x_j^2: one chain over the selected columns, ascending
    double sq = 0.0;
    for (int c = 0; c < q.n_cols; ++c) {
      const double v = x.at(q.cols[c]);
      sq = __builtin_fma(v, v, sq);
    }
    if (live) norm2[unit] = sq;
  }
}

template <int NM, int TB>
__global__ __launch_bounds__(256) void zk_align_kernel(const double* __restrict__ rows, long long n_rows, int P, align_params q,
                                                       double* __restrict__ angle, double* __restrict__ score,
                                                       int32_t* __restrict__ best) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < n_rows;
  const rows_access x{rows + (live ? r : 0) * P, r, q.T};
  align_body<NM, TB>(x, live, r, q, angle, score, best, nullptr);
}

// One pixel per lane: a wave reads one contiguous 512-byte run per moment plane.  A lane past the end reads pixel 0 and writes
// nothing.  All offsets are 64-bit.
template <int NM, int TB>
__global__ __launch_bounds__(256) void zk_align_planes_kernel(const double* __restrict__ planes, long long n_pixels, long long plane_stride,
                                                              align_params q, double* __restrict__ angle, double* __restrict__ score,
                                                              int32_t* __restrict__ best, double* __restrict__ norm2,
                                                              long long out_plane_stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n_pixels;
  const planes_access x{planes + (live ? i : 0), (size_t)plane_stride, (size_t)out_plane_stride, i};
  align_body<NM, TB>(x, live, i, q, angle, score, best, norm2);
}

__global__ __launch_bounds__(256) void zk_rotate_rows_kernel(const double* rows, long long n_rows, int P, const int32_t* __restrict__ starts,
                                                             const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, int m_top,
                                                             const double* __restrict__ angles, double* out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const double* src = rows + r * P;  // may alias dst: a pair is read before it is written, and no other lane touches the row
  double* dst = out + r * P;
  const double x = to_radians(angles[r]);
  for (int k = starts[0]; k < starts[1]; ++k) dst[ia[k]] = src[ia[k]];
  for (int m = 1; m <= m_top; ++m) {
    const int k0 = starts[m], k1 = starts[m + 1];
    if (k0 == k1) continue;
    double s, c;
    sincos((double)m * x, &s, &c);
    for (int k = k0; k < k1; ++k) {
      const double a = src[ia[k]], b = src[ib[k]];
      dst[ia[k]] = __builtin_fma(a, c, b * s);
      dst[ib[k]] = __builtin_fma(b, c, -(a * s));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

// the pairs of a label set, sorted by |m|: pair k has columns ia[k] (m >= 0) and ib[k] (m < 0; ia[k] again where m = 0, never
// read), and bucket m is [starts[m], starts[m + 1])
struct align_pairs {
  std::vector<int32_t> ia, ib, starts;
  std::vector<char> sel;  // per column
  int m_top = 0;          // largest |m| among the pairs kept
  int K = 0;
};

int build_pairs(const char* who, int P, const int32_t* n, const int32_t* m, const int32_t* select, bool selected_only, align_pairs* out) {
  const std::string name(who);
  if (P < 1 || P > (ZK_ALIGN_MAX_M + 1) * (ZK_ALIGN_MAX_M + 1)) return zk_fail(ZK_E_BADARG, name + ": needs between 1 and 1681 moments per row");
  if (!n || !m) return zk_fail(ZK_E_BADARG, name + ": null label pointer");
  const int W = 2 * ZK_ALIGN_MAX_M + 1;
  std::vector<int32_t> col((size_t)(ZK_ALIGN_MAX_M + 1) * W, -1);
  for (int j = 0; j < P; ++j) {
    const int am = m[j] < 0 ? -m[j] : m[j];
    if (n[j] < 0 || n[j] > ZK_ALIGN_MAX_M || am > n[j]) return zk_fail(ZK_E_BADARG, name + ": labels need 0 <= |m| <= n <= 40");
    int32_t& c = col[(size_t)n[j] * W + m[j] + ZK_ALIGN_MAX_M];
    if (c >= 0) return zk_fail(ZK_E_BADARG, name + ": a label (n, m) occurs twice");
    c = j;
  }
  out->sel.assign(P, 1);
  if (select)
    for (int j = 0; j < P; ++j) out->sel[j] = select[j] != 0;
  std::vector<std::vector<int32_t>> bucket(ZK_ALIGN_MAX_M + 1);
  for (int j = 0; j < P; ++j) {
    const int32_t partner = col[(size_t)n[j] * W - m[j] + ZK_ALIGN_MAX_M];
    if (partner < 0)
      return zk_fail(ZK_E_BADARG, name + ": the label set is not paired: (n, m) = (" + std::to_string(n[j]) + ", " + std::to_string(m[j]) +
                                      ") has no (n, -m) beside it (full ZPs sets and select()ed sets qualify)");
    if (out->sel[j] != out->sel[partner]) return zk_fail(ZK_E_BADARG, name + ": the selection splits the pair (n, +-m)");
    if (m[j] >= 0 && (out->sel[j] || !selected_only)) bucket[m[j]].push_back(j);
  }
  out->starts.assign(ZK_ALIGN_STARTS, 0);
  out->ia.clear();
  out->ib.clear();
  out->m_top = 0;
  for (int mm = 0; mm <= ZK_ALIGN_MAX_M; ++mm) {
    out->starts[mm] = (int32_t)out->ia.size();
    for (int32_t j : bucket[mm]) {
      out->ia.push_back(j);
      out->ib.push_back(col[(size_t)n[j] * W - m[j] + ZK_ALIGN_MAX_M]);
      out->m_top = mm;
    }
  }
  for (int mm = ZK_ALIGN_MAX_M + 1; mm < ZK_ALIGN_STARTS; ++mm) out->starts[mm] = (int32_t)out->ia.size();
  out->K = (int)out->ia.size();
  return 0;
}

struct align_table {
  std::vector<double> key;  // [NM, n_theta, symmetry | theta (n_theta) | trig (n_theta, 2 NM)]
  double* dev = nullptr;    // theta, then trig
};

struct align_slot {
  void* h_pin = nullptr;
  void* d = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;  // the last launch that reads the slot
  bool used = false;
};

struct align_state {
  zk_stage stage;  // the host variants: their kernel stream and staging (zk_ring.h)
  std::vector<align_table> tables;
  align_slot slots[ZK_ALIGN_SLOTS];
  int next = 0;
};

std::mutex g_mu;                                // one call at a time per process: the state below is shared
align_state* g_state[ZK_DEVICE_TABLE] = {};     // per device, created on first use, kept for the life of the process
zk_device_bytes g_host_chunk;                   // zk_align_set_host_chunk: input + output of a chunk of the host variants; 0: 256 MiB
zk_device_bytes g_band_bytes;                   // zk_align_set_band_bytes: moments per band of zk_frame_align; 0: 1 GiB

int get_state(int device, align_state** out) {
  if (!g_state[device]) {
    align_state* s = new (std::nothrow) align_state();
    if (!s) return zk_fail(ZK_E_NOMEM, "out of host memory");
    int rc = zk_stage_create(&s->stage);
    for (int k = 0; k < ZK_ALIGN_SLOTS && !rc; ++k) {
      const hipError_t e = hipEventCreateWithFlags(&s->slots[k].ev, hipEventDisableTiming);
      if (e != hipSuccess) rc = zk_hip_fail(e, "hipEventCreateWithFlags");
    }
    if (rc) {
      zk_stage_destroy(&s->stage);
      for (int k = 0; k < ZK_ALIGN_SLOTS; ++k)
        if (s->slots[k].ev) (void)hipEventDestroy(s->slots[k].ev);
      delete s;
      return rc;
    }
    g_state[device] = s;
  }
  *out = g_state[device];
  return 0;
}

// how every entry point opens, once its arguments have passed: the device is there and current, the call is the only one, and
// the device's state exists
struct align_call {
  std::optional<zk_device_scope> scope;
  std::unique_lock<std::mutex> lock;
  align_state* s = nullptr;
  int open(int device) {
    const int rc = zk_check_device(device, ZK_DEVICE_TABLE);
    if (rc) return rc;
    scope.emplace(device);
    if (scope->err != hipSuccess) return zk_hip_fail(scope->err, "hipSetDevice");
    lock = std::unique_lock<std::mutex>(g_mu);
    return get_state(device, &s);
  }
};

// the two byte knobs only keep a number; like every entry point they refuse a device that is not there
int set_bytes(zk_device_bytes* knob, int device, int64_t bytes) {
  if (bytes < 0) return zk_fail(ZK_E_BADARG, "bad arguments");
  const int rc = zk_check_device(device, ZK_DEVICE_TABLE);
  return rc ? rc : knob->set(device, bytes, "bad arguments");
}

// the next operand slot with room for `bytes`; its previous reader has finished (a wait only when ZK_ALIGN_SLOTS calls are
// still in flight)
int take_slot(align_state* s, size_t bytes, align_slot** out) {
  align_slot* sl = &s->slots[s->next];
  s->next = (s->next + 1) % ZK_ALIGN_SLOTS;
  if (sl->used) {
    ZK_HIP(hipEventSynchronize(sl->ev));
    sl->used = false;
  }
  if (sl->cap < bytes) {
    if (sl->h_pin) (void)hipHostFree(sl->h_pin);
    if (sl->d) (void)hipFree(sl->d);
    sl->h_pin = sl->d = nullptr;
    sl->cap = 0;
    const size_t want = (bytes + 4095) & ~(size_t)4095;
    ZK_HIP(hipHostMalloc(&sl->h_pin, want, hipHostMallocDefault));
    ZK_HIP(hipMalloc(&sl->d, want));
    sl->cap = want;
  }
  *out = sl;
  return 0;
}

// what a launch reads besides the operand
struct align_job {
  int P = 0, K = 0, T = 0, NM = 0, n_theta = 0, newton = 0, key = 0, m_top = 0, n_cols = 0;
  double step = 0.0, period = 0.0;
  const int32_t *starts = nullptr, *ia = nullptr, *ib = nullptr, *cols = nullptr;
  const double *tmpl = nullptr, *keyval = nullptr, *theta = nullptr, *trig = nullptr;
  align_slot* slot = nullptr;
  align_params params() const {
    return {starts, ia, ib, cols, tmpl, keyval, theta, trig, K, T, n_theta, newton, key, n_cols, step, period};
  }
};

const int NM_INSTANCES[] = {2, 4, 6, 8, 10, 12, 16, 24, 40};

// one launch; `pl` (planes) selects the layout: planes of plane_stride, outputs of out_stride and norm2, or rows of P
struct align_operand {
  const double* data;
  bool planes;
  int64_t plane_stride, out_stride;
  double* norm2;
};

template <int NM, int TB>
int launch_align_one(const align_job& j, const align_operand& o, int64_t n, double* angle, double* score, int32_t* best, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256));
  if (o.planes)
    hipLaunchKernelGGL((zk_align_planes_kernel<NM, TB>), grid, dim3(256), 0, s, o.data, (long long)n, (long long)o.plane_stride, j.params(),
                       angle, score, best, o.norm2, (long long)o.out_stride);
  else
    hipLaunchKernelGGL((zk_align_kernel<NM, TB>), grid, dim3(256), 0, s, o.data, (long long)n, j.P, j.params(), angle, score, best);
  ZK_HIP(hipGetLastError());
  return 0;
}

int launch_align_any(const align_job& j, const align_operand& o, int64_t n, double* angle, double* score, int32_t* best, hipStream_t s) {
  switch (j.NM) {
    case 2: return launch_align_one<2, 4>(j, o, n, angle, score, best, s);
    case 4: return launch_align_one<4, 4>(j, o, n, angle, score, best, s);
    case 6: return launch_align_one<6, 4>(j, o, n, angle, score, best, s);
    case 8: return launch_align_one<8, 4>(j, o, n, angle, score, best, s);
    case 10: return launch_align_one<10, 4>(j, o, n, angle, score, best, s);
    case 12: return launch_align_one<12, 4>(j, o, n, angle, score, best, s);
    case 16: return launch_align_one<16, 2>(j, o, n, angle, score, best, s);
    case 24: return launch_align_one<24, 2>(j, o, n, angle, score, best, s);
    case 40: return launch_align_one<40, 1>(j, o, n, angle, score, best, s);
  }
  return zk_fail(ZK_E_BADARG, "align: no kernel instance");
}

int launch_align(const align_job& j, const double* rows, int64_t n, double* angle, double* score, int32_t* best, hipStream_t s) {
  return launch_align_any(j, align_operand{rows, false, 0, 0, nullptr}, n, angle, score, best, s);
}

int launch_align_planes(const align_job& j, const double* planes, int64_t n, int64_t plane_stride, double* angle, double* score,
                        int32_t* best, double* norm2, int64_t out_stride, hipStream_t s) {
  return launch_align_any(j, align_operand{planes, true, plane_stride, out_stride, norm2}, n, angle, score, best, s);
}

// the device table of an option set: looked up by value, uploaded (blocking) on the first call with it only
int find_table(align_state* s, int NM, int n_theta, int symmetry, const double* trig_host, int trig_m, const double** theta_dev,
               const double** trig_dev) {
  std::vector<double> key(3 + (size_t)n_theta * (1 + 2 * NM), 0.0);
  key[0] = NM;
  key[1] = n_theta;
  key[2] = symmetry;
  double* th = key.data() + 3;
  double* tr = th + n_theta;
  const double step = (360.0 / (double)symmetry) / (double)n_theta;  // numpy.linspace(0, 360 / symmetry, n_theta, endpoint=False)
  for (int j = 0; j < n_theta; ++j) {
    th[j] = (double)j * step;
    for (int m = 1; m <= NM; ++m) {
      double c = 0.0, sn = 0.0;  // columns past the set's largest m: their c_m are zero
      if (trig_host) {
        if (m <= trig_m) {
          c = trig_host[(size_t)j * 2 * trig_m + m - 1];
          sn = trig_host[(size_t)j * 2 * trig_m + trig_m + m - 1];
        }
      } else {
        const double x = (double)m * (th[j] * (M_PI / 180.0));
        c = cos(x);
        sn = sin(x);
      }
      tr[(size_t)j * 2 * NM + m - 1] = c;
      tr[(size_t)j * 2 * NM + NM + m - 1] = sn;
    }
  }
  for (size_t k = 0; k < s->tables.size(); ++k)
    if (s->tables[k].key == key) {
      if (k) std::swap(s->tables[k], s->tables[k - 1]);  // drift towards the front: eviction takes the back
      const align_table& t = s->tables[k ? k - 1 : 0];
      *theta_dev = t.dev;
      *trig_dev = t.dev + n_theta;
      return 0;
    }
  if (s->tables.size() >= ZK_ALIGN_TABLES) {
    ZK_HIP(hipDeviceSynchronize());  // some launch may still read the table that goes
    if (s->tables.back().dev) (void)hipFree(s->tables.back().dev);
    s->tables.pop_back();
  }
  align_table t;
  const size_t bytes = (key.size() - 3) * sizeof(double);
  ZK_HIP(hipMalloc((void**)&t.dev, bytes));
  const hipError_t e = hipMemcpy(t.dev, key.data() + 3, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    return zk_hip_fail(e, "hipMemcpy(align table)");
  }
  t.key = std::move(key);
  *theta_dev = t.dev;
  *trig_dev = t.dev + n_theta;
  s->tables.insert(s->tables.begin(), std::move(t));
  return 0;
}

// pair lists (and templates, key values) into a slot, on their way to the device on `stream`
int upload_blob(align_state* s, const align_pairs& pr, const double* tmpl_pairs, const double* keyval, int T, hipStream_t stream,
                align_job* job, bool with_cols = false) {
  std::vector<int32_t> cols;  // the selected columns, ascending (norm2 of the planes kernel); none for the other callers
  if (with_cols)
    for (size_t jc = 0; jc < pr.sel.size(); ++jc)
      if (pr.sel[jc]) cols.push_back((int32_t)jc);
  const size_t C = cols.size(), cpad = (C + 1) & ~(size_t)1;
  const size_t K = (size_t)pr.K, ints = ZK_ALIGN_STARTS + 2 * ((K + 1) & ~(size_t)1) + cpad;
  const size_t bytes = ints * sizeof(int32_t) + ((size_t)T * K * 2 + (size_t)T) * sizeof(double);
  align_slot* sl = nullptr;
  const int rc = take_slot(s, bytes, &sl);
  if (rc) return rc;
  int32_t* hi = (int32_t*)sl->h_pin;
  const size_t kpad = (K + 1) & ~(size_t)1;
  memcpy(hi, pr.starts.data(), ZK_ALIGN_STARTS * sizeof(int32_t));
  if (K) memcpy(hi + ZK_ALIGN_STARTS, pr.ia.data(), K * sizeof(int32_t));
  if (K) memcpy(hi + ZK_ALIGN_STARTS + kpad, pr.ib.data(), K * sizeof(int32_t));
  if (C) memcpy(hi + ZK_ALIGN_STARTS + 2 * kpad, cols.data(), C * sizeof(int32_t));
  double* hd = (double*)(hi + ints);
  if (T && K) memcpy(hd, tmpl_pairs, (size_t)T * K * 2 * sizeof(double));
  if (T) memcpy(hd + (size_t)T * K * 2, keyval, (size_t)T * sizeof(double));
  ZK_HIP(hipMemcpyAsync(sl->d, sl->h_pin, bytes, hipMemcpyHostToDevice, stream));
  const int32_t* di = (const int32_t*)sl->d;
  job->starts = di;
  job->ia = di + ZK_ALIGN_STARTS;
  job->ib = di + ZK_ALIGN_STARTS + kpad;
  job->cols = di + ZK_ALIGN_STARTS + 2 * kpad;
  job->n_cols = (int)C;
  job->tmpl = (const double*)(di + ints);
  job->keyval = job->tmpl + (size_t)T * K * 2;
  job->slot = sl;
  return 0;
}

int slot_done(align_job* job, hipStream_t stream) {
  ZK_HIP(hipEventRecord(job->slot->ev, stream));
  job->slot->used = true;
  return 0;
}

// ---- argument checks: everything that can be refused is refused here, before any device call
struct align_args {
  align_pairs pairs;
  std::vector<double> tmpl_pairs, keyval;
  int NM = 0;
};

int check_align(const void* rows, int64_t n_rows, int P, const int32_t* n, const int32_t* m, const double* templates, int T,
                const int32_t* select, int n_theta, int symmetry, int newton, int key, const double* trig_host, int trig_m,
                const double* key_values, align_args* a) {
  if (n_rows < 0) return zk_fail(ZK_E_BADARG, "align: negative row count");
  if (T < 1 || T > ZK_ALIGN_MAX_T) return zk_fail(ZK_E_BADARG, "align: needs between 1 and 64 templates");
  if (n_theta < 1 || n_theta > ZK_ALIGN_MAX_THETA) return zk_fail(ZK_E_BADARG, "align: n_theta must be between 1 and 4096");
  if (symmetry < 1 || symmetry > 360) return zk_fail(ZK_E_BADARG, "align: symmetry must be between 1 and 360");
  if (newton < 0 || newton > ZK_ALIGN_MAX_NEWTON) return zk_fail(ZK_E_BADARG, "align: newton_iters must be between 0 and 16");
  if (key != ZK_ALIGN_DISTANCE && key != ZK_ALIGN_COSINE) return zk_fail(ZK_E_BADARG, "align: key must be ZK_ALIGN_DISTANCE or ZK_ALIGN_COSINE");
  if (!templates || (n_rows > 0 && !rows)) return zk_fail(ZK_E_BADARG, "align: null pointer");
  const int rc = build_pairs("align", P, n, m, select, true, &a->pairs);
  if (rc) return rc;
  const align_pairs& pr = a->pairs;
  if (trig_host && trig_m < pr.m_top) return zk_fail(ZK_E_BADARG, "align: the trig table is narrower than the largest selected |m|");
  a->NM = 0;
  for (int v : NM_INSTANCES)
    if (!a->NM && v >= pr.m_top) a->NM = v;
  a->tmpl_pairs.assign((size_t)T * pr.K * 2, 0.0);
  a->keyval.assign(T, 0.0);
  for (int t = 0; t < T; ++t) {
    const double* row = templates + (size_t)t * P;
    for (int k = 0; k < pr.K; ++k) {
      a->tmpl_pairs[((size_t)t * pr.K + k) * 2] = row[pr.ia[k]];
      a->tmpl_pairs[((size_t)t * pr.K + k) * 2 + 1] = pr.ib[k] != pr.ia[k] ? row[pr.ib[k]] : 0.0;
    }
    if (key_values)
      a->keyval[t] = key_values[t];
    else {
      double sq = 0.0;
      for (int j = 0; j < P; ++j)
        if (pr.sel[j]) sq += row[j] * row[j];
      a->keyval[t] = key == ZK_ALIGN_DISTANCE ? sq : 1.0 / sqrt(sq);
    }
  }
  return 0;
}

int prepare_align(align_state* s, const align_args& a, int P, int T, int n_theta, int symmetry, int newton, int key, const double* trig_host,
                  int trig_m, hipStream_t stream, align_job* job, bool with_cols = false) {
  job->P = P;
  job->K = a.pairs.K;
  job->T = T;
  job->NM = a.NM;
  job->n_theta = n_theta;
  job->newton = newton;
  job->key = key;
  job->period = 360.0 / (double)symmetry;
  job->step = job->period / (double)n_theta;
  int rc = find_table(s, a.NM, n_theta, symmetry, trig_host, trig_m, &job->theta, &job->trig);
  if (rc) return rc;
  return upload_blob(s, a.pairs, a.tmpl_pairs.data(), a.keyval.data(), T, stream, job, with_cols);
}

// what the planes entry points refuse on top of check_align
int check_planes(int64_t n_pixels, int64_t plane_stride, int64_t out_plane_stride) {
  if (plane_stride < n_pixels) return zk_fail(ZK_E_BADARG, "align: plane_stride is smaller than n_pixels");
  if (out_plane_stride < n_pixels) return zk_fail(ZK_E_BADARG, "align: out_plane_stride is smaller than n_pixels");
  if (n_pixels > (int64_t)0x7fffffff * 256) return zk_fail(ZK_E_BADARG, "align: more than 2^39 pixels in one call");
  return 0;
}

int check_rotate(const void* rows, int64_t n_rows, int P, const int32_t* n, const int32_t* m, const void* angles, const void* out,
                 align_pairs* pr) {
  if (n_rows < 0) return zk_fail(ZK_E_BADARG, "rotate_rows: negative row count");
  if (n_rows > 0 && (!rows || !angles || !out)) return zk_fail(ZK_E_BADARG, "rotate_rows: null pointer");
  return build_pairs("rotate_rows", P, n, m, nullptr, false, pr);
}

int launch_rotate(const align_job& j, const double* rows, int64_t n, const double* angles, double* out, hipStream_t s) {
  hipLaunchKernelGGL(zk_rotate_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, (long long)n, j.P, j.starts, j.ia, j.ib,
                     j.m_top, angles, out);
  ZK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int zk_align_set_host_chunk(int device, int64_t chunk_bytes) { return set_bytes(&g_host_chunk, device, chunk_bytes); }

extern "C" int zk_align_rows_dev(int device, const double* rows_dev, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                                 const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                                 int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                                 double* angle_dev, double* score_dev, int32_t* best_dev, void* hip_stream) {
  align_args a;
  int rc = check_align(rows_dev, n_rows, n_poly, n, m, templates_host, n_templates, select, n_theta, symmetry, newton_iters, key, trig_host,
                       trig_m, key_values_host, &a);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  const hipStream_t stream = (hipStream_t)hip_stream;  // exactly the caller's stream
  align_job job;
  if ((rc = prepare_align(s, a, n_poly, n_templates, n_theta, symmetry, newton_iters, key, trig_host, trig_m, stream, &job))) return rc;
  rc = launch_align(job, rows_dev, n_rows, angle_dev, score_dev, best_dev, stream);
  const int rd = slot_done(&job, stream);
  return rc ? rc : rd;
}

extern "C" int zk_align_rows(int device, const double* rows_host, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                             const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                             int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                             double* angle_out, double* score_out, int32_t* best_out) {
  align_args a;
  int rc = check_align(rows_host, n_rows, n_poly, n, m, templates_host, n_templates, select, n_theta, symmetry, newton_iters, key, trig_host,
                       trig_m, key_values_host, &a);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  align_job job;
  if ((rc = prepare_align(s, a, n_poly, n_templates, n_theta, symmetry, newton_iters, key, trig_host, trig_m, s->stage.stream, &job))) return rc;
  zk_ring* r = &s->stage.ring;
  const size_t T = (size_t)n_templates, in_unit = (size_t)n_poly * sizeof(double), out_unit = T * 2 * sizeof(double) + sizeof(int32_t);
  const size_t budget = g_host_chunk.get(device, (size_t)256 << 20);
  const zk_chunks ch = zk_chunk_plan(budget, in_unit + out_unit, 256, n_rows);
  // a slot's output: angle (chunk, T) | score (chunk, T) | best (chunk), each at the offset of a full chunk
  const size_t plane = (size_t)ch.chunk * T * sizeof(double);
  rc = zk_ring_run(
      r, s->stage.stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, 2 * plane + (size_t)ch.chunk * sizeof(int32_t));
        if (!e) e = zk_ring_up(r, s->stage.stream, c, slot, r->d_in[slot], rows_host + (size_t)ch.first(c) * n_poly, (size_t)ch.count(c) * in_unit);
        char* o = (char*)r->d_out[slot];
        return e ? e : launch_align(job, (const double*)r->d_in[slot], ch.count(c), (double*)o, (double*)(o + plane), (int32_t*)(o + 2 * plane), s->stage.stream);
      },
      [&](int64_t c, int slot) -> int {
        const char* o = (const char*)r->d_out[slot];
        const size_t first = (size_t)ch.first(c), cnt = (size_t)ch.count(c);
        if (angle_out) ZK_HIP(hipMemcpyAsync(angle_out + first * T, o, cnt * T * sizeof(double), hipMemcpyDeviceToHost, r->s_out));
        if (score_out) ZK_HIP(hipMemcpyAsync(score_out + first * T, o + plane, cnt * T * sizeof(double), hipMemcpyDeviceToHost, r->s_out));
        if (best_out) ZK_HIP(hipMemcpyAsync(best_out + first, o + 2 * plane, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, r->s_out));
        return 0;
      });
  job.slot->used = false;  // the job has drained
  zk_stage_trim(&s->stage, ZK_STAGE_KEEP_ROWS);
  return rc;
}

extern "C" int zk_align_set_band_bytes(int device, int64_t bytes) { return set_bytes(&g_band_bytes, device, bytes); }

extern "C" int zk_align_planes_dev(int device, const double* planes_dev, int64_t n_pixels, int64_t plane_stride, int n_poly, const int32_t* n,
                                   const int32_t* m, const double* templates_host, int n_templates, const int32_t* select, int n_theta,
                                   int symmetry, int newton_iters, int key, const double* trig_host, int trig_m,
                                   const double* key_values_host, double* angle_dev, double* score_dev, int32_t* best_dev, double* norm2_dev,
                                   int64_t out_plane_stride, void* hip_stream) {
  align_args a;
  int rc = check_align(planes_dev, n_pixels, n_poly, n, m, templates_host, n_templates, select, n_theta, symmetry, newton_iters, key,
                       trig_host, trig_m, key_values_host, &a);
  if (rc) return rc;
  if ((rc = check_planes(n_pixels, plane_stride, out_plane_stride))) return rc;
  if (n_pixels == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  const hipStream_t stream = (hipStream_t)hip_stream;  // exactly the caller's stream
  align_job job;
  if ((rc = prepare_align(s, a, n_poly, n_templates, n_theta, symmetry, newton_iters, key, trig_host, trig_m, stream, &job, true))) return rc;
  rc = launch_align_planes(job, planes_dev, n_pixels, plane_stride, angle_dev, score_dev, best_dev, norm2_dev, out_plane_stride, stream);
  const int rd = slot_done(&job, stream);
  return rc ? rc : rd;
}

extern "C" int zk_align_planes(int device, const double* planes_host, int64_t n_pixels, int64_t plane_stride, int n_poly, const int32_t* n,
                               const int32_t* m, const double* templates_host, int n_templates, const int32_t* select, int n_theta,
                               int symmetry, int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                               double* angle_out, double* score_out, int32_t* best_out, double* norm2_out, int64_t out_plane_stride) {
  align_args a;
  int rc = check_align(planes_host, n_pixels, n_poly, n, m, templates_host, n_templates, select, n_theta, symmetry, newton_iters, key,
                       trig_host, trig_m, key_values_host, &a);
  if (rc) return rc;
  if ((rc = check_planes(n_pixels, plane_stride, out_plane_stride))) return rc;
  if (n_pixels == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  align_job job;
  if ((rc = prepare_align(s, a, n_poly, n_templates, n_theta, symmetry, newton_iters, key, trig_host, trig_m, s->stage.stream, &job, true))) return rc;
  zk_ring* r = &s->stage.ring;
  const size_t T = (size_t)n_templates, in_unit = (size_t)n_poly * sizeof(double), out_unit = (T * 2 + 1) * sizeof(double) + sizeof(int32_t);
  const size_t budget = g_host_chunk.get(device, (size_t)256 << 20);
  const zk_chunks ch = zk_chunk_plan(budget, in_unit + out_unit, 256, n_pixels);
  // a slot's input: (P, chunk) planes; its output: angle (T, chunk) | score (T, chunk) | norm2 (chunk) | best (chunk)
  const size_t line = (size_t)ch.chunk * sizeof(double), plane = T * line;
  rc = zk_ring_run(
      r, s->stage.stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)n_poly * line, 2 * plane + line + (size_t)ch.chunk * sizeof(int32_t));
        if (!e)  // a chunk of a (P, .) operand: P pieces, one per plane
          e = zk_ring_up_2d(r, s->stage.stream, c, slot, r->d_in[slot], line, planes_host + ch.first(c), (size_t)plane_stride * sizeof(double),
                            (size_t)ch.count(c) * sizeof(double), (size_t)n_poly);
        char* o = (char*)r->d_out[slot];
        return e ? e : launch_align_planes(job, (const double*)r->d_in[slot], ch.count(c), ch.chunk, (double*)o, (double*)(o + plane),
                                           (int32_t*)(o + 2 * plane + line), (double*)(o + 2 * plane), ch.chunk, s->stage.stream);
      },
      [&](int64_t c, int slot) -> int {
        const char* o = (const char*)r->d_out[slot];
        const size_t first = (size_t)ch.first(c), w = (size_t)ch.count(c) * sizeof(double), op = (size_t)out_plane_stride * sizeof(double);
        if (angle_out) ZK_HIP(hipMemcpy2DAsync(angle_out + first, op, o, line, w, T, hipMemcpyDeviceToHost, r->s_out));
        if (score_out) ZK_HIP(hipMemcpy2DAsync(score_out + first, op, o + plane, line, w, T, hipMemcpyDeviceToHost, r->s_out));
        if (norm2_out) ZK_HIP(hipMemcpyAsync(norm2_out + first, o + 2 * plane, w, hipMemcpyDeviceToHost, r->s_out));
        if (best_out)
          ZK_HIP(hipMemcpyAsync(best_out + first, o + 2 * plane + line, (size_t)ch.count(c) * sizeof(int32_t), hipMemcpyDeviceToHost, r->s_out));
        return 0;
      });
  job.slot->used = false;  // the job has drained
  zk_stage_trim(&s->stage, ZK_STAGE_KEEP_ROWS);
  return rc;
}

// ---- frame -> maps
// everything zk_frame_align(_dev) refuses, before any device call; fills `a` when given
static int frame_align_check(const zk_plan* p, const void* image, int dtype, bool narrow_ok, int64_t H, int64_t W, int64_t row0,
                             int64_t n_rows, const double* templates, int T, const int32_t* select, int n_theta, int symmetry, int newton,
                             int key, const double* trig_host, int trig_m, const double* key_values, int64_t out_plane_stride,
                             align_args* a) {
  if (!p) return zk_fail(ZK_E_BADARG, "null plan");
  if (narrow_ok ? !zk_is_elem(dtype) : (dtype != ZK_F32 && dtype != ZK_F64))
    return zk_fail(ZK_E_BADARG, narrow_ok ? "dtype must be ZK_F32, ZK_F64, ZK_U8, ZK_U16 or ZK_I16" : "dtype must be ZK_F32 or ZK_F64");
  if (H <= 0 || W <= 0 || H > 0x3fffffff || W > 0x3fffffff) return zk_fail(ZK_E_BADARG, "bad frame shape");
  if (row0 < 0 || n_rows < 0 || row0 + n_rows > H) return zk_fail(ZK_E_BADARG, "row band outside the frame");
  const int rc = check_align(image, n_rows * W, p->n_poly, p->n.data(), p->m.data(), templates, T, select, n_theta, symmetry, newton, key,
                             trig_host, trig_m, key_values, a);
  return rc ? rc : check_planes(n_rows * W, n_rows * W, out_plane_stride);
}

int zk_frame_align_check(const zk_plan* p, const void* image, int dtype, int64_t H, int64_t W, int64_t row0, int64_t n_rows,
                         const double* templates, int T, const int32_t* select, int n_theta, int symmetry, int newton, int key,
                         const double* trig_host, int trig_m, const double* key_values, int64_t out_plane_stride) {
  align_args a;
  return frame_align_check(p, image, dtype, true, H, W, row0, n_rows, templates, T, select, n_theta, symmetry, newton, key, trig_host, trig_m,
                           key_values, out_plane_stride, &a);
}

extern "C" int zk_frame_align_dev(zk_plan* p, const void* image_dev, int dtype, int64_t H, int64_t W, int64_t row0, int64_t n_rows,
                                  const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                                  int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                                  double* angle_dev, double* score_dev, int32_t* best_dev, double* norm2_dev, int64_t out_plane_stride,
                                  void* hip_stream) {
  align_args a;
  int rc = frame_align_check(p, image_dev, dtype, false, H, W, row0, n_rows, templates_host, n_templates, select, n_theta, symmetry,
                             newton_iters, key, trig_host, trig_m, key_values_host, out_plane_stride, &a);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  align_call call;
  if ((rc = call.open(p->device))) return rc;
  align_state* s = call.s;
  const hipStream_t stream = (hipStream_t)hip_stream;  // exactly the caller's stream
  // rows per band: what the byte limit holds, at least one, whole blocks of the dense kernels (8 rows) where there are that many
  const size_t row_bytes = (size_t)p->n_poly * (size_t)W * sizeof(double);
  const size_t limit = std::min(g_band_bytes.get(p->device, (size_t)1 << 30), (size_t)1 << 30);
  int64_t band = (int64_t)(limit / row_bytes);
  if (band < 1) band = 1;
  if (band >= n_rows) band = n_rows;
  else if (band > 8) band &= ~(int64_t)7;
  if ((rc = zk_ensure((void**)&p->d_scratch, &p->d_scratch_bytes, (size_t)band * row_bytes))) return rc;
  align_job job;
  if ((rc = prepare_align(s, a, p->n_poly, n_templates, n_theta, symmetry, newton_iters, key, trig_host, trig_m, stream, &job, true))) return rc;
  for (int64_t b0 = 0; b0 < n_rows && !rc; b0 += band) {
    const int64_t nb = n_rows - b0 < band ? n_rows - b0 : band, off = b0 * W;
    const long long keep = p->out_plane;
    p->out_plane = 0;  // the scratch matrix is compact: (P, nb, W)
    rc = zk_transform_frame_dev(p, image_dev, dtype, H, W, row0 + b0, nb, p->d_scratch, hip_stream);
    p->out_plane = keep;
    if (!rc)
      rc = launch_align_planes(job, p->d_scratch, nb * W, nb * W, angle_dev ? angle_dev + off : nullptr, score_dev ? score_dev + off : nullptr,
                               best_dev ? best_dev + off : nullptr, norm2_dev ? norm2_dev + off : nullptr, out_plane_stride, stream);
  }
  const int rd = slot_done(&job, stream);
  return rc ? rc : rd;
}

extern "C" int zk_rotate_rows_dev(int device, const double* rows_dev, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                                  const double* angles_dev, double* out_dev, void* hip_stream) {
  align_pairs pr;
  int rc = check_rotate(rows_dev, n_rows, n_poly, n, m, angles_dev, out_dev, &pr);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  const hipStream_t stream = (hipStream_t)hip_stream;
  align_job job;
  job.P = n_poly;
  job.m_top = pr.m_top;
  if ((rc = upload_blob(s, pr, nullptr, nullptr, 0, stream, &job))) return rc;
  rc = launch_rotate(job, rows_dev, n_rows, angles_dev, out_dev, stream);
  const int rd = slot_done(&job, stream);
  return rc ? rc : rd;
}

extern "C" int zk_rotate_rows(int device, const double* rows_host, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                              const double* angles_host, double* out_host) {
  align_pairs pr;
  int rc = check_rotate(rows_host, n_rows, n_poly, n, m, angles_host, out_host, &pr);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  align_call call;
  if ((rc = call.open(device))) return rc;
  align_state* s = call.s;
  align_job job;
  job.P = n_poly;
  job.m_top = pr.m_top;
  if ((rc = upload_blob(s, pr, nullptr, nullptr, 0, s->stage.stream, &job))) return rc;
  zk_ring* r = &s->stage.ring;
  const size_t row_bytes = (size_t)n_poly * sizeof(double);
  const size_t budget = g_host_chunk.get(device, (size_t)256 << 20);
  const zk_chunks ch = zk_chunk_plan(budget, 2 * row_bytes + sizeof(double), 256, n_rows);
  const size_t rows_cap = (size_t)ch.chunk * row_bytes;  // a slot's input: the rows, then their angles
  rc = zk_ring_run(
      r, s->stage.stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, rows_cap + (size_t)ch.chunk * sizeof(double), rows_cap);
        if (e) return e;
        char* in = (char*)r->d_in[slot];
        // the angles go up ahead of the rows on the same stream; zk_ring_up's event then covers both
        if (c >= ZK_RING_SLOTS) ZK_HIP(hipStreamWaitEvent(r->s_in, r->ev_k[slot], 0));
        ZK_HIP(hipMemcpyAsync(in + rows_cap, angles_host + ch.first(c), (size_t)ch.count(c) * sizeof(double), hipMemcpyHostToDevice, r->s_in));
        e = zk_ring_up(r, s->stage.stream, c, slot, in, rows_host + (size_t)ch.first(c) * n_poly, (size_t)ch.count(c) * row_bytes);
        return e ? e : launch_rotate(job, (const double*)in, ch.count(c), (const double*)(in + rows_cap), (double*)r->d_out[slot], s->stage.stream);
      },
      [&](int64_t c, int slot) -> int {
        return zk_ring_down(r, slot, (char*)out_host + (size_t)ch.first(c) * row_bytes, (size_t)ch.count(c) * row_bytes);
      });
  job.slot->used = false;
  zk_stage_trim(&s->stage, ZK_STAGE_KEEP_ROWS);
  return rc;
}
