// zk_host.hip -- the host-buffer entry points of the C ABI (what ZPs.transform calls with NumPy arrays):
// zk_transform_patches / zk_transform_frame / zk_transform_points / zk_frame_maps / zk_moment_maps / zk_points_maps.
// Each cuts its job into chunks and sends them through the plan's stage; state and protocol are zk_ring.h's.
#include <string.h>

#include "zk_ring.h"

struct zk_host_ring {
  zk_stage stage;                          // on the plan's own stream
  void* d_frame = nullptr;                 // whole frame (+ points) of the dense / key-point calls
  size_t frame_cap = 0;
  void* d_raw[ZK_RING_SLOTS] = {};         // narrow inputs (ZK_U8 / U16 / I16) as they arrive, before widening
  size_t raw_cap[ZK_RING_SLOTS] = {};
};

namespace {

bool is_narrow(int dtype) { return dtype == ZK_U8 || dtype == ZK_U16 || dtype == ZK_I16; }
int kernel_dtype(int dtype) { return is_narrow(dtype) ? ZK_F32 : dtype; }  // what the kernels read

// narrow integers -> float32 (exact), 4 elements per thread
template <typename S>
__global__ __launch_bounds__(256) void widen_kernel(const S* __restrict__ in, float* __restrict__ out, long long n) {
  const long long t = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (t + 3 < n) {
    float4 v;
    v.x = (float)in[t];
    v.y = (float)in[t + 1];
    v.z = (float)in[t + 2];
    v.w = (float)in[t + 3];
    *(float4*)(out + t) = v;
  } else {
    for (long long k = t; k < n; ++k) out[k] = (float)in[k];
  }
}

int widen(int dtype, const void* in, float* out, long long n, hipStream_t s) {
  const unsigned blocks = (unsigned)((n + 1023) / 1024);
  if (dtype == ZK_U8) hipLaunchKernelGGL(widen_kernel<uint8_t>, dim3(blocks), dim3(256), 0, s, (const uint8_t*)in, out, n);
  else if (dtype == ZK_U16) hipLaunchKernelGGL(widen_kernel<uint16_t>, dim3(blocks), dim3(256), 0, s, (const uint16_t*)in, out, n);
  else hipLaunchKernelGGL(widen_kernel<int16_t>, dim3(blocks), dim3(256), 0, s, (const int16_t*)in, out, n);
  ZK_HIP(hipGetLastError());
  return 0;
}

size_t chunk_bytes(const zk_plan* p) {
  if (p->host_chunk) return p->host_chunk;
  const long mb = zk_switch_int(ZK_HOST_CHUNK_MB, 256);
  return (size_t)(mb > 0 ? mb : 256) << 20;
}

// What every entry point refuses before it touches the device, in this order.  An entry point without a dtype passes
// ZK_F64, one without a frame H = W = 1, one without a count unit = nullptr.  1: an empty job, nothing to do.
int check_job(const zk_plan* p, int dtype, int64_t H, int64_t W, const char* unit, int64_t n, bool pointers) {
  if (!p) return zk_fail(ZK_E_BADARG, "null plan");
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "dtype must be ZK_F32, ZK_F64, ZK_U8, ZK_U16 or ZK_I16");
  if (H <= 0 || W <= 0) return zk_fail(ZK_E_BADARG, "bad frame shape");
  if (unit && n < 0) return zk_fail(ZK_E_BADARG, std::string("negative ") + unit + " count");
  if (unit && n == 0) return 1;
  if (!pointers) return zk_fail(ZK_E_BADARG, "null host pointer");
  return 0;
}

// the plan's ring, created on the first host call
int ring_get(zk_plan* p, zk_host_ring** out) {
  if (!p->ring) {
    p->ring = new (std::nothrow) zk_host_ring();
    if (!p->ring) return zk_fail(ZK_E_NOMEM, "out of host memory");
    const int rc = zk_stage_create(&p->ring->stage, p->stream);
    if (rc) {
      zk_host_release(p);
      return rc;
    }
  }
  *out = p->ring;
  return 0;
}

}  // namespace

void zk_host_release(zk_plan* p) {
  zk_host_ring* h = p->ring;
  if (!h) return;
  zk_stage_destroy(&h->stage);
  for (int k = 0; k < ZK_RING_SLOTS; ++k)
    if (h->d_raw[k]) (void)hipFree(h->d_raw[k]);
  if (h->d_frame) (void)hipFree(h->d_frame);
  delete h;
  p->ring = nullptr;
}

extern "C" int zk_plan_set_host_chunk(zk_plan* p, int64_t bytes) {
  if (!p || bytes < 0) return zk_fail(ZK_E_BADARG, "bad arguments");
  p->host_chunk = (size_t)bytes;
  return 0;
}

extern "C" int zk_plan_release_staging(zk_plan* p) {
  if (!p) return zk_fail(ZK_E_BADARG, "null plan");
  ZK_ON_PLAN_DEVICE(p);
  ZK_HIP(hipStreamSynchronize(p->stream));
  zk_host_release(p);
  if (p->d_gather) (void)hipFree(p->d_gather);
  p->d_gather = nullptr;
  p->d_gather_bytes = 0;
  if (p->d_scratch) (void)hipFree(p->d_scratch);
  p->d_scratch = nullptr;
  p->d_scratch_bytes = 0;
  return 0;
}

extern "C" int zk_host_alloc(int64_t bytes, void** out) {
  if (!out || bytes < 0) return zk_fail(ZK_E_BADARG, "bad arguments");
  *out = nullptr;
  if (bytes == 0) return 0;
  ZK_HIP(hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable));
  return 0;
}

extern "C" int zk_host_free(void* ptr) {
  if (!ptr) return 0;
  ZK_HIP(hipHostFree(ptr));
  return 0;
}

// ------------------------------------------------------------------------------------------------------
// batch of patches
// ------------------------------------------------------------------------------------------------------
extern "C" int zk_transform_patches(zk_plan* p, const void* patches_host, int dtype, int64_t n_patches,
                                    double* out_host) {
  int rc = check_job(p, dtype, 1, 1, "patch", n_patches, patches_host && out_host);
  if (rc) return rc < 0 ? rc : 0;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  const int kdt = kernel_dtype(dtype);
  const bool narrow = is_narrow(dtype);
  const size_t px_per = (size_t)p->size * p->size;
  const size_t raw_unit = px_per * zk_elem_size(dtype), in_unit = px_per * zk_elem_size(kdt),
               out_unit = (size_t)p->n_poly * sizeof(double);
  const zk_chunks ch = zk_chunk_plan(chunk_bytes(p), in_unit + out_unit, 256, n_patches);  // whole waves of 64 patches
  p->job_units = n_patches;
  struct reset_units {
    zk_plan* p;
    ~reset_units() { p->job_units = 0; }
  } reset{p};
  return zk_ring_run(
      r, p->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, (size_t)ch.chunk * out_unit);
        if (!e && narrow) e = zk_ensure(&h->d_raw[slot], &h->raw_cap[slot], (size_t)ch.chunk * raw_unit);
        if (!e)
          e = zk_ring_up(r, p->stream, c, slot, narrow ? h->d_raw[slot] : r->d_in[slot],
                         (const char*)patches_host + (size_t)ch.first(c) * raw_unit, (size_t)ch.count(c) * raw_unit);
        if (!e && narrow) e = widen(dtype, h->d_raw[slot], (float*)r->d_in[slot], (long long)ch.count(c) * (long long)px_per, p->stream);
        return e ? e : zk_transform_patches_dev(p, r->d_in[slot], kdt, ch.count(c), (double*)r->d_out[slot], p->stream);
      },
      [&](int64_t c, int slot) -> int {
        return zk_ring_down(r, slot, (char*)out_host + (size_t)ch.first(c) * out_unit, (size_t)ch.count(c) * out_unit);
      });
}

// ------------------------------------------------------------------------------------------------------
// dense frame: the frame goes up once, the result comes down a row band at a time
// ------------------------------------------------------------------------------------------------------
namespace {

// copy the (planes, nb, W) band in d_src into rows [b0, b0 + nb) of the host array (planes, H, W)
int band_to_host(double* host, const double* d_src, int64_t planes, int64_t H, int64_t W, int64_t b0, int64_t nb,
                 hipStream_t s) {
  if (nb == H) {
    ZK_HIP(hipMemcpyAsync(host, d_src, (size_t)planes * H * W * sizeof(double), hipMemcpyDeviceToHost, s));
    return 0;
  }
  ZK_HIP(hipMemcpy2DAsync(host + (size_t)b0 * W, (size_t)H * W * sizeof(double), d_src, (size_t)nb * W * sizeof(double),
                          (size_t)nb * W * sizeof(double), (size_t)planes, hipMemcpyDeviceToHost, s));
  return 0;
}

// the whole frame onto the device as the kernels' element type (narrow formats: raw bytes up, widened there), on the
// plan's stream; `extra` = room behind it for the caller
int frame_up(zk_plan* p, zk_host_ring* h, const void* image_host, int dtype, int64_t H, int64_t W, size_t extra) {
  const long long n_px = (long long)H * W;
  const size_t bytes = (size_t)n_px * zk_elem_size(kernel_dtype(dtype));
  int rc = zk_ensure(&h->d_frame, &h->frame_cap, bytes + extra);
  if (rc) return rc;
  if (!is_narrow(dtype)) {
    ZK_HIP(hipMemcpyAsync(h->d_frame, image_host, bytes, hipMemcpyHostToDevice, p->stream));
    return 0;
  }
  const size_t raw = (size_t)n_px * zk_elem_size(dtype);
  if ((rc = zk_ensure(&h->d_raw[0], &h->raw_cap[0], raw))) return rc;
  ZK_HIP(hipMemcpyAsync(h->d_raw[0], image_host, raw, hipMemcpyHostToDevice, p->stream));
  return widen(dtype, h->d_raw[0], (float*)h->d_frame, n_px, p->stream);
}

// the frame, and behind it (256-byte aligned) the point list of a key-point call: *d_pts
int frame_points_up(zk_plan* p, zk_host_ring* h, const void* image_host, int dtype, int64_t H, int64_t W,
                    const int32_t* points_host, int64_t n_points, int32_t** d_pts) {
  const size_t img_bytes = (size_t)H * W * zk_elem_size(kernel_dtype(dtype));
  const size_t img_pad = (img_bytes + 255) & ~(size_t)255;
  const size_t pts_bytes = (size_t)n_points * 2 * sizeof(int32_t);
  const int rc = frame_up(p, h, image_host, dtype, H, W, img_pad - img_bytes + pts_bytes);
  if (rc) return rc;
  *d_pts = (int32_t*)((char*)h->d_frame + img_pad);
  const hipError_t e = hipMemcpyAsync(*d_pts, points_host, pts_bytes, hipMemcpyHostToDevice, p->stream);
  return e == hipSuccess ? 0 : zk_hip_fail(e, "hipMemcpyAsync(points)");
}

// The three outputs of the symmetry maps, each optional, of n units (rows of a moment matrix, or the pixels of a row
// band) a chunk: packed in the slot's d_out as [rot | abs | mirror], planes of n doubles.
struct maps_out {
  double *rot, *ab, *mir;     // host destinations (may be null)
  int64_t pl_rot, pl_abs, pl_mir;
  maps_out(const zk_plan* p, double* rot_host, double* abs_host, double* mirror_host, int n_folds)
      : rot(rot_host), ab(abs_host), mir(mirror_host), pl_rot(rot_host ? n_folds : 0),
        pl_abs(abs_host ? zk_complex_count(zk_full_set_nmax(p)) : 0), pl_mir(mirror_host ? 1 : 0) {}
  size_t unit_bytes() const { return (size_t)(pl_rot + pl_abs + pl_mir + 1) * sizeof(double); }
  double* d_rot(void* d, int64_t n) const { return rot ? (double*)d : nullptr; }
  double* d_abs(void* d, int64_t n) const { return ab ? (double*)d + n * pl_rot : nullptr; }
  double* d_mir(void* d, int64_t n) const { return mir ? (double*)d + n * (pl_rot + pl_abs) : nullptr; }
  // D2H of one chunk of the three row-major outputs
  int rows_to_host(void* d, int64_t first, int64_t n, hipStream_t s) const {
    if (rot) ZK_HIP(hipMemcpyAsync(rot + first * pl_rot, d_rot(d, n), (size_t)n * pl_rot * 8, hipMemcpyDeviceToHost, s));
    if (ab) ZK_HIP(hipMemcpyAsync(ab + first * pl_abs, d_abs(d, n), (size_t)n * pl_abs * 8, hipMemcpyDeviceToHost, s));
    if (mir) ZK_HIP(hipMemcpyAsync(mir + first, d_mir(d, n), (size_t)n * 8, hipMemcpyDeviceToHost, s));
    return 0;
  }
};

}  // namespace

extern "C" int zk_transform_frame(zk_plan* p, const void* image_host, int dtype, int64_t H, int64_t W,
                                  double* out_host) {
  int rc = check_job(p, dtype, H, W, nullptr, 0, image_host && out_host);
  if (rc) return rc;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  if ((rc = frame_up(p, h, image_host, dtype, H, W, 0))) return zk_ring_drain(r, p->stream, rc);
  const size_t row_bytes = (size_t)p->n_poly * W * sizeof(double);
  const zk_chunks band = zk_chunk_plan(chunk_bytes(p), row_bytes, 8, H);  // whole blocks of the dense kernels
  return zk_ring_run(
      r, p->stream, band.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int e = zk_ring_slot(r, slot, 0, (size_t)band.chunk * row_bytes);
        return e ? e : zk_transform_frame_dev(p, h->d_frame, kernel_dtype(dtype), H, W, band.first(c), band.count(c),
                                              (double*)r->d_out[slot], p->stream);
      },
      [&](int64_t c, int slot) -> int {
        return band_to_host(out_host, (const double*)r->d_out[slot], p->n_poly, H, W, band.first(c), band.count(c), r->s_out);
      });
}

// ------------------------------------------------------------------------------------------------------
// fused symmetry maps
// ------------------------------------------------------------------------------------------------------
extern "C" int zk_frame_maps(zk_plan* p, const void* image_host, int dtype, int64_t H, int64_t W,
                             const int32_t* folds, int n_folds, const int32_t* m_unselect, int n_unselect,
                             int p_norm, const double* theta, int n_theta, double* rot_host, double* abs_host,
                             double* mirror_host) {
  int rc = check_job(p, dtype, H, W, nullptr, 0, image_host);
  if (rc) return rc;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  if ((rc = frame_up(p, h, image_host, dtype, H, W, 0))) return zk_ring_drain(r, p->stream, rc);
  const maps_out o(p, rot_host, abs_host, mirror_host, n_folds);
  const size_t row_bytes = o.unit_bytes() * W;
  const zk_chunks band = zk_chunk_plan(chunk_bytes(p), row_bytes, 8, H);
  return zk_ring_run(
      r, p->stream, band.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int e = zk_ring_slot(r, slot, 0, (size_t)band.chunk * row_bytes);
        void* d = r->d_out[slot];
        const int64_t n = band.count(c) * W;
        return e ? e : zk_frame_maps_dev(p, h->d_frame, kernel_dtype(dtype), H, W, band.first(c), band.count(c), folds, n_folds,
                                         m_unselect, n_unselect, p_norm, theta, n_theta, o.d_rot(d, n), o.d_abs(d, n), o.d_mir(d, n),
                                         p->stream);
      },
      [&](int64_t c, int slot) -> int {
        void* d = r->d_out[slot];
        const int64_t b0 = band.first(c), nb = band.count(c);
        int e = 0;
        if (o.rot) e = band_to_host(o.rot, o.d_rot(d, nb * W), o.pl_rot, H, W, b0, nb, r->s_out);
        if (o.ab && !e) e = band_to_host(o.ab, o.d_abs(d, nb * W), o.pl_abs, H, W, b0, nb, r->s_out);
        if (o.mir && !e) e = band_to_host(o.mir, o.d_mir(d, nb * W), 1, H, W, b0, nb, r->s_out);
        return e;
      });
}

// ------------------------------------------------------------------------------------------------------
// rotation-aligned template maps (zk_align.hip): the frame goes up once, the maps of rows [row0, row0 + n_rows) come down a
// row band at a time; a slot holds angle (T, band, W) | score (T, band, W) | norm2 (band, W) | best (band, W)
// ------------------------------------------------------------------------------------------------------
extern "C" int zk_frame_align(zk_plan* p, const void* image_host, int dtype, int64_t H, int64_t W, int64_t row0, int64_t n_rows,
                              const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                              int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                              double* angle_host, double* score_host, int32_t* best_host, double* norm2_host, int64_t out_plane_stride) {
  int rc = zk_frame_align_check(p, image_host, dtype, H, W, row0, n_rows, templates_host, n_templates, select, n_theta, symmetry, newton_iters,
                                key, trig_host, trig_m, key_values_host, out_plane_stride);
  if (rc) return rc;
  if (n_rows == 0) return 0;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  if ((rc = frame_up(p, h, image_host, dtype, H, W, 0))) return zk_ring_drain(r, p->stream, rc);
  const size_t T = (size_t)n_templates, px_bytes = (2 * T + 1) * sizeof(double) + sizeof(int32_t);
  const zk_chunks band = zk_chunk_plan(chunk_bytes(p), px_bytes * W, 8, n_rows);
  const size_t line = (size_t)band.chunk * W * sizeof(double), plane = T * line;
  return zk_ring_run(
      r, p->stream, band.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int e = zk_ring_slot(r, slot, 0, 2 * plane + line + (size_t)band.chunk * W * sizeof(int32_t));
        char* o = (char*)r->d_out[slot];
        return e ? e : zk_frame_align_dev(p, h->d_frame, kernel_dtype(dtype), H, W, row0 + band.first(c), band.count(c), templates_host,
                                          n_templates, select, n_theta, symmetry, newton_iters, key, trig_host, trig_m, key_values_host,
                                          (double*)o, (double*)(o + plane), (int32_t*)(o + 2 * plane + line), (double*)(o + 2 * plane),
                                          band.chunk * W, p->stream);
      },
      [&](int64_t c, int slot) -> int {
        const char* o = (const char*)r->d_out[slot];
        const size_t first = (size_t)band.first(c) * W, n = (size_t)band.count(c) * W, w = n * sizeof(double),
                     op = (size_t)out_plane_stride * sizeof(double);
        if (angle_host) ZK_HIP(hipMemcpy2DAsync(angle_host + first, op, o, line, w, T, hipMemcpyDeviceToHost, r->s_out));
        if (score_host) ZK_HIP(hipMemcpy2DAsync(score_host + first, op, o + plane, line, w, T, hipMemcpyDeviceToHost, r->s_out));
        if (norm2_host) ZK_HIP(hipMemcpyAsync(norm2_host + first, o + 2 * plane, w, hipMemcpyDeviceToHost, r->s_out));
        if (best_host) ZK_HIP(hipMemcpyAsync(best_host + first, o + 2 * plane + line, n * sizeof(int32_t), hipMemcpyDeviceToHost, r->s_out));
        return 0;
      });
}

// ------------------------------------------------------------------------------------------------------
// moments at key points: frame and point list go up once, the moments come down in chunks
// ------------------------------------------------------------------------------------------------------
extern "C" int zk_transform_points(zk_plan* p, const void* image_host, int dtype, int64_t H, int64_t W,
                                   const int32_t* points_host, int64_t n_points, double* out_host) {
  int rc = check_job(p, dtype, H, W, "point", n_points, image_host && points_host && out_host);
  if (rc) return rc < 0 ? rc : 0;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  int32_t* d_pts;
  if ((rc = frame_points_up(p, h, image_host, dtype, H, W, points_host, n_points, &d_pts))) return zk_ring_drain(r, p->stream, rc);
  const size_t out_unit = (size_t)p->n_poly * sizeof(double);
  const zk_chunks ch = zk_chunk_plan(chunk_bytes(p), out_unit, 256, n_points);
  return zk_ring_run(
      r, p->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int e = zk_ring_slot(r, slot, 0, (size_t)ch.chunk * out_unit);
        return e ? e : zk_transform_points_dev(p, h->d_frame, kernel_dtype(dtype), H, W, d_pts + 2 * ch.first(c), ch.count(c),
                                               (double*)r->d_out[slot], p->stream);
      },
      [&](int64_t c, int slot) -> int {
        return zk_ring_down(r, slot, (char*)out_host + (size_t)ch.first(c) * out_unit, (size_t)ch.count(c) * out_unit);
      });
}

// ------------------------------------------------------------------------------------------------------
// symmetry maps of a batch of moment vectors (rank-2 tail), and of the windows at key points (moments + tail fused:
// the (N, n_poly) matrix stays on the device)
// ------------------------------------------------------------------------------------------------------
extern "C" int zk_moment_maps(zk_plan* p, const double* moments_host, int64_t n_rows, const int32_t* folds, int n_folds,
                              const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta, int n_theta,
                              double* rot_host, double* abs_host, double* mirror_host) {
  int rc = check_job(p, ZK_F64, 1, 1, "row", n_rows, moments_host);
  if (rc) return rc < 0 ? rc : 0;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  const maps_out o(p, rot_host, abs_host, mirror_host, n_folds);
  const size_t in_unit = (size_t)p->n_poly * 8, out_unit = o.unit_bytes();
  const zk_chunks ch = zk_chunk_plan(chunk_bytes(p), in_unit + out_unit, 256, n_rows);
  return zk_ring_run(
      r, p->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int64_t n = ch.count(c);
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, (size_t)ch.chunk * out_unit);
        if (!e) e = zk_ring_up(r, p->stream, c, slot, r->d_in[slot], moments_host + (size_t)ch.first(c) * p->n_poly, (size_t)n * in_unit);
        void* d = r->d_out[slot];
        return e ? e : zk_moment_maps_dev(p, (const double*)r->d_in[slot], n, folds, n_folds, m_unselect, n_unselect, p_norm, theta,
                                          n_theta, o.d_rot(d, n), o.d_abs(d, n), o.d_mir(d, n), p->stream);
      },
      [&](int64_t c, int slot) -> int { return o.rows_to_host(r->d_out[slot], ch.first(c), ch.count(c), r->s_out); });
}

extern "C" int zk_points_maps(zk_plan* p, const void* image_host, int dtype, int64_t H, int64_t W, const int32_t* points_host,
                              int64_t n_points, const int32_t* folds, int n_folds, const int32_t* m_unselect, int n_unselect,
                              int p_norm, const double* theta, int n_theta, double* rot_host, double* abs_host,
                              double* mirror_host) {
  int rc = check_job(p, dtype, H, W, "point", n_points, image_host && points_host);
  if (rc) return rc < 0 ? rc : 0;
  ZK_ON_PLAN_DEVICE(p);
  zk_host_ring* h;
  if ((rc = ring_get(p, &h))) return rc;
  zk_ring* r = &h->stage.ring;
  int32_t* d_pts;
  if ((rc = frame_points_up(p, h, image_host, dtype, H, W, points_host, n_points, &d_pts))) return zk_ring_drain(r, p->stream, rc);
  const maps_out o(p, rot_host, abs_host, mirror_host, n_folds);
  const size_t mom_unit = (size_t)p->n_poly * 8, out_unit = o.unit_bytes();
  const zk_chunks ch = zk_chunk_plan(chunk_bytes(p), mom_unit + out_unit, 256, n_points);
  return zk_ring_run(
      r, p->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        const int64_t n = ch.count(c);
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * mom_unit, (size_t)ch.chunk * out_unit);  // d_in: the chunk's moments, device only
        double* mom = (double*)r->d_in[slot];
        void* d = r->d_out[slot];
        if (!e) e = zk_transform_points_dev(p, h->d_frame, kernel_dtype(dtype), H, W, d_pts + 2 * ch.first(c), n, mom, p->stream);
        return e ? e : zk_moment_maps_dev(p, mom, n, folds, n_folds, m_unselect, n_unselect, p_norm, theta, n_theta, o.d_rot(d, n),
                                          o.d_abs(d, n), o.d_mir(d, n), p->stream);
      },
      [&](int64_t c, int slot) -> int { return o.rows_to_host(r->d_out[slot], ch.first(c), ch.count(c), r->s_out); });
}
