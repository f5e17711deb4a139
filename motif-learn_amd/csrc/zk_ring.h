// zk_ring.h -- the staging of the NumPy-in / NumPy-out calls, for every unit that has them (zk_host, zk_synth, zk_align,
// zk_resample, zk_register, zk_strain): the ring and its protocol, and zk_stage, the state a unit keeps for it -- its kernel
// stream, the ring, and how much of the ring stays on the device between calls.
//
// A job is cut into chunks of at most `budget` bytes of input + output (default 256 MiB); chunk c goes
//     H2D on the ring's copy-in stream  ->  kernel on the caller's stream  ->  D2H on the ring's copy-out stream
// through one of ZK_RING_SLOTS device slots, consecutive chunks overlapping (events order the three streams;
// the host only waits when it needs a slot back).  The device footprint is the ring (<= 3 chunks), whatever
// the job size: a 4096^2 frame at n_max 10 needs 0.8 GB of staging instead of the 9 GB result.
//
// Host memory: copies straight from / into the caller's arrays.  Page-locked arrays (zk_host_alloc -- the
// Python layer hands its results out of a pool of them -- or anything hipHostRegister'ed) move by DMA at
// link speed and fully asynchronously; pageable arrays go through the runtime's own staging, which blocks
// the calling thread per copy (the kernel of the chunk before still overlaps with it).
#pragma once

#include <mutex>

#include "zk_internal.h"

#define ZK_RING_SLOTS 3

struct zk_ring {
  void* d_in[ZK_RING_SLOTS] = {};
  size_t in_cap[ZK_RING_SLOTS] = {};
  void* d_out[ZK_RING_SLOTS] = {};
  size_t out_cap[ZK_RING_SLOTS] = {};
  hipEvent_t ev_in[ZK_RING_SLOTS] = {};    // H2D of the slot's chunk done
  hipEvent_t ev_k[ZK_RING_SLOTS] = {};     // kernel of the slot's chunk done
  hipEvent_t ev_out[ZK_RING_SLOTS] = {};   // D2H of the slot's chunk done
  bool out_busy[ZK_RING_SLOTS] = {};
  hipStream_t s_in = nullptr, s_out = nullptr;
};

static inline int zk_ring_create(zk_ring* r) {
  ZK_HIP(hipStreamCreateWithFlags(&r->s_in, hipStreamNonBlocking));
  ZK_HIP(hipStreamCreateWithFlags(&r->s_out, hipStreamNonBlocking));
  for (int k = 0; k < ZK_RING_SLOTS; ++k) {
    ZK_HIP(hipEventCreateWithFlags(&r->ev_in[k], hipEventDisableTiming));
    ZK_HIP(hipEventCreateWithFlags(&r->ev_k[k], hipEventDisableTiming));
    ZK_HIP(hipEventCreateWithFlags(&r->ev_out[k], hipEventDisableTiming));
  }
  return 0;
}

static inline size_t zk_ring_bytes(const zk_ring* r) {
  size_t held = 0;
  for (int k = 0; k < ZK_RING_SLOTS; ++k) held += r->in_cap[k] + r->out_cap[k];
  return held;
}

// the device slots go back (zk_ring_slot re-creates them on demand); no job may be in flight
static inline void zk_ring_free_slots(zk_ring* r) {
  for (int k = 0; k < ZK_RING_SLOTS; ++k) {
    if (r->d_in[k]) (void)hipFree(r->d_in[k]);
    if (r->d_out[k]) (void)hipFree(r->d_out[k]);
    r->d_in[k] = r->d_out[k] = nullptr;
    r->in_cap[k] = r->out_cap[k] = 0;
  }
}

// takes a ring in any state of a failed zk_ring_create as well
static inline void zk_ring_destroy(zk_ring* r) {
  if (r->s_in) (void)hipStreamSynchronize(r->s_in);
  if (r->s_out) (void)hipStreamSynchronize(r->s_out);
  zk_ring_free_slots(r);
  for (int k = 0; k < ZK_RING_SLOTS; ++k) {
    if (r->ev_in[k]) (void)hipEventDestroy(r->ev_in[k]);
    if (r->ev_k[k]) (void)hipEventDestroy(r->ev_k[k]);
    if (r->ev_out[k]) (void)hipEventDestroy(r->ev_out[k]);
  }
  if (r->s_in) (void)hipStreamDestroy(r->s_in);
  if (r->s_out) (void)hipStreamDestroy(r->s_out);
  *r = zk_ring();
}

// The staging state of a unit's host-buffer entry points: the stream their kernels run on and the ring.  A plan lends its own
// stream (`kernel`); every other owner (a synthesis object, the per-device state of zk_align / zk_resample / zk_register /
// zk_strain) has the stage make a non-blocking one, which then goes with it.
struct zk_stage {
  hipStream_t stream = nullptr;
  bool own_stream = false, made = false;
  zk_ring ring;
};

static inline void zk_stage_destroy(zk_stage* st) {
  zk_ring_destroy(&st->ring);
  if (st->own_stream && st->stream) (void)hipStreamDestroy(st->stream);
  *st = zk_stage();
}

// the stream, then the ring; nothing on a stage that is made already, and nothing is left of one that could not be
static inline int zk_stage_create(zk_stage* st, hipStream_t kernel = nullptr) {
  if (st->made) return 0;
  st->stream = kernel;
  st->own_stream = !kernel;
  if (!kernel) ZK_HIP(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
  const int rc = zk_ring_create(&st->ring);
  if (rc) {
    zk_stage_destroy(st);
    return rc;
  }
  st->made = true;
  return 0;
}

// a unit whose host entry points take a device index keeps a table of these: a stage per device, made at the first call there
// and kept, one call at a time
struct zk_device_stage {
  std::mutex lock;
  zk_stage stage;
};

// What a stage keeps on the device between calls: slots of up to `keep_bytes` stay (repeated small calls allocate nothing), the
// slots of a larger job, up to three chunks, go back at once.  No job may be in flight.
constexpr size_t ZK_STAGE_KEEP_STACKS = (size_t)64 << 20;  // per device: zk_resample, zk_register, zk_strain
constexpr size_t ZK_STAGE_KEEP_ROWS = (size_t)32 << 20;    // zk_align, and per object in zk_synth: callers hold several at a time

static inline void zk_stage_trim(zk_stage* st, size_t keep_bytes) {
  if (zk_ring_bytes(&st->ring) > keep_bytes) zk_ring_free_slots(&st->ring);
}

// The chunks of a job of n units (patches, points, rows) of `unit` bytes each, input + output: as many units as the budget
// holds, rounded down to whole grains (a power of two: what a block of the job's kernel takes), at least one grain, at most n.
struct zk_chunks {
  int64_t n, chunk, n_chunks;
  int64_t first(int64_t c) const { return c * chunk; }
  int64_t count(int64_t c) const { return n - c * chunk < chunk ? n - c * chunk : chunk; }
};

static inline zk_chunks zk_chunk_plan(size_t budget, size_t unit, int64_t grain, int64_t n) {
  int64_t chunk = (int64_t)(budget / unit) & ~(grain - 1);
  if (chunk < grain) chunk = grain;
  if (chunk > n) chunk = n;
  return {n, chunk, (n + chunk - 1) / chunk};
}

// wait until every copy of the job has landed, whatever happened before; `kernel` is the stream the job's kernels ran on
static inline int zk_ring_drain(zk_ring* r, hipStream_t kernel, int rc) {
  const hipError_t a = hipStreamSynchronize(r->s_in), b = hipStreamSynchronize(kernel), c = hipStreamSynchronize(r->s_out);
  for (int k = 0; k < ZK_RING_SLOTS; ++k) r->out_busy[k] = false;
  if (rc) return rc;
  if (a != hipSuccess) return zk_hip_fail(a, "hipStreamSynchronize(copy-in)");
  if (b != hipSuccess) return zk_hip_fail(b, "hipStreamSynchronize(kernel)");
  if (c != hipSuccess) return zk_hip_fail(c, "hipStreamSynchronize(copy-out)");
  return 0;
}

// the slot is about to be reused: its previous D2H must have left d_out (the host waits); then its kernels are enqueued
template <class L>
static inline int zk_ring_chunk_in(zk_ring* r, hipStream_t kernel, int64_t c, L& launch) {
  const int slot = (int)(c % ZK_RING_SLOTS);
  if (r->out_busy[slot]) {
    ZK_HIP(hipEventSynchronize(r->ev_out[slot]));
    r->out_busy[slot] = false;
  }
  const int e = launch(c, slot);
  if (e) return e;
  ZK_HIP(hipEventRecord(r->ev_k[slot], kernel));
  return 0;
}

// kernel done, bytes down, slot busy
template <class O>
static inline int zk_ring_chunk_out(zk_ring* r, int64_t c, O& copy_out) {
  const int slot = (int)(c % ZK_RING_SLOTS);
  ZK_HIP(hipStreamWaitEvent(r->s_out, r->ev_k[slot], 0));
  const int e = copy_out(c, slot);
  if (e) return e;
  ZK_HIP(hipEventRecord(r->ev_out[slot], r->s_out));
  r->out_busy[slot] = true;
  return 0;
}

// Software pipeline over the chunks of a job: chunk c is staged in and its kernel enqueued BEFORE the copy-out
// of chunk c-1 is issued, so that a copy that blocks the calling thread (pageable memory) still runs under the
// kernel of the next chunk.  `launch(c, slot)` sizes the slot (zk_ring_slot), brings the chunk's input up (zk_ring_up) and
// enqueues its kernels on `kernel`; `copy_out(c, slot)` enqueues the chunk's downloads on r->s_out (zk_ring_down).  Both
// return 0 or a negative code; the streams are drained before returning, whatever happened.
template <class L, class O>
static inline int zk_ring_run(zk_ring* r, hipStream_t kernel, int64_t n_chunks, L launch, O copy_out) {
  int rc = 0;
  for (int64_t c = 0; c <= n_chunks && !rc; ++c) {
    if (c < n_chunks) rc = zk_ring_chunk_in(r, kernel, c, launch);
    if (c > 0 && !rc) rc = zk_ring_chunk_out(r, c - 1, copy_out);
  }
  return zk_ring_drain(r, kernel, rc);
}

// room in the slot for a chunk's input and output (0 bytes: that side is not used)
static inline int zk_ring_slot(zk_ring* r, int slot, size_t in_bytes, size_t out_bytes) {
  const int e = zk_ensure(&r->d_in[slot], &r->in_cap[slot], in_bytes);
  return e ? e : zk_ensure(&r->d_out[slot], &r->out_cap[slot], out_bytes);
}

// bytes up into the slot (dst: its d_in, or another landing buffer of the caller's per slot), then the kernel may start
static inline int zk_ring_up(zk_ring* r, hipStream_t kernel, int64_t c, int slot, void* dst, const void* src, size_t bytes) {
  // the slot's previous kernels must have consumed the landing buffer before the next H2D overwrites it
  if (c >= ZK_RING_SLOTS) ZK_HIP(hipStreamWaitEvent(r->s_in, r->ev_k[slot], 0));
  ZK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, r->s_in));
  ZK_HIP(hipEventRecord(r->ev_in[slot], r->s_in));
  ZK_HIP(hipStreamWaitEvent(kernel, r->ev_in[slot], 0));
  return 0;
}

// as zk_ring_up for `rows` pieces of `width` bytes each, `spitch` bytes apart on the host and `dpitch` in the slot
static inline int zk_ring_up_2d(zk_ring* r, hipStream_t kernel, int64_t c, int slot, void* dst, size_t dpitch, const void* src, size_t spitch,
                                size_t width, size_t rows) {
  if (c >= ZK_RING_SLOTS) ZK_HIP(hipStreamWaitEvent(r->s_in, r->ev_k[slot], 0));
  ZK_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, r->s_in));
  ZK_HIP(hipEventRecord(r->ev_in[slot], r->s_in));
  ZK_HIP(hipStreamWaitEvent(kernel, r->ev_in[slot], 0));
  return 0;
}

// the slot's d_out down in one piece
static inline int zk_ring_down(zk_ring* r, int slot, void* dst, size_t bytes) {
  ZK_HIP(hipMemcpyAsync(dst, r->d_out[slot], bytes, hipMemcpyDeviceToHost, r->s_out));
  return 0;
}
