// zk_switches.h -- every environment switch of libzernike_hip, and the library's only getenv.
//
// Measurement aids and deployment settings; nothing here is needed to use the library.  A switch is read from the environment
// at its point of use, every time: setting or clearing one between two calls takes effect on the next call.  The ones marked
// "plan" / "comm" shape tables that are built once, so they are read when the plan / communicator is created and hold for
// its life.  A flag is on when the variable is set, whatever its value.  INTEGRATION.md section 7 lists the same table
// (tests/test_switches_cpu.py holds the two together).
#pragma once

#include <stdlib.h>

// X(name, kind, default, read, what it selects)
#define ZK_SWITCHES(X)                                                                                                                 \
  X(ZK_NO_STRIP, flag, off, call, "dense transform, n_max <= 12: the one-output kernel instead of the strip kernels")                  \
  X(ZK_STRIP_V3, flag, off, call, "strip kernel with the x table in VGPR lanes (even windows <= 32 px, n_max <= 8; same bits)")        \
  X(ZK_STRIP_NO_SPLIT, flag, off, call, "dense transform, n_max 9-12: the one-output kernel instead of the two-pass strip form")       \
  X(ZK_NO_DIRECT, flag, off, call, "ZK_PATH_AUTO never takes the matrix-core plain sum (n_max 17-24: separable; 25-40: generic)")      \
  X(ZK_NO_CONV_FLIP, flag, off, plan, "dense mode of the generic and direct kernels as the plain inner product, no flip + sign")       \
  X(ZK_DIRECT_CH96, flag, off, plan, "matrix-core plain sum in chunks of 96 functions instead of blocks of 16 dealt evenly")           \
  X(ZK_POINTS_NO_BUCKET, flag, off, call, "key points in the caller's order instead of bucket order (same bits)")                      \
  X(ZK_POINTS_NO_WIDE, flag, off, call, "key points: window pixels by 4-byte loads instead of rows of 16-byte loads (same bits)")      \
  X(ZK_ESTEP_VALU, flag, off, call, "mixture E step on the vector pipe (the kernel of D > 48 or k > 8) instead of the matrix cores")   \
  X(ZK_WGRAM_VALU, flag, off, call, "mixture M step: the register-tiled kernel (that of D > 47) instead of the matrix cores")          \
  X(ZK_KNN_SCALAR, integer, 0, call, "1: correlation kNN, k <= 16: the four-wave scalar-operand knn_kernel<16, 4>, no matrix cores")   \
  X(ZK_KNN_PARTS, integer, auto, call, "parts of the candidate range of the matrix-core kNN (1 .. 16; default by matrix size)")        \
  X(ZK_HOST_CHUNK_MB, integer, 256, call, "MiB of input + output per chunk of the host-buffer pipeline (a plan's own setting wins)")   \
  X(ZK_CLOCK_MONITOR_MODE, integer, 0, call, "zk_clock_monitor: the resident wave naps (0), spins (1) or does FP64 work (2)")          \
  X(ZK_COMM_ALGO, string, auto, comm, "p2p / allgather / bcast: force one form of zk_allgather_rows")                                  \
  X(ZK_COMM_BIND_ADDR, string, auto, comm, "address rank 0 of zk_comm_init_tcp listens on: an IPv4 literal, or any")

#define ZK_SWITCH_ID(name, kind, dflt, read, what) name,
#define ZK_SWITCH_NAME(name, kind, dflt, read, what) #name,
enum zk_switch { ZK_SWITCHES(ZK_SWITCH_ID) };
static const char* const zk_switch_names[] = {ZK_SWITCHES(ZK_SWITCH_NAME)};
#undef ZK_SWITCH_ID
#undef ZK_SWITCH_NAME

static inline const char* zk_switch_str(zk_switch s) { return getenv(zk_switch_names[s]); }  // nullptr when unset
static inline bool zk_switch_on(zk_switch s) { return zk_switch_str(s) != nullptr; }
static inline long zk_switch_int(zk_switch s, long unset) {
  const char* v = zk_switch_str(s);
  return v ? atol(v) : unset;
}
