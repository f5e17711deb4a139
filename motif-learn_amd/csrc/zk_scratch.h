// zk_scratch.h -- host-side scratch helpers of the translation units that own their device memory per call: a device buffer
// freed with its scope (dev_buf), which is also how a host-array entry point takes its operands up and its results down
// (upload / download), the error word of a call (dev_flag), the block count of a launch, and rocPRIM's temporary storage
// with the one way to call an algorithm that needs it.
#pragma once

#include <rocprim/device/device_scan.hpp>

#include "zk_internal.h"

// device memory that goes with its scope
struct dev_buf {
  void* p = nullptr;
  ~dev_buf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    ZK_HIP(hipMalloc(&p, bytes ? bytes : 16));
    return 0;
  }
  // The copies of the host-array entry points: pageable memory, blocking, on the null stream (these calls are not the hot
  // path).  A null `host` is an operand the caller did not pass -- p stays null, and as<T>() is the nullptr the device
  // body expects for it -- or a result the caller does not want.
  int upload(const void* host, size_t bytes) {
    if (!host) return 0;
    int rc;
    if ((rc = alloc(bytes))) return rc;
    ZK_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return 0;
  }
  int download(void* host, size_t bytes) const {
    if (host) ZK_HIP(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  void* release() {                                  // the pointer is the caller's from here on
    void* q = p;
    p = nullptr;
    return q;
  }
  template <typename T>
  T* as() const {
    return (T*)p;
  }
};

// the error word of one call: kernels raise bits in it with atomicOr, the host reads it once, at the call's one synchronise
struct dev_flag {
  dev_buf buf;
  int* word() const { return buf.as<int>(); }
  int arm(hipStream_t s) {                           // allocated and zeroed
    int rc;
    if ((rc = buf.alloc(16))) return rc;
    ZK_HIP(hipMemsetAsync(buf.p, 0, 16, s));
    return 0;
  }
  int read(hipStream_t s, int* flags) {              // everything queued on `s` before this has finished when it returns
    *flags = 0;
    ZK_HIP(hipMemcpyAsync(flags, buf.p, sizeof(int), hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return 0;
  }
};

static inline unsigned blocks_of(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// rocPRIM's temporary storage, grown to the largest request of the call
struct temp_store {
  void* p = nullptr;
  size_t have = 0;
  ~temp_store() {
    if (p) (void)hipFree(p);
  }
  int ensure(size_t need) { return zk_ensure(&p, &have, need ? need : 16); }
};

// A rocPRIM algorithm is called twice with the same arguments: without storage it reports the bytes it needs, with storage it
// runs.  `call(void* storage, size_t& bytes) -> hipError_t` holds the one argument list; zk_prim_bytes asks, zk_prim asks,
// grows the store and runs.
template <class Call>
int zk_prim_bytes(size_t* bytes, Call call) {
  *bytes = 0;
  ZK_HIP(call(nullptr, *bytes));
  return 0;
}

template <class Call>
int zk_prim(temp_store& tmp, Call call) {
  size_t bytes = 0;
  int rc;
  if ((rc = zk_prim_bytes(&bytes, call)) || (rc = tmp.ensure(bytes))) return rc;
  ZK_HIP(call(tmp.p, bytes));
  return 0;
}

template <typename T>
int exclusive_sum(temp_store& tmp, const T* in, T* out, size_t n, hipStream_t s) {
  return zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::exclusive_scan(p, b, in, out, (T)0, n, rocprim::plus<T>(), s); });
}
