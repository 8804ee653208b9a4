// Stand-in for <hip/hip_runtime.h> on the CPU: the four calls csrc/dev_mem.h makes, backed by malloc / free / memcpy, counted,
// with every requested size logged (tests/cpp/dev_mem_cases.cpp).  fake_hip::fail_next_malloc makes the next hipMalloc fail.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyDeviceToDevice = 3 };

namespace fake_hip {
inline int mallocs = 0, frees = 0, copies = 0, syncs = 0;
inline bool fail_next_malloc = false;
inline std::vector<size_t> sizes;  // what every hipMalloc was asked for
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) {
  fake_hip::sizes.push_back(bytes);
  if (fake_hip::fail_next_malloc) {
    fake_hip::fail_next_malloc = false;
    return hipErrorOutOfMemory;
  }
  ++fake_hip::mallocs;
  *p = std::malloc(bytes);
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  ++fake_hip::frees;
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  ++fake_hip::copies;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  ++fake_hip::syncs;
  return hipSuccess;
}
