// Host side of every .hip file: the one HIP error check and the one way to
// the current stream.
#pragma once

#include <c10/hip/HIPStream.h>
#include <c10/util/Exception.h>
#include <hip/hip_runtime.h>

#define CHECK_HIP(x)                                                    \
  do {                                                                  \
    hipError_t e = (x);                                                 \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e));  \
  } while (0)

inline hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// the error of the launches before it, under the entry point's name
inline void check_launch(const char* who) {
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, who, ": ", hipGetErrorString(e));
}
