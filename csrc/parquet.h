// What parquet.hip shares with the module's bindings in kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

// "This group is decoded": the event pq_decode_group records on the decode
// stream after the group's kernels.  Python holds it as an opaque handle.
struct PqDone {
  hipEvent_t ev;
  int device;

  explicit PqDone(int device);
  ~PqDone();
  PqDone(const PqDone&) = delete;
  PqDone& operator=(const PqDone&) = delete;

  void synchronize();  // the host waits
  bool query();        // true once the group is decoded
};
