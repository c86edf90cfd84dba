// svo_grow.h -- the one routine that grows a family of per-set device buffers (host code): the persistent pipeline's counter-set
// buffers (svo_persistent.hip.h) and the beam pass's images (svo_beam.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace svo {

// Grows a family of equally sized device buffers to `bytes` each: nothing in flight may still use the old ones, so the device is
// waited for; then all are freed, `have` (and their in-use flags, if they have any) cleared, and all allocated anew.  `have`
// becomes `want` only behind the last allocation: a failed grow leaves nothing half-sized, and the next launch grows again.
template <class T, size_t N>
inline hipError_t grow_device_buffers(T *(&bufs)[N], bool *used, size_t &have, size_t want, size_t bytes) {
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
  for (size_t i = 0; i < N; i++) {
    if (bufs[i]) (void)hipFree(bufs[i]);
    bufs[i] = nullptr;
    if (used) used[i] = false;
  }
  have = 0;
  for (size_t i = 0; i < N; i++)
    if ((e = hipMalloc((void **)&bufs[i], bytes)) != hipSuccess) return e;
  have = want;
  return hipSuccess;
}

}  // namespace svo
