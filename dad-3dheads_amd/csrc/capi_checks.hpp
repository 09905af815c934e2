// What the host units of the C ABI (capi*.cpp) write out over and over: the owners of device memory (device_memory.hpp), the device and
// batch checks, the capture test. Host code only: no kernel unit and no other header includes this.
#pragma once
#include <algorithm>
#include <cstddef>

#include "device_memory.hpp"
#include "plan_pods.hpp"

namespace dad3d {

// the host planners' vectors are uploaded as arrays of HIP's vector types (DeviceArray::upload)
static_assert(sizeof(plan::Int4) == sizeof(int4) && sizeof(plan::UInt2) == sizeof(uint2) && sizeof(plan::UInt4) == sizeof(uint4) &&
                  sizeof(plan::Float4) == sizeof(float4) && offsetof(plan::Float4, w) == offsetof(float4, w) &&
                  offsetof(plan::Int4, w) == offsetof(int4, w) && offsetof(plan::UInt2, y) == offsetof(uint2, y) &&
                  offsetof(plan::UInt4, w) == offsetof(uint4, w),
              "plan_pods.hpp: not the layout of HIP's vector types");

// `device` current until the end of the caller's scope, or the caller returns DAD3D_E_INVALID (a macro: DAD3D_REQUIRE returns from the caller)
#define DAD3D_SELECT_DEVICE(device) \
    DeviceGuard guard(device);      \
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", (device))

// the batch bound of the entry points that launch one grid row per file or image
#define DAD3D_REQUIRE_BATCH(who, batch) DAD3D_REQUIRE((batch) >= 1 && (batch) <= 65535, "%s: batch %d outside 1 .. 65535", who, (batch))

inline bool aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

inline bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (s != nullptr) (void)hipStreamIsCapturing(s, &capture);
    return capture != hipStreamCaptureStatusNone;
}

}  // namespace dad3d
