// What the host units of the C ABI (capi*.cpp) write out over and over. Host code only: no kernel unit and no other header includes this.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "common.hpp"

namespace dad3d {

template <typename T>
static dad3d_status upload(T** dst, const std::vector<T>& src) {
    *dst = nullptr;
    const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), bytes));
    if (!src.empty()) DAD3D_HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return DAD3D_OK;
}

inline void free_device(int device, std::initializer_list<void*> ptrs) {
    DeviceGuard guard(device);
    for (void* p : ptrs) (void)hipFree(p);
}

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
