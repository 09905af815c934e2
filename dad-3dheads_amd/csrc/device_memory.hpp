// Who owns device memory behind the C ABI: DeviceArray (one allocation) and DeviceScratch (a buffer that only grows). Every device member
// of a handle is one of the two, so a handle's destructor is the compiler's. Host code only: capi_checks.hpp includes this, nothing else does.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.hpp"

namespace dad3d {

// One hipMalloc. Move-only; remembers the device that was current when it allocated and frees there.
template <typename T>
class DeviceArray {
    T* p_ = nullptr;
    int device_ = 0;

public:
    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), device_(o.device_) {}
    DeviceArray& operator=(DeviceArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr), device_ = o.device_;
        }
        return *this;
    }
    ~DeviceArray() { reset(); }

    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (!p_) return;
        DeviceGuard guard(device_);
        (void)hipFree(p_);
        p_ = nullptr;
    }
    // `count` elements on the current device, uninitialised; what it held before is freed first
    dad3d_status allocate(size_t count) {
        reset();
        (void)hipGetDevice(&device_);
        DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T)));
        return DAD3D_OK;
    }
    // A host vector's copy; at least one element is allocated (an empty table is still an address a kernel may be handed). U: T itself or
    // the host planners' plain twin of a HIP vector type
    template <typename U>
    dad3d_status upload(const std::vector<U>& src) {
        static_assert(sizeof(U) == sizeof(T) && std::is_trivially_copyable<U>::value, "upload: the host element is not T's layout");
        if (dad3d_status st = allocate(std::max<size_t>(src.size(), 1))) return st;
        if (!src.empty()) DAD3D_HIP_TRY(hipMemcpy(p_, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
        return DAD3D_OK;
    }
};

// A scratch buffer that only grows. Memory comes from allocate() or grow(), nothing else; after a failure it is empty with capacity 0.
class DeviceScratch {
    DeviceArray<char> buf_;
    size_t bytes_ = 0;

public:
    void* get() const { return buf_.get(); }
    size_t capacity() const { return bytes_; }
    // on an empty buffer; no synchronisation: nothing can be using what does not exist
    dad3d_status allocate(size_t bytes) {
        bytes_ = 0;
        if (dad3d_status st = buf_.allocate(bytes)) return st;
        bytes_ = bytes;
        return DAD3D_OK;
    }
    // at least `bytes`; a larger buffer replaces the old one once the device is idle (a launch in flight may still use it). Contents are lost.
    dad3d_status grow(size_t bytes) {
        if (bytes <= bytes_) return DAD3D_OK;
        DAD3D_HIP_TRY(hipDeviceSynchronize());
        buf_.reset();
        return allocate(bytes);
    }
    // hands the buffer over and leaves the scratch empty: for an owner that must keep outgrown memory alive
    DeviceArray<char> retire() {
        bytes_ = 0;
        return std::move(buf_);
    }
};

}  // namespace dad3d
