// Host-side owners of HIP resources: the device check, the current-device scope, one device allocation, one stream.
// Every other file of the library takes its device memory, its streams and its current device through these (the pinned
// blocks with a device alias, Arena and HostBuf, keep their own rules).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gecco_crf.h"
#include "crf_model.hpp"

namespace gecco {

int check_hip(hipError_t e, const char *what);  // crf_plan.cpp: GECCO_CRF_* of a HIP status, with the error text set

// Is there a device `device`?  The one copy of the two ENODEV refusals; entries call it after their argument checks.
inline int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return GECCO_CRF_ENODEV;
    }
    if (device < 0 || device >= n) {
        set_error("device index out of range");
        return GECCO_CRF_ENODEV;
    }
    return GECCO_CRF_OK;
}

inline int set_device(int device) { return check_hip(hipSetDevice(device), "hipSetDevice"); }

// hipSetDevice only when the calling thread is on another device (the C ABI's scope restores the caller's device afterwards):
// a launch-bound step used to make four runtime calls for this
inline int use_device(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return GECCO_CRF_OK;
    return set_device(device);
}

// Restores the caller's current device on every way out: only if the save succeeded, and only if the current device differs
// from the saved one by then.  DeviceScope() saves at once (the C entries); DeviceScope(device) also makes `device` current.
// An owner of device memory keeps a DeviceScope(DeviceScope::kLater) as its FIRST member and calls enter(device) in its
// destructor: the members after it then free themselves with the owner's device current, and the scope, destroyed last,
// hands the caller's device back.  enter() of a negative device (an owner that never reached a device) makes no HIP call.
class DeviceScope {
    int prev_ = -1;

public:
    enum Later { kLater };
    DeviceScope() { save(); }
    explicit DeviceScope(int device) { enter(device); }
    explicit DeviceScope(Later) {}
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    ~DeviceScope() {
        int cur = -1;
        if (prev_ >= 0 && (hipGetDevice(&cur) != hipSuccess || cur != prev_)) (void)hipSetDevice(prev_);
    }
    void save() {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    }
    void enter(int device) {
        if (device < 0) return;
        save();
        (void)hipSetDevice(device);
    }
};

// One hipMalloc block, freed with its owner.  The device that it was allocated on must be current when it is freed.
template <class T>
class DeviceBlock {
    T *p_ = nullptr;
    size_t cap_ = 0;  // bytes that reserve() keeps; 0 for a block of alloc() / upload()

public:
    DeviceBlock() = default;
    DeviceBlock(DeviceBlock &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DeviceBlock &operator=(DeviceBlock &&o) noexcept {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DeviceBlock() { release(); }

    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    template <class U>
    U *at(size_t byte_offset) const {
        return reinterpret_cast<U *>(reinterpret_cast<char *>(p_) + byte_offset);
    }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // max(n, 1) elements, so that the pointer is a device pointer either way; a block held before is freed first
    int alloc(size_t n, const char *what) {
        release();
        int rc = check_hip(hipMalloc(reinterpret_cast<void **>(&p_), std::max<size_t>(n, 1) * sizeof(T)), what);
        if (rc) p_ = nullptr;
        return rc;
    }
    // alloc(n) and a synchronous copy of src[0, n) (none for n == 0 or a null src)
    int upload(const T *src, size_t n, const char *what) {
        int rc = alloc(n, what);
        if (rc || !src || n == 0) return rc;
        return check_hip(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice), what);
    }
    int upload(const std::vector<T> &h, const char *what) { return upload(h.data(), h.size(), what); }
    // ... the copy asynchronous on `stream`: src stays alive and unchanged until the stream has passed it
    int upload(const T *src, size_t n, const char *what, hipStream_t stream) {
        int rc = alloc(n, what);
        if (rc || !src || n == 0) return rc;
        return check_hip(hipMemcpyAsync(p_, src, n * sizeof(T), hipMemcpyHostToDevice, stream), what);
    }
    // Grow-only work space of at least `bytes`: a block that is too small is freed first (hipFree waits for the launches that
    // may still use it), and the new one keeps bytes + bytes / 8 + 256, since the chunks of one batch differ a little.
    int reserve(size_t bytes, const char *what) {
        if (p_ && bytes <= cap_) return GECCO_CRF_OK;
        release();
        const size_t want = bytes + bytes / 8 + 256;
        int rc = check_hip(hipMalloc(reinterpret_cast<void **>(&p_), want), what);
        if (rc) p_ = nullptr;
        else cap_ = want;
        return rc;
    }
};
static_assert(!std::is_copy_constructible<DeviceBlock<char>>::value && !std::is_copy_assignable<DeviceBlock<char>>::value,
              "a device block has one owner");

// One non-blocking stream, created on the current device and destroyed with its owner.  Declare it BEFORE the blocks that
// its work uses: members go in reverse order, so the blocks are freed (hipFree waits) before the stream is destroyed.
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipStream_t get() const { return s_; }
    int create() { return s_ ? GECCO_CRF_OK : check_hip(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), "hipStreamCreate"); }
};

}  // namespace gecco
