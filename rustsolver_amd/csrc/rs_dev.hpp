// rs_dev.hpp -- owners of device memory and HIP handles.  The library allocates and frees device memory here and nowhere else (rs_dmalloc / rs_dfree
// aside: they hand raw memory to the caller).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <utility>

namespace rs {

inline std::atomic<size_t> g_dev_held{0};            // bytes every DevBuf of the process holds (rs_device_held_bytes)
inline std::atomic<long long> g_dev_fail_after{-1};  // test hook (rs_debug_fail_alloc): allocations granted before the next one is refused; < 0: off

// One device allocation of n T's, move-only, freed by its destructor.  It is charged to g_dev_held and, when alloc is given one, to the owning object's ledger;
// freeing takes it off both, so a ledger always equals what its object holds.  Converts to T* so that it reads like the pointer it owns; whatever aliases it
// stays a plain (non-owning) pointer.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), ledger_(std::exchange(o.ledger_, nullptr)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
            ledger_ = std::exchange(o.ledger_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // frees what it held, then allocates max(n, 1) elements.  A failed hipMalloc leaves it empty and clears HIP's last error, so that a later launch
    // check does not report it again.
    hipError_t alloc(size_t n, size_t *ledger = nullptr) {
        reset();
        long long k = g_dev_fail_after.load();
        while (k >= 0 && !g_dev_fail_after.compare_exchange_weak(k, k - 1)) {}
        if (k == 0) return hipErrorOutOfMemory;   // refused by the test hook: nothing reaches the device
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        p_ = static_cast<T *>(p);
        bytes_ = bytes;
        ledger_ = ledger;
        g_dev_held += bytes;
        if (ledger_) *ledger_ += bytes;
        return hipSuccess;
    }
    void reset() {
        if (!p_) return;
        (void)hipFree(p_);
        g_dev_held -= bytes_;
        if (ledger_) *ledger_ -= bytes_;
        p_ = nullptr;
        bytes_ = 0;
        ledger_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t bytes() const { return bytes_; }

  private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
    size_t *ledger_ = nullptr;
};

// a HIP stream, event or graph handle, destroyed with its owner
template <class H, hipError_t (*Destroy)(H)>
class DevHandle {
  public:
    DevHandle() = default;
    DevHandle(const DevHandle &) = delete;
    DevHandle &operator=(const DevHandle &) = delete;
    DevHandle(DevHandle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    DevHandle &operator=(DevHandle &&o) noexcept {
        if (this != &o) reset(std::exchange(o.h_, nullptr));
        return *this;
    }
    ~DevHandle() { reset(); }

    void reset(H h = nullptr) {
        if (h_) (void)Destroy(h_);
        h_ = h;
    }
    H *put() {   // the out-parameter of the create call
        reset();
        return &h_;
    }
    H get() const { return h_; }
    operator H() const { return h_; }

  private:
    H h_ = nullptr;
};

using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevGraph = DevHandle<hipGraph_t, hipGraphDestroy>;
using DevGraphExec = DevHandle<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace rs
