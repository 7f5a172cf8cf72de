// devbuf.hpp -- the owner of one device allocation.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

namespace rwkvmi {

// Owns one hipMalloc allocation of size() elements of T: move-only, freed by the destructor and by
// reset().  It converts to T *, so it stands wherever the raw pointer stood (pointer arithmetic,
// argument structs, launch_* calls); a kernel launch, which would copy it, takes get().  No stream
// and no growth policy: who may free a buffer that queued work or a captured graph still points at
// is the caller's business (Engine::grow).
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf && o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf & operator=(DevBuf && o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    // Frees what it holds, then allocates n elements and the 64 bytes of slack that the kernels'
    // whole-vector loads of a last partial row may touch.  On failure the buffer is empty and HIP's
    // sticky error is cleared: the next launch checks hipGetLastError() for faults of its own.
    bool alloc(size_t n) {
        reset();
        if (hipMalloc((void **)&p_, n * sizeof(T) + 64) != hipSuccess) {
            p_ = nullptr;
            (void)hipGetLastError();
            return false;
        }
        n_ = n;
        return true;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T * get() const { return p_; }
    size_t size() const { return n_; }
    operator T *() const { return p_; }

  private:
    T * p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace rwkvmi
