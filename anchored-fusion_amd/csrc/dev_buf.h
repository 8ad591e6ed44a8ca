// dev_buf.h -- the owner of the library's device buffers (host code only).
// A DevBuf<T> is a device pointer and its element count: move-only, freed with hipFree by its
// destructor (hipFree's implicit device synchronisation included).  After a failed allocation the
// buffer is empty (null, size 0), so its size never exceeds what is allocated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

// the untyped part: pointer, element count and element size
class DevMem {
  public:
    explicit DevMem(size_t elem) : elem_(elem) {}
    DevMem(DevMem &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)), elem_(o.elem_) {}
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { reset(); }

    int64_t size() const { return n_; }  // elements
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // frees the buffer and allocates n elements
    hipError_t alloc(int64_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, elem_ * (size_t)n);
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }
    // nothing when need <= size(); else frees the buffer and allocates max(need, floor) elements
    hipError_t grow(int64_t need, int64_t floor = 0) { return need <= n_ ? hipSuccess : alloc(std::max(need, floor)); }
    // grow() for counters: a new allocation is zero-filled (the kernels keep them zero between calls)
    hipError_t grow_zeroed(int64_t need, int64_t floor = 0) {
        if (need <= n_) return hipSuccess;
        hipError_t e = alloc(std::max(need, floor));
        if (e == hipSuccess && (e = hipMemset(p_, 0, elem_ * (size_t)n_)) != hipSuccess) reset();
        return e;
    }

  protected:
    void *p_ = nullptr;
    int64_t n_ = 0;
    size_t elem_;
};

template <class T>
class DevBuf : public DevMem {
  public:
    DevBuf() : DevMem(sizeof(T)) {}
    DevBuf(DevBuf &&) noexcept = default;
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }  // stands where a kernel argument or a view wants the pointer
};

// Buffers that share one capacity are reallocated together and fail as a unit: after a failure
// every buffer of the group is empty, so the size of any one of them stands for the group.
//   dev_alloc_all({{a, n}, {b, 2 * n}})
struct DevWant {
    DevMem &buf;
    int64_t n;
};
inline hipError_t dev_alloc_all(std::initializer_list<DevWant> group) {
    for (const DevWant &w : group) {
        const hipError_t e = w.buf.alloc(w.n);
        if (e == hipSuccess) continue;
        for (const DevWant &x : group) x.buf.reset();
        return e;
    }
    return hipSuccess;
}

// The buffers an index owns for its whole life (bytes each), freed with the list.
using DevBufList = std::vector<DevBuf<uint8_t>>;
template <class T>
hipError_t dev_list_alloc(DevBufList &owned, size_t bytes, T **out) {
    DevBuf<uint8_t> b;
    const hipError_t e = b.alloc((int64_t)bytes);
    if (e != hipSuccess) return e;
    *out = reinterpret_cast<T *>(b.get());
    owned.push_back(std::move(b));
    return hipSuccess;
}
