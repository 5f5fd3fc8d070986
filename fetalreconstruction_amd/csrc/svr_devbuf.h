// DevBuf<T>: the one owner of a hipMalloc allocation (DESIGN.md "Who owns device memory").  Grow-only: reserve(n) keeps a block that holds
// n elements, otherwise frees it FIRST and then asks for exactly n * sizeof(T) bytes (no rounding, no geometric growth: the coefficient
// table and the cell staging size themselves by what hipMemGetInfo reports).  Contents are not kept across a growth; a failed growth
// leaves the buffer empty.  Never static or global: the destructor calls hipFree, which must not run after the runtime is gone.
// Uses nothing of HIP beyond hipMalloc / hipFree / hipError_t / hipSuccess (tests/devbuf_check.cpp supplies stand-ins for them).
#pragma once
#include <cstddef>
#include <type_traits>

template <class T>
class DevBuf {
  T *p_ = nullptr;
  size_t cap_ = 0;   // elements
  static constexpr size_t elem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);   // DevBuf<void>: bytes

 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  hipError_t reserve(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, n * elem);
    if (e != hipSuccess) return e;
    p_ = static_cast<T *>(q);
    cap_ = n;
    return hipSuccess;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  size_t capacity() const { return cap_; }
  T *get() const { return p_; }
  operator T *() const { return p_; }
};
