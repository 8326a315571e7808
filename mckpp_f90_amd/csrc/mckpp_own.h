// mckpp_own.h - move-only owners of the HIP resources of the host runtime (mckpp_runtime.cpp): device blocks, pinned
// host blocks, events, streams.  Host code only.
//
// An owner never synchronises and never reports an error from its destructor: whoever drops a buffer that queued work
// may still use waits first, at the call site.  (The one wait in this file is pinned_turns::take, which is that type's
// purpose.)
#ifndef MCKPP_OWN_H
#define MCKPP_OWN_H

#include <hip/hip_runtime.h>

// a hipMalloc block of n elements
template <class T>
class dev_buf {
  T *p_ = nullptr;
  size_t n_ = 0;
 public:
  dev_buf() = default;
  dev_buf(dev_buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  dev_buf &operator=(dev_buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  ~dev_buf() { reset(); }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
  // empty after a failure
  hipError_t alloc(size_t n)
  {
    reset();
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr; else n_ = n;
    return e;
  }
  // grow-only users: nothing if the capacity suffices, otherwise free, then allocate (contents are not kept)
  hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t size() const { return n_; }
};

// a hipHostMalloc block of n elements
template <class T>
class pinned_buf {
  T *p_ = nullptr;
  size_t n_ = 0;
 public:
  pinned_buf() = default;
  pinned_buf(pinned_buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  pinned_buf &operator=(pinned_buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  ~pinned_buf() { reset(); }
  void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault)
  {
    reset();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), n * sizeof(T), flags);
    if (e != hipSuccess) p_ = nullptr; else n_ = n;
    return e;
  }
  hipError_t reserve(size_t n, unsigned flags = hipHostMallocDefault) { return n <= n_ ? hipSuccess : alloc(n, flags); }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t size() const { return n_; }
};

class hip_event {
  hipEvent_t e_ = nullptr;
 public:
  hip_event() = default;
  hip_event(hip_event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  hip_event &operator=(hip_event &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~hip_event() { reset(); }
  void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
  // an ordering event by default; hipEventDefault for one that is timed
  hipError_t create(unsigned flags = hipEventDisableTiming) { reset(); return hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }
};

class hip_stream {
  hipStream_t s_ = nullptr;
 public:
  hip_stream() = default;
  hip_stream(hip_stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  hip_stream &operator=(hip_stream &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
  ~hip_stream() { reset(); }
  void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
  hipError_t create() { reset(); return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
  operator hipStream_t() const { return s_; }
};

// A pinned host image used in turn: two slots and an event per slot, so a call that queues a copy of the image never
// waits for its own copy - a slot is taken again only when the copy that read it, two turns back, has completed.
template <class T>
class pinned_turns {
  pinned_buf<T> slot_[2];
  hip_event ev_[2];
  unsigned seq_ = 0;
 public:
  // both slots and their events up front (a user whose turns must not allocate)
  hipError_t prepare(size_t n)
  {
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = ev_[b].create();
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = slot_[b].reserve(n);
    return e;
  }
  // the next slot with room for n elements, once the copy that last read it has completed
  hipError_t take(size_t n, T **out)
  {
    const unsigned b = seq_++ & 1u;
    hipError_t e = ev_[b] ? hipSuccess : ev_[b].create();
    if (e == hipSuccess) e = hipEventSynchronize(ev_[b]);
    if (e == hipSuccess) e = slot_[b].reserve(n);
    *out = slot_[b];
    return e;
  }
  // the copy of the slot taken last has been queued on `s`
  hipError_t queued(hipStream_t s) { return hipEventRecord(ev_[(seq_ - 1) & 1u], s); }
};

#endif
