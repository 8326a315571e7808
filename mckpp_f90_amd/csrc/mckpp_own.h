// mckpp_own.h - what the host runtime (mckpp_runtime.cpp) owns at its C boundary.  Host code only.
//
// The error state: the thread's last error text (g_err, fail, HIPCHK) and the one guard every extern "C" function goes
// through (entry): a null pointer for the handle is refused by the function's name, and no C++ exception leaves the
// library - it becomes -1 and a text.  for_columns, the host's loop over the columns on a few threads, is here because
// the guard must be able to guard it: it joins what it started and brings a worker's exception back to the caller's
// thread.
//
// The resources: move-only owners of device blocks, pinned host blocks, events, streams and plane tables, and
// half_built, the owner of an object until its init function hands it out.  An owner never synchronises and never
// reports an error from its destructor: whoever drops a buffer that queued work may still use waits first, at the
// call site.  (The one wait in this file is pinned_turns::take, which is that type's purpose.)
#ifndef MCKPP_OWN_H
#define MCKPP_OWN_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <string>
#include <thread>
#include <vector>

inline thread_local std::string g_err;

inline int fail(const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// The guard of an extern "C" function that returns an error code: `who` is its __func__ (evaluated there, not in the
// body's lambda), `body` its code, which returns what the function returns - HIPCHK inside it returns from it.
template <class F>
int entry(const char *who, F &&body) noexcept
{
  try {
    return body();
  } catch (const std::exception &e) {
    return fail("%s: %s", who, e.what());
  } catch (...) {
    return fail("%s: unknown exception", who);
  }
}

// ... of one that takes a handle
template <class H, class F>
int entry(const char *who, H *h, F &&body) noexcept
{
  return entry(who, [&]() -> int { return h ? body() : fail("%s: null handle", who); });
}

// An object between `new` and the end of its init function: finalized by Fin unless release() hands it out.
template <class T, int (*Fin)(T *)>
struct finalizes {
  void operator()(T *p) const { (void)Fin(p); }
};
template <class T, int (*Fin)(T *)>
using half_built = std::unique_ptr<T, finalizes<T, Fin>>;

// The host loops over the columns (compaction of the forcing, scatter of the per-column records) on a few
// threads: at 1e5 columns they are milliseconds of a 3.4 ms step otherwise.  MCKPP_HIP_HOST_THREADS sets the count
// (default: the machine's, at most 8).  Every thread started is joined before the call is left, by return or by
// exception; the first chunk's exception (in chunk order) is rethrown on the caller's thread once all have been.
template <class F>
void for_columns(int64_t n, F &&body)
{
  static const int want = [] {
    const char *e = getenv("MCKPP_HIP_HOST_THREADS");
    int t = e ? atoi(e) : (int)std::thread::hardware_concurrency();
    return t < 1 ? 1 : t > 8 ? 8 : t;
  }();
  const int nt = n < 32768 ? 1 : want;
  if (nt == 1) { body((int64_t)0, n); return; }
  const int64_t chunk = (n + nt - 1) / nt;
  std::vector<std::exception_ptr> thrown((size_t)nt);   // a slot per chunk: nothing to lock
  auto run = [&](int t, int64_t a, int64_t b) noexcept {
    try { body(a, b); } catch (...) { thrown[(size_t)t] = std::current_exception(); }
  };
  {
    struct joined { std::vector<std::thread> th; ~joined() { for (auto &x : th) x.join(); } } j;
    j.th.reserve((size_t)nt - 1);
    for (int t = 1; t < nt; ++t) {
      const int64_t a = t * chunk, b = a + chunk < n ? a + chunk : n;
      if (a < b) j.th.emplace_back([&run, t, a, b] { run(t, a, b); });
    }
    run(0, (int64_t)0, chunk < n ? chunk : n);
  }
  for (auto &e : thrown) if (e) std::rethrow_exception(e);
}

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
  // recorded on `s`; an ordering event is created on first use
  hipError_t record(hipStream_t s) { const hipError_t e = e_ ? hipSuccess : create(); return e == hipSuccess ? hipEventRecord(e_, s) : e; }
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

// A table of planes onto the device on a stream (the plane kernels of mckpp_device.h read theirs there): the device
// block of CAP entries, allocated on first use, and the pinned image it is written from, used in turn - so a call
// never waits for its own copy, and the copy is ordered on the stream ahead of the launch that reads the table.
template <class T, size_t CAP>
class plane_table {
  dev_buf<T> dev_;
  pinned_turns<T> host_;
 public:
  // tab (at most CAP entries) to the device behind what `s` holds
  hipError_t put(const std::vector<T> &tab, hipStream_t s)
  {
    T *q = nullptr;
    hipError_t e = dev_ ? hipSuccess : dev_.alloc(CAP);
    if (e == hipSuccess) e = host_.take(CAP, &q);
    for (size_t i = 0; e == hipSuccess && i < tab.size(); ++i) q[i] = tab[i];
    if (e == hipSuccess) e = hipMemcpyAsync(dev_, q, tab.size() * sizeof(T), hipMemcpyHostToDevice, s);
    return e == hipSuccess ? host_.queued(s) : e;
  }
  operator const T *() const { return dev_; }
};

#endif
