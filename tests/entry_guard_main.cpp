// entry_guard_main.cpp - the guard of the C boundary (mckpp_f90_amd/csrc/mckpp_own.h: entry, for_columns, half_built) on
// its own: a host program that makes no HIP call, built with the address and undefined-behaviour sanitizers and run as a
// child process by tests/test_entry_cpu.py.  It exits non-zero at the first check that does not hold.
#include "mckpp_own.h"

#include <atomic>
#include <cstring>
#include <new>
#include <stdexcept>
#include <system_error>

static int checks = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    ++checks;                                                                                                \
    if (!(cond)) {                                                                                           \
      fprintf(stderr, "%s:%d: (%s) does not hold; last error \"%s\"\n", __FILE__, __LINE__, #cond, g_err.c_str()); \
      return 1;                                                                                              \
    }                                                                                                        \
  } while (0)

// a stand-in for a context: its finalizer counts its calls
struct thing { int made = 1; };
static int finalized = 0;
static int thing_finalize(thing *t) { ++finalized; delete t; return 0; }

static int thing_init(bool fails, thing **out)
{
  return entry(__func__, [&]() -> int {
    half_built<thing, thing_finalize> g(new thing());
    if (fails) throw std::runtime_error("half built");
    *out = g.release();
    return 0;
  });
}

// what() of the exception `thrower` throws
template <class F>
static std::string what_of(F &&thrower)
{
  try { thrower(); } catch (const std::exception &e) { return e.what(); }
  return "";
}

static void throw_length_error()
{
  volatile size_t n = size_t(-1);
  std::vector<int> v(n);
  (void)v;
}
static void throw_system_error() { throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "thread"); }

static int guard_checks()
{
  thing t, *none = nullptr;
  bool ran = false;
  // a null handle: -1, the text, and the body does not run
  CHECK(entry("f_null", none, [&]() -> int { ran = true; return 0; }) == -1);
  CHECK(g_err == "f_null: null handle" && !ran);
  // a body's return value passes through; the error text is untouched on 0
  g_err = "before";
  CHECK(entry("f_zero", &t, [&]() -> int { return 0; }) == 0 && g_err == "before");
  CHECK(entry("f_seven", &t, [&]() -> int { return 7; }) == 7 && g_err == "before");
  CHECK(entry("f_plain", [&]() -> int { return -3; }) == -3 && g_err == "before");
  CHECK(entry("f_fail", &t, [&]() -> int { return fail("f_fail: %d", 5); }) == -1 && g_err == "f_fail: 5");
  // no exception leaves it
  CHECK(entry("f_alloc", &t, [&]() -> int { throw std::bad_alloc(); }) == -1);
  CHECK(g_err == "f_alloc: " + what_of([] { throw std::bad_alloc(); }));
  const std::string le = what_of(throw_length_error), se = what_of(throw_system_error);
  CHECK(!le.empty() && !se.empty());
  CHECK(entry("f_length", &t, [&]() -> int { throw_length_error(); return 0; }) == -1 && g_err == "f_length: " + le);
  CHECK(entry("f_system", [&]() -> int { throw_system_error(); return 0; }) == -1 && g_err == "f_system: " + se);
  CHECK(entry("f_int", &t, [&]() -> int { throw 42; }) == -1 && g_err == "f_int: unknown exception");
  return 0;
}

static int columns_checks()
{
  // every index exactly once, on one thread below 32768 indices and on MCKPP_HIP_HOST_THREADS = 4 from there on
  for (const int64_t n : {(int64_t)0, (int64_t)1, (int64_t)32767, (int64_t)32768, (int64_t)32769, (int64_t)65537}) {
    std::vector<std::atomic<int>> seen((size_t)n);
    for (auto &s : seen) s = 0;
    std::atomic<int> chunks{0};
    for_columns(n, [&](int64_t a, int64_t b) {
      ++chunks;
      for (int64_t i = a; i < b; ++i) ++seen[(size_t)i];
    });
    int64_t once = 0;
    for (auto &s : seen) once += s == 1;
    CHECK(once == n);
    CHECK(chunks == (n < 32768 ? 1 : 4));
  }
  // a throw from a worker's chunk, from the caller's own, from both: -1 and the thrown text through the guard, on this
  // thread, after every chunk has run to its end (the threads were joined: a joinable one would have ended the program)
  const int64_t n = 65536, chunk = n / 4;
  for (const int who_throws : {1, 2, 3}) {   // bit 0: the caller's chunk, bit 1: the second worker's
    std::vector<std::atomic<int>> seen((size_t)n);
    for (auto &s : seen) s = 0;
    const int rc = entry("f_columns", [&]() -> int {
      for_columns(n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) ++seen[(size_t)i];
        if (a == 0 && (who_throws & 1)) throw std::runtime_error("the caller's chunk");
        if (a == 2 * chunk && (who_throws & 2)) throw std::runtime_error("a worker's chunk");
      });
      return 0;
    });
    CHECK(rc == -1);
    CHECK(g_err == ((who_throws & 1) ? "f_columns: the caller's chunk" : "f_columns: a worker's chunk"));
    int64_t once = 0;
    for (auto &s : seen) once += s == 1;
    CHECK(once == n);
  }
  return 0;
}

static int ownership_checks()
{
  thing *got = nullptr;
  CHECK(thing_init(true, &got) == -1 && g_err == "thing_init: half built");
  CHECK(finalized == 1 && got == nullptr);   // finalized once after the throw
  CHECK(thing_init(false, &got) == 0 && got != nullptr);
  CHECK(finalized == 1);                     // ... and not at all after success
  thing_finalize(got);
  return 0;
}

int main()
{
  setenv("MCKPP_HIP_HOST_THREADS", "4", 1);   // read once, by the first for_columns
  if (guard_checks() || columns_checks() || ownership_checks()) return 1;
  printf("entry_guard: %d checks hold\n", checks);
  return 0;
}
