// Shared by the stand-alone sanitizer programs (host_surface.cpp, host_threads.cpp): a fixed-seed generator, the FNV-1a fold of everything a
// call hands back, exact-size heap buffers (one byte too many is a heap-buffer-overflow under AddressSanitizer) and the SECTION lines
// tests/test_host_sanitizers.py reads:   SECTION <name> cases=<n> digest=<fnv1a-64, 16 hex digits>
#ifndef IPK_TESTS_SAN_COMMON_HPP
#define IPK_TESTS_SAN_COMMON_HPP
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "imagepipe_amd.h"

namespace san {

struct Rng {                                               // SplitMix64
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  uint64_t below(uint64_t n) { return next() % n; }
  int range(int lo, int hi) { return lo + (int)below((uint64_t)(hi - lo + 1)); }     // inclusive
  float unit() { return (float)(next() >> 40) / 16777216.0f; }
};

struct Section {
  const char *name; uint64_t h = 0xcbf29ce484222325ull; uint64_t cases = 0;
  explicit Section(const char *n) : name(n) {}
  void bytes(const void *p, size_t n) { const unsigned char *b = static_cast<const unsigned char *>(p); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; } }
  void i32(int32_t v) { unsigned char b[4]; for (int i = 0; i < 4; ++i) b[i] = (unsigned char)((uint32_t)v >> (8 * i)); bytes(b, 4); }
  void u64(uint64_t v) { unsigned char b[8]; for (int i = 0; i < 8; ++i) b[i] = (unsigned char)(v >> (8 * i)); bytes(b, 8); }
  // float outputs: a NaN enters as one canonical NaN -- its sign and payload are not defined by IEEE 754 arithmetic (0/0 made at run time on x86 is
  // negative, the same quotient folded by the compiler positive), so two correct builds may differ there and nowhere else
  void f32s(const float *v, size_t n) { for (size_t i = 0; i < n; ++i) { uint32_t u; std::memcpy(&u, &v[i], 4); if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u; i32((int32_t)u); } }
  void str(const char *s) { bytes(s, std::strlen(s) + 1); }
  // a return code; a failure's message goes into the digest too
  int rc(int code) { i32(code); if (code < 0) str(ipk_last_error()); return code; }
  void done() const { std::printf("SECTION %s cases=%llu digest=%016llx\n", name, (unsigned long long)cases, (unsigned long long)h); std::fflush(stdout); }
};

// a fresh heap block of exactly n elements (n = 0: a block no byte of which may be touched), filled with a pattern
template <typename T> struct Exact {
  T *p; size_t n;
  explicit Exact(size_t count, unsigned char fill = 0x55) : p(static_cast<T *>(std::malloc(count * sizeof(T)))), n(count) {
    if (!p) { std::fprintf(stderr, "out of memory\n"); std::exit(3); }
    std::memset(static_cast<void *>(p), fill, count * sizeof(T));
  }
  ~Exact() { std::free(p); }
  Exact(const Exact &) = delete; Exact &operator=(const Exact &) = delete;
  T &operator[](size_t i) { return p[i]; }
  operator T *() { return p; }
  size_t size_bytes() const { return n * sizeof(T); }
};

inline int g_failures = 0;
#define SAN_EXPECT(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "CONTRACT %s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); ++san::g_failures; } } while (0)

}  // namespace san
#endif
