// What the stand-alone sanitizer programs (asan_*.cpp) share: the check that counts, a heap copy of exactly the stated size, so that a
// read past a list is an error of the sanitizer, and the verdict: "clean" and exit code 0 only if every check held.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond, what)                                       \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAILED: %s (line %d)\n", what, __LINE__); \
      failures++;                                                \
    }                                                            \
  } while (0)

template <class T>
struct Exact {  // a heap copy of exactly the stated size
  T* p;
  explicit Exact(const std::vector<T>& v) : p(v.empty() ? nullptr : (T*)malloc(v.size() * sizeof(T))) {
    if (p) memcpy(p, v.data(), v.size() * sizeof(T));
  }
  ~Exact() { free(p); }
};

static inline uint64_t pow2(uint64_t v, uint64_t least = 1) {  // the least power of two >= max(least, v)
  uint64_t p = least;
  while (p < v) p <<= 1;
  return p;
}

// main's return value: `what` says what ran ("asan_x", or "12 calls of mh_x")
static inline int verdict(const char* what) {
  if (failures) {
    fprintf(stderr, "%s: %d failure(s)\n", what, failures);
    return 1;
  }
  printf("%s: clean\n", what);
  return 0;
}
