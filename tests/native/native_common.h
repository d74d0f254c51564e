// What the stand-alone drivers of this directory share; each driver is one program, so this is included once a program.
//   pr::set_error   what the code under test reports through: keeps the last message in pr::g_error and echoes it to stderr
//                   (not with NATIVE_QUIET_ERRORS defined before the include: drivers that provoke refusals by the hundred)
//   exact<T>(n)     a zeroed heap block of exactly n elements: the sanitizer sees the first byte read or written outside it
//   CHECK           counts a failed condition in g_fail and reports it on a line tests/host_build.py looks for
//   read_pack       the file tests/host_build.py's pack_streams writes: int64 F, int64 offsets[F + 1], the streams back to back
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "host_common.h"

namespace pr {
inline char g_error[1024];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
#ifndef NATIVE_QUIET_ERRORS
  fprintf(stderr, "%s\n", g_error);
#endif
}
}  // namespace pr

template <class T>
inline std::unique_ptr<T[]> exact(size_t n) {   // at least one element: new T[0] may not be read
  return std::unique_ptr<T[]>(new T[n ? n : 1]());
}

inline int g_fail = 0;
#define CHECK(cond, ...)                                           \
  do {                                                             \
    if (!(cond)) {                                                 \
      fprintf(stderr, "CHECK FAILED %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                \
      fprintf(stderr, "\n");                                       \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct Pack {
  int64_t F = 0;
  std::vector<int64_t> off;
  std::vector<uint8_t> all;
  int64_t size(int64_t i) const { return off[i + 1] - off[i]; }
  std::unique_ptr<uint8_t[]> copy(int64_t i) const {   // stream i in a block of exactly its size
    auto data = exact<uint8_t>((size_t)size(i));
    memcpy(data.get(), all.data() + off[i], (size_t)size(i));
    return data;
  }
};

inline Pack read_pack(const char* in) {
  Pack k;
  std::ifstream f(in, std::ios::binary);
  f.read((char*)&k.F, 8);
  k.off.resize((size_t)k.F + 1);
  f.read((char*)k.off.data(), (std::streamsize)(8 * (k.F + 1)));
  k.all.resize((size_t)k.off[k.F]);
  f.read((char*)k.all.data(), (std::streamsize)k.all.size());
  return k;
}
