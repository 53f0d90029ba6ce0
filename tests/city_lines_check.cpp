// city_lines_check.cpp -- the line forms of city_core.h against its plain form,
// on the host (tests/test_city_lines_cpu.py builds and runs this).
//
// The long-key kernels hash through readers that set kPairs / kLines / kStream
// (kernels.h GlobalReaderT): CityHash64's loop and CityHash128WithSeed's loop
// then read 128 B per span, and CityHashCrc256Long's 240-B blocks come as
// whole 128-B lines with a carried remainder, or as a stream of lines.  Here
// the same templates run over a host reader with those constants set and are
// compared with HostReader (pinned to the oracle by the scalar tests) at every
// length 0..6000.  Each key lives in a heap block of exactly len bytes
// (round16(len) for the kStream reader, whose line_lim may read up to there),
// and the reader checks every read against that size itself, so a read past
// the key ends the program with or without a sanitizer.
//
// Arguments: any number of LEN:LO:HI (hex digests), CityHashCrc128 of this
// program's key of that length as the oracle computes it.
#include "city_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace pdht;

// byte i of the key of length len (test_city_lines_cpu.py makes the same bytes)
static uint8_t key_byte(u64 i, u64 len) {
  return (uint8_t)(((i + 1 + len * 1000003ull) * 0x9E3779B97F4A7C15ull) >> 56);
}

static const char *g_what = "";
static u64 g_len = 0;

template <bool LINES, bool STREAM>
struct CheckReader {
  static constexpr bool kLines = LINES;
  static constexpr bool kPairs = true;
  static constexpr bool kStream = STREAM;
  const uint8_t *p;
  size_t cap;  // bytes of the heap block
  void need(size_t o, size_t n) const {
    if (o + n > cap) {
      printf("FAIL %s len=%llu: read of bytes [%zu, %zu) past the key's %zu\n", g_what, (unsigned long long)g_len, o,
             o + n, cap);
      exit(1);
    }
  }
  template <int N>
  Words<N / 4> span(size_t o) const {
    need(o, N);
    Words<N / 4> w;
    memcpy(w.d, p + o, N);
    return w;
  }
  // the 16-B pieces of [o, o + N) that start below lim, the rest zero
  template <int N>
  Words<N / 4> line_lim(u32 o, u32 lim) const {
    static_assert(N % 16 == 0, "whole 16-B pieces");
    Words<N / 4> w;
    memset(w.d, 0, N);
    for (int j = 0; j < N / 16; ++j)
      if (o + 16u * j < lim) {
        need(o + 16u * j, 16);
        memcpy(w.d + 4 * j, p + o + 16 * j, 16);
      }
    return w;
  }
  u32 w32(size_t o) const { return span<4>(o).d[0]; }
  u32 b8(size_t o) const {
    need(o, 1);
    return p[o];
  }
};
typedef CheckReader<true, false> LinesReader;    // GlobalReaderT<true, kLongLines>
typedef CheckReader<false, true> StreamReader;  // GlobalReaderT<true, kLongStream>

static u64 g_checks = 0;

static void same(const char *what, u64 len, u128 got, u128 want) {
  ++g_checks;
  if (got.lo == want.lo && got.hi == want.hi) return;
  printf("FAIL %s len=%llu: got %016llx:%016llx want %016llx:%016llx\n", what, (unsigned long long)len,
         (unsigned long long)got.lo, (unsigned long long)got.hi, (unsigned long long)want.lo,
         (unsigned long long)want.hi);
  exit(1);
}

// `what` names the read that CheckReader reports, should one leave the key
#define CHECK(what, got, want) \
  do {                         \
    g_what = what;             \
    same(what, len, got, want); \
  } while (0)

static uint8_t *make_key(u64 len, size_t cap) {
  uint8_t *k = static_cast<uint8_t *>(malloc(cap ? cap : 1));
  for (u64 i = 0; i < cap; ++i) k[i] = i < len ? key_byte(i, len) : 0xA5;  // padding the digests must not see
  return k;
}

int main(int argc, char **argv) {
  const u64 s0 = 0x0123456789ABCDEFull, s1 = 0xFEDCBA9876543210ull;
  const u128 seed{s0, s1};
  for (u64 len = 0; len <= 6000; ++len) {
    g_len = len;
    const size_t cap16 = (len + 15) / 16 * 16;
    uint8_t *ke = make_key(len, len), *kr = make_key(len, cap16);
    const HostReader H{ke};
    const LinesReader L{ke, (size_t)len};
    const StreamReader S{kr, cap16};
    const u64 h64 = city64(H, len);
    CHECK("city64 lines", (u128{city64(L, len), 0}), (u128{h64, 0}));
    CHECK("city64_seeds lines", (u128{city64_seeds(L, len, s0, s1), 0}), (u128{city64_seeds(H, len, s0, s1), 0}));
    CHECK("city128 lines", city128(L, len), city128(H, len));
    CHECK("city128_seed lines", city128_seed(L, len, seed), city128_seed(H, len, seed));
    const u128 c = crc128(H, len), cs = crc128_seed(H, len, seed);
    CHECK("crc128 lines", crc128(L, len), c);
    CHECK("crc128_seed lines", crc128_seed(L, len, seed), cs);
    CHECK("crc128 stream", crc128(S, len), c);
    CHECK("crc128_seed stream", crc128_seed(S, len, seed), cs);
    free(ke);
    free(kr);
  }
  // the oracle's CityHashCrc128 of a few lengths, from the command line
  for (int a = 1; a < argc; ++a) {
    unsigned long long len, lo, hi;
    if (sscanf(argv[a], "%llu:%llx:%llx", &len, &lo, &hi) != 3) {
      printf("FAIL argument %s is not LEN:LO:HI\n", argv[a]);
      return 1;
    }
    g_len = len;
    const size_t cap16 = (len + 15) / 16 * 16;
    uint8_t *ke = make_key(len, len), *kr = make_key(len, cap16);
    const u128 want{lo, hi};
    CHECK("crc128 plain against the oracle", crc128(HostReader{ke}, len), want);
    CHECK("crc128 lines against the oracle", crc128(LinesReader{ke, (size_t)len}, len), want);
    CHECK("crc128 stream against the oracle", crc128(StreamReader{kr, cap16}, len), want);
    free(ke);
    free(kr);
  }
  printf("OK %llu\n", (unsigned long long)g_checks);
  return 0;
}
