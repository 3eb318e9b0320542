/*
 * lut_span_host.cpp — sn_lut_span (csrc/engine_internal.h) under UBSan and
 * AddressSanitizer, stand-alone: no engine, no HIP, no GPU.
 *
 * sn_lut_span decides whether a join dimension gets a dense LUT and how many
 * entries it holds; both build sites (sn_dim_put's host table and
 * sn_dim_from_table's device table) size an allocation of span * 4 bytes from
 * it and index it with key - min.  The cases are the bounds at which a signed
 * or truncated difference goes wrong: spans past 2^63 wrap negative in int64,
 * and the true spans 2^63 + 1 and 3 * 2^62 + 1 are the two for which
 * (size_t)span * 4 wraps to 4 bytes.  For every accepted span the program
 * allocates exactly span * 4 bytes and writes the first and the last entry,
 * as the builders do, so a span that is too small is a heap overflow.
 * Prints one line per case and OK.
 */
#include "../snappydata_amd/csrc/engine_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

struct Case {
  const char *name;
  int64_t mn, mx;
  int64_t want;
};

int main() {
  const int64_t P24 = 1ll << 24, P61 = 1ll << 61, P62 = 1ll << 62;
  const Case cases[] = {
    { "one key", 0, 0, 1 },
    { "empty range", 5, 4, 0 },
    { "span 2^24, negative min", -3, P24 - 4, P24 },
    { "span 2^24 + 1", -3, P24 - 3, 0 },
    { "span 2^63 + 1 (4 * span wraps to 4)", -P62, P62, 0 },
    { "span 2^63 - 1", -P62, P62 - 2, 0 },
    { "span 2^64", INT64_MIN, INT64_MAX, 0 },
    { "span 8 at INT64_MIN", INT64_MIN, INT64_MIN + 7, 8 },
    { "span 8 at INT64_MAX", INT64_MAX - 7, INT64_MAX, 8 },
    { "span 3 * 2^62 + 1 (4 * span wraps to 4)", -3 * P61, 3 * P61, 0 },
  };
  int bad = 0, accepted = 0, refused = 0;
  for (const Case &c : cases) {
    const int64_t got = sn_lut_span(c.mn, c.mx);
    printf("case %-42s mn %lld mx %lld span %lld want %lld\n", c.name,
           (long long)c.mn, (long long)c.mx, (long long)got,
           (long long)c.want);
    if (got != c.want) { bad++; continue; }
    if (got == 0) { refused++; continue; }
    accepted++;
    /* what the builders do with an accepted span */
    std::vector<int32_t> lut((size_t)got, -1);
    const uint64_t first = (uint64_t)c.mn - (uint64_t)c.mn;
    const uint64_t last = (uint64_t)c.mx - (uint64_t)c.mn;
    lut[(size_t)first] = 1;
    lut[(size_t)last] = 2;
    if (lut.size() * 4 != (size_t)got * 4 || last != (uint64_t)got - 1) bad++;
  }
  printf("cases %d accepted %d refused %d\n",
         (int)(sizeof(cases) / sizeof(cases[0])), accepted, refused);
  if (bad) { printf("FAILED %d\n", bad); return 1; }
  printf("OK\n");
  return 0;
}
