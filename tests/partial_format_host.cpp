/*
 * partial_format_host.cpp — csrc/partial_format.h under AddressSanitizer and
 * UBSan, stand-alone: no engine, no HIP, no GPU.
 *
 * Every partial block lives in a malloc'd buffer of exactly the bytes the
 * case gives the reader, so a read past `stride` is a heap overflow the
 * sanitizer reports.  Prints one line per case, one "reader <field> seen N
 * accepted A rejected R" line per field the block reader checks, one "hash"
 * line per key tuple (tests/test_partial_format_cpu.py recomputes those) and
 * OK.
 */
#include "../snappydata_amd/csrc/partial_format.h"

#include <cstdio>
#include <cstdlib>

static int g_bad = 0;
static void expect(bool ok, const char *name) {
  printf("case %-58s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) g_bad++;
}

/* exactly n bytes on the heap (n == 0 included), a copy of src's first n */
struct Heap {
  uint8_t *p;
  explicit Heap(size_t n, const uint8_t *src = nullptr)
      : p((uint8_t *)malloc(n ? n : 1)) {
    if (n == 0) { free(p); p = (uint8_t *)malloc(0); }
    if (src && n) memcpy(p, src, n); else if (n) memset(p, 0, n);
  }
  ~Heap() { free(p); }
  Heap(const Heap &) = delete;
  Heap &operator=(const Heap &) = delete;
};

struct Tally { const char *field; int seen, ok, bad; };
static Tally T_STRIDE = { "stride", 0, 0, 0 }, T_COUNT = { "count", 0, 0, 0 },
             T_KEY = { "key", 0, 0, 0 }, T_KEYLESS = { "keyless", 0, 0, 0 };
static int tally(Tally &t, int why) {
  t.seen++;
  if (why == SN_PARTIAL_OK) t.ok++; else t.bad++;
  return why;
}

static GroupOut group(const char *k0, const char *k1, double base) {
  GroupOut g;
  if (k0) g.keys[0] = k0; else g.key_null[0] = true;
  if (k1) g.keys[1] = k1; else g.key_null[1] = true;
  for (int a = 0; a < SN_MAX_AGGS; a++) {
    g.sums[a] = base + a + 0.25;
    g.counts[a] = base * 2 + a;
  }
  g.rowcount = base * 3 + 1;
  return g;
}
static bool same_values(const GroupOut &a, const GroupOut &b) {
  return !memcmp(a.sums, b.sums, sizeof(a.sums)) &&
         !memcmp(a.counts, b.counts, sizeof(a.counts)) &&
         !memcmp(&a.rowcount, &b.rowcount, 8);
}
/* what a key reads as after the block: cut at SN_KEY_MAX - 1 bytes */
static bool same_group_after_block(const GroupOut &in, const GroupOut &out,
                                   int ng) {
  for (int k = 0; k < SN_MAX_GROUPS; k++) {
    const bool carried = k < ng;
    if (out.key_null[k] != (carried && in.key_null[k])) return false;
    if (out.keys[k] != (carried ? in.keys[k].substr(0, SN_KEY_MAX - 1)
                                : std::string()))
      return false;
  }
  return same_values(in, out);
}

static void round_trip() {
  const std::string k47(47, 'q'), k60 = std::string(47, 'w') + std::string(13, 'x');
  const GroupOut G[4] = { group("", "a", 1), group(k47.c_str(), nullptr, 2),
                          group(nullptr, k60.c_str(), 3), group("k", "", 4) };
  bool sizes = sizeof(PartialSlot) == 304 && partial_grouped_bytes(1) == 8 + 304 &&
               partial_grouped_bytes(4) == 8 + 4 * 304 &&
               partial_keyless_bytes(1) == 24 && partial_keyless_bytes(12) == 200;
  expect(sizes, "block sizes: 8 + cap * 304, (2 * naggs + 1) * 8");
  bool ok = true;
  int blocks = 0;
  for (int cap : { 1, 4 })
    for (int n : { 0, 1, cap })
      for (int start = 0; start < 4; start++)
        for (int ng : { 1, 2 }) {
          const size_t bytes = (size_t)partial_grouped_bytes(cap);
          Heap h(bytes);
          partial_write_header(h.p, n, cap);
          for (int i = 0; i < n; i++)
            partial_write_slot(h.p, i, G[(start + i) % 4]);
          int32_t hn = -7, hcap = -7, got = -7;
          memcpy(&hn, h.p, 4);
          memcpy(&hcap, h.p + 4, 4);
          ok &= hn == n && hcap == cap;
          ok &= partial_check_grouped(h.p, (int64_t)bytes, ng, &got) ==
                    SN_PARTIAL_OK && got == n;
          for (int i = 0; i < n; i++) {
            GroupOut back;
            partial_read_slot(h.p, i, ng, &back);
            ok &= same_group_after_block(G[(start + i) % 4], back, ng);
          }
          /* slots past n stay zero */
          for (size_t b = 8 + (size_t)n * 304; b < bytes; b++) ok &= h.p[b] == 0;
          blocks++;
        }
  printf("round trip: %d grouped blocks\n", blocks);
  expect(ok, "grouped round trip: key lengths 0 1 47 60, NULLs, n 0 1 cap");
  ok = true;
  for (int naggs : { 1, 12 }) {
    const size_t bytes = (size_t)partial_keyless_bytes(naggs);
    Heap h(bytes);
    const GroupOut in = group("", "", 5);
    partial_write_keyless(h.p, in, naggs);
    ok &= partial_check_keyless((int64_t)bytes, naggs) == SN_PARTIAL_OK;
    GroupOut back;
    partial_read_keyless(h.p, naggs, &back);
    for (int a = 0; a < SN_MAX_AGGS; a++) {
      ok &= back.sums[a] == (a < naggs ? in.sums[a] : 0.0);
      ok &= back.counts[a] == (a < naggs ? in.counts[a] : 0.0);
    }
    ok &= back.rowcount == in.rowcount;
    double raw[25];
    memcpy(raw, h.p, bytes);
    ok &= raw[0] == in.sums[0] && raw[naggs] == in.counts[0] &&
          raw[2 * naggs] == in.rowcount;
  }
  expect(ok, "keyless round trip: naggs 1 and 12");
}

/* merge of [good block, bad block] must refuse block 1 and leave *out alone */
static bool merge_refuses(const uint8_t *good, const uint8_t *bad, size_t stride,
                          int ng, int naggs, int want) {
  Heap two(2 * stride);
  if (stride) { memcpy(two.p, good, stride); memcpy(two.p + stride, bad, stride); }
  const int kinds[SN_MAX_AGGS] = { SN_AGG_SUM };
  std::vector<GroupOut> out(1, group("sentinel", "", 9));
  int32_t at = -1;
  const int why = partial_merge(two.p, (int64_t)stride, 2, ng, naggs, kinds,
                                &out, &at);
  /* a stride too short for block 0 refuses that one first */
  return why == want && (at == 1 || at == 0) && out.size() == 1 &&
         out[0].keys[0] == "sentinel";
}

static void reader_refusals() {
  const GroupOut a = group("alpha", "x", 1), b = group("beta", nullptr, 2);
  const size_t full = (size_t)partial_grouped_bytes(2);
  Heap blk(full);
  partial_write_header(blk.p, 2, 2);
  partial_write_slot(blk.p, 0, a);
  partial_write_slot(blk.p, 1, b);
  bool ok = true;
  int32_t n = 0;
  for (size_t stride = 0; stride < full; stride++) {
    Heap cut(stride, blk.p);
    const int why = tally(T_STRIDE,
                          partial_check_grouped(cut.p, (int64_t)stride, 2, &n));
    ok &= why == (stride < 8 ? SN_PARTIAL_SHORT : SN_PARTIAL_COUNT_OVER);
  }
  ok &= tally(T_STRIDE, partial_check_grouped(blk.p, (int64_t)full, 2, &n)) ==
            SN_PARTIAL_OK && n == 2;
  ok &= partial_check_grouped(blk.p, -8, 2, &n) == SN_PARTIAL_SHORT;
  {
    Heap cut(8 + 304, blk.p);   /* n = 2 in one slot's room */
    Heap good(8 + 304, blk.p);
    partial_write_header(good.p, 1, 1);
    ok &= merge_refuses(good.p, cut.p, 8 + 304, 2, 1, SN_PARTIAL_COUNT_OVER);
  }
  expect(ok, "every stride short of 8 + 2 * 304 refused, the exact one read");

  ok = true;
  const size_t four = (size_t)partial_grouped_bytes(4);
  const struct { int32_t n; int want; } counts[] = {
    { -1, SN_PARTIAL_NEG_COUNT }, { 0x7fffffff, SN_PARTIAL_COUNT_OVER },
    { 5, SN_PARTIAL_COUNT_OVER }, { 4, SN_PARTIAL_OK }, { 0, SN_PARTIAL_OK } };
  for (const auto &c : counts) {
    Heap h(four);
    for (int i = 0; i < 4; i++) partial_write_slot(h.p, i, a);
    partial_write_header(h.p, c.n, 4);
    ok &= tally(T_COUNT, partial_check_grouped(h.p, (int64_t)four, 2, &n)) == c.want;
    if (c.want != SN_PARTIAL_OK) {
      Heap good(four);
      partial_write_header(good.p, 0, 4);
      ok &= merge_refuses(good.p, h.p, four, 2, 1, c.want);
    }
  }
  expect(ok, "slot count -1, 0x7fffffff, one more than fits refused");

  ok = true;
  for (int slot = 0; slot < 4; slot++)
    for (int col = 0; col < 2; col++)
      for (int ng = 1; ng <= 2; ng++) {
        Heap h(four);
        for (int i = 0; i < 4; i++) partial_write_slot(h.p, i, a);
        partial_write_header(h.p, 2, 4);            /* slots 2 and 3 unused */
        memset(partial_slot_at(h.p, slot) + col * SN_KEY_MAX, 'A', SN_KEY_MAX);
        const bool read = slot < 2 && col < ng;
        const int want = read ? SN_PARTIAL_KEY_OPEN : SN_PARTIAL_OK;
        ok &= tally(T_KEY, partial_check_grouped(h.p, (int64_t)four, ng, &n)) == want;
        if (read) {
          Heap good(four);
          partial_write_header(good.p, 0, 4);
          ok &= merge_refuses(good.p, h.p, four, ng, 1, want);
        }
      }
  expect(ok, "unterminated key refused in a used slot, passed over in an unused");

  ok = true;
  for (int naggs : { 1, 12 }) {
    const int64_t row = partial_keyless_bytes(naggs);
    ok &= tally(T_KEYLESS, partial_check_keyless(row - 1, naggs)) == SN_PARTIAL_SHORT;
    ok &= tally(T_KEYLESS, partial_check_keyless(row, naggs)) == SN_PARTIAL_OK;
    ok &= tally(T_KEYLESS, partial_check_keyless(0, naggs)) == SN_PARTIAL_SHORT;
    const size_t cut = (size_t)(2 * naggs + 1) * 8 - 1;
    Heap h(cut);
    ok &= merge_refuses(h.p, h.p, cut, 0, naggs, SN_PARTIAL_SHORT);
  }
  expect(ok, "keyless row one byte short refused, exact accepted");
  for (const Tally *t : { &T_STRIDE, &T_COUNT, &T_KEY, &T_KEYLESS })
    printf("reader %s seen %d accepted %d rejected %d\n", t->field, t->seen,
           t->ok, t->bad);
}

static double fold2(int kind, double s0, double c0, double s1, double c1,
                    bool *is_null) {
  GroupOut g;
  partial_fold(g, 0, kind, s0, c0);
  partial_fold(g, 0, kind, s1, c1);
  double v = -12345.0;
  *is_null = !group_value(g, 0, kind, &v);
  return v;
}

static void fold_rules() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  bool nul;
  GroupOut g;
  partial_fold(g, 0, SN_AGG_SUM, 1.5, 2);
  partial_fold(g, 0, SN_AGG_SUM, 2.5, 3);
  partial_fold(g, 1, SN_AGG_COUNT_STAR, 7, 7);
  partial_fold(g, 1, SN_AGG_COUNT_STAR, 5, 5);
  partial_fold(g, 2, SN_AGG_AVG, 1.5, 2);
  partial_fold(g, 2, SN_AGG_AVG, 2.5, 3);
  double v;
  expect(g.sums[0] == 4.0 && g.counts[0] == 5.0 && g.sums[1] == 12.0 &&
         g.counts[1] == 12.0, "SUM and COUNT add");
  expect(g.sums[2] == 4.0 && g.counts[2] == 5.0 &&
         group_value(g, 2, SN_AGG_AVG, &v) && v == 4.0 / 5.0,
         "AVG keeps sum and count, divides at read");
  expect(fold2(SN_AGG_MIN, 5, 1, -100, 0, &nul) == 5 && !nul &&
         fold2(SN_AGG_MAX, 5, 1, 100, 0, &nul) == 5 && !nul &&
         fold2(SN_AGG_MIN, -100, 0, 5, 1, &nul) == 5 && !nul &&
         fold2(SN_AGG_MAX, 100, 0, 5, 1, &nul) == 5 && !nul,
         "a count-0 contribution changes neither MIN nor MAX");
  expect(fold2(SN_AGG_MIN, nan, 1, 1, 1, &nul) == 1 &&
         fold2(SN_AGG_MIN, 1, 1, nan, 1, &nul) == 1, "MIN(NaN, 1) = 1, either order");
  const double m0 = fold2(SN_AGG_MAX, nan, 1, 1, 1, &nul);
  const double m1 = fold2(SN_AGG_MAX, 1, 1, nan, 1, &nul);
  expect(m0 != m0 && m1 != m1 && !nul, "MAX(NaN, 1) = NaN, either order");
  expect(fold2(SN_AGG_MIN, -inf, 1, 1, 1, &nul) == -inf &&
         fold2(SN_AGG_MIN, 1, 1, -inf, 1, &nul) == -inf &&
         fold2(SN_AGG_MAX, inf, 1, 1, 1, &nul) == inf &&
         fold2(SN_AGG_MAX, 1, 1, inf, 1, &nul) == inf &&
         fold2(SN_AGG_MIN, inf, 1, inf, 1, &nul) == inf &&
         fold2(SN_AGG_SUM, inf, 1, 1, 1, &nul) == inf, "+-inf are kept");
  bool all_null = true;
  for (int kind : { SN_AGG_SUM, SN_AGG_AVG, SN_AGG_MIN, SN_AGG_MAX }) {
    (void)fold2(kind, 0, 0, 0, 0, &nul);
    all_null &= nul;
  }
  expect(all_null, "a group whose every contribution has count 0 reads NULL");
  expect(fold2(SN_AGG_COUNT_STAR, 0, 0, 0, 0, &nul) == 0 && !nul,
         "COUNT(*) reads its sum even then");

  /* ORDER BY the value: NULLs last either way, NaN above +inf, stable */
  std::vector<GroupOut> rows(5);
  const double vals[5] = { 1, nan, 0, inf, 1 };
  for (int i = 0; i < 5; i++) {
    rows[i].sums[0] = vals[i];
    rows[i].counts[0] = i == 2 ? 0 : 1;      /* row 2 is NULL */
    rows[i].slot = i;
  }
  std::vector<GroupOut> asc = rows, desc = rows;
  std::stable_sort(asc.begin(), asc.end(), GroupValueLess{ 0, SN_AGG_SUM, false });
  std::stable_sort(desc.begin(), desc.end(), GroupValueLess{ 0, SN_AGG_SUM, true });
  const int want_asc[5] = { 0, 4, 3, 1, 2 }, want_desc[5] = { 1, 3, 0, 4, 2 };
  bool ok = true;
  for (int i = 0; i < 5; i++)
    ok &= asc[i].slot == want_asc[i] && desc[i].slot == want_desc[i];
  expect(ok, "order by value: NULLs last, NaN above +inf, ties stable");
}

static void identity() {
  const int kinds[SN_MAX_AGGS] = { SN_AGG_SUM };
  const size_t bb = (size_t)partial_grouped_bytes(2);
  Heap two(2 * bb);
  GroupOut ctl, nul, b;
  ctl.keys[0] = "\x01"; ctl.sums[0] = 10; ctl.counts[0] = 1; ctl.rowcount = 1;
  nul.key_null[0] = true; nul.sums[0] = 20; nul.counts[0] = 2; nul.rowcount = 2;
  b.keys[0] = "b"; b.sums[0] = 0.1; b.counts[0] = 1; b.rowcount = 1;
  partial_write_header(two.p, 2, 2);
  partial_write_slot(two.p, 0, ctl);
  partial_write_slot(two.p, 1, b);
  partial_write_header(two.p + bb, 2, 2);
  partial_write_slot(two.p + bb, 0, nul);
  ctl.sums[0] = 1;
  partial_write_slot(two.p + bb, 1, ctl);
  std::vector<GroupOut> out;
  int32_t at = -1;
  const int why = partial_merge(two.p, (int64_t)bb, 2, 1, 1, kinds, &out, &at);
  expect(why == SN_PARTIAL_OK && out.size() == 3 &&
         out[0].keys[0] == "\x01" && !out[0].key_null[0] &&
         out[0].sums[0] == 11 && out[0].counts[0] == 2 &&
         out[1].keys[0] == "b" && out[1].sums[0] == 0.1 &&
         out[2].key_null[0] && out[2].sums[0] == 20 && out[2].rowcount == 2,
         "key \"\\x01\" and the NULL key stay two groups, NULL last");
  std::vector<GroupOut> sorted(out.rbegin(), out.rend());
  std::sort(sorted.begin(), sorted.end(), GroupKeyLess());
  expect(sorted.size() == 3 && sorted[0].keys[0] == "\x01" &&
         sorted[1].keys[0] == "b" && sorted[2].key_null[0],
         "the result order is the merge's order");
  /* the keyless form folds block by block */
  const int mm[SN_MAX_AGGS] = { SN_AGG_SUM, SN_AGG_MIN };
  const size_t kb = (size_t)partial_keyless_bytes(2);
  Heap k3(3 * kb);
  for (int i = 0; i < 3; i++) {
    GroupOut g;
    g.sums[0] = 0.1 * (i + 1); g.counts[0] = 1;
    g.sums[1] = 5 - i; g.counts[1] = i == 2 ? 0 : 1;
    g.rowcount = 1;
    partial_write_keyless(k3.p + i * kb, g, 2);
  }
  const int w2 = partial_merge(k3.p, (int64_t)kb, 3, 0, 2, mm, &out, &at);
  expect(w2 == SN_PARTIAL_OK && out.size() == 1 &&
         out[0].sums[0] == (0.0 + 0.1 + 0.2) + 0.1 * 3 && out[0].sums[1] == 4 &&
         out[0].counts[1] == 2 && out[0].rowcount == 3,
         "keyless merge folds block by block");
}

static void print_hex(const GroupKey &g, int k) {
  if (g.key_null[k]) { printf(" NULL"); return; }
  printf(" x");
  for (char c : g.keys[k]) printf("%02x", (unsigned)(uint8_t)c);
}

static void shard_hash() {
  const std::string k47(47, 'z');
  const struct { int ng; const char *k0, *k1; } tuples[] = {
    { 1, "", "" }, { 1, "a", "" }, { 2, "ab", "c" }, { 2, nullptr, "x" },
    { 2, "x", nullptr }, { 1, k47.c_str(), "" } };
  for (const auto &t : tuples) {
    GroupOut g = group(t.k0, t.ng > 1 ? t.k1 : "", 0);
    printf("hash ng %d keys", t.ng);
    for (int k = 0; k < t.ng; k++) print_hex(g, k);
    printf(" h %016llx shards", (unsigned long long)partial_key_hash(g, t.ng));
    for (int world : { 1, 2, 3, 1024 })
      printf(" %d", partial_shard_of(g, t.ng, world));
    printf("\n");
  }
}

static void row_decoder() {
  /* four logical aggregates over two device sweeps: SUM(x), COUNT(*), MIN(y)
   * and SUM(x) again */
  AccRowLayout L;
  memset(&L, 0, sizeof(L));
  const int map[4] = { 0, -1, 1, 0 };
  const int kinds[4] = { SN_AGG_SUM, SN_AGG_COUNT_STAR, SN_AGG_MIN, SN_AGG_SUM };
  for (int a = 0; a < 4; a++) { L.agg_map[a] = map[a]; L.kinds[a] = kinds[a]; }
  L.na_t = 4; L.dev_naggs = 2;
  double row[9];
  auto set = [&](int form, int naggs, bool pac) {
    L.form = form; L.naggs = naggs; L.pac = pac;
    L.rowcount_at = acc_rowcount_at(form, L.na_t, L.dev_naggs, pac);
    for (int i = 0; i < 9; i++) row[i] = 10 + i;
  };
  GroupOut g;
  set(SN_ROW_KEYLESS, 3, false);
  acc_row_decode(L, row, &g);
  expect(L.rowcount_at == 8 && g.rowcount == 18 && g.sums[0] == 10 &&
         g.sums[1] == 11 && g.sums[2] == 12 && g.counts[0] == 14 &&
         g.counts[1] == 15 && g.counts[2] == 16, "row keyless: counts at na_t + a");
  set(SN_ROW_KEYLESS, 3, true);
  g = GroupOut();
  acc_row_decode(L, row, &g);
  expect(g.rowcount == 18 && g.sums[2] == 12 && g.counts[0] == 13 &&
         g.counts[1] == 14 && g.counts[2] == 15, "row keyless pac: counts at naggs + a");
  set(SN_ROW_DENSE, 4, false);
  g = GroupOut();
  acc_row_decode(L, row, &g);
  expect(L.rowcount_at == 8 && g.rowcount == 18 && g.sums[0] == 10 &&
         g.sums[1] == 18 && g.sums[2] == 11 && g.sums[3] == 10 &&
         g.counts[0] == 18 && g.counts[1] == 18 && g.counts[2] == 18 &&
         g.counts[3] == 18, "row dense grouped: counts are the rowcount");
  set(SN_ROW_DENSE, 4, true);
  g = GroupOut();
  acc_row_decode(L, row, &g);
  expect(g.rowcount == 18 && g.sums[0] == 10 && g.sums[1] == 18 &&
         g.sums[2] == 11 && g.sums[3] == 10 && g.counts[0] == 12 &&
         g.counts[1] == 18 && g.counts[2] == 13 && g.counts[3] == 12,
         "row dense grouped pac: counts at dev_naggs + di");
  const unsigned long long ord = sn_f64_ord_h(-2.5);
  set(SN_ROW_SPARSE, 4, false);
  memcpy(&row[1], &ord, 8);
  g = GroupOut();
  acc_row_decode(L, row, &g);
  expect(L.rowcount_at == 2 && g.rowcount == 12 && g.sums[0] == 10 &&
         g.sums[1] == 12 && g.sums[2] == -2.5 && g.sums[3] == 10 &&
         g.counts[0] == 12 && g.counts[2] == 12,
         "row sparse: packed, MIN cell decoded from its ord image");
  set(SN_ROW_SPARSE, 4, true);
  memcpy(&row[1], &ord, 8);
  g = GroupOut();
  acc_row_decode(L, row, &g);
  expect(L.rowcount_at == 4 && g.rowcount == 14 && g.sums[0] == 10 &&
         g.sums[1] == 14 && g.sums[2] == -2.5 && g.counts[0] == 12 &&
         g.counts[1] == 14 && g.counts[2] == 13 && g.counts[3] == 12,
         "row sparse pac: counts behind the sums");
  bool occ = acc_row_occupied(L, row);
  row[4] = 0.0;
  expect(occ && !acc_row_occupied(L, row), "a row with rowcount 0 is unoccupied");
}

int main() {
  round_trip();
  reader_refusals();
  fold_rules();
  identity();
  shard_hash();
  row_decoder();
  if (g_bad) { printf("FAILED %d\n", g_bad); return 1; }
  printf("OK\n");
  return 0;
}
