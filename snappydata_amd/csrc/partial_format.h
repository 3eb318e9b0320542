/*
 * partial_format.h — what the host does with a finished aggregate, as pure
 * values-in / values-out functions: no HIP, no engine state, no locks.
 *
 * One place each for: the accumulator-row layout the kernels leave behind,
 * a group's identity and order, the value an aggregate reads as, the
 * partial-block byte format of the multi-GPU exchange (include/
 * snappy_engine.h), its op-aware merge and the key-shard hash.
 *
 * Partial blocks arrive from other ranks through a collective, so the merge
 * reads them only through partial_check_*: a block whose header, slot count
 * or key text does not fit its `stride` bytes is refused before anything is
 * read past them.
 */
#ifndef SN_PARTIAL_FORMAT_H
#define SN_PARTIAL_FORMAT_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "engine_internal.h"

/* ---- a group: identity, order, values ---- */

struct GroupKey {
  std::string keys[SN_MAX_GROUPS];
  bool key_null[SN_MAX_GROUPS] = {};
};

struct GroupOut : GroupKey {
  double sums[SN_MAX_AGGS] = { 0 };
  double counts[SN_MAX_AGGS] = { 0 };
  double rowcount = 0;
  int slot = 0;   /* dense accumulator slot (decimal queries look their
                     exact values up by it after the key sort) */
};

/* two groups are one when neither orders before the other: per column a
 * non-NULL key before the NULL key, then the key bytes.  The result order
 * and the merge's map share it, so a NULL key is no text of its own. */
struct GroupKeyLess {
  bool operator()(const GroupKey &a, const GroupKey &b) const {
    for (int k = 0; k < SN_MAX_GROUPS; k++) {
      if (a.key_null[k] != b.key_null[k]) return !a.key_null[k];
      const int c = a.keys[k].compare(b.keys[k]);
      if (c) return c < 0;
    }
    return false;
  }
};

/* key text as results and partial slots carry it: at most SN_KEY_MAX - 1
 * bytes, NUL-terminated.  dst must be zeroed. */
static inline void group_key_put(char *dst, const std::string &key) {
  strncpy(dst, key.c_str(), SN_KEY_MAX - 1);
}

/* the value aggregate `a` (of `kind`) of a group reads as; false: NULL.
 * COUNT(*) is never NULL; the others are when nothing non-null came in;
 * AVG divides only here. */
static inline bool group_value(const GroupOut &g, int a, int kind, double *v) {
  if (kind == SN_AGG_COUNT_STAR) { *v = g.sums[a]; return true; }
  if (!(g.counts[a] > 0)) return false;
  *v = kind == SN_AGG_AVG ? g.sums[a] / g.counts[a] : g.sums[a];
  return true;
}

/* ORDER BY that value: NULLs last either way, and a strict weak order with
 * NaN in it — every NaN is one value above +inf */
struct GroupValueLess {
  int a, kind;
  bool descending;
  bool operator()(const GroupOut &x, const GroupOut &y) const {
    double vx, vy;
    const bool hx = group_value(x, a, kind, &vx);
    const bool hy = group_value(y, a, kind, &vy);
    if (hx != hy) return hx;
    if (!hx) return false;
    const bool nx = vx != vx, ny = vy != vy;
    if (nx || ny) return descending ? nx && !ny : ny && !nx;
    return descending ? vx > vy : vx < vy;
  }
};

/* ---- accumulator rows: the contract with the kernels ----
 * A row is doubles.  Three forms:
 *   KEYLESS  k_keyless / one-slot result: [sums naggs] .. [counts naggs] ..
 *            [rowcount]; the counts start at na_t, the kernel's template
 *            capacity — or at naggs when the plan ran the per-agg-count
 *            (pac) grouped layout with one slot, as MIN/MAX plans do
 *   DENSE    k_reduce's grouped row, one per dense slot: the deduped device
 *            sweeps [sums dev_naggs][counts dev_naggs, pac only] and the
 *            rowcount at 2 * na_t
 *   SPARSE   the hash aggregate's compacted row: the same cells packed,
 *            rowcount right behind them; MIN/MAX cells still hold the
 *            ord-u64 image (these rows bypass k_reduce)
 * In the grouped forms logical aggregate a reads device sweep agg_map[a];
 * -1 is COUNT(*), the rowcount.  Without pac every count is the rowcount. */
enum { SN_ROW_KEYLESS, SN_ROW_DENSE, SN_ROW_SPARSE };

struct AccRowLayout {
  int form;
  int naggs, na_t, dev_naggs;
  bool pac;
  int agg_map[SN_MAX_AGGS];
  int kinds[SN_MAX_AGGS];      /* SN_AGG_* per logical aggregate */
  int rowcount_at;             /* the row is rowcount_at + 1 doubles */
};

static inline int acc_rowcount_at(int form, int na_t, int dev_naggs, bool pac) {
  return form == SN_ROW_SPARSE ? (pac ? 2 : 1) * dev_naggs : 2 * na_t;
}

/* did any row reach this slot? */
static inline bool acc_row_occupied(const AccRowLayout &L, const double *row) {
  return row[L.rowcount_at] != 0.0;
}

static inline void acc_row_decode(const AccRowLayout &L, const double *row,
                                  GroupOut *g) {
  const double rowcount = g->rowcount = row[L.rowcount_at];
  for (int a = 0; a < L.naggs; a++) {
    if (L.form == SN_ROW_KEYLESS) {
      g->sums[a] = row[a];
      g->counts[a] = row[(L.pac ? L.naggs : L.na_t) + a];
      continue;
    }
    const int di = L.agg_map[a];
    double s = di < 0 ? rowcount : row[di];
    if (L.form == SN_ROW_SPARSE && di >= 0 &&
        (L.kinds[a] == SN_AGG_MIN || L.kinds[a] == SN_AGG_MAX)) {
      unsigned long long o;
      memcpy(&o, &row[di], 8);
      s = sn_ord_f64_h(o);
    }
    g->sums[a] = s;
    g->counts[a] = (di < 0 || !L.pac) ? rowcount : row[L.dev_naggs + di];
  }
}

/* ---- partial blocks ----
 *   keyless: [naggs sums][naggs counts][rowcount], all f64
 *   grouped: [i32 n][i32 cap] then cap slots, the first n used */
struct PartialSlot {
  char keys[SN_MAX_GROUPS][SN_KEY_MAX];
  uint8_t key_null[SN_MAX_GROUPS];
  uint8_t pad[6];
  double sums[SN_MAX_AGGS];
  double counts[SN_MAX_AGGS];
  double rowcount;
};
static_assert(sizeof(PartialSlot) == SN_MAX_GROUPS * SN_KEY_MAX + 8 +
              2 * SN_MAX_AGGS * 8 + 8, "partial slot layout");

#define SN_PARTIAL_HEADER 8

static inline int64_t partial_keyless_bytes(int naggs) {
  return (int64_t)(2 * naggs + 1) * 8;
}
static inline int64_t partial_grouped_bytes(int32_t cap) {
  return SN_PARTIAL_HEADER + (int64_t)cap * (int64_t)sizeof(PartialSlot);
}

static inline void partial_write_keyless(uint8_t *block, const GroupOut &g,
                                         int naggs) {
  memcpy(block, g.sums, (size_t)naggs * 8);
  memcpy(block + (size_t)naggs * 8, g.counts, (size_t)naggs * 8);
  memcpy(block + (size_t)naggs * 16, &g.rowcount, 8);
}
static inline void partial_write_header(uint8_t *block, int32_t n, int32_t cap) {
  memcpy(block, &n, 4);
  memcpy(block + 4, &cap, 4);
}
static inline uint8_t *partial_slot_at(const uint8_t *block, int32_t i) {
  return (uint8_t *)block + SN_PARTIAL_HEADER + (size_t)i * sizeof(PartialSlot);
}
/* keys longer than SN_KEY_MAX - 1 bytes are cut there */
static inline void partial_write_slot(uint8_t *block, int32_t i,
                                      const GroupOut &g) {
  PartialSlot s;
  memset(&s, 0, sizeof(s));
  for (int k = 0; k < SN_MAX_GROUPS; k++) {
    group_key_put(s.keys[k], g.keys[k]);
    s.key_null[k] = g.key_null[k] ? 1 : 0;
  }
  memcpy(s.sums, g.sums, sizeof(s.sums));
  memcpy(s.counts, g.counts, sizeof(s.counts));
  s.rowcount = g.rowcount;
  memcpy(partial_slot_at(block, i), &s, sizeof(s));
}

/* why a block of `stride` bytes cannot be read */
enum {
  SN_PARTIAL_OK = 0,
  SN_PARTIAL_SHORT,        /* stride below the keyless row / grouped header */
  SN_PARTIAL_NEG_COUNT,    /* n < 0 */
  SN_PARTIAL_COUNT_OVER,   /* n slots do not fit stride */
  SN_PARTIAL_KEY_OPEN      /* a used key without a NUL in SN_KEY_MAX bytes */
};
static inline const char *partial_bad_text(int why) {
  switch (why) {
    case SN_PARTIAL_SHORT: return "stride is shorter than the block's fixed part";
    case SN_PARTIAL_NEG_COUNT: return "negative slot count";
    case SN_PARTIAL_COUNT_OVER: return "slot count does not fit stride";
    case SN_PARTIAL_KEY_OPEN: return "group key without a terminating NUL";
    default: return "ok";
  }
}

static inline int partial_check_keyless(int64_t stride, int naggs) {
  return stride >= partial_keyless_bytes(naggs) ? SN_PARTIAL_OK
                                                : SN_PARTIAL_SHORT;
}
/* reads the header, then only the key bytes of the n slots it proved present */
static inline int partial_check_grouped(const uint8_t *block, int64_t stride,
                                        int eff_ngroup, int32_t *n_out) {
  if (stride < SN_PARTIAL_HEADER) return SN_PARTIAL_SHORT;
  int32_t n;
  memcpy(&n, block, 4);
  if (n < 0) return SN_PARTIAL_NEG_COUNT;
  if (n > (stride - SN_PARTIAL_HEADER) / (int64_t)sizeof(PartialSlot))
    return SN_PARTIAL_COUNT_OVER;
  for (int32_t i = 0; i < n; i++)
    for (int k = 0; k < eff_ngroup; k++)
      if (!memchr(partial_slot_at(block, i) + (size_t)k * SN_KEY_MAX, 0,
                  SN_KEY_MAX))
        return SN_PARTIAL_KEY_OPEN;
  *n_out = n;
  return SN_PARTIAL_OK;
}
/* slot i < n of a block partial_check_grouped accepted */
static inline void partial_read_slot(const uint8_t *block, int32_t i,
                                     int eff_ngroup, GroupOut *g) {
  PartialSlot s;
  memcpy(&s, partial_slot_at(block, i), sizeof(s));
  *g = GroupOut();
  for (int k = 0; k < eff_ngroup; k++) {
    g->keys[k] = s.keys[k];
    g->key_null[k] = s.key_null[k] != 0;
  }
  memcpy(g->sums, s.sums, sizeof(s.sums));
  memcpy(g->counts, s.counts, sizeof(s.counts));
  g->rowcount = s.rowcount;
}
static inline void partial_read_keyless(const uint8_t *block, int naggs,
                                        GroupOut *g) {
  *g = GroupOut();
  memcpy(g->sums, block, (size_t)naggs * 8);
  memcpy(g->counts, block + (size_t)naggs * 8, (size_t)naggs * 8);
  memcpy(&g->rowcount, block + (size_t)naggs * 16, 8);
}

/* op-aware fold of one contribution (sum s over c non-null inputs) into
 * aggregate a of g.  MIN/MAX ignore a contribution nothing went into and
 * order NaN above +inf: fmin returns the other side of a NaN, which is MIN's
 * rule already; MAX keeps the NaN (std::min/std::max would keep whichever
 * side came first). */
static inline void partial_fold(GroupOut &g, int a, int kind, double s,
                                double c) {
  if (kind == SN_AGG_MIN || kind == SN_AGG_MAX) {
    if (c > 0)
      g.sums[a] = g.counts[a] <= 0 ? s
                  : kind == SN_AGG_MIN ? fmin(g.sums[a], s)
                  : (g.sums[a] != g.sums[a] || s != s)
                      ? std::numeric_limits<double>::quiet_NaN()
                      : fmax(g.sums[a], s);
  } else {
    g.sums[a] += s;
  }
  g.counts[a] += c;
}
static inline void partial_fold_group(GroupOut &g, const GroupOut &in,
                                      int naggs, const int *kinds) {
  for (int a = 0; a < naggs; a++)
    partial_fold(g, a, kinds[a], in.sums[a], in.counts[a]);
  g.rowcount += in.rowcount;
}

/* n_blocks blocks, `stride` bytes apart, into one group list in key order
 * (eff_ngroup == 0: the keyless form, one group).  Every block is checked
 * before any is folded; a refusal returns its SN_PARTIAL_* reason with
 * *bad_block set and leaves *out alone.  Each group folds its contributions
 * block by block, slot by slot. */
static inline int partial_merge(const void *blocks, int64_t stride,
                                int32_t n_blocks, int eff_ngroup, int naggs,
                                const int *kinds, std::vector<GroupOut> *out,
                                int32_t *bad_block) {
  const uint8_t *base = (const uint8_t *)blocks;
  std::vector<int32_t> used((size_t)n_blocks, 0);
  for (int32_t bi = 0; bi < n_blocks; bi++) {
    const int why = eff_ngroup == 0
        ? partial_check_keyless(stride, naggs)
        : partial_check_grouped(base + bi * stride, stride, eff_ngroup,
                                &used[(size_t)bi]);
    if (why != SN_PARTIAL_OK) { *bad_block = bi; return why; }
  }
  GroupOut in;
  if (eff_ngroup == 0) {
    GroupOut g;
    for (int32_t bi = 0; bi < n_blocks; bi++) {
      partial_read_keyless(base + bi * stride, naggs, &in);
      partial_fold_group(g, in, naggs, kinds);
    }
    out->assign(1, g);
    return SN_PARTIAL_OK;
  }
  std::map<GroupKey, GroupOut, GroupKeyLess> bykey;
  for (int32_t bi = 0; bi < n_blocks; bi++)
    for (int32_t i = 0; i < used[(size_t)bi]; i++) {
      partial_read_slot(base + bi * stride, i, eff_ngroup, &in);
      auto it = bykey.find(in);
      if (it == bykey.end()) {
        GroupOut g;
        static_cast<GroupKey &>(g) = in;
        it = bykey.emplace(in, std::move(g)).first;
      }
      partial_fold_group(it->second, in, naggs, kinds);
    }
  out->clear();
  out->reserve(bykey.size());
  for (auto &kv : bykey) out->push_back(std::move(kv.second));
  return SN_PARTIAL_OK;
}

/* the rank that owns a group in the key-sharded exchange: FNV-1a over the
 * first eff_ngroup keys — a NULL key is the byte 1, any other its bytes, and
 * 0xff closes every key.  Ranks must agree on it bit for bit. */
static inline uint64_t partial_key_hash(const GroupKey &g, int eff_ngroup) {
  uint64_t h = 1469598103934665603ull;
  for (int k = 0; k < eff_ngroup; k++) {
    if (g.key_null[k]) { h ^= 1; h *= 1099511628211ull; }
    else
      for (char c : g.keys[k]) { h ^= (uint8_t)c; h *= 1099511628211ull; }
    h ^= 0xff; h *= 1099511628211ull;
  }
  return h;
}
static inline int partial_shard_of(const GroupKey &g, int eff_ngroup,
                                   int world) {
  return (int)(partial_key_hash(g, eff_ngroup) % (uint64_t)world);
}

#endif
