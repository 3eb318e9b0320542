/*
 * engine_internal.h — device-visible descriptors shared between the host
 * runtime (engine.cpp) and the HIP kernels (kernels.hip).
 *
 * The engine stores column batches in HBM in the reference's encoded byte
 * format and decodes INSIDE the scan kernel.  The host
 * pre-parses each blob's header once at sn_batch_put and keeps these
 * descriptors so the kernel never re-parses headers:
 *   - body pointer (fixed-width array / dictionary index array)
 *   - null bitset words + a per-64-row prefix-sum of null counts, so
 *     nonNullPosition = prefix[row/64] + popcount(word & mask) is O(1) per
 *     row on the GPU (the reference decodes sequentially on the JVM —
 *     NullableDecoder, ColumnEncoding.scala:1069-1135 — which has no
 *     data-parallel analogue, hence the auxiliary prefix array)
 *   - delete mask re-expressed as a row bitmap
 *   - update deltas (ColumnDeltaDecoder/UpdatedColumnDecoder semantics)
 *     merged on host into a per-column sorted patch list applied by the
 *     kernel during the scan (deltas are small by construction:
 *     ColumnMaxDeltaRows=10000, Literals.scala:138-146)
 */
#ifndef SN_ENGINE_INTERNAL_H
#define SN_ENGINE_INTERNAL_H

#include <stdint.h>
#include <stdlib.h>

#include "../../include/snappy_engine.h"

/* bytes per value of a fixed-width column type; 0 for STRING */
static inline int sn_type_width(sn_type_t dtype) {
  switch (dtype) {
    case SN_TYPE_DOUBLE: case SN_TYPE_INT64: return 8;
    case SN_TYPE_INT32: case SN_TYPE_FLOAT: return 4;
    case SN_TYPE_INT16: return 2;
    case SN_TYPE_INT8: case SN_TYPE_BOOL: return 1;
    default: return 0;
  }
}

/* entries of a dense join LUT over the keys [mn, mx]: mx - mn + 1 when that
 * lies in [1, SN_LUT_MAX_SPAN], else 0 (no LUT: the probe walks the hash
 * table).  The difference is formed in uint64_t, where it is exact for every
 * int64 pair with mx >= mn; in int64 it wraps for spans past 2^63 and a
 * wrapped span can pass the bound. */
#define SN_LUT_MAX_SPAN (1ll << 24)
static inline int64_t sn_lut_span(int64_t mn, int64_t mx) {
  if (mx < mn) return 0;
  const uint64_t d = (uint64_t)mx - (uint64_t)mn;     /* span - 1 */
  return d < (uint64_t)SN_LUT_MAX_SPAN ? (int64_t)d + 1 : 0;
}

#define SN_DEV_MAX_COLS 8      /* referenced columns per plan */

/* column value kinds as seen by the kernel */
enum {
  SN_K_F64 = 0, SN_K_I32 = 1, SN_K_I64 = 2, SN_K_F32 = 3,
  SN_K_DICT16 = 4,   /* int16 dictionary index (group cols) */
  SN_K_DICT32 = 5,   /* int32 dictionary index (BigDictionary) */
  SN_K_I16 = 6, SN_K_BOOLBIT = 7,
  SN_K_U8 = 8,       /* uncompressed boolean byte body */
  SN_K_S8 = 9,       /* uncompressed int8 */
  SN_K_RLE = 10,     /* run-length: host-built run-ends + values aux */
  SN_K_RLE_I64 = 11, /* run-length over an INT64 column: rle_vals carry the
                        RAW int64 bits memcpy'd into doubles (the LDS-image
                        convention for i64), not numeric doubles.
                        (Int-typed DICTIONARY columns have no kernel kind:
                        the host materializes their values into a plain
                        fixed-width body at put — decompress-on-put, like
                        the LZ4 wrapper.) */
  SN_K_F64C8 = 12,   /* narrowed double: body = 1-byte codes (the put-time
                        sidecar, not the blob), rle_vals = the batch's value
                        dictionary of rle_n <= 256 doubles, value =
                        rle_vals[body[row]] — bit for bit the f64 body's */
  SN_K_F64_LATE = 13,/* JIT-only, never in a device descriptor (which keeps
                        SN_K_F64 and the same body): a double column that only
                        aggregate factors use, in a keyless plan whose
                        predicates keep few rows.  The compiled kernel does
                        not stage it; it reads it in the row phase, for the
                        rows that pass alone. */
  SN_K_F64_LATE_DIRECT = 14 /* JIT-only like SN_K_F64_LATE, and read the same
                        way; selects the image-free keyless kernel (DESIGN.md
                        §2d): the plan has range predicates only and every
                        other used column is SN_K_I32, SN_K_I16 or SN_K_F64C8 */
};

typedef struct {
  const void     *body;        /* fixed-width values / dict index array */
  const uint64_t *nullw;       /* null bitset words (NULL if none) */
  const uint32_t *nullpfx;     /* nulls in words [0, w) — host-built */
  const int32_t  *dictmap;     /* group col: local dict idx -> premultiplied
                                  global group contribution */
  /* update-delta patches (host-merged, sorted by row) */
  const uint64_t *patch_bm;    /* bitmap: row has patch */
  const int32_t  *patch_pos;   /* sorted patched rows */
  const double   *patch_val;   /* patched value (f64 or int bits in .i64) */
  const uint64_t *patch_nullbm;/* bitmap over patch index: patch writes NULL */
  /* RLE aux (host-extracted): cumulative run END positions (exclusive) and
   * run values widened to f64 (i64 raw-bitcast); kernel binary-searches the
   * run for each nonNullPosition (RunLengthEncoding.scala decodes
   * sequentially — no parallel analogue) */
  const int32_t *rle_ends;
  const double  *rle_vals;
  int32_t rle_n;
  int32_t patch_n;
  int32_t kind;
  int32_t has_nulls;
  int32_t null_gid;            /* group col: premultiplied global id of NULL */
} sn_dev_col;

typedef struct {
  int32_t num_rows;
  int32_t clean;               /* 1: no nulls/deletes/patches on any referenced
                                  col and all plain fixed-width -> fast path */
  const uint64_t *del_bm;      /* delete bitmap (NULL if none) */
  sn_dev_col cols[SN_DEV_MAX_COLS];
} sn_dev_batch;

typedef struct { int32_t batch; int32_t row_start; } sn_dev_tile;

/* Canonical (branchless) predicate: alive &= (lo <= x && x <= hi).
 * Strictness and missing bounds are folded by the host (nextafter for
 * strict double bounds, +-1 for strict integer bounds, +-inf when absent),
 * so the kernel does exactly two compares per predicate. */
typedef struct { double lo, hi; int32_t cslot; int32_t _p; } sn_dev_pred_d;
typedef struct { int64_t lo, hi; int32_t cslot; int32_t _p; } sn_dev_pred_i;

/* Canonical aggregate input: value = (a0+m0*x0)*(a1+m1*x1)*(a2+m2*x2) over
 * the first nf factors; the unused ones carry (a=1, m=0, c=c0) but are never
 * evaluated (0*x is NaN for a NaN or infinite x).  COUNT(*) has nf == 0 and
 * value 1.  nf also drives the general path's per-factor null checks.
 * op: 0 = sum-accumulate (SUM/AVG/COUNT),
 * 1 = MIN, 2 = MAX — min/max accumulators store the ORDER-PRESERVING u64
 * encoding (sn_f64_ord) so device atomics are integer atomicMin/Max;
 * k_reduce (dense) or the host (sparse readback) decodes. */
typedef struct {
  double a0, m0, a1, m1, a2, m2;
  int32_t c0, c1, c2;
  int32_t nf;                  /* real factors (0 for COUNT(*)) */
  int32_t op;
  int32_t _p2;
} sn_dev_agg;

/* order-preserving bijection double -> u64 (non-NaN): u64 min/max of the
 * encoding equals double min/max.  Identity elements: min = enc(+inf),
 * max = enc(-inf). */
static inline unsigned long long sn_f64_ord_h(double x) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
static inline double sn_ord_f64_h(unsigned long long o) {
  unsigned long long b = (o & 0x8000000000000000ull)
      ? (o ^ 0x8000000000000000ull) : ~o;
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}

typedef struct {
  int32_t npreds_d, npreds_i, naggs, ngroup;
  int32_t nslots, nused;
  uint32_t i64_mask;           /* bit c: cslot c is INT64 (raw bits in LDS) */
  int32_t gcol[2];
  /* broadcast-dimension probe (empty-slot sentinel key = INT64_MIN) */
  const int64_t *jkeys;        /* open-address key array (NULL = no join) */
  const int32_t *jpayload;     /* per-slot payload: dim attr gid (or 0) */
  int32_t jcap_log2;           /* table capacity = 1 << jcap_log2 */
  int32_t jcslot;              /* fact key column slot */
  int32_t jmode;               /* 0 semi, 1 group-by-dim-attr */
  int32_t jslot_mul;           /* >0: composite GROUP BY dim_attr, fact_col —
                                  slot = pay * jslot_mul + dense fact slot */
  /* dense probe LUT (built when the dim key span fits 16M entries):
   * pay = key in [jlut_min, jlut_max] ? jlut[key - jlut_min] : -1.
   * One dependent load per row instead of the open-address chain. */
  const int32_t *jlut;
  int64_t jlut_min, jlut_max;
  /* group slot formula: slot = ((v0 - gbase[0]) * gmul0) + (v1 - gbase[1]).
   * Dictionary key columns arrive premultiplied via dictmap (base 0, and
   * gmul0 folded into the map), integer key columns use their stats-derived
   * minimum as base and the second key's span as gmul0. */
  int64_t gbase[2];
  int32_t gmul0, _pad2;
  sn_dev_pred_d preds_d[8];
  sn_dev_pred_i preds_i[4];
  sn_dev_agg aggs[12];
  /* IN-list membership predicates: bitmap LUT over [base, base+nwords*64)
   * when the value span is dense enough (dictionary ids always are), else
   * a sorted list binary-searched per row (interpreted kernels only) */
  struct {
    const uint64_t *bm;
    const int64_t *list;
    int64_t base;
    int32_t nwords;
    int32_t n;
    int32_t cslot;
    int32_t _p;
  } inp[2];
  int32_t npreds_in;
  int32_t _pad4b;
  /* sparse-key open-address hash aggregate (the ByteBufferHashMap /
   * SHAMapAccessor analogue, ByteBufferHashMap.scala:140-183,
   * SHAMapAccessor.scala:716-830): integer group keys WITHOUT dense-slot
   * structure (int64 keys; int32/int16 spans beyond the dense cap or
   * without stats).  hkeys = open-address key array of 1<<hcap_log2
   * (sentinel SN_HASH_EMPTY = -1; a row whose key IS -1 lands in the
   * reserved row at index 1<<hcap_log2); hacc = accumulators
   * [(1<<hcap_log2)+1][naggs+1]; hflags[0] = overflow (table full — host
   * grows and relaunches).  ngroup==2 packs two 32-bit keys into one i64. */
  long long *hkeys;
  double *hacc;
  int32_t *hflags;
  int32_t hcap_log2;
  int32_t sparse;              /* 1: hash-aggregate mode */
  /* 1: per-agg counts — grouped accumulator rows widen to
   * [sums naggs][counts naggs][rowcount] because some aggregate input
   * column carries ACTUAL nulls (Spark Sum/Average skip null inputs,
   * SnappyHashAggregateExec.scala:450-500); 0 keeps [sums][rowcount] with
   * counts == rowcount (non-null inputs) */
  int32_t pac;
  int32_t _pad3;
  /* radix-partitioned two-pass hash aggregate (query-compiled pass 1 only;
   * big tables, clean batches).  Pass 1 scatters (key, agg values) records
   * into 1 << (hcap_log2 - SN_RADIX_SUB_LOG2) hash partitions instead of
   * probing the table; pass 2 (k_radix_agg) aggregates each partition into
   * its own 4096-slot SEGMENT of hkeys/hacc, so the probe + accumulate
   * working set per workgroup is ~100 KB and stays in the XCD's L2 instead
   * of thrashing HBM with 64 B random lines.  precs = record buffer
   * [npart][percap][(1+naggs) doubles] (slot 0 = key bits); pcount[npart]
   * fill counters; hflags[3] = partition overflow (host retries without
   * radix).  radix == 0 leaves the single-pass probe behavior. */
  double *precs;
  int32_t *pcount;
  int32_t percap;
  int32_t radix;
} sn_dev_plan;

/* radix partition shift (plan->radix): slots per partition table.
 * Swept on the 1M-key bench: sub 9 (512-slot LDS tables, 13 KB, high
 * occupancy) beat 10/11/12/13 at 25.7 / 24.9 / 21.2 / 17.0 / 6.5 Grows/s
 * — pass 2 wants occupancy, not bigger tables.  Clamped below so
 * npart = cap >> radix never exceeds the 4096 the pass-1 histogram
 * sizes for. */
#define SN_RADIX_SUB_MIN 9
#define SN_RADIX_NPART_MAX_LOG2 12
#define SN_RADIX_LDS_MAX (144u * 1024)
static inline unsigned sn_radix_lds_bytes(int sub_log2, int naggs1) {
  return (unsigned)((1u << sub_log2) * (8u + 8u * (unsigned)naggs1) +
                    256 /*WG*/ * 4u);
}
/* does pass 2 compact DIRECTLY from LDS (host then skips k_hash_compact)?
 * SN_RADIX_GLOB=1 forces the wide-row global-segment variant so its parity
 * is testable at small sizes (it otherwise only triggers at cap 2^24 with
 * 4 aggregates).  Shared by the host (compact decision) and the launcher
 * (kernel choice) so the two can never disagree. */
static inline int sn_radix_direct(int sub_log2, int naggs1) {
  const char *fg = getenv("SN_RADIX_GLOB");
  if (fg && fg[0] == '1') return 0;
  return sn_radix_lds_bytes(sub_log2, naggs1) <= SN_RADIX_LDS_MAX;
}

/* sparse hash-aggregate empty-slot sentinel: -1 so the host can memset the
 * key array (a REAL key of -1 routes to the reserved row at index cap) */
#define SN_HASH_EMPTY (-1ll)

#define SN_SCAN_CHUNK 1024     /* rows per LDS conversion chunk (kernels.hip) */

/* ---- exact DECIMAL aggregation (k_dec_keyless / k_dec_grouped) ----
 * Canonical decimal aggregate input: value = f0*f1*f2 with
 * f_i = add[i] + mul[i]*x_i formed in int64 (the host proves no int64 wrap
 * from the declared precision) and the product formed in 128 bits.
 * op: 0 = sum-accumulate (SUM/AVG), 1 = MIN, 2 = MAX (exactly one factor). */
typedef struct {
  int64_t add[3], mul[3];
  int32_t c[3];
  int32_t nf;
  int32_t op;
  int32_t _p;
} sn_dev_dec_agg;

typedef struct {
  int32_t naggs, _p;
  sn_dev_dec_agg aggs[12];
} sn_dev_dec_plan;

/* accumulator cells (u64) per aggregate:
 *   [0..2] sum as a 192-bit two's-complement integer (lo, mid, hi limb) —
 *          MIN/MAX keep the sign-biased value (v ^ 2^63) in cell 0
 *   [3]    contributing (all-factors-non-null) row count
 *   [4]    rows whose |product| reached 10^38 (group result becomes NULL)
 * and one trailing surviving-row count per slot. */
#define SN_DEC_CELLS 5
#define SN_DEC_ROW_CELLS(naggs) ((naggs) * SN_DEC_CELLS + 1)   /* device-usable */
static inline int sn_dec_row_cells(int naggs) {
  return SN_DEC_ROW_CELLS(naggs);
}
#define SN_DEC_GRID_CAP 512   /* blocks (scratch rows) of a decimal scan */

#define SN_GRID_CAP 2048
#define SN_RESULT_PAGE 1024      /* == SN_MAX_GROUP_SLOTS (result page) */
#define SN_BIG_GROUP_CAP (1 << 20) /* dense-slot cap of the global-atomic
                                      grouped path (>SN_RESULT_PAGE) */
#define SN_GRID_BIGSLOT 256   /* grid cap for the >16-slot LDS hash-agg path */
#define SN_TILE_ROWS 16384     /* rows per workgroup tile (16 LDS chunks;
                                  long pipelines for the staged conversion) */

#ifdef __HIP__
#define SN_HD __host__ __device__
#else
#define SN_HD
#endif

/* ---- the scan kernels' dynamic-LDS layout, for kernels and host alike ----
 * Every scan kernel stages one chunk of each referenced column into the same
 * image and carves its pointers from sn_lds_layout; every launcher and
 * routing predicate takes its byte count from the same call, so a kernel and
 * its launcher cannot disagree on an offset or a size.  Regions, in order:
 *   sval    [nused][CHUNK] f64 values (offset 0)
 *   svalid  [nused][CHUNK/64] validity words
 *   sdead   [CHUNK/64], salive [CHUNK/64]
 *   sslot   [CHUNK] int16 per-row slot image          (slot_image only)
 *   plan    sn_dev_plan mirror, then plan2 = any further mirror
 *   acc     the block accumulator
 *   slack   unused tail
 * LDS bytes decide occupancy, the 160 KiB rejections and the LDS-versus-
 * global routing, so each kernel's historical pad is kept as a named slack
 * constant instead of being trimmed. */
#define SN_LDS_LIMIT (160ull * 1024)
#define SN_LDS_BITMAP (SN_SCAN_CHUNK / 64 * 8)      /* one row bitmap */
#define SN_LDS_SLOT_IMAGE (SN_SCAN_CHUNK * 2)
#define SN_LDS_KEYLESS_ACC 512  /* k_keyless block row, 2 * 12 + 1 doubles */
#define SN_LDS_SLACK_GROUPED (512 + SN_LDS_BITMAP + 16)
#define SN_LDS_SLACK_LDS (512 + SN_LDS_BITMAP + 64)    /* also k_grouped_reg */
#define SN_LDS_SLACK_GLOBAL (SN_LDS_SLACK_LDS + sizeof(sn_dev_plan))
#define SN_LDS_SLACK_HASH 64                           /* also k_join_build */
#define SN_LDS_SLACK_DEC 16
#define SN_REG_SLOTS 8          /* k_grouped_reg's slot capacity */

typedef struct {
  unsigned svalid, sdead, salive, sslot, plan, plan2, acc;  /* byte offsets */
  unsigned long long total;
} sn_lds;

static inline SN_HD sn_lds sn_lds_layout(int nused, int slot_image,
                                         unsigned mirror_bytes,
                                         unsigned long long acc_bytes,
                                         unsigned long long slack) {
  sn_lds l;
  l.svalid = (unsigned)nused * SN_SCAN_CHUNK * 8;
  l.sdead = l.svalid + (unsigned)nused * SN_LDS_BITMAP;
  l.salive = l.sdead + SN_LDS_BITMAP;
  l.sslot = l.salive + SN_LDS_BITMAP;
  l.plan = l.sslot + (slot_image ? SN_LDS_SLOT_IMAGE : 0);
  l.plan2 = l.plan + (unsigned)sizeof(sn_dev_plan);
  l.acc = l.plan + mirror_bytes;
  l.total = l.acc + acc_bytes + slack;
  return l;
}

/* template roundings: aggregate capacity of the keyless kernels (also the
 * result stride), slot capacity of k_grouped */
static inline SN_HD int sn_na_t(int na) {
  return na <= 2 ? 2 : na <= 4 ? 4 : na <= 8 ? 8 : 12;
}
static inline SN_HD int sn_grouped_ns_t(int ns) {
  return ns <= 4 ? 4 : ns <= 8 ? 8 : 16;
}

static inline SN_HD sn_lds sn_lds_keyless(int nused) {
  return sn_lds_layout(nused, 0, sizeof(sn_dev_plan), SN_LDS_KEYLESS_ACC, 0);
}
/* acc [ns_t][naggs + 1]: ns_t is the kernel's template slot capacity */
static inline SN_HD sn_lds sn_lds_grouped(int nused, int ns_t, int naggs) {
  return sn_lds_layout(nused, 1, sizeof(sn_dev_plan),
                       (unsigned long long)ns_t * (naggs + 1) * 8,
                       SN_LDS_SLACK_GROUPED);
}
static inline SN_HD sn_lds sn_lds_grouped_lds(int nused, int nslots, int na1) {
  return sn_lds_layout(nused, 1, sizeof(sn_dev_plan),
                       (unsigned long long)nslots * na1 * 8, SN_LDS_SLACK_LDS);
}
static inline SN_HD sn_lds sn_lds_grouped_reg(int nused, int naggs) {
  return sn_lds_layout(nused, 0, sizeof(sn_dev_plan),
                       (unsigned long long)SN_REG_SLOTS * (naggs + 1) * 8,
                       SN_LDS_SLACK_LDS);
}
static inline SN_HD sn_lds sn_lds_grouped_global(int nused) {
  return sn_lds_layout(nused, 1, sizeof(sn_dev_plan), 0, SN_LDS_SLACK_GLOBAL);
}
static inline SN_HD sn_lds sn_lds_hash(int nused) {
  return sn_lds_layout(nused, 0, sizeof(sn_dev_plan), 0, SN_LDS_SLACK_HASH);
}
static inline SN_HD sn_lds sn_lds_join_build(int nused) {
  return sn_lds_layout(nused, 0, 0, 0, SN_LDS_SLACK_HASH);
}
/* decimal kernels: both plan mirrors; acc = nslots accumulator rows
 * (keyless: one) plus the keyless kernel's four per-wave partial rows */
static inline SN_HD sn_lds sn_lds_dec(int nused, int nslots, int naggs) {
  return sn_lds_layout(nused, 0, sizeof(sn_dev_plan) + sizeof(sn_dev_dec_plan),
                       ((unsigned long long)nslots + 4) *
                           SN_DEC_ROW_CELLS(naggs) * 8,
                       SN_LDS_SLACK_DEC);
}

/* row-returning scan, pass 1 (k_select_mark): the plan mirror only */
static inline SN_HD sn_lds sn_lds_select(int nused) {
  return sn_lds_layout(nused, 0, sizeof(sn_dev_plan), 0, 0);
}

/* does the grouped LDS-accumulator kernel fit, or must the plan take the
 * global-atomic route?  Asked by the launcher and by the engine, which must
 * zero the global accumulator before launch. */
static inline int sn_grouped_needs_global(int nused, int nslots, int na1) {
  return sn_lds_grouped_lds(nused, nslots, na1).total > SN_LDS_LIMIT;
}

static inline unsigned long long sn_dec_lds_bytes(int nused, int nslots,
                                                  int naggs) {
  return sn_lds_dec(nused, nslots, naggs).total;
}
/* largest dense slot count the decimal grouped kernel admits (160 KiB LDS) */
static inline int sn_dec_max_slots(int nused, int naggs) {
  const unsigned long long fixed = sn_dec_lds_bytes(nused, 0, naggs);
  if (fixed >= SN_LDS_LIMIT) return 0;
  return (int)((SN_LDS_LIMIT - fixed) /
               ((unsigned long long)sn_dec_row_cells(naggs) * 8));
}
/* replication factor of the grouped LDS accumulator (lane l updates copy
 * l % copies, so few-group shapes do not serialize a whole wave on one LDS
 * address): the largest power of two <= 16 that keeps a block within half
 * the CU's LDS (two resident blocks), or within all of it when one copy
 * already needs more than half. */
static inline int sn_dec_copies(int nused, int nslots, int naggs) {
  const unsigned long long budget =
      sn_dec_lds_bytes(nused, nslots, naggs) <= SN_LDS_LIMIT / 2
          ? SN_LDS_LIMIT / 2 : SN_LDS_LIMIT;
  int c = 1;
  while (c < 16 && sn_dec_lds_bytes(nused, nslots * c * 2, naggs) <= budget)
    c *= 2;
  return c;
}

/* ---- launch geometry ---- */

/* every block gets the same tile count (a ragged grid-stride leaves half the
 * blocks with 2x work and CUs idle in the tail) */
static inline int sn_balanced_grid(int ntiles, int cap) {
  if (ntiles <= cap) return ntiles;
  const int rounds = (ntiles + cap - 1) / cap;
  return (ntiles + rounds - 1) / rounds;
}

/* one dense (keyless or direct-slot grouped) launch, as sn_launch_scan_agg
 * performs it and as the engine sizes scratch and folds partials for it */
enum {
  SN_ROUTE_KEYLESS,   /* k_keyless */
  SN_ROUTE_GLOBAL,    /* k_grouped_global: unbounded cardinality, or a pac
                         accumulator too wide for LDS */
  SN_ROUTE_LDS,       /* k_grouped_lds: > 16 slots, or per-agg counts */
  SN_ROUTE_REG,       /* k_grouped_reg: Q1's shape */
  SN_ROUTE_GROUPED    /* k_grouped */
};
typedef struct {
  int route;
  int grid;           /* blocks of the interpreted kernel */
  int grid_compiled;  /* blocks of the query-compiled twin */
  int global_acc;     /* accumulates into 8 XCD-private global copies (the
                         caller zeroes them) instead of per-block rows */
  int na_t, na1;      /* template aggregate count; accumulator row width */
  int nv;             /* doubles per partial row */
  int naggs1;         /* k_reduce row width (0: keyless layout) */
  int out_stride;
  unsigned long long lds;
} sn_dense_launch;

/* partial rows k_reduce folds == rows the scratch buffer must hold */
static inline int sn_dense_rows(const sn_dense_launch *d, int compiled) {
  return d->global_acc ? 8 : compiled ? d->grid_compiled : d->grid;
}

static inline sn_dense_launch sn_dense_launch_of(const sn_dev_plan *p,
                                                 int ntiles) {
  sn_dense_launch d;
  const int ns = p->nslots, na = p->naggs, nused = p->nused;
  d.na_t = sn_na_t(na);
  d.na1 = p->pac ? 2 * na + 1 : na + 1;
  d.out_stride = 2 * d.na_t + 1;
  d.grid = ntiles <= 0 ? 1 : sn_balanced_grid(ntiles, SN_GRID_CAP);
  /* > 16-slot partial rows are wide: the grid cap keeps scratch small */
  d.grid_compiled = ns > 16 && d.grid > SN_GRID_BIGSLOT ? SN_GRID_BIGSLOT
                                                        : d.grid;
  d.global_acc = 0;
  if (ns <= 1 && !p->pac) {
    d.route = SN_ROUTE_KEYLESS;
    d.nv = d.out_stride; d.naggs1 = 0;
    d.lds = sn_lds_keyless(nused).total;
    return d;
  }
  /* grouped layout (also keyless MIN/MAX plans routed through the grouped
   * kernels with one slot) */
  d.nv = (ns < 1 ? 1 : ns) * d.na1; d.naggs1 = d.na1;
  if (ns > SN_RESULT_PAGE ||
      (p->pac && sn_grouped_needs_global(nused, ns, d.na1))) {
    d.route = SN_ROUTE_GLOBAL;
    d.global_acc = 1;
    d.lds = sn_lds_grouped_global(nused).total;
  } else if (ns > 16 || p->pac) {
    d.route = SN_ROUTE_LDS;
    if (d.grid > SN_GRID_BIGSLOT) d.grid = SN_GRID_BIGSLOT;
    d.lds = sn_lds_grouped_lds(nused, ns, d.na1).total;
  } else if (p->jmode != 1 && ns <= SN_REG_SLOTS && na <= 6) {
    d.route = SN_ROUTE_REG;
    d.lds = sn_lds_grouped_reg(nused, na).total;
  } else {
    d.route = SN_ROUTE_GROUPED;
    d.lds = sn_lds_grouped(nused, sn_grouped_ns_t(ns), na).total;
  }
  return d;
}

#ifdef __cplusplus
extern "C" {
#endif

/* launches the scan+filter+aggregate over all tiles.
 * out: device array [nslots][naggs+1] doubles (last = group row count),
 * zeroed by caller.  Returns hipError_t as int. */
int sn_launch_scan_agg(const sn_dev_plan *plan,
                       const sn_dev_plan *dev_plan,  /* device copy (LDS mirror source) */
                       const sn_dev_batch *dev_batches,
                       const sn_dev_tile *dev_tiles, int32_t ntiles,
                       double *dev_out,
                       double *dev_scratch,  /* >= sn_dense_rows x nv doubles */
                       void *stream);

/* exact decimal scan+filter+aggregate: block partials into dev_scratch
 * (>= min(ntiles, SN_DEC_GRID_CAP) rows of nslots * sn_dec_row_cells u64),
 * folded with carries into dev_out [nslots][sn_dec_row_cells].  plan->nslots
 * <= 1 with ngroup == 0 runs the register-accumulator keyless kernel. */
int sn_launch_dec_scan(const sn_dev_plan *plan, const sn_dev_plan *dev_plan,
                       const sn_dev_dec_plan *dec,
                       const sn_dev_dec_plan *dev_dec,
                       const sn_dev_batch *dev_batches,
                       const sn_dev_tile *dev_tiles, int32_t ntiles,
                       unsigned long long *dev_out,
                       unsigned long long *dev_scratch, void *stream);

/* ---- row-returning filter scan (sn_scan_submit): mark, offsets, gather ----
 * Pass 1 leaves one alive bit per scanned row, tile-major: tile t owns the
 * SN_SEL_TILE_WORDS 64-bit words from t * SN_SEL_TILE_WORDS, chunk c of the
 * tile the SN_SCAN_CHUNK / 64 words from c * (SN_SCAN_CHUNK / 64); bit r of
 * word w is row tile.row_start + c * SN_SCAN_CHUNK + w * 64 + r.  Words of
 * chunks beyond the tile's last row are never written and never read. */
#define SN_SEL_TILE_WORDS (SN_TILE_ROWS / 64)
#define SN_SEL_MAX_PROJ 8
#define SN_SEL_ROWID 8         /* otype of the ROWID pseudo-column (sn_type_t
                                  values are 0..7) */
#define SN_SEL_DIM_ATTR 9      /* otype of the joined dimension row's attribute
                                  (sn_scan_submit_join): int32 attribute id,
                                  validity 0 where the row did not join */
typedef struct {
  int32_t nproj, _p;
  int64_t out_rows;            /* min(matching rows, limit): every store is
                                  guarded by it */
  int32_t cslot[SN_SEL_MAX_PROJ];   /* device column slot (unused for ROWID) */
  int32_t otype[SN_SEL_MAX_PROJ];   /* sn_type_t of the output, ROWID or
                                       DIM_ATTR */
  void *val[SN_SEL_MAX_PROJ];       /* dense typed output array */
  uint8_t *valid[SN_SEL_MAX_PROJ];  /* one validity byte per output row */
  /* the dimension a DIM_ATTR projection probes (sn_dev_plan's j* fields; all
   * zero without one): pass 2 reads the row's key again and looks it up,
   * instead of pass 1 writing 4 B of payload for every scanned row */
  int32_t jcslot;              /* device column slot of the fact key */
  int32_t jis64;               /* the key column is INT64 */
  int32_t jcap_log2, _pj;
  const int64_t *jkeys;
  const int32_t *jpayload;
  const int32_t *jlut;
  int64_t jlut_min, jlut_max;
} sn_dev_select;

/* pass 1's join step (k_select_mark): none, alive &= joined, alive &= ~joined */
#define SN_MARK_NOJOIN 0
#define SN_MARK_INNER  1
#define SN_MARK_ANTI   2

/* pass 1: plan->nused must be the number of PREDICATE column slots (they come
 * first in the descriptor set); counts[ntiles] zeroed by the caller */
int sn_launch_select_mark(const sn_dev_plan *plan, const sn_dev_plan *dev_plan,
                          const sn_dev_batch *dev_batches,
                          const sn_dev_tile *dev_tiles, int32_t ntiles,
                          uint64_t *bitmap, int32_t *counts, void *stream);
/* pass 1 of a join scan (INNER, LEFT_ANTI): the fact key column is one of the
 * staged slots (plan->jcslot < plan->nused) and plan->jkeys is set; after the
 * predicates, the rows still alive are looked up and kept (SN_MARK_INNER) or
 * dropped (SN_MARK_ANTI) when their key is NOT NULL and a dimension key */
int sn_launch_select_mark_join(const sn_dev_plan *plan,
                               const sn_dev_plan *dev_plan,
                               const sn_dev_batch *dev_batches,
                               const sn_dev_tile *dev_tiles, int32_t ntiles,
                               int32_t mark, uint64_t *bitmap, int32_t *counts,
                               void *stream);
/* offsets[i] = counts[0] + ... + counts[i-1] in 64 bits, *total = the sum;
 * one workgroup, any n >= 0 */
int sn_launch_tile_offsets(const int32_t *counts, int32_t n, int64_t *offsets,
                           int64_t *total, void *stream);
/* pass 2: table_batch[scan-set batch] = the table's own batch index */
int sn_launch_select_gather(const sn_dev_select *sel,
                            const sn_dev_batch *dev_batches,
                            const sn_dev_tile *dev_tiles, int32_t ntiles,
                            const uint64_t *bitmap, const int32_t *counts,
                            const int64_t *offsets, const int32_t *table_batch,
                            void *stream);

/* ---- ordered row scan (sn_scan_submit_ordered): ORDER BY key LIMIT k ----
 * After mark + offsets, a radix select over the alive rows' key images finds
 * the k-th smallest (the threshold T), a quota pass takes the rows below T
 * and the first `need` rows equal to T in scan order, one workgroup sorts the
 * k candidates and a gather projects them in that order.
 *
 * Key image: (class, u64).  class orders NULLs against values — NULLS FIRST
 * rows are class 0, values class 1, NULLS LAST rows class 2 — and the u64 is
 * an order-preserving map of the value, complemented for DESC; a NULL's u64
 * is 0.  Images compare as (class, u64); rows whose images are equal keep
 * their scan order. */
#define SN_ORD_DIGIT_BITS 11
#define SN_ORD_BINS (1 << SN_ORD_DIGIT_BITS)
/* one pass's histogram: [0] the NULLS FIRST class, [1 + d] digit d,
 * [SN_ORD_BINS + 1] the NULLS LAST class — bin order is image order */
#define SN_ORD_HIST (SN_ORD_BINS + 2)
#define SN_ORD_MAX_PASSES 6
#define SN_ORD_CLS_FIRST 0
#define SN_ORD_CLS_VALUE 1
#define SN_ORD_CLS_LAST 2
#define SN_ORD_CLS_PAD 3       /* k_order_sort's padding, above everything */
#define SN_ORD_POS_MASK 0x3fffffffffffffffull

/* a candidate row: cp = class << 62 | scan-set batch << 32 | row ordinal
 * (batch < 2^30, row < 2^31), so entries order as (cp >> 62, key, cp) */
typedef struct { uint64_t key; uint64_t cp; } sn_order_ent;

/* device state of one ordered scan: k_order_pick extends `prefix` by a digit
 * per pass and lowers `need` to the rank wanted inside the chosen bin; after
 * the last pass (cls, prefix) is T and need the quota of rows equal to T */
typedef struct {
  uint64_t prefix;
  int64_t need;
  int32_t cls;                 /* class of T, fixed by pass 0 */
  int32_t cursor;              /* candidates appended so far */
} sn_order_state;

typedef struct {
  int32_t cslot;               /* device column slot of the key */
  int32_t dtype;               /* sn_type_t of the key column */
  int32_t desc;
  int32_t null_cls;            /* SN_ORD_CLS_FIRST or SN_ORD_CLS_LAST */
  int32_t npass;               /* ceil(key bits / 11) */
  int32_t nranks;              /* STRING: entries of ranks */
  const int32_t *ranks;        /* STRING: global dictionary id -> bytewise rank */
} sn_dev_order;

static inline SN_HD int sn_order_key_bits(int dtype) {
  switch (dtype) {
    case SN_TYPE_DOUBLE: case SN_TYPE_INT64: return 64;
    case SN_TYPE_INT32: case SN_TYPE_FLOAT: case SN_TYPE_STRING: return 32;
    case SN_TYPE_INT16: return 16;
    case SN_TYPE_INT8: return 8;
    default: return 1;         /* BOOL */
  }
}
static inline SN_HD int sn_order_passes(int dtype) {
  return (sn_order_key_bits(dtype) + SN_ORD_DIGIT_BITS - 1) / SN_ORD_DIGIT_BITS;
}

/* the u64 of a non-NULL key.  vi: the integer value (sign-extended), the f64
 * bit pattern, the STRING's rank or the BOOL as 0/1; fbits: the f32 pattern.
 * Floats order as Spark's nanSafeCompare: -0.0 folds to 0.0 and every NaN to
 * one pattern above +inf, then the sn_f64_ord map.  Integers get a sign bias.
 * DESC complements within the key width. */
static inline SN_HD unsigned long long sn_order_image(int dtype, long long vi,
                                                      unsigned fbits, int desc) {
  unsigned long long k;
  switch (dtype) {
    case SN_TYPE_DOUBLE: {
      unsigned long long b = (unsigned long long)vi;
      if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
        b = 0x7ff8000000000000ull;
      else if (b == 0x8000000000000000ull) b = 0;
      k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
      break;
    }
    case SN_TYPE_FLOAT: {
      unsigned b = fbits;
      if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
      else if (b == 0x80000000u) b = 0;
      k = (b >> 31) ? (unsigned)~b : (b | 0x80000000u);
      break;
    }
    case SN_TYPE_INT64: k = (unsigned long long)vi ^ 0x8000000000000000ull; break;
    case SN_TYPE_INT32: k = (unsigned)(int32_t)vi ^ 0x80000000u; break;
    case SN_TYPE_STRING: k = (unsigned)(int32_t)vi; break;
    case SN_TYPE_INT16: k = (unsigned)((uint16_t)(int16_t)vi ^ 0x8000u); break;
    case SN_TYPE_INT8: k = (unsigned)((uint8_t)(int8_t)vi ^ 0x80u); break;
    default: k = vi != 0; break;
  }
  if (desc) {
    const int bits = sn_order_key_bits(dtype);
    k ^= bits == 64 ? ~0ull : ((1ull << bits) - 1ull);
  }
  return k;
}

/* the whole order stage but the sort and the gather, on `stream` with no host
 * sync: npass x (k_order_hist, k_order_pick), k_order_count, k_tile_offsets
 * over the equal counts, k_order_collect.  bitmap / counts are pass 1's.
 * The caller zeroes state, hist [npass][SN_ORD_HIST] and eq_counts [ntiles];
 * cand holds k_eff entries, 1 <= k_eff <= min(alive rows, SN_ORDER_MAX_LIMIT),
 * and is filled completely, in no particular order. */
int sn_launch_order_select(const sn_dev_order *od,
                           const sn_dev_batch *dev_batches,
                           const sn_dev_tile *dev_tiles, int32_t ntiles,
                           const uint64_t *bitmap, const int32_t *counts,
                           sn_order_state *state, unsigned long long *hist,
                           int32_t *eq_counts, int64_t *eq_offsets,
                           int64_t *eq_total, sn_order_ent *cand,
                           int32_t k_eff, void *stream);
/* sorts ents[0, n) in place by (class, key, position), 0 <= n <=
 * SN_ORDER_MAX_LIMIT: one workgroup, a bitonic network in LDS */
int sn_launch_order_sort(sn_order_ent *ents, int32_t n, void *stream);
/* output row j = candidate j, every projection through select_emit */
int sn_launch_order_gather(const sn_dev_select *sel,
                           const sn_dev_batch *dev_batches,
                           const sn_order_ent *cand,
                           const int32_t *table_batch, void *stream);

/* put-time patch materialization into a null-free fixed-width device body */
int sn_launch_patch_apply(void *body, const int32_t *pos, const double *val,
                          int n, int kind, void *stream);

/* sparse-key open-address hash aggregate: scan into plan->hkeys/hacc, then
 * compact the used rows into (key, accumulator-row) pairs for readback */
int sn_launch_hash_scan(const sn_dev_plan *plan, const sn_dev_plan *dev_plan,
                        const sn_dev_batch *dev_batches,
                        const sn_dev_tile *dev_tiles, int32_t ntiles,
                        void *stream);
int sn_launch_hash_compact(const long long *hk, const double *hacc,
                           int cap, int naggs1, long long *okeys,
                           double *orows, int *counter, void *stream);

/* radix pass 2: aggregate each partition's records in an LDS table and
 * compact straight into (okeys, orows) — or, for rows too wide for LDS,
 * into per-partition segments of the global table (host runs
 * k_hash_compact as usual; sn_radix_direct says which) */
int sn_launch_radix_agg(const sn_dev_plan *plan, const sn_dev_plan *dev_plan,
                        long long *okeys, double *orows, int *counter,
                        void *stream);

/* device-side join-table build from a column table (colocated
 * partitioned-partitioned join): fills an open-address (key, payload)
 * table in the probe_sweep layout; optional LUT densification */
int sn_launch_join_build(const sn_dev_plan *plan, const sn_dev_plan *dev_plan,
                         const sn_dev_batch *dev_batches,
                         const sn_dev_tile *dev_tiles, int32_t ntiles,
                         long long *hk, int32_t *hp, int cap_log2,
                         int has_attr, int32_t *flags, void *stream);
/* lut covers [lmin, lmax]; a table key outside it is not written and sets
 * oob[0] (one zeroed device word), so bounds the build keys do not honour
 * cost the LUT, never memory */
int sn_launch_hash_to_lut(const long long *hk, const int32_t *hp,
                          long long cap, int32_t *lut, long long lmin,
                          long long lmax, int32_t *oob, void *stream);

/* wave-cooperative raw LZ4 block decode (f1 compressed-upload ingest);
 * err[0]: 0 ok, 1 malformed, 2 length mismatch */
int sn_launch_lz4_decompress(const void *src, long long slen, void *dst,
                             long long dlen, int32_t *err, void *stream);

/* f2: device min/max over one raw fixed-width column; omin memset 0xFF,
 * omax memset 0x00 (values land as order-preserving u64 encodings:
 * f64 ord / integer sign-bias) */
int sn_launch_col_minmax(const void *body, long long n, int kind,
                         unsigned long long *omin, unsigned long long *omax,
                         void *stream);

/* put-time narrowing of one null-free f64 body into 1-byte codes and a
 * dictionary of at most SN_NARROW_MAX doubles; async on `stream`, no host
 * sync.  Values are told apart by their 64-bit pattern (-0.0 and +0.0, and
 * every NaN payload, are entries of their own).
 *   fits:     dict[0..*ndict) = the distinct patterns ascending as unsigned
 *             64-bit integers, dict[*ndict..256) = 0, codes[i] = index of
 *             body[i]'s pattern;
 *   overflow: (> 256 patterns) *ndict = -1, dict[0..256) = 0, codes untouched
 *             — the encode kernel reads *ndict on device and returns.
 * Writes nothing outside [codes, codes + n), dict[0..256) and *ndict.
 * sn_f64_narrow_host (snappy_engine.h) is the same contract in plain C++. */
#define SN_NARROW_MAX 256
int sn_launch_f64_narrow(const double *body, long long n, unsigned char *codes,
                         double *dict, int *ndict, void *stream);

/* launches only the partial-fold (k_reduce): scratch[nblocks][nv] -> out.
 * Used by the JIT path, whose scan kernel writes the same scratch rows.
 * plan_dev (nullable) supplies per-agg ops for MIN/MAX folding. */
int sn_launch_reduce(const double *dev_scratch, int nblocks, int nv,
                     double *dev_out, int naggs1, int out_stride,
                     const void *plan_dev, void *stream);

/* initialize a global accumulator's MIN/MAX cells to their ord-encoding
 * identities (rows x na1 cells; sum/count cells keep the host's memset 0) */
int sn_launch_acc_init(double *acc, long long rows, int naggs, int na1,
                       const void *plan_dev, void *stream);

/* query-compiled scan kernels (jit.cpp, hipRTC).  sn_jit_get returns an
 * opaque hipFunction_t for the plan (compiling + caching on first use) or
 * NULL -> caller falls back to the interpreted kernels. */
/* does a plan of this shape (nused, nslots, naggs, pac, sparse) fit a
 * query-compiled kernel?  The slot, aggregate and LDS limits live next to
 * the generator's mode classifier, so the host's routing and the generated
 * kernel can never disagree. */
int sn_jit_shape_ok(const sn_dev_plan *p);
void *sn_jit_cache_create(void);
void sn_jit_cache_destroy(void *cache);
int sn_jit_cache_count(void *cache);
void *sn_jit_get(void *cache, const sn_dev_plan *p, const int *kinds,
                 int nslots, int na_t, int has_del);
/* how many blocks of a kernel sn_jit_get returned the device holds at once
 * (blocks per CU by the runtime's occupancy query x CUs); 0 when unknown */
int sn_jit_resident(void *cache, void *fn);
int sn_jit_launch(void *fn, int grid, const sn_dev_batch *batches,
                  const sn_dev_tile *tiles, int ntiles, double *scratch,
                  const int64_t *jkeys, const int32_t *jpayload,
                  const int32_t *jlut, const sn_dev_plan *plan_dev,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif
