/*
 * jit.cpp — query-compiled scan kernels via hipRTC.
 *
 * The MI355X-native analogue of the reference's WholeStageCodegen
 * (SnappySession.scala:2388-2460 compiles one Java class per query stage;
 * here one gfx950 kernel per plan signature).  Motivation is measured, not
 * aesthetic: a probe kernel with Q1's exact shape and the plan constants
 * compile-time reaches 5.7 TB/s, while the best runtime-plan kernel stops at
 * 1.76 TB/s — literal predicates/aggregates let the compiler
 * CSE shared factors, keep every parameter in registers and emit zero
 * uniform branches in the row loop.
 *
 * Scope: plans whose unskipped batches are all CLEAN (no nulls, deletes or
 * patches) with uniform stageable column kinds, <= 4 double predicates, no
 * join, dictionary-slot or keyless grouping.  Everything else falls back to
 * the interpreted kernels (still GPU — never CPU).
 *
 * Compiled modules cache per engine by plan SHAPE: predicate bounds and
 * aggregate coefficients are tokenized (read from the cached device plan
 * at run time), so different literal values of the same shape reuse one
 * compiled kernel — the reference's ParamLiteral tokenization.
 *
 * Layout of this file: the shape classifier (JitShape: which accumulator,
 * join-probe and slot scheme a plan gets, and the limits the engine asks
 * about), the column-kind table, one emitter per piece of the kernel, and
 * gen_source, which strings the emitters together in kernel order.
 */
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"

struct JitFn {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int resident = 0;   /* blocks of fn the device holds at once; 0 = unknown */
};

struct JitCache {
  std::map<uint64_t, JitFn> fns;
  std::mutex mu;
};

extern "C" void *sn_jit_cache_create(void) { return new JitCache(); }
extern "C" void sn_jit_cache_destroy(void *c) {
  auto *jc = (JitCache *)c;
  if (!jc) return;
  for (auto &kv : jc->fns)
    if (kv.second.mod) (void)hipModuleUnload(kv.second.mod);
  delete jc;
}

/* printf into a string: sized by a first pass, so no line can truncate */
__attribute__((format(printf, 1, 2)))
static std::string strf(const char *fmt, ...) {
  va_list ap, ap2;
  va_start(ap, fmt);
  va_copy(ap2, ap);
  const int n = vsnprintf(nullptr, 0, fmt, ap);
  va_end(ap);
  std::string s(n > 0 ? (size_t)n + 1 : 0, '\0');
  if (n > 0) vsnprintf(&s[0], s.size(), fmt, ap2), s.resize((size_t)n);
  va_end(ap2);
  return s;
}
#define emitf(o, ...) ((o) += strf(__VA_ARGS__))

/* ---- plan shape ---------------------------------------------------------
 * Everything the emitters branch on, decided once. */

#define JIT_CHUNK 1024          /* rows per LDS image chunk */
#define JIT_WG 256
#define JIT_DIRECT_SLOTS 8      /* rows per lane and step of the direct kernel */
#define JIT_MAX_AGGS 12         /* sn_dev_plan.aggs */
#define JIT_REG_MAX_SLOTS 8     /* most slots the per-lane registers carry */
#define JIT_REG_MAX_AGGS 6      /* ... and most aggregates per slot */
#define JIT_LDS_MAX_SLOTS 1024  /* most slots of the block LDS accumulator */
#define JIT_LDS_BUDGET (160 * 1024)   /* static LDS of one workgroup */
#define JIT_SLUT_MAX_BYTES (100 * 1024)

/* where a surviving row's aggregate values go — exactly one per kernel */
enum JitAcc {
  ACC_KEYLESS,   /* per-lane registers, no slots: [sums][counts][rowcount] */
  ACC_REGS,      /* per-lane registers per slot, slot-predicated fma */
  ACC_WBIN,      /* 16 LDS bins of 16 lanes each */
  ACC_LDS,       /* one block-level LDS accumulator */
  ACC_GLOBAL,    /* HBM accumulator, privatised 8 ways by XCD */
  ACC_SPARSE,    /* open-address hash table in HBM, probed per row */
  ACC_RADIX      /* pass 1 of the radix two-pass: scatter records */
};

/* how a fact row finds its broadcast-dimension payload */
enum JitProbe {
  PROBE_NONE,
  PROBE_HASH,    /* open-address chain in global memory */
  PROBE_SPAY,    /* dense int32 LUT, probed from the staged registers */
  PROBE_SLUT     /* dense LUT packed into 4-bit LDS nibbles */
};

/* how a row's accumulator slot is computed */
enum JitSlot {
  SLOT_NONE,          /* keyless */
  SLOT_SINGLE,        /* keyless plan in the grouped (pac) layout */
  SLOT_DENSE,         /* (v0 - base0) * mul0 + (v1 - base1) */
  SLOT_JOIN_ATTR,     /* the join payload (times jslot_mul + fact slot) */
  SLOT_SPARSE_PROBE,  /* position in the hash table */
  SLOT_RADIX_RANK     /* (partition, rank) in the chunk's histogram */
};

struct JitShape {
  int NC, NA;        /* used columns, aggregates */
  int NS, NA1;       /* slots (>= 1), cells per slot row */
  int nv;            /* doubles per block scratch row */
  int mm_any;        /* some aggregate is MIN/MAX */
  JitAcc acc;
  JitProbe probe;
  JitSlot slot;
  long long slut_span, slut_words;
  int occupancy;     /* second __launch_bounds__ argument */
  int nlate;         /* late columns: read in the row phase, passing rows only */
  int nstaged;       /* staged columns = rows of the LDS image */
  int lds_dict;      /* value dictionaries are looked up in an LDS copy */
  int direct;        /* image-free row loop (SN_K_F64_LATE_DIRECT) */
  int late[SN_DEV_MAX_COLS];   /* column is late */
  int srow[SN_DEV_MAX_COLS];   /* a staged column's row of the LDS image */
};

/* pac: per-agg-count accumulator rows ([sums][counts][rowcount]).  In
 * the JIT this occurs only for MIN/MAX plans (null-carrying batches are
 * never JIT-eligible, so counts == rowcount and the count cells simply
 * mirror the rowcount); mm plans route through the grouped layouts,
 * keyless included (one slot). */
static JitAcc jit_acc_mode(int nslots, int naggs, int pac, int sparse,
                           int radix, int mm_any) {
  /* sparse: open-address hash aggregate — accumulator IS `out` (hacc),
   * key table and flag words arrive via the jkeys/jpayload params, and the
   * capacity is tokenized (read from the device plan) so grow-and-retry
   * reuses one compiled kernel */
  /* radix two-pass: instead of probing the global table per row (64 B
   * random lines across tens of MB — the measured 182 B/row), pass 1
   * scatters (key, agg values) records into 1 << (hcap_log2-12) hash
   * partitions via an LDS-histogram multi-split; k_radix_agg then
   * aggregates each partition into its private L2-resident table segment */
  if (sparse) return radix ? ACC_RADIX : ACC_SPARSE;
  if (nslots <= 1 && !pac) return ACC_KEYLESS;
  if (nslots > JIT_LDS_MAX_SLOTS) return ACC_GLOBAL;
  /* >8 slots: block-level LDS accumulators (f64 LDS atomics) instead of
   * per-lane registers — the high-cardinality SHAMap analogue.  Occupancy 1
   * (the LDS image + accumulator array leave no room for a second group). */
  if (nslots > JIT_REG_MAX_SLOTS) return ACC_LDS;
  /* wbin mode: few aggregates over many slots makes the per-slot
   * select-accumulate VALU-bound (star join: 8 slots x 2 updates vs 2 LDS
   * atomics per row) — per-wave LDS bins shift the work to the LDS pipe,
   * which the row phase barely uses.
   * wbin eligibility: NA<=2 only.  Widening to Q1's 6-slot/5-agg shape was
   * MEASURED SLOWER (3.51 vs 5.13 TB/s on Q1 SF10): 6 LDS f64 atomics/row
   * across 16-lane bins conflict harder than the 36 slot-predicated fmas
   * cost, so the register accumulators stay the measured optimum for
   * multi-aggregate small-slot shapes. */
  if (naggs <= 2 && !mm_any && nslots * (naggs + 1) >= 12) return ACC_WBIN;
  return ACC_REGS;
}

/* Does the plan's shape fit a query-compiled kernel?  The engine asks before
 * sn_jit_get; the limits are those of the mode the classifier will pick
 * (MIN/MAX-ness moves a plan between REGS and WBIN only, which share one). */
extern "C" int sn_jit_shape_ok(const sn_dev_plan *p) {
  const int naggs = p->naggs, nslots = p->nslots;
  const int na1 = p->pac ? 2 * naggs + 1 : naggs + 1;
  switch (jit_acc_mode(nslots, naggs, p->pac != 0, p->sparse != 0, 0, 0)) {
    case ACC_KEYLESS: case ACC_SPARSE: case ACC_RADIX:
      return naggs <= JIT_MAX_AGGS;
    case ACC_REGS: case ACC_WBIN: return naggs <= JIT_REG_MAX_AGGS;
    case ACC_LDS:
      /* LDS-accumulator mode: static shared = LDS image + gacc must fit */
      return (size_t)p->nused * JIT_CHUNK * 8 + (size_t)nslots * na1 * 8 + 1024
             <= (size_t)JIT_LDS_BUDGET;
    case ACC_GLOBAL:
      /* global-atomic mode: only the LDS image constrains */
      return nslots <= SN_BIG_GROUP_CAP;
  }
  return 0;
}

static JitShape jit_classify(const sn_dev_plan *p, const int *kinds,
                             int nslots, int na_t, int has_del) {
  (void)has_del;
  JitShape s;
  s.NC = p->nused;
  s.NA = p->naggs;
  const int sparse = p->sparse != 0, pac = p->pac != 0;
  s.mm_any = 0;
  for (int a = 0; a < s.NA; a++) s.mm_any |= p->aggs[a].op != 0;
  s.NS = nslots < 1 ? 1 : nslots;
  s.NA1 = pac ? 2 * s.NA + 1 : s.NA + 1;
  s.acc = jit_acc_mode(nslots, s.NA, pac, sparse, p->radix != 0, s.mm_any);
  s.nv = s.acc == ACC_KEYLESS ? 2 * na_t + 1 : s.NS * s.NA1;

  /* LDS-packed dense LUT: the star probe's dependent gathers stall on
   * L2/HBM latency (measured 58% SQ_WAIT_INST issue-stall).  When the
   * payload fits 4 bits (group-by-attr gid <= 14, or semi-join presence)
   * and the packed span fits LDS, each workgroup packs the int32 LUT
   * into nibbles ONCE at kernel start and probes LDS instead.
   * SN_JIT_SLUT=0 reverts to the register-staged L2 probe. */
  static const int slut_env = [] {
    const char *v = getenv("SN_JIT_SLUT");
    return !v || v[0] != '0';
  }();
  s.slut_span = (p->jkeys && p->jlut)
      ? (long long)(p->jlut_max - p->jlut_min + 1) : 0;
  s.slut_words = (s.slut_span + 7) / 8;
  const int slut = slut_env && s.slut_span > 0 &&
                   (p->jmode == 0 || nslots <= 14) &&
                   s.slut_words * 4 <= JIT_SLUT_MAX_BYTES;
  s.probe = !p->jkeys ? PROBE_NONE
            : slut ? PROBE_SLUT : p->jlut ? PROBE_SPAY : PROBE_HASH;

  if (sparse) s.slot = s.acc == ACC_RADIX ? SLOT_RADIX_RANK : SLOT_SPARSE_PROBE;
  else if (s.acc == ACC_KEYLESS) s.slot = SLOT_NONE;
  else if (p->jkeys && p->jmode == 1) s.slot = SLOT_JOIN_ATTR;
  else s.slot = p->ngroup == 0 ? SLOT_SINGLE : SLOT_DENSE;

  /* sparse is random-probe latency-bound: more waves cover the
   * dependent loads (its LDS footprint is only the sval image).
   * SN_JIT_SPOCC overrides for occupancy sweeps. */
  static const int spocc_env = [] {
    const char *v = getenv("SN_JIT_SPOCC");
    return v ? atoi(v) : 0;
  }();
  if (sparse) s.occupancy = spocc_env > 0 ? spocc_env : 4;
  else if (s.acc == ACC_LDS || s.acc == ACC_GLOBAL) s.occupancy = 1;
  else s.occupancy = s.acc == ACC_WBIN ? 4 : 2;

  /* Late columns (SN_K_F64_LATE): honoured where the engine tags them, in
   * the keyless register modes without a probe; anywhere else, and when no
   * staged column would be left to carry the predicates, the column is
   * staged like the SN_K_F64 its descriptor says it is.  So is a column
   * that a predicate reads: predicates run on the image. */
  const bool late_mode = s.probe == PROBE_NONE &&
      (s.acc == ACC_KEYLESS || (s.acc == ACC_REGS && s.slot == SLOT_SINGLE));
  unsigned pred_cols = 0;
  for (int i = 0; i < p->npreds_d; i++) pred_cols |= 1u << p->preds_d[i].cslot;
  for (int i = 0; i < p->npreds_i; i++) pred_cols |= 1u << p->preds_i[i].cslot;
  for (int i = 0; i < p->npreds_in && i < 2; i++)
    pred_cols |= 1u << p->inp[i].cslot;
  s.nlate = 0;
  int direct_tag = 0;
  for (int c = 0; c < s.NC; c++) {
    direct_tag |= kinds[c] == SN_K_F64_LATE_DIRECT;
    s.nlate += s.late[c] = late_mode && !((pred_cols >> c) & 1) &&
        (kinds[c] == SN_K_F64_LATE || kinds[c] == SN_K_F64_LATE_DIRECT);
  }
  if (s.nlate == s.NC) {
    s.nlate = 0;
    for (int c = 0; c < s.NC; c++) s.late[c] = 0;
  }
  s.nstaged = 0;
  for (int c = 0; c < s.NC; c++) s.srow[c] = s.late[c] ? -1 : s.nstaged++;
  /* A kernel with a late column copies each value dictionary (256 doubles,
   * one per lane) into LDS once per tile and converts the staged codes from
   * there: two 8-byte gathers per row through the vector L1 are what bounds
   * the all-staged Q6 kernel (profiles/README.md, r04), not its HBM bytes.
   * SN_JIT_LATE_LDSDICT=0 keeps the global lookups, for A/B runs. */
  static const int lds_dict_env = [] {
    const char *v = getenv("SN_JIT_LATE_LDSDICT");
    return !v || v[0] != '0';
  }();
  s.lds_dict = s.nlate > 0 && lds_dict_env;
  /* The direct variant (SN_K_F64_LATE_DIRECT) goes by the tag
   * alone; the engine sets it only on plans the row loop can serve.  It keeps
   * no image, so its LDS is a few KB and the wave count bounds residency. */
  s.direct = direct_tag && s.nlate > 0 && s.acc == ACC_KEYLESS;
  if (s.direct) s.lds_dict = 0;   /* it keeps its own copy */
  return s;
}

/* ---- column kinds -------------------------------------------------------
 * All the generator knows about a stageable column kind.  A chunk of a
 * column is staged as two registers per lane, two rows each: st<c>_0 holds
 * rows 2*tid(+1), st<c>_1 rows 2*(tid+WG)(+1); 16-bit kinds pack their two
 * rows into one unsigned, the 1-byte kind both into one unsigned short.
 * The LDS image holds every value as a double,
 * except that 8-byte kinds keep their raw bits (an i64 converts where it is
 * read, by the plan's i64_mask). */
enum JitConv {
  CV_BITS64,   /* the 8 bytes as they are */
  CV_NUM,      /* numeric cast */
  CV_F32,      /* float bits in an int register */
  CV_DICT,     /* dm<c>[index]: premultiplied dictionary contribution */
  CV_VDICT     /* vd<c>[code]: the batch's value dictionary of doubles */
};
struct JitKind {
  const char *reg;   /* register type of one staged load */
  int bytes;         /* bytes per row in the column body */
  const char *mem;   /* row type in the column body */
  JitConv conv;      /* row -> double of the LDS image */
  int i64;           /* the 8 bytes are an integer whatever i64_mask says */
  int store_each;    /* stage_write stores y0 before it forms y1 (the text of
                        the measured kernels, kept as it is) */
};
static const JitKind &jit_kind(int k) {
  static const JitKind f64 = { "double2_t", 8, "double", CV_BITS64, 0, 0 };
  static const JitKind i64 = { "double2_t", 8, "double", CV_BITS64, 1, 0 };
  static const JitKind i32 = { "int2_t", 4, "int", CV_NUM, 0, 1 };
  static const JitKind f32 = { "int2_t", 4, "float", CV_F32, 0, 0 };
  static const JitKind d32 = { "int2_t", 4, "int", CV_DICT, 0, 0 };
  static const JitKind d16 = { "unsigned", 2, "unsigned short", CV_DICT, 0, 0 };
  static const JitKind i16 = { "unsigned", 2, "short", CV_NUM, 0, 0 };
  static const JitKind c8 = { "unsigned short", 1, "unsigned char", CV_VDICT,
                              0, 0 };
  switch (k) {
    case SN_K_F64: case SN_K_F64_LATE: case SN_K_F64_LATE_DIRECT: return f64;
    case SN_K_I64: return i64;
    case SN_K_I32: return i32;
    case SN_K_F32: return f32;
    case SN_K_DICT32: return d32;
    case SN_K_DICT16: return d16;
    case SN_K_F64C8: return c8;
    default: return i16;   /* SN_K_I16; the engine stages no other kind */
  }
}

/* staged register row j of column c (j: 0 -> st_0.x row base+2*tid,
 * 1 -> st_0.y, 2 -> st_1.x row base+2*(tid+WG), 3 -> .y) */
static std::string kind_reg_row(const JitKind &K, int c, int j) {
  if (K.bytes == 2)
    return strf((j & 1) ? "st%d_%d >> 16" : "st%d_%d & 0xffff", c, j >> 1);
  if (K.bytes == 1)
    return strf((j & 1) ? "st%d_%d >> 8" : "st%d_%d & 0xff", c, j >> 1);
  return strf("st%d_%d.%s", c, j >> 1, (j & 1) ? "y" : "x");
}

/* the LDS image's double for staged register row j (a CV_F32 row reads the
 * float2_t view f0/f1 that stage_write declares) */
static std::string kind_image_from_reg(const JitKind &K, int c, int j) {
  const std::string r = kind_reg_row(K, c, j);
  switch (K.conv) {
    case CV_BITS64: return r;
    case CV_DICT: return strf("(double)dm%d[%s]", c, r.c_str());
    case CV_VDICT: return strf("vd%d[%s]", c, r.c_str());
    case CV_F32: return strf("(double)f%d.%s", j >> 1, (j & 1) ? "y" : "x");
    default:
      return K.bytes == 2 ? strf("(double)(short)(%s)", r.c_str())
                          : strf("(double)%s", r.c_str());
  }
}

/* integer key from staged register row j.  Keys are int16/int32/int64
 * columns (the engine admits no other join key). */
static std::string kind_key_from_reg(const JitKind &K, int c, int j,
                                     int is_i64) {
  const std::string r = kind_reg_row(K, c, j);
  if (K.bytes == 8)
    return strf("%s(%s)", is_i64 || K.i64 ? "__double_as_longlong" : "(i64)",
                r.c_str());
  return K.bytes == 4 ? strf("(i64)%s", r.c_str())
                      : strf("(i64)(short)(%s)", r.c_str());
}

/* the LDS image's double for row base + r, read from global memory */
static std::string kind_image_from_mem(const JitKind &K, int c) {
  const std::string m =
      strf("((const GAS %s *)(body%d))[base + r]", K.mem, c);
  switch (K.conv) {
    case CV_BITS64: return m;
    case CV_DICT:
      return strf("(double)dm%d[%s%s]", c, K.bytes == 2 ? "(int)" : "",
                  m.c_str());
    case CV_VDICT: return strf("vd%d[%s]", c, m.c_str());
    default: return strf("(double)%s", m.c_str());
  }
}

/* ---- emitters -----------------------------------------------------------
 * Each appends one piece of the kernel to g.o; gen_source gives the order. */

struct Gen {
  std::string o;
  const sn_dev_plan *p;
  const int *kinds;
  int na_t, has_del;
  JitShape s;
};

/* trivial factors (a=0, m=1 — plain column reads, the common case) fold
 * back to the raw product; their triviality is part of the shape hash */
static bool ftriv(double a, double m) { return a == 0.0 && m == 1.0; }

static bool plan_col_is_i64(const sn_dev_plan *p, int cslot) {
  return (p->i64_mask >> cslot) & 1u;
}

/* typedefs, the device-struct layout mirror and the wave helpers; ends with
 * static_asserts that pin the mirror to the host's own layout, so a field
 * added to engine_internal.h fails the compile instead of shifting every
 * tokenized literal the kernel reads */
static void emit_prelude(std::string &o) {
  o += R"(
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef int int2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
#define GAS __attribute__((address_space(1)))
typedef unsigned long long u64;
typedef long long i64;
/* layout mirror of engine_internal.h (pointers + i32 fields only) */
struct sn_dev_col {
  const void *body; const u64 *nullw; const unsigned *nullpfx;
  const int *dictmap; const u64 *patch_bm; const int *patch_pos;
  const double *patch_val; const u64 *patch_nullbm;
  const int *rle_ends; const double *rle_vals; int rle_n;
  int patch_n; int kind; int has_nulls; int null_gid;
};
struct sn_dev_batch { int num_rows; int clean; const u64 *del_bm; sn_dev_col cols[)";
  emitf(o, "%d", SN_DEV_MAX_COLS);
  o += R"(]; };
struct sn_dev_tile { int batch; int row_start; };
struct sn_dev_pred_d { double lo, hi; int cslot, _p; };
struct sn_dev_pred_i { i64 lo, hi; int cslot, _p; };
struct sn_dev_agg { double a0, m0, a1, m1, a2, m2; int c0, c1, c2, nf, op, _p2; };
struct sn_dev_plan {
  int npreds_d, npreds_i, naggs, ngroup, nslots, nused;
  unsigned i64_mask; int gcol[2];
  const i64 *jkeys; const int *jpayload;
  int jcap_log2, jcslot, jmode, jslot_mul;
  const int *jlut; i64 jlut_min, jlut_max;
  i64 gbase[2]; int gmul0, _pad2;
  sn_dev_pred_d preds_d[8];
  sn_dev_pred_i preds_i[4];
  sn_dev_agg aggs[12];
  struct { const u64 *bm; const i64 *list; i64 base;
           int nwords, n, cslot, _p; } inp[2];
  int npreds_in, _pad4b;
  i64 *hkeys; double *hacc; int *hflags;
  int hcap_log2, sparse, pac, _pad3;
  double *precs; int *pcount; int percap, radix;
};
__device__ __forceinline__ double wsum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ u64 f64ord(double x) {
  u64 b = (u64)__double_as_longlong(x);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double wmin(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_down(x, off, 64));
  return x;
}
__device__ __forceinline__ double wmax(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
  return x;
}
__device__ __forceinline__ u64 mix64(u64 x) {
  x += 0x9E3779B97f4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
)";
  emitf(o, "#define CHUNK %d\n#define WG %d\n#define TILE %d\n",
        JIT_CHUNK, JIT_WG, SN_TILE_ROWS);
  /* every mirrored size, and the offset of every member the kernel reads */
#define SZ(T) { "sizeof(" #T ")", sizeof(T) }
#define OFF(T, M) { "__builtin_offsetof(" #T ", " #M ")", offsetof(T, M) }
  static const struct { const char *what; size_t is; } pins[] = {
    SZ(sn_dev_col), SZ(sn_dev_batch), SZ(sn_dev_tile), SZ(sn_dev_pred_d),
    SZ(sn_dev_pred_i), SZ(sn_dev_agg), SZ(sn_dev_plan),
    OFF(sn_dev_col, body), OFF(sn_dev_col, dictmap),
    OFF(sn_dev_batch, num_rows), OFF(sn_dev_batch, del_bm),
    OFF(sn_dev_batch, cols), OFF(sn_dev_tile, row_start),
    OFF(sn_dev_pred_d, hi), OFF(sn_dev_pred_i, hi), OFF(sn_dev_agg, m2),
    OFF(sn_dev_plan, preds_d), OFF(sn_dev_plan, preds_i),
    OFF(sn_dev_plan, aggs), OFF(sn_dev_plan, inp[1].bm),
    OFF(sn_dev_plan, inp[1].base), OFF(sn_dev_plan, inp[1].nwords),
    OFF(sn_dev_plan, hcap_log2), OFF(sn_dev_plan, precs),
    OFF(sn_dev_plan, pcount), OFF(sn_dev_plan, percap),
    OFF(sn_dev_plan, radix),
  };
#undef SZ
#undef OFF
  for (const auto &pin : pins)
    emitf(o, "static_assert(%s == %zu, \"layout mirror differs from "
             "engine_internal.h\");\n", pin.what, pin.is);
}

/* MIN/MAX order values by the aggregates' total order (non-finite
 * aggregate inputs): f64ord's, with every NaN, whatever its sign and payload,
 * one value above +inf.  Its image, that of the positive quiet NaN, is also
 * MIN's identity.  Emitted into kernels with a MIN/MAX aggregate only, the
 * wave folds into the register mode only, so every other kernel keeps its
 * text. */
static void emit_order_helpers(Gen &g) {
  if (!g.s.mm_any) return;
  g.o += R"(__device__ __forceinline__ u64 f64ordc(double x) {
  return x != x ? 0xFFF8000000000000ull : f64ord(x);
}
)";
  if (g.s.acc != ACC_REGS) return;
  g.o += R"(__device__ __forceinline__ u64 wminu(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = (u64)__shfl_down((i64)x, off, 64);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ u64 wmaxu(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = (u64)__shfl_down((i64)x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}
)";
}

static void emit_signature(Gen &g) {
  emitf(g.o, "extern \"C\" __global__ __launch_bounds__(WG, %d)\n"
           "void jit_scan(const sn_dev_batch *__restrict__ batches,\n"
           "              const sn_dev_tile *__restrict__ tiles, int ntiles,\n"
           "              double *__restrict__ out,\n"
           "              const i64 *__restrict__ jkeys_p,\n"
           "              const int *__restrict__ jpayload_p,\n"
           "              const int *__restrict__ jlut_p,\n"
           "              const sn_dev_plan *__restrict__ plan_p) {\n"
           "  const GAS i64 *jkeys = (const GAS i64 *)(u64)jkeys_p;\n"
           "  const GAS int *jpayload = (const GAS int *)(u64)jpayload_p;\n"
           "  const GAS int *jlut = (const GAS int *)(u64)jlut_p;\n"
           "  const GAS sn_dev_plan *P = (const GAS sn_dev_plan *)(u64)plan_p;\n"
           "  (void)jkeys; (void)jpayload; (void)jlut; (void)P;\n",
        g.s.occupancy);
}

/* tokenized plan values (the reference's ParamLiteral tokenization,
 * TokenizationTest / SnappySession plan cache): predicate bounds and
 * aggregate coefficients load once per wave from the cached device plan
 * (uniform scalar loads hoisted to kernel entry), so one compiled
 * kernel serves every literal value of the same plan SHAPE.  Structure
 * (counts, columns, neutral factors, group/join/LUT geometry) stays
 * compile-time. */
static void emit_literals(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  for (int i = 0; i < p->npreds_d; i++)
    emitf(o, "  const double pd%d_lo = P->preds_d[%d].lo, pd%d_hi = P->preds_d[%d].hi;\n",
          i, i, i, i);
  for (int i = 0; i < p->npreds_i; i++)
    emitf(o, "  const i64 pi%d_lo = P->preds_i[%d].lo, pi%d_hi = P->preds_i[%d].hi;\n",
          i, i, i, i);
  for (int i = 0; i < p->npreds_in && i < 2; i++)
    emitf(o, "  const GAS u64 *inbm%d = (const GAS u64 *)(u64)P->inp[%d].bm;\n"
             "  const i64 inb%d_base = P->inp[%d].base;\n"
             "  const i64 inb%d_lim = (i64)P->inp[%d].nwords * 64;\n",
          i, i, i, i, i, i);
  for (int a = 0; a < g.s.NA; a++) {
    const sn_dev_agg &A = p->aggs[a];
    if (A.nf >= 1 && !ftriv(A.a0, A.m0))
      emitf(o, "  const double ag%d_a0 = P->aggs[%d].a0, ag%d_m0 = P->aggs[%d].m0;\n", a, a, a, a);
    if (A.nf >= 2 && !ftriv(A.a1, A.m1))
      emitf(o, "  const double ag%d_a1 = P->aggs[%d].a1, ag%d_m1 = P->aggs[%d].m1;\n", a, a, a, a);
    if (A.nf >= 3 && !ftriv(A.a2, A.m2))
      emitf(o, "  const double ag%d_a2 = P->aggs[%d].a2, ag%d_m2 = P->aggs[%d].m2;\n", a, a, a, a);
  }
}

/* zero an LDS accumulator of n cells; with MIN/MAX aggregates (mm) their
 * cells take the ord-encoding identities instead */
static void emit_acc_init(std::string &o, const Gen &g, const char *acc,
                          int n, int mm) {
  if (!mm) {
    emitf(o, "  for (int i = tid; i < %d; i += WG) %s[i] = 0.0;\n", n, acc);
  } else {
    emitf(o, "  for (int i = tid; i < %d; i += WG) {\n"
             "    const int a = i %% %d;\n"
             "    double iv = 0.0;\n", n, g.s.NA1);
    for (int a = 0; a < g.s.NA; a++)
      if (g.p->aggs[a].op != 0)
        emitf(o, "    if (a == %d) iv = __longlong_as_double(%s);\n", a,
              g.p->aggs[a].op == 1 ? "0xFFF8000000000000ll"
                                   : "0x0000000000000000ll");
    emitf(o, "    %s[i] = iv;\n  }\n", acc);
  }
  o += "  __syncthreads();\n";
}

/* the LDS image, then whatever holds the aggregates during the scan */
static void emit_acc_decl(Gen &g) {
  std::string &o = g.o;
  const JitShape &s = g.s;
  emitf(o, "  __shared__ __attribute__((aligned(16))) double sval[%d][CHUNK];\n", s.nstaged);
  static_assert(JIT_WG == SN_NARROW_MAX, "one dictionary entry per lane");
  for (int c = 0; c < s.NC && s.lds_dict; c++)
    if (jit_kind(g.kinds[c]).conv == CV_VDICT)
      emitf(o, "  __shared__ __attribute__((aligned(16))) double svd%d[WG];\n", c);
  /* shared arrays precede tid in the text; the rest of each mode follows */
  std::string d;
  const char *bacc = "  __shared__ __attribute__((aligned(16))) double bacc[%d];\n";
  const char *sparse_tables =
      /* single HBM accumulator (sparse keys -> low per-address contention;
       * probe position indexes the rows); capacity tokenized from the plan */
      "  GAS double *gacc = (GAS double *)(u64)out;\n"
      "  GAS i64 *hkeys = (GAS i64 *)(u64)jkeys_p;\n"
      "  GAS int *hflags = (GAS int *)(u64)jpayload_p;\n"
      "  const int hcl = P->hcap_log2;\n"
      "  const unsigned hmask = (1u << hcl) - 1;\n"
      "  const int hcap = 1 << hcl;\n"
      "  (void)gacc; (void)hkeys; (void)hmask; (void)hcap;\n";
  switch (s.acc) {
    case ACC_RADIX:
      o += "  __shared__ int phist[4096];\n";   /* npart <= 4096 (cap 2^24) */
      d += sparse_tables;
      d += "  GAS double *precs = (GAS double *)(u64)P->precs;\n"
           "  GAS int *pcount = (GAS int *)(u64)P->pcount;\n"
           "  const int percap = P->percap;\n"
           "  const int npart = 1 << (hcl - P->radix);\n";
      break;
    case ACC_SPARSE:
      d += sparse_tables;
      break;
    case ACC_GLOBAL:
      /* HBM accumulator IS the out/scratch pointer (host-zeroed), privatized
       * 8 ways by XCD (blockIdx & 7 matches the dispatch round-robin) so
       * same-slot atomics from different XCDs never contend and stay in the
       * local L2; k_reduce folds the 8 copies */
      emitf(d, "  GAS double *gacc = (GAS double *)(u64)out"
               " + (u64)(blockIdx.x & 7) * %d;\n", s.nv);
      break;
    case ACC_LDS:
      /* block-level LDS accumulator, initialized once (min/max cells take
       * their ord-encoding identities), flushed once at the end */
      emitf(d, "  __shared__ __attribute__((aligned(16))) double gacc[%d];\n",
            s.nv);
      emit_acc_init(d, g, "gacc", s.nv, s.mm_any);
      break;
    case ACC_WBIN:
      /* 16 bins of 16 lanes each: ~2-way LDS atomic conflicts instead of the
       * 8-way a per-wave bin sees (measured: issue-stall bound, 58% of wave
       * cycles in SQ_WAIT_INST_ANY with per-wave bins) */
      emitf(d, "  __shared__ __attribute__((aligned(16))) double wbin[16][%d];\n"
               "  for (int i = tid; i < 16 * %d; i += WG)\n"
               "    ((double *)wbin)[i] = 0.0;\n"
               "  __syncthreads();\n",
            s.nv, s.nv);
      break;
    case ACC_REGS:
      emitf(o, bacc, s.nv);
      emitf(d, "  double sums[%d][%d]; double rc[%d];\n", s.NS, s.NA, s.NS);
      if (s.mm_any) emitf(d, "  u64 ords[%d][%d];\n", s.NS, s.NA);
      /* the block accumulator starts here, not at the flush: non-finite
       * values reach it during the scan */
      emit_acc_init(d, g, "bacc", s.nv, s.mm_any);
      emitf(d, "#pragma unroll\n  for (int s = 0; s < %d; s++) {\n"
               "    rc[s] = 0;\n", s.NS);
      /* a MIN/MAX aggregate keeps the order image of its value in ords,
       * a sum its double in sums; the unused half of each pair folds away */
      for (int a = 0; a < s.NA; a++) {
        const int op = g.p->aggs[a].op;
        if (op == 0) emitf(d, "    sums[s][%d] = 0.0;\n", a);
        else emitf(d, "    ords[s][%d] = %s;\n", a,
                   op == 1 ? "0xFFF8000000000000ull" : "0ull");
      }
      d += "  }\n";
      break;
    case ACC_KEYLESS:
      emitf(o, bacc, s.nv);
      emitf(d, "  double sums[%d], cnts[%d], rcnt = 0.0;\n", s.NA, s.NA);
      emitf(d, "#pragma unroll\n  for (int a = 0; a < %d; a++) { sums[a] = 0; cnts[a] = 0; }\n", s.NA);
      break;
  }
  o += "  const int tid = threadIdx.x;\n";
  o += d;
}

static void emit_probe_decl(Gen &g) {
  if (g.s.probe == PROBE_SPAY)
    g.o += "  __shared__ int spay[CHUNK];\n";
  if (g.s.probe == PROBE_SLUT)
    emitf(g.o, "  __shared__ unsigned slut[%lld];\n", g.s.slut_words);
}

/* staged register buffers: per column, by width class */
static void emit_stage_regs(Gen &g) {
  for (int c = 0; c < g.s.NC; c++)
    if (!g.s.late[c])
      emitf(g.o, "  %s st%d_0, st%d_1;\n", jit_kind(g.kinds[c]).reg, c, c);
}

/* pack the dense LUT into 4-bit LDS nibbles, once per workgroup:
 * 15 = absent; group-by-attr payloads are gids <= 14 (structural
 * gate), semi-join presence packs as 0 */
static void emit_slut_pack(Gen &g) {
  emitf(g.o, "  for (unsigned i = tid; i < %lldu; i += WG) {\n"
           "    unsigned wd = 0u;\n"
           "#pragma unroll\n"
           "    for (int j = 0; j < 8; j++) {\n"
           "      const long long ix = (long long)i * 8 + j;\n"
           "      const int v = ix < %lldll ? jlut[ix] : -1;\n"
           "      const unsigned nib = v < 0 ? 15u : %s;\n"
           "      wd |= nib << (4 * j);\n"
           "    }\n"
           "    slut[i] = wd;\n"
           "  }\n"
           "  __syncthreads();\n",
        g.s.slut_words, g.s.slut_span, g.p->jmode == 0 ? "0u" : "(unsigned)v");
}

/* tile loop head; hoist body/dict pointers */
static void emit_tile_prologue(Gen &g) {
  std::string &o = g.o;
  o += R"(
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int num_rows = b.num_rows;
    const int tile_end = min(tile.row_start + TILE, num_rows);
)";
  if (g.has_del)
    o += "    const GAS u64 *del = (const GAS u64 *)(u64)b.del_bm;\n";
  for (int c = 0; c < g.s.NC; c++) {
    emitf(o, "    const GAS char *body%d = (const GAS char *)(unsigned long long)b.cols[%d].body;\n", c, c);
    if (jit_kind(g.kinds[c]).conv == CV_DICT)
      emitf(o, "    const GAS int *dm%d = (const GAS int *)(unsigned long long)b.cols[%d].dictmap;\n", c, c);
    if (jit_kind(g.kinds[c]).conv == CV_VDICT)
      emitf(o, "    const GAS double *vd%d = (const GAS double *)(unsigned long long)b.cols[%d].rle_vals;\n", c, c);
  }
  if (!g.s.lds_dict) return;
  /* the batch's dictionaries into LDS (a sidecar always holds 256 entries).
   * The last reads of the previous tile's copy are behind the barrier that
   * ends its chunk loop; this one orders the copy before stage_write. */
  bool any = false;
  for (int c = 0; c < g.s.NC; c++)
    if (jit_kind(g.kinds[c]).conv == CV_VDICT) {
      emitf(o, "    svd%d[tid] = vd%d[tid];\n", c, c);
      any = true;
    }
  if (any) o += "    __syncthreads();\n";
}

/* stage_load body, emitted in the prologue and inside the chunk loop */
static void emit_stage_load(Gen &g, const char *base_expr, const char *ind) {
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c]) continue;
    const JitKind &K = jit_kind(g.kinds[c]);
    emitf(g.o, "%sst%d_0 = ((const GAS %s *)(body%d + (u64)(%s) * %d))[tid];\n",
          ind, c, K.reg, c, base_expr, K.bytes);
    emitf(g.o, "%sst%d_1 = ((const GAS %s *)(body%d + (u64)(%s) * %d))[tid + WG];\n",
          ind, c, K.reg, c, base_expr, K.bytes);
  }
}

/* stage_write: the staged registers, converted, into the LDS image */
static void emit_stage_write(Gen &g, const char *ind) {
  std::string &o = g.o;
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c]) continue;
    const JitKind &K = jit_kind(g.kinds[c]);
    const int sr = g.s.srow[c];
    if (K.conv == CV_BITS64) {
      emitf(o, "%s((double2_t *)sval[%d])[tid] = st%d_0;\n", ind, sr, c);
      emitf(o, "%s((double2_t *)sval[%d])[tid + WG] = st%d_1;\n", ind, sr, c);
      continue;
    }
    std::string y[2], st[2];
    for (int h = 0; h < 2; h++) {
      y[h] = strf("double2_t y%d; y%d.x = %s; y%d.y = %s;", h, h,
                  kind_image_from_reg(K, c, 2 * h).c_str(), h,
                  kind_image_from_reg(K, c, 2 * h + 1).c_str());
      st[h] = strf("((double2_t *)sval[%d])[tid%s] = y%d;", sr,
                   h ? " + WG" : "", h);
      if (g.s.lds_dict && K.conv == CV_VDICT) {   /* vd<c>[..] -> svd<c>[..] */
        const std::string gl = strf(" vd%d[", c);
        for (size_t at; (at = y[h].find(gl)) != std::string::npos;)
          y[h].replace(at, gl.size(), strf(" svd%d[", c));
      }
    }
    emitf(o, "%s{ ", ind);
    if (K.conv == CV_F32)
      emitf(o, "float2_t f0 = *(float2_t *)&st%d_0, f1 = *(float2_t *)&st%d_1;\n%s  ",
            c, c, ind);
    if (K.store_each)
      emitf(o, "%s\n%s  %s\n%s  %s\n%s  %s }\n", y[0].c_str(), ind,
            st[0].c_str(), ind, y[1].c_str(), ind, st[1].c_str());
    else
      emitf(o, "%s\n%s  %s\n%s  %s\n%s  %s }\n", y[0].c_str(), ind,
            y[1].c_str(), ind, st[0].c_str(), ind, st[1].c_str());
  }
}

/* tail / unstaged chunk: convert straight from global memory */
static void emit_scalar_tail(Gen &g) {
  std::string &o = g.o;
  o += "        /* scalar tail conversion (the [rows, CHUNK) image tail is\n"
       "         * zeroed below: raw LDS can hold NaN-pattern bits from the\n"
       "         * previous kernel, and fma(0, NaN, sum) = NaN would poison\n"
       "         * the slot-predicated register accumulators) */\n";
  for (int c = 0; c < g.s.NC; c++)
    if (!g.s.late[c])
      emitf(o, "        for (int r = tid; r < rows; r += WG) sval[%d][r] = %s;\n",
            g.s.srow[c], kind_image_from_mem(jit_kind(g.kinds[c]), c).c_str());
  for (int c = 0; c < g.s.NC; c++)
    if (!g.s.late[c])
      emitf(o, "        for (int r = rows + tid; r < CHUNK; r += WG)"
               " sval[%d][r] = 0.0;\n", g.s.srow[c]);
}

/* one dense-LUT lookup: dst = payload of kexpr, or -1 outside the span */
static void emit_lut_probe(Gen &g, const std::string &kexpr,
                           const std::string &dst, const char *ind) {
  const sn_dev_plan *p = g.p;
  emitf(g.o, "%s{ const i64 key = %s;\n"
           "%s  const int inr = (key >= %lldll) & (key <= %lldll);\n"
           "%s  const i64 ck = key < %lldll ? %lldll : (key > %lldll ? %lldll : key);\n"
           "%s  const int pv = jlut[ck - %lldll];\n"
           "%s  %s = inr ? pv : -1; }\n",
        ind, kexpr.c_str(),
        ind, (long long)p->jlut_min, (long long)p->jlut_max,
        ind, (long long)p->jlut_min, (long long)p->jlut_min,
        (long long)p->jlut_max, (long long)p->jlut_max,
        ind, (long long)p->jlut_min,
        ind, dst.c_str());
}

/* LUT probe straight from the staged key registers, BEFORE they are
 * written to LDS: the dependent LUT gathers then overlap the stage_write
 * + barrier + next stage_load instead of stalling the row pass
 * (measured: in-pass probing leaves 35% of wave cycles parked).
 * Register mapping: st_0 covers rows 2*tid(+1), st_1 rows 2*(tid+WG)(+1);
 * the row pass reads spay[tid + k*WG] after the barrier. */
static void emit_spay_from_regs(Gen &g) {
  const int jc = g.p->jcslot;
  static const char *const dst[4] = { "spay[2 * tid]", "spay[2 * tid + 1]",
                                      "spay[2 * (tid + WG)]",
                                      "spay[2 * (tid + WG) + 1]" };
  for (int j = 0; j < 4; j++)
    emit_lut_probe(g, kind_key_from_reg(jit_kind(g.kinds[jc]), jc, j,
                                        plan_col_is_i64(g.p, jc)),
                   dst[j], "        ");
}

/* tail / unstaged chunks: fill spay from the LDS image (lane-local
 * mapping, so no extra barrier before the row pass reads it) */
static void emit_spay_from_image(Gen &g) {
  emitf(g.o, "      if (!staged) {\n"
           "#pragma unroll\n"
           "        for (int k = 0; k < CHUNK / WG; k++) {\n"
           "          const int r = tid + k * WG;\n"
           "          const double jx = sval[%d][r];\n",
        g.p->jcslot);
  emit_lut_probe(g, plan_col_is_i64(g.p, g.p->jcslot)
                        ? "__double_as_longlong(jx)" : "(i64)jx",
                 "spay[r]", "          ");
  g.o += "        }\n"
         "      }\n";
}

/* radix pass A state.  per-k register stash: pass A computes (partition,
 * rank, key, values) per row; pass B scatters after the per-chunk base
 * reservation.  Fully unrolled so the arrays stay in registers. */
static void emit_radix_stash(Gen &g) {
  emitf(g.o, "      i64 rkey[CHUNK / WG];\n"
           "      int rok[CHUNK / WG], rpk[CHUNK / WG], rrnk[CHUNK / WG];\n");
  for (int a = 0; a < g.s.NA; a++)
    emitf(g.o, "      double rva%d[CHUNK / WG];\n", a);
}

/* the row's delete bit (row base + r of the batch) */
static void emit_delete_pred(Gen &g) {
  if (g.has_del)
    g.o += "        if (del) {\n"
           "          const int gr = base + r;\n"
           "          ok &= (int)(~(del[(u64)gr >> 6] >> (gr & 63)) & 1ull);\n"
           "        }\n";
}

/* row predicates: delete mask, range predicates, bitmap IN-lists */
static void emit_row_predicates(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  emit_delete_pred(g);
  for (int i = 0; i < p->npreds_d; i++) {
    emitf(o, "        { const double x = sval[%d][r];\n"
             "          ok &= (x >= pd%d_lo) & (x <= pd%d_hi); }\n",
          g.s.srow[p->preds_d[i].cslot], i, i);
  }
  for (int i = 0; i < p->npreds_i; i++) {
    emitf(o, "        { const i64 x = __double_as_longlong(sval[%d][r]);\n"
             "          ok &= (x >= pi%d_lo) & (x <= pi%d_hi); }\n",
          g.s.srow[p->preds_i[i].cslot], i, i);
  }
  for (int i = 0; i < p->npreds_in && i < 2; i++) {
    const int cs = p->inp[i].cslot;
    const int is64 = plan_col_is_i64(p, cs);
    emitf(o, "        { const i64 v = %ssval[%d][r]%s;\n"
             "          const i64 ix = v - inb%d_base;\n"
             "          ok &= (ix >= 0) & (ix < inb%d_lim) &\n"
             "                (int)((inbm%d[ix >> 6] >> (ix & 63)) & 1ull); }\n",
          is64 ? "__double_as_longlong(" : "(i64)", g.s.srow[cs],
          is64 ? ")" : "", i, i, i);
  }
}

/* Late columns: the row phase runs as two fully unrolled passes, so the
 * arrays below stay in registers.  Pass A forms every slot's `ok` from the
 * image of the staged columns and issues the late loads of the chunk, each
 * under its row's `ok`: `ok` holds r < rows and the delete bit, so no lane
 * reads past num_rows; a 128-byte line of the column in which no row passes
 * is not requested; and a row that does not pass is never read, whatever it
 * holds.  Pass B consumes them in ascending k, the order of the one-pass
 * row phase. */
static void emit_late_stash(Gen &g) {
  g.o += "      int okv[CHUNK / WG];\n";
  for (int c = 0; c < g.s.NC; c++)
    if (g.s.late[c]) emitf(g.o, "      double e%d[CHUNK / WG];\n", c);
}

/* end of pass A, head of pass B */
static void emit_late_split(Gen &g) {
  std::string &o = g.o;
  o += "        okv[k] = ok;\n";
  for (int c = 0; c < g.s.NC; c++)
    if (g.s.late[c])
      emitf(o, "        e%d[k] = 0.0;\n"
               "        if (ok) e%d[k] = ((const GAS double *)(body%d))[base + r];\n",
            c, c, c);
  o += "      }\n"
       "#pragma unroll\n"
       "      for (int k = 0; k < CHUNK / WG; k++) {\n"
       "        const int r = tid + k * WG;\n"
       "        const int ok = okv[k];\n"
       "        (void)r;\n";
}

/* broadcast-dimension probe with literal table shape (mask, key slot,
 * i64-ness); empty-slot sentinel = INT64_MIN, same as the interpreted
 * probe_sweep */
static void emit_join_probe(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  const char *key = plan_col_is_i64(p, p->jcslot) ? "__double_as_longlong(jx)"
                                                  : "(i64)jx";
  switch (g.s.probe) {
    case PROBE_NONE: break;
    case PROBE_SLUT:
      /* 4-bit LDS probe: range check + one LDS read per row */
      emitf(o, "        int pay = -1;\n"
               "        {\n"
               "          const double jx = sval[%d][r];\n"
               "          const i64 key = %s;\n"
               "          const i64 ix = key - %lldll;\n"
               "          if (ix >= 0 && ix < %lldll) {\n"
               "            const unsigned nib =\n"
               "                (slut[ix >> 3] >> (((unsigned)ix & 7u) * 4u)) & 15u;\n"
               "            pay = nib == 15u ? -1 : (int)nib;\n"
               "          }\n"
               "        }\n"
               "        ok &= pay >= 0;\n",
            p->jcslot, key, (long long)p->jlut_min, g.s.slut_span);
      break;
    case PROBE_SPAY:
      /* probed from the staged registers into spay */
      o += "        const int pay = spay[r];\n"
           "        ok &= pay >= 0;\n";
      break;
    case PROBE_HASH:
      emitf(o, "        int pay = -1;\n"
               "        if (ok) {\n"
               "          const double jx = sval[%d][r];\n"
               "          const i64 key = %s;\n"
               "          unsigned h = (unsigned)mix64((u64)key) & %uu;\n"
               "          while (true) {\n"
               "            const i64 k0 = jkeys[h];\n"
               "            if (k0 == key) { pay = jpayload[h]; break; }\n"
               "            if (k0 == (i64)0x8000000000000000ll) break;\n"
               "            h = (h + 1) & %uu;\n"
               "          }\n"
               "          ok = pay >= 0;\n"
               "        }\n",
            p->jcslot, key,
            (1u << p->jcap_log2) - 1, (1u << p->jcap_log2) - 1);
      break;
  }
}

/* sparse group key: key geometry is compile-time */
static void emit_sparse_key(Gen &g) {
  const sn_dev_plan *p = g.p;
  if (p->ngroup == 1) {
    if (plan_col_is_i64(p, p->gcol[0]))
      emitf(g.o, "        const i64 skey = __double_as_longlong(sval[%d][r]);\n",
            p->gcol[0]);
    else
      emitf(g.o, "        const i64 skey = (i64)sval[%d][r];\n", p->gcol[0]);
  } else {
    emitf(g.o, "        const i64 skey = (i64)(((u64)(unsigned)(int)sval[%d][r]"
             " << 32) | (unsigned)(int)sval[%d][r]);\n",
          p->gcol[0], p->gcol[1]);
  }
}

/* the row's accumulator slot */
static void emit_slot(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  switch (g.s.slot) {
    case SLOT_NONE: break;
    case SLOT_RADIX_RANK:
      emit_sparse_key(g);
      /* pass A: partition by mix64 HIGH bits (pass 2 probes the segment
       * with the LOW bits — independent), rank via the LDS histogram */
      o += "        rkey[k] = skey;\n"
           "        int rpk_ = 0, rrnk_ = 0;\n"
           "        if (ok) {\n"
           "          rpk_ = (int)((mix64((u64)skey) >> 44) & (u64)(npart - 1));\n"
           "          rrnk_ = atomicAdd(&phist[rpk_], 1);\n"
           "        }\n"
           "        rpk[k] = rpk_; rrnk[k] = rrnk_;\n";
      break;
    case SLOT_SPARSE_PROBE:
      /* open-address probe (ByteBufferHashMap.putBufferIfAbsent shape):
       * capacity tokenized */
      emit_sparse_key(g);
      o += R"(        int slot = -1;
        if (ok) {
          if (skey == -1ll) slot = hcap;     /* sentinel-valued key */
          else {
            unsigned h = (unsigned)mix64((u64)skey) & hmask;
            for (unsigned it = 0; it <= hmask; ++it) {
              const i64 k0 = hkeys[h];
              if (k0 == skey) { slot = (int)h; break; }
              if (k0 == -1ll) {
                const i64 old = (i64)atomicCAS((unsigned long long *)&hkeys[h],
                                               (unsigned long long)-1ll,
                                               (unsigned long long)skey);
                if (old == -1ll) { atomicAdd((int *)(hflags + 2), 1); slot = (int)h; break; }
                if (old == skey) { slot = (int)h; break; }
              }
              h = (h + 1) & hmask;
            }
            if (slot < 0) atomicOr((int *)hflags, 1);
          }
        }
        ok &= slot >= 0;
)";
      break;
    case SLOT_JOIN_ATTR:
      if (p->jslot_mul > 0 && p->ngroup >= 1)
        /* composite GROUP BY dim_attr, fact_col (all literals) */
        emitf(o, "        const int slot = (pay > 0 ? pay : 0) * %d +"
                 " (int)((i64)sval[%d][r] - %lldll);\n",
              p->jslot_mul, p->gcol[0], (long long)p->gbase[0]);
      else
        o += "        const int slot = pay > 0 ? pay : 0;\n";
      break;
    case SLOT_SINGLE:
      /* keyless plan in the grouped (pac) layout: one slot */
      o += "        const int slot = 0;\n";
      break;
    case SLOT_DENSE:
      /* slot = (v0 - base0)*mul0 + (v1 - base1), all literals; dictionary
       * keys arrive premultiplied (base 0, mul 1) so this folds to the
       * plain cast for them */
      emitf(o, "        int slot = (int)(((i64)sval[%d][r] - %lldll) * %d);\n",
            p->gcol[0], (long long)p->gbase[0], p->gmul0 ? p->gmul0 : 1);
      if (p->ngroup >= 2)
        emitf(o, "        slot += (int)((i64)sval[%d][r] - %lldll);\n",
              p->gcol[1], (long long)p->gbase[1]);
      break;
  }
}

/* ---- the direct (image-free) keyless kernel: DESIGN.md §2d --------------
 * No LDS image and no barrier in the row loop.  Per tile each workgroup
 * copies the value dictionaries that aggregate factors read (svd<c>) and
 * evaluates every narrowed predicate column's range predicates once, on its
 * dictionary, into a 256-bit pass set (spass<c>).  Both are double-buffered
 * by tile parity (pb), so the one barrier per tile orders the writes before
 * the reads, and the reads of tile n before the writes of tile n + 2.  A
 * lane then handles DS rows per step, row = base + tid + k * WG: the staged
 * loads of all DS rows are issued together (and the next step's before this
 * step's late values are used), integer columns compare in registers, a
 * narrowed predicate column tests its code's bit, and the late loads of the
 * DS rows fly together. */

static bool direct_has_pred(const Gen &g, int c) {
  for (int i = 0; i < g.p->npreds_d; i++)
    if (g.p->preds_d[i].cslot == c) return true;
  return false;
}

static bool direct_is_factor(const Gen &g, int c) {
  for (int a = 0; a < g.s.NA; a++) {
    const sn_dev_agg &A = g.p->aggs[a];
    if ((A.nf >= 1 && A.c0 == c) || (A.nf >= 2 && A.c1 == c) ||
        (A.nf >= 3 && A.c2 == c))
      return true;
  }
  return false;
}

/* an aggregate factor of a column that is not late: f<c>[k] is the row's
 * code or integer, kept from the staged registers */
static std::string direct_factor(const Gen &g, int cs) {
  return jit_kind(g.kinds[cs]).conv == CV_VDICT
             ? strf("svd%d[pb][f%d[k]]", cs, cs)
             : strf("(double)f%d[k]", cs);
}

static const char *direct_reg_type(const JitKind &K) {
  return K.conv == CV_VDICT ? "unsigned" : "int";
}

static void emit_direct_decl(Gen &g) {
  std::string &o = g.o;
  const JitShape &s = g.s;
  static_assert(JIT_WG == SN_NARROW_MAX, "one dictionary entry per lane");
  for (int c = 0; c < s.NC; c++) {
    if (jit_kind(g.kinds[c]).conv != CV_VDICT) continue;
    if (direct_is_factor(g, c))
      emitf(o, "  __shared__ __attribute__((aligned(16))) double svd%d[2][WG];\n", c);
    if (direct_has_pred(g, c))
      emitf(o, "  __shared__ __attribute__((aligned(16))) u64 spass%d[2][4];\n", c);
  }
  emitf(o, "  __shared__ __attribute__((aligned(16))) double bacc[%d];\n", s.nv);
  o += "  const int tid = threadIdx.x;\n";
  emitf(o, "  double sums[%d], cnts[%d], rcnt = 0.0;\n", s.NA, s.NA);
  emitf(o, "#pragma unroll\n  for (int a = 0; a < %d; a++) { sums[a] = 0; cnts[a] = 0; }\n", s.NA);
  o += "  int pb = 0;\n";
  for (int c = 0; c < s.NC; c++)
    if (!s.late[c])
      emitf(o, "  %s x%d[DS];\n", direct_reg_type(jit_kind(g.kinds[c])), c);
}

/* per tile: dictionaries and pass sets into the pb half, one barrier */
static void emit_direct_dicts(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  for (int c = 0; c < g.s.NC; c++) {
    if (jit_kind(g.kinds[c]).conv != CV_VDICT) continue;
    if (direct_is_factor(g, c))
      emitf(o, "    svd%d[pb][tid] = vd%d[tid];\n", c, c);
    if (!direct_has_pred(g, c)) continue;
    /* entries past the batch's count are 0.0 and no code names them */
    emitf(o, "    { const double x = vd%d[tid];\n"
             "      int in = 1;\n", c);
    for (int i = 0; i < p->npreds_d; i++)
      if (p->preds_d[i].cslot == c)
        emitf(o, "      in &= (x >= pd%d_lo) & (x <= pd%d_hi);\n", i, i);
    emitf(o, "      const u64 m = __ballot(in);\n"
             "      if ((tid & 63) == 0) spass%d[pb][tid >> 6] = m; }\n", c);
  }
  o += "    __syncthreads();\n";
  for (int c = 0; c < g.s.NC; c++)
    if (jit_kind(g.kinds[c]).conv == CV_VDICT && direct_has_pred(g, c))
      emitf(o, "    const unsigned *pw%d = (const unsigned *)spass%d[pb];\n", c, c);
}

/* the staged loads of DS rows per lane from `base_expr`, for a step that
 * holds at least one row.  Addresses are the step's uniform base plus a lane
 * offset below DS * WG, so each load takes one 32-bit offset register.  The
 * lane offset is clamped to the tile's last row, so every lane loads inside
 * the column body without a branch; `ok` drops the clamped rows.  (A second,
 * unclamped copy of the loads for whole steps cost registers: with it the
 * 4-slot kernel spilled at 64 VGPRs.) */
static void emit_direct_load(Gen &g, const char *base_expr, const char *ind) {
  std::string &o = g.o;
  emitf(o, "%sif (%s < tile_end) {\n"
           "#pragma unroll\n"
           "%s  for (int k = 0; k < DS; k++) {\n"
           "%s    const unsigned rr = min((unsigned)(tid + k * WG),\n"
           "%s                            (unsigned)(tile_end - 1 - (%s)));\n",
        ind, base_expr, ind, ind, ind, base_expr);
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c]) continue;
    const JitKind &K = jit_kind(g.kinds[c]);
    emitf(o, "%s    x%d[k] = ((const GAS %s *)(body%d + (u64)(%s) * %d))[rr];\n",
          ind, c, K.mem, c, base_expr, K.bytes);
  }
  emitf(o, "%s  }\n%s}\n", ind, ind);
}

/* pass A of a step: every slot's `ok`, the factor inputs kept, and the late
 * loads issued under `ok` (the contract of emit_late_stash) */
static void emit_direct_pass_a(Gen &g) {
  std::string &o = g.o;
  const sn_dev_plan *p = g.p;
  o += "      int okv[DS];\n";
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c]) emitf(o, "      double e%d[DS];\n", c);
    else if (direct_is_factor(g, c))
      emitf(o, "      %s f%d[DS];\n", direct_reg_type(jit_kind(g.kinds[c])), c);
  }
  o += "#pragma unroll\n"
       "      for (int k = 0; k < DS; k++) {\n"
       "        const int r = tid + k * WG;\n"
       "        int ok = base + r < tile_end;\n";
  emit_delete_pred(g);
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c] || !direct_has_pred(g, c)) continue;
    if (jit_kind(g.kinds[c]).conv == CV_VDICT) {
      emitf(o, "        ok &= (int)((pw%d[x%d[k] >> 5] >> (x%d[k] & 31u)) & 1u);\n",
            c, c, c);
      continue;
    }
    for (int i = 0; i < p->npreds_d; i++)
      if (p->preds_d[i].cslot == c)
        emitf(o, "        { const double x = (double)x%d[k];\n"
                 "          ok &= (x >= pd%d_lo) & (x <= pd%d_hi); }\n", c, i, i);
  }
  o += "        okv[k] = ok;\n";
  for (int c = 0; c < g.s.NC; c++) {
    if (g.s.late[c])
      emitf(o, "        e%d[k] = 0.0;\n"
               "        if (ok) e%d[k] = ((const GAS double *)(body%d + (u64)base * 8))[r];\n",
            c, c, c);
    else if (direct_is_factor(g, c))
      emitf(o, "        f%d[k] = x%d[k];\n", c, c);
  }
  o += "      }\n";
}

/* va<a>: each aggregate's input value for this row */
static void emit_agg_values(Gen &g) {
  std::string &o = g.o;
  /* factor read: i64 slots hold raw bits in the LDS image — emit the
   * convert only for those slots (compile-time; i64_mask is in the shape) */
  auto factor = [&](int a, int i, int cs, double fa, double fm) {
    const std::string f = g.s.late[cs] ? strf("e%d[k]", cs)
        : g.s.direct ? direct_factor(g, cs)
        : plan_col_is_i64(g.p, cs)
        ? strf("(double)__double_as_longlong(sval[%d][r])", g.s.srow[cs])
        : strf("sval[%d][r]", g.s.srow[cs]);
    if (ftriv(fa, fm)) return f;
    return strf("__builtin_fma(ag%d_m%d, %s, ag%d_a%d)", a, i, f.c_str(), a, i);
  };
  for (int a = 0; a < g.s.NA; a++) {
    const sn_dev_agg &A = g.p->aggs[a];
    if (A.nf < 1) { emitf(o, "        const double va%d = 1.0;\n", a); continue; }
    /* the register mode replaces a non-finite value before its fma */
    emitf(o, "        %sdouble va%d = %s", g.s.acc == ACC_REGS ? "" : "const ", a,
          factor(a, 0, A.c0, A.a0, A.m0).c_str());
    if (A.nf >= 2) emitf(o, " * %s", factor(a, 1, A.c1, A.a1, A.m1).c_str());
    if (A.nf >= 3) emitf(o, " * %s", factor(a, 2, A.c2, A.a2, A.m2).c_str());
    o += ";\n";
  }
}

/* the row's values into the accumulator the mode keeps */
static void emit_accumulate(Gen &g) {
  std::string &o = g.o;
  const JitShape &s = g.s;
  switch (s.acc) {
    case ACC_RADIX:   /* stashed for the scatter */
      for (int a = 0; a < s.NA; a++)
        emitf(o, "        rva%d[k] = va%d;\n", a, a);
      break;
    case ACC_SPARSE: case ACC_GLOBAL: case ACC_LDS:
      /* atomics into the row of gacc (HBM, or LDS) that `slot` names */
      emitf(o, "        if (ok) {\n"
               "          %sdouble *row = &gacc[(u64)slot * %d];\n"
               "          atomicAdd((double *)&row[%d], 1.0);\n",
            s.acc == ACC_LDS ? "" : "GAS ", s.NA1, s.NA1 - 1);
      for (int a = 0; a < s.NA; a++) {
        const int op = g.p->aggs[a].op;
        if (op == 0)
          emitf(o, "          atomicAdd((double *)&row[%d], va%d);\n", a, a);
        else
          emitf(o, "          %s((unsigned long long *)&row[%d], f64ordc(va%d));\n",
                op == 1 ? "atomicMin" : "atomicMax", a, a);
        if (g.p->pac)
          emitf(o, "          atomicAdd((double *)&row[%d], 1.0);\n", s.NA + a);
      }
      o += "        }\n";
      break;
    case ACC_WBIN:
      emitf(o, "        if (ok) {\n"
               "          double *row = &wbin[tid >> 4][slot * %d];\n"
               "          atomicAdd(&row[%d], 1.0);\n", s.NA + 1, s.NA);
      for (int a = 0; a < s.NA; a++)
        emitf(o, "          atomicAdd(&row[%d], va%d);\n", a, a);
      o += "        }\n";
      break;
    case ACC_REGS: {
      /* Each row adds to its own slot alone, and a row that did not pass to
       * none.  With m = 0.0 or 1.0, fma(m, va, sum) does that in one VALU op
       * per slot and aggregate where select + add takes three, and is
       * bit-identical to it (m = 0 leaves sum, m = 1 rounds once like the
       * add), but only for finite va: fma(0, +-inf or NaN, sum) is NaN, so
       * one such value, of a filtered row included, would turn every slot of
       * the lane NaN.  One compare per aggregate and row finds those values.
       * An iteration in which some lane of the wave holds one adds the
       * passing ones straight into the block accumulator (zeroed at kernel
       * entry, LDS atomics) and hands the fma a 0.0 in their place.  The
       * rare block writes no register accumulator, so the common path keeps
       * the registers and the schedule it had without the check. */
      std::string nonfin;
      for (int a = 0; a < s.NA; a++)
        if (g.p->aggs[a].op == 0 && g.p->aggs[a].nf >= 1)
          nonfin += strf("%s!(__builtin_fabs(va%d) <= 1.7976931348623157e308)",
                         nonfin.empty() ? "" : " |\n            ", a);
      if (!nonfin.empty()) {
        emitf(o, "        if (__ballot(%s)) {\n", nonfin.c_str());
        for (int a = 0; a < s.NA; a++)
          if (g.p->aggs[a].op == 0 && g.p->aggs[a].nf >= 1)
            emitf(o, "          if (!(__builtin_fabs(va%d) <= 1.7976931348623157e308)) {\n"
                     "            if (ok) atomicAdd(&bacc[slot * %d + %d], va%d);\n"
                     "            va%d = 0.0;\n"
                     "          }\n", a, s.NA1, a, a, a);
        o += "        }\n";
      }
      for (int a = 0; a < s.NA; a++)
        if (g.p->aggs[a].op != 0)
          emitf(o, "        const u64 vo%d = f64ordc(va%d);\n", a, a);
      emitf(o, "#pragma unroll\n        for (int s = 0; s < %d; s++) {\n"
               "          const bool mine = ok && slot == s;\n"
               "          const double m = mine ? 1.0 : 0.0;\n"
               "          rc[s] += m;\n", s.NS);
      for (int a = 0; a < s.NA; a++) {
        const int op = g.p->aggs[a].op;
        if (op == 0)
          emitf(o, "          sums[s][%d] = __builtin_fma(m, va%d, sums[s][%d]);\n",
                a, a, a);
        else
          emitf(o, "          if (mine && vo%d %s ords[s][%d]) ords[s][%d] = vo%d;\n",
                a, op == 1 ? "<" : ">", a, a, a);
      }
      o += "        }\n";
      break;
    }
    case ACC_KEYLESS:
      for (int a = 0; a < s.NA; a++) {
        emitf(o, "        sums[%d] += ok ? va%d : 0.0;\n", a, a);
        emitf(o, "        cnts[%d] += ok ? 1.0 : 0.0;\n", a);
      }
      o += "        rcnt += ok ? 1.0 : 0.0;\n";
      break;
  }
}

/* radix pass B: reserve contiguous global space per (chunk, partition) —
 * one global atomic per NON-EMPTY partition per chunk, not one per row —
 * then scatter the stashed records to [base, base+count) */
static void emit_radix_scatter(Gen &g) {
  std::string &o = g.o;
  emitf(o, "      __syncthreads();\n"
           "      for (int i = tid; i < npart; i += WG) {\n"
           "        const int c = phist[i];\n"
           "        phist[i] = c ? atomicAdd(&pcount[i], c) : 0;\n"
           "      }\n"
           "      __syncthreads();\n"
           "#pragma unroll\n"
           "      for (int k = 0; k < CHUNK / WG; k++) {\n"
           "        if (!rok[k]) continue;\n"
           "        const u64 off = (u64)phist[rpk[k]] + (u64)rrnk[k];\n"
           "        if (off >= (u64)percap) { atomicOr(hflags + 3, 1); continue; }\n"
           "        GAS double *rec = precs + ((u64)rpk[k] * (u64)percap + off) * %d;\n"
           "        ((GAS i64 *)rec)[0] = rkey[k];\n", 1 + g.s.NA);
  for (int a = 0; a < g.s.NA; a++)
    emitf(o, "        rec[%d] = rva%d[k];\n", 1 + a, a);
  o += "      }\n";
}

/* copy a block-level accumulator of nv cells to the block's scratch row */
static void emit_store_row(Gen &g, const char *cell) {
  emitf(g.o, "  __syncthreads();\n"
           "  for (int i = tid; i < %d; i += WG)\n"
           "    out[(u64)blockIdx.x * %d + i] = %s;\n", g.s.nv, g.s.nv, cell);
}

/* after the tile loop: the block's partials to its scratch row */
static void emit_flush(Gen &g) {
  std::string &o = g.o;
  const JitShape &s = g.s;
  switch (s.acc) {
    case ACC_GLOBAL: case ACC_SPARSE: case ACC_RADIX:
      /* nothing to flush — the HBM accumulator holds the single partial set */
      break;
    case ACC_LDS:
      /* gacc IS the block accumulator — flush it straight to the scratch row */
      emit_store_row(g, "gacc[i]");
      break;
    case ACC_WBIN:
      emitf(o, "  __syncthreads();\n"
               "  for (int i = tid; i < %d; i += WG) {\n"
               "    double acc = 0.0;\n"
               "#pragma unroll\n"
               "    for (int w = 0; w < 16; w++) acc += wbin[w][i];\n"
               "    out[(u64)blockIdx.x * %d + i] = acc;\n"
               "  }\n", s.nv, s.nv);
      break;
    case ACC_REGS:
      /* block reduce into LDS bacc (zeroed at entry) then scratch row */
      emitf(o, "#pragma unroll\n  for (int s = 0; s < %d; s++) {\n", s.NS);
      for (int a = 0; a < s.NA; a++) {
        const int op = g.p->aggs[a].op;
        if (op == 0)
          emitf(o, "    { double x = wsum(sums[s][%d]);\n"
                   "      if ((tid & 63) == 0 && x != 0.0) atomicAdd(&bacc[s * %d + %d], x); }\n",
                a, s.NA1, a);
        else
          emitf(o, "    { const u64 x = %s(ords[s][%d]);\n"
                   "      if ((tid & 63) == 0)\n"
                   "        %s((unsigned long long *)&bacc[s * %d + %d], x); }\n",
                op == 1 ? "wminu" : "wmaxu", a,
                op == 1 ? "atomicMin" : "atomicMax", s.NA1, a);
      }
      emitf(o, "    { double x = wsum(rc[s]);\n"
               "      if ((tid & 63) == 0 && x != 0.0) {\n"
               "        atomicAdd(&bacc[s * %d + %d], x);\n", s.NA1, s.NA1 - 1);
      if (g.p->pac)
        for (int a = 0; a < s.NA; a++)
          emitf(o, "        atomicAdd(&bacc[s * %d + %d], x);\n", s.NA1, s.NA + a);
      o += "      } }\n  }\n";
      emit_store_row(g, "bacc[i]");
      break;
    case ACC_KEYLESS:
      emit_acc_init(o, g, "bacc", s.nv, 0);
      for (int a = 0; a < s.NA; a++) {
        emitf(o, "  { double x = wsum(sums[%d]);\n"
                 "    if ((tid & 63) == 0 && x != 0.0) atomicAdd(&bacc[%d], x); }\n", a, a);
        emitf(o, "  { double x = wsum(cnts[%d]);\n"
                 "    if ((tid & 63) == 0 && x != 0.0) atomicAdd(&bacc[%d], x); }\n",
              a, g.na_t + a);
      }
      emitf(o, "  { double x = wsum(rcnt);\n"
               "    if ((tid & 63) == 0 && x != 0.0) atomicAdd(&bacc[%d], x); }\n",
            2 * g.na_t);
      emit_store_row(g, "bacc[i]");
      break;
  }
  o += "}\n";
}

/* rows per lane and step of the direct kernel.  SN_DIRECT_SLOTS (4, 8 or
 * 16) and SN_DIRECT_PREFETCH=0 exist for the measurements of DESIGN.md §2d;
 * both are read once per process, before the first kernel is generated. */
static int direct_slots(void) {
  static const int v = [] {
    const char *e = getenv("SN_DIRECT_SLOTS");
    const int n = e ? atoi(e) : 0;
    return n == 4 || n == 8 || n == 16 ? n : JIT_DIRECT_SLOTS;
  }();
  return v;
}
static int direct_prefetch(void) {
  static const int v = [] {
    const char *e = getenv("SN_DIRECT_PREFETCH");
    return !e || e[0] != '0';
  }();
  return v;
}

/* the direct kernel: the same prelude, signature, literals, tile head,
 * value expressions, accumulate and flush as every keyless kernel; its own
 * declarations, per-tile dictionary work and row loop */
static void gen_direct(Gen &g) {
  std::string &o = g.o;
  /* waves traded for registers: 8 slots with the next step's loads in
   * flight take about 100 VGPRs, that is 4 waves per SIMD, and measured
   * faster than 4 slots in 64 VGPRs at 8 waves */
  g.s.occupancy = 32 / direct_slots();
  emitf(o, "#define DS %d\n", direct_slots());
  emit_signature(g);
  emit_literals(g);
  emit_direct_decl(g);
  emit_tile_prologue(g);
  emit_direct_dicts(g);
  emit_direct_load(g, "tile.row_start", "    ");
  o += "    for (int base = tile.row_start; base < tile_end; base += DS * WG) {\n";
  emit_direct_pass_a(g);
  o += "      const int nbase = base + DS * WG;\n";
  /* behind the late loads in issue order: waiting for those leaves the next
   * step's staged loads in flight */
  if (direct_prefetch()) emit_direct_load(g, "nbase", "      ");
  o += "#pragma unroll\n"
       "      for (int k = 0; k < DS; k++) {\n"
       "        const int ok = okv[k];\n"
       "        if (__popcll(__ballot(ok)) == 0) continue;\n";
  emit_agg_values(g);
  emit_accumulate(g);
  o += "      }\n";
  if (!direct_prefetch()) emit_direct_load(g, "nbase", "      ");
  o += "    }\n"
       "    pb ^= 1;\n"
       "  }\n";
  emit_flush(g);
}

/* Generate the specialized kernel source.
 * kinds[c]: SN_K_* per used column slot (uniform across batches).
 * Layout contract identical to the interpreted kernels:
 *   keyless: scratch row [2*na_t+1] = [sums][counts][rowcount]
 *   grouped: scratch row [nslots*(naggs+1)], rowcount at +naggs.
 * (Fused register pass, stage-time predicate folding: measured slower and
 * removed — DESIGN.md, "Built, MEASURED, and reverted".) */
static std::string gen_source(const sn_dev_plan *p, const int *kinds,
                              int nslots, int na_t, int has_del) {
  Gen g = { std::string(), p, kinds, na_t, has_del,
            jit_classify(p, kinds, nslots, na_t, has_del) };
  std::string &o = g.o;
  const bool radix = g.s.acc == ACC_RADIX;

  emit_prelude(o);
  /* a value-dictionary column reads one more descriptor member; its pin is
   * emitted with it, so kernels without such a column keep their text */
  for (int c = 0; c < g.s.NC; c++)
    if (jit_kind(kinds[c]).conv == CV_VDICT) {
      emitf(o, "static_assert(__builtin_offsetof(sn_dev_col, rle_vals) == %zu, "
               "\"layout mirror differs from engine_internal.h\");\n",
            offsetof(sn_dev_col, rle_vals));
      break;
    }
  if (g.s.direct) {
    gen_direct(g);
    return std::move(g.o);
  }
  emit_order_helpers(g);
  emit_signature(g);
  emit_literals(g);
  emit_acc_decl(g);
  emit_probe_decl(g);
  emit_stage_regs(g);
  if (g.s.probe == PROBE_SLUT) emit_slut_pack(g);

  /* per tile: chunks of CHUNK rows, double-buffered through registers —
   * chunk n+1's global loads fly while chunk n's row pass runs from LDS */
  emit_tile_prologue(g);
  o += "    int staged = 0;\n"
       "    if (tile.row_start + CHUNK <= tile_end) {\n";
  emit_stage_load(g, "tile.row_start", "      ");
  o += "      staged = 1;\n    }\n"
       "    for (int base = tile.row_start; base < tile_end; base += CHUNK) {\n"
       "      const int rows = min(CHUNK, tile_end - base);\n";
  if (radix)   /* previous chunk's scatter is behind the tail barrier */
    o += "      for (int i = tid; i < npart; i += WG) phist[i] = 0;\n";
  o += "      if (staged) {\n";
  if (g.s.probe == PROBE_SPAY) emit_spay_from_regs(g);
  emit_stage_write(g, "        ");
  o += "      } else {\n";
  emit_scalar_tail(g);
  o += "      }\n"
       "      __syncthreads();\n"
       "      const int nbase = base + CHUNK;\n"
       "      const int next_staged = nbase + CHUNK <= tile_end;\n"
       "      if (next_staged) {\n";
  emit_stage_load(g, "nbase", "        ");
  o += "      }\n";
  if (g.s.probe == PROBE_SPAY) emit_spay_from_image(g);

  /* row pass: predicates, probe, slot, values and accumulate in one sweep */
  if (radix) emit_radix_stash(g);
  if (g.s.nlate) emit_late_stash(g);
  o += radix || g.s.nlate ? "#pragma unroll\n" : "#pragma unroll 2\n";
  o += "      for (int k = 0; k < CHUNK / WG; k++) {\n"
       "        const int r = tid + k * WG;\n"
       "        int ok = r < rows;\n";
  emit_row_predicates(g);
  if (radix)   /* before the wave skip: pass B keys off rok alone */
    o += "        rok[k] = ok;\n";
  if (g.s.nlate) emit_late_split(g);
  o += "        if (__popcll(__ballot(ok)) == 0) continue;\n";
  emit_join_probe(g);
  emit_slot(g);
  emit_agg_values(g);
  emit_accumulate(g);
  o += "      }\n";
  if (radix) emit_radix_scatter(g);
  o += "      __syncthreads();\n"
       "      staged = next_staged;\n"
       "    }\n"
       "  }\n";

  emit_flush(g);
  return std::move(g.o);
}

/* compile (or fetch) the kernel for this plan; returns NULL on any failure
 * (caller falls back to the interpreted kernels) */
extern "C" void *sn_jit_get(void *cache, const sn_dev_plan *p,
                            const int *kinds, int nslots, int na_t,
                            int has_del) {
  auto *jc = (JitCache *)cache;
  if (!jc) return nullptr;
  /* hash the plan SHAPE only — predicate bounds and aggregate
   * coefficients are tokenized (read from the device plan at run time),
   * so every literal value of the same shape reuses one compiled kernel
   * (the reference's tokenized plan cache) */
  sn_dev_plan shape = *p;
  /* pointers travel as kernel params; only their NULLness shapes the
   * source.  Capacity (hcap_log2) is tokenized, so grow-and-retry and
   * fresh workspaces reuse one compiled kernel. */
  shape.jkeys = shape.jkeys ? (const int64_t *)1 : nullptr;
  shape.jpayload = shape.jpayload ? (const int32_t *)1 : nullptr;
  shape.jlut = shape.jlut ? (const int32_t *)1 : nullptr;
  shape.hkeys = nullptr;
  shape.hacc = nullptr;
  shape.hflags = nullptr;
  shape.hcap_log2 = 0;
  /* radix stays in the hash as a BOOLEAN (it changes the source; the
   * partition shift itself is read from the plan at run time) and the
   * record-buffer geometry is tokenized */
  shape.precs = nullptr;
  shape.pcount = nullptr;
  shape.percap = 0;
  shape.radix = shape.radix ? 1 : 0;
  for (int i = 0; i < 2; i++) {
    shape.inp[i].bm = shape.inp[i].bm ? (const uint64_t *)1 : nullptr;
    shape.inp[i].list = shape.inp[i].list ? (const int64_t *)1 : nullptr;
    shape.inp[i].base = 0;
    shape.inp[i].nwords = 0;
    shape.inp[i].n = 0;
  }
  auto trivm = [](double a, double m) { return (a == 0.0 && m == 1.0) ? 1.0 : 0.0; };
  for (int i = 0; i < 8; i++) { shape.preds_d[i].lo = shape.preds_d[i].hi = 0.0; }
  for (int i = 0; i < 4; i++) { shape.preds_i[i].lo = shape.preds_i[i].hi = 0; }
  for (int a = 0; a < 12; a++) {
    /* keep only the per-factor triviality bit (it changes the source) */
    double t0 = trivm(shape.aggs[a].a0, shape.aggs[a].m0);
    double t1 = trivm(shape.aggs[a].a1, shape.aggs[a].m1);
    double t2 = trivm(shape.aggs[a].a2, shape.aggs[a].m2);
    shape.aggs[a].a0 = t0; shape.aggs[a].m0 = 0.0;
    shape.aggs[a].a1 = t1; shape.aggs[a].m1 = 0.0;
    shape.aggs[a].a2 = t2; shape.aggs[a].m2 = 0.0;
  }
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *d, size_t n) {
    const uint8_t *b = (const uint8_t *)d;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  };
  mix(&shape, sizeof(shape));
  mix(kinds, sizeof(int) * SN_DEV_MAX_COLS);
  mix(&nslots, 4); mix(&na_t, 4); mix(&has_del, 4);
  {
    std::lock_guard<std::mutex> g(jc->mu);
    auto it = jc->fns.find(h);
    if (it != jc->fns.end()) return (void *)it->second.fn;
  }
  std::string src = gen_source(p, kinds, nslots, na_t, has_del);
  if (const char *dump = getenv("SN_JIT_DUMP")) {
    if (FILE *f = fopen(dump, "a")) {
      fputs(src.c_str(), f);
      fputs("\n/* ---- */\n", f);
      fclose(f);
    }
  }
  std::lock_guard<std::mutex> g(jc->mu);
  auto it = jc->fns.find(h);
  if (it != jc->fns.end()) return (void *)it->second.fn;

  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "sn_jit.cu", 0, nullptr,
                          nullptr) != HIPRTC_SUCCESS)
    return nullptr;
  const char *opts[] = { "--offload-arch=gfx950", "-O3" };
  hiprtcResult crc = hiprtcCompileProgram(prog, 2, opts);
  if (crc != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    std::vector<char> log(lsz + 1, 0);
    if (lsz) hiprtcGetProgramLog(prog, log.data());
    fprintf(stderr, "[sn_jit] compile failed:\n%s\n", log.data());
    hiprtcDestroyProgram(&prog);
    jc->fns[h] = JitFn();   /* negative-cache */
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(prog, &csz);
  std::vector<char> code(csz);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);

  JitFn jf;
  if (hipModuleLoadData(&jf.mod, code.data()) != hipSuccess) return nullptr;
  if (hipModuleGetFunction(&jf.fn, jf.mod, "jit_scan") != hipSuccess) {
    (void)hipModuleUnload(jf.mod);
    return nullptr;
  }
  /* blocks of this kernel the device holds at once: the keyless launch
   * sizes its grid by it.  Left 0 (the caller keeps its own grid) when the
   * runtime cannot say. */
  int per_cu = 0, dev = 0, cus = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, jf.fn, JIT_WG,
                                                         0) == hipSuccess &&
      per_cu > 0 && hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) == hipSuccess && cus > 0)
    jf.resident = per_cu * cus;
  jc->fns[h] = jf;
  return (void *)jf.fn;
}

/* resident blocks of a kernel sn_jit_get returned; 0 when unknown */
extern "C" int sn_jit_resident(void *cache, void *fn) {
  auto *jc = (JitCache *)cache;
  if (!jc || !fn) return 0;
  std::lock_guard<std::mutex> g(jc->mu);
  for (const auto &kv : jc->fns)
    if ((void *)kv.second.fn == fn) return kv.second.resident;
  return 0;
}

extern "C" int sn_jit_cache_count(void *cache) {
  auto *jc = (JitCache *)cache;
  if (!jc) return 0;
  std::lock_guard<std::mutex> g(jc->mu);
  return (int)jc->fns.size();
}

extern "C" int sn_jit_launch(void *fn, int grid,
                             const sn_dev_batch *batches,
                             const sn_dev_tile *tiles, int ntiles,
                             double *scratch, const int64_t *jkeys,
                             const int32_t *jpayload, const int32_t *jlut,
                             const sn_dev_plan *plan_dev, void *stream) {
  void *args[] = { (void *)&batches, (void *)&tiles, (void *)&ntiles,
                   (void *)&scratch, (void *)&jkeys, (void *)&jpayload,
                   (void *)&jlut, (void *)&plan_dev };
  hipError_t e = hipModuleLaunchKernel((hipFunction_t)fn, grid, 1, 1,
                                       256, 1, 1, 0, (hipStream_t)stream,
                                       args, nullptr);
  return (int)e;
}
