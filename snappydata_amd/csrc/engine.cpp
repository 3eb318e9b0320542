/*
 * engine.cpp — host runtime of the MI355X-native columnar scan/filter/agg
 * engine behind the C ABI declared in include/snappy_engine.h.
 *
 * Responsibilities (each mirrors a reference seam — SnappyDataInc/snappydata):
 *  - batch registry keyed by (uuid, bucket): replaces the GemFire column
 *    region entries (ColumnFormatKey/ColumnFormatValue,
 *    ColumnFormatEntry.scala:99-102) with an in-process table of
 *    device-resident batches; sn_batch_put = ExternalStore.storeColumnBatch
 *    (ExternalStore.scala:43-45) fused with upload-to-HBM.
 *  - blob header pre-parse + auxiliary decode indexes (null-count prefix per
 *    64-row word, delete bitmap, host-merged update patches) so the GPU scan
 *    decodes in O(1) per row — see engine_internal.h.
 *  - per-column global dictionary interning across batches: the reference
 *    consumes batch-local dictionary indexes inside one generated loop
 *    (DictionaryEncoding.scala:85-160, DictionaryOptimizedMapAccessor);
 *    a data-parallel engine needs batch-local -> global group mapping, built
 *    here and shipped to the kernel as a tiny per-batch map array.
 *  - host-side stats-predicate batch skip (ColumnTableScan.generateStatPredicate
 *    :820-963): conservative, never skips batches with deltas/deletes.
 *  - thin planner/validator for the hot-path plan shapes
 *    (SnappyStrategies.scala:340,547-603).
 *  - the product batch builder (ColumnBatchCreator.createAndStoreBatch,
 *    ColumnBatchCreator.scala:46-131): sn_ingest_columns encodes raw arrays
 *    into reference-format blobs (uncompressed numerics, dictionary strings —
 *    the default encoder choice of ColumnEncoding.getColumnEncoder :838-870)
 *    with a ColumnStatsSchema stats row, and a seeded TPC-H lineitem
 *    generator for benchmarks (no network: synthetic data).
 *
 * The GPU path NEVER falls back to CPU: any query on an engine without a HIP
 * device fails with SN_ERR_NOGPU.
 */
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <malloc.h>
#include <limits>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/snappy_engine.h"
#include "engine_internal.h"
#include "blob_format.h"
#include "partial_format.h"

/* ------------------------------------------------------------------ */
/* error reporting                                                     */
static thread_local char g_err[512];
static thread_local int g_err_code = SN_OK;
static int fail(int code, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  g_err_code = code;
  return code;
}
extern "C" const char *sn_last_error(void) { return g_err; }
extern "C" int32_t sn_last_error_code(void) { return g_err_code; }
extern "C" const char *sn_engine_arch(void) { return "gfx950"; }

#define HIP_OR_FAIL(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
  return fail(SN_ERR_GENERIC, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)

/* ------------------------------------------------------------------ */
/* device memory arena: bump allocator over big HBM slabs, plus a
 * size-bucketed free list so per-query transients (result buffers,
 * uncached descriptor sets, sparse plan copies) recycle instead of
 * leaking ~100 KB/query in a long-lived executor */
struct Arena {
  int device = -1;               /* -1: host-only shadow mode */
  std::vector<void *> slabs;
  std::vector<void *> host_allocs;   /* host-only mode: freed on destroy */
  size_t slab_sz = 512ull << 20;
  size_t off = 0;
  std::multimap<size_t, void *> freelist;   /* rounded size -> block */
  std::mutex mu;

  static size_t rnd(size_t n) { return (n + 255) & ~size_t(255); }

  void *alloc(size_t n) {
    std::lock_guard<std::mutex> g(mu);
    n = rnd(n);
    if (device < 0) {
      void *p = malloc(n);
      if (p) host_allocs.push_back(p);
      return p;
    }
    /* exact-bucket reuse (blocks are only ever freed at the size they
     * were allocated with, so exact match is the common case) */
    auto it = freelist.find(n);
    if (it != freelist.end()) {
      void *p = it->second;
      freelist.erase(it);
      return p;
    }
    if (slabs.empty() || off + n > slab_sz) {
      size_t sz = std::max(slab_sz, n);
      void *p = nullptr;
      if (hipMalloc(&p, sz) != hipSuccess) return nullptr;
      slabs.push_back(p);
      off = 0;
      if (sz != slab_sz) { off = n; return p; }
    }
    void *p = (char *)slabs.back() + off;
    off += n;
    return p;
  }
  /* return a block for reuse (device mode only; host blocks die with the
   * arena).  n must be the original request size. */
  void release(void *p, size_t n) {
    if (!p || device < 0) return;
    std::lock_guard<std::mutex> g(mu);
    freelist.emplace(rnd(n), p);
  }
  ~Arena() {
    for (void *p : slabs) (void)hipFree(p);
    for (void *p : host_allocs) free(p);
  }
};

/* host-merged update patch for one column of one batch */
struct Patch {
  std::vector<int32_t> pos;      /* sorted row ordinals */
  std::vector<double> val;       /* f64 value or integer bits as double;
                                    dict cols: raw GLOBAL dict id */
  std::vector<uint8_t> isnull;
};

struct Batch {
  int64_t uuid = 0;
  int32_t bucket = 0;
  int32_t num_rows = 0;
  bool has_deltas = false;
  bool has_deletes = false;
  /* device pointers */
  std::vector<void *> col_dev;        /* whole blob per column */
  std::vector<const uint32_t *> nullpfx_dev;
  const uint64_t *del_bm_dev = nullptr;
  /* per-col patch device data */
  struct PatchDev {
    const uint64_t *bm = nullptr;
    const int32_t *pos = nullptr;
    const double *val = nullptr;
    const uint64_t *nullbm = nullptr;
    int32_t n = 0;
  };
  std::vector<PatchDev> patch_dev;
  std::vector<Patch> patch_host;      /* kept for dict premultiply at query */
  std::vector<uint8_t> had_patches;   /* survives materialization: int group
                                         keys must reject patched columns
                                         (stats no longer bound the values) */
  /* RLE aux (device): cumulative run ends + values widened to f64 */
  std::vector<const int32_t *> rle_ends_dev;
  std::vector<const double *> rle_vals_dev;
  std::vector<int32_t> rle_n;
  /* premultiplied dictionary maps, cached per (mul, null_gid): profiles
   * showed ~2000 per-batch map uploads on a first Q1 SF=100 submit —
   * local2global is fixed per batch, so the device map is reusable
   * across queries with the same group geometry */
  std::vector<std::map<std::pair<int32_t, int32_t>, const int32_t *>> dictmap_cache;
  /* f2 raw ingest: device-computed stats pending a sync.  Layout:
   * [nc mins][nc maxs] as order-preserving u64 encodings (f64 ord / int
   * sign-bias); is_raw marks which columns the device bounds cover. */
  const unsigned long long *stats_dev = nullptr;
  std::vector<uint8_t> is_raw;
  bool stats_pending = false;
  /* 1-byte code sidecars of narrowed f64 columns: one arena
   * block [256-entry dictionary][num_rows codes] per column, built on device
   * at put; ndict > 0 = live, `pending` = the device result (a word of
   * narrow_nd_dev) is not read yet — sync_pending_stats resolves it and
   * returns overflowed blocks to the free list */
  struct Narrow {
    void *block = nullptr;
    int32_t ndict = 0;
    bool pending = false;
    const double *dict() const { return (const double *)block; }
    const uint8_t *codes() const {
      return (const uint8_t *)block + SN_NARROW_MAX * 8;
    }
  };
  std::vector<Narrow> narrow;
  int32_t *narrow_nd_dev = nullptr;   /* [ncols] device entry counts */
  bool narrow_pending = false;
  std::vector<ColMeta> cols;
  /* stats (parsed) */
  bool stats_valid = false;
  std::vector<double> lo_d, hi_d;
  std::vector<int64_t> lo_i, hi_i;
  std::vector<int32_t> null_count;
  std::vector<uint8_t> bounds_null;
  /* host shadow (device == -1 only) */
  std::vector<std::vector<uint8_t>> host_blobs;
};

/* what a launch needs to know about the batches it scans: the device
 * descriptor set for one plan shape, built fresh or cached on the table by
 * `sig` (the reference caches generated plans per query signature,
 * SnappySession plan cache) */
struct ScanSet {
  uint64_t sig = 0;
  size_t batch_count = 0;       /* invalidation: table grew */
  const void *db_dev = nullptr;
  const void *tl_dev = nullptr;
  size_t db_bytes = 0, tl_bytes = 0;   /* released to the free list on evict */
  int32_t ntiles = 0;
  int64_t rows = 0;
  /* JIT eligibility of this descriptor set: every batch clean with these
   * uniform stageable kinds (needed again on cache hits, when the
   * per-batch loop that derives them is skipped) */
  int jit_ok = 0;
  int jit_del = 0;
  int jit_kinds[SN_DEV_MAX_COLS] = {0};
  int pac = 0;        /* batches carry nulls on aggregate-input columns */
};

struct Table {
  std::string name;
  std::vector<sn_col_schema> schema;
  std::vector<Batch> batches;
  std::vector<ScanSet> desc_caches;
  /* global dictionary per column (string dict cols) */
  std::vector<std::vector<std::string>> gdict;
  std::vector<std::map<std::string, int32_t>> gdict_idx;
  /* longest interned entry per column: group keys beyond SN_KEY_MAX-1
   * bytes cannot travel in results/partial blocks — queries grouping on
   * such a column fail loudly instead of silently merging truncated keys */
  std::vector<int32_t> gdict_maxlen;
  /* ORDER BY on a string column: global dictionary id -> bytewise rank,
   * built on first use and rebuilt when the dictionary has grown */
  std::map<int32_t, std::vector<int32_t>> order_ranks;
  /* last adequate sparse hash-table capacity (log2): later queries start
   * there instead of rediscovering it through grow-and-retry */
  int sparse_cap_hint = 0;
  /* DecimalType(precision, scale) metadata of INT64 columns holding
   * unscaled decimals (sn_table_set_decimal); precision 0 = not decimal */
  std::vector<int8_t> dec_prec, dec_scale;
  int64_t total_rows = 0;
  std::mutex mu;
};

/* broadcast dimension (row-store stand-in): host rows + cached device
 * open-address table (HashedObjectCache analogue, HashJoinExec.scala:449-470) */
struct Dim {
  std::string name;
  std::vector<int64_t> keys;
  std::vector<std::string> attrs;          /* per-key attr (may be empty) */
  std::vector<std::string> attr_dict;      /* distinct attrs (gid order) */
  std::vector<int32_t> attr_gid;           /* per-key gid */
  /* device table (built lazily, cached) */
  const int64_t *dev_keys = nullptr;
  const int32_t *dev_payload = nullptr;
  int32_t cap_log2 = 0;
  /* dense payload LUT over [lut_min, lut_max] when the span is small */
  const int32_t *dev_lut = nullptr;
  int64_t lut_min = 0, lut_max = -1;
  int32_t attr_maxlen = 0;
  bool from_table = false;   /* device-built from a column table (f3):
                                host keys unknown, sn_dim_put forbidden */
  /* guards keys/attrs/device-table pointers: sn_dim_put may run while a
   * submit builds/reads the device table (the reference's replicated
   * region puts are similarly concurrent with task-side get()s) */
  std::mutex mu;
};

struct sn_engine {
  sn_config cfg;
  Arena arena;
  std::vector<std::unique_ptr<Table>> tables;
  std::vector<std::unique_ptr<Dim>> dims;
  hipStream_t stream = nullptr;
  bool has_gpu = false;
  /* SN_NARROW (default on, 0 = off), read once per engine: narrow
   * low-cardinality f64 columns into 1-byte code sidecars at put */
  bool narrow = true;
  /* SN_LATE (default on, 0 = off), read once per engine: a keyless compiled
   * scan reads its aggregate-only f64 columns for the passing rows alone
   * when the predicates are estimated to keep at most SN_LATE_MAX_SEL of the
   * rows.  SN_LATE=force engages whatever the estimate
   * (measurement only). */
  bool late = true, late_force = false;
  /* SN_DIRECT (default on, 0 = off), read once per engine: a late plan with
   * range predicates only, over int32/int16/narrowed columns, runs the
   * image-free kernel.  SN_GRID_RESIDENT (default on, 0 =
   * off): a keyless compiled kernel's grid comes from how many of its blocks
   * the device holds at once instead of SN_GRID_CAP. */
  bool direct = true, grid_resident = true;
  /* reusable per-engine scratch for block-partial reduction rows
   * (queries on one engine serialize on its stream) */
  double *scratch = nullptr;
  size_t scratch_sz = 0;
  /* sparse hash-aggregate workspace (reused: the sparse path reads its
   * results back inside submit, so no two queries share it live) */
  long long *hws_keys = nullptr;
  long long *hws_okeys = nullptr;
  double *hws_acc = nullptr;
  double *hws_orows = nullptr;
  int32_t *hws_flags = nullptr;   /* [0] overflow, [1] compact counter,
                                     [2] fill, [3] radix record overflow */
  int hws_cap_log2 = 0;
  size_t hws_acc_bytes = 0;
  /* radix two-pass record buffer + per-partition fill counters (engine-
   * cached like the table workspace; sized to the largest query seen) */
  double *rws_recs = nullptr;
  size_t rws_bytes = 0;
  int32_t *rws_pcount = nullptr;
  int rws_npart = 0;
  int32_t *lz4_err_dev = nullptr; /* device error word for the LZ4 decode */
  std::mutex lz4_mu;              /* serializes decode launch+sync+readback */
  /* serializes sn_query_submit: queries on one engine share the stream,
   * the block-partial scratch and the hash/radix workspaces, so two
   * submits from different threads (even on DIFFERENT tables — t->mu
   * does not cover this) must not interleave their enqueue+readback
   * sections.  Ingest does not take this lock. */
  std::mutex query_mu;
  /* pinned staging for big blob uploads: pageable hipMemcpy bounces through
   * the runtime's staging path at ~1-2 GB/s with a device sync per call
   * (measured: SF=10 ingest spent ~2 s there, 27 Mrows/s).  A pool of
   * pinned bounce slots lets concurrent ingest threads overlap their
   * host->pinned memcpys while the DMAs queue at full PCIe rate
   * (one slot: 105 Mrows/s measured; the pool removes the memcpy serial). */
  static const int PIN_SLOTS = 4;
  struct PinSlot { void *buf = nullptr; size_t sz = 0; std::mutex mu; };
  PinSlot pins[PIN_SLOTS];
  std::atomic<uint32_t> pin_rr { 0 };
  /* per-engine cache of query-compiled kernels (jit.cpp) */
  void *jit = nullptr;
  /* steady-state submit caches: device plan copies by content hash, and a
   * small HIP-event pool (create/destroy costs ~µs per query otherwise) */
  std::map<uint64_t, void *> dp_cache;
  std::vector<hipEvent_t> ev_pool;
  std::set<sn_query *> live_q;   /* outstanding queries: detached (e=NULL)
                                    at engine destroy so a later
                                    sn_query_destroy stays safe */
  std::mutex aux_mu;
  std::mutex mu;

  hipEvent_t ev_acquire() {
    { std::lock_guard<std::mutex> g(aux_mu);
      if (!ev_pool.empty()) { hipEvent_t e2 = ev_pool.back(); ev_pool.pop_back(); return e2; } }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
  }
  void ev_release(hipEvent_t ev) {
    if (!ev) return;
    std::lock_guard<std::mutex> g(aux_mu);
    if (ev_pool.size() < 16) ev_pool.push_back(ev);
    else (void)hipEventDestroy(ev);
  }
};

/* ------------------------------------------------------------------ */
extern "C" sn_engine *sn_engine_create(const sn_config *cfg) {
  auto *e = new sn_engine();
  if (cfg) e->cfg = *cfg;
  else memset(&e->cfg, 0, sizeof(e->cfg));
  if (e->cfg.column_batch_size <= 0) e->cfg.column_batch_size = 24ll << 20;
  if (e->cfg.column_max_delta_rows <= 0) e->cfg.column_max_delta_rows = 10000;
  if (e->cfg.hash_join_size <= 0) e->cfg.hash_join_size = 100ll << 20;
  if (e->cfg.shard_count <= 0) e->cfg.shard_count = 1;
  if (e->cfg.n_buckets <= 0) e->cfg.n_buckets = 128;
  if (const char *nv = getenv("SN_NARROW")) e->narrow = nv[0] != '0';
  if (const char *lv = getenv("SN_LATE")) {
    e->late = lv[0] != '0';
    e->late_force = !strcmp(lv, "force");
  }
  if (const char *dv = getenv("SN_DIRECT")) e->direct = dv[0] != '0';
  if (const char *gv = getenv("SN_GRID_RESIDENT")) e->grid_resident = gv[0] != '0';
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && e->cfg.device >= 0) {
    if (hipSetDevice(e->cfg.device) == hipSuccess &&
        hipStreamCreate(&e->stream) == hipSuccess) {
      e->has_gpu = true;
      e->arena.device = e->cfg.device;
    }
  }
  if (!e->has_gpu) {
    e->arena.device = -1;   /* host-only: ingest/encode testable, queries fail */
  } else {
    e->jit = sn_jit_cache_create();
  }
  /* big per-query result vectors (1M-group readbacks are ~24 MB) must
   * recycle through the heap, not mmap/munmap per query — the page-fault
   * churn measured as a bimodal 1.4-3.6 ms of host time per sparse query */
  (void)mallopt(M_MMAP_THRESHOLD, 256 << 20);
  (void)mallopt(M_TRIM_THRESHOLD, 256 << 20);
  return e;
}

/* D2H copy through a pinned bounce slot: pageable hipMemcpy D2H runs at
 * ~50 GB/s with run-to-run stalls (the sparse 1M-group readback measured
 * 1.4-3.6 ms of host time per query on identical kernels); the pinned DMA
 * + one host memcpy is both faster and stable */
static hipError_t d2h_copy(sn_engine *e, void *dst, const void *src, size_t n) {
  if (n < (1u << 20))
    return hipMemcpy(dst, src, n, hipMemcpyDeviceToHost);
  auto &slot = e->pins[e->pin_rr.fetch_add(1) % sn_engine::PIN_SLOTS];
  std::lock_guard<std::mutex> g(slot.mu);
  if (slot.sz < n) {
    size_t want = std::max<size_t>(n, 32u << 20);
    void *p = nullptr;
    if (hipHostMalloc(&p, want) != hipSuccess)
      return hipMemcpy(dst, src, n, hipMemcpyDeviceToHost);  /* fall back */
    if (slot.buf) (void)hipHostFree(slot.buf);
    slot.buf = p;
    slot.sz = want;
  }
  hipError_t rc = hipMemcpy(slot.buf, src, n, hipMemcpyDeviceToHost);
  if (rc != hipSuccess) return rc;
  memcpy(dst, slot.buf, n);
  return hipSuccess;
}

/* H2D copy through a pinned bounce slot (big transfers; small ones direct) */
static hipError_t h2d_copy(sn_engine *e, void *dst, const void *src, size_t n) {
  if (n < (1u << 20))
    return hipMemcpy(dst, src, n, hipMemcpyHostToDevice);
  auto &slot = e->pins[e->pin_rr.fetch_add(1) % sn_engine::PIN_SLOTS];
  std::lock_guard<std::mutex> g(slot.mu);
  if (slot.sz < n) {
    size_t want = std::max<size_t>(n, 32u << 20);
    void *p = nullptr;
    if (hipHostMalloc(&p, want) != hipSuccess)
      return hipMemcpy(dst, src, n, hipMemcpyHostToDevice);  /* fall back */
    if (slot.buf) (void)hipHostFree(slot.buf);
    slot.buf = p;
    slot.sz = want;
  }
  memcpy(slot.buf, src, n);
  return hipMemcpy(dst, slot.buf, n, hipMemcpyHostToDevice);
}

static void sn_detach_queries(sn_engine *e);   /* defined below sn_query */

extern "C" void sn_engine_destroy(sn_engine *e) {
  if (!e) return;
  sn_detach_queries(e);
  for (auto &ps : e->pins)
    if (ps.buf) (void)hipHostFree(ps.buf);
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  if (e->jit) sn_jit_cache_destroy(e->jit);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

extern "C" int32_t sn_table_define(sn_engine *e, const char *name,
                                   int32_t ncols, const sn_col_schema *schema) {
  if (!e || ncols <= 0 || ncols > 64 || !schema) { fail(SN_ERR_BADARG, "bad table args"); return SN_ERR_BADARG; }
  std::lock_guard<std::mutex> g(e->mu);
  auto t = std::make_unique<Table>();
  t->name = name ? name : "";
  t->schema.assign(schema, schema + ncols);
  t->gdict.resize(ncols);
  t->gdict_idx.resize(ncols);
  t->gdict_maxlen.assign(ncols, 0);
  e->tables.push_back(std::move(t));
  return (int32_t)e->tables.size() - 1;
}

extern "C" int32_t sn_dim_define(sn_engine *e, const char *name) {
  if (!e) return SN_ERR_BADARG;
  std::lock_guard<std::mutex> g(e->mu);
  auto d = std::make_unique<Dim>();
  d->name = name ? name : "";
  e->dims.push_back(std::move(d));
  return (int32_t)e->dims.size() - 1;
}

extern "C" int32_t sn_dim_put(sn_engine *e, int32_t dim, int64_t nkeys,
                              const int64_t *keys, const char *attr_payload,
                              const int32_t *attr_lens) {
  if (!e || dim < 0 || dim >= (int32_t)e->dims.size() || !keys || nkeys <= 0)
    return fail(SN_ERR_BADARG, "bad dim args");
  Dim *d = e->dims[dim].get();
  std::lock_guard<std::mutex> gd(d->mu);
  if (d->from_table)
    return fail(SN_ERR_BADARG, "dimension was built from a column table");
  /* INT64_MIN marks an empty slot of the device table: as a key it would be
   * stored as "empty" and overwritten by a later insert (sn_dim_from_table
   * refuses it likewise) */
  for (int64_t i = 0; i < nkeys; i++)
    if (keys[i] == INT64_MIN)
      return fail(SN_ERR_BADARG, "INT64_MIN is not a legal dimension key");
  int64_t off = 0;
  for (int64_t i = 0; i < nkeys; i++) {
    d->keys.push_back(keys[i]);
    if (attr_payload && attr_lens) {
      std::string a(attr_payload + off, (size_t)attr_lens[i]);
      off += attr_lens[i];
      int32_t gid = -1;
      for (size_t j = 0; j < d->attr_dict.size(); j++)
        if (d->attr_dict[j] == a) { gid = (int32_t)j; break; }
      if (gid < 0) { gid = (int32_t)d->attr_dict.size(); d->attr_dict.push_back(a); }
      if ((int32_t)a.size() > d->attr_maxlen) d->attr_maxlen = (int32_t)a.size();
      d->attrs.push_back(std::move(a));
      d->attr_gid.push_back(gid);
    } else {
      d->attrs.emplace_back();
      d->attr_gid.push_back(0);
    }
  }
  /* invalidate the cached device table (and the dense LUT with it) */
  d->dev_keys = nullptr; d->dev_payload = nullptr;
  d->dev_lut = nullptr; d->lut_min = 0; d->lut_max = -1;
  return SN_OK;
}

static void *up(sn_engine *e, const void *host, size_t n);
static Table *get_table(sn_engine *e, int32_t t);
static void sync_pending_stats(sn_engine *e, Table *t);

static inline uint64_t mix64h(uint64_t x) {
  x += 0x9E3779B97f4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

/* the kernel kind and byte width of an UNCOMPRESSED body of `dtype`; false
 * for types with no fixed-width body.  Callers that take only the numeric
 * types (raw ingest, patch materialization, RLE values) ask for width >= 2:
 * the 1-byte types are BOOL and INT8. */
static bool fixed_type(sn_type_t dtype, int *kind, int *width) {
  switch (dtype) {
    case SN_TYPE_DOUBLE: *kind = SN_K_F64; break;
    case SN_TYPE_INT32:  *kind = SN_K_I32; break;
    case SN_TYPE_INT64:  *kind = SN_K_I64; break;
    case SN_TYPE_FLOAT:  *kind = SN_K_F32; break;
    case SN_TYPE_INT16:  *kind = SN_K_I16; break;
    case SN_TYPE_BOOL:   *kind = SN_K_U8; break;
    case SN_TYPE_INT8:   *kind = SN_K_S8; break;
    default: return false;
  }
  *width = sn_type_width(dtype);
  return true;
}

/* device descriptor of column c of batch b: body/null pointers, encoding ->
 * SN_K_* kind, RLE aux, dictionary map, patch pointers.  The one place a new
 * encoding or kind is added — the query descriptor build and the join build
 * both come through here.  A dictionary column's map carries its global ids
 * times `mul` with nulls at `null_gid` (dict_premul; join builds pass 1, 0);
 * premul_patches uploads string patch values times `mul` for this query
 * instead of pointing at the stored global ids.  Clears *clean when the
 * column carries nulls or patches. */
static int fill_dev_col(sn_engine *e, const Table *t, Batch &b, int c, int mul,
                        int null_gid, bool premul_patches, sn_dev_col *out,
                        bool *clean) {
  const ColMeta &m = b.cols[c];
  sn_dev_col &dc = *out;
  memset(&dc, 0, sizeof(dc));
  sn_type_t dt = t->schema[c].dtype;
  dc.body = (const uint8_t *)b.col_dev[c] + m.body_off;
  dc.has_nulls = m.num_null_words > 0;
  if (dc.has_nulls) {
    dc.nullw = (const uint64_t *)((const uint8_t *)b.col_dev[c] + m.null_off);
    dc.nullpfx = b.nullpfx_dev[c];
    *clean = false;
  }
  switch (m.type_id) {
    case SN_ENC_UNCOMPRESSED: {
      int width;
      if (!fixed_type(dt, &dc.kind, &width))
        return fail(SN_ERR_UNSUPPORTED, "uncompressed %d on GPU path", (int)dt);
      break;
    }
    case SN_ENC_RUNLENGTH:
      if (b.rle_n[c] <= 0 && b.num_rows > 0)
        return fail(SN_ERR_UNSUPPORTED, "RLE col %d has no run aux", c);
      /* INT64 runs carry raw bits in rle_vals (put-time extraction) —
       * a distinct kind so read_general bitcasts instead of rounding */
      dc.kind = dt == SN_TYPE_INT64 ? SN_K_RLE_I64 : SN_K_RLE;
      dc.rle_ends = b.rle_ends_dev[c];
      dc.rle_vals = b.rle_vals_dev[c];
      dc.rle_n = b.rle_n[c];
      break;
    case SN_ENC_BOOLEAN_BITSET:
      dc.kind = SN_K_BOOLBIT;
      break;
    case SN_ENC_DICTIONARY:
    case SN_ENC_BIG_DICTIONARY: {
      if (dt != SN_TYPE_STRING)
        return fail(SN_ERR_UNSUPPORTED,
                    "int dictionary col %d on GPU path not yet supported", c);
      dc.kind = m.type_id == SN_ENC_DICTIONARY ? SN_K_DICT16 : SN_K_DICT32;
      /* local->premultiplied-global map, cached per (mul, null_gid) —
       * local2global is fixed per batch, so queries with the same
       * group geometry reuse one device map */
      dc.null_gid = null_gid;
      auto &mcache = b.dictmap_cache[c];
      auto mit = mcache.find({ mul, null_gid });
      if (mit != mcache.end()) {
        dc.dictmap = mit->second;
      } else {
        std::vector<int32_t> map(m.local2global.size() + 1);
        for (size_t i = 0; i < m.local2global.size(); i++)
          map[i] = m.local2global[i] * mul;
        /* index == numElements denotes null (DictionaryEncoding.scala:90) */
        map[m.local2global.size()] = null_gid;
        dc.dictmap = (const int32_t *)up(e, map.data(), map.size() * 4);
        if (!dc.dictmap) return fail(SN_ERR_NOMEM, "dictmap upload");
        mcache.emplace(std::make_pair(mul, null_gid), dc.dictmap);
      }
      break;
    }
    default:
      return fail(SN_ERR_UNSUPPORTED, "encoding %d on GPU path not yet supported",
                  m.type_id);
  }
  if (b.patch_dev[c].n > 0) {
    *clean = false;
    const Batch::PatchDev &pd = b.patch_dev[c];
    dc.patch_bm = pd.bm;
    dc.patch_pos = pd.pos;
    dc.patch_nullbm = pd.nullbm;
    dc.patch_n = pd.n;
    if (dt == SN_TYPE_STRING && premul_patches) {
      /* premultiply global ids for this query */
      std::vector<double> pv(b.patch_host[c].val.size());
      for (size_t i = 0; i < pv.size(); i++)
        pv[i] = b.patch_host[c].val[i] * mul;
      dc.patch_val = (const double *)up(e, pv.data(), pv.size() * 8);
    } else {
      dc.patch_val = pd.val;   /* string patches carry global ids (mul 1) */
    }
  }
  return SN_OK;
}

/* ---- partitioned-partitioned (colocated) join build: populate a Dim from
 * a resident column table, built ON DEVICE (k_join_build) — the
 * HashJoinExec per-task ObjectHashSet build + HashedObjectCache reuse
 * (HashJoinExec.scala:285-520, :449-470).  Colocated tables join
 * bucket-locally, so each shard builds from its own build-side rows. ---- */
extern "C" int32_t sn_dim_from_table(sn_engine *e, int32_t dim, int32_t table,
                                     int32_t key_col, int32_t attr_col) {
  if (!e || dim < 0 || dim >= (int32_t)e->dims.size())
    return fail(SN_ERR_BADARG, "bad dim handle");
  Table *t = get_table(e, table);
  if (!t) return fail(SN_ERR_BADARG, "bad table");
  if (!e->has_gpu)
    return fail(SN_ERR_NOGPU, "join build runs on device");
  Dim *d = e->dims[dim].get();
  std::lock_guard<std::mutex> gd(d->mu);
  if (d->dev_keys || !d->keys.empty())
    return fail(SN_ERR_BADARG, "dimension is not empty");
  std::lock_guard<std::mutex> g(t->mu);
  const int nc = (int)t->schema.size();
  if (key_col < 0 || key_col >= nc) return fail(SN_ERR_BADARG, "bad key col");
  sn_type_t kdt = t->schema[key_col].dtype;
  if (kdt != SN_TYPE_INT32 && kdt != SN_TYPE_INT64 && kdt != SN_TYPE_INT16)
    return fail(SN_ERR_UNSUPPORTED, "join build key must be int16/int32/int64");
  const bool has_attr = attr_col >= 0;
  if (has_attr) {
    if (attr_col >= nc || t->schema[attr_col].dtype != SN_TYPE_STRING)
      return fail(SN_ERR_UNSUPPORTED, "attr col must be a string column");
    if (t->schema[attr_col].nullable)
      return fail(SN_ERR_UNSUPPORTED,
                  "nullable attribute columns not supported in join build");
    if (t->gdict_maxlen[attr_col] > SN_KEY_MAX - 1)
      return fail(SN_ERR_UNSUPPORTED, "attr exceeds the group-key limit");
  }
  /* (key columns may be nullable: null keys never join and are masked at
   * build time via the validity bitmap) */
  if (t->total_rows > (1ll << 23))
    return fail(SN_ERR_UNSUPPORTED,
                "build side exceeds 2^23 rows (HashJoinSize-class bound)");
  sync_pending_stats(e, t);   /* the LUT span reads stats bounds */

  sn_dev_plan dp;
  memset(&dp, 0, sizeof(dp));
  dp.nused = has_attr ? 2 : 1;
  dp.i64_mask = kdt == SN_TYPE_INT64 ? 1u : 0u;
  dp.naggs = 1;

  std::vector<sn_dev_batch> hb;
  std::vector<sn_dev_tile> ht;
  const int used[2] = { key_col, attr_col };
  for (auto &b : t->batches) {
    sn_dev_batch db;
    memset(&db, 0, sizeof(db));
    db.num_rows = b.num_rows;
    db.del_bm = b.del_bm_dev;
    bool clean = !b.has_deletes;
    for (int ui = 0; ui < dp.nused; ui++) {
      /* payload gid = table-global dictionary id (mul 1, null slot 0); the
       * dtype checks above leave only int16/int32/int64 keys and a string
       * attribute to reach the fill */
      int rc = fill_dev_col(e, t, b, used[ui], 1, 0, false, &db.cols[ui], &clean);
      if (rc != SN_OK) return rc;
    }
    db.clean = clean ? 1 : 0;
    int32_t bi = (int32_t)hb.size();
    hb.push_back(db);
    for (int32_t r = 0; r < b.num_rows; r += SN_TILE_ROWS)
      ht.push_back({ bi, r });
  }

  int cap_log2 = 10;
  while ((1ll << cap_log2) < 2 * t->total_rows && cap_log2 < 25) cap_log2++;
  const size_t cap = 1ull << cap_log2;
  long long *hk = (long long *)e->arena.alloc(cap * 8);
  int32_t *hp = (int32_t *)e->arena.alloc(cap * 4);
  int32_t *flags = (int32_t *)e->arena.alloc(64);
  void *dp_dev = e->arena.alloc(sizeof(dp));
  void *db_dev = hb.empty() ? nullptr : e->arena.alloc(hb.size() * sizeof(sn_dev_batch));
  void *tl_dev = ht.empty() ? nullptr : e->arena.alloc(ht.size() * sizeof(sn_dev_tile));
  if (!hk || !hp || !flags || !dp_dev || (!hb.empty() && (!db_dev || !tl_dev)))
    return fail(SN_ERR_NOMEM, "join build alloc");
  if (hipMemsetAsync(flags, 0, 16, e->stream) != hipSuccess ||
      hipMemcpy(dp_dev, &dp, sizeof(dp), hipMemcpyHostToDevice) != hipSuccess)
    return fail(SN_ERR_GENERIC, "join build upload");
  if (!hb.empty() &&
      (hipMemcpy(db_dev, hb.data(), hb.size() * sizeof(sn_dev_batch),
                 hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(tl_dev, ht.data(), ht.size() * sizeof(sn_dev_tile),
                 hipMemcpyHostToDevice) != hipSuccess))
    return fail(SN_ERR_GENERIC, "join build upload");
  int rc = sn_launch_join_build(&dp, (const sn_dev_plan *)dp_dev,
                                (const sn_dev_batch *)db_dev,
                                (const sn_dev_tile *)tl_dev,
                                (int32_t)ht.size(), hk, hp, cap_log2,
                                has_attr ? 1 : 0, flags, e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "join build: %s",
                hipGetErrorString((hipError_t)rc));
  if (hipStreamSynchronize(e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "join build sync");
  int32_t fl[2] = { 0, 0 };
  (void)hipMemcpy(fl, flags, 8, hipMemcpyDeviceToHost);
  if (fl[0])
    return fail(SN_ERR_BADARG,
                "duplicate build keys with conflicting payloads (or a "
                "sentinel-valued key)");
  if (fl[1]) return fail(SN_ERR_OVERFLOW, "join build table full");

  d->dev_keys = (const int64_t *)hk;
  d->dev_payload = hp;
  d->cap_log2 = cap_log2;
  d->from_table = true;
  if (has_attr) {
    d->attr_dict = t->gdict[attr_col];
    d->attr_maxlen = t->gdict_maxlen[attr_col];
  } else {
    d->attr_dict.assign(1, std::string());
  }
  /* dense LUT when the key span (from stats bounds) is small.  The bounds
   * must be ones the engine can trust: a batch whose key column carries
   * update deltas or patches may hold keys outside its stats row (the rule
   * of int_key_span), so it leaves the dimension on the hash table */
  bool have_span = !t->batches.empty();
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (auto &b : t->batches) {
    if (!b.stats_valid || b.bounds_null.size() <= (size_t)key_col ||
        b.bounds_null[key_col] || b.has_deltas ||
        (b.had_patches.size() > (size_t)key_col && b.had_patches[key_col])) {
      have_span = false;
      break;
    }
    mn = std::min(mn, b.lo_i[key_col]);
    mx = std::max(mx, b.hi_i[key_col]);
  }
  const int64_t span = have_span ? sn_lut_span(mn, mx) : 0;
  if (span > 0) {
    /* flags[2]: a build key outside [mn, mx] (zeroed with the build flags).
     * The stats row of a put without deltas can still be wrong, so the
     * kernel checks every key and a LUT that misses one is dropped. */
    int32_t *lut = (int32_t *)e->arena.alloc((size_t)span * 4);
    int32_t oob = 1;
    if (lut &&
        hipMemsetAsync(lut, 0xff, (size_t)span * 4, e->stream) == hipSuccess &&
        sn_launch_hash_to_lut(hk, hp, (long long)cap, lut, mn, mx, flags + 2,
                              e->stream) == 0 &&
        hipStreamSynchronize(e->stream) == hipSuccess &&
        hipMemcpy(&oob, flags + 2, 4, hipMemcpyDeviceToHost) == hipSuccess &&
        oob == 0) {
      d->dev_lut = lut;
      d->lut_min = mn;
      d->lut_max = mx;
    } else if (lut) {
      (void)hipStreamSynchronize(e->stream);   /* nothing in flight on it */
      e->arena.release(lut, (size_t)span * 4);
    }
  }
  return SN_OK;
}

/* build (or reuse) the device open-address table: the broadcast into HBM */
static int dim_device_table(sn_engine *e, Dim *d) {
  std::lock_guard<std::mutex> gd(d->mu);
  if (d->dev_keys) return SN_OK;
  int32_t lg = 1;
  while ((1u << lg) < 2 * d->keys.size() + 1) lg++;
  size_t cap = 1ull << lg;
  std::vector<int64_t> hk(cap, INT64_MIN);
  std::vector<int32_t> hp(cap, -1);
  for (size_t i = 0; i < d->keys.size(); i++) {
    int64_t k = d->keys[i];
    uint32_t h = (uint32_t)mix64h((uint64_t)k) & (cap - 1);
    while (hk[h] != INT64_MIN) {
      if (hk[h] == k) return fail(SN_ERR_BADARG, "duplicate dimension key");
      h = (h + 1) & (cap - 1);
    }
    hk[h] = k;
    hp[h] = d->attr_gid[i];
  }
  d->dev_keys = (const int64_t *)up(e, hk.data(), cap * 8);
  d->dev_payload = (const int32_t *)up(e, hp.data(), cap * 4);
  d->cap_log2 = lg;
  if (!d->dev_keys || !d->dev_payload) return fail(SN_ERR_NOMEM, "dim upload");
  /* dense LUT when the key span is small (16M entries = 64 MB worst case;
   * typical dimensions are far smaller and sit in L2): replaces the
   * dependent open-address chain with one load per probed row */
  if (!d->keys.empty()) {
    int64_t mn = d->keys[0], mx = d->keys[0];
    for (int64_t k : d->keys) { mn = k < mn ? k : mn; mx = k > mx ? k : mx; }
    const int64_t span = sn_lut_span(mn, mx);
    if (span > 0) {
      std::vector<int32_t> lut((size_t)span, -1);
      for (size_t i = 0; i < d->keys.size(); i++)
        lut[(size_t)(d->keys[i] - mn)] = d->attr_gid[i];
      d->dev_lut = (const int32_t *)up(e, lut.data(), lut.size() * 4);
      d->lut_min = mn; d->lut_max = mx;
    }
  }
  return SN_OK;
}

static Table *get_table(sn_engine *e, int32_t t) {
  if (!e || t < 0 || t >= (int32_t)e->tables.size()) return nullptr;
  return e->tables[t].get();
}

/* ---- LZ4 compression wrapper (CompressionUtils.scala:53-61,132-160):
 * [int32 -codecId][int32 uncompressedLen][payload]; codec 1 = LZ4 (default),
 * 2 = Snappy.  The engine decompresses on put, mirroring
 * ColumnFormatValue.getValueRetain(DECOMPRESS)
 * (ColumnFormatEntry.scala:267-330).  liblz4 loaded lazily via dlopen
 * (runtime-only .so in this image). ---- */
typedef int (*lz4_decomp_fn)(const char *, char *, int, int);
static lz4_decomp_fn get_lz4(void) {
  static lz4_decomp_fn fn = nullptr;
  static bool tried = false;
  if (!tried) {
    tried = true;
    void *h = dlopen("liblz4.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("liblz4.so", RTLD_NOW | RTLD_GLOBAL);
    if (h) fn = (lz4_decomp_fn)dlsym(h, "LZ4_decompress_safe");
  }
  return fn;
}

/* if blob is codec-wrapped, decompress into *out and return 1; 0 if plain;
 * negative = error */
static int maybe_decompress(const uint8_t *blob, int64_t len,
                            std::vector<uint8_t> *out) {
  if (len < 8) return 0;
  int32_t tag = rd_i32(blob);
  if (tag >= 0) return 0;                  /* plain typeId */
  int32_t codec = -tag;
  int32_t ulen = rd_i32(blob + 4);
  if (ulen <= 0) return fail(SN_ERR_BADFORMAT, "bad compressed length");
  if (codec == 1) {
    lz4_decomp_fn fn = get_lz4();
    if (!fn) return fail(SN_ERR_UNSUPPORTED, "liblz4 unavailable");
    out->resize((size_t)ulen);
    int n = fn((const char *)blob + 8, (char *)out->data(),
               (int)(len - 8), ulen);
    if (n != ulen) return fail(SN_ERR_BADFORMAT, "LZ4 decompress failed (%d)", n);
    return 1;
  }
  if (codec == 2) {
    if (snappy_decompress(blob + 8, len - 8, out) != 0 ||
        (int64_t)out->size() != ulen)
      return fail(SN_ERR_BADFORMAT, "Snappy decompress failed");
    return 1;
  }
  return fail(SN_ERR_UNSUPPORTED, "codec %d not supported", codec);
}

/* upload helper */
static void *up(sn_engine *e, const void *host, size_t n) {
  void *d = e->arena.alloc(n);
  if (!d) return nullptr;
  if (e->arena.device >= 0) {
    if (hipMemcpy(d, host, n, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  } else {
    memcpy(d, host, n);
  }
  return d;
}

/* ---- f64 narrowing: 1-byte code sidecars built at put ---- */

/* host reference of sn_launch_f64_narrow's contract (engine_internal.h) */
extern "C" void sn_f64_narrow_host(const double *body, int64_t n,
                                   uint8_t *codes, double *dict,
                                   int32_t *ndict) {
  std::vector<uint64_t> keys;          /* distinct patterns, kept ascending */
  bool fits = true;
  for (int64_t i = 0; i < n && fits; i++) {
    uint64_t k;
    memcpy(&k, &body[i], 8);
    auto it = std::lower_bound(keys.begin(), keys.end(), k);
    if (it != keys.end() && *it == k) continue;
    if (keys.size() == SN_NARROW_MAX) fits = false;
    else keys.insert(it, k);
  }
  memset(dict, 0, SN_NARROW_MAX * 8);
  if (!fits) { *ndict = -1; return; }
  if (!keys.empty()) memcpy(dict, keys.data(), keys.size() * 8);
  *ndict = (int32_t)keys.size();
  for (int64_t i = 0; i < n; i++) {
    uint64_t k;
    memcpy(&k, &body[i], 8);
    codes[i] = (uint8_t)(std::lower_bound(keys.begin(), keys.end(), k) -
                         keys.begin());
  }
}

/* cheap host pre-filter where the put path holds the values: does a prefix
 * of the column already carry more than 256 distinct patterns?  Then the
 * device attempt (and the sidecar allocation) is skipped — l_extendedprice
 * never allocates.  The device result decides for everything that passes. */
static bool narrow_prefix_fits(const uint8_t *vals, int64_t n) {
  const int64_t np = std::min<int64_t>(n, 4096);
  uint64_t set[1024];
  bool zero_seen = false;              /* 0 marks an empty slot */
  memset(set, 0, sizeof(set));
  int distinct = 0;
  for (int64_t i = 0; i < np; i++) {
    const uint64_t k = (uint64_t)rd_i64(vals + i * 8);
    if (k == 0) { distinct += !zero_seen; zero_seen = true; continue; }
    uint32_t h = (uint32_t)mix64h(k) & 1023u;
    while (set[h] != 0 && set[h] != k) h = (h + 1) & 1023u;
    if (set[h] == k) continue;
    set[h] = k;
    if (++distinct > SN_NARROW_MAX) return false;
  }
  return distinct <= SN_NARROW_MAX;
}

static size_t narrow_block_bytes(const Batch &b) {
  return (size_t)SN_NARROW_MAX * 8 + (size_t)b.num_rows;
}

static void narrow_drop(sn_engine *e, Batch &b, int c) {
  Batch::Narrow &nw = b.narrow[c];
  if (nw.block) e->arena.release(nw.block, narrow_block_bytes(b));
  nw = Batch::Narrow();
}

/* (re)build column c's sidecar from its device body, async on the engine
 * stream behind whatever wrote the body; allocation or launch failure just
 * leaves the column un-narrowed */
static void narrow_launch(sn_engine *e, const Table *t, Batch &b, int c) {
  if (!e->narrow || !e->has_gpu || b.num_rows <= 0) return;
  const size_t nc = t->schema.size();
  if (!b.narrow_nd_dev)
    b.narrow_nd_dev = (int32_t *)e->arena.alloc(nc * 4);
  Batch::Narrow &nw = b.narrow[c];
  if (!nw.block) nw.block = e->arena.alloc(narrow_block_bytes(b));
  if (!b.narrow_nd_dev || !nw.block) { narrow_drop(e, b, c); return; }
  const double *body = (const double *)((const uint8_t *)b.col_dev[c] +
                                        b.cols[c].body_off);
  if (sn_launch_f64_narrow(body, b.num_rows, (unsigned char *)nw.codes(),
                           (double *)nw.block, b.narrow_nd_dev + c,
                           e->stream) != 0) {
    narrow_drop(e, b, c);
    return;
  }
  nw.ndict = 0;
  nw.pending = true;
  b.narrow_pending = true;
}

static bool narrow_eligible(const Table *t, const Batch &b, int c) {
  return t->schema[c].dtype == SN_TYPE_DOUBLE &&
         b.cols[c].type_id == SN_ENC_UNCOMPRESSED &&
         b.cols[c].num_null_words == 0;
}

/* ---- one of each: batch sizing, bounds sizing, dictionary interning ---- */

static void batch_init(Batch &b, int nc, int64_t uuid, int32_t bucket,
                       int32_t rows) {
  b.uuid = uuid;
  b.bucket = bucket;
  b.num_rows = rows;
  b.cols.resize(nc);
  b.col_dev.resize(nc);
  b.nullpfx_dev.resize(nc, nullptr);
  b.patch_dev.resize(nc);
  b.patch_host.resize(nc);
  b.had_patches.assign(nc, 0);
  b.rle_ends_dev.resize(nc, nullptr);
  b.rle_vals_dev.resize(nc, nullptr);
  b.rle_n.resize(nc, 0);
  b.dictmap_cache.resize(nc);
  b.narrow.resize(nc);
  b.is_raw.assign(nc, 0);
}

/* size the stats vectors with every column unbounded and null-free; whoever
 * knows a column's bounds fills them in and clears bounds_null[c] */
static void alloc_bounds(Batch &b, int nc) {
  b.lo_d.resize(nc); b.hi_d.resize(nc);
  b.lo_i.resize(nc); b.hi_i.resize(nc);
  b.null_count.assign(nc, 0);
  b.bounds_null.assign(nc, 1);
}

/* id of s in column c's table-global dictionary, appended when new; the
 * caller holds t->mu */
static int32_t intern(Table *t, int c, const std::string &s) {
  auto it = t->gdict_idx[c].find(s);
  if (it != t->gdict_idx[c].end()) return it->second;
  const int32_t gid = (int32_t)t->gdict[c].size();
  t->gdict[c].push_back(s);
  t->gdict_idx[c].emplace(s, gid);
  if ((int32_t)s.size() > t->gdict_maxlen[c])
    t->gdict_maxlen[c] = (int32_t)s.size();
  return gid;
}

static void intern_batch_dicts(Table *t, Batch &b) {
  for (int c = 0; c < (int)t->schema.size(); c++) {
    if (t->schema[c].dtype != SN_TYPE_STRING || b.cols[c].dict.empty())
      continue;
    auto &l2g = b.cols[c].local2global;
    l2g.reserve(b.cols[c].dict.size());
    for (auto &s : b.cols[c].dict) l2g.push_back(intern(t, c, s));
  }
}

/* ---- batch mutation processing (shared by sn_batch_put and
 * sn_batch_mutate — the reference writes delete masks and delta blobs to
 * region entries of an EXISTING batch after UPDATE/DELETE statements;
 * the ColumnBatchIterator hands the current state per scan) ---- */

/* delete mask -> bitmap (ColumnDeleteDecoder.scala:24-55 semantics); the mask
 * is cumulative, so it REPLACES any previous one.  A mask that does not parse
 * leaves the batch as it was. */
static int32_t apply_delete_mask(sn_engine *e, Batch &b,
                                 const sn_buf *delete_mask) {
  const uint8_t *pos = nullptr;
  int32_t n = 0;
  if (delete_mask && delete_mask->data &&
      parse_delete_mask((const uint8_t *)delete_mask->data, delete_mask->len,
                        &pos, &n) != SN_OK)
    return fail(SN_ERR_BADFORMAT, delete_mask->len < 12
                    ? "delete mask shorter than its header" : "bad delete mask");
  b.has_deletes = n > 0;
  b.del_bm_dev = nullptr;
  if (n > 0) {
    std::vector<uint64_t> bm(((size_t)b.num_rows + 63) / 64, 0);
    for (int32_t i = 0; i < n; i++) {
      int32_t p = rd_i32(pos + (int64_t)i * 4);
      if (p >= 0 && p < b.num_rows) bm[p >> 6] |= 1ull << (p & 63);
    }
    b.del_bm_dev = (const uint64_t *)up(e, bm.data(), bm.size() * 8);
  }
  return SN_OK;
}

/* per column: (delta1, delta2), empty where the caller passed none */
typedef std::vector<std::pair<DeltaRows, DeltaRows>> ColDeltas;

/* decode every delta blob before anything is applied: this touches neither
 * the batch nor the table, so a corrupt blob changes nothing */
static int32_t decode_deltas(const Table *t, const sn_buf *deltas,
                             ColDeltas *out) {
  const int nc = (int)t->schema.size();
  out->resize(deltas ? nc : 0);
  for (int c = 0; c < (int)out->size(); c++) {
    for (int j = 1; j >= 0; j--) {
      const sn_buf &d = deltas[c * 2 + j];
      if (!d.data) continue;
      int rc = decode_delta((const uint8_t *)d.data, d.len, t->schema[c].dtype,
                            j ? &(*out)[c].second : &(*out)[c].first);
      if (rc != SN_OK) return fail(rc, "delta%d decode col %d", j + 1, c);
    }
  }
  return SN_OK;
}

/* delta2 then delta1 (delta1 overrides, UpdatedColumnDecoder.scala:69-115)
 * into one patch sorted by row; string values are interned here and travel
 * as table-global ids.  The caller holds t->mu. */
static void merge_patch(Table *t, int c, const DeltaRows &d1,
                        const DeltaRows &d2, Patch *P) {
  std::map<int32_t, std::pair<double, uint8_t>> merged;
  for (const DeltaRows *d : { &d2, &d1 })
    for (size_t i = 0; i < d->pos.size(); i++) {
      double v = d->val[i];
      if (d->sidx[i] >= 0) v = (double)intern(t, c, d->strs[d->sidx[i]]);
      merged[d->pos[i]] = { v, d->isnull[i] };
    }
  for (auto &kv : merged) {
    P->pos.push_back(kv.first);
    P->val.push_back(kv.second.first);
    P->isnull.push_back(kv.second.second);
  }
}

/* device form of a patch: row bitmap, positions, values, null bitmap over
 * patch entries (absent when no entry writes NULL) */
static Batch::PatchDev upload_patch(sn_engine *e, const Batch &b,
                                    const Patch &P) {
  std::vector<uint64_t> bm(((size_t)b.num_rows + 63) / 64, 0);
  for (int32_t p : P.pos)
    if (p >= 0 && p < b.num_rows) bm[p >> 6] |= 1ull << (p & 63);
  std::vector<uint64_t> nbm((P.pos.size() + 63) / 64, 0);
  bool any_null = false;
  for (size_t i = 0; i < P.isnull.size(); i++)
    if (P.isnull[i]) { nbm[i >> 6] |= 1ull << (i & 63); any_null = true; }
  Batch::PatchDev pd;
  pd.n = (int32_t)P.pos.size();
  pd.bm = (const uint64_t *)up(e, bm.data(), bm.size() * 8);
  pd.pos = (const int32_t *)up(e, P.pos.data(), P.pos.size() * 4);
  pd.val = (const double *)up(e, P.val.data(), P.val.size() * 8);
  pd.nullbm = any_null ? (const uint64_t *)up(e, nbm.data(), nbm.size() * 8)
                       : nullptr;
  return pd;
}

/* write value-only patches straight into the device body when the base
 * column is null-free fixed-width: the batch then scans clean (query-compiled
 * kernels apply).  Scan results are identical by construction — read_general
 * would hand back exactly these values; the host blob (sn_table_get_blob)
 * keeps the base bytes. */
static void materialize_patch(sn_engine *e, const Table *t, Batch &b, int c) {
  Batch::PatchDev &pd = b.patch_dev[c];
  const std::vector<uint8_t> &isnull = b.patch_host[c].isnull;
  const bool any_null = std::find(isnull.begin(), isnull.end(), 1) != isnull.end();
  int k, width;
  if (!e->has_gpu || any_null || b.cols[c].num_null_words != 0 ||
      b.cols[c].type_id != SN_ENC_UNCOMPRESSED ||
      !fixed_type(t->schema[c].dtype, &k, &width) || width < 2)
    return;
  void *body = (uint8_t *)(uintptr_t)b.col_dev[c] + b.cols[c].body_off;
  if (sn_launch_patch_apply(body, pd.pos, pd.val, pd.n, k, e->stream) != 0)
    return;
  pd = Batch::PatchDev();
  b.patch_host[c] = Patch();
  /* the body changed under the sidecar: rebuild it behind the patch kernel
   * (an overflow drops it at the next query) */
  if (k == SN_K_F64 && b.narrow[c].block) narrow_launch(e, t, b, c);
}

/* decoded update deltas -> host-merged patches.  Delta blobs are cumulative
 * for their batch (the encoder merges upward), so the decoded set REPLACES
 * any previous patch state; values already materialized into the body are
 * simply rewritten with the same bytes.  The caller holds t->mu. */
static void apply_deltas(sn_engine *e, Table *t, Batch &b, const sn_buf *deltas,
                         const ColDeltas &dec) {
  for (int c = 0; c < (int)dec.size(); c++) {
    if (!deltas[c * 2].data && !deltas[c * 2 + 1].data) continue;
    /* deltas may arrive with a positive row count too (the reference
     * signals them via the stats row's negative batchCount); either way
     * the batch must never stats-skip — base bounds don't cover patches */
    b.has_deltas = true;
    Patch &P = b.patch_host[c];
    P = Patch();                          /* cumulative: replace prior state */
    b.patch_dev[c] = Batch::PatchDev();
    merge_patch(t, c, dec[c].first, dec[c].second, &P);
    if (P.pos.empty()) continue;
    b.had_patches[c] = 1;
    b.patch_dev[c] = upload_patch(e, b, P);
    materialize_patch(e, t, b, c);
  }
}

/* stats row parse (UnsafeRow: [null words][3*ncols+1 x 8B slots],
 * ColumnStatsSchema, ColumnEncoding.scala:1015-1036); a row too short for
 * the schema is ignored */
static void apply_stats(Table *t, Batch &b, const sn_buf *stats) {
  if (!stats || !stats->data) return;
  const int nc = (int)t->schema.size();
  const int32_t num_fields = nc * 3 + 1;
  BlobReader r((const uint8_t *)stats->data, stats->len);
  const uint8_t *bits = r.array((num_fields + 63) >> 6, 8);
  const uint8_t *slots = r.array(num_fields, 8);
  if (!r.ok) return;
  auto bit = [&](int f) {
    return (rd_i64(bits + ((f >> 6) << 3)) >> (f & 63)) & 1;
  };
  alloc_bounds(b, nc);
  for (int c = 0; c < nc; c++) {
    const uint8_t *lo = slots + (int64_t)(1 + c * 3) * 8, *hi = lo + 8;
    const int f_lo = 1 + c * 3, f_hi = 2 + c * 3, f_nc = 3 + c * 3;
    b.bounds_null[c] = bit(f_lo) || bit(f_hi);
    b.null_count[c] = bit(f_nc) ? 0 : rd_i32(hi + 8);
    if (b.bounds_null[c]) continue;
    switch (t->schema[c].dtype) {
      case SN_TYPE_DOUBLE: b.lo_d[c] = rd_f64(lo); b.hi_d[c] = rd_f64(hi); break;
      case SN_TYPE_FLOAT:  b.lo_d[c] = rd_f32(lo); b.hi_d[c] = rd_f32(hi); break;
      case SN_TYPE_INT64:  b.lo_i[c] = rd_i64(lo); b.hi_i[c] = rd_i64(hi); break;
      case SN_TYPE_STRING: b.bounds_null[c] = 1; break;
      default:             b.lo_i[c] = rd_i32(lo); b.hi_i[c] = rd_i32(hi);
    }
  }
  b.stats_valid = true;
}

/* ---- the stages of one encoded column's put, in the order
 * process_encoded_col runs them ---- */

/* the bytes that get stored for a column: the caller's, their decompressed
 * form, or a re-encoding synthesized here */
struct ColBlob {
  const uint8_t *blob = nullptr;
  int64_t len = 0;
  std::vector<uint8_t> decomp, synth;   /* own the bytes that are not the caller's */
  bool lz4 = false;                     /* the caller's bytes are an LZ4 wrapper */
};

/* stage 1: strip the compression wrapper, if any */
static int32_t unwrap_blob(const sn_buf &column, ColBlob *cb) {
  cb->blob = (const uint8_t *)column.data;
  cb->len = column.len;
  int dec = maybe_decompress(cb->blob, cb->len, &cb->decomp);
  if (dec < 0) return dec;
  if (dec == 1) {
    cb->lz4 = rd_i32(cb->blob) == -1;
    cb->blob = cb->decomp.data();
    cb->len = (int64_t)cb->decomp.size();
  }
  return SN_OK;
}

/* stage 3: what a kernel would index by row count must be there.  A corrupt
 * dictionary index would walk the kernel off the end of the local->global
 * map; a short fixed-width body would have it read a neighbouring block. */
static int32_t check_col_body(const ColBlob &cb, const ColMeta &m,
                              sn_type_t dtype, int32_t rows, int c) {
  if (dtype == SN_TYPE_STRING && !m.dict.empty()) {
    int64_t bad;
    if (check_dict_indices(cb.blob, cb.len, m, rows, (int32_t)m.dict.size(),
                           &bad) == SN_OK)
      return SN_OK;
    if (bad < 0)
      return fail(SN_ERR_BADFORMAT, "dictionary index array truncated col %d", c);
    return fail(SN_ERR_BADFORMAT,
                "dictionary index %d out of range [0,%d] at row %lld col %d",
                dict_index(cb.blob + m.body_off, dict_index_width(m.type_id), bad),
                (int)m.dict.size(), (long long)bad, c);
  }
  const int width = sn_type_width(dtype);
  if (m.type_id == SN_ENC_UNCOMPRESSED && width > 0 &&
      check_fixed_body(cb.blob, cb.len, m, rows, width) != SN_OK)
    return fail(SN_ERR_BADFORMAT,
                "column %d body shorter than its %d non-null rows", c,
                (int)(rows - count_nulls(cb.blob, m)));
  return SN_OK;
}

/* stage 4: encodings no kernel reads are re-encoded at put, the same idea as
 * decompress-on-put: var-width strings become BIG_DICTIONARY (global
 * interning, premultiplied maps, pushdown equality and group keys then apply
 * wholesale), int dictionaries become a plain body (the plain I32/I64 scan
 * path, JIT-eligible).  The synthesized blob replaces cb's and is re-parsed. */
static int32_t reencode_col(ColBlob *cb, ColMeta *m, sn_type_t dtype,
                            int32_t rows, int c) {
  const bool dict_enc = m->type_id == SN_ENC_DICTIONARY ||
                        m->type_id == SN_ENC_BIG_DICTIONARY;
  const char *what;
  if (dtype == SN_TYPE_STRING && m->type_id == SN_ENC_UNCOMPRESSED) {
    what = "transcoded string col %d";
    if (transcode_strings(cb->blob, cb->len, *m, rows, &cb->synth) != SN_OK)
      return fail(SN_ERR_BADFORMAT, "string body truncated col %d", c);
  } else if (dict_enc && dtype != SN_TYPE_STRING) {
    what = "materialized dict col %d";
    int64_t bad;
    if (materialize_int_dict(cb->blob, cb->len, *m, dtype, rows, &cb->synth,
                             &bad) != SN_OK) {
      if (bad < 0)
        return fail(SN_ERR_BADFORMAT,
                    "dictionary index array truncated col %d", c);
      return fail(SN_ERR_BADFORMAT,
                  "dictionary index %d out of range [0,%d] col %d",
                  dict_index(cb->blob + m->body_off,
                             dict_index_width(m->type_id), bad), m->dict_n, c);
    }
  } else {
    return SN_OK;
  }
  cb->blob = cb->synth.data();
  cb->len = (int64_t)cb->synth.size();
  *m = ColMeta();
  int rc = parse_blob(cb->blob, cb->len, dtype, m);
  return rc == SN_OK ? SN_OK : fail(rc, what, c);
}

/* f1 compressed-upload: an LZ4-wrapped blob ships its COMPRESSED bytes over
 * PCIe (the host's decompressed copy served only parse and validation) and
 * decodes wave-cooperatively on device into dst[0, len) — byte-identical
 * output, ~2-4x less bus traffic per blob.  1 = decoded, 0 = not done (the
 * caller copies the host bytes instead), negative = the device found the
 * stream malformed. */
static int32_t lz4_decode_on_device(sn_engine *e, const sn_buf &column,
                                    char *dst, int64_t len, int c) {
  const int64_t clen = column.len - 8;
  /* the engine stream + error word are shared: one decode at a time
   * (concurrent puts overlap their host work; device decodes queue) */
  std::lock_guard<std::mutex> glz(e->lz4_mu);
  void *cdev = e->arena.alloc((size_t)clen);
  if (!e->lz4_err_dev) e->lz4_err_dev = (int32_t *)e->arena.alloc(64);
  int32_t done = 0;
  if (cdev && e->lz4_err_dev &&
      hipMemcpy(cdev, (const uint8_t *)column.data + 8, (size_t)clen,
                hipMemcpyHostToDevice) == hipSuccess &&
      hipMemsetAsync(e->lz4_err_dev, 0, 4, e->stream) == hipSuccess &&
      sn_launch_lz4_decompress(cdev, clen, dst, len, e->lz4_err_dev,
                               e->stream) == 0 &&
      hipStreamSynchronize(e->stream) == hipSuccess) {
    int32_t derr = -1;
    (void)hipMemcpy(&derr, e->lz4_err_dev, 4, hipMemcpyDeviceToHost);
    if (derr != 0)
      return fail(SN_ERR_BADFORMAT, "device LZ4 decode failed (%d) col %d",
                  derr, c);
    done = 1;
  }
  if (cdev) e->arena.release(cdev, (size_t)clen);
  return done;
}

/* stage 5: the blob into the arena, placed so the BODY is 16-byte aligned
 * (the scan kernel issues 16 B/lane vector loads on the body; the 8-byte
 * blob header would otherwise leave it 8-aligned).  Host-only engines keep
 * the bytes for sn_table_get_blob: one host_blobs entry per column, in
 * column order. */
static int32_t upload_blob(sn_engine *e, Batch &b, int c, const ColBlob &cb,
                           const sn_buf &column) {
  const int64_t pad = (16 - (b.cols[c].body_off & 15)) & 15;
  char *base = (char *)e->arena.alloc((size_t)cb.len + 16);
  if (!base) return fail(SN_ERR_NOMEM, "HBM upload failed");
  char *dst = base + pad;
  if (e->arena.device < 0) {
    memcpy(dst, cb.blob, (size_t)cb.len);
    b.host_blobs.emplace_back(cb.blob, cb.blob + cb.len);
  } else {
    int32_t dev = cb.lz4 ? lz4_decode_on_device(e, column, dst, cb.len, c) : 0;
    if (dev < 0) return dev;
    if (dev == 0 && h2d_copy(e, dst, cb.blob, (size_t)cb.len) != hipSuccess)
      return fail(SN_ERR_NOMEM, "HBM upload failed");
  }
  b.col_dev[c] = dst;
  return SN_OK;
}

/* stage 6: RLE aux — (cumulative end, value-as-f64) per run, extracted on
 * host (the decoder accumulates run lengths sequentially, which has no
 * data-parallel analogue) */
static int32_t build_rle_aux(sn_engine *e, const Table *t, Batch &b, int c,
                             const ColBlob &cb) {
  if (b.cols[c].type_id != SN_ENC_RUNLENGTH) return SN_OK;
  const sn_type_t dt = t->schema[c].dtype;
  int kind, w;
  if (!fixed_type(dt, &kind, &w) ||
      (kind != SN_K_I16 && kind != SN_K_I32 && kind != SN_K_I64))
    return fail(SN_ERR_UNSUPPORTED, "RLE col %d dtype %d on GPU path", c, dt);
  std::vector<int32_t> ends;
  std::vector<double> vals;
  extract_rle_runs(cb.blob, cb.len, b.cols[c], w, kind == SN_K_I64, &ends, &vals);
  if (!ends.empty()) {
    b.rle_ends_dev[c] = (const int32_t *)up(e, ends.data(), ends.size() * 4);
    b.rle_vals_dev[c] = (const double *)up(e, vals.data(), vals.size() * 8);
    b.rle_n[c] = (int32_t)ends.size();
  }
  return SN_OK;
}

/* stage 7: nulls in words [0, w) for each null word w */
static void build_null_prefix(sn_engine *e, Batch &b, int c, const ColBlob &cb) {
  const ColMeta &m = b.cols[c];
  if (!m.num_null_words) return;
  std::vector<uint32_t> pfx((size_t)m.num_null_words);
  uint32_t acc = 0;
  for (int w = 0; w < m.num_null_words; w++) {
    pfx[w] = acc;
    acc += (uint32_t)__builtin_popcountll(
        (unsigned long long)rd_i64(cb.blob + m.null_off + (int64_t)w * 8));
  }
  b.nullpfx_dev[c] = (const uint32_t *)up(e, pfx.data(), pfx.size() * 4);
}

/* one encoded column blob -> device-resident state — batch-local, no table
 * lock; shared by sn_batch_put and sn_batch_put_raw */
static int32_t process_encoded_col(sn_engine *e, Table *t, Batch &b, int c,
                                   const sn_buf &column) {
  const sn_type_t dt = t->schema[c].dtype;
  ColMeta &m = b.cols[c];
  ColBlob cb;
  int32_t rc = unwrap_blob(column, &cb);
  if (rc != SN_OK) return rc;
  rc = parse_blob(cb.blob, cb.len, dt, &m);
  if (rc != SN_OK) return fail(rc, "column %d blob parse failed", c);
  if ((rc = check_col_body(cb, m, dt, b.num_rows, c)) != SN_OK) return rc;
  if ((rc = reencode_col(&cb, &m, dt, b.num_rows, c)) != SN_OK) return rc;
  if ((rc = upload_blob(e, b, c, cb, column)) != SN_OK) return rc;
  if ((rc = build_rle_aux(e, t, b, c, cb)) != SN_OK) return rc;
  build_null_prefix(e, b, c, cb);
  /* stage 8: low-cardinality doubles get a code sidecar from the uploaded
   * (or device-decoded) body, behind whatever wrote it on the stream */
  if (narrow_eligible(t, b, c) &&
      narrow_prefix_fits(cb.blob + m.body_off, b.num_rows))
    narrow_launch(e, t, b, c);
  return SN_OK;
}

/* host-only engines: scalar bounds of one raw column, so stats-skip still
 * works without the device min/max */
static void host_bounds(Batch &b, int nc, int c, sn_type_t dt, int w,
                        const uint8_t *vals) {
  if (b.bounds_null.empty()) alloc_bounds(b, nc);
  if (dt == SN_TYPE_DOUBLE || dt == SN_TYPE_FLOAT) {
    double mn = 0, mx = 0;
    for (int32_t i = 0; i < b.num_rows; i++) {
      double v = w == 8 ? rd_f64(vals + (int64_t)i * 8)
                        : rd_f32(vals + (int64_t)i * 4);
      if (i == 0 || v < mn) mn = v;
      if (i == 0 || v > mx) mx = v;
    }
    b.lo_d[c] = mn; b.hi_d[c] = mx;
  } else {
    int64_t mn = 0, mx = 0;
    for (int32_t i = 0; i < b.num_rows; i++) {
      int64_t v = w == 8 ? rd_i64(vals + (int64_t)i * 8)
                : w == 4 ? rd_i32(vals + (int64_t)i * 4)
                         : rd_i16(vals + (int64_t)i * 2);
      if (i == 0 || v < mn) mn = v;
      if (i == 0 || v > mx) mx = v;
    }
    b.lo_i[c] = mn; b.hi_i[c] = mx;
  }
  b.bounds_null[c] = 0;
  b.stats_valid = true;
}

/* one raw (non-null, fixed-width) value array -> device blob
 * [typeId=0][nullBytes=0][body]: header at base+8 (8-aligned), body at
 * base+16 (16-aligned — arena blocks are 256-aligned); blob pointer =
 * base+8, body_off = 8.  On device the bounds come from an async min/max into
 * sd (the caller zeroed it on the same stream); host-only from host_bounds. */
static int32_t put_raw_col(sn_engine *e, Table *t, Batch &b, int c,
                           const sn_buf &raw, unsigned long long *sd) {
  const int nc = (int)t->schema.size();
  const sn_type_t dt = t->schema[c].dtype;
  int kind, w;
  if (!fixed_type(dt, &kind, &w) || w < 2)
    return fail(SN_ERR_UNSUPPORTED, "raw column %d dtype %d", c, (int)dt);
  if (raw.len != (int64_t)b.num_rows * w)
    return fail(SN_ERR_BADARG, "raw column %d length", c);
  char *base = (char *)e->arena.alloc((size_t)raw.len + 16);
  if (!base) return fail(SN_ERR_NOMEM, "HBM upload failed");
  char *body = base + 16;
  const int32_t hdr[2] = { SN_ENC_UNCOMPRESSED, 0 };
  b.cols[c].type_id = SN_ENC_UNCOMPRESSED;
  b.cols[c].body_off = 8;
  b.col_dev[c] = base + 8;
  if (e->arena.device < 0) {
    memcpy(base + 8, hdr, 8);
    memcpy(body, raw.data, (size_t)raw.len);
    b.host_blobs.emplace_back((const uint8_t *)base + 8,
                              (const uint8_t *)body + raw.len);
    host_bounds(b, nc, c, dt, w, (const uint8_t *)raw.data);
    return SN_OK;
  }
  if (hipMemcpy(base + 8, hdr, 8, hipMemcpyHostToDevice) != hipSuccess ||
      h2d_copy(e, body, raw.data, (size_t)raw.len) != hipSuccess)
    return fail(SN_ERR_NOMEM, "HBM upload failed");
  if (sn_launch_col_minmax(body, b.num_rows, kind, sd + c, sd + nc + c,
                           e->stream) != 0)
    return fail(SN_ERR_GENERIC, "stats kernel");
  b.is_raw[c] = 1;
  if (dt == SN_TYPE_DOUBLE &&
      narrow_prefix_fits((const uint8_t *)raw.data, b.num_rows))
    narrow_launch(e, t, b, c);
  return SN_OK;
}

/* f2 fast ingest: fixed-width NON-NULL columns arrive as RAW value arrays
 * (the Uncompressed encoder for numerics is the identity), other columns as
 * encoded blobs.  Bounds for the raw columns compute ON DEVICE (async
 * min/max on the engine stream — ColumnEncoder's lowerLong/upperLong
 * tracking, ColumnEncoding.scala:188-251, moved to the GPU); queries force
 * the pending sync.  This is the ColumnBatchCreator rollover with encode +
 * stats offloaded — ingest threads only touch the bytes once. */
extern "C" int32_t sn_batch_put_raw(sn_engine *e, int32_t table,
                                    int64_t uuid, int32_t bucket_id,
                                    int32_t num_rows, const sn_buf *raw,
                                    const sn_buf *encoded) {
  Table *t = get_table(e, table);
  if (!t || !raw || !encoded || num_rows <= 0)
    return fail(SN_ERR_BADARG, "bad raw batch args");
  if (e->cfg.shard_count > 1 &&
      (bucket_id % e->cfg.shard_count) != e->cfg.shard_rank)
    return SN_OK;
  const int nc = (int)t->schema.size();
  Batch b;
  batch_init(b, nc, uuid, bucket_id, num_rows);

  /* both memsets go on the stream before any column's min/max launch */
  unsigned long long *sd = nullptr;
  if (e->has_gpu) {
    sd = (unsigned long long *)e->arena.alloc((size_t)nc * 16);
    if (!sd) return fail(SN_ERR_NOMEM, "stats scratch");
    if (hipMemsetAsync(sd, 0xff, (size_t)nc * 8, e->stream) != hipSuccess ||
        hipMemsetAsync(sd + nc, 0, (size_t)nc * 8, e->stream) != hipSuccess)
      return fail(SN_ERR_GENERIC, "stats scratch init");
  }
  bool any_raw = false;
  for (int c = 0; c < nc; c++) {
    if (!raw[c].data && !encoded[c].data)
      return fail(SN_ERR_BADARG, "column %d has neither raw nor encoded", c);
    int32_t rc = raw[c].data ? put_raw_col(e, t, b, c, raw[c], sd)
                             : process_encoded_col(e, t, b, c, encoded[c]);
    if (rc != SN_OK) return rc;
    any_raw |= b.is_raw[c] != 0;
  }
  if (any_raw) {
    b.stats_dev = sd;
    b.stats_pending = true;
  } else if (sd) {
    e->arena.release(sd, (size_t)nc * 16);
  }

  std::lock_guard<std::mutex> g(t->mu);
  intern_batch_dicts(t, b);
  t->total_rows += b.num_rows;
  t->batches.push_back(std::move(b));
  return SN_OK;
}

/* resolve device-computed bounds for raw-ingested batches (one stream sync
 * for ALL pending batches; called under t->mu before any bounds are read) */
static void sync_pending_stats(sn_engine *e, Table *t) {
  bool any = false;
  for (auto &b : t->batches) any |= b.stats_pending | b.narrow_pending;
  if (!any) return;
  (void)hipStreamSynchronize(e->stream);
  const int nc = (int)t->schema.size();
  /* pending code sidecars: read the device entry counts; a column that
   * overflowed (or whose readback failed) gives its block back */
  std::vector<int32_t> nd((size_t)nc);
  for (auto &b : t->batches) {
    if (!b.narrow_pending) continue;
    b.narrow_pending = false;
    const bool got = hipMemcpy(nd.data(), b.narrow_nd_dev, (size_t)nc * 4,
                               hipMemcpyDeviceToHost) == hipSuccess;
    for (int c = 0; c < nc; c++) {
      Batch::Narrow &nw = b.narrow[c];
      if (!nw.pending) continue;
      nw.pending = false;
      if (got && nd[c] > 0 && nd[c] <= SN_NARROW_MAX) nw.ndict = nd[c];
      else narrow_drop(e, b, c);
    }
  }
  std::vector<unsigned long long> h((size_t)nc * 2);
  for (auto &b : t->batches) {
    if (!b.stats_pending) continue;
    b.stats_pending = false;
    if (hipMemcpy(h.data(), b.stats_dev, (size_t)nc * 16,
                  hipMemcpyDeviceToHost) != hipSuccess)
      continue;                         /* bounds stay absent: conservative */
    alloc_bounds(b, nc);
    for (int c = 0; c < nc; c++) {
      if (!b.is_raw[c]) continue;
      sn_type_t dt = t->schema[c].dtype;
      if (dt == SN_TYPE_DOUBLE || dt == SN_TYPE_FLOAT) {
        b.lo_d[c] = sn_ord_f64_h(h[c]);
        b.hi_d[c] = sn_ord_f64_h(h[nc + c]);
      } else {
        b.lo_i[c] = (int64_t)(h[c] ^ 0x8000000000000000ull);
        b.hi_i[c] = (int64_t)(h[nc + c] ^ 0x8000000000000000ull);
      }
      b.bounds_null[c] = 0;
    }
    b.stats_valid = true;
    e->arena.release((void *)b.stats_dev, (size_t)nc * 16);
    b.stats_dev = nullptr;
  }
}

extern "C" int32_t sn_batch_put(sn_engine *e, int32_t table,
                                int64_t uuid, int32_t bucket_id, int32_t num_rows,
                                const sn_buf *columns, const sn_buf *stats,
                                const sn_buf *delete_mask, const sn_buf *deltas) {
  Table *t = get_table(e, table);
  if (!t || !columns || num_rows == 0) return fail(SN_ERR_BADARG, "bad batch args");
  /* shard filter: batches whose bucket belongs to another rank are ignored */
  if (e->cfg.shard_count > 1 &&
      (bucket_id % e->cfg.shard_count) != e->cfg.shard_rank)
    return SN_OK;

  const int nc = (int)t->schema.size();
  Batch b;
  batch_init(b, nc, uuid, bucket_id, num_rows < 0 ? -num_rows : num_rows);
  b.has_deltas = num_rows < 0;

  /* Phase 1 — NO table lock: decompress, parse, validate, materialize and
   * upload are all batch-local (the arena has its own mutex), so concurrent
   * puts from many ingest threads overlap their heavy work.  Only the
   * global-dictionary interning, the delta merge (which interns) and the
   * batches-vector append need t->mu (phase 2 below). */
  int32_t rc = SN_OK;
  for (int c = 0; c < nc && rc == SN_OK; c++)
    rc = process_encoded_col(e, t, b, c, columns[c]);
  if (rc != SN_OK) return rc;
  if ((rc = apply_delete_mask(e, b, delete_mask)) != SN_OK) return rc;
  apply_stats(t, b, stats);

  /* Phase 2 — under t->mu: global-dictionary interning, delta decode and
   * merge (interns new entries) and the append */
  std::lock_guard<std::mutex> g(t->mu);
  ColDeltas dec;
  if ((rc = decode_deltas(t, deltas, &dec)) != SN_OK) return rc;
  intern_batch_dicts(t, b);
  apply_deltas(e, t, b, deltas, dec);
  t->total_rows += b.num_rows;
  t->batches.push_back(std::move(b));
  return SN_OK;
}

/* Attach the CURRENT mutation state to an existing batch — the seam the
 * reference exercises when UPDATE/DELETE statements write delta blobs and
 * delete masks to the region entries of a batch that already exists
 * (ColumnDelta.scala:300-301 key addressing; ColumnBatchIterator then hands
 * the latest buffers to every scan).  delete_mask and the delta pairs are
 * CUMULATIVE (the reference merges delta chains upward), so they replace
 * any previous state; stats, when given, replace the stats row (the
 * reference rewrites it with a negative batchCount). */
extern "C" int32_t sn_batch_mutate(sn_engine *e, int32_t table, int64_t uuid,
                                   int32_t bucket_id,
                                   const sn_buf *delete_mask,
                                   const sn_buf *deltas,
                                   const sn_buf *stats) {
  Table *t = get_table(e, table);
  if (!t) return fail(SN_ERR_BADARG, "bad table");
  if (e->cfg.shard_count > 1 &&
      (bucket_id % e->cfg.shard_count) != e->cfg.shard_rank)
    return SN_OK;
  std::lock_guard<std::mutex> g(t->mu);
  Batch *b = nullptr;
  for (auto &bb : t->batches)
    if (bb.uuid == uuid && bb.bucket == bucket_id) { b = &bb; break; }
  if (!b) return fail(SN_ERR_BADARG, "no batch uuid=%lld bucket=%d",
                      (long long)uuid, bucket_id);
  /* decode before the first change, so a corrupt blob leaves the batch alone */
  ColDeltas dec;
  int32_t rc = decode_deltas(t, deltas, &dec);
  if (rc != SN_OK) return rc;
  if (delete_mask && (rc = apply_delete_mask(e, *b, delete_mask)) != SN_OK)
    return rc;
  apply_deltas(e, t, *b, deltas, dec);
  if (b->stats_pending) {
    /* caller-provided (or absent) stats supersede the device-computed ones */
    b->stats_pending = false;
    if (b->stats_dev) {
      e->arena.release((void *)b->stats_dev,
                       t->schema.size() * 16);
      b->stats_dev = nullptr;
    }
  }
  if (stats) apply_stats(t, b[0], stats);
  else b->stats_valid = false;   /* old bounds no longer trustworthy */
  /* cached descriptor sets reference the old patch/delete device data */
  for (auto &dc : t->desc_caches) {
    e->arena.release((void *)dc.db_dev, dc.db_bytes);
    e->arena.release((void *)dc.tl_dev, dc.tl_bytes);
  }
  t->desc_caches.clear();
  return SN_OK;
}

struct TableInfoProbe { int32_t ncols; sn_type_t dtypes[64]; uint8_t nullable[64]; };
extern "C" int32_t sn_table_schema(sn_engine *e, int32_t table, TableInfoProbe *out) {
  Table *t = get_table(e, table);
  if (!t || !out) return SN_ERR_BADARG;
  out->ncols = (int32_t)t->schema.size();
  for (size_t i = 0; i < t->schema.size(); i++) {
    out->dtypes[i] = t->schema[i].dtype;
    out->nullable[i] = (uint8_t)t->schema[i].nullable;
  }
  return SN_OK;
}
extern "C" void sn_engine_shard(sn_engine *e, int32_t *rank, int32_t *count) {
  *rank = e ? e->cfg.shard_rank : 0;
  *count = e ? e->cfg.shard_count : 1;
}

extern "C" int64_t sn_table_num_batches(sn_engine *e, int32_t table) {
  Table *t = get_table(e, table);
  return t ? (int64_t)t->batches.size() : -1;
}
extern "C" int64_t sn_table_num_rows(sn_engine *e, int32_t table) {
  Table *t = get_table(e, table);
  return t ? t->total_rows : -1;
}
extern "C" int64_t sn_table_narrowed_batches(sn_engine *e, int32_t table,
                                             int32_t col) {
  Table *t = get_table(e, table);
  if (!t || col < 0 || col >= (int32_t)t->schema.size()) return -1;
  std::lock_guard<std::mutex> g(t->mu);
  if (e->has_gpu) sync_pending_stats(e, t);
  int64_t n = 0;
  for (auto &b : t->batches) n += b.narrow[col].ndict > 0;
  return n;
}

/* fetch back an engine-stored blob (tests / cross-validation) */
extern "C" int64_t sn_table_get_blob(sn_engine *e, int32_t table, int32_t batch,
                                     int32_t col, void *out, int64_t cap) {
  Table *t = get_table(e, table);
  if (!t || batch < 0 || batch >= (int32_t)t->batches.size()) return SN_ERR_BADARG;
  Batch &b = t->batches[batch];
  if (col < 0 || col >= (int32_t)b.cols.size()) return SN_ERR_BADARG;
  if (e->arena.device < 0) {
    auto &hb = b.host_blobs[col];
    if ((int64_t)hb.size() > cap) return SN_ERR_NOMEM;
    memcpy(out, hb.data(), hb.size());
    return (int64_t)hb.size();
  }
  return SN_ERR_UNSUPPORTED;
}

/* ================================================================== */
/* query plane                                                         */

/* decimal-query request threaded through the shared submit body */
struct DecReq {
  int32_t naggs;
  const sn_dec_agg *aggs;
};

struct sn_query {
  sn_engine *e = nullptr;
  Table *t = nullptr;
  sn_plan plan;
  int cslot_of_col[64];                 /* table col -> device col slot */
  std::vector<int32_t> used_cols;       /* cslot -> table col */
  int nslots = 0;
  int g1cap = 0, g2cap = 0;             /* per-group-col slot counts */
  int fact_slots = 1;                   /* composite dim_attr x fact_col:
                                           dense fact span (slot minor) */
  bool sparse = false;                  /* open-address hash-aggregate mode */
  bool pac = false;                     /* per-agg counts (nullable agg inputs) */
  bool mm = false;                      /* plan has MIN/MAX aggregates */
  /* compacted group keys + [n][na1] accumulator rows.  Raw arrays, NOT
   * vectors: resize() would zero-fill the ~24 MB 1M-group readback before
   * the copy overwrites it (measured ~1 ms/query of pure host overhead) */
  std::unique_ptr<long long[]> sparse_keys;
  std::unique_ptr<double[]> sparse_rows;
  size_t sparse_n = 0;
  std::vector<double> sparse_null_row;  /* NULL-key group accumulator */
  bool gint[2] = { false, false };      /* integer group key (stats-ranged) */
  int64_t gmin[2] = { 0, 0 };           /* integer key minimum (slot base) */
  int gnull1 = -1, gnull2 = -1;         /* null slot index per group col (-1: none) */
  /* grouped-mode device aggregate dedup: logical agg -> device sweep index
   * (-1 = COUNT(*), derived from the per-slot rowcount) */
  int agg_map[SN_MAX_AGGS];
  int dev_naggs = 0;
  Dim *join_dim = nullptr;          /* group-by-dim-attr key source */
  bool join_group = false;
  /* device buffers */
  double *dev_out = nullptr;
  size_t out_stride = 0;                /* 2*NA_t+1 of the launched template */
  int na_t = 0;                          /* template NAGGS actually launched */
  std::vector<double> host_out;
  int64_t rows_scanned = 0;             /* host metric: rows in unskipped batches */
  int64_t batches_seen = 0, batches_skipped = 0;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;  /* brackets the scan kernel */
  /* per-query arena blocks, recycled via the free list at destroy */
  std::vector<std::pair<void *, size_t>> owned;
  float kernel_ms = -1.0f;
  bool used_jit = false;                /* query-compiled kernel ran */
  int64_t late_cols = 0;                /* table columns it read late (bit c) */
  int direct = 0;                       /* the image-free keyless kernel ran */
  bool done = false;
  bool merged = false;
  std::vector<GroupOut> final_groups;
  /* exact DECIMAL query state (sn_query_submit_dec) */
  bool dec = false;
  int dec_ndev = 0;                      /* deduped device aggregates */
  int dec_map[SN_MAX_AGGS];              /* logical agg -> device agg (-1: COUNT(*)) */
  int dec_scale_of[SN_MAX_AGGS];         /* result scale per logical agg */
  unsigned long long *dec_out = nullptr; /* device [nslots][sn_dec_row_cells] */
  std::vector<sn_dec_val> dec_vals;      /* host [nslots][plan.naggs] */
  /* row-returning scan state (sn_scan_submit): the result stays on the
   * device, one dense typed array and one validity array per projection */
  bool select = false;
  int sel_nproj = 0;
  int32_t sel_cols[SN_SEL_MAX_PROJ];     /* table column or SN_PROJ_ROWID */
  int64_t sel_limit = 0;
  int64_t sel_total = 0;                 /* matching rows before the limit */
  int64_t sel_rows = 0;                  /* rows returned */
  int sel_width[SN_SEL_MAX_PROJ];        /* bytes per output element */
  void *sel_val[SN_SEL_MAX_PROJ];
  uint8_t *sel_valid[SN_SEL_MAX_PROJ];
  int sel_kernels = 0;                   /* kernels launched: 0, 2 or 3 */
  /* ordered scan (sn_scan_submit_ordered): the third interval is the whole
   * order stage, select to gather */
  bool ordered = false;
  int32_t ord_col = 0, ord_flags = 0;
  /* join scan (sn_scan_submit_join): SN_RJOIN_*, -1 without a join.  INNER
   * and LEFT_ANTI probe in pass 1; LEFT_OUTER only in pass 2's projection */
  int32_t rjoin = -1;
  float sel_ms[3] = { 0.0f, 0.0f, 0.0f };  /* mark, offsets, gather */
  hipEvent_t sel_ev[6] = { nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr };    /* (start, stop) of mark, offsets, gather */
  ~sn_query() {
    if (e) { e->ev_release(ev_start); e->ev_release(ev_stop); ev_start = ev_stop = nullptr; }
    if (ev_start) (void)hipEventDestroy(ev_start);
    if (ev_stop) (void)hipEventDestroy(ev_stop);
    for (hipEvent_t &ev : sel_ev) {
      if (e) e->ev_release(ev);
      else if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
    }
  }
};

static bool batch_skippable(const Batch &b, const sn_plan *p, const Table *t) {
  if (!b.stats_valid || b.has_deltas || b.has_deletes) return false;
  for (int i = 0; i < p->npreds; i++) {
    const sn_pred &pr = p->preds[i];
    int c = pr.col;
    if (b.null_count[c] >= b.num_rows && b.num_rows > 0) return true;
    if (b.bounds_null[c]) continue;
    sn_type_t dt = t->schema[c].dtype;
    bool is_d = dt == SN_TYPE_DOUBLE || dt == SN_TYPE_FLOAT;
    if (is_d) {
      if (pr.has_lo && (pr.lo_strict ? b.hi_d[c] <= pr.lo_d : b.hi_d[c] < pr.lo_d)) return true;
      if (pr.has_hi && (pr.hi_strict ? b.lo_d[c] >= pr.hi_d : b.lo_d[c] > pr.hi_d)) return true;
    } else {
      if (pr.has_lo && (pr.lo_strict ? b.hi_i[c] <= pr.lo_i : b.hi_i[c] < pr.lo_i)) return true;
      if (pr.has_hi && (pr.hi_strict ? b.lo_i[c] >= pr.hi_i : b.lo_i[c] > pr.hi_i)) return true;
    }
  }
  return false;
}

/* engine-cached device workspace for the open-address hash aggregate */
static int ensure_sparse_ws(sn_engine *e, int cap_log2, int naggs1) {
  size_t cap = 1ull << cap_log2;
  if (!e->hws_keys || e->hws_cap_log2 < cap_log2) {
    e->hws_keys = (long long *)e->arena.alloc(cap * 8);
    e->hws_okeys = (long long *)e->arena.alloc((cap + 1) * 8);
    e->hws_cap_log2 = cap_log2;
    e->hws_acc_bytes = 0;
    if (!e->hws_keys || !e->hws_okeys) return SN_ERR_NOMEM;
  }
  size_t accb = ((1ull << e->hws_cap_log2) + 2) * (size_t)naggs1 * 8;
  if (e->hws_acc_bytes < accb) {
    e->hws_acc = (double *)e->arena.alloc(accb);
    e->hws_orows = (double *)e->arena.alloc(accb);
    e->hws_acc_bytes = accb;
    if (!e->hws_acc || !e->hws_orows) return SN_ERR_NOMEM;
  }
  if (!e->hws_flags) {
    e->hws_flags = (int32_t *)e->arena.alloc(64);
    if (!e->hws_flags) return SN_ERR_NOMEM;
  }
  return SN_OK;
}

/* ---- submit phases ----
 * submit_impl (below) calls these in order.  Each returns SN_OK or the code
 * it has already passed to fail(). */

static int use_col(sn_query *q, int c) {
  if (c < 0 || c >= (int)q->t->schema.size()) return -1;
  if (q->cslot_of_col[c] < 0) {
    if ((int)q->used_cols.size() >= SN_DEV_MAX_COLS) return -1;
    q->cslot_of_col[c] = (int)q->used_cols.size();
    q->used_cols.push_back(c);
  }
  return q->cslot_of_col[c];
}

/* collect referenced columns -> device col slots */
static int32_t collect_plan_columns(sn_query *q) {
  const Table *t = q->t;
  const sn_plan *plan = &q->plan;
  for (int i = 0; i < 64; i++) q->cslot_of_col[i] = -1;
  for (int i = 0; i < plan->npreds; i++) {
    const sn_pred &pr = plan->preds[i];
    if (use_col(q, pr.col) < 0) return fail(SN_ERR_BADARG, "bad pred col");
    if (t->schema[pr.col].dtype == SN_TYPE_STRING &&
        (!pr.str_eq || pr.str_len <= 0) && pr.in_n <= 0)
      return fail(SN_ERR_UNSUPPORTED,
                  "string predicate supports dictionary equality (str_eq) and "
                  "IN-lists (in_s) only");
  }
  for (int i = 0; i < plan->ngroup; i++) {
    int c = plan->group_cols[i];
    sn_type_t gdt = t->schema[c].dtype;
    bool int_key = gdt == SN_TYPE_INT32 || gdt == SN_TYPE_INT16 ||
                   gdt == SN_TYPE_INT64;
    if (gdt != SN_TYPE_STRING && !int_key)
      return fail(SN_ERR_UNSUPPORTED,
                  "group-by supports dictionary string and int16/int32/int64 key columns");
    if (int_key && t->schema[c].nullable && plan->ngroup != 1)
      /* a NULL in one key of a pair is a distinct composite group the
       * packed sparse key cannot represent */
      return fail(SN_ERR_UNSUPPORTED,
                  "nullable integer group keys supported for single-column "
                  "group-bys only");
    if (use_col(q, c) < 0) return fail(SN_ERR_BADARG, "bad group col");
  }
  if (plan->ngroup == 2 && plan->group_cols[0] == plan->group_cols[1])
    /* both keys share one device column slot, which cannot carry two
     * different premultiplied dictionary images — found by the parity
     * fuzzer producing off-diagonal keys.  GROUP BY a, a is degenerate;
     * reject loudly so the planner dedups upstream. */
    return fail(SN_ERR_UNSUPPORTED, "duplicate group column (dedup upstream)");
  for (int a = 0; a < plan->naggs; a++)
    for (int f = 0; f < plan->aggs[a].nfactors; f++) {
      int c = plan->aggs[a].factors[f].col;
      sn_type_t dt = t->schema[c].dtype;
      if (dt == SN_TYPE_STRING) return fail(SN_ERR_UNSUPPORTED, "string agg input");
      if (use_col(q, c) < 0) return fail(SN_ERR_BADARG, "too many plan columns");
    }
  return SN_OK;
}

/* broadcast-dimension join: q->join_dim stays null without one */
static int32_t resolve_join(sn_query *q) {
  sn_engine *e = q->e;
  const Table *t = q->t;
  const sn_plan *plan = &q->plan;
  if (plan->join_dim == SN_JOIN_NONE) return SN_OK;
  if (plan->join_dim < 0 || plan->join_dim >= (int32_t)e->dims.size())
    return fail(SN_ERR_BADARG, "unknown dimension %d", plan->join_dim);
  Dim *jd = e->dims[plan->join_dim].get();
  if (jd->keys.empty() && !jd->dev_keys)
    return fail(SN_ERR_BADARG, "empty dimension");
  sn_type_t kt = t->schema[plan->join_fact_col].dtype;
  if (kt != SN_TYPE_INT32 && kt != SN_TYPE_INT64)
    return fail(SN_ERR_UNSUPPORTED, "join key must be int32/int64");
  if (plan->join_mode == SN_JOIN_GROUP && plan->ngroup > 1)
    return fail(SN_ERR_UNSUPPORTED,
                "dim-attr grouping supports at most ONE fact group column "
                "(attr + fact key fill the 2-key result row)");
  if (use_col(q, plan->join_fact_col) < 0)
    return fail(SN_ERR_BADARG, "too many plan columns");
  if (plan->join_mode == SN_JOIN_GROUP && jd->attr_maxlen > SN_KEY_MAX - 1)
    return fail(SN_ERR_UNSUPPORTED,
                "dimension attribute exceeds the %d-byte group-key limit",
                SN_KEY_MAX - 1);
  int rc = dim_device_table(e, jd);
  if (rc != SN_OK) return rc;
  q->join_dim = jd;
  q->join_group = plan->join_mode == SN_JOIN_GROUP;
  return SN_OK;
}

/* integer group keys: the slot space is the stats-derived value range
 * (the DictionaryOptimizedMapAccessor direct-slot idea applied to ints).
 * Requires every batch to carry valid bounds for the key column and no
 * update patches on it (patches may move values outside the bounds).
 * Returns the dense-slot span of an integer key column, or -1 when the dense
 * path is unavailable (missing stats bounds, update patches, overflowing
 * span) — the caller then falls back to the open-address hash aggregate */
static int64_t int_key_span(const Table *t, int c, int64_t *mn_out) {
  int64_t mn = 0, mx = -1;
  bool first = true;
  for (auto &b : t->batches) {
    if (!b.stats_valid || b.bounds_null[c]) return -1;
    if (b.had_patches.size() > (size_t)c && b.had_patches[c]) return -1;
    if (first) { mn = b.lo_i[c]; mx = b.hi_i[c]; first = false; }
    else {
      mn = b.lo_i[c] < mn ? b.lo_i[c] : mn;
      mx = b.hi_i[c] > mx ? b.hi_i[c] : mx;
    }
  }
  if (first) { *mn_out = 0; return 1; }   /* empty table */
  *mn_out = mn;
  return mx - mn + 1;
}

/* group slot space: global dict sizes, plus a null slot only when the
 * schema allows null keys (non-nullable key columns waste no slots —
 * keeps Q1's 3x2 keys in the register-friendly 8x8 kernel) */
static int32_t derive_group_slots(sn_query *q, bool dec) {
  const Table *t = q->t;
  const sn_plan *plan = &q->plan;
  if (plan->ngroup >= 1) {
    /* group keys travel as fixed SN_KEY_MAX-byte strings in results and
     * partial blocks; distinct keys sharing a 47-byte prefix would silently
     * merge — reject loudly instead (the reference has no key-length limit,
     * so this is a declared engine restriction, not silent divergence) */
    for (int i = 0; i < plan->ngroup; i++) {
      int gc = plan->group_cols[i];
      if (t->schema[gc].dtype == SN_TYPE_STRING &&
          t->gdict_maxlen[gc] > SN_KEY_MAX - 1)
        return fail(SN_ERR_UNSUPPORTED,
                    "group key col %d has a %d-byte dictionary entry > %d-byte key limit",
                    gc, t->gdict_maxlen[gc], SN_KEY_MAX - 1);
    }
    /* try the dense direct-slot space (dictionary ids / stats-ranged
     * integers); integer keys whose span is unbounded, statless, patched or
     * beyond SN_BIG_GROUP_CAP fall back to the open-address hash aggregate
     * (the ByteBufferHashMap/SHAMap analogue, k_grouped_hash) */
    bool col_sparse[2] = { false, false };
    bool any_string = false;
    int caps[2] = { 1, 1 };
    for (int i = 0; i < plan->ngroup; i++) {
      int c = plan->group_cols[i];
      sn_type_t gdt = t->schema[c].dtype;
      if (gdt == SN_TYPE_STRING) {
        any_string = true;
        caps[i] = (int)t->gdict[c].size() + (t->schema[c].nullable ? 1 : 0);
        continue;
      }
      int64_t span = (gdt == SN_TYPE_INT64 || t->schema[c].nullable)
                         ? -1 : int_key_span(t, c, &q->gmin[i]);
      if (span < 0 || span > SN_BIG_GROUP_CAP) { col_sparse[i] = true; continue; }
      q->gint[i] = true;
      caps[i] = (int)span;
    }
    int64_t dense_slots = (int64_t)std::max(caps[0], 1) *
                          (int64_t)std::max(caps[1], 1);
    q->sparse = col_sparse[0] || col_sparse[1] ||
                (!any_string && dense_slots > SN_BIG_GROUP_CAP);
    if (q->sparse && dec)
      return fail(SN_ERR_UNSUPPORTED,
                  "decimal aggregation needs dense group slots (dictionary strings "
                  "or stats-dense int16/int32 keys); sparse-hash group keys are "
                  "not supported");
    if (q->sparse) {
      if (any_string)
        return fail(SN_ERR_UNSUPPORTED,
                    "mixed string + sparse integer group keys not supported");
      if (plan->ngroup == 2 &&
          (t->schema[plan->group_cols[0]].dtype == SN_TYPE_INT64 ||
           t->schema[plan->group_cols[1]].dtype == SN_TYPE_INT64))
        return fail(SN_ERR_UNSUPPORTED,
                    "two-column group keys with an int64 column not supported "
                    "(keys pack into one 64-bit word)");
      if (q->join_dim)
        return fail(SN_ERR_UNSUPPORTED, "join combined with sparse group keys");
      q->gint[0] = q->gint[1] = false;
      q->nslots = 0;
      q->g1cap = q->g2cap = 1;
    } else {
      q->g1cap = caps[0];
      q->g2cap = plan->ngroup == 2 ? caps[1] : 1;
      if (!q->gint[0] && t->schema[plan->group_cols[0]].nullable)
        q->gnull1 = q->g1cap - 1;
      if (plan->ngroup == 2 && !q->gint[1] &&
          t->schema[plan->group_cols[1]].nullable)
        q->gnull2 = q->g2cap - 1;
      if (q->g1cap == 0) q->g1cap = 1;
      if (q->g2cap == 0) q->g2cap = 1;
      q->nslots = q->g1cap * q->g2cap;
      if (q->nslots > SN_BIG_GROUP_CAP)
        return fail(SN_ERR_UNSUPPORTED, "group cardinality %d > %d",
                    q->nslots, SN_BIG_GROUP_CAP);
    }
  } else if (q->join_group) {
    q->nslots = (int)q->join_dim->attr_dict.size();
    if (q->nslots > SN_MAX_GROUP_SLOTS)
      return fail(SN_ERR_UNSUPPORTED, "dim attr cardinality %d > %d",
                  q->nslots, SN_MAX_GROUP_SLOTS);
  } else {
    q->nslots = 1;
  }
  if (q->join_group && plan->ngroup >= 1) {
    /* composite GROUP BY dim_attr, fact_col: attr-major slots over the
     * dense fact slot space (sparse fact keys were rejected above) */
    const int attr_cap = (int)q->join_dim->attr_dict.size();
    if (attr_cap > SN_MAX_GROUP_SLOTS)
      return fail(SN_ERR_UNSUPPORTED, "dim attr cardinality %d > %d",
                  attr_cap, SN_MAX_GROUP_SLOTS);
    q->fact_slots = q->nslots;
    const int64_t total = (int64_t)attr_cap * q->fact_slots;
    if (total > SN_BIG_GROUP_CAP)
      return fail(SN_ERR_UNSUPPORTED, "attr x fact group cardinality %lld > %d",
                  (long long)total, SN_BIG_GROUP_CAP);
    q->nslots = (int)total;
  }
  return SN_OK;
}

/* a dictionary column's global ids reach the kernels premultiplied by g2cap
 * (so slot = id0 * g2cap + id1 needs no multiply per row) unless it is the
 * second group column; its nulls map to the column's null slot likewise.
 * Predicate literals, IN-lists, dictmaps and string patch values must all
 * agree on this, so all of them ask here. */
struct DictPremul { int mul, null_gid; };
static DictPremul dict_premul(const sn_query *q, const sn_plan *plan, int col) {
  const bool is_g2 = plan->ngroup == 2 && plan->group_cols[1] == col;
  const int gn = is_g2 ? q->gnull2 : q->gnull1;
  return { is_g2 ? 1 : (q->g2cap > 0 ? q->g2cap : 1),
           gn >= 0 ? (is_g2 ? gn : gn * q->g2cap) : 0 };
}

/* global dict id of a string literal, -1 when no batch interned it */
static int64_t dict_lookup(const Table *t, int col, const char *s, size_t len) {
  auto it = t->gdict_idx[col].find(std::string(s, len));
  return it != t->gdict_idx[col].end() ? it->second : -1;
}

/* upload a query-owned block (recycled at sn_query_destroy) */
static const void *up_owned(sn_query *q, const void *host, size_t n) {
  void *d = q->e->arena.alloc(n);
  if (!d || hipMemcpy(d, host, n, hipMemcpyHostToDevice) != hipSuccess)
    return nullptr;
  q->owned.push_back({ d, n });
  return d;
}

/* predicates as closed intervals (strictness folded via nextafter / +-1,
 * missing bounds as +-inf) */
static int32_t build_preds(sn_query *q, sn_dev_plan &dp) {
  const Table *t = q->t;
  const sn_plan *plan = &q->plan;
  for (int i = 0; i < plan->npreds; i++) {
    const sn_pred &s = plan->preds[i];
    sn_type_t dt = t->schema[s.col].dtype;
    int cslot = q->cslot_of_col[s.col];
    if (s.in_n > 0) {
      /* IN-list membership (Q12/Q19-class): integer values directly,
       * dictionary strings resolved to premultiplied global ids (absent
       * literals drop out).  Dense value spans build a bitmap LUT; wide
       * spans keep a sorted list (binary-searched; interpreted kernels). */
      if (dp.npreds_in >= 2) return fail(SN_ERR_BADARG, "too many IN predicates");
      if (s.has_lo || s.has_hi)
        return fail(SN_ERR_BADARG, "an IN predicate may not also carry range bounds");
      std::vector<int64_t> vals;
      if (dt == SN_TYPE_STRING) {
        if (!s.in_s || !s.in_s_len) return fail(SN_ERR_BADARG, "IN needs in_s");
        const int64_t mul = dict_premul(q, plan, s.col).mul;
        for (int32_t vi = 0; vi < s.in_n; vi++) {
          int64_t gid = dict_lookup(t, s.col, s.in_s[vi], (size_t)s.in_s_len[vi]);
          if (gid >= 0) vals.push_back(gid * mul);
        }
      } else {
        if (!s.in_i) return fail(SN_ERR_BADARG, "IN needs in_i");
        vals.assign(s.in_i, s.in_i + s.in_n);
      }
      std::sort(vals.begin(), vals.end());
      vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
      if (vals.empty()) {
        /* no literal matches anything: impossible range */
        sn_dev_pred_d &d = dp.preds_d[dp.npreds_d++];
        d.cslot = cslot; d.lo = 1.0; d.hi = 0.0;
        continue;
      }
      auto &ip = dp.inp[dp.npreds_in++];
      memset(&ip, 0, sizeof(ip));
      ip.cslot = cslot;
      const int64_t mn = vals.front(), mx = vals.back();
      if (mx - mn < (1ll << 20)) {
        const int64_t nwords = ((mx - mn) >> 6) + 1;
        std::vector<uint64_t> bm((size_t)nwords, 0);
        for (int64_t v : vals) bm[(v - mn) >> 6] |= 1ull << ((v - mn) & 63);
        ip.bm = (const uint64_t *)up_owned(q, bm.data(), bm.size() * 8);
        if (!ip.bm) return fail(SN_ERR_NOMEM, "IN bitmap upload");
        ip.base = mn;
        ip.nwords = (int32_t)nwords;
      } else {
        ip.list = (const int64_t *)up_owned(q, vals.data(), vals.size() * 8);
        if (!ip.list) return fail(SN_ERR_NOMEM, "IN list upload");
        ip.n = (int32_t)vals.size();
      }
      continue;
    }
    if (dt == SN_TYPE_STRING) {
      /* dictionary pushdown: literal -> global dict id, compared against
       * the (possibly premultiplied) id the conversion pass writes */
      const int64_t mul = dict_premul(q, plan, s.col).mul;
      const int64_t gid = dict_lookup(t, s.col, s.str_eq, (size_t)s.str_len);
      sn_dev_pred_d &d = dp.preds_d[dp.npreds_d++];
      d.cslot = cslot;
      if (gid < 0) { d.lo = 1.0; d.hi = 0.0; }   /* literal absent: no rows */
      else { d.lo = d.hi = (double)(gid * mul); }
      continue;
    }
    if (dt == SN_TYPE_INT64) {
      if (dp.npreds_i >= 4) return fail(SN_ERR_BADARG, "too many int64 preds");
      sn_dev_pred_i &d = dp.preds_i[dp.npreds_i++];
      d.cslot = cslot;
      d.lo = s.has_lo ? (s.lo_strict && s.lo_i < INT64_MAX ? s.lo_i + 1 : s.lo_i)
                      : INT64_MIN;
      d.hi = s.has_hi ? (s.hi_strict && s.hi_i > INT64_MIN ? s.hi_i - 1 : s.hi_i)
                      : INT64_MAX;
    } else {
      bool is_d = (dt == SN_TYPE_DOUBLE || dt == SN_TYPE_FLOAT);
      sn_dev_pred_d &d = dp.preds_d[dp.npreds_d++];
      d.cslot = cslot;
      double lo = s.has_lo ? (is_d ? s.lo_d : (double)s.lo_i) : -INFINITY;
      double hi = s.has_hi ? (is_d ? s.hi_d : (double)s.hi_i) : INFINITY;
      if (s.has_lo && s.lo_strict) lo = std::nextafter(lo, INFINITY);
      if (s.has_hi && s.hi_strict) hi = std::nextafter(hi, -INFINITY);
      d.lo = lo; d.hi = hi;
    }
  }
  return SN_OK;
}

/* INT64 factors: kernels convert the raw-bit i64 LDS image to double per
 * i64_mask.  A pure SUM(bigint_col) must stay BIT-EXACT (north star): f64
 * accumulation of integers is exact while every partial sum < 2^53, which
 * the stats bounds prove; when they cannot, fail loudly rather than round
 * silently.  (Affine/multi-factor expressions are double-typed in SQL — the
 * 1e-6 double budget applies, no gate.) */
static int32_t prove_i64_sum_exact(const Table *t, int gc) {
  double bound = 0.0;
  bool provable = true;
  for (auto &bb : t->batches) {
    if (!bb.stats_valid || bb.bounds_null[gc] ||
        (bb.had_patches.size() > (size_t)gc && bb.had_patches[gc])) {
      provable = false;
      break;
    }
    double mx = std::max(std::fabs((double)bb.lo_i[gc]),
                         std::fabs((double)bb.hi_i[gc]));
    bound += (double)bb.num_rows * mx;
  }
  if (!provable || bound >= 9007199254740992.0 /* 2^53 */)
    return fail(SN_ERR_UNSUPPORTED,
                "SUM over int64 col %d cannot be proven f64-exact "
                "(needs stats bounds with rows*max|v| < 2^53)", gc);
  return SN_OK;
}

/* aggregates as three neutral-padded factors: canonicalize each; in grouped
 * mode dedupe identical expressions and fold COUNT(*) into the per-slot
 * rowcount, so e.g. Q1's 8 logical aggregates run 5 device sweeps (sum/avg
 * pairs share) */
static int32_t build_aggs(sn_query *q, sn_dev_plan &dp, bool dec) {
  const sn_plan *plan = &q->plan;
  const bool grouped = plan->ngroup > 0 || q->join_group;
  int ndev = 0;
  for (int a = 0; a < plan->naggs; a++) {
    sn_dev_agg da;
    da.a0 = da.a1 = da.a2 = 1.0;
    da.m0 = da.m1 = da.m2 = 0.0;
    da.c0 = da.c1 = da.c2 = 0;
    da.nf = 0;
    da._p2 = 0;
    const sn_agg &sa = plan->aggs[a];
    da.op = sa.kind == SN_AGG_MIN ? 1 : sa.kind == SN_AGG_MAX ? 2 : 0;
    if (da.op != 0 && sa.nfactors < 1)
      return fail(SN_ERR_BADARG, "MIN/MAX needs at least one factor");
    if (sa.kind != SN_AGG_COUNT_STAR) {
      /* neutral factors get c = c0 below so their LDS reads CSE away */
      da.nf = sa.nfactors;
      if (sa.nfactors >= 1) {
        da.c0 = q->cslot_of_col[sa.factors[0].col];
        da.a0 = sa.factors[0].add; da.m0 = sa.factors[0].mul;
        if (!dec && (dp.i64_mask & (1u << da.c0)) && sa.kind == SN_AGG_SUM &&
            sa.nfactors == 1 && sa.factors[0].add == 0.0 &&
            sa.factors[0].mul == 1.0) {
          int rc = prove_i64_sum_exact(q->t, sa.factors[0].col);
          if (rc != SN_OK) return rc;
        }
      }
      if (sa.nfactors >= 2) {
        da.c1 = q->cslot_of_col[sa.factors[1].col];
        da.a1 = sa.factors[1].add; da.m1 = sa.factors[1].mul;
      }
      if (sa.nfactors >= 3) {
        da.c2 = q->cslot_of_col[sa.factors[2].col];
        da.a2 = sa.factors[2].add; da.m2 = sa.factors[2].mul;
      }
      if (sa.nfactors < 2) da.c1 = da.c0;
      if (sa.nfactors < 3) da.c2 = sa.nfactors >= 2 ? da.c1 : da.c0;
    }
    if (grouped && sa.kind == SN_AGG_COUNT_STAR) {
      q->agg_map[a] = -1;
      continue;
    }
    int idx = -1;
    if (grouped) {
      for (int j = 0; j < ndev; j++)
        if (memcmp(&dp.aggs[j], &da, sizeof(da)) == 0) { idx = j; break; }
    }
    if (idx < 0) { idx = ndev; dp.aggs[ndev++] = da; }
    q->agg_map[a] = idx;
  }
  q->dev_naggs = grouped ? ndev : plan->naggs;
  dp.naggs = q->dev_naggs;
  for (int a = 0; a < q->dev_naggs; a++)
    if (dp.aggs[a].op != 0) q->mm = true;
  q->na_t = sn_na_t(q->dev_naggs);
  q->out_stride = 2 * (size_t)q->na_t + 1;
  return SN_OK;
}

/* build device plan — canonical branchless forms (build_preds, build_aggs) */
static int32_t build_dev_plan(sn_query *q, bool dec, sn_dev_plan &dp) {
  const Table *t = q->t;
  const sn_plan *plan = &q->plan;
  memset(&dp, 0, sizeof(dp));
  dp.naggs = plan->naggs;
  dp.ngroup = plan->ngroup; dp.nslots = q->nslots;
  dp.nused = (int32_t)q->used_cols.size();
  dp.i64_mask = 0;
  for (size_t ui = 0; ui < q->used_cols.size(); ui++)
    if (t->schema[q->used_cols[ui]].dtype == SN_TYPE_INT64)
      dp.i64_mask |= 1u << ui;
  for (int i = 0; i < plan->ngroup; i++) dp.gcol[i] = q->cslot_of_col[plan->group_cols[i]];
  dp.gmul0 = 1;
  if (plan->ngroup >= 1 && q->gint[0]) {
    dp.gbase[0] = q->gmin[0];
    dp.gmul0 = q->g2cap;       /* dict col0 premultiplies via its dictmap */
  }
  if (plan->ngroup == 2 && q->gint[1]) dp.gbase[1] = q->gmin[1];
  if (const Dim *jd = q->join_dim) {
    dp.jkeys = jd->dev_keys;
    dp.jpayload = jd->dev_payload;
    dp.jcap_log2 = jd->cap_log2;
    dp.jcslot = q->cslot_of_col[plan->join_fact_col];
    dp.jmode = plan->join_mode == SN_JOIN_GROUP ? 1 : 0;
    if (q->join_group && plan->ngroup >= 1)
      dp.jslot_mul = q->fact_slots;   /* composite dim_attr x fact_col */
    dp.jlut = jd->dev_lut;
    dp.jlut_min = jd->lut_min;
    dp.jlut_max = jd->lut_max;
  }
  int rc = build_preds(q, dp);
  return rc != SN_OK ? rc : build_aggs(q, dp, dec);
}

/* the batch descriptors + tile map this plan scans.  Expensive at many
 * batches (dict-map premultiply + uploads), so cached per plan signature; a
 * cached set is only reusable when stats-skip removes nothing for THIS plan
 * (skipping is an optimization — correctness is unaffected either way).  An
 * uncacheable set's blocks belong to the query.  (The caller holds t->mu —
 * same critical section as the slot derivation.) */
static int32_t resolve_scan_set(sn_query *q, const sn_dev_plan &dp,
                                bool narrow_ok, ScanSet *out) {
  sn_engine *e = q->e;
  Table *t = q->t;
  const sn_plan *plan = &q->plan;
  uint64_t sig = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { sig ^= v; sig *= 1099511628211ull; };
  for (int32_t c : q->used_cols) mix((uint64_t)c + 1);
  mix((uint64_t)plan->ngroup << 8);
  for (int i = 0; i < plan->ngroup; i++) mix((uint64_t)plan->group_cols[i] + 17);
  mix((uint64_t)(q->g1cap * 131 + q->g2cap));
  mix((uint64_t)(plan->join_dim + 3) * 29 + (uint64_t)plan->join_mode);
  mix((uint64_t)t->batches.size());
  for (auto &c : t->gdict) mix(c.size() * 7919);
  mix(narrow_ok ? 0x6e617277ull : 0);
  /* a row-returning scan's set (projection-only columns behind the predicate
   * columns, no aggregate inputs, so no pac) is not an aggregate plan's */
  if (q->select) mix(0x73656c656374ull + (uint64_t)plan->npreds);
  /* ... and a join scan's is not a plain select's: the fact key is a staged
   * slot behind the predicate columns (INNER, LEFT_ANTI) or a projection-only
   * one (LEFT_OUTER) */
  if (q->rjoin >= 0)
    mix(0x726a6f696eull + (q->rjoin == SN_RJOIN_LEFT_OUTER ? 1u : 0u));

  int64_t skip_count = 0;
  for (auto &b : t->batches)
    if (batch_skippable(b, plan, t)) skip_count++;
  q->batches_seen = (int64_t)t->batches.size();
  q->batches_skipped = skip_count;

  if (skip_count == 0) {
    for (auto &dc : t->desc_caches)
      if (dc.sig == sig && dc.batch_count == t->batches.size()) {
        *out = dc;
        q->rows_scanned = dc.rows;
        return SN_OK;
      }
  }

  ScanSet set;
  set.sig = sig; set.batch_count = t->batches.size();
  std::vector<sn_dev_batch> hbatches;
  std::vector<sn_dev_tile> htiles;
  /* JIT eligibility: every unskipped batch clean, kinds uniform + stageable
   * (derived here; kept in the cached set for reuse on hits) */
  bool jit_ok = true, jit_first = true;
  /* per-agg counts needed?  Only when a grouped plan's aggregate-input
   * columns carry ACTUAL nulls (null-free nullable schemas keep the
   * counts==rowcount fast layout, JIT included) */
  uint32_t agg_cmask = 0;
  for (int a = 0; a < q->dev_naggs; a++) {
    const sn_dev_agg &A = dp.aggs[a];
    if (A.nf >= 1) agg_cmask |= 1u << A.c0;
    if (A.nf >= 2) agg_cmask |= 1u << A.c1;
    if (A.nf >= 3) agg_cmask |= 1u << A.c2;
  }
  const size_t nused = q->used_cols.size();
  DictPremul pm[SN_DEV_MAX_COLS];
  for (size_t ui = 0; ui < nused; ui++) pm[ui] = dict_premul(q, plan, q->used_cols[ui]);
  /* a used f64 column scans from its 1-byte codes (SN_K_F64C8) only when
   * EVERY unskipped batch holds a live sidecar for it; otherwise all its
   * batches keep SN_K_F64 and the body, so kinds stay uniform per column
   * (the JIT's rule) and one high-cardinality batch simply means the plain
   * scan.  Decimal scans never narrow. */
  bool narrow_col[SN_DEV_MAX_COLS];
  for (size_t ui = 0; ui < nused; ui++) {
    const int c = q->used_cols[ui];
    bool all = narrow_ok && e->narrow &&
               t->schema[c].dtype == SN_TYPE_DOUBLE;
    for (auto &b : t->batches) {
      if (!all) break;
      if (skip_count && batch_skippable(b, plan, t)) continue;
      all = b.narrow[c].ndict > 0;
    }
    narrow_col[ui] = all;
  }
  for (auto &b : t->batches) {
    if (skip_count && batch_skippable(b, plan, t)) continue;
    sn_dev_batch db;
    memset(&db, 0, sizeof(db));
    db.num_rows = b.num_rows;
    db.del_bm = b.del_bm_dev;
    bool clean = !b.has_deletes;
    for (size_t ui = 0; ui < nused; ui++) {
      int rc = fill_dev_col(e, t, b, q->used_cols[ui], pm[ui].mul,
                            pm[ui].null_gid, true, &db.cols[ui], &clean);
      if (rc != SN_OK) return rc;
      if (narrow_col[ui]) {
        const Batch::Narrow &nw = b.narrow[q->used_cols[ui]];
        db.cols[ui].kind = SN_K_F64C8;
        db.cols[ui].body = nw.codes();
        db.cols[ui].rle_vals = nw.dict();
        db.cols[ui].rle_n = nw.ndict;
      }
    }
    db.clean = clean ? 1 : 0;
    for (size_t ui = 0; ui < nused; ui++)
      if (((agg_cmask >> ui) & 1) &&
          (db.cols[ui].has_nulls || db.cols[ui].patch_nullbm))
        set.pac = 1;
    /* deletes alone don't disqualify the JIT (the generated kernel reads
     * del_bm); nulls or unmaterialized patches on a used column do */
    if (db.del_bm) set.jit_del = 1;
    for (size_t ui = 0; ui < nused && jit_ok; ui++) {
      const sn_dev_col &jc = db.cols[ui];
      int k = jc.kind;
      bool stageable = k == SN_K_F64 || k == SN_K_I64 || k == SN_K_I32 ||
                       k == SN_K_F32 || k == SN_K_I16 || k == SN_K_DICT16 ||
                       k == SN_K_DICT32 || k == SN_K_F64C8;
      if (!stageable || jc.has_nulls || jc.patch_n > 0) jit_ok = false;
      else if (jit_first) set.jit_kinds[ui] = k;
      else if (set.jit_kinds[ui] != k) jit_ok = false;
    }
    jit_first = false;
    int32_t bi = (int32_t)hbatches.size();
    hbatches.push_back(db);
    set.rows += b.num_rows;
    for (int32_t r = 0; r < b.num_rows; r += SN_TILE_ROWS)
      htiles.push_back({ bi, r });
  }
  set.jit_ok = (jit_ok && !jit_first) ? 1 : 0;
  q->rows_scanned = set.rows;

  if (!htiles.empty()) {
    set.db_bytes = hbatches.size() * sizeof(sn_dev_batch);
    set.tl_bytes = htiles.size() * sizeof(sn_dev_tile);
    void *dbp = e->arena.alloc(set.db_bytes);
    void *tlp = e->arena.alloc(set.tl_bytes);
    if (!dbp || !tlp) return fail(SN_ERR_NOMEM, "desc alloc");
    /* blocking copies: the host vectors are stack-local and die at return */
    if (hipMemcpy(dbp, hbatches.data(), set.db_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tlp, htiles.data(), set.tl_bytes, hipMemcpyHostToDevice) != hipSuccess)
      return fail(SN_ERR_GENERIC, "desc upload");
    set.db_dev = dbp; set.tl_dev = tlp;
    set.ntiles = (int32_t)htiles.size();
    if (skip_count != 0) {
      /* not cacheable (stats-skip removed batches): this query owns the
       * descriptor blocks; they recycle at sn_query_destroy */
      q->owned.push_back({ dbp, set.db_bytes });
      q->owned.push_back({ tlp, set.tl_bytes });
    } else {
      if (t->desc_caches.size() > 16) {
        /* evict the oldest cached set (FIFO); stream ordering guarantees
         * any in-flight kernel reading it finishes before a reuse write */
        ScanSet &old = t->desc_caches.front();
        e->arena.release((void *)old.db_dev, old.db_bytes);
        e->arena.release((void *)old.tl_dev, old.tl_bytes);
        t->desc_caches.erase(t->desc_caches.begin());
      }
      t->desc_caches.push_back(set);
    }
  }
  *out = set;
  return SN_OK;
}

/* ---- launch helpers ---- */

/* IN-lists run compiled only in bitmap form (sorted-list search stays
 * interpreted) */
static bool jit_inlists_ok(const sn_dev_plan &dp) {
  return dp.npreds_in == 0 ||
         (dp.inp[0].bm && (dp.npreds_in < 2 || dp.inp[1].bm));
}

static void register_live(sn_engine *e, sn_query *q) {
  std::lock_guard<std::mutex> ga(e->aux_mu);
  e->live_q.insert(q);
}

/* grow the per-engine block-partial scratch to at least `need` bytes */
static int32_t ensure_scratch(sn_engine *e, size_t need) {
  if (e->scratch_sz >= need) return SN_OK;
  e->scratch = (double *)e->arena.alloc(need);
  e->scratch_sz = e->scratch ? need : 0;
  return e->scratch ? SN_OK : fail(SN_ERR_NOMEM, "scratch alloc");
}

/* HIP events bracket the scan kernel on ITS stream for the roofline leg
 * (torch.cuda.Event would only see torch's current stream) */
static void acquire_events(sn_query *q) {
  q->ev_start = q->e->ev_acquire();
  q->ev_stop = q->e->ev_acquire();
}

/* ---- exact DECIMAL launch (k_dec_keyless / k_dec_grouped) ----
 * canonical int64 factors, identical expressions deduped (Q1's sum/avg
 * pairs share a device aggregate), COUNT(*) from the slot rowcount */
static int32_t launch_decimal(sn_query *q, sn_dev_plan &dp, const ScanSet &set,
                              const DecReq *dec) {
  sn_engine *e = q->e;
  const sn_plan *plan = &q->plan;
  sn_dev_dec_plan ddp;
  memset(&ddp, 0, sizeof(ddp));
  int nd = 0;
  for (int a = 0; a < dec->naggs; a++) {
    const sn_dec_agg &sa = dec->aggs[a];
    q->agg_map[a] = a;
    if (sa.kind == SN_AGG_COUNT_STAR) { q->dec_map[a] = -1; continue; }
    sn_dev_dec_agg da;
    memset(&da, 0, sizeof(da));
    da.op = sa.kind == SN_AGG_MIN ? 1 : sa.kind == SN_AGG_MAX ? 2 : 0;
    da.nf = sa.nfactors;
    for (int f = 0; f < 3; f++) {
      if (f < sa.nfactors) {
        da.c[f] = q->cslot_of_col[sa.factors[f].col];
        da.add[f] = sa.factors[f].add;
        da.mul[f] = sa.factors[f].mul;
      } else {
        da.c[f] = da.c[0]; da.add[f] = 1; da.mul[f] = 0;
      }
    }
    int idx = -1;
    for (int j = 0; j < nd; j++)
      if (memcmp(&ddp.aggs[j], &da, sizeof(da)) == 0) { idx = j; break; }
    if (idx < 0) { idx = nd; ddp.aggs[nd++] = da; }
    q->dec_map[a] = idx;
  }
  ddp.naggs = nd;
  q->dec_ndev = nd;
  if (plan->ngroup == 0) q->nslots = 1;
  if (plan->ngroup > 0 && q->nslots > sn_dec_max_slots(dp.nused, nd))
    return fail(SN_ERR_UNSUPPORTED,
                "decimal group cardinality %d exceeds the %d-slot LDS accumulator "
                "capacity for %d columns x %d aggregates",
                q->nslots, sn_dec_max_slots(dp.nused, nd), dp.nused, nd);
  /* double view for sn_query_result: [sums naggs][counts naggs][rowcount] */
  q->dec = true;
  q->pac = true;
  q->dev_naggs = plan->naggs;
  q->na_t = plan->naggs;
  q->out_stride = 2 * (size_t)plan->naggs + 1;
  dp.nslots = q->nslots;
  if (set.ntiles == 0) return SN_OK;
  const size_t row_cells = (size_t)sn_dec_row_cells(nd);
  const size_t outb = (size_t)q->nslots * row_cells * 8;
  q->dec_out = (unsigned long long *)e->arena.alloc(outb);
  if (!q->dec_out) return fail(SN_ERR_NOMEM, "decimal out alloc");
  q->owned.push_back({ q->dec_out, outb });
  const size_t planb = sizeof(dp) + sizeof(ddp);
  uint8_t *plans_dev = (uint8_t *)e->arena.alloc(planb);
  if (!plans_dev ||
      hipMemcpy(plans_dev, &dp, sizeof(dp), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(plans_dev + sizeof(dp), &ddp, sizeof(ddp),
                hipMemcpyHostToDevice) != hipSuccess)
    return fail(SN_ERR_NOMEM, "decimal plan upload");
  q->owned.push_back({ plans_dev, planb });
  const size_t grid = (size_t)std::min<int32_t>(set.ntiles, SN_DEC_GRID_CAP);
  int rc = ensure_scratch(e, grid * (size_t)q->nslots * row_cells * 8);
  if (rc != SN_OK) return rc;
  acquire_events(q);
  if (q->ev_start) (void)hipEventRecord(q->ev_start, e->stream);
  rc = sn_launch_dec_scan(&dp, (const sn_dev_plan *)plans_dev, &ddp,
                          (const sn_dev_dec_plan *)(plans_dev + sizeof(dp)),
                          (const sn_dev_batch *)set.db_dev,
                          (const sn_dev_tile *)set.tl_dev, set.ntiles,
                          q->dec_out,
                          (unsigned long long *)e->scratch, e->stream);
  if (q->ev_stop) (void)hipEventRecord(q->ev_stop, e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "decimal kernel launch: %s",
                hipGetErrorString((hipError_t)rc));
  return SN_OK;
}

/* radix pass-1 buffers for one sparse attempt: grow the engine-cached record
 * buffer and per-partition counters, point dps at them and zero the
 * counters.  *radix goes false (single-pass probe instead) when the records
 * would not fit. */
static int32_t radix_prepare(sn_query *q, sn_dev_plan &dps, int cap_log2,
                             int sub_log2, bool *radix) {
  sn_engine *e = q->e;
  const int npart = 1 << (cap_log2 - sub_log2);
  const long long percap =
      2 * q->rows_scanned / npart + 4096;
  const size_t recb = (size_t)npart * (size_t)percap *
                      (size_t)(1 + q->dev_naggs) * 8;
  if (percap > INT32_MAX / 2 || recb > (48ull << 30)) {
    *radix = false;
    return SN_OK;
  }
  if (!e->rws_recs || e->rws_bytes < recb) {
    if (e->rws_recs) e->arena.release(e->rws_recs, e->rws_bytes);
    e->rws_recs = (double *)e->arena.alloc(recb);
    e->rws_bytes = e->rws_recs ? recb : 0;
  }
  if (e->rws_npart < npart) {
    if (e->rws_pcount)
      e->arena.release(e->rws_pcount, (size_t)e->rws_npart * 4);
    e->rws_pcount = (int32_t *)e->arena.alloc((size_t)npart * 4);
    e->rws_npart = e->rws_pcount ? npart : 0;
  }
  if (!e->rws_recs || !e->rws_pcount) {
    *radix = false;               /* fall back to the single pass */
    return SN_OK;
  }
  dps.radix = sub_log2;
  dps.precs = e->rws_recs;
  dps.pcount = e->rws_pcount;
  dps.percap = (int32_t)percap;
  if (hipMemsetAsync(e->rws_pcount, 0, (size_t)npart * 4,
                     e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "radix counters zero");
  return SN_OK;
}

/* compact the finished hash table on device (unless the LDS radix pass
 * already did) and read the groups back into the query */
static int32_t sparse_readback(sn_query *q, size_t cap, int naggs1,
                               bool radix_direct) {
  sn_engine *e = q->e;
  /* the LDS radix pass already compacted into okeys/orows (counter at
   * hws_flags[1]); otherwise compact the table here */
  if (!radix_direct &&
      (hipMemsetAsync(e->hws_flags + 1, 0, 4, e->stream) != hipSuccess ||
       sn_launch_hash_compact(e->hws_keys, e->hws_acc, (int)cap, naggs1,
                              e->hws_okeys, e->hws_orows,
                              (int *)(e->hws_flags + 1), e->stream) != 0 ||
       hipStreamSynchronize(e->stream) != hipSuccess))
    return fail(SN_ERR_GENERIC, "hash-agg compact");
  int32_t ngrp = 0;
  (void)hipMemcpy(&ngrp, e->hws_flags + 1, 4, hipMemcpyDeviceToHost);
  /* the NULL-key group accumulates in the extra row at cap+1 (the
   * compaction covers rows [0, cap]) */
  q->sparse_null_row.assign((size_t)naggs1, 0.0);
  (void)hipMemcpy(q->sparse_null_row.data(),
                  e->hws_acc + (size_t)(cap + 1) * naggs1,
                  (size_t)naggs1 * 8, hipMemcpyDeviceToHost);
  q->sparse_keys.reset(new long long[(size_t)ngrp + 1]);
  q->sparse_rows.reset(new double[((size_t)ngrp + 1) * naggs1]);
  q->sparse_n = (size_t)ngrp;
  if (ngrp > 0) {
    /* plain pageable D2H: measured ~55 GB/s and stable once the heap
     * recycles (mallopt in engine create) — the pinned bounce costs a
     * second 24 MB host memcpy for nothing */
    if (hipMemcpy(q->sparse_keys.get(), e->hws_okeys, (size_t)ngrp * 8,
                  hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(q->sparse_rows.get(), e->hws_orows,
                  (size_t)ngrp * naggs1 * 8,
                  hipMemcpyDeviceToHost) != hipSuccess)
      return fail(SN_ERR_GENERIC, "hash-agg readback");
  }
  if (radix_direct) {
    /* the LDS compaction never scans the (untouched) global table, so
     * append the reserved sentinel-key row (a REAL key of -1) here —
     * the same row k_hash_compact emits from index cap (the arrays
     * were sized ngrp+1 for exactly this) */
    double *rrow = q->sparse_rows.get() + q->sparse_n * naggs1;
    (void)hipMemcpy(rrow, e->hws_acc + (size_t)cap * naggs1,
                    (size_t)naggs1 * 8, hipMemcpyDeviceToHost);
    if (rrow[naggs1 - 1] != 0.0) {
      q->sparse_keys[q->sparse_n] = SN_HASH_EMPTY;
      q->sparse_n++;
    }
  }
  return SN_OK;
}

/* ---- open-address hash-aggregate launch (k_grouped_hash) ----
 * The workspace (key table + accumulators) is engine-cached; results
 * are compacted on device and read back HERE (inside submit, stream
 * synchronized), so concurrent queries never share the live table. */
static int32_t launch_sparse(sn_query *q, const sn_dev_plan &dp,
                             const ScanSet &set) {
  sn_engine *e = q->e;
  Table *t = q->t;
  if (set.ntiles == 0) return SN_OK;
  const int naggs1 = (q->pac ? 2 : 1) * q->dev_naggs + 1;
  /* capacity: 2x headroom over the worst-case distinct count keeps the
   * linear probe short (load factor <= 0.5 at full distinctness); the
   * fill counter grows the table before probing turns pathological,
   * and the per-table hint skips the rediscovery next query */
  int cap_log2 = 21;
  while (cap_log2 > 12 && (1ll << (cap_log2 - 1)) >= 2 * q->rows_scanned)
    cap_log2--;                      /* small tables: smaller table */
  if (t->sparse_cap_hint > cap_log2) cap_log2 = t->sparse_cap_hint;
  acquire_events(q);
  /* radix two-pass: the single-pass probe touches ~3 random
   * 64 B lines per row across a table far bigger than L2 (measured
   * 182 B/row of HBM traffic on 1M keys).  For big tables the compiled
   * pass 1 scatters (key, values) records into cap/4096 hash partitions
   * (streaming traffic) and k_radix_agg aggregates each partition into
   * its private L2-resident table segment.  JIT-only (clean batches);
   * pac excluded (records carry values, not per-agg validity). */
  static const bool radix_env = [] {
    const char *v = getenv("SN_RADIX");
    return !v || v[0] != '0';
  }();
  static const int sub_env = [] {      /* A/B lever for the sweep */
    const char *v = getenv("SN_RADIX_SUB");
    return v ? atoi(v) : 0;
  }();
  bool radix_ok = radix_env && !q->pac && q->dev_naggs <= 4;
  bool done_h = false;
  for (int attempt = 0; attempt < 4 && !done_h; attempt++) {
    if (ensure_sparse_ws(e, cap_log2, naggs1) != SN_OK)
      return fail(SN_ERR_NOMEM, "sparse hash workspace");
    const size_t cap = 1ull << cap_log2;
    sn_dev_plan dps = dp;
    dps.sparse = 1;
    dps.hkeys = e->hws_keys;
    dps.hacc = e->hws_acc;
    dps.hflags = e->hws_flags;
    dps.hcap_log2 = cap_log2;
    bool radix = radix_ok && cap_log2 >= 17;
    const int sub_log2 =
        std::max(sub_env ? sub_env : SN_RADIX_SUB_MIN,
                 cap_log2 - SN_RADIX_NPART_MAX_LOG2);
    if (radix) {
      int rc = radix_prepare(q, dps, cap_log2, sub_log2, &radix);
      if (rc != SN_OK) return rc;
    }
    const void *dps_dev = up_owned(q, &dps, sizeof(dps));
    if (!dps_dev) return fail(SN_ERR_NOMEM, "sparse plan upload");
    if (hipMemsetAsync(e->hws_keys, 0xff, cap * 8, e->stream) != hipSuccess ||
        hipMemsetAsync(e->hws_acc, 0, (cap + 2) * (size_t)naggs1 * 8,
                       e->stream) != hipSuccess ||
        hipMemsetAsync(e->hws_flags, 0, 16, e->stream) != hipSuccess)
      return fail(SN_ERR_GENERIC, "sparse workspace zero");
    if (q->mm &&
        sn_launch_acc_init(e->hws_acc, (long long)cap + 2, q->dev_naggs,
                           naggs1, dps_dev, e->stream) != 0)
      return fail(SN_ERR_GENERIC, "sparse min/max init");
    /* query-compiled twin first (plan structure compile-time, capacity
     * tokenized); any miss falls back to the interpreted hash kernel */
    void *jfn = nullptr;
    if (e->jit && jit_inlists_ok(dp) && sn_jit_shape_ok(&dps) && set.jit_ok)
      jfn = sn_jit_get(e->jit, &dps, set.jit_kinds, 0, q->na_t, set.jit_del);
    if (q->ev_start) (void)hipEventRecord(q->ev_start, e->stream);
    int rc = -1;
    if (jfn) {
      rc = sn_jit_launch(jfn, sn_balanced_grid(set.ntiles, SN_GRID_CAP),
                         (const sn_dev_batch *)set.db_dev,
                         (const sn_dev_tile *)set.tl_dev, set.ntiles,
                         e->hws_acc, (const int64_t *)e->hws_keys,
                         (const int32_t *)e->hws_flags, nullptr,
                         (const sn_dev_plan *)dps_dev, e->stream);
      q->used_jit = rc == 0;
      if (rc != 0) jfn = nullptr;
    }
    if (!jfn)
      rc = sn_launch_hash_scan(&dps, (const sn_dev_plan *)dps_dev,
                               (const sn_dev_batch *)set.db_dev,
                               (const sn_dev_tile *)set.tl_dev, set.ntiles,
                               e->stream);
    /* radix pass 2: aggregate the partitioned records (only meaningful
     * after the compiled pass 1).  The LDS variant compacts straight
     * into okeys/orows via the counter at hws_flags[1]. */
    const bool radix_ran = radix && jfn;
    const bool radix_direct = radix_ran && sn_radix_direct(sub_log2, naggs1);
    if (rc == 0 && radix_ran)
      rc = sn_launch_radix_agg(&dps, (const sn_dev_plan *)dps_dev,
                               e->hws_okeys, e->hws_orows,
                               (int *)(e->hws_flags + 1), e->stream);
    if (q->ev_stop) (void)hipEventRecord(q->ev_stop, e->stream);
    if (rc != 0)
      return fail(SN_ERR_GENERIC, "hash-agg launch: %s",
                  hipGetErrorString((hipError_t)rc));
    if (hipStreamSynchronize(e->stream) != hipSuccess)
      return fail(SN_ERR_GENERIC, "hash-agg sync");
    int32_t fl[4] = { 0, 0, 0, 0 };
    (void)hipMemcpy(fl, e->hws_flags, 16, hipMemcpyDeviceToHost);
    if (radix_ran && fl[3]) {
      /* record buffer overflow (pathological key skew): redo this
       * attempt through the single-pass probe — nothing was lost, the
       * table is re-zeroed per attempt */
      radix_ok = false;
      attempt--;
      continue;
    }
    const int32_t ovf = fl[0];
    const int64_t fill = fl[2];
    /* grow on hard overflow OR load factor > 0.6 (probe chains degrade
     * sharply past that); results so far are correct either way */
    if (ovf || (fill * 5 > (int64_t)cap * 3 && cap_log2 < 24)) {
      if (ovf && cap_log2 >= 24)
        return fail(SN_ERR_OVERFLOW,
                    "sparse group cardinality exceeds the 2^24 hash table");
      cap_log2 = std::min(cap_log2 + 2, 24);
      continue;
    }
    t->sparse_cap_hint = std::max(t->sparse_cap_hint, cap_log2);
    rc = sparse_readback(q, cap, naggs1, radix_direct);
    if (rc != SN_OK) return rc;
    done_h = true;
  }
  return SN_OK;
}

/* device copy of a dense-path plan, cached per engine by content hash */
static void *cached_dev_plan(sn_engine *e, const sn_dev_plan &dp) {
  uint64_t dph = 1469598103934665603ull;
  const uint8_t *db_ = (const uint8_t *)&dp;
  for (size_t i = 0; i < sizeof(dp); i++) { dph ^= db_[i]; dph *= 1099511628211ull; }
  std::lock_guard<std::mutex> ga(e->aux_mu);
  auto it = e->dp_cache.find(dph);
  if (it != e->dp_cache.end()) return it->second;
  void *dp_dev = e->arena.alloc(sizeof(dp));
  if (!dp_dev ||
      hipMemcpy(dp_dev, &dp, sizeof(dp), hipMemcpyHostToDevice) != hipSuccess)
    return nullptr;
  if (e->dp_cache.size() > 64) {
    for (auto &kv : e->dp_cache)
      e->arena.release(kv.second, sizeof(sn_dev_plan));
    e->dp_cache.clear();
  }
  e->dp_cache[dph] = dp_dev;
  return dp_dev;
}

/* ---- late columns ----
 * The fraction of rows the plan's predicates keep, estimated from what the
 * batch-skip test already holds: each range predicate is taken as uniform
 * over [min, max] of its column across the unskipped batches (value counts
 * for integer columns, widths for doubles), and the fractions multiply.
 * String-equality and IN-list predicates count as keeping everything.  A
 * predicate column without bounds in some batch, or a batch with update
 * deltas (its bounds do not cover them), means no estimate: 1.0. */
#define SN_LATE_MAX_SEL 0.05

static double estimate_selectivity(const sn_query *q) {
  const Table *t = q->t;
  const sn_plan *p = &q->plan;
  double sel = 1.0;
  for (int i = 0; i < p->npreds; i++) {
    const sn_pred &pr = p->preds[i];
    if (pr.in_n > 0 || pr.str_eq || (!pr.has_lo && !pr.has_hi)) continue;
    const int c = pr.col;
    const sn_type_t dt = t->schema[c].dtype;
    const bool is_d = dt == SN_TYPE_DOUBLE || dt == SN_TYPE_FLOAT;
    bool any = false;
    double cmin = 0, cmax = 0;
    for (auto &b : t->batches) {
      if (q->batches_skipped && batch_skippable(b, p, t)) continue;
      if (!b.stats_valid || b.has_deltas || b.bounds_null[c]) return 1.0;
      const double lo = is_d ? b.lo_d[c] : (double)b.lo_i[c];
      const double hi = is_d ? b.hi_d[c] : (double)b.hi_i[c];
      cmin = any ? std::min(cmin, lo) : lo;
      cmax = any ? std::max(cmax, hi) : hi;
      any = true;
    }
    if (!any || !(cmax >= cmin)) return 1.0;   /* no batch, or NaN bounds */
    /* integer columns count values: [lo, hi] closed after the strict bits */
    const double unit = is_d ? 0.0 : 1.0;
    double lo = cmin, hi = cmax;
    if (pr.has_lo) lo = std::max(lo, is_d ? pr.lo_d : (double)pr.lo_i + (pr.lo_strict ? 1 : 0));
    if (pr.has_hi) hi = std::min(hi, is_d ? pr.hi_d : (double)pr.hi_i - (pr.hi_strict ? 1 : 0));
    const double span = cmax - cmin + unit, kept = hi - lo + unit;
    if (!(kept > 0.0)) return 0.0;
    if (span > 0.0) sel *= std::min(1.0, kept / span);
  }
  return sel;
}

/* Which used columns the compiled kernel of this launch reads late: plain
 * f64 columns (SN_K_F64 in every unskipped batch; the set is JIT-eligible,
 * so no nulls and no patches) that aggregate factors use and nothing else
 * does, in a keyless plan whose predicates are estimated to keep at most
 * SN_LATE_MAX_SEL of the rows.  kinds[] is the launch's copy of the set's
 * kinds; the device descriptors keep SN_K_F64.  Returns the used-slot mask. */
static uint32_t tag_late_columns(const sn_query *q, const sn_dev_plan &dp,
                                 int *kinds) {
  const sn_engine *e = q->e;
  const sn_plan *plan = &q->plan;
  if (!e->late || plan->ngroup > 0 || q->join_dim || q->sparse || dp.nslots > 1)
    return 0;
  uint32_t agg = 0, other = 0;
  for (int a = 0; a < dp.naggs; a++) {
    const sn_dev_agg &A = dp.aggs[a];
    if (A.nf >= 1) agg |= 1u << A.c0;
    if (A.nf >= 2) agg |= 1u << A.c1;
    if (A.nf >= 3) agg |= 1u << A.c2;
  }
  for (int i = 0; i < dp.npreds_d; i++) other |= 1u << dp.preds_d[i].cslot;
  for (int i = 0; i < dp.npreds_i; i++) other |= 1u << dp.preds_i[i].cslot;
  for (int i = 0; i < dp.npreds_in && i < 2; i++) other |= 1u << dp.inp[i].cslot;
  uint32_t mask = 0;
  for (int ui = 0; ui < dp.nused; ui++)
    if (kinds[ui] == SN_K_F64 && ((agg & ~other) >> ui & 1)) mask |= 1u << ui;
  /* some staged column must remain to carry the predicates */
  if (!mask || !other) return 0;
  if (!e->late_force && !(estimate_selectivity(q) <= SN_LATE_MAX_SEL)) return 0;
  /* the image-free kernel serves sums and counts under
   * range predicates over columns it can test in a register or by code */
  bool direct = e->direct && !q->mm && !dp.pac && dp.npreds_i == 0 &&
                dp.npreds_in == 0;
  for (int ui = 0; ui < dp.nused && direct; ui++)
    direct = ((mask >> ui) & 1) || kinds[ui] == SN_K_I32 ||
             kinds[ui] == SN_K_I16 || kinds[ui] == SN_K_F64C8;
  for (int ui = 0; ui < dp.nused; ui++)
    if ((mask >> ui) & 1)
      kinds[ui] = direct ? SN_K_F64_LATE_DIRECT : SN_K_F64_LATE;
  return mask;
}

/* ---- dense launch: keyless or direct-slot grouped (k_scan_agg family or
 * its query-compiled twin) into a per-query result buffer ---- */
static int32_t launch_dense(sn_query *q, const sn_dev_plan &dp,
                            const ScanSet &set) {
  sn_engine *e = q->e;
  const int32_t ntiles = set.ntiles;
  size_t out_n = (size_t)q->nslots * q->out_stride;
  q->dev_out = (double *)e->arena.alloc(out_n * 8);
  if (!q->dev_out) return fail(SN_ERR_NOMEM, "out alloc");
  q->owned.push_back({ q->dev_out, out_n * 8 });
  if (hipMemsetAsync(q->dev_out, 0, out_n * 8, e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "memset out");
  if (ntiles == 0) return SN_OK;
  void *dp_dev = cached_dev_plan(e, dp);
  if (!dp_dev) return fail(SN_ERR_NOMEM, "plan upload");
  /* one description of the launch, shared with sn_launch_scan_agg: scratch
   * holds the partial rows of whichever twin runs (interpreted or
   * compiled), or the 8 XCD-private copies of a global accumulator */
  sn_dense_launch d = sn_dense_launch_of(&dp, ntiles);
  /* query-compiled kernel (jit.cpp): plan constants baked as literals —
   * the WholeStageCodegen analogue; measured 3x on Q1's shape over the
   * interpreted runtime-plan kernel.  Any miss falls back, still on GPU. */
  void *jfn = nullptr;
  /* pac from ACTUAL nulls never reaches here (jit_ok excludes null
   * batches); pac from MIN/MAX compiles op-aware kernels. */
  uint32_t late = 0;
  bool direct = false;
  if (e->jit && sn_jit_shape_ok(&dp) && jit_inlists_ok(dp) && set.jit_ok) {
    /* the late tag depends on this plan's predicate bounds, which the cached
     * set's signature leaves out: it goes on a copy of the set's kinds */
    int kinds[SN_DEV_MAX_COLS];
    memcpy(kinds, set.jit_kinds, sizeof(kinds));
    late = tag_late_columns(q, dp, kinds);
    for (int ui = 0; ui < dp.nused; ui++)
      direct |= kinds[ui] == SN_K_F64_LATE_DIRECT;
    jfn = sn_jit_get(e->jit, &dp, kinds, dp.nslots, q->na_t, set.jit_del);
  }
  /* A keyless compiled kernel gets equal blocks in as few rounds as the
   * device can hold at once: with SN_GRID_CAP blocks on a device that holds
   * fewer, the last round runs part-filled.  d stays the one description:
   * scratch and the reduce below follow d.grid_compiled. */
  if (jfn && e->grid_resident && d.route == SN_ROUTE_KEYLESS) {
    const int resident = sn_jit_resident(e->jit, jfn);
    if (resident > 0 && resident <= SN_GRID_CAP)
      d.grid_compiled = sn_balanced_grid(ntiles, resident);
  }
  const size_t rows = (size_t)std::max(sn_dense_rows(&d, 0), sn_dense_rows(&d, 1));
  int rc = ensure_scratch(e, rows * d.nv * 8);
  if (rc != SN_OK) return rc;
  if (d.global_acc &&
      hipMemsetAsync(e->scratch, 0, rows * d.nv * 8, e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "accumulator zero");
  if (d.global_acc && q->mm &&
      sn_launch_acc_init(e->scratch, (long long)rows * dp.nslots, q->dev_naggs,
                         d.na1, dp_dev, e->stream) != 0)
    return fail(SN_ERR_GENERIC, "accumulator min/max init");
  acquire_events(q);
  if (jfn)
    for (size_t ui = 0; ui < q->used_cols.size(); ui++)
      if (((late >> ui) & 1) && q->used_cols[ui] < 63)
        q->late_cols |= 1ll << q->used_cols[ui];
  if (q->ev_start) (void)hipEventRecord(q->ev_start, e->stream);
  rc = -1;
  if (jfn) {
    rc = sn_jit_launch(jfn, d.grid_compiled, (const sn_dev_batch *)set.db_dev,
                       (const sn_dev_tile *)set.tl_dev, ntiles, e->scratch,
                       dp.jkeys, dp.jpayload, dp.jlut,
                       (const sn_dev_plan *)dp_dev, e->stream);
    if (rc == 0)
      rc = sn_launch_reduce(e->scratch, sn_dense_rows(&d, 1), d.nv,
                            q->dev_out, d.naggs1, d.out_stride,
                            dp_dev, e->stream);
    q->used_jit = rc == 0;
    q->direct = rc == 0 && direct;
    if (rc != 0) jfn = nullptr;   /* interpreted kernels take over */
  }
  if (!jfn)
    rc = sn_launch_scan_agg(&dp, (const sn_dev_plan *)dp_dev,
                            (const sn_dev_batch *)set.db_dev,
                            (const sn_dev_tile *)set.tl_dev, ntiles,
                            q->dev_out, e->scratch, e->stream);
  if (q->ev_stop) (void)hipEventRecord(q->ev_stop, e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "kernel launch: %s", hipGetErrorString((hipError_t)rc));
  return SN_OK;
}

/* shared submit body: a short orchestrator over the phases above, in an
 * order that decides which check of a bad plan fails first.  dec == NULL is
 * sn_query_submit; otherwise `plan` carries a double-typed image of the
 * decimal aggregates (so column collection, slot derivation, descriptor
 * build and stats skipping are the double path's own code) and the launch
 * routes to the exact decimal kernels. */
static sn_query *submit_impl(sn_engine *e, const sn_plan *plan,
                             const DecReq *dec) {
  if (!e || !plan) { fail(SN_ERR_BADARG, "null engine/plan"); return nullptr; }
  Table *t = get_table(e, plan->table);
  if (!t) { fail(SN_ERR_BADARG, "unknown table %d", plan->table); return nullptr; }
  if (!e->has_gpu) { fail(SN_ERR_NOGPU, "no HIP device — the engine never falls back to CPU"); return nullptr; }
  /* one submit at a time per engine (shared stream/scratch/workspaces) */
  std::lock_guard<std::mutex> qg(e->query_mu);
  if (plan->npreds > SN_MAX_PREDS || plan->naggs > SN_MAX_AGGS ||
      plan->ngroup > SN_MAX_GROUPS || plan->naggs <= 0) {
    fail(SN_ERR_BADARG, "plan limits exceeded"); return nullptr;
  }

  auto q = std::make_unique<sn_query>();
  q->e = e; q->t = t; q->plan = *plan;
  if (collect_plan_columns(q.get()) != SN_OK) return nullptr;
  if (resolve_join(q.get()) != SN_OK) return nullptr;

  /* ONE t->mu critical section from group-slot derivation through the
   * descriptor build below: a concurrent sn_batch_put (config-5
   * ingest+scan) may grow the global dictionary and append batches; slot
   * capacities, premultiplied dictmaps and the descriptor set must all see
   * the same consistent table state or grouped kernels write accumulator
   * rows out of bounds.  Held to return: the sparse launch synchronizes
   * and reads back under it too. */
  std::lock_guard<std::mutex> g(t->mu);
  sync_pending_stats(e, t);   /* raw-ingested batches: resolve device bounds */

  if (derive_group_slots(q.get(), dec != nullptr) != SN_OK) return nullptr;
  sn_dev_plan dp;
  if (build_dev_plan(q.get(), dec != nullptr, dp) != SN_OK) return nullptr;
  ScanSet set;
  if (resolve_scan_set(q.get(), dp, dec == nullptr, &set) != SN_OK)
    return nullptr;
  /* MIN/MAX plans always take the pac layout (per-agg counts carry the
   * empty-group NULL semantics; routing goes through the op-aware
   * grouped kernels, keyless included) */
  const bool grouped_mode = plan->ngroup > 0 || q->join_group;
  q->pac = (grouped_mode && set.pac) || q->mm;
  dp.pac = q->pac ? 1 : 0;

  int32_t rc = dec         ? launch_decimal(q.get(), dp, set, dec)
               : q->sparse ? launch_sparse(q.get(), dp, set)
                           : launch_dense(q.get(), dp, set);
  if (rc != SN_OK) return nullptr;
  register_live(e, q.get());
  return q.release();
}

extern "C" sn_query *sn_query_submit(sn_engine *e, const sn_plan *plan) {
  return submit_impl(e, plan, nullptr);
}

/* ================================================================== */
/* row-returning filter scan: SELECT cols WHERE preds [LIMIT n]         */

/* ---- ORDER BY on a string key: ranks[gid] = position of value gid among the
 * values sorted by unsigned bytewise comparison (a shorter value sorts before
 * its extensions).  Interned values are distinct, so rank is a bijection. */
static void order_ranks_of(const std::vector<std::pair<const char *, size_t>> &v,
                           int32_t *ranks) {
  std::vector<int32_t> idx(v.size());
  for (size_t i = 0; i < idx.size(); i++) idx[i] = (int32_t)i;
  std::sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {
    const size_t la = v[(size_t)a].second, lb = v[(size_t)b].second;
    const size_t m = std::min(la, lb);
    const int c = m ? memcmp(v[(size_t)a].first, v[(size_t)b].first, m) : 0;
    if (c != 0) return c < 0;
    if (la != lb) return la < lb;
    return a < b;                /* equal values (the exported builder only) */
  });
  for (size_t r = 0; r < idx.size(); r++) ranks[(size_t)idx[r]] = (int32_t)r;
}

/* test aid (not in the public header, like sn_rows_kernel_ms): the rank table
 * of n values, value i = bytes [offsets[i], offsets[i + 1]) */
extern "C" int32_t sn_order_dict_ranks(int32_t n, const uint8_t *bytes,
                                       const int64_t *offsets, int32_t *ranks) {
  if (n < 0 || (n > 0 && (!offsets || !ranks)))
    return fail(SN_ERR_BADARG, "null argument");
  std::vector<std::pair<const char *, size_t>> v((size_t)n);
  for (int32_t i = 0; i < n; i++) {
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i] ||
        (offsets[i + 1] > offsets[i] && !bytes))
      return fail(SN_ERR_BADARG, "bad offsets at value %d", i);
    v[(size_t)i] = { (const char *)bytes + offsets[i],
                     (size_t)(offsets[i + 1] - offsets[i]) };
  }
  order_ranks_of(v, ranks);
  return SN_OK;
}

/* test aid: the device's key image of a non-NULL value, computed on the host.
 * bits: the integer value sign-extended to 64 bits, a DOUBLE's bit pattern, a
 * FLOAT's in the low 32 bits, a STRING's rank, a BOOL as 0/1. */
extern "C" uint64_t sn_order_key_h(int32_t dtype, uint64_t bits, int32_t desc) {
  return sn_order_image(dtype, (long long)bits, (unsigned)bits, desc != 0);
}

/* the table's cached rank table for string column c (caller holds t->mu) */
static const std::vector<int32_t> &table_order_ranks(Table *t, int32_t c) {
  std::vector<int32_t> &r = t->order_ranks[c];
  const std::vector<std::string> &d = t->gdict[(size_t)c];
  if (r.size() != d.size()) {
    std::vector<std::pair<const char *, size_t>> v(d.size());
    for (size_t i = 0; i < d.size(); i++) v[i] = { d[i].data(), d[i].size() };
    r.assign(d.size(), 0);
    order_ranks_of(v, r.data());
  }
  return r;
}

/* ---- the order stage of an ordered scan, after launch_select has read the
 * total and allocated q->sel_rows output rows: radix select, tie quota,
 * sort, ordered gather — all on the stream, bracketed by one event pair ---- */
static int32_t launch_order_stage(sn_query *q, const ScanSet &set,
                                  uint8_t *ord_base, size_t zero_b,
                                  size_t off_b, const uint64_t *bitmap,
                                  const int32_t *counts,
                                  const sn_dev_select &sel,
                                  const int32_t *tb_dev) {
  sn_engine *e = q->e;
  Table *t = q->t;
  const int32_t ntiles = set.ntiles;
  const sn_type_t dt = t->schema[(size_t)q->ord_col].dtype;
  sn_dev_order od;
  memset(&od, 0, sizeof(od));
  od.cslot = q->cslot_of_col[q->ord_col];
  od.dtype = (int32_t)dt;
  od.desc = (q->ord_flags & SN_ORDER_DESC) ? 1 : 0;
  const bool nulls_first = (q->ord_flags & SN_ORDER_NULLS_FIRST) ? true
      : (q->ord_flags & SN_ORDER_NULLS_LAST) ? false : !od.desc;
  od.null_cls = nulls_first ? SN_ORD_CLS_FIRST : SN_ORD_CLS_LAST;
  od.npass = sn_order_passes((int)dt);
  if (dt == SN_TYPE_STRING) {
    const std::vector<int32_t> &r = table_order_ranks(t, q->ord_col);
    od.nranks = (int32_t)r.size();
    if (!r.empty()) {
      od.ranks = (const int32_t *)up_owned(q, r.data(), r.size() * 4);
      if (!od.ranks) return fail(SN_ERR_NOMEM, "rank table upload");
    }
  }
  sn_order_state *state = (sn_order_state *)ord_base;
  unsigned long long *hist = (unsigned long long *)(ord_base + 256);
  int32_t *eq_counts = (int32_t *)(ord_base + 256 +
                                   (size_t)SN_ORD_MAX_PASSES * SN_ORD_HIST * 8);
  int64_t *eq_offsets = (int64_t *)(ord_base + zero_b);
  int64_t *eq_total = (int64_t *)(ord_base + zero_b + off_b);
  sn_order_ent *cand = (sn_order_ent *)(ord_base + zero_b + off_b + 256);
  if (q->sel_ev[4]) (void)hipEventRecord(q->sel_ev[4], e->stream);
  if (hipMemsetAsync(ord_base, 0, zero_b, e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "order state zero");
  int rc = sn_launch_order_select(&od, (const sn_dev_batch *)set.db_dev,
                                  (const sn_dev_tile *)set.tl_dev, ntiles,
                                  bitmap, counts, state, hist, eq_counts,
                                  eq_offsets, eq_total, cand,
                                  (int32_t)q->sel_rows, e->stream);
  if (rc == 0) rc = sn_launch_order_sort(cand, (int32_t)q->sel_rows, e->stream);
  if (rc == 0)
    rc = sn_launch_order_gather(&sel, (const sn_dev_batch *)set.db_dev, cand,
                                tb_dev, e->stream);
  if (q->sel_ev[5]) (void)hipEventRecord(q->sel_ev[5], e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "order stage launch: %s",
                hipGetErrorString((hipError_t)rc));
  q->sel_kernels = 3;
  return SN_OK;
}

/* ---- select launch: mark -> tile offsets -> (host reads the total) ->
 * gather.  dp.nused covers predicate and projection-only columns; pass 1
 * stages the first npc (predicate) slots only.  The caller holds t->mu, so
 * the scan-set -> table batch map sees the batches resolve_scan_set saw. ---- */
static int32_t launch_select(sn_query *q, const sn_dev_plan &dp,
                             const ScanSet &set, int npc) {
  sn_engine *e = q->e;
  const Table *t = q->t;
  const int32_t ntiles = set.ntiles;
  if (ntiles == 0) return SN_OK;
  sn_dev_plan mp = dp;
  mp.nused = npc;
  void *mp_dev = cached_dev_plan(e, mp);
  if (!mp_dev) return fail(SN_ERR_NOMEM, "plan upload");
  /* engine scratch: [total][offsets ntiles][counts ntiles][bitmap], each
   * region 256-byte aligned */
  const size_t off_b = Arena::rnd((size_t)ntiles * 8);
  const size_t cnt_b = Arena::rnd((size_t)ntiles * 4);
  const size_t bm_b = Arena::rnd((size_t)ntiles * SN_SEL_TILE_WORDS * 8);
  /* an ordered scan appends [state + histograms + equal counts] (zeroed by
   * one memset) [equal offsets][equal total][candidates] */
  const size_t ord_zero_b = Arena::rnd(
      256 + (size_t)SN_ORD_MAX_PASSES * SN_ORD_HIST * 8 + (size_t)ntiles * 4);
  const size_t ord_b = !q->ordered ? 0
      : ord_zero_b + off_b + 256 +
        (size_t)SN_ORDER_MAX_LIMIT * sizeof(sn_order_ent);
  int rc = ensure_scratch(e, 256 + off_b + cnt_b + bm_b + ord_b);
  if (rc != SN_OK) return rc;
  uint8_t *base = (uint8_t *)e->scratch;
  uint8_t *ord_base = base + 256 + off_b + cnt_b + bm_b;
  int64_t *total_dev = (int64_t *)base;
  int64_t *offsets = (int64_t *)(base + 256);
  int32_t *counts = (int32_t *)(base + 256 + off_b);
  uint64_t *bitmap = (uint64_t *)(base + 256 + off_b + cnt_b);
  for (hipEvent_t &ev : q->sel_ev) ev = e->ev_acquire();
  if (hipMemsetAsync(counts, 0, (size_t)ntiles * 4, e->stream) != hipSuccess)
    return fail(SN_ERR_GENERIC, "tile count zero");
  if (q->sel_ev[0]) (void)hipEventRecord(q->sel_ev[0], e->stream);
  if (q->rjoin == SN_RJOIN_INNER || q->rjoin == SN_RJOIN_LEFT_ANTI)
    rc = sn_launch_select_mark_join(
        &mp, (const sn_dev_plan *)mp_dev, (const sn_dev_batch *)set.db_dev,
        (const sn_dev_tile *)set.tl_dev, ntiles,
        q->rjoin == SN_RJOIN_INNER ? SN_MARK_INNER : SN_MARK_ANTI, bitmap,
        counts, e->stream);
  else
    rc = sn_launch_select_mark(&mp, (const sn_dev_plan *)mp_dev,
                               (const sn_dev_batch *)set.db_dev,
                               (const sn_dev_tile *)set.tl_dev, ntiles, bitmap,
                               counts, e->stream);
  if (q->sel_ev[1]) (void)hipEventRecord(q->sel_ev[1], e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "select mark launch: %s",
                hipGetErrorString((hipError_t)rc));
  if (q->sel_ev[2]) (void)hipEventRecord(q->sel_ev[2], e->stream);
  rc = sn_launch_tile_offsets(counts, ntiles, offsets, total_dev, e->stream);
  if (q->sel_ev[3]) (void)hipEventRecord(q->sel_ev[3], e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "tile offsets launch: %s",
                hipGetErrorString((hipError_t)rc));
  q->sel_kernels = 2;
  /* the output is sized from the match count: one stream sync inside submit,
   * as on the sparse route */
  int64_t total = 0;
  if (hipStreamSynchronize(e->stream) != hipSuccess ||
      hipMemcpy(&total, total_dev, 8, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(SN_ERR_GENERIC, "select count readback: %s",
                hipGetErrorString(hipGetLastError()));
  q->sel_total = total;
  q->sel_rows = q->sel_limit > 0 ? std::min(total, q->sel_limit) : total;
  if (q->sel_rows <= 0) return SN_OK;

  sn_dev_select sel;
  memset(&sel, 0, sizeof(sel));
  sel.nproj = q->sel_nproj;
  sel.out_rows = q->sel_rows;
  if (q->rjoin >= 0) {
    sel.jcslot = dp.jcslot;
    sel.jis64 = (int32_t)((dp.i64_mask >> dp.jcslot) & 1u);
    sel.jcap_log2 = dp.jcap_log2;
    sel.jkeys = dp.jkeys;
    sel.jpayload = dp.jpayload;
    sel.jlut = dp.jlut;
    sel.jlut_min = dp.jlut_min;
    sel.jlut_max = dp.jlut_max;
  }
  for (int p = 0; p < q->sel_nproj; p++) {
    const int32_t c = q->sel_cols[p];
    sel.otype[p] = c == SN_PROJ_ROWID ? SN_SEL_ROWID
                   : c == SN_PROJ_DIM_ATTR ? SN_SEL_DIM_ATTR
                                           : (int)t->schema[c].dtype;
    sel.cslot[p] = c < 0 ? 0 : q->cslot_of_col[c];
    const size_t vb = (size_t)q->sel_rows * (size_t)q->sel_width[p];
    const size_t nb = (size_t)q->sel_rows;
    q->sel_val[p] = e->arena.alloc(vb);
    if (q->sel_val[p]) q->owned.push_back({ q->sel_val[p], vb });
    q->sel_valid[p] = (uint8_t *)e->arena.alloc(nb);
    if (q->sel_valid[p]) q->owned.push_back({ q->sel_valid[p], nb });
    if (!q->sel_val[p] || !q->sel_valid[p])
      return fail(SN_ERR_NOMEM, "select output alloc (%lld rows)",
                  (long long)q->sel_rows);
    sel.val[p] = q->sel_val[p];
    sel.valid[p] = q->sel_valid[p];
  }
  /* tile.batch indexes the scan set; ROWID names the table's own batch */
  std::vector<int32_t> tb;
  for (size_t bi = 0; bi < t->batches.size(); bi++)
    if (!(q->batches_skipped && batch_skippable(t->batches[bi], &q->plan, t)))
      tb.push_back((int32_t)bi);
  const int32_t *tb_dev = (const int32_t *)up_owned(q, tb.data(), tb.size() * 4);
  if (!tb_dev) return fail(SN_ERR_NOMEM, "batch map upload");
  if (q->ordered)
    return launch_order_stage(q, set, ord_base, ord_zero_b, off_b, bitmap,
                              counts, sel, tb_dev);
  if (q->sel_ev[4]) (void)hipEventRecord(q->sel_ev[4], e->stream);
  rc = sn_launch_select_gather(&sel, (const sn_dev_batch *)set.db_dev,
                               (const sn_dev_tile *)set.tl_dev, ntiles, bitmap,
                               counts, offsets, tb_dev, e->stream);
  if (q->sel_ev[5]) (void)hipEventRecord(q->sel_ev[5], e->stream);
  if (rc != 0)
    return fail(SN_ERR_GENERIC, "select gather launch: %s",
                hipGetErrorString((hipError_t)rc));
  q->sel_kernels = 3;
  return SN_OK;
}

/* ORDER BY request of sn_scan_submit_ordered */
struct OrderReq { int32_t col, flags; };

/* join request of sn_scan_submit_join: an SN_RJOIN_* type */
struct JoinReq { int32_t type; };

/* the join checks of sn_scan_submit_join, in the header's order; *out is the
 * dimension.  Everything here runs without a device. */
static int32_t check_scan_join(sn_engine *e, const Table *t,
                               const sn_plan *plan, const JoinReq *jr,
                               Dim **out) {
  if (jr->type < SN_RJOIN_INNER || jr->type > SN_RJOIN_LEFT_ANTI)
    return fail(SN_ERR_BADARG, "join type %d outside 0..2", jr->type);
  if (plan->join_dim == SN_JOIN_NONE)
    return fail(SN_ERR_BADARG, "sn_scan_submit_join needs plan->join_dim");
  if (plan->join_dim < 0 || plan->join_dim >= (int32_t)e->dims.size())
    return fail(SN_ERR_BADARG, "unknown dimension %d", plan->join_dim);
  if (plan->join_mode != SN_JOIN_SEMI)
    return fail(SN_ERR_BADARG,
                "a row-returning join takes join_mode SN_JOIN_SEMI (the "
                "attribute is a projection, SN_PROJ_DIM_ATTR)");
  Dim *jd = e->dims[plan->join_dim].get();
  {
    std::lock_guard<std::mutex> gd(jd->mu);
    if (jd->keys.empty() && !jd->dev_keys)
      return fail(SN_ERR_BADARG, "empty dimension");
  }
  if (plan->join_fact_col < 0 ||
      plan->join_fact_col >= (int32_t)t->schema.size())
    return fail(SN_ERR_BADARG, "bad join key column %d", plan->join_fact_col);
  const sn_type_t kt = t->schema[plan->join_fact_col].dtype;
  if (kt != SN_TYPE_INT32 && kt != SN_TYPE_INT64)
    return fail(SN_ERR_UNSUPPORTED, "join key must be int32/int64");
  *out = jd;
  return SN_OK;
}

static sn_query *scan_submit_impl(sn_engine *e, const sn_plan *plan,
                                  int32_t nproj, const int32_t *proj_cols,
                                  int64_t limit, const OrderReq *ord,
                                  const JoinReq *jr) {
  if (!e || !plan || !proj_cols) {
    fail(SN_ERR_BADARG, "null engine/plan/projection");
    return nullptr;
  }
  Table *t = get_table(e, plan->table);
  if (!t) { fail(SN_ERR_BADARG, "unknown table %d", plan->table); return nullptr; }
  if (plan->naggs != 0 || plan->ngroup != 0) {
    fail(SN_ERR_BADARG,
         "a row-returning scan takes no aggregates and no group columns");
    return nullptr;
  }
  if (!jr && plan->join_dim != SN_JOIN_NONE) {
    fail(SN_ERR_UNSUPPORTED,
         "sn_scan_submit and sn_scan_submit_ordered take no join "
         "(sn_scan_submit_join does)");
    return nullptr;
  }
  if (plan->npreds < 0 || plan->npreds > SN_MAX_PREDS) {
    fail(SN_ERR_BADARG, "plan limits exceeded");
    return nullptr;
  }
  if (nproj < 1 || nproj > SN_SEL_MAX_PROJ) {
    fail(SN_ERR_BADARG, "nproj %d outside 1..%d", nproj, SN_SEL_MAX_PROJ);
    return nullptr;
  }
  Dim *jd = nullptr;
  if (jr && check_scan_join(e, t, plan, jr, &jd) != SN_OK) return nullptr;
  auto q = std::make_unique<sn_query>();
  q->e = e; q->t = t; q->plan = *plan;
  q->select = true;
  q->sel_nproj = nproj;
  q->sel_limit = limit > 0 ? limit : 0;
  if (jr) q->rjoin = jr->type;
  /* predicate columns take the first device slots, projection-only ones
   * follow: pass 1 stages the former alone */
  if (collect_plan_columns(q.get()) != SN_OK) return nullptr;
  int npc = (int)q->used_cols.size();
  if (jr) {
    /* INNER and LEFT_ANTI probe in pass 1: the key is staged with the
     * predicate columns.  LEFT_OUTER's pass 1 is the plain one; the key is
     * read by pass 2 alone, like a projected column. */
    if (use_col(q.get(), plan->join_fact_col) < 0) {
      fail(SN_ERR_UNSUPPORTED,
           "predicates and join key name more than %d distinct columns",
           SN_DEV_MAX_COLS);
      return nullptr;
    }
    if (jr->type != SN_RJOIN_LEFT_OUTER) npc = (int)q->used_cols.size();
  }
  for (int p = 0; p < nproj; p++) {
    const int32_t c = proj_cols[p];
    q->sel_cols[p] = c;
    if (c == SN_PROJ_ROWID) { q->sel_width[p] = 8; continue; }
    if (jr && c == SN_PROJ_DIM_ATTR) {
      if (jr->type == SN_RJOIN_LEFT_ANTI) {
        fail(SN_ERR_BADARG,
             "a left anti join has no right side to project (SN_PROJ_DIM_ATTR)");
        return nullptr;
      }
      std::lock_guard<std::mutex> gd(jd->mu);
      if (jd->attr_dict.empty()) {
        fail(SN_ERR_BADARG, "dimension %d was loaded without attributes",
             plan->join_dim);
        return nullptr;
      }
      q->sel_width[p] = 4;
      continue;
    }
    if (c < 0 || c >= (int32_t)t->schema.size()) {
      fail(SN_ERR_BADARG, "bad projection column %d", c);
      return nullptr;
    }
    if (use_col(q.get(), c) < 0) {
      fail(SN_ERR_UNSUPPORTED,
           "predicates and projection name more than %d distinct columns",
           SN_DEV_MAX_COLS);
      return nullptr;
    }
    const sn_type_t dt = t->schema[c].dtype;
    q->sel_width[p] = dt == SN_TYPE_STRING ? 4 : sn_type_width(dt);
  }
  if (ord && jr && ord->col == SN_ORDER_NONE) {
    /* sn_scan_submit_join in scan order: sn_scan_submit's limit rules */
    if (ord->flags != 0) {
      fail(SN_ERR_BADARG, "order flags 0x%x without an order column",
           (unsigned)ord->flags);
      return nullptr;
    }
    ord = nullptr;
  }
  if (ord) {
    if (ord->col < 0 || ord->col >= (int32_t)t->schema.size()) {
      fail(SN_ERR_BADARG, "bad order column %d", ord->col);
      return nullptr;
    }
    const int32_t known =
        SN_ORDER_DESC | SN_ORDER_NULLS_FIRST | SN_ORDER_NULLS_LAST;
    if ((ord->flags & ~known) ||
        ((ord->flags & SN_ORDER_NULLS_FIRST) &&
         (ord->flags & SN_ORDER_NULLS_LAST))) {
      fail(SN_ERR_BADARG, "bad order flags 0x%x", (unsigned)ord->flags);
      return nullptr;
    }
    if (limit < 1) {
      fail(SN_ERR_BADARG, "an ordered scan needs a limit of at least 1 "
                          "(no limit would be a full sort)");
      return nullptr;
    }
    if (limit > SN_ORDER_MAX_LIMIT) {
      fail(SN_ERR_UNSUPPORTED, "ordered scan limit %lld beyond %d",
           (long long)limit, SN_ORDER_MAX_LIMIT);
      return nullptr;
    }
    if (use_col(q.get(), ord->col) < 0) {
      fail(SN_ERR_UNSUPPORTED,
           "predicates, projection and order key name more than %d distinct "
           "columns", SN_DEV_MAX_COLS);
      return nullptr;
    }
    q->ordered = true;
    q->ord_col = ord->col;
    q->ord_flags = ord->flags;
  }
  if (!e->has_gpu) {
    fail(SN_ERR_NOGPU, "no HIP device — the engine never falls back to CPU");
    return nullptr;
  }
  std::lock_guard<std::mutex> qg(e->query_mu);
  if (jd) {
    /* as on the aggregate route (resolve_join): the device table is built or
     * reused under the dimension's mutex, inside the engine's one-submit
     * section, before the table's mutex is taken (sn_dim_from_table's order) */
    if (dim_device_table(e, jd) != SN_OK) return nullptr;
    q->join_dim = jd;
  }
  std::lock_guard<std::mutex> g(t->mu);
  sync_pending_stats(e, t);
  sn_dev_plan dp;
  ScanSet set;
  if (build_dev_plan(q.get(), false, dp) != SN_OK ||
      resolve_scan_set(q.get(), dp, true, &set) != SN_OK ||
      launch_select(q.get(), dp, set, npc) != SN_OK) {
    /* a refused output allocation must not strand the blocks already taken
     * (they can be large); nothing may still be reading them */
    (void)hipStreamSynchronize(e->stream);
    for (auto &pr : q->owned) e->arena.release(pr.first, pr.second);
    return nullptr;
  }
  register_live(e, q.get());
  return q.release();
}

extern "C" sn_query *sn_scan_submit(sn_engine *e, const sn_plan *plan,
                                    int32_t nproj, const int32_t *proj_cols,
                                    int64_t limit) {
  return scan_submit_impl(e, plan, nproj, proj_cols, limit, nullptr, nullptr);
}

extern "C" sn_query *sn_scan_submit_ordered(sn_engine *e, const sn_plan *plan,
                                            int32_t nproj,
                                            const int32_t *proj_cols,
                                            int32_t order_col,
                                            int32_t order_flags,
                                            int64_t limit) {
  const OrderReq ord = { order_col, order_flags };
  return scan_submit_impl(e, plan, nproj, proj_cols, limit, &ord, nullptr);
}

extern "C" sn_query *sn_scan_submit_join(sn_engine *e, const sn_plan *plan,
                                         int32_t join_type, int32_t nproj,
                                         const int32_t *proj_cols,
                                         int32_t order_col,
                                         int32_t order_flags, int64_t limit) {
  const JoinReq jr = { join_type };
  const OrderReq ord = { order_col, order_flags };
  return scan_submit_impl(e, plan, nproj, proj_cols, limit, &ord, &jr);
}

extern "C" int32_t sn_dim_num_attrs(sn_engine *e, int32_t dim) {
  if (!e || dim < 0 || dim >= (int32_t)e->dims.size())
    return fail(SN_ERR_BADARG, "bad dim handle");
  Dim *d = e->dims[(size_t)dim].get();
  std::lock_guard<std::mutex> gd(d->mu);
  return (int32_t)d->attr_dict.size();
}

extern "C" int32_t sn_dim_attr_value(sn_engine *e, int32_t dim, int32_t id,
                                     char *buf, int32_t cap) {
  if (!e || dim < 0 || dim >= (int32_t)e->dims.size())
    return fail(SN_ERR_BADARG, "bad dim handle");
  Dim *d = e->dims[(size_t)dim].get();
  std::lock_guard<std::mutex> gd(d->mu);
  if (id < 0 || (size_t)id >= d->attr_dict.size())
    return fail(SN_ERR_BADARG, "attribute id %d out of range", id);
  const std::string &s = d->attr_dict[(size_t)id];
  if (buf) {
    if (cap < 0 || (size_t)cap < s.size())
      return fail(SN_ERR_BADARG, "buffer of %d bytes for a %zu-byte value",
                  cap, s.size());
    memcpy(buf, s.data(), s.size());
    if ((size_t)cap > s.size()) buf[s.size()] = 0;
  }
  return (int32_t)s.size();
}

static sn_query *rows_query(sn_query *q) {
  if (!q) { fail(SN_ERR_BADARG, "null query"); return nullptr; }
  if (!q->select) {
    fail(SN_ERR_BADARG, "not a row-returning query (sn_scan_submit)");
    return nullptr;
  }
  return q;
}

extern "C" int64_t sn_rows_count(sn_query *q) {
  if (!rows_query(q)) return SN_ERR_BADARG;
  int rc = sn_query_wait(q);
  return rc != SN_OK ? rc : q->sel_rows;
}

/* measurement aid (not in the public header, like sn_engine_jit_count): the
 * device intervals of k_select_mark, k_tile_offsets and k_select_gather, 0
 * for a kernel that did not run; sn_query_kernel_ms is their sum.  On an
 * ordered handle the third is the whole order stage (one event pair). */
extern "C" int32_t sn_rows_kernel_ms(sn_query *q, double *ms3) {
  if (!rows_query(q) || !ms3) return SN_ERR_BADARG;
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  for (int i = 0; i < 3; i++) ms3[i] = (double)q->sel_ms[i];
  return SN_OK;
}

extern "C" int32_t sn_rows_fetch(sn_query *q, int32_t proj, int64_t offset,
                                 int64_t n, void *values, uint8_t *valid,
                                 int32_t dst_is_device) {
  if (!rows_query(q)) return SN_ERR_BADARG;
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  if (proj < 0 || proj >= q->sel_nproj)
    return fail(SN_ERR_BADARG, "projection %d out of range", proj);
  if (offset < 0 || n < 0 || offset > q->sel_rows || n > q->sel_rows - offset)
    return fail(SN_ERR_BADARG, "rows [%lld, %lld) outside [0, %lld]",
                (long long)offset, (long long)(offset + n),
                (long long)q->sel_rows);
  if (n == 0) return SN_OK;
  if (!values) return fail(SN_ERR_BADARG, "null values buffer");
  const hipMemcpyKind kind =
      dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t w = (size_t)q->sel_width[proj];
  HIP_OR_FAIL(hipMemcpy(values, (const uint8_t *)q->sel_val[proj] +
                                    (size_t)offset * w, (size_t)n * w, kind));
  if (valid)
    HIP_OR_FAIL(hipMemcpy(valid, q->sel_valid[proj] + offset, (size_t)n, kind));
  return SN_OK;
}

extern "C" int32_t sn_table_dict_value(sn_engine *e, int32_t table,
                                       int32_t col, int32_t gid, char *buf,
                                       int32_t cap) {
  if (!e) return fail(SN_ERR_BADARG, "null engine");
  Table *t = get_table(e, table);
  if (!t) return fail(SN_ERR_BADARG, "unknown table %d", table);
  std::lock_guard<std::mutex> g(t->mu);
  if (col < 0 || col >= (int32_t)t->schema.size() ||
      t->schema[col].dtype != SN_TYPE_STRING)
    return fail(SN_ERR_BADARG, "column %d is not a string column", col);
  if (gid < 0 || (size_t)gid >= t->gdict[col].size())
    return fail(SN_ERR_BADARG, "dictionary id %d out of range", gid);
  const std::string &s = t->gdict[col][(size_t)gid];
  if (buf) {
    if (cap < 0 || (size_t)cap < s.size())
      return fail(SN_ERR_BADARG, "buffer of %d bytes for a %zu-byte value",
                  cap, s.size());
    memcpy(buf, s.data(), s.size());
    if ((size_t)cap > s.size()) buf[s.size()] = 0;
  }
  return (int32_t)s.size();
}

extern "C" int32_t sn_table_batch_id(sn_engine *e, int32_t table,
                                     int32_t batch, int64_t *uuid,
                                     int32_t *bucket) {
  if (!e || !uuid || !bucket) return fail(SN_ERR_BADARG, "null argument");
  Table *t = get_table(e, table);
  if (!t) return fail(SN_ERR_BADARG, "unknown table %d", table);
  std::lock_guard<std::mutex> g(t->mu);
  if (batch < 0 || (size_t)batch >= t->batches.size())
    return fail(SN_ERR_BADARG, "batch %d out of range", batch);
  *uuid = t->batches[(size_t)batch].uuid;
  *bucket = t->batches[(size_t)batch].bucket;
  return SN_OK;
}

/* ================================================================== */
/* exact DECIMAL aggregation: host side                                */

typedef unsigned __int128 u128_t;
typedef __int128 i128_t;
static const u128_t DEC_1E38 =
    ((u128_t)0x4B3B4CA85A86C47Aull << 64) | 0x098A224000000000ull;

static sn_dec_val dec_null(int32_t scale) {
  sn_dec_val v;
  memset(&v, 0, sizeof(v));
  v.scale = scale;
  v.is_null = 1;
  return v;
}
static sn_dec_val dec_make(i128_t x, int32_t scale) {
  sn_dec_val v;
  memset(&v, 0, sizeof(v));
  v.lo = (uint64_t)(u128_t)x;
  v.hi = (int64_t)(x >> 64);
  v.scale = scale;
  return v;
}
static i128_t dec_i128(const sn_dec_val &v) {
  return (i128_t)(((u128_t)(uint64_t)v.hi << 64) | v.lo);
}
static double dec_to_double(const sn_dec_val &v) {
  return (double)((long double)dec_i128(v) / powl(10.0L, (long double)v.scale));
}

extern "C" int32_t sn_dec_to_string(const sn_dec_val *v, char *buf,
                                    int32_t cap) {
  if (!v || !buf || cap <= 0 || v->scale < 0 || v->scale > 76)
    return fail(SN_ERR_BADARG, "bad decimal/buffer");
  std::string s;
  if (v->is_null) {
    s = "NULL";
  } else {
    const i128_t x = dec_i128(*v);
    u128_t m = x < 0 ? (u128_t)0 - (u128_t)x : (u128_t)x;
    std::string digits;
    do {
      digits.push_back((char)('0' + (int)(m % 10)));
      m /= 10;
    } while (m != 0);
    while ((int32_t)digits.size() < v->scale + 1) digits.push_back('0');
    std::reverse(digits.begin(), digits.end());
    if (x < 0) s.push_back('-');
    s.append(digits, 0, digits.size() - (size_t)v->scale);
    if (v->scale > 0) {
      s.push_back('.');
      s.append(digits, digits.size() - (size_t)v->scale, (size_t)v->scale);
    }
  }
  if ((int32_t)s.size() + 1 > cap)
    return fail(SN_ERR_BADARG, "decimal string needs %zu bytes", s.size() + 1);
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int32_t)s.size();
}

/* Average's result expression: sum / count at scale+4, HALF_UP (Spark:
 * avg(decimal(p,s)) -> decimal(p+4,s+4)).  |sum| * 10^4 needs up to ~140
 * bits: three 64-bit limbs long-divided by the 64-bit count. */
extern "C" int32_t sn_dec_avg(const sn_dec_val *sum, int64_t count,
                              sn_dec_val *out) {
  if (!sum || !out) return fail(SN_ERR_BADARG, "null decimal");
  const int32_t scale = sum->scale + 4;
  if (sum->is_null || count <= 0) { *out = dec_null(scale); return SN_OK; }
  const i128_t x = dec_i128(*sum);
  const bool neg = x < 0;
  const u128_t m = neg ? (u128_t)0 - (u128_t)x : (u128_t)x;
  const u128_t lo = (u128_t)(uint64_t)m * 10000u;
  const u128_t hi = (u128_t)(uint64_t)(m >> 64) * 10000u + (lo >> 64);
  const uint64_t limb[3] = { (uint64_t)lo, (uint64_t)hi, (uint64_t)(hi >> 64) };
  const uint64_t d = (uint64_t)count;
  uint64_t qd[3];
  uint64_t rem = 0;
  for (int i = 2; i >= 0; i--) {
    const u128_t cur = ((u128_t)rem << 64) | limb[i];
    qd[i] = (uint64_t)(cur / d);
    rem = (uint64_t)(cur % d);
  }
  u128_t qv = ((u128_t)qd[1] << 64) | qd[0];
  bool over = qd[2] != 0;
  if ((u128_t)rem * 2 >= (u128_t)d) {      /* HALF_UP on the magnitude */
    qv += 1;
    if (qv == 0) over = true;
  }
  if (over || qv >= DEC_1E38) { *out = dec_null(scale); return SN_OK; }
  *out = dec_make(neg ? -(i128_t)qv : (i128_t)qv, scale);
  return SN_OK;
}

extern "C" int32_t sn_table_set_decimal(sn_engine *e, int32_t table,
                                        int32_t col, int32_t precision,
                                        int32_t scale) {
  if (!e) return fail(SN_ERR_BADARG, "null engine");
  Table *t = get_table(e, table);
  if (!t) return fail(SN_ERR_BADARG, "unknown table %d", table);
  std::lock_guard<std::mutex> g(t->mu);
  if (col < 0 || col >= (int32_t)t->schema.size())
    return fail(SN_ERR_BADARG, "bad column %d", col);
  if (t->schema[col].dtype != SN_TYPE_INT64)
    return fail(SN_ERR_BADARG,
                "decimal column %d must be INT64 (unscaled long decimal)", col);
  if (precision < 1 || precision > 18)
    return fail(SN_ERR_BADARG,
                "decimal precision %d outside 1..18 (long-decimal range)",
                precision);
  if (scale < 0 || scale > precision)
    return fail(SN_ERR_BADARG, "decimal scale %d outside 0..precision %d",
                scale, precision);
  t->dec_prec.resize(t->schema.size(), 0);
  t->dec_scale.resize(t->schema.size(), 0);
  t->dec_prec[col] = (int8_t)precision;
  t->dec_scale[col] = (int8_t)scale;
  return SN_OK;
}

extern "C" sn_query *sn_query_submit_dec(sn_engine *e, const sn_plan *plan,
                                         int32_t naggs,
                                         const sn_dec_agg *aggs) {
  if (!e || !plan || !aggs) { fail(SN_ERR_BADARG, "null engine/plan/aggs"); return nullptr; }
  Table *t = get_table(e, plan->table);
  if (!t) { fail(SN_ERR_BADARG, "unknown table %d", plan->table); return nullptr; }
  if (naggs <= 0 || naggs > SN_MAX_AGGS) {
    fail(SN_ERR_BADARG, "decimal naggs %d outside 1..%d", naggs, SN_MAX_AGGS);
    return nullptr;
  }
  if (plan->naggs != 0) {
    fail(SN_ERR_BADARG,
         "decimal submit takes its aggregates separately: plan->naggs must be 0");
    return nullptr;
  }
  if (plan->join_dim != SN_JOIN_NONE) {
    fail(SN_ERR_UNSUPPORTED, "decimal aggregation over a join is not supported");
    return nullptr;
  }
  sn_plan sp = *plan;
  sp.naggs = naggs;
  int scales[SN_MAX_AGGS];
  {
    std::lock_guard<std::mutex> g(t->mu);
    static const int64_t P10[19] = {
      1ll, 10ll, 100ll, 1000ll, 10000ll, 100000ll, 1000000ll, 10000000ll,
      100000000ll, 1000000000ll, 10000000000ll, 100000000000ll,
      1000000000000ll, 10000000000000ll, 100000000000000ll,
      1000000000000000ll, 10000000000000000ll, 100000000000000000ll,
      1000000000000000000ll };
    for (int a = 0; a < naggs; a++) {
      const sn_dec_agg &sa = aggs[a];
      sn_agg &da = sp.aggs[a];
      memset(&da, 0, sizeof(da));
      da.kind = sa.kind;
      scales[a] = 0;
      if (sa.kind == SN_AGG_COUNT_STAR) continue;
      const bool mm = sa.kind == SN_AGG_MIN || sa.kind == SN_AGG_MAX;
      if (sa.kind != SN_AGG_SUM && sa.kind != SN_AGG_AVG && !mm) {
        fail(SN_ERR_BADARG, "decimal aggregate %d: unknown kind %d", a, sa.kind);
        return nullptr;
      }
      if (sa.nfactors < 1 || sa.nfactors > SN_MAX_FACTORS ||
          (mm && sa.nfactors != 1)) {
        fail(SN_ERR_BADARG,
             "decimal aggregate %d: %d factors (SUM/AVG take 1..%d, MIN/MAX "
             "exactly 1)", a, sa.nfactors, SN_MAX_FACTORS);
        return nullptr;
      }
      da.nfactors = sa.nfactors;
      for (int f = 0; f < sa.nfactors; f++) {
        const sn_dec_factor &fa = sa.factors[f];
        if (fa.col < 0 || fa.col >= (int32_t)t->schema.size()) {
          fail(SN_ERR_BADARG, "decimal aggregate %d: bad column %d", a, fa.col);
          return nullptr;
        }
        const int prec = (size_t)fa.col < t->dec_prec.size()
                             ? t->dec_prec[fa.col] : 0;
        if (prec <= 0) {
          fail(SN_ERR_BADARG,
               "decimal aggregate %d: column %d is not declared decimal "
               "(sn_table_set_decimal)", a, fa.col);
          return nullptr;
        }
        /* factor values are formed in int64 on the device: prove
         * |add| + |mul| * 10^precision cannot exceed it */
        const i128_t aa = fa.add < 0 ? -(i128_t)fa.add : (i128_t)fa.add;
        const i128_t am = fa.mul < 0 ? -(i128_t)fa.mul : (i128_t)fa.mul;
        if (aa + am * (i128_t)P10[prec] > (i128_t)INT64_MAX) {
          fail(SN_ERR_UNSUPPORTED,
               "decimal aggregate %d factor %d: |add| + |mul| * 10^%d can "
               "exceed int64", a, f, prec);
          return nullptr;
        }
        scales[a] += t->dec_scale[fa.col];
        da.factors[f].col = fa.col;
        da.factors[f].add = (double)fa.add;
        da.factors[f].mul = (double)fa.mul;
      }
      if (sa.kind == SN_AGG_AVG) scales[a] += 4;
    }
  }
  DecReq req = { naggs, aggs };
  sn_query *q = submit_impl(e, &sp, &req);
  if (q) memcpy(q->dec_scale_of, scales, sizeof(int) * (size_t)naggs);
  return q;
}

/* cells -> exact values (+ the double view sn_query_result reads) */
static void dec_finalize(sn_query *q, const unsigned long long *cells) {
  const sn_plan &p = q->plan;
  const int nd = q->dec_ndev;
  const size_t RC = (size_t)sn_dec_row_cells(nd);
  q->dec_vals.assign((size_t)q->nslots * p.naggs, dec_null(0));
  q->host_out.assign((size_t)q->nslots * q->out_stride, 0.0);
  for (int s = 0; s < q->nslots; s++) {
    const unsigned long long *row = cells ? cells + (size_t)s * RC : nullptr;
    const unsigned long long rowcount = row ? row[RC - 1] : 0;
    double *hrow = &q->host_out[(size_t)s * q->out_stride];
    hrow[2 * p.naggs] = (double)rowcount;
    for (int a = 0; a < p.naggs; a++) {
      const int kind = p.aggs[a].kind;
      const int scale = q->dec_scale_of[a];
      sn_dec_val v = dec_null(scale);
      unsigned long long cnt = 0;
      if (kind == SN_AGG_COUNT_STAR) {
        v = dec_make((i128_t)rowcount, 0);
        cnt = rowcount;
      } else if (row) {
        const unsigned long long *c = row + (size_t)q->dec_map[a] * SN_DEC_CELLS;
        cnt = c[3];
        if (cnt > 0 && (kind == SN_AGG_MIN || kind == SN_AGG_MAX)) {
          v = dec_make((i128_t)(int64_t)(c[0] ^ 0x8000000000000000ull), scale);
        } else if (cnt > 0 && c[4] == 0) {
          /* the 192-bit sum must fit i128 and stay below 10^38 */
          const bool neg = (c[1] >> 63) != 0;
          const bool fits = c[2] == (neg ? ~0ull : 0ull);
          const i128_t x = (i128_t)(((u128_t)c[1] << 64) | c[0]);
          const u128_t m = neg ? (u128_t)0 - (u128_t)x : (u128_t)x;
          if (fits && m < DEC_1E38) {
            const int sum_scale = kind == SN_AGG_AVG ? scale - 4 : scale;
            v = dec_make(x, sum_scale);
            if (kind == SN_AGG_AVG) {
              sn_dec_val av;
              (void)sn_dec_avg(&v, (int64_t)cnt, &av);
              v = av;
            }
          }
        }
      }
      q->dec_vals[(size_t)s * p.naggs + a] = v;
      /* double view: result_fill_page divides AVG sums by counts, so a
       * finished average travels as (value, 1); NULL as count 0 */
      if (kind == SN_AGG_COUNT_STAR) {
        hrow[a] = (double)rowcount;
        hrow[p.naggs + a] = (double)rowcount;
      } else if (!v.is_null) {
        hrow[a] = dec_to_double(v);
        hrow[p.naggs + a] = kind == SN_AGG_AVG ? 1.0 : (double)cnt;
      }
    }
  }
}

/* ================================================================== */
/* read-back: everything below runs after the stream has synchronised  */

/* The handle kinds an entry point does not serve.  Every caller checks its
 * arguments first, then this, then sn_query_wait. */
enum { REFUSE_ROWS = 1, REFUSE_DEC = 2 };
static int32_t refuse_kind(const sn_query *q, const char *fn, int kinds) {
  if ((kinds & REFUSE_ROWS) && q->select)
    return fail(SN_ERR_UNSUPPORTED,
                "%s is not supported on a row-returning query (its result is "
                "rows, read with sn_rows_fetch)", fn);
  if ((kinds & REFUSE_DEC) && q->dec)
    return fail(SN_ERR_UNSUPPORTED,
                "%s is not supported on an exact decimal query (its state is "
                "128-bit fixed point, not the f64 partial layout)", fn);
  return SN_OK;
}
#define REFUSE_KIND(q, kinds)                                   \
  do {                                                          \
    int32_t rk_ = refuse_kind((q), __func__, (kinds));          \
    if (rk_ != SN_OK) return rk_;                               \
  } while (0)

extern "C" int32_t sn_query_result_dec(sn_query *q, int64_t row, int32_t agg,
                                       sn_dec_val *out) {
  if (!q || !out) return fail(SN_ERR_BADARG, "null query/out");
  REFUSE_KIND(q, REFUSE_ROWS);
  if (!q->dec) return fail(SN_ERR_BADARG, "not a decimal query");
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  const int64_t n = sn_query_num_groups(q);
  if (n < 0) return (int32_t)n;
  if (row < 0 || row >= n || agg < 0 || agg >= q->plan.naggs)
    return fail(SN_ERR_BADARG, "row/agg out of range");
  const GroupOut &g = q->final_groups[(size_t)row];
  *out = q->dec_vals[(size_t)g.slot * q->plan.naggs + agg];
  return SN_OK;
}

/* the rows stay on the device (sn_rows_fetch); the duration is the sum of
 * the three kernels' own intervals, without the host readback gap */
static int32_t wait_select(sn_query *q) {
  float sum = 0.0f;
  bool any = false;
  for (int i = 0; i < 2 * q->sel_kernels; i += 2) {
    float ms = 0.0f;
    if (q->sel_ev[i] && q->sel_ev[i + 1] &&
        hipEventElapsedTime(&ms, q->sel_ev[i], q->sel_ev[i + 1]) == hipSuccess) {
      q->sel_ms[i / 2] = ms;
      sum += ms;
      any = true;
    }
  }
  if (any) q->kernel_ms = sum;
  return SN_OK;
}

static int32_t wait_decimal(sn_query *q) {
  std::vector<unsigned long long> cells;
  if (q->dec_out) {
    cells.resize((size_t)q->nslots * sn_dec_row_cells(q->dec_ndev));
    HIP_OR_FAIL(hipMemcpy(cells.data(), q->dec_out, cells.size() * 8,
                          hipMemcpyDeviceToHost));
  }
  dec_finalize(q, q->dec_out ? cells.data() : nullptr);
  return SN_OK;
}

static int32_t wait_f64(sn_query *q) {
  size_t out_n = (size_t)q->nslots * q->out_stride;
  q->host_out.resize(out_n);
  if (out_n > 0 && q->dev_out)
    HIP_OR_FAIL(hipMemcpy(q->host_out.data(), q->dev_out, out_n * 8,
                          hipMemcpyDeviceToHost));
  return SN_OK;
}

extern "C" int32_t sn_query_wait(sn_query *q) {
  if (!q) return SN_ERR_BADARG;
  if (q->done) return SN_OK;
  HIP_OR_FAIL(hipStreamSynchronize(q->e->stream));
  int32_t rc = q->select ? wait_select(q)
               : q->dec  ? wait_decimal(q) : wait_f64(q);
  if (rc != SN_OK) return rc;
  /* an aggregate scan is bracketed by one event pair; a row scan has none */
  if (q->ev_start && q->ev_stop)
    (void)hipEventElapsedTime(&q->kernel_ms, q->ev_start, q->ev_stop);
  q->done = true;
  return SN_OK;
}

/* scan-kernel duration in ms (HIP events on the launch stream); -1 if the
 * query launched nothing */
extern "C" double sn_query_kernel_ms(sn_query *q) {
  if (!q) return -1.0;
  (void)sn_query_wait(q);
  return (double)q->kernel_ms;
}

/* 1 when the query ran a query-compiled (hipRTC) kernel, 0 interpreted */
extern "C" int32_t sn_query_used_jit(sn_query *q) {
  return q && q->used_jit ? 1 : 0;
}

/* bit c set: the compiled kernel of this query read table column c late,
 * for the passing rows only (columns 0..62; 0 when none, or interpreted) */
extern "C" int64_t sn_query_late_cols(sn_query *q) {
  return q && q->used_jit ? q->late_cols : 0;
}

extern "C" int32_t sn_query_direct(sn_query *q) {
  return q && q->used_jit ? q->direct : 0;
}

/* number of compiled kernels in this engine's JIT cache (tokenized plan
 * shapes — different literal values share one entry) */
extern "C" int32_t sn_engine_jit_count(sn_engine *e) {
  return e ? sn_jit_cache_count(e->jit) : 0;
}

/* group-key columns of the result: a dimension-attribute group leads them */
static int eff_ngroup(const sn_query *q) {
  return q->join_group ? 1 + q->plan.ngroup : q->plan.ngroup;
}

/* how this query's accumulator rows read (partial_format.h) */
static AccRowLayout row_layout(const sn_query *q) {
  const sn_plan &p = q->plan;
  AccRowLayout L;
  L.form = q->sparse ? SN_ROW_SPARSE
           : eff_ngroup(q) == 0 ? SN_ROW_KEYLESS : SN_ROW_DENSE;
  L.naggs = p.naggs; L.na_t = q->na_t; L.dev_naggs = q->dev_naggs;
  L.pac = q->pac;
  for (int a = 0; a < SN_MAX_AGGS; a++) {
    L.agg_map[a] = q->agg_map[a];
    L.kinds[a] = p.aggs[a].kind;
  }
  L.rowcount_at = acc_rowcount_at(L.form, L.na_t, L.dev_naggs, L.pac);
  return L;
}

/* hash-aggregate results: compacted (key, accumulator-row) pairs.  Keys
 * surface as decimal text like the dense integer-key path (the partial-block
 * and result formats stay shared). */
static void sparse_groups(sn_query *q, const AccRowLayout &L,
                          std::vector<GroupOut> *out) {
  const size_t width = (size_t)L.rowcount_at + 1;
  const bool packed = q->plan.ngroup == 2;
  for (size_t i = 0; i < q->sparse_n; i++) {
    const double *row = &q->sparse_rows[i * width];
    if (!acc_row_occupied(L, row)) continue;
    GroupOut g;
    acc_row_decode(L, row, &g);
    long long key = q->sparse_keys[i];
    if (packed) {
      g.keys[0] = std::to_string((int32_t)((unsigned long long)key >> 32));
      g.keys[1] = std::to_string((int32_t)(unsigned)key);
    } else {
      g.keys[0] = std::to_string(key);
    }
    out->push_back(std::move(g));
  }
  if (!q->sparse_null_row.empty() &&
      acc_row_occupied(L, q->sparse_null_row.data())) {
    GroupOut g;
    acc_row_decode(L, q->sparse_null_row.data(), &g);
    g.key_null[0] = true;               /* the NULL-key group */
    out->push_back(std::move(g));
  }
}

/* key `at` of g from index i of the dense slot space of group column gc: an
 * integer key counts up from its minimum, the null slot is NULL, anything
 * else is a dictionary entry.  The caller holds t->mu. */
static void dense_key(const sn_query *q, int gc, int i, GroupOut *g, int at) {
  if (q->gint[gc]) g->keys[at] = std::to_string(q->gmin[gc] + i);
  else if (i == (gc == 0 ? q->gnull1 : q->gnull2)) g->key_null[at] = true;
  else g->keys[at] = q->t->gdict[q->plan.group_cols[gc]][i];
}

static void dense_groups(sn_query *q, const AccRowLayout &L,
                         std::vector<GroupOut> *out) {
  const sn_plan &p = q->plan;
  const bool keyless = L.form == SN_ROW_KEYLESS;
  /* concurrent ingest may be interning new dictionary entries; group ids
   * recorded at submit stay valid (dictionaries only grow) but the vector
   * needs the lock for stability */
  std::lock_guard<std::mutex> gt(q->t->mu);
  std::unique_lock<std::mutex> gd;
  if (q->join_group) gd = std::unique_lock<std::mutex>(q->join_dim->mu);
  for (int s = 0; s < q->nslots; s++) {
    const double *row = &q->host_out[(size_t)s * q->out_stride];
    if (!keyless && !acc_row_occupied(L, row)) continue;
    GroupOut g;
    g.slot = s;
    acc_row_decode(L, row, &g);
    if (q->join_group && p.ngroup >= 1) {
      /* composite: attr-major, fact minor */
      g.keys[0] = q->join_dim->attr_dict[s / q->fact_slots];
      dense_key(q, 0, s % q->fact_slots, &g, 1);
    } else if (q->join_group) {
      g.keys[0] = q->join_dim->attr_dict[s];
    } else if (p.ngroup >= 1) {
      dense_key(q, 0, s / q->g2cap, &g, 0);
      if (p.ngroup == 2) dense_key(q, 1, s % q->g2cap, &g, 1);
    }
    out->push_back(std::move(g));
  }
  if (keyless && out->empty()) out->push_back(GroupOut());
}

/* local accumulators -> GroupOut list (pre-merge view) */
static void local_groups(sn_query *q, std::vector<GroupOut> *out) {
  const AccRowLayout L = row_layout(q);
  if (q->sparse) sparse_groups(q, L, out);
  else dense_groups(q, L, out);
}

static void finalize_groups(sn_query *q, std::vector<GroupOut> &&groups) {
  std::sort(groups.begin(), groups.end(), GroupKeyLess());
  q->final_groups = std::move(groups);
}

/* the result rows, unless a merge or an earlier call already left them */
static bool final_groups_ready(const sn_query *q) {
  return !q->final_groups.empty() || q->merged;
}
static void ensure_final_groups(sn_query *q) {
  if (final_groups_ready(q)) return;
  std::vector<GroupOut> groups;
  local_groups(q, &groups);
  finalize_groups(q, std::move(groups));
}

static int32_t result_fill_page(sn_query *q, int64_t offset, sn_result *out) {
  if (!q || !out || offset < 0) return SN_ERR_BADARG;
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  ensure_final_groups(q);
  memset(out, 0, sizeof(*out));
  const sn_plan &p = q->plan;
  out->ngroup = eff_ngroup(q);
  out->naggs = p.naggs;
  int64_t total = (int64_t)q->final_groups.size();
  int64_t start = offset < total ? offset : total;
  out->nrows = (int32_t)std::min((int64_t)SN_MAX_GROUP_SLOTS, total - start);
  out->rows_scanned = q->rows_scanned;
  out->batches_seen = q->batches_seen;
  out->batches_skipped = q->batches_skipped;
  for (int32_t i = 0; i < out->nrows; i++) {
    GroupOut &g = q->final_groups[(size_t)(start + i)];
    for (int k = 0; k < out->ngroup; k++) {
      group_key_put(out->keys[i][k], g.keys[k]);
      out->key_is_null[i][k] = g.key_null[k] ? 1 : 0;
    }
    for (int a = 0; a < p.naggs; a++)
      if (!group_value(g, a, p.aggs[a].kind, &out->vals[i][a]))
        out->val_is_null[i][a] = 1;
    out->rows_passed += (int64_t)g.rowcount;
  }
  return SN_OK;
}

extern "C" int32_t sn_query_result(sn_query *q, sn_result *out) {
  if (q && q->select) {
    /* no group rows: the metrics alone (the rows come from sn_rows_fetch) */
    if (!out) return SN_ERR_BADARG;
    int rc = sn_query_wait(q);
    if (rc != SN_OK) return rc;
    memset(out, 0, sizeof(*out));
    out->rows_scanned = q->rows_scanned;
    out->rows_passed = q->sel_total;
    out->batches_seen = q->batches_seen;
    out->batches_skipped = q->batches_skipped;
    return SN_OK;
  }
  return result_fill_page(q, 0, out);
}

/* result paging for group counts beyond SN_MAX_GROUP_SLOTS (the
 * global-atomic grouped path): fills up to one page from `offset`. */
extern "C" int32_t sn_query_result_page(sn_query *q, int64_t offset,
                                        sn_result *out) {
  if (!q) return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS);
  return result_fill_page(q, offset, out);
}

/* ORDER BY <aggregate value> [DESC] LIMIT k epilogue — the SnappySortExec /
 * TakeOrderedAndProject analogue over the finalized group rows.  The sort
 * key is the RESULT value of aggregate agg_idx (AVG divides, COUNT(*)
 * counts, NULL groups order last); ties keep the key ordering (stable). */
extern "C" int32_t sn_query_order_by(sn_query *q, int32_t agg_idx,
                                     int32_t descending, int64_t k) {
  if (!q) return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS | REFUSE_DEC);
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  ensure_final_groups(q);
  const sn_plan &p = q->plan;
  if (agg_idx >= p.naggs) return fail(SN_ERR_BADARG, "agg_idx out of range");
  if (agg_idx >= 0)
    std::stable_sort(q->final_groups.begin(), q->final_groups.end(),
                     GroupValueLess{ agg_idx, p.aggs[agg_idx].kind,
                                     descending != 0 });
  else                                                /* restore key order */
    std::sort(q->final_groups.begin(), q->final_groups.end(), GroupKeyLess());
  if (k > 0 && (int64_t)q->final_groups.size() > k)
    q->final_groups.resize((size_t)k);
  return SN_OK;
}

/* total group rows of the finalized result */
extern "C" int64_t sn_query_num_groups(sn_query *q) {
  if (!q) return SN_ERR_BADARG;
  if (q->select) return 0;
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  if (q->sparse && !final_groups_ready(q)) {
    /* count without materializing ~1M string-keyed GroupOuts — the
     * multi-GPU capacity negotiation calls this every step (550 ms vs
     * ~2 ms at 1M groups) */
    const AccRowLayout L = row_layout(q);
    const size_t width = (size_t)L.rowcount_at + 1;
    int64_t n = 0;
    for (size_t i = 0; i < q->sparse_n; i++)
      n += acc_row_occupied(L, &q->sparse_rows[i * width]);
    if (!q->sparse_null_row.empty())
      n += acc_row_occupied(L, q->sparse_null_row.data());
    return n;
  }
  ensure_final_groups(q);
  return (int64_t)q->final_groups.size();
}

static void sn_detach_queries(sn_engine *e) {
  std::lock_guard<std::mutex> g(e->aux_mu);
  for (sn_query *q : e->live_q) q->e = nullptr;
  e->live_q.clear();
}

extern "C" void sn_query_destroy(sn_query *q) {
  if (q && q->e) {
    /* the stream may still reference this query's buffers */
    (void)sn_query_wait(q);
    for (auto &pr : q->owned) q->e->arena.release(pr.first, pr.second);
    std::lock_guard<std::mutex> g(q->e->aux_mu);
    q->e->live_q.erase(q);
  }
  delete q;
}

/* ---- partial exchange (block format: partial_format.h) ----
 * Grouped blocks carry a caller-chosen slot CAPACITY (the *2 entry points):
 * group counts beyond SN_MAX_GROUP_SLOTS — the big dense-slot and sparse
 * hash-aggregate paths — export by negotiating a capacity across ranks
 * (e.g. allreduce-MAX of sn_query_num_groups) before the collective.  The
 * legacy entry points keep the fixed SN_MAX_GROUP_SLOTS capacity. */
static int64_t partial_bytes_cap(const sn_query *q, int32_t cap) {
  return eff_ngroup(q) == 0 ? partial_keyless_bytes(q->plan.naggs)
                            : partial_grouped_bytes(cap);
}

extern "C" int64_t sn_query_partial_bytes2(sn_query *q, int32_t cap_slots) {
  if (!q || cap_slots <= 0) return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS | REFUSE_DEC);
  return partial_bytes_cap(q, cap_slots);
}

extern "C" int64_t sn_query_partial_bytes(sn_query *q) {
  return sn_query_partial_bytes2(q, SN_MAX_GROUP_SLOTS);
}

extern "C" int32_t sn_query_partials2(sn_query *q, void *dst,
                                      int32_t dst_is_device, int32_t cap_slots) {
  if (!q || !dst || cap_slots <= 0) return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS | REFUSE_DEC);
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  std::vector<GroupOut> groups;
  local_groups(q, &groups);
  std::vector<uint8_t> block((size_t)partial_bytes_cap(q, cap_slots), 0);
  if (eff_ngroup(q) == 0) {
    partial_write_keyless(block.data(), groups[0], q->plan.naggs);
  } else {
    if (groups.size() > (size_t)cap_slots)
      return fail(SN_ERR_OVERFLOW,
                  "%zu groups exceed the partial-block capacity %d "
                  "(negotiate a larger capacity via sn_query_partial_bytes2)",
                  groups.size(), cap_slots);
    const int32_t n = (int32_t)groups.size();
    partial_write_header(block.data(), n, cap_slots);
    for (int32_t i = 0; i < n; i++)
      partial_write_slot(block.data(), i, groups[(size_t)i]);
  }
  if (dst_is_device) {
    HIP_OR_FAIL(hipMemcpy(dst, block.data(), block.size(), hipMemcpyHostToDevice));
  } else {
    memcpy(dst, block.data(), block.size());
  }
  return SN_OK;
}

extern "C" int32_t sn_query_partials(sn_query *q, void *dst, int32_t dst_is_device) {
  return sn_query_partials2(q, dst, dst_is_device, SN_MAX_GROUP_SLOTS);
}

/* Split this shard's grouped partials into `world` same-format blocks by
 * key-hash shard — the key-sharded all-to-all of SURVEY §8(e): rank r keeps
 * only keys hashing to shard r; every other key's partial travels to its
 * owner (the reference's partial->final ShuffleExchange with hash
 * partitioning, SnappyStrategies.scala:560-601).  dst must hold
 * world * sn_query_partial_bytes(q) bytes; block d goes to rank d. */
extern "C" int32_t sn_query_partials_sharded2(sn_query *q, int32_t world,
                                              void *dst, int32_t cap_slots) {
  if (!q || !dst || world <= 0 || world > 1024 || cap_slots <= 0)
    return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS | REFUSE_DEC);
  const int ng = eff_ngroup(q);
  if (ng == 0) return SN_ERR_UNSUPPORTED;
  int rc = sn_query_wait(q);
  if (rc != SN_OK) return rc;
  const int64_t bb = partial_bytes_cap(q, cap_slots);
  memset(dst, 0, (size_t)bb * world);
  std::vector<GroupOut> groups;
  local_groups(q, &groups);
  std::vector<int32_t> counts(world, 0);
  for (const GroupOut &g : groups) {
    const int d = partial_shard_of(g, ng, world);
    if (counts[d] >= cap_slots)
      return fail(SN_ERR_OVERFLOW,
                  "shard %d exceeds the partial-block capacity %d", d, cap_slots);
    partial_write_slot((uint8_t *)dst + (int64_t)d * bb, counts[d]++, g);
  }
  for (int d = 0; d < world; d++)
    partial_write_header((uint8_t *)dst + (int64_t)d * bb, counts[d], cap_slots);
  return SN_OK;
}

extern "C" int32_t sn_query_partials_sharded(sn_query *q, int32_t world,
                                             void *dst) {
  return sn_query_partials_sharded2(q, world, dst, SN_MAX_GROUP_SLOTS);
}

/* The blocks come from other ranks: all of them are checked against `stride`
 * before the first is folded, and a refusal leaves the query as it was. */
extern "C" int32_t sn_query_merge(sn_query *q, const void *blocks, int64_t stride,
                                  int32_t n_blocks) {
  if (!q || !blocks || n_blocks <= 0) return SN_ERR_BADARG;
  REFUSE_KIND(q, REFUSE_ROWS | REFUSE_DEC);
  const AccRowLayout L = row_layout(q);
  std::vector<GroupOut> merged;
  int32_t bad = 0;
  const int why = partial_merge(blocks, stride, n_blocks, eff_ngroup(q),
                                L.naggs, L.kinds, &merged, &bad);
  if (why != SN_PARTIAL_OK)
    return fail(SN_ERR_BADARG,
                "sn_query_merge: partial block %d of %d (stride %lld): %s",
                bad, n_blocks, (long long)stride, partial_bad_text(why));
  finalize_groups(q, std::move(merged));
  q->merged = true;
  return SN_OK;
}
