/*
 * snappy_engine.h — C ABI of the MI355X-native columnar scan/filter/aggregate
 * engine that drops in behind SnappyData's physical-operator surface.
 *
 * This is the JNI-shaped boundary a SnappyData (reference: SnappyDataInc/snappydata
 * @ /root/reference) host JVM would bind to replace the generated
 * WholeStageCodegen scan+aggregate loop.  Each entry point mirrors a reference
 * seam (file:line cites refer to the reference tree):
 *
 *   sn_engine_create / sn_engine_destroy
 *       — engine lifecycle; replaces per-executor codegen context.
 *   sn_table_define
 *       — schema registration; mirrors ColumnFormatRelation table metadata
 *         (core/.../columnar/impl/ColumnFormatRelation.scala) consumed by
 *         PartitionedPhysicalScan.createFromDataSource
 *         (core/.../ExistingPlans.scala:153-209).
 *   sn_batch_put
 *       — accepts one encoded ColumnBatch: exactly the buffers the
 *         ColumnBatchIterator protocol exposes per batch
 *         (core/.../columnar/ColumnBatchIterator.scala:96-163:
 *          next() -> stats blob, getColumnLob(i), getUpdatedColumnDecoder(i)
 *          -> (delta1,delta2), getDeletedColumnDecoder -> delete mask), and the
 *         store seam ExternalStore.storeColumnBatch
 *         (core/.../columnar/ExternalStore.scala:43-45).  Buffer byte formats
 *         are the reference's column encodings (encoders/.../encoding/
 *         ColumnEncoding.scala:37-53 header; Uncompressed.scala;
 *         DictionaryEncoding.scala; RunLengthEncoding.scala;
 *         BooleanBitSetEncoding.scala; ColumnDeleteEncoder.scala:101-126;
 *         ColumnDeltaDecoder.scala:45-58).  The engine copies the buffers into
 *         GPU HBM; the caller may free them after return (the reference's
 *         retain/release contract, ColumnBatchIterator.scala:102-120, becomes
 *         copy-on-put).
 *   sn_query_submit / sn_query_wait / sn_query_result
 *       — replaces plan execution of
 *         ColumnTableScan (core/.../columnar/ColumnTableScan.scala:186-672)
 *         -> Filter -> SnappyHashAggregateExec
 *         (core/.../aggregate/SnappyHashAggregateExec.scala:240-263,337-500)
 *         and driver-side CollectAggregateExec.executeCollect
 *         (core/.../aggregate/CollectAggregateExec.scala:46-91).
 *   sn_query_partials / sn_query_merge
 *       — the partial->final aggregation exchange the reference performs with a
 *         Spark ShuffleExchange between partial and final
 *         SnappyHashAggregateExec (requiredChildDistribution,
 *         SnappyHashAggregateExec.scala:161-167).  In the MI355X engine the
 *         exchange is an RCCL collective over xGMI run by the caller (one
 *         process per GPU); these functions export/import the fixed-width
 *         partial-aggregate state through a caller-provided DEVICE buffer.
 *
 * All integers little-endian; all buffers plain (pointer,size) pairs — no
 * torch/JVM types.  Status codes: 0 = OK, negative = error (sn_last_error()
 * returns a message for the calling thread's last failure).
 */
#ifndef SNAPPY_ENGINE_H
#define SNAPPY_ENGINE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define SN_OK                0
#define SN_ERR_GENERIC      -1
#define SN_ERR_BADARG       -2
#define SN_ERR_NOMEM        -3
#define SN_ERR_BADFORMAT    -4   /* malformed column blob */
#define SN_ERR_UNSUPPORTED  -5   /* plan/encoding shape not supported yet */
#define SN_ERR_NOGPU        -6   /* HIP device unavailable (the engine never
                                    silently falls back to CPU) */
#define SN_ERR_OVERFLOW     -7   /* result/group-count capacity exceeded */

/* ---- scalar types (SQL-side view of a column) ----
 * Mirrors the subset of Spark types on the hot path
 * (TPCHTableSchema.scala:145-163 load path: int/date->int32, double,
 *  char(1)/varchar -> string). */
typedef enum {
  SN_TYPE_INT32  = 0,   /* IntegerType / DateType (days since epoch)  */
  SN_TYPE_INT64  = 1,   /* LongType / TimestampType (micros)          */
  SN_TYPE_DOUBLE = 2,   /* DoubleType                                 */
  SN_TYPE_STRING = 3,   /* StringType (dictionary-encoded on the path)*/
  SN_TYPE_BOOL   = 4,   /* BooleanType                                */
  SN_TYPE_INT16  = 5,   /* ShortType                                  */
  SN_TYPE_INT8   = 6,   /* ByteType                                   */
  SN_TYPE_FLOAT  = 7    /* FloatType                                  */
} sn_type_t;

/* column encodings = reference typeIds (ColumnEncoding.scala:766-773) */
#define SN_ENC_UNCOMPRESSED  0
#define SN_ENC_RUNLENGTH     1
#define SN_ENC_DICTIONARY    2
#define SN_ENC_BIG_DICTIONARY 3
#define SN_ENC_BOOLEAN_BITSET 4

typedef struct {
  const void *data;
  int64_t     len;     /* bytes; data==NULL,len==0 for an absent buffer */
} sn_buf;

typedef struct {
  sn_type_t dtype;
  int32_t   nullable;  /* 0/1 */
} sn_col_schema;

/* ---- engine config (the knobs of io.snappydata.Property,
 *      core/.../Literals.scala:129-159) ---- */
typedef struct {
  int32_t device;            /* HIP device ordinal this engine binds to */
  int64_t column_batch_size; /* bytes; default 24MB (Literals.scala:129-136) */
  int32_t column_max_delta_rows; /* default 10000 (Literals.scala:138-146) */
  int64_t hash_join_size;    /* broadcast-build threshold; default 100MB
                                (Literals.scala:153-159) */
  int32_t n_buckets;         /* partition count for bucket sharding */
  int32_t shard_rank;        /* this process's rank (one process per GPU) */
  int32_t shard_count;       /* world size; batches whose bucket%shard_count
                                != shard_rank are ignored by sn_batch_put */
} sn_config;

typedef struct sn_engine sn_engine;
typedef struct sn_query  sn_query;

/* ---- plan description ----
 * A thin physical plan for the hot-path shapes the reference plans via
 * SnappyStrategies (core/.../SnappyStrategies.scala:340,547-603):
 * scan -> conjunctive range filter -> (grouped|keyless) aggregate
 * [optionally joined to a broadcast dimension table].                   */

#define SN_MAX_PREDS    8
#define SN_MAX_AGGS     12
#define SN_MAX_GROUPS   2     /* group-by columns */
#define SN_MAX_FACTORS  3
#define SN_MAX_GROUP_SLOTS 1024  /* max distinct groups in round-1 path */
#define SN_KEY_MAX      48    /* max bytes of one group-key string */

/* conjunct range predicate on a scanned column:
 * lo OP value OP hi, with each bound optional.
 * Dictionary string columns take equality only (str_eq/str_len): the
 * engine resolves the literal to its global dictionary id and compares
 * ids — the reference's dictionary filter pushdown
 * (ColumnTableScan + DictionaryOptimizedMapAccessor consume the
 * dictionary INDEX instead of the decoded string).                      */
typedef struct {
  int32_t col;          /* scan-table column ordinal */
  int32_t _pad;
  double  lo_d, hi_d;   /* used when the column is DOUBLE/FLOAT */
  int64_t lo_i, hi_i;   /* used when the column is integer/date */
  uint8_t has_lo, has_hi;
  uint8_t lo_strict, hi_strict;  /* 1: strict inequality */
  uint8_t _pad2[4];
  const char *str_eq;   /* string equality literal (STRING cols only);
                           valid for the duration of the submit call */
  int32_t str_len;
  int32_t _pad3;
  /* IN-list membership (the reference's Q12/Q19-class `col IN (...)`
   * filters, compiled into the generated loop by ColumnTableScan):
   * integer/date columns take in_i[in_n]; dictionary string columns take
   * in_s/in_s_len[in_n] (resolved to dictionary ids at submit, like
   * str_eq).  in_n == 0 disables; all pointers valid only during submit.
   * An IN pred may not also carry range bounds. */
  const int64_t *in_i;
  const char *const *in_s;
  const int32_t *in_s_len;
  int32_t in_n;
  int32_t _pad6;
} sn_pred;

/* one multiplicative factor of an aggregate input: (add + mul * col) */
typedef struct {
  int32_t col;
  int32_t _pad;
  double  add;
  double  mul;
} sn_factor;

#define SN_AGG_SUM        0
#define SN_AGG_COUNT_STAR 1
#define SN_AGG_AVG        2
#define SN_AGG_MIN        3
#define SN_AGG_MAX        4

/* aggregate: SUM/AVG/MIN/MAX over a product of factors, or COUNT(*).
 * Null semantics follow Spark Sum/Average/Count and the Min/Max
 * DeclarativeAggregates (SnappyHashAggregateExec.scala:450-500 accumulate
 * rules): a row contributes iff every referenced column is non-null;
 * COUNT(*) counts every surviving row; MIN/MAX of an empty/all-null
 * input group is NULL. */
typedef struct {
  int32_t kind;
  int32_t nfactors;
  sn_factor factors[SN_MAX_FACTORS];
} sn_agg;

#define SN_JOIN_NONE  -1
#define SN_JOIN_SEMI   0   /* fact row survives iff key present in dim */
#define SN_JOIN_GROUP  1   /* additionally GROUP BY the dim attribute;
                              may combine with ONE fact group column
                              (group_cols[0]) — results then carry
                              (attr, fact key) composite keys */

typedef struct {
  int32_t table;        /* handle from sn_table_define */
  int32_t npreds;
  sn_pred preds[SN_MAX_PREDS];
  int32_t ngroup;       /* 0 = keyless aggregate */
  int32_t group_cols[SN_MAX_GROUPS]; /* dictionary string columns, or integer
                           (int16/int32/int64) key columns.  Integer keys
                           with dense stats-derived spans use direct slots;
                           sparse/unbounded integer keys run the
                           open-address hash aggregate (ByteBufferHashMap /
                           SHAMapAccessor analogue) */
  int32_t naggs;
  int32_t _pad;
  sn_agg  aggs[SN_MAX_AGGS];
  /* broadcast-dimension join (HashJoinExec semantics, HashJoinExec.scala:
   * 285-520: per-task ObjectHashSet build from the replicated row-store
   * dimension, cached across tasks via HashedObjectCache :449-470; here the
   * device hash table is built once per dimension and cached on the engine,
   * resident in HBM — the broadcast).  join_dim = SN_JOIN_NONE disables. */
  int32_t join_dim;       /* handle from sn_dim_define */
  int32_t join_fact_col;  /* int32/int64 fact key column */
  int32_t join_mode;      /* SN_JOIN_SEMI | SN_JOIN_GROUP */
  int32_t _pad4;
} sn_plan;

/* ---- results ----
 * Grouped results are returned sorted ascending by key strings (the
 * reference's Q1 "order by l_returnflag, l_linestatus").                */
typedef struct {
  int32_t nrows;        /* number of (group) rows; 1 for keyless */
  int32_t ngroup;
  int32_t naggs;
  int32_t _pad;
  /* row r, key g: NUL-terminated; empty string for SQL NULL key */
  char    keys[SN_MAX_GROUP_SLOTS][SN_MAX_GROUPS][SN_KEY_MAX];
  uint8_t key_is_null[SN_MAX_GROUP_SLOTS][SN_MAX_GROUPS];
  /* row r, agg a: value (AVG already divided; COUNT as exact integer-valued
   * double; SUM of an all-null/empty input group is NULL) */
  double  vals[SN_MAX_GROUP_SLOTS][SN_MAX_AGGS];
  uint8_t val_is_null[SN_MAX_GROUP_SLOTS][SN_MAX_AGGS];
  int64_t rows_scanned;   /* rows examined after batch skipping */
  int64_t rows_passed;    /* rows surviving the filter */
  int64_t batches_seen;   /* SQLMetrics columnBatchesSeen
                             (ColumnTableScan.scala:111-127) */
  int64_t batches_skipped;/* stats-predicate skips (ColumnTableScan.scala:820-963) */
} sn_result;

/* ---- engine lifecycle ---- */
sn_engine *sn_engine_create(const sn_config *cfg);
void       sn_engine_destroy(sn_engine *e);
const char *sn_last_error(void);
/* version/capability probe; returns the gfx arch the .so was built for */
const char *sn_engine_arch(void);

/* ---- schema / data plane ---- */
int32_t sn_table_define(sn_engine *e, const char *name,
                        int32_t ncols, const sn_col_schema *schema);

/* Ingest one encoded column batch (all buffers little-endian, reference
 * formats).  columns[i] = blob for column i (required).  delete_mask and
 * deltas may be absent.  deltas is laid out [ncols][2] (delta1,delta2 per
 * column; ColumnDelta.deltaColumnIndex depths 0..1, ColumnDelta.scala:256-301)
 * — pass NULL when the batch has no update deltas.  stats is the UnsafeRow
 * stats blob (ColumnStatsSchema, ColumnEncoding.scala:1015-1036); pass an
 * empty buf to disable stats-based skipping for this batch. */
int32_t sn_batch_put(sn_engine *e, int32_t table,
                     int64_t uuid, int32_t bucket_id, int32_t num_rows,
                     const sn_buf *columns, const sn_buf *stats,
                     const sn_buf *delete_mask, const sn_buf *deltas);

/* f2 fast ingest (the ColumnBatchCreator rollover with encode + stats
 * offloaded to the GPU): fixed-width NON-NULL columns arrive as RAW value
 * arrays (the Uncompressed encoder for numerics is the identity — the
 * engine uploads the bytes once and computes the ColumnStatsSchema bounds
 * ON DEVICE, async on the ingest stream); other columns arrive as encoded
 * blobs in `encoded`.  Per column exactly one of raw[c].data /
 * encoded[c].data is set.  Queries resolve the pending device bounds with
 * one stream sync. */
int32_t sn_batch_put_raw(sn_engine *e, int32_t table, int64_t uuid,
                         int32_t bucket_id, int32_t num_rows,
                         const sn_buf *raw, const sn_buf *encoded);

/* number of resident batches / rows for a table on this shard */
int64_t sn_table_num_batches(sn_engine *e, int32_t table);
int64_t sn_table_num_rows(sn_engine *e, int32_t table);

/* ---- low-cardinality f64 columns: 1-byte code sidecars ----
 * At put time the engine tries to narrow every null-free uncompressed DOUBLE
 * column of a batch: when the batch holds at most 256 distinct 64-bit value
 * patterns, it keeps a num_rows-byte code array and a 256-entry dictionary
 * beside the blob, and scans read 1 B/row instead of 8 (the f64 body stays
 * resident for every other reader, so a narrowed column costs 1 B/row of
 * extra HBM — about 3 B on lineitem's 34 B/row).  Results do not change:
 * dictionary[code] is the body's exact bit pattern.  Any write to the body
 * (update deltas at put or sn_batch_mutate) rebuilds or drops the sidecar.
 * A query uses the codes for a column only when every batch it scans has
 * them.  SN_NARROW=0 in the environment at sn_engine_create turns the
 * feature off for that engine.
 *
 * sn_table_narrowed_batches: batches of `table` holding a live sidecar for
 * column `col` (resolves pending device results first; -1 on bad args).
 * sn_f64_narrow_host: the put-time kernels' contract in plain C++ — fits:
 * dict[0..*ndict) = distinct patterns ascending as unsigned 64-bit integers,
 * dict[*ndict..256) = 0, codes[i] = index of body[i]; more than 256
 * patterns: *ndict = -1, dict[0..256) = 0, codes untouched. */
int64_t sn_table_narrowed_batches(sn_engine *e, int32_t table, int32_t col);
void    sn_f64_narrow_host(const double *body, int64_t n, uint8_t *codes,
                           double *dict, int32_t *ndict);

/* ---- dimension tables (row-store stand-in for the broadcast join) ----
 * The reference keeps dimension tables in the GemFire row store and builds
 * the probe map per task from region get()s; here the host holds the rows
 * and the engine broadcasts a key -> attribute hash table into HBM. */
int32_t sn_dim_define(sn_engine *e, const char *name);
/* keys must be unique (the dimension's primary key).  attrs: optional
 * per-key attribute strings (payload + lens) for SN_JOIN_GROUP; NULL for
 * semi-join-only dimensions. */
int32_t sn_dim_put(sn_engine *e, int32_t dim, int64_t nkeys,
                   const int64_t *keys, const char *attr_payload,
                   const int32_t *attr_lens);

/* ---- partitioned-partitioned (colocated) join build ----
 * Populate an EMPTY dimension handle from a resident COLUMN TABLE's rows,
 * built on device: the HashJoinExec per-task build of the probe map from
 * the build side (HashJoinExec.scala:285-520) with HashedObjectCache reuse
 * (:449-470).  The reference's partitioned-partitioned joins run
 * bucket-LOCALLY when tables are colocated on the join key (GemFire
 * colocation) — both sides sharded identically means no exchange step, so
 * each shard builds from ITS build-side rows and probes ITS fact rows.
 * key_col: int32/int64 column with UNIQUE values per shard (duplicate keys
 * with conflicting payloads fail with SN_ERR_BADARG); attr_col: optional
 * dictionary-string column whose values become the SN_JOIN_GROUP
 * attributes (-1 = semi-join only).  Rebuild after the build table
 * changes; deleted/patched rows are honored at build time. */
int32_t sn_dim_from_table(sn_engine *e, int32_t dim, int32_t table,
                          int32_t key_col, int32_t attr_col);

/* attach the CURRENT (cumulative) mutation state to an existing batch —
 * the UPDATE/DELETE seam: delete_mask and the per-column delta pairs
 * replace any previous state for that batch; stats (if given) replace the
 * stats row, else stats-based skipping is disabled for the batch.
 * (ColumnDelta.scala:300-301; UpdatedColumnDecoder.scala:69-115) */
int32_t sn_batch_mutate(sn_engine *e, int32_t table, int64_t uuid,
                        int32_t bucket_id, const sn_buf *delete_mask,
                        const sn_buf *deltas, const sn_buf *stats);

/* ---- query plane ---- */
sn_query *sn_query_submit(sn_engine *e, const sn_plan *plan);
/* blocks until device work completes; returns status */
int32_t   sn_query_wait(sn_query *q);
/* fills final (or this shard's partial, before any merge) result */
int32_t   sn_query_result(sn_query *q, sn_result *out);
void      sn_query_destroy(sn_query *q);
/* scan-kernel duration in ms (HIP events on the launch stream); -1 if the
 * query launched nothing */
double    sn_query_kernel_ms(sn_query *q);
/* result paging for group counts beyond SN_MAX_GROUP_SLOTS (dense group
 * spaces up to 2^20 slots run through a global-atomic accumulate path);
 * sn_query_result returns the first page */
int32_t   sn_query_result_page(sn_query *q, int64_t offset, sn_result *out);
int64_t   sn_query_num_groups(sn_query *q);
/* 1 when the query ran a query-compiled (hipRTC) kernel, 0 interpreted */
int32_t   sn_query_used_jit(sn_query *q);
/* bit c set: the compiled kernel read table column c "late", that is for the
 * rows that pass the predicates only, instead of streaming it whole.  The
 * engine does this for plain DOUBLE columns that only aggregate factors use,
 * in keyless plans whose predicates are estimated (from the batch bounds)
 * to keep few rows.  0 when no column was, SN_LATE=0 was set when the
 * engine was created, or the query ran interpreted.  Columns 0..62. */
int64_t   sn_query_late_cols(sn_query *q);
/* 1 when the late columns were read by the image-free ("direct") compiled
 * kernel: a late plan of SUM/COUNT/AVG aggregates whose predicates are all
 * ranges and whose other columns are INT32, INT16 or narrowed DOUBLE.  0
 * otherwise, or with SN_DIRECT=0 set when the engine was created. */
int32_t   sn_query_direct(sn_query *q);
/* ORDER BY <aggregate value> [DESC] LIMIT k epilogue (SnappySortExec /
 * TakeOrderedAndProject semantics, core/.../SnappySortExec.scala): reorders
 * the finalized group rows by aggregate `agg_idx`'s value (NULLs last,
 * ties broken by the key ordering) and truncates to k (k <= 0: no limit).
 * Call after any partial merge; subsequent sn_query_result/`_page` calls
 * return the reordered rows.  agg_idx < 0 restores the key ordering. */
int32_t   sn_query_order_by(sn_query *q, int32_t agg_idx, int32_t descending,
                            int64_t k);

/* ---- multi-GPU partial exchange (caller runs the RCCL collective) ----
 * The caller (one process per GPU, torch.distributed over RCCL/xGMI)
 * exchanges fixed-width partial blocks between the shards' local aggregates
 * and feeds the gathered blocks back for the final merge — mirroring the
 * reference's partial->final ShuffleExchange + CollectAggregateExec.
 *
 * Block layouts (all f64 so the block is directly collective-reducible;
 * counts are exact in f64 up to 2^53):
 *   keyless: [naggs sums][naggs non-null counts][1 row count]
 *            -> identical slot layout on every shard: ncclAllReduce-able.
 *   grouped: [i32 n_slots][i32 capacity] then capacity slots of
 *            { char keys[SN_MAX_GROUPS][SN_KEY_MAX]; u8 key_null[SN_MAX_GROUPS];
 *              u8 pad[6]; f64 sums[naggs]; f64 counts[naggs]; f64 rowcount }
 *            -> self-describing (per-batch dictionaries mean shards need not
 *            agree on slot order): ncclAllGather + key-merge.              */
int64_t sn_query_partial_bytes(sn_query *q);
/* export this shard's partial block; dst_is_device: 1 = HIP device memory */
int32_t sn_query_partials(sn_query *q, void *dst, int32_t dst_is_device);
/* variable-capacity variants for group counts beyond SN_MAX_GROUP_SLOTS
 * (big dense slot spaces and the sparse hash aggregate): the caller
 * negotiates one capacity across ranks (e.g. an allreduce-MAX of
 * sn_query_num_groups) so every block in the collective is the same size —
 * mirroring how the reference's hash-partitioned partial->final exchange
 * sizes its shuffle blocks dynamically (SnappyHashAggregateExec.scala:
 * 161-167).  Block layout is unchanged; capacity rides in the header. */
int64_t sn_query_partial_bytes2(sn_query *q, int32_t cap_slots);
int32_t sn_query_partials2(sn_query *q, void *dst, int32_t dst_is_device,
                           int32_t cap_slots);
int32_t sn_query_partials_sharded2(sn_query *q, int32_t world, void *dst,
                                   int32_t cap_slots);
/* key-sharded split for the grouped all-to-all: write
 * `world` same-format blocks into dst (world * partial_bytes), block d
 * holding only the groups whose key hashes to shard d.  After the
 * all-to-all, each rank merges the world blocks it received (all of which
 * carry only its keys) with sn_query_merge. */
int32_t sn_query_partials_sharded(sn_query *q, int32_t world, void *dst);
/* merge n_blocks partial blocks (stride bytes apart, host memory) into the
 * final result; n_blocks=1 imports an already-all-reduced keyless block.
 * The blocks come from other ranks, so each is checked against `stride`
 * before any is folded, and nothing past `stride` bytes of a block is read.
 * SN_ERR_BADARG, with the block's index and the reason in sn_last_error and
 * the query's result left as it was, when
 *   keyless: stride < (2 * naggs + 1) * 8;
 *   grouped: stride < 8, n_slots < 0, 8 + n_slots * sizeof(slot) > stride,
 *            or one of the group keys of a used slot has no NUL within its
 *            SN_KEY_MAX bytes.
 * Groups are matched on (key_null, key bytes) per column: a NULL key and a
 * key whose text is "\x01" are two groups. */
int32_t sn_query_merge(sn_query *q, const void *blocks, int64_t stride,
                       int32_t n_blocks);

/* ---- exact DECIMAL aggregation (precision <= 18) ----
 * The reference loads TPC-H measures as DECIMAL(15,2) and Catalyst returns
 * SUM/AVG over them as exact decimals (Sum/Average over DecimalType in
 * SnappyHashAggregateExec's generated accumulate code).  A decimal column of
 * precision <= 18 is stored by the reference as an 8-byte long holding the
 * unscaled value — the readLongDecimal/writeLongDecimal path of
 * ColumnEncoding/Uncompressed (cited from memory of the reference tree; the
 * variable-length binary decimals of precision > 18 stay unbuilt).  Here
 * such a column is an SN_TYPE_INT64 column: every INT64 ingest path
 * (uncompressed, RLE, nulls, delete masks, update deltas, sn_batch_put_raw)
 * and the exact lo_i/hi_i and IN-list predicates apply unchanged, with
 * literals given unscaled (`l_discount between 0.05 and 0.07` at scale 2 is
 * 5..7).  sn_query_submit keeps accepting decimal-declared columns as plain
 * INT64 columns on the double path.
 *
 *   sn_table_set_decimal
 *       — attaches DecimalType(precision, scale) metadata to an INT64 column
 *         (ColumnFormatRelation schema metadata).  1 <= precision <= 18,
 *         0 <= scale <= precision; anything else, or a non-INT64 column, is
 *         SN_ERR_BADARG.
 *   sn_query_submit_dec / sn_query_result_dec
 *       — the decimal twin of sn_query_submit/sn_query_result: the same
 *         ColumnTableScan -> Filter -> SnappyHashAggregateExec pipeline with
 *         DecimalType aggregation buffers.  `plan` supplies table, predicates
 *         and group columns (plan->naggs must be 0, join_dim SN_JOIN_NONE);
 *         every factor column must be decimal-declared.  Kinds: SUM, AVG,
 *         COUNT_STAR, MIN, MAX (MIN/MAX take exactly one factor).  The result
 *         scale is the sum of the factor scales; AVG adds 4 and rounds
 *         HALF_UP (Spark: avg(decimal(p,s)) -> decimal(p+4,s+4)); COUNT has
 *         scale 0.  Spark non-ANSI semantics: a row contributes iff every
 *         referenced column is non-null; SUM/AVG/MIN/MAX of an empty or
 *         all-null group are NULL; a group with any surviving row whose
 *         |product| >= 10^38, or whose final |sum| >= 10^38, is NULL.
 *         Rejected with SN_ERR_UNSUPPORTED: sparse-hash group keys, slot
 *         counts beyond the LDS accumulator capacity, joins, and factors
 *         whose |add| + |mul| * 10^precision can exceed int64.
 *         sn_query_wait/_destroy/_kernel_ms/_num_groups/_result/_result_page
 *         work on the handle (vals = nearest double of the exact value);
 *         sn_query_used_jit is 0; sn_query_order_by, sn_query_partials* and
 *         sn_query_merge return SN_ERR_UNSUPPORTED.
 *   sn_dec_to_string / sn_dec_avg
 *       — host-only helpers (no GPU needed): Decimal.toString and the
 *         Average result expression's divide. */
typedef struct {
  int32_t col, _pad;
  int64_t add, mul;      /* add + mul*col, unscaled, at col's scale */
} sn_dec_factor;

typedef struct {
  int32_t kind, nfactors;
  sn_dec_factor factors[SN_MAX_FACTORS];
} sn_dec_agg;

typedef struct {
  uint64_t lo;           /* two's-complement i128: (hi << 64) | lo */
  int64_t  hi;
  int32_t  scale;
  uint8_t  is_null, _pad[3];
} sn_dec_val;

int32_t   sn_table_set_decimal(sn_engine *e, int32_t table, int32_t col,
                               int32_t precision, int32_t scale);
sn_query *sn_query_submit_dec(sn_engine *e, const sn_plan *plan,
                              int32_t naggs, const sn_dec_agg *aggs);
/* exact value of aggregate `agg` in result row `row` (the row order of
 * sn_query_result) */
int32_t   sn_query_result_dec(sn_query *q, int64_t row, int32_t agg,
                              sn_dec_val *out);
/* "-123.4500": writes a NUL-terminated string, returns its length
 * (SN_ERR_BADARG when cap is too small; NULL formats as "NULL") */
int32_t   sn_dec_to_string(const sn_dec_val *v, char *buf, int32_t cap);
/* sum / count at scale+4, rounded HALF_UP; NULL for a NULL sum, count <= 0
 * or a quotient of 10^38 or more */
int32_t   sn_dec_avg(const sn_dec_val *sum, int64_t count, sn_dec_val *out);
/* ---- row-returning filter scan: SELECT cols WHERE preds [LIMIT n] ----
 * The ColumnTableScan -> Filter -> Project half of the operator surface
 * (ColumnTableScan.scala:186-672 without an aggregate above it): what a host
 * needs for plain SELECTs, for operators the engine does not run itself
 * (non-colocated joins, sorts, windows), and for ColumnUpdateExec /
 * ColumnDeleteExec, which need the batch and ordinal of every matching row
 * to build the delta and delete blobs sn_batch_mutate accepts.
 *
 *   sn_scan_submit
 *       — `plan` supplies table and predicates (every form sn_query_submit
 *         takes: ranges, str_eq, IN-lists); plan->naggs and plan->ngroup must
 *         be 0 (else SN_ERR_BADARG) and join_dim SN_JOIN_NONE (else
 *         SN_ERR_UNSUPPORTED).  proj_cols[nproj], 1 <= nproj <= 8, are table
 *         column ordinals or SN_PROJ_ROWID, duplicates allowed; predicate and
 *         projected columns together may name at most 8 distinct table
 *         columns (else SN_ERR_UNSUPPORTED).  limit <= 0: no limit.  Checks
 *         run in the order: null arguments, unknown table, plan shape,
 *         columns, then SN_ERR_NOGPU.
 *         Rows come back in scan order — the table's batch order, then row
 *         ordinal — the same from run to run; limit k keeps the first k rows
 *         of that order.  Stats-based batch skipping applies.
 *         The result is columnar and stays in device memory, owned by the
 *         query and released at sn_query_destroy: projection p is a dense
 *         array of sn_rows_count elements in the column's own type —
 *         DOUBLE f64, INT64 i64, INT32 i32, FLOAT f32, INT16 i16, INT8 i8,
 *         BOOL u8 0/1, STRING i32 global dictionary id (sn_table_dict_value),
 *         ROWID i64 — plus one validity byte per row (1 value, 0 NULL; a NULL
 *         row's value bytes are zero).  Values are copies, bit for bit: a
 *         DOUBLE keeps its 64-bit pattern (-0.0, infinities, NaN payloads)
 *         through plain bodies, 1-byte codes, run-length runs and update
 *         deltas; INT64 is exact beyond 2^53.  (A FLOAT NaN stays a NaN; its
 *         payload is not promised on batches with nulls or deltas.)
 *         SN_PROJ_ROWID yields (batch << 32) | row ordinal, batch being the
 *         table's own batch index — the one sn_table_get_blob takes, whatever
 *         the scan skipped — which sn_table_batch_id turns into the
 *         (uuid, bucket_id) of sn_batch_mutate.
 *         On the handle: sn_query_wait/_destroy/_kernel_ms work (the time is
 *         the sum of the three scan kernels' own intervals);
 *         sn_query_result fills nrows = 0, naggs = 0 and the four metrics,
 *         rows_passed being the matching rows BEFORE the limit;
 *         sn_query_used_jit and sn_query_late_cols return 0;
 *         sn_query_result_page, sn_query_order_by, sn_query_partials*,
 *         sn_query_merge and sn_query_result_dec return SN_ERR_UNSUPPORTED.
 *         A sharded engine returns its local rows; there is no exchange.
 *   sn_rows_count
 *       — rows returned (after the limit); waits for the query.
 *   sn_rows_fetch
 *       — copies rows [offset, offset + n) of projection `proj` to host
 *         (dst_is_device 0) or HIP device memory (1): n elements to `values`,
 *         n validity bytes to `valid` (may be NULL).  n == 0 is fine; a range
 *         outside [0, count] is SN_ERR_BADARG.
 *       Both return SN_ERR_BADARG on a handle from an aggregate submit.
 *   sn_table_dict_value
 *       — the bytes of global dictionary id `gid` of STRING column `col`:
 *         returns the length and, when buf is not NULL, copies the value
 *         (cap < length is SN_ERR_BADARG; a NUL follows when there is room).
 *         A bad table, column or id is SN_ERR_BADARG.
 *   sn_table_batch_id
 *       — (uuid, bucket_id) of the table's batch `batch`, as given at put. */
#define SN_PROJ_ROWID (-1)   /* pseudo-column: int64 (table batch index << 32)
                                | row ordinal */
sn_query *sn_scan_submit(sn_engine *e, const sn_plan *plan,
                         int32_t nproj, const int32_t *proj_cols,
                         int64_t limit);
int64_t   sn_rows_count(sn_query *q);
int32_t   sn_rows_fetch(sn_query *q, int32_t proj, int64_t offset, int64_t n,
                        void *values, uint8_t *valid, int32_t dst_is_device);
int32_t   sn_table_dict_value(sn_engine *e, int32_t table, int32_t col,
                              int32_t gid, char *buf, int32_t cap);
int32_t   sn_table_batch_id(sn_engine *e, int32_t table, int32_t batch,
                            int64_t *uuid, int32_t *bucket);

/* ---- ordered row scan: SELECT cols WHERE preds ORDER BY key LIMIT k ----
 * Spark's TakeOrderedAndProjectExec over ColumnTableScan -> Filter: the k
 * rows with the smallest keys among the rows that pass the predicates, in
 * key order, selected and sorted on the device.  The host never sees the
 * other matching rows.
 *
 *   sn_scan_submit_ordered
 *       — plan, nproj, proj_cols as in sn_scan_submit, validated the same way
 *         in the same order; then
 *           order_col: a table column ordinal (SN_PROJ_ROWID or an ordinal out
 *             of range is SN_ERR_BADARG).  It need not be projected.  It
 *             counts towards the 8 distinct device columns (a ninth is
 *             SN_ERR_UNSUPPORTED);
 *           order_flags: SN_ORDER_DESC, and at most one of
 *             SN_ORDER_NULLS_FIRST / SN_ORDER_NULLS_LAST (any other bit, or
 *             both NULLS bits, is SN_ERR_BADARG);
 *           limit: 1 <= limit <= SN_ORDER_MAX_LIMIT.  limit < 1 is
 *             SN_ERR_BADARG (an ordered scan without a limit is a full sort,
 *             which this is not); a larger limit is SN_ERR_UNSUPPORTED;
 *         then SN_ERR_NOGPU.
 *         Ordering contract:
 *           Key types — every column type can be the key.  INT8/16/32/64 sort
 *             as signed integers (INT64 exact over its full range), BOOL false
 *             < true, STRING by unsigned bytewise comparison of the values
 *             (UTF8String's binary compare, not dictionary ids), FLOAT and
 *             DOUBLE as Spark's nanSafeCompareDoubles: -0.0 equals 0.0, every
 *             NaN equals every other NaN, and NaN is greater than +inf.
 *           NULLs — Spark's default: NULLS FIRST ascending, NULLS LAST
 *             descending; a NULLS flag overrides it.
 *           Ties — rows whose keys compare equal (-0.0 and 0.0, NaNs of
 *             different payloads, NULL and NULL included) come out in scan
 *             order (table batch, then ordinal), ascending and descending
 *             alike, so the result is a pure function of the table contents.
 *           Values — projected values are copies with sn_scan_submit's
 *             guarantees: a -0.0 key comes back as -0.0, NaN payloads survive.
 *         The result is a rows handle like sn_scan_submit's: sn_rows_count is
 *         min(matching rows, limit); sn_rows_fetch, sn_query_wait/_destroy/
 *         _kernel_ms work (the time is mark + offsets + the order stage);
 *         sn_query_result gives the metrics, rows_passed counted BEFORE the
 *         limit; the other calls return SN_ERR_UNSUPPORTED as on an unordered
 *         rows handle.
 *         A sharded engine returns its LOCAL top k; merging the shards' sorted
 *         locals (a k-way merge of at most k rows each) is the host's job. */
#define SN_ORDER_DESC         1
#define SN_ORDER_NULLS_FIRST  2   /* explicit; at most one of the two */
#define SN_ORDER_NULLS_LAST   4
#define SN_ORDER_MAX_LIMIT    8192
sn_query *sn_scan_submit_ordered(sn_engine *e, const sn_plan *plan,
                                 int32_t nproj, const int32_t *proj_cols,
                                 int32_t order_col, int32_t order_flags,
                                 int64_t limit);

/* ---- row scan over a dimension join: inner, left outer, left anti ----
 * ColumnTableScan -> Filter -> HashJoinExec -> Project
 * [-> TakeOrderedAndProject]: SELECT f.cols, d.attr FROM fact f JOIN dim d ON
 * f.k = d.key WHERE preds [ORDER BY f.col] [LIMIT k], the probe running on
 * the device between the filter and the projection (HashJoinExec.scala:285-520
 * runs Inner, LeftOuter, LeftSemi and LeftAnti through one probe; so does
 * this).  The dimension's keys are unique, so every type yields at most one
 * output row per fact row.
 *
 *   sn_scan_submit_join
 *       — plan, nproj, proj_cols, limit as in sn_scan_submit, with the join in
 *         plan->join_dim / join_fact_col (join_mode SN_JOIN_SEMI).
 *         sn_scan_submit and sn_scan_submit_ordered keep answering a join plan
 *         with SN_ERR_UNSUPPORTED; this is the entry that takes one.
 *         Join contract (a row JOINS iff its key is NOT NULL and equal to a
 *         dimension key; INT64_MIN as a fact value never joins):
 *           SN_RJOIN_INNER       rows that pass the predicates and join.  With
 *                                no SN_PROJ_DIM_ATTR projected this is the
 *                                left semi join.
 *           SN_RJOIN_LEFT_OUTER  every row that passes the predicates; the
 *                                attribute is NULL where the row does not join.
 *           SN_RJOIN_LEFT_ANTI   rows that pass and do NOT join (Spark's
 *                                LeftAnti, NOT EXISTS — not the null-aware
 *                                NOT IN): NULL-key rows survive.
 *         SN_PROJ_DIM_ATTR among proj_cols is the joined dimension row's
 *         attribute: an int32 attribute id (sn_dim_attr_value gives its bytes)
 *         plus the validity byte; an unjoined row (LEFT_OUTER only) has
 *         validity 0 and value bytes 0.
 *         order_col == SN_ORDER_NONE: sn_scan_submit's scan order and limit
 *         rules (limit <= 0: none); order_flags must be 0.  Any other
 *         order_col: sn_scan_submit_ordered's contract verbatim, limit bounds
 *         included.  The key is a fact column: SN_PROJ_ROWID or
 *         SN_PROJ_DIM_ATTR as order_col is SN_ERR_BADARG.
 *         Checks run in this order: sn_scan_submit's (null arguments, unknown
 *         table, naggs/ngroup non-zero SN_ERR_BADARG, npreds, nproj);
 *         join_type outside 0..2, join_dim SN_JOIN_NONE or unknown, join_mode
 *         not SN_JOIN_SEMI, an empty dimension, join_fact_col outside the
 *         schema: SN_ERR_BADARG; a key column that is not INT32/INT64:
 *         SN_ERR_UNSUPPORTED; the columns — a bad predicate or projection
 *         ordinal, SN_PROJ_DIM_ATTR under LEFT_ANTI (there is no right side to
 *         project) or on a dimension with sn_dim_num_attrs == 0:
 *         SN_ERR_BADARG; a ninth distinct device column, the key column
 *         counting: SN_ERR_UNSUPPORTED; the order checks; then SN_ERR_NOGPU.
 *         The result is a rows handle: sn_rows_count, sn_rows_fetch,
 *         sn_query_wait/_destroy/_kernel_ms and sn_query_result work as on
 *         the other two, rows_passed counting the rows AFTER the join and
 *         BEFORE the limit; the other calls return SN_ERR_UNSUPPORTED.
 *         A sharded engine returns its local rows.
 *   sn_dim_num_attrs
 *       — distinct attribute values of dimension `dim` (the ids
 *         SN_PROJ_DIM_ATTR yields are 0 .. that - 1); 0 for a dimension loaded
 *         without attributes; SN_ERR_BADARG for a bad handle.
 *   sn_dim_attr_value
 *       — the bytes of attribute id `id`, in sn_table_dict_value's shape:
 *         returns the length and, when buf is not NULL, copies the value
 *         (cap < length is SN_ERR_BADARG; a NUL follows when there is room).
 *         A bad dimension or id is SN_ERR_BADARG.  Needs no GPU. */
#define SN_PROJ_DIM_ATTR   (-2)  /* pseudo-column: the joined dimension row's
                                    attribute */
#define SN_RJOIN_INNER      0
#define SN_RJOIN_LEFT_OUTER 1
#define SN_RJOIN_LEFT_ANTI  2
#define SN_ORDER_NONE      (-1)  /* order_col: scan order, limit optional */
sn_query *sn_scan_submit_join(sn_engine *e, const sn_plan *plan,
                              int32_t join_type, int32_t nproj,
                              const int32_t *proj_cols, int32_t order_col,
                              int32_t order_flags, int64_t limit);
int32_t   sn_dim_num_attrs(sn_engine *e, int32_t dim);
int32_t   sn_dim_attr_value(sn_engine *e, int32_t dim, int32_t id, char *buf,
                            int32_t cap);

/* status code of the calling thread's last failure (pairs with
 * sn_last_error; lets callers of the pointer-returning submits tell
 * SN_ERR_UNSUPPORTED from SN_ERR_BADARG) */
int32_t   sn_last_error_code(void);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_ENGINE_H */
