/*
 * kernels.hip — CDNA4 (gfx950) scan -> filter -> aggregate kernels (v4).
 *
 * MI355X-native replacement for the reference's generated per-partition JVM
 * loop (WholeStageCodegen of ColumnTableScan -> Filter ->
 * SnappyHashAggregateExec; ColumnTableScan.scala:636-815,
 * SnappyHashAggregateExec.scala:337-500).  HBM-bandwidth-bound by nature
 * (no dense contraction — MFMA unused by design; DESIGN.md roofline).
 *
 * Iteration history (measured on MI355X):
 *  v1 per-lane value arrays -> 112 B/lane scratch -> 9.6% of HBM peak.
 *  v2 scalar registers + per-row kind switches -> 1863 blocks, SGPR spill
 *     storm -> 15%.
 *  v3 columnar LDS conversion + branch-free row phase -> 23% (Q6); grouped
 *     8x8 register accumulators spilled 372 B/lane -> 3.9% (Q1).
 *  v4 (this file):
 *     - conversion loops compile-time unrolled and vectorized (double2 /
 *       int2 loads, ds_write_b128) on full chunks;
 *     - separate grouped kernel that evaluates predicates once into an LDS
 *       (slot, alive) image, then processes aggregates in groups of 4 with
 *       per-lane sums[NSLOTS][4] registers, wave-reducing each chunk into an
 *       LDS block accumulator — register pressure bounded for any slot
 *       count; one global atomic per accumulator per block at the end.
 *
 * One launch covers EVERY column batch via a host-built tile array.
 */
#include <hip/hip_runtime.h>
#include "engine_internal.h"

#define WG 256
#define CHUNK 1024
#define AGRP 4                  /* aggregates per register pass (grouped) */

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef int int2_t __attribute__((ext_vector_type(2)));

/* Global-address-space pointer cast.  Pointers reaching the kernel through
 * descriptor structs are generic, so plain derefs lower to flat_load_* —
 * and flat loads tick BOTH vmcnt and lgkmcnt, so every LDS wait drains all
 * in-flight global loads (measured: the whole prefetch pipeline collapsed).
 * Casting to address_space(1) lowers them to global_load_* (vmcnt only). */
#define GAS __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const GAS T *as_global(const T *p) {
  return (const GAS T *)(unsigned long long)(uintptr_t)p;
}

__device__ __forceinline__ int bm_get(const uint64_t *bm, int row) {
  return (int)((as_global(bm)[row >> 6] >> (row & 63)) & 1ull);
}

__device__ __forceinline__ int nonnull_pos(const uint64_t *nullw,
                                           const uint32_t *pfx, int row) {
  uint64_t w = as_global(nullw)[row >> 6];
  uint64_t mask = (1ull << (row & 63)) - 1ull;
  return row - (int)(as_global(pfx)[row >> 6] + __popcll(w & mask));
}

__device__ __forceinline__ int patch_find(const int32_t *pos_, int n, int row) {
  const GAS int32_t *pos = as_global(pos_);
  int lo = 0, hi = n - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    int p = pos[mid];
    if (p == row) return mid;
    if (p < row) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

/* RLE: value of nonNullPosition nnp = vals[first run whose end > nnp] */
__device__ __forceinline__ double rle_value(const sn_dev_col &c, int nnp) {
  const GAS int32_t *ends = (const GAS int32_t *)(uintptr_t)c.rle_ends;
  const GAS double *vals = (const GAS double *)(uintptr_t)c.rle_vals;
  int lo = 0, hi = c.rle_n - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ends[mid] > nnp) hi = mid; else lo = mid + 1;
  }
  return vals[lo];
}

/* general-path read (nulls/patches/any kind); returns 0 if NULL */
__device__ __forceinline__ int read_general(const sn_dev_col &c, int row,
                                            double *vd, long long *vi, int *gid) {
  if (c.patch_n && bm_get(c.patch_bm, row)) {
    int pi = patch_find(c.patch_pos, c.patch_n, row);
    if (pi >= 0) {
      if (c.patch_nullbm && bm_get(c.patch_nullbm, pi)) return 0;
      double pv = as_global(c.patch_val)[pi];
      if (c.kind == SN_K_DICT16 || c.kind == SN_K_DICT32) {
        *gid = (int)__double2ll_rn(pv);
        return 1;
      }
      if (c.kind == SN_K_F64 || c.kind == SN_K_F32 || c.kind == SN_K_F64C8) {
        *vd = pv; *vi = (long long)pv;
      }
      else if (c.kind == SN_K_I64 || c.kind == SN_K_RLE_I64) {
        /* INT64 patch values travel as RAW BITS (decode_delta keeps them
         * exact beyond 2^53); vd keeps the raw-bit double so the LDS image
         * stays in the i64 raw-bit convention */
        *vi = __double_as_longlong(pv); *vd = pv;
      }
      else { long long b = __double2ll_rn(pv); *vi = b; *vd = (double)b; }
      return 1;
    }
  }
  int nnp = row;
  if (c.has_nulls) {
    if (bm_get(c.nullw, row)) return 0;
    nnp = nonnull_pos(c.nullw, c.nullpfx, row);
  }
  switch (c.kind) {
    case SN_K_F64: *vd = as_global((const double *)c.body)[nnp]; *vi = (long long)*vd; break;
    case SN_K_I32: *vi = as_global((const int32_t *)c.body)[nnp]; *vd = (double)*vi; break;
    case SN_K_I64: *vi = as_global((const long long *)c.body)[nnp]; *vd = (double)*vi; break;
    case SN_K_F32: *vd = as_global((const float *)c.body)[nnp]; *vi = (long long)*vd; break;
    case SN_K_I16: *vi = as_global((const int16_t *)c.body)[nnp]; *vd = (double)*vi; break;
    case SN_K_DICT16: *gid = as_global(c.dictmap)[(int)(uint16_t)as_global((const int16_t *)c.body)[nnp]]; break;
    case SN_K_DICT32: *gid = as_global(c.dictmap)[as_global((const int32_t *)c.body)[nnp]]; break;
    case SN_K_BOOLBIT: *vi = bm_get((const uint64_t *)c.body, nnp); *vd = (double)*vi; break;
    case SN_K_U8: *vi = as_global((const uint8_t *)c.body)[nnp] == 1; *vd = (double)*vi; break;
    case SN_K_S8: *vi = as_global((const int8_t *)c.body)[nnp]; *vd = (double)*vi; break;
    case SN_K_F64C8:   /* 1-byte code into the batch's value dictionary */
      *vd = as_global(c.rle_vals)[as_global((const uint8_t *)c.body)[nnp]];
      *vi = (long long)*vd;
      break;
    case SN_K_RLE:
      *vd = rle_value(c, nnp);
      *vi = __double2ll_rn(*vd);        /* numeric doubles (i16/i32 runs) */
      break;
    case SN_K_RLE_I64:
      *vd = rle_value(c, nnp);          /* raw i64 bits as double */
      *vi = __double_as_longlong(*vd);  /* bitcast back to the exact value */
      break;
  }
  return 1;
}

/* ---- conversion pass: decode one chunk of every referenced column into the
 * canonical LDS image (f64 values; int64 raw-bitcast; dict -> premultiplied
 * group id as f64).  Vectorized (16 B/lane) on full chunks. ---- */
__device__ __forceinline__ void convert_chunk(
    const sn_dev_batch &b, int nused, int base, int rows, int num_rows,
    double *sval, uint64_t *svalid, uint64_t *sdead) {
  const int tid = threadIdx.x;
  const int clean = b.clean;
  for (int c = 0; c < nused; c++) {
    const sn_dev_col col = b.cols[c];
    double *dst = sval + (size_t)c * CHUNK;
    if (clean) {
      switch (col.kind) {
        case SN_K_F64: {
          const GAS double *src = as_global((const double *)col.body) + base;
          if (rows == CHUNK) {
#pragma unroll
            for (int k = 0; k < CHUNK / (2 * WG); k++) {
              int h = tid + k * WG;   /* pair index */
              ((double2_t *)dst)[h] = ((const GAS double2_t *)src)[h];
            }
          } else {
#pragma unroll
            for (int k = 0; k < CHUNK / WG; k++) {
              int r = tid + k * WG;
              if (r < rows) dst[r] = src[r];
            }
          }
          break;
        }
        case SN_K_I32: {
          const GAS int32_t *src = as_global((const int32_t *)col.body) + base;
          if (rows == CHUNK) {
#pragma unroll
            for (int k = 0; k < CHUNK / (2 * WG); k++) {
              int h = tid + k * WG;
              int2_t x = ((const GAS int2_t *)src)[h];
              double2_t y; y.x = (double)x.x; y.y = (double)x.y;
              ((double2_t *)dst)[h] = y;
            }
          } else {
#pragma unroll
            for (int k = 0; k < CHUNK / WG; k++) {
              int r = tid + k * WG;
              if (r < rows) dst[r] = (double)src[r];
            }
          }
          break;
        }
        case SN_K_I64: {
          const GAS long long *src = as_global((const long long *)col.body) + base;
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = __longlong_as_double(src[r]);
          }
          break;
        }
        case SN_K_F32: {
          const GAS float *src = as_global((const float *)col.body) + base;
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)src[r];
          }
          break;
        }
        case SN_K_I16: {
          const GAS int16_t *src = as_global((const int16_t *)col.body) + base;
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)src[r];
          }
          break;
        }
        case SN_K_DICT16: {
          const GAS int16_t *src = as_global((const int16_t *)col.body) + base;
          const GAS int32_t *dm = as_global(col.dictmap);
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)dm[(int)(uint16_t)src[r]];
          }
          break;
        }
        case SN_K_DICT32: {
          const GAS int32_t *src = as_global((const int32_t *)col.body) + base;
          const GAS int32_t *dm = as_global(col.dictmap);
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)dm[src[r]];
          }
          break;
        }
        case SN_K_BOOLBIT: {
          const uint64_t *src = (const uint64_t *)col.body;  /* via bm_get */
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)bm_get(src, base + r);
          }
          break;
        }
        case SN_K_U8: {
          const GAS uint8_t *src = as_global((const uint8_t *)col.body) + base;
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)(src[r] == 1);
          }
          break;
        }
        case SN_K_S8: {
          const GAS int8_t *src = as_global((const int8_t *)col.body) + base;
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = (double)src[r];
          }
          break;
        }
        case SN_K_F64C8: {
          const GAS uint8_t *src = as_global((const uint8_t *)col.body) + base;
          const GAS double *vd = as_global(col.rle_vals);
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = vd[src[r]];
          }
          break;
        }
        case SN_K_RLE:
        case SN_K_RLE_I64: {
          /* RLE_I64 run values are raw i64 bits as doubles — exactly the
           * i64 LDS-image convention, so the same copy is correct */
#pragma unroll
          for (int k = 0; k < CHUNK / WG; k++) {
            int r = tid + k * WG;
            if (r < rows) dst[r] = rle_value(col, base + r);
          }
          break;
        }
      }
    } else {
      uint64_t *vw = svalid + (size_t)c * (CHUNK / 64);
      const int is_dict = col.kind == SN_K_DICT16 || col.kind == SN_K_DICT32;
      const int is_i64 = col.kind == SN_K_I64 || col.kind == SN_K_RLE_I64;
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        int r = tid + k * WG;
        int row = base + r;
        int ok = 0;
        double vd = 0.0; long long vi = 0; int gid = col.null_gid;
        if (row < num_rows) ok = read_general(col, row, &vd, &vi, &gid);
        dst[r] = is_dict ? (double)gid : (is_i64 ? __longlong_as_double(vi) : vd);
        uint64_t w = __ballot(ok);
        if ((tid & 63) == 0) vw[r >> 6] = w;
      }
    }
  }
  if (!clean) {
    const uint64_t *del = b.del_bm;
#pragma unroll
    for (int k = 0; k < CHUNK / WG; k++) {
      int r = tid + k * WG;
      int row = base + r;
      int dead = (row >= num_rows) || (del && bm_get(del, row));
      uint64_t w = __ballot(dead);
      if ((tid & 63) == 0) sdead[r >> 6] = w;
    }
  }
  /* short chunks zero the image tail: sval beyond `rows` is raw LDS left by
   * whatever kernel ran last on this CU.  Every accumulator selects a dead
   * row's value away, so this is no longer what keeps a parked NaN pattern
   * (0xFFF8...) out of the sums; it keeps the values that the row phase
   * computes on defined. */
  if (rows < CHUNK) {
    for (int c = 0; c < nused; c++) {
      double *dst = sval + (size_t)c * CHUNK;
      for (int r = rows + tid; r < CHUNK; r += WG) dst[r] = 0.0;
    }
  }
}

/* ---- staged (software-pipelined) conversion for clean full chunks ----
 * T14 async-STAGE split: the NEXT chunk's global loads are issued into
 * registers right after the barrier that frees LDS, so they stay in flight
 * underneath the current chunk's row phase (the single biggest lever here:
 * SQ_WAIT_ANY was 75% of wave cycles with the unstaged conversion).
 * Raw loads are width-based (8/4/2 B); kind conversion happens at the LDS
 * write.  I64 shares the w8 path (its LDS image is the raw bits). */
/* per-tile register copy of the hot column-descriptor fields: reading
 * b.cols[c].body/kind per CHUNK emits serialized global_load_dword +
 * vmcnt(0) chains (measured: a fixed ~0.35 ms per query = the whole Q6
 * budget).  Copy once per tile into compile-time-indexed registers. */
struct ColRegs {
  const void *body;
  const int32_t *dictmap;
  int kind;
};

template <int NC>
__device__ __forceinline__ void hoist_cols(const sn_dev_batch &b, int nused,
                                           ColRegs (&cr)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; c++) {
    cr[c].body = c < nused ? b.cols[c].body : nullptr;
    cr[c].kind = c < nused ? b.cols[c].kind : -1;
    /* a code column keeps its value dictionary (doubles) in the map slot */
    cr[c].dictmap = c >= nused ? nullptr
        : cr[c].kind == SN_K_F64C8 ? (const int32_t *)b.cols[c].rle_vals
                                   : b.cols[c].dictmap;
  }
}

/* one shared register buffer for every width class (64 VGPRs total): raw
 * bits packed into double2 lanes; row mapping is pair-based for every width
 * (pair h = tid + p*WG covers rows 2h, 2h+1) */
template <int NC>
struct Stage {
  double2_t buf[NC][CHUNK / (2 * WG)];
};
__device__ __forceinline__ double pack_u64(unsigned lo, unsigned hi) {
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ int col_width_class(int kind) {
  switch (kind) {
    case SN_K_F64: case SN_K_I64: return 8;
    case SN_K_I32: case SN_K_F32: case SN_K_DICT32: return 4;
    case SN_K_I16: case SN_K_DICT16: return 2;
    case SN_K_F64C8: return 1;
    default: return 0;   /* BOOLBIT: not stageable */
  }
}

template <int NC, int NB>
__device__ __forceinline__ void stage_load(const ColRegs (&cr)[NC], int nused,
                                           int base, Stage<NB> &st) {
  static_assert(NB >= NC || NB == 1, "stage buffer too small");
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c >= nused) break;
    const ColRegs &col = cr[c];
    const int w = col_width_class(col.kind);
    if (w == 8) {
      const GAS double2_t *s2 = (const GAS double2_t *)
          as_global((const char *)col.body + (size_t)base * 8);
#pragma unroll
      for (int p = 0; p < CHUNK / (2 * WG); p++) st.buf[NB == 1 ? 0 : c][p] = s2[tid + p * WG];
    } else if (w == 4) {
      /* two int2 pair-loads -> raw bits in buf[c][0].x / .y */
      const GAS int2_t *s2 = (const GAS int2_t *)
          as_global((const char *)col.body + (size_t)base * 4);
      int2_t a0 = s2[tid], a1 = s2[tid + WG];
      st.buf[NB == 1 ? 0 : c][0].x = *(double *)&a0;
      st.buf[NB == 1 ? 0 : c][0].y = *(double *)&a1;
    } else if (w == 1) {
      /* two 2 B pair-loads -> packed into the low word of buf[c][0].x */
      const GAS unsigned short *s2 = (const GAS unsigned short *)
          as_global((const char *)col.body + (size_t)base);
      unsigned a0 = s2[tid], a1 = s2[tid + WG];
      st.buf[NB == 1 ? 0 : c][0].x = pack_u64(a0 | (a1 << 16), 0u);
    } else {
      /* two short2 (4 B) pair-loads -> packed into buf[c][0].x */
      const GAS unsigned *s2 = (const GAS unsigned *)
          as_global((const char *)col.body + (size_t)base * 2);
      unsigned a0 = s2[tid], a1 = s2[tid + WG];
      st.buf[NB == 1 ? 0 : c][0].x = pack_u64(a0, a1);
    }
  }
}

template <int NC, int NB>
__device__ __forceinline__ void stage_write(const ColRegs (&cr)[NC], int nused,
                                            Stage<NB> &st, double *sval) {
  static_assert(NB >= NC || NB == 1, "stage buffer too small");
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c >= nused) break;
    const ColRegs &col = cr[c];
    double *dst = sval + (size_t)c * CHUNK;
    switch (col.kind) {
      case SN_K_F64: case SN_K_I64:
#pragma unroll
        for (int p = 0; p < CHUNK / (2 * WG); p++)
          ((double2_t *)dst)[tid + p * WG] = st.buf[NB == 1 ? 0 : c][p];
        break;
      case SN_K_I32: case SN_K_F32: case SN_K_DICT32: {
        const GAS int32_t *dm = as_global(col.dictmap);
#pragma unroll
        for (int p = 0; p < CHUNK / (2 * WG); p++) {
          double raw = p == 0 ? st.buf[NB == 1 ? 0 : c][0].x : st.buf[NB == 1 ? 0 : c][0].y;
          int2_t a = *(int2_t *)&raw;
          double2_t y;
          if (col.kind == SN_K_I32) { y.x = (double)a.x; y.y = (double)a.y; }
          else if (col.kind == SN_K_F32) {
            float2 f = *(float2 *)&raw;
            y.x = (double)f.x; y.y = (double)f.y;
          } else { y.x = (double)dm[a.x]; y.y = (double)dm[a.y]; }
          ((double2_t *)dst)[tid + p * WG] = y;
        }
        break;
      }
      case SN_K_I16: case SN_K_DICT16: {
        const GAS int32_t *dm = as_global(col.dictmap);
        unsigned long long raw = __double_as_longlong(st.buf[NB == 1 ? 0 : c][0].x);
#pragma unroll
        for (int p = 0; p < CHUNK / (2 * WG); p++) {
          unsigned half = (unsigned)(raw >> (32 * p));
          int16_t e0 = (int16_t)(half & 0xffff), e1 = (int16_t)(half >> 16);
          double2_t y;
          if (col.kind == SN_K_I16) { y.x = (double)e0; y.y = (double)e1; }
          else {
            y.x = (double)dm[(int)(uint16_t)e0];
            y.y = (double)dm[(int)(uint16_t)e1];
          }
          ((double2_t *)dst)[tid + p * WG] = y;
        }
        break;
      }
      case SN_K_F64C8: {
        const GAS double *vd = (const GAS double *)as_global(col.dictmap);
        unsigned raw = (unsigned)__double_as_longlong(st.buf[NB == 1 ? 0 : c][0].x);
#pragma unroll
        for (int p = 0; p < CHUNK / (2 * WG); p++) {
          unsigned half = (raw >> (16 * p)) & 0xffffu;
          double2_t y;
          y.x = vd[half & 0xff];
          y.y = vd[half >> 8];
          ((double2_t *)dst)[tid + p * WG] = y;
        }
        break;
      }
      default: break;
    }
  }
}

/* can this batch use the staged pipeline? (clean + every col stageable) */
template <int NC>
__device__ __forceinline__ int batch_stageable(int clean, int nused,
                                               const ColRegs (&cr)[NC]) {
  if (!clean) return 0;
  int ok = 1;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c >= nused) break;
    ok &= col_width_class(cr[c].kind) != 0;
  }
  return ok;
}

/* predicate evaluation for row r (branchless; plan mirrored in LDS) */
__device__ __forceinline__ int eval_preds(const sn_dev_plan *P, int npd, int npi,
                                          int clean, const double *sval,
                                          const uint64_t *svalid,
                                          const uint64_t *sdead, int r) {
  int alive = clean ? 1 : !((sdead[r >> 6] >> (r & 63)) & 1ull);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i >= npd) break;
    const int cs = P->preds_d[i].cslot;
    const double x = sval[(size_t)cs * CHUNK + r];
    alive &= (x >= P->preds_d[i].lo) & (x <= P->preds_d[i].hi);
    if (!clean)
      alive &= (int)((svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)] >> (r & 63)) & 1ull);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npi) break;
    const int cs = P->preds_i[i].cslot;
    const long long x = __double_as_longlong(sval[(size_t)cs * CHUNK + r]);
    alive &= (x >= P->preds_i[i].lo) & (x <= P->preds_i[i].hi);
    if (!clean)
      alive &= (int)((svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)] >> (r & 63)) & 1ull);
  }
  return alive;
}

/* aggregate-factor read: i64 column slots hold RAW BITS in the LDS image
 * (so integer predicates stay exact); aggregate arithmetic is double, so
 * convert on read.  The mask test is scalar-uniform — a scalar branch,
 * free for plans without i64 factors. */
__device__ __forceinline__ double sv_agg(const sn_dev_plan *P,
                                         const double *sval, int cs, int r) {
  const double x = sval[(size_t)cs * CHUNK + r];
  const double xc = (double)__double_as_longlong(x);   /* select, not branch */
  return ((P->i64_mask >> cs) & 1u) ? xc : x;
}

/* aggregate input value: the product of the REAL factors only (A.nf is
 * wave-uniform, so these are scalar branches).  A neutral factor must not be
 * evaluated as (1 + 0*x): 0*x is NaN when x is NaN or +-inf, and COUNT(*)
 * (nf == 0) of a plan that references no column has no staged slot to read
 * at all.  Same rule as the query-compiled kernels (jit.cpp). */
__device__ __forceinline__ double eval_agg(const sn_dev_plan *P,
                                           const sn_dev_agg &A,
                                           const double *sval, int r) {
  if (A.nf < 1) return 1.0;
  double v = A.a0 + A.m0 * sv_agg(P, sval, A.c0, r);
  if (A.nf >= 2) v *= A.a1 + A.m1 * sv_agg(P, sval, A.c1, r);
  if (A.nf >= 3) v *= A.a2 + A.m2 * sv_agg(P, sval, A.c2, r);
  return v;
}

/* order-preserving double<->u64 for MIN/MAX accumulators (device twin of
 * sn_f64_ord_h): integer atomicMin/Max implement f64 min/max */
__device__ __forceinline__ unsigned long long f64_ord(double x) {
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
#define ORD_MIN_IDENT 0xFFF8000000000000ull   /* enc(+inf) < this; safe top */
#define ORD_MAX_IDENT 0x0000000000000000ull   /* below enc(-inf) */
/* the aggregates' ordering (non-finite aggregate inputs): every
 * NaN, whatever its sign and payload, is one value above +inf.  Its image is
 * that of the positive quiet NaN, which is also MIN's identity: a group of
 * NaNs alone leaves the cell there and decodes to NaN, its count says it is
 * not NULL. */
__device__ __forceinline__ unsigned long long f64_ord_agg(double x) {
  return x != x ? ORD_MIN_IDENT : f64_ord(x);
}

/* op-aware accumulate into an accumulator cell (LDS or global).
 * Sum cells hold plain doubles; min/max cells hold the ord-u64 encoding
 * bit-cast into the double slot. */
template <typename PTR>
__device__ __forceinline__ void acc_cell(PTR *cell, int op, double va) {
  if (op == 0) {
    (void)atomicAdd((double *)cell, va);
  } else if (op == 1) {
    (void)atomicMin((unsigned long long *)cell, f64_ord_agg(va));
  } else {
    (void)atomicMax((unsigned long long *)cell, f64_ord_agg(va));
  }
}

/* identity value (as raw double bits) for an accumulator cell */
__device__ __forceinline__ double acc_ident(int op) {
  if (op == 0) return 0.0;
  return __longlong_as_double(
      (long long)(op == 1 ? ORD_MIN_IDENT : ORD_MAX_IDENT));
}

/* per-agg factor validity on general batches: 1 when every referenced
 * factor column is non-null for row r (Spark Sum/Average skip null
 * inputs; COUNT(*) has nf == 0 and is always valid) */
__device__ __forceinline__ int agg_valid(const sn_dev_agg &A,
                                         const uint64_t *svalid, int r) {
  int ok = 1;
  if (A.nf >= 1)
    ok &= (int)((svalid[(size_t)A.c0 * (CHUNK / 64) + (r >> 6)] >> (r & 63)) & 1ull);
  if (A.nf >= 2)
    ok &= (int)((svalid[(size_t)A.c1 * (CHUNK / 64) + (r >> 6)] >> (r & 63)) & 1ull);
  if (A.nf >= 3)
    ok &= (int)((svalid[(size_t)A.c2 * (CHUNK / 64) + (r >> 6)] >> (r & 63)) & 1ull);
  return ok;
}

/* wave (64-lane) sum reduction */
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x += __shfl_down(x, off, 64);
  return x;
}

/* initialize the alive bitmap words (wave-owned: the wave that processes
 * rows [w*64, w*64+64) is the only writer of word w in every later pass) */
__device__ __forceinline__ void alive_init(uint64_t *salive,
                                           const uint64_t *sdead, int rows,
                                           int clean) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < CHUNK / WG; k++) {
    const int r = tid + k * WG;
    const int w = r >> 6;
    if ((tid & 63) == 0) {
      uint64_t aw = clean ? ~0ull : ~sdead[w];
      const int rbase = w << 6;
      if (rbase + 64 > rows)
        aw &= rows > rbase ? ((1ull << (rows - rbase)) - 1ull) : 0ull;
      salive[w] = aw;
    }
  }
}

/* fused sweep for <= 3 double predicates (the common fast path): one
 * traversal, params hoisted to ~20 registers, one alive-word RMW */
__device__ __forceinline__ void pred_sweep_fused(const sn_dev_plan *P, int npd,
                                                 int clean, const double *sval,
                                                 const uint64_t *svalid,
                                                 uint64_t *salive) {
  const int tid = threadIdx.x;
  double lo0 = -1e308, hi0 = 1e308, lo1 = lo0, hi1 = hi0, lo2 = lo0, hi2 = hi0;
  int c0 = 0, c1 = 0, c2 = 0;
  if (npd >= 1) { lo0 = P->preds_d[0].lo; hi0 = P->preds_d[0].hi; c0 = P->preds_d[0].cslot; }
  if (npd >= 2) { lo1 = P->preds_d[1].lo; hi1 = P->preds_d[1].hi; c1 = P->preds_d[1].cslot; }
  if (npd >= 3) { lo2 = P->preds_d[2].lo; hi2 = P->preds_d[2].hi; c2 = P->preds_d[2].cslot; }
#pragma unroll 2
  for (int k = 0; k < CHUNK / WG; k++) {
    const int r = tid + k * WG;
    const double x0 = sval[(size_t)c0 * CHUNK + r];
    const double x1 = sval[(size_t)c1 * CHUNK + r];
    const double x2 = sval[(size_t)c2 * CHUNK + r];
    int ok = (x0 >= lo0 && x0 <= hi0) &&
             (npd < 2 || (x1 >= lo1 && x1 <= hi1)) &&
             (npd < 3 || (x2 >= lo2 && x2 <= hi2));
    uint64_t w = __ballot(ok);
    if (!clean) {
      if (npd >= 1) w &= svalid[(size_t)c0 * (CHUNK / 64) + (r >> 6)];
      if (npd >= 2) w &= svalid[(size_t)c1 * (CHUNK / 64) + (r >> 6)];
      if (npd >= 3) w &= svalid[(size_t)c2 * (CHUNK / 64) + (r >> 6)];
    }
    if ((tid & 63) == 0) salive[r >> 6] &= w;
  }
}

/* IN-list membership sweep (bitmap LUT or sorted-list binary search) */
__device__ __forceinline__ void in_sweeps(const sn_dev_plan *P, int clean,
                                          const double *sval,
                                          const uint64_t *svalid,
                                          uint64_t *salive) {
  const int tid = threadIdx.x;
  for (int i = 0; i < P->npreds_in && i < 2; i++) {
    const int cs = P->inp[i].cslot;
    const int is64 = (int)((P->i64_mask >> cs) & 1u);
    const uint64_t *bm = P->inp[i].bm;
    const int64_t *list = P->inp[i].list;
    const long long base = P->inp[i].base;
    const long long lim = (long long)P->inp[i].nwords * 64;
    const int n = P->inp[i].n;
#pragma unroll
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const double x = sval[(size_t)cs * CHUNK + r];
      const long long v = is64 ? __double_as_longlong(x) : (long long)x;
      int ok;
      if (bm) {
        const long long idx = v - base;
        ok = idx >= 0 && idx < lim &&
             (int)((as_global(bm)[idx >> 6] >> (idx & 63)) & 1ull);
      } else {
        const GAS int64_t *ls = as_global(list);
        int lo = 0, hi = n - 1;
        ok = 0;
        while (lo <= hi) {
          const int mid = (lo + hi) >> 1;
          const long long m = (long long)ls[mid];
          if (m == v) { ok = 1; break; }
          if (m < v) lo = mid + 1; else hi = mid - 1;
        }
      }
      uint64_t w = __ballot(ok);
      if (!clean) w &= svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)];
      if ((tid & 63) == 0) salive[r >> 6] &= w;
    }
  }
}

/* one sweep per predicate, params hoisted; wave-owned word updates */
__device__ __forceinline__ void pred_sweeps(const sn_dev_plan *P, int npd,
                                            int npi, int clean,
                                            const double *sval,
                                            const uint64_t *svalid,
                                            uint64_t *salive) {
  const int tid = threadIdx.x;
  if (P->npreds_in > 0) in_sweeps(P, clean, sval, svalid, salive);
  if (npd <= 3 && npi == 0) {
    if (npd > 0) pred_sweep_fused(P, npd, clean, sval, svalid, salive);
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i >= npd) break;
    const int cs = P->preds_d[i].cslot;
    const double lo = P->preds_d[i].lo, hi = P->preds_d[i].hi;
#pragma unroll
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const double x = sval[(size_t)cs * CHUNK + r];
      uint64_t w = __ballot(x >= lo && x <= hi);
      if (!clean) w &= svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)];
      if ((tid & 63) == 0) salive[r >> 6] &= w;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npi) break;
    const int cs = P->preds_i[i].cslot;
    const long long lo = P->preds_i[i].lo, hi = P->preds_i[i].hi;
#pragma unroll
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const long long x = __double_as_longlong(sval[(size_t)cs * CHUNK + r]);
      uint64_t w = __ballot(x >= lo && x <= hi);
      if (!clean) w &= svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)];
      if ((tid & 63) == 0) salive[r >> 6] &= w;
    }
  }
}

/* broadcast-dimension probe sweep (HashJoinExec probe, device-side):
 * open-address linear-probe table in HBM (L2/L3-resident by the 100 MB
 * HashJoinSize design bound); filters alive and, for group-by-dim-attr
 * joins, assigns the group slot from the dimension payload. */
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97f4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ void probe_sweep(const sn_dev_plan *P, int clean,
                                            const double *sval,
                                            const uint64_t *svalid,
                                            uint64_t *salive,
                                            int16_t *sslot) {
  const int tid = threadIdx.x;
  const GAS long long *jk = (const GAS long long *)(uintptr_t)P->jkeys;
  const GAS int32_t *jp = (const GAS int32_t *)(uintptr_t)P->jpayload;
  const int cs = P->jcslot;
  const unsigned mask = (1u << P->jcap_log2) - 1;
  const int is_i64 = (P->i64_mask >> cs) & 1u;
  const GAS int32_t *lut = (const GAS int32_t *)(uintptr_t)P->jlut;
  const long long lmin = P->jlut_min, lmax = P->jlut_max;
#pragma unroll 2
  for (int k = 0; k < CHUNK / WG; k++) {
    const int r = tid + k * WG;
    const double xv = sval[(size_t)cs * CHUNK + r];
    const long long key = is_i64 ? __double_as_longlong(xv) : (long long)xv;
    int pay = -1;
    if (lut) {
      /* dense span: one dependent load, no hash chain */
      if (key >= lmin && key <= lmax) pay = lut[key - lmin];
    } else {
      unsigned h = (unsigned)mix64((unsigned long long)key) & mask;
      while (true) {
        long long k0 = jk[h];
        if (k0 == key) { pay = jp[h]; break; }
        if (k0 == LLONG_MIN) break;
        h = (h + 1) & mask;
      }
    }
    uint64_t w = __ballot(pay >= 0);
    /* a NULL key never joins: its image slot holds a 0, which may be a key */
    if (!clean) w &= svalid[(size_t)cs * (CHUNK / 64) + (r >> 6)];
    if ((tid & 63) == 0) salive[r >> 6] &= w;
    if (sslot) sslot[r] = (int16_t)(pay > 0 ? pay : 0);
  }
}

/* one key against the dimension, for the row scans (pass 1's probe_alive and
 * pass 2's attribute projection share it): the payload, or a negative value
 * when the key is absent.  Dense LUT when there is one, else the mix64
 * linear-probe chain up to the LLONG_MIN empty mark.  LLONG_MIN itself never
 * joins (it is no legal dimension key, and in the table it would "match" an
 * empty slot).  The walk visits at most every slot once. */
__device__ __forceinline__ int join_lookup(const GAS long long *jk,
                                           const GAS int32_t *jp,
                                           unsigned mask,
                                           const GAS int32_t *lut,
                                           long long lmin, long long lmax,
                                           long long key) {
  if (key == LLONG_MIN) return -1;
  if (lut) return key >= lmin && key <= lmax ? lut[key - lmin] : -1;
  unsigned h = (unsigned)mix64((unsigned long long)key) & mask;
  for (unsigned it = 0; it <= mask; ++it) {
    const long long k0 = jk[h];
    if (k0 == key) return jp[h];
    if (k0 == LLONG_MIN) break;
    h = (h + 1) & mask;
  }
  return -1;
}

/* join step of a row scan's pass 1, after the predicates: only rows that are
 * still alive are looked up (probe_sweep looks up every row of the chunk; at a
 * few percent selectivity nearly all of those dependent loads are wasted), and
 * a wave whose 64 rows are all dead skips its word.  joined = found & key
 * validity; INNER keeps the joined rows, ANTI the others.  Lane 0 of the
 * owning wave is the only reader and writer of an alive word, as everywhere. */
template <int ANTI>
__device__ __forceinline__ void probe_alive(const sn_dev_plan *P, int clean,
                                            const double *sval,
                                            const uint64_t *svalid,
                                            uint64_t *salive) {
  const int tid = threadIdx.x, lane = tid & 63;
  const GAS long long *jk = (const GAS long long *)(uintptr_t)P->jkeys;
  const GAS int32_t *jp = (const GAS int32_t *)(uintptr_t)P->jpayload;
  const GAS int32_t *lut = (const GAS int32_t *)(uintptr_t)P->jlut;
  const int cs = P->jcslot;
  const unsigned mask = (1u << P->jcap_log2) - 1;
  const int is_i64 = (P->i64_mask >> cs) & 1u;
  const long long lmin = P->jlut_min, lmax = P->jlut_max;
#pragma unroll
  for (int k = 0; k < CHUNK / WG; k++) {
    const int r = tid + k * WG, w = r >> 6;
    unsigned lo = 0, hi = 0;
    if (lane == 0) {
      const uint64_t a = salive[w];
      lo = (unsigned)a; hi = (unsigned)(a >> 32);
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    const uint64_t aw = ((uint64_t)hi << 32) | lo;
    if (aw == 0) continue;                         /* wave-uniform */
    int pay = -1;
    if ((aw >> lane) & 1ull) {
      const double xv = sval[(size_t)cs * CHUNK + r];
      const long long key = is_i64 ? __double_as_longlong(xv) : (long long)xv;
      pay = join_lookup(jk, jp, mask, lut, lmin, lmax, key);
    }
    uint64_t joined = __ballot(pay >= 0);
    /* a NULL key never joins: its image slot holds a 0, which may be a key */
    if (!clean) joined &= svalid[(size_t)cs * (CHUNK / 64) + w];
    if (lane == 0) salive[w] = aw & (ANTI ? ~joined : joined);
  }
}

/* ================= shared scan front end =================
 * Every scan kernel below is a row phase plugged into the same three pieces:
 * the LDS carve-up (scan_lds over engine_internal.h's sn_lds layout, which
 * the launchers size from), the tile/chunk driver (scan_tiles) and the
 * row-phase helpers (dense_slot, acc_row, hash_find_or_insert). */

/* copy a plan struct into its LDS mirror: row-phase field reads become
 * broadcast ds_reads instead of SGPR-spilled kernarg loads.  The caller
 * places the barrier. */
template <typename T>
__device__ __forceinline__ void lds_mirror(T *dst_, const T *src_g) {
  const GAS unsigned *src = (const GAS unsigned *)(uintptr_t)src_g;
  unsigned *dst = (unsigned *)dst_;
  for (unsigned i = threadIdx.x; i < sizeof(T) / 4; i += WG) dst[i] = src[i];
}

struct ScanLds {
  double *sval;
  uint64_t *svalid, *sdead, *salive;
  int16_t *sslot;        /* valid only for layouts with a slot image */
  sn_dev_plan *P;
  char *plan2, *acc;
};

/* carve the block's dynamic LDS by layout L */
__device__ __forceinline__ ScanLds scan_lds(char *smem, const sn_lds &L) {
  ScanLds S;
  S.sval = (double *)smem;
  S.svalid = (uint64_t *)(smem + L.svalid);
  S.sdead = (uint64_t *)(smem + L.sdead);
  S.salive = (uint64_t *)(smem + L.salive);
  S.sslot = (int16_t *)(smem + L.sslot);
  S.P = (sn_dev_plan *)(smem + L.plan);
  S.plan2 = smem + L.plan2;
  S.acc = smem + L.acc;
  return S;
}
/* ... and start the plan mirror copy */
__device__ __forceinline__ ScanLds scan_lds(char *smem, const sn_lds &L,
                                            const sn_dev_plan *plan_g) {
  const ScanLds S = scan_lds(smem, L);
  lds_mirror(S.P, plan_g);
  return S;
}

/* the tile/chunk driver: grid-stride over tiles; per tile hoist the column
 * descriptors and decide stageability; per chunk land the image in LDS
 * (staged registers or convert_chunk), barrier, issue the NEXT full chunk's
 * loads so they fly under the row phase, run row_phase(batch, base, rows,
 * clean), barrier.  STAGED = 0 drops the register pipeline (every chunk
 * through convert_chunk). */
template <int NC, int STAGED, typename RowPhase>
__device__ __forceinline__ void scan_tiles(
    const sn_dev_batch *__restrict__ batches,
    const sn_dev_tile *__restrict__ tiles, int ntiles, int nused,
    const ScanLds &S, RowPhase &&row_phase) {
  Stage<STAGED ? NC : 1> st;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int num_rows = b.num_rows;
    const int tile_end = min(tile.row_start + SN_TILE_ROWS, num_rows);
    const int clean = b.clean;
    [[maybe_unused]] ColRegs cr[NC];
    int pipe = 0, staged = 0;
    if constexpr (STAGED) {
      hoist_cols(b, nused, cr);
      pipe = batch_stageable(clean, nused, cr);
      if (pipe && tile.row_start + CHUNK <= tile_end) {
        stage_load(cr, nused, tile.row_start, st);
        staged = 1;
      }
    }
    for (int base = tile.row_start; base < tile_end; base += CHUNK) {
      const int rows = min(CHUNK, tile_end - base);
      if (STAGED && staged) {
        if constexpr (STAGED) stage_write(cr, nused, st, S.sval);
      } else {
        convert_chunk(b, nused, base, rows, num_rows, S.sval, S.svalid, S.sdead);
      }
      __syncthreads();
      /* prefetch the NEXT full chunk under this chunk's row phase */
      const int nbase = base + CHUNK;
      const int next_staged = pipe && nbase + CHUNK <= tile_end;
      if constexpr (STAGED) {
        if (next_staged) stage_load(cr, nused, nbase, st);
      }
      row_phase(b, base, rows, clean);
      __syncthreads();
      staged = next_staged;
    }
  }
}
/* a row phase: ROW_PHASE(captures) { ... }.  Capture scalars by value and
 * only the kernel's register accumulators by reference where a kernel sits
 * at its register ceiling. */
#define ROW_PHASE(...) [__VA_ARGS__](const sn_dev_batch &b, int base, \
                                     int rows, int clean)              \
    __attribute__((always_inline))

/* dense group slot of row r: ((v0 - gbase[0]) * gmul0) + (v1 - gbase[1]);
 * T is the slot width the kernel's accumulator indexing uses */
template <typename T>
__device__ __forceinline__ T dense_slot(const sn_dev_plan *P,
                                        const double *sval, int ngroup,
                                        int gc0, int gc1, int r) {
  T slot = 0;
  if (ngroup >= 1)
    slot = (T)(((long long)sval[(size_t)gc0 * CHUNK + r] - P->gbase[0]) *
               P->gmul0);
  if (ngroup >= 2)
    slot += (T)((long long)sval[(size_t)gc1 * CHUNK + r] - P->gbase[1]);
  return slot;
}
/* composite GROUP BY dim_attr, fact_col: the probed attr gid widened by the
 * dense fact-slot space */
template <typename T>
__device__ __forceinline__ T join_slot(const sn_dev_plan *P, const double *sval,
                                       int pay, int gc0, int r) {
  return (T)pay * P->jslot_mul +
         (T)((long long)sval[(size_t)gc0 * CHUNK + r] - P->gbase[0]);
}
/* slot of a live row in the kernels that derive it per row: from the join
 * payload image (jslot), alone or composite, else from the key columns */
template <typename T>
__device__ __forceinline__ T row_slot(const sn_dev_plan *P, const ScanLds &S,
                                      int jslot, int ngroup, int gc0, int gc1,
                                      int r) {
  if (!jslot) return dense_slot<T>(P, S.sval, ngroup, gc0, gc1, r);
  const int pay = S.sslot[r];
  return ngroup >= 1 ? join_slot<T>(P, S.sval, pay, gc0, r) : (T)pay;
}

/* accumulate live row r into its accumulator row (LDS or global):
 * [aggregates naggs][per-agg counts naggs, pac only][rowcount] */
template <typename PTR>
__device__ __forceinline__ void acc_row(PTR *row_acc, const sn_dev_plan *P,
                                        int naggs, int na1, int pac, int clean,
                                        const double *sval,
                                        const uint64_t *svalid, int r) {
  for (int a = 0; a < naggs; a++) {
    const sn_dev_agg &A = P->aggs[a];
    if (pac) {
      const int av = clean ? 1 : agg_valid(A, svalid, r);
      if (!av) continue;
      (void)atomicAdd((double *)&row_acc[naggs + a], 1.0);
    }
    acc_cell(&row_acc[a], A.op, eval_agg(P, A, sval, r));
  }
  (void)atomicAdd((double *)&row_acc[na1 - 1], 1.0);
}

/* open-address find-or-insert of `key` (never SN_HASH_EMPTY) in a table of
 * mask + 1 keys (global table, global segment or LDS); returns its index, or
 * -1 when the table is full.  `fill`, when given, counts the inserts so the
 * host can grow the table BEFORE load factor makes linear probing
 * pathological. */
template <typename KEYS>
__device__ __forceinline__ int hash_find_or_insert(KEYS keys, unsigned mask,
                                                   long long key,
                                                   GAS int32_t *fill) {
  unsigned h = (unsigned)mix64((unsigned long long)key) & mask;
  for (unsigned it = 0; it <= mask; ++it) {
    const long long k0 = keys[h];
    if (k0 == key) return (int)h;
    if (k0 == SN_HASH_EMPTY) {
      const long long old = (long long)atomicCAS(
          (unsigned long long *)&keys[h], (unsigned long long)SN_HASH_EMPTY,
          (unsigned long long)key);
      if (old == SN_HASH_EMPTY) {
        if (fill) (void)atomicAdd((int *)fill, 1);
        return (int)h;
      }
      if (old == key) return (int)h;
      /* lost the insert race to a DIFFERENT key: step on */
    }
    h = (h + 1) & mask;
  }
  return -1;
}

/* ================= keyless kernel ================= */
template <int NAGGS, int NC>
__launch_bounds__(WG, NAGGS <= 4 ? 4 : 2)
__global__ void k_keyless(sn_dev_plan plan,
                          const sn_dev_plan *__restrict__ plan_g,
                          const sn_dev_batch *__restrict__ batches,
                          const sn_dev_tile *__restrict__ tiles, int ntiles,
                          double *__restrict__ out /* [2*NAGGS+1] */) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_keyless(nused), plan_g);
  const sn_dev_plan *P = S.P;
  double *const sval = S.sval;
  uint64_t *const svalid = S.svalid, *const salive = S.salive;

  double sums[NAGGS], cnts[NAGGS], rcnt = 0.0;
#pragma unroll
  for (int a = 0; a < NAGGS; a++) { sums[a] = 0.0; cnts[a] = 0.0; }
  const int naggs = plan.naggs;
  const int npd = plan.npreds_d, npi = plan.npreds_i;

  scan_tiles<NC, 1>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
    /* fully-fused single pass (clean chunks, <=3 double preds, no join):
     * one traversal computes predicates, aggregates and counts — the
     * minimal LDS-read structure (matches the membw probe's shape) */
    if (clean && npd <= 3 && npi == 0 && !plan.jkeys &&
        plan.npreds_in == 0) {
      double lo0 = -1e308, hi0 = 1e308, lo1 = lo0, hi1 = hi0, lo2 = lo0, hi2 = hi0;
      int c0 = 0, c1 = 0, c2 = 0;
      if (npd >= 1) { lo0 = P->preds_d[0].lo; hi0 = P->preds_d[0].hi; c0 = P->preds_d[0].cslot; }
      if (npd >= 2) { lo1 = P->preds_d[1].lo; hi1 = P->preds_d[1].hi; c1 = P->preds_d[1].cslot; }
      if (npd >= 3) { lo2 = P->preds_d[2].lo; hi2 = P->preds_d[2].hi; c2 = P->preds_d[2].cslot; }
#pragma unroll 2
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        const int inr = r < rows;
        const double x0 = sval[(size_t)c0 * CHUNK + r];
        const double x1 = sval[(size_t)c1 * CHUNK + r];
        const double x2 = sval[(size_t)c2 * CHUNK + r];
        const int ok = inr &&
            (npd < 1 || (x0 >= lo0 && x0 <= hi0)) &&
            (npd < 2 || (x1 >= lo1 && x1 <= hi1)) &&
            (npd < 3 || (x2 >= lo2 && x2 <= hi2));
        if (__popcll(__ballot(ok)) == 0) continue;
#pragma unroll
        for (int a = 0; a < NAGGS; a++) {
          if (a >= naggs) break;
          const double va = eval_agg(P, P->aggs[a], sval, r);
          sums[a] += ok ? va : 0.0;
          cnts[a] += ok ? 1.0 : 0.0;
        }
        rcnt += ok ? 1.0 : 0.0;
      }
      return;
    }

    /* ---- row phase as sweep passes: each wave owns its 64-row words of
     * the alive bitmap, so pred/agg passes need no barriers; plan params
     * hoisted per pass (row-invariant LDS reads once, not per row) ---- */
    alive_init(salive, S.sdead, rows, clean);
    pred_sweeps(P, npd, npi, clean, sval, svalid, salive);
    if (plan.jkeys) probe_sweep(P, clean, sval, svalid, salive, nullptr);
#pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      if (a >= naggs) break;
      const sn_dev_agg A = P->aggs[a];
#pragma unroll 2
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        uint64_t w = salive[r >> 6];
        if (!clean) {
          if (A.nf >= 1) w &= svalid[(size_t)A.c0 * (CHUNK / 64) + (r >> 6)];
          if (A.nf >= 2) w &= svalid[(size_t)A.c1 * (CHUNK / 64) + (r >> 6)];
          if (A.nf >= 3) w &= svalid[(size_t)A.c2 * (CHUNK / 64) + (r >> 6)];
        }
        if (w == 0) continue;
        const int m = (int)((w >> (tid & 63)) & 1ull);
        const double val = eval_agg(P, A, sval, r);
        sums[a] += m ? val : 0.0;
        cnts[a] += m ? 1.0 : 0.0;
      }
    }
#pragma unroll 2
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      rcnt += (double)((salive[r >> 6] >> (tid & 63)) & 1ull);
    }
  });

  /* block partials to scratch (plain stores) — per-wave atomicAdd to the
   * same few global addresses serialized at ~45ns each (8K+ per address =
   * a fixed ~0.35 ms per query); a tiny reduce kernel sums the partials.
   * The row is [sums na_t][counts na_t][rowcount] with na_t the result
   * stride's aggregate count, which the <12, *> instances serve at both
   * 8 and 12. */
  double *bacc = (double *)S.acc;
  {
    const int na_t = NAGGS <= 4 ? NAGGS : sn_na_t(naggs);
    const int NV = 2 * na_t + 1;
    for (int i = tid; i < NV; i += WG) bacc[i] = 0.0;
    __syncthreads();
    /* (no early exit on a >= na_t: a runtime trip count would leave the
     * loop rolled and sums[] in scratch; those partials are zero anyway) */
#pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      const int lead = (tid & 63) == 0 && a < na_t;
      double x = wave_sum(sums[a]);
      if (lead && x != 0.0) atomicAdd(bacc + a, x);
      x = wave_sum(cnts[a]);
      if (lead && x != 0.0) atomicAdd(bacc + na_t + a, x);
    }
    double x = wave_sum(rcnt);
    if ((tid & 63) == 0 && x != 0.0) atomicAdd(bacc + 2 * na_t, x);
    __syncthreads();
    for (int i = tid; i < NV; i += WG)
      out[(size_t)blockIdx.x * NV + i] = bacc[i];
  }
}

/* ================= grouped kernel =================
 * Aggregates processed in groups of AGRP with per-lane sums[NSLOTS][AGRP]
 * registers; after each chunk the registers wave-reduce into the LDS block
 * accumulator (nslots x (naggs+1)), which flushes once per block to global
 * atomics.  Requires non-nullable aggregate inputs (engine-validated);
 * output layout [slot][2*NA+1]: sums, counts(=rowcount written host-side),
 * rowcount. */
template <int NSLOTS, int NC>
__launch_bounds__(WG, 2)
__global__ void k_grouped(sn_dev_plan plan,
                          const sn_dev_plan *__restrict__ plan_g,
                          const sn_dev_batch *__restrict__ batches,
                          const sn_dev_tile *__restrict__ tiles, int ntiles,
                          double *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int naggs = plan.naggs, ngroup = plan.ngroup;
  const int npd = plan.npreds_d, npi = plan.npreds_i;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_grouped(nused, NSLOTS, naggs), plan_g);
  const sn_dev_plan *P = S.P;
  double *const sval = S.sval;
  uint64_t *const svalid = S.svalid, *const salive = S.salive;
  int16_t *const sslot = S.sslot;
  /* block accumulator: [NSLOTS][naggs+1], init once */
  double *bacc = (double *)S.acc;
  for (int i = tid; i < NSLOTS * (naggs + 1); i += WG) bacc[i] = 0.0;
  __syncthreads();

  scan_tiles<NC, 1>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
      /* pass A: alive bitmap via sweeps + slot per row (wave-owned words,
       * no barrier needed before this block's own later passes) */
      alive_init(salive, S.sdead, rows, clean);
      pred_sweeps(P, npd, npi, clean, sval, svalid, salive);
      if (plan.jkeys) {
        /* join: filter by probe; group-by-dim-attr takes its slot from the
         * dimension payload */
        probe_sweep(P, clean, sval, svalid, salive,
                    plan.jmode == 1 ? sslot : nullptr);
      }
      if (!(plan.jkeys && plan.jmode == 1)) {
        const int gc0 = plan.gcol[0], gc1 = plan.gcol[1];
#pragma unroll
        for (int k = 0; k < CHUNK / WG; k++) {
          const int r = tid + k * WG;
          sslot[r] = (int16_t)dense_slot<int>(P, sval, ngroup, gc0, gc1, r);
        }
      } else if (ngroup >= 1) {
        /* composite GROUP BY dim_attr, fact_col: probe_sweep staged the
         * attr gid (dead rows keep garbage slots — they are never
         * accumulated) */
        const int gc0 = plan.gcol[0];
#pragma unroll
        for (int k = 0; k < CHUNK / WG; k++) {
          const int r = tid + k * WG;
          sslot[r] = (int16_t)join_slot<int>(P, sval, sslot[r], gc0, r);
        }
      }

      /* rowcount per slot */
      {
        double rc[NSLOTS];
#pragma unroll
        for (int s = 0; s < NSLOTS; s++) rc[s] = 0.0;
#pragma unroll 2
        for (int k = 0; k < CHUNK / WG; k++) {
          int r = tid + k * WG;
          int alive = (int)((salive[r >> 6] >> (r & 63)) & 1ull);
          int slot = sslot[r];
#pragma unroll
          for (int s = 0; s < NSLOTS; s++)
            rc[s] += (alive && slot == s) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int s = 0; s < NSLOTS; s++) {
          double x = wave_sum(rc[s]);
          if ((tid & 63) == 0 && x != 0.0)
            atomicAdd(&bacc[s * (naggs + 1) + naggs], x);
        }
      }

      /* pass B: aggregate PAIRS per sweep, params hoisted, slot-predicated
       * register accumulators (2 x NSLOTS live at a time) */
      for (int a0 = 0; a0 < naggs; a0 += 2) {
        const sn_dev_agg A = P->aggs[a0];
        const int has2 = a0 + 1 < naggs;
        const sn_dev_agg B2 = P->aggs[has2 ? a0 + 1 : a0];
        double sa[NSLOTS], sb[NSLOTS];
#pragma unroll
        for (int s = 0; s < NSLOTS; s++) { sa[s] = 0.0; sb[s] = 0.0; }
#pragma unroll 4
        for (int k = 0; k < CHUNK / WG; k++) {
          const int r = tid + k * WG;
          const uint64_t w = salive[r >> 6];
          if (w == 0) continue;
          const int m = (int)((w >> (tid & 63)) & 1ull);
          const int slot = sslot[r];
          const double va = eval_agg(P, A, sval, r);
          const double vb = eval_agg(P, B2, sval, r);
#pragma unroll
          for (int s = 0; s < NSLOTS; s++) {
            /* select + add: a row adds to its own slot alone and a dead row
             * to none.  (fma(0 or 1, x, acc) is one op less, but
             * fma(0, +-inf or NaN, acc) is NaN: one such value, of a
             * filtered row included, turned every slot of the lane NaN.) */
            const bool mine = m && slot == s;
            sa[s] += mine ? va : 0.0;
            sb[s] += mine ? vb : 0.0;
          }
        }
#pragma unroll
        for (int s = 0; s < NSLOTS; s++) {
          double x = wave_sum(sa[s]);
          if ((tid & 63) == 0 && x != 0.0)
            atomicAdd(&bacc[s * (naggs + 1) + a0], x);
          if (has2) {
            x = wave_sum(sb[s]);
            if ((tid & 63) == 0 && x != 0.0)
              atomicAdd(&bacc[s * (naggs + 1) + a0 + 1], x);
          }
        }
      }
  });

  /* flush block accumulator to a per-block scratch row (plain stores);
   * the reduce kernel folds rows into the final [slot][stride] layout.
   * Row width uses the RUNTIME slot count (the engine sizes scratch by it;
   * the template NSLOTS is only the register-capacity ceiling). */
  __syncthreads();
  const int NV = plan.nslots * (naggs + 1);
  for (int i = tid; i < NV; i += WG)
    out[(size_t)blockIdx.x * NV + i] = bacc[i];
}

/* ---- LDS-accumulator grouped kernel (large slot counts: 17..1024) ----
 * The ByteBufferHashMap/SHAMap analogue for dictionary group keys: the
 * premultiplied global dictionary id IS the table slot (the reference's
 * DictionaryOptimizedMapAccessor direct-array idea scaled up), and the
 * per-block accumulator lives in LDS with f64 atomics — collisions are
 * per-wave lanes hitting one slot, rare at high cardinality.  One LDS
 * accumulator per block accumulates across all its tiles and flushes to a
 * per-block scratch row at the end (grid is capped so scratch stays small).
 * Open-address hashing of arbitrary (non-dictionary) keys is round-2. */
__global__ __launch_bounds__(WG, 1)
void k_grouped_lds(sn_dev_plan plan,
                   const sn_dev_plan *__restrict__ plan_g,
                   const sn_dev_batch *__restrict__ batches,
                   const sn_dev_tile *__restrict__ tiles, int ntiles,
                   double *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int naggs = plan.naggs, ngroup = plan.ngroup;
  const int npd = plan.npreds_d, npi = plan.npreds_i;
  const int nslots = plan.nslots;
  /* pac: accumulator rows widen to [sums][per-agg counts][rowcount] */
  const int pac = plan.pac;
  const int na1 = pac ? 2 * naggs + 1 : naggs + 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S =
      scan_lds(smem, sn_lds_grouped_lds(nused, nslots, na1), plan_g);
  const sn_dev_plan *P = S.P;
  double *bacc = (double *)S.acc;   /* [nslots][na1] */
  /* min/max cells initialize to their ord-encoding identity (read ops from
   * the by-value plan — the LDS mirror copy has no barrier yet) */
  const int NV = nslots * na1;
  for (int i = tid; i < NV; i += WG) {
    const int a = i % na1;
    bacc[i] = a < naggs ? acc_ident(plan.aggs[a].op) : 0.0;
  }
  __syncthreads();

  const int gc0 = plan.gcol[0], gc1 = plan.gcol[1];
  const int jslot = plan.jkeys && plan.jmode == 1;
  scan_tiles<1, 0>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
    alive_init(S.salive, S.sdead, rows, clean);
    pred_sweeps(P, npd, npi, clean, S.sval, S.svalid, S.salive);
    if (plan.jkeys)
      probe_sweep(P, clean, S.sval, S.svalid, S.salive,
                  jslot ? S.sslot : nullptr);

#pragma unroll 2
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const uint64_t w = S.salive[r >> 6];
      if (w == 0) continue;
      const int m = (int)((w >> (tid & 63)) & 1ull);
      if (!m) continue;
      const int slot = row_slot<int>(P, S, jslot, ngroup, gc0, gc1, r);
      acc_row(bacc + (size_t)slot * na1, P, naggs, na1, pac, clean, S.sval,
              S.svalid, r);
    }
  });

  __syncthreads();
  for (int i = tid; i < NV; i += WG)
    out[(size_t)blockIdx.x * NV + i] = bacc[i];
}

/* ---- register-accumulator grouped kernel (small shapes: NSLOTS x NA
 * accumulators live across the WHOLE kernel) ----
 * The sweep kernel's per-chunk wave reductions made it LDS-latency-bound
 * (measured: 61% of wave cycles parked, LDS array 40% busy, HBM 12%).
 * Here each lane accumulates slot-predicated sums in registers through all
 * tiles and reduces ONCE at kernel end, one LDS read per referenced value
 * per row.  Dict-group plans with nslots <= NSLOTS and deduped aggs <= NA;
 * join-group and larger shapes use k_grouped. */
template <int NSLOTS, int NA, int NC, int STAGED = 1>
__launch_bounds__(WG, STAGED ? 2 : 3)
__global__ void k_grouped_reg(sn_dev_plan plan,
                              const sn_dev_plan *__restrict__ plan_g,
                              const sn_dev_batch *__restrict__ batches,
                              const sn_dev_tile *__restrict__ tiles, int ntiles,
                              double *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int naggs = plan.naggs, ngroup = plan.ngroup;
  const int npd = plan.npreds_d, npi = plan.npreds_i;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_grouped_reg(nused, naggs), plan_g);
  const sn_dev_plan *P = S.P;
  double *const sval = S.sval;
  uint64_t *const svalid = S.svalid, *const salive = S.salive;
  double *bacc = (double *)S.acc;
  __syncthreads();

  const int gc0 = plan.gcol[0], gc1 = plan.gcol[1];

  double sums[NSLOTS][NA];
  double rc[NSLOTS];
#pragma unroll
  for (int s = 0; s < NSLOTS; s++) {
    rc[s] = 0.0;
#pragma unroll
    for (int a = 0; a < NA; a++) sums[s][a] = 0.0;
  }

  scan_tiles<NC, STAGED>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
      const int inline_preds = clean && npi == 0 && !plan.jkeys &&
                               plan.npreds_in == 0;
      if (!inline_preds) {
        alive_init(salive, S.sdead, rows, clean);
        pred_sweeps(P, npd, npi, clean, sval, svalid, salive);
        if (plan.jkeys) probe_sweep(P, clean, sval, svalid, salive, nullptr);
      }

#pragma unroll 2
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        int m;
        if (inline_preds) {
          m = r < rows;
          for (int i = 0; i < npd; i++) {
            const double x = sval[(size_t)P->preds_d[i].cslot * CHUNK + r];
            m &= (x >= P->preds_d[i].lo) & (x <= P->preds_d[i].hi);
          }
          if (__popcll(__ballot(m)) == 0) continue;
        } else {
          const uint64_t w = salive[r >> 6];
          if (w == 0) continue;
          m = (int)((w >> (tid & 63)) & 1ull);
        }
        const int slot = dense_slot<int>(P, sval, ngroup, gc0, gc1, r);
        double va[NA];
#pragma unroll
        for (int a = 0; a < NA; a++) {
          if (a >= naggs) { va[a] = 0.0; continue; }
          va[a] = eval_agg(P, P->aggs[a], sval, r);
        }
#pragma unroll
        for (int s = 0; s < NSLOTS; s++) {
          /* select + add, not fma(0 or 1, va, sum): see k_grouped */
          const bool mine = m && slot == s;
          rc[s] += mine ? 1.0 : 0.0;
#pragma unroll
          for (int a = 0; a < NA; a++)
            sums[s][a] += mine ? va[a] : 0.0;
        }
      }
  });

  /* final block reduction into a scratch row (like the keyless kernel) */
  const int NV = plan.nslots * (naggs + 1);
  for (int i = tid; i < NV; i += WG) bacc[i] = 0.0;
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NSLOTS; s++) {
    if (s >= plan.nslots) break;
#pragma unroll
    for (int a = 0; a < NA + 1; a++) {
      if (a > naggs) break;
      double x = wave_sum(a < naggs && a < NA ? sums[s][a] : rc[s]);
      if ((tid & 63) == 0 && x != 0.0)
        atomicAdd(&bacc[s * (naggs + 1) + (a < naggs ? a : naggs)], x);
    }
  }
  __syncthreads();
  for (int i = tid; i < NV; i += WG)
    out[(size_t)blockIdx.x * NV + i] = bacc[i];
}

/* ---- unbounded-cardinality grouped scan (the SHAMap-overflow analogue):
 * accumulates straight into a GLOBAL [nslots][naggs+1] array with f64
 * atomics (zeroed by the host).  High cardinality means low per-address
 * contention, which is exactly when global atomics are cheap; the slot
 * space is still dense (dictionary ids / stats-ranged integers). ---- */
__global__ __launch_bounds__(WG, 1)
void k_grouped_global(sn_dev_plan plan,
                      const sn_dev_plan *__restrict__ plan_g,
                      const sn_dev_batch *__restrict__ batches,
                      const sn_dev_tile *__restrict__ tiles, int ntiles,
                      double *__restrict__ gacc) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int naggs = plan.naggs, ngroup = plan.ngroup;
  const int npd = plan.npreds_d, npi = plan.npreds_i;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_grouped_global(nused), plan_g);
  const sn_dev_plan *P = S.P;
  __syncthreads();

  /* 8-way XCD privatization (see the JIT twin): fold happens in k_reduce */
  const int pac = plan.pac;
  const int na1 = pac ? 2 * naggs + 1 : naggs + 1;
  GAS double *acc = (GAS double *)(uintptr_t)gacc +
                    (size_t)(blockIdx.x & 7) * (size_t)plan.nslots * na1;
  const int gc0 = plan.gcol[0], gc1 = plan.gcol[1];
  const int jslot = plan.jkeys && plan.jmode == 1;
  scan_tiles<1, 0>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
    alive_init(S.salive, S.sdead, rows, clean);
    pred_sweeps(P, npd, npi, clean, S.sval, S.svalid, S.salive);
    if (plan.jkeys)
      probe_sweep(P, clean, S.sval, S.svalid, S.salive,
                  jslot ? S.sslot : nullptr);

#pragma unroll 2
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const uint64_t w = S.salive[r >> 6];
      if (w == 0) continue;
      const int m = (int)((w >> (tid & 63)) & 1ull);
      if (!m) continue;
      const long long slot =
          row_slot<long long>(P, S, jslot, ngroup, gc0, gc1, r);
      acc_row(acc + (size_t)slot * na1, P, naggs, na1, pac, clean, S.sval,
              S.svalid, r);
    }
  });
}

/* ---- sparse-key open-address hash aggregate ----
 * The ByteBufferHashMap / SHAMapAccessor analogue for integer group keys
 * WITHOUT dense-slot structure (ByteBufferHashMap.putBufferIfAbsent,
 * ByteBufferHashMap.scala:140-183 — open addressing, hash+key probe,
 * append-on-miss; SHAMapAccessor.generateMapGetOrInsert,
 * SHAMapAccessor.scala:716-830).  Instead of the JVM's byte-buffer value
 * records, the device keeps an open-address KEY array in HBM (sentinel
 * SN_HASH_EMPTY, atomicCAS insert) whose probe position IS the accumulator row
 * index — high key cardinality means low per-address contention, exactly
 * when HBM f64 atomics are cheap (same argument as k_grouped_global). */
__device__ __forceinline__ long long sparse_key(const sn_dev_plan *P,
                                                const double *sval, int r) {
  const int gc0 = P->gcol[0];
  if (P->ngroup == 1) {
    const double x = sval[(size_t)gc0 * CHUNK + r];
    return ((P->i64_mask >> gc0) & 1u) ? __double_as_longlong(x)
                                       : (long long)x;
  }
  /* two <=32-bit keys packed into one i64 (reversible; a pack that lands
   * exactly on the sentinel routes to the reserved row like any other) */
  const unsigned k0 = (unsigned)(int)sval[(size_t)gc0 * CHUNK + r];
  const unsigned k1 = (unsigned)(int)sval[(size_t)P->gcol[1] * CHUNK + r];
  return (long long)(((unsigned long long)k0 << 32) | k1);
}

__global__ __launch_bounds__(WG, 1)
void k_grouped_hash(sn_dev_plan plan,
                    const sn_dev_plan *__restrict__ plan_g,
                    const sn_dev_batch *__restrict__ batches,
                    const sn_dev_tile *__restrict__ tiles, int ntiles) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int naggs = plan.naggs;
  const int npd = plan.npreds_d, npi = plan.npreds_i;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_hash(nused), plan_g);
  const sn_dev_plan *P = S.P;
  __syncthreads();

  const int pac = plan.pac;
  const int na1 = pac ? 2 * naggs + 1 : naggs + 1;
  GAS double *acc = (GAS double *)(uintptr_t)plan.hacc;
  GAS long long *hk = (GAS long long *)(uintptr_t)plan.hkeys;
  GAS int32_t *flags = (GAS int32_t *)(uintptr_t)plan.hflags;
  const int cap = 1 << plan.hcap_log2;
  scan_tiles<1, 0>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
    alive_init(S.salive, S.sdead, rows, clean);
    pred_sweeps(P, npd, npi, clean, S.sval, S.svalid, S.salive);
    /* not reachable today: the engine rejects a join combined with sparse
     * group keys before it picks this kernel, so no test probes from here */
    if (plan.jkeys) probe_sweep(P, clean, S.sval, S.svalid, S.salive, nullptr);

#pragma unroll 2
    for (int k = 0; k < CHUNK / WG; k++) {
      const int r = tid + k * WG;
      const uint64_t w = S.salive[r >> 6];
      if (w == 0) continue;
      const int m = (int)((w >> (tid & 63)) & 1ull);
      if (!m) continue;
      /* a NULL key routes to the dedicated null-group row at cap+1
       * (nullable keys are single-column by the engine contract) */
      int kvalid = 1;
      if (!clean)
        kvalid = (int)((S.svalid[(size_t)plan.gcol[0] * (CHUNK / 64) +
                                 (r >> 6)] >> (r & 63)) & 1ull);
      int slot;
      if (!kvalid) {
        slot = cap + 1;
      } else {
        const long long key = sparse_key(P, S.sval, r);
        /* a REAL key of -1 lands in the reserved row at cap */
        slot = key == SN_HASH_EMPTY
                   ? cap
                   : hash_find_or_insert(hk, (unsigned)cap - 1, key, flags + 2);
        if (slot < 0) {                   /* table full: host grows, retries */
          atomicOr((int *)flags, 1);
          continue;
        }
      }
      acc_row(acc + (size_t)slot * na1, P, naggs, na1, pac, clean, S.sval,
              S.svalid, r);
    }
  });
}

/* ---- device-side join-table build (the partitioned-partitioned /
 * colocated join's HashedObjectCache analogue, HashJoinExec.scala:285-520,
 * ObjectHashSet.scala:107-135): scan the BUILD-side column table's batches
 * and insert (key -> payload gid) into an open-address table with the SAME
 * layout probe_sweep consumes (sentinel LLONG_MIN).  Colocated partitioned
 * tables join bucket-locally in the reference (GemFire colocation), so no
 * exchange step exists on this path. ---- */
__global__ void k_fill_i64(long long *dst, long long n, long long v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ((GAS long long *)(uintptr_t)dst)[i] = v;
}

/* flags: [0] = duplicate key with conflicting payload / key == sentinel,
 * [1] = table full */
__global__ __launch_bounds__(WG, 2)
void k_join_build(sn_dev_plan plan,
                  const sn_dev_batch *__restrict__ batches,
                  const sn_dev_tile *__restrict__ tiles, int ntiles,
                  long long *__restrict__ hk_, int32_t *__restrict__ hp_,
                  int cap_log2, int has_attr, int32_t *__restrict__ flags_) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  GAS long long *hk = (GAS long long *)(uintptr_t)hk_;
  GAS int32_t *hp = (GAS int32_t *)(uintptr_t)hp_;
  GAS int32_t *flags = (GAS int32_t *)(uintptr_t)flags_;
  const unsigned mask = (1u << cap_log2) - 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_join_build(nused));
  double *const sval = S.sval;
  uint64_t *const salive = S.salive;

  scan_tiles<1, 0>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
      alive_init(salive, S.sdead, rows, clean);
      if (!clean) {
        /* null build keys never join (SQL equality) */
#pragma unroll
        for (int k = 0; k < CHUNK / WG; k++) {
          const int r = tid + k * WG;
          uint64_t w = S.svalid[(size_t)0 * (CHUNK / 64) + (r >> 6)];
          if ((tid & 63) == 0) salive[r >> 6] &= w;
        }
      }
#pragma unroll 2
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        const uint64_t w = salive[r >> 6];
        if (w == 0) continue;
        if (!((w >> (tid & 63)) & 1ull)) continue;
        const double kx = sval[r];
        const long long key = ((plan.i64_mask >> 0) & 1u)
                                  ? __double_as_longlong(kx)
                                  : (long long)kx;
        const int32_t pay = has_attr ? (int32_t)sval[(size_t)1 * CHUNK + r] : 0;
        if (key == LLONG_MIN) { atomicOr((int *)&flags[0], 1); continue; }
        unsigned h = (unsigned)mix64((unsigned long long)key) & mask;
        int done = 0;
        /* payload publication: the inserter CASes the key then atomically
         * exchanges the payload over the INT32_MIN sentinel; a concurrent
         * duplicate spins (bounded) until the payload is visible before
         * checking for a conflict */
        for (unsigned it = 0; it <= mask && !done; ++it) {
          long long k0 = hk[h];
          int won = 0;
          if (k0 == LLONG_MIN) {
            k0 = (long long)atomicCAS(
                (unsigned long long *)&hk[h], (unsigned long long)LLONG_MIN,
                (unsigned long long)key);
            won = k0 == LLONG_MIN;              /* we inserted */
          }
          /* the inserter publishes here, on a path every lane has left
           * before any lane waits below: the lanes of a wave run in
           * lockstep, so a duplicate in the inserter's own wave that began
           * to spin first would wait for a store that cannot happen, time
           * out and report a conflict that is none */
          if (won) (void)atomicExch((int *)&hp[h], pay);
          if (won) {
            done = 1;
          } else if (k0 == key) {
            int pv;
            int spins = 0;
            do {
              pv = atomicOr((int *)&hp[h], 0);  /* atomic read */
            } while (pv == INT_MIN && ++spins < (1 << 20));
            if (pv != pay) atomicOr((int *)&flags[0], 1);
            done = 1;
          } else {
            h = (h + 1) & mask;
          }
        }
        if (!done) atomicOr((int *)&flags[1], 1);
      }
  });
}

/* densify the open-address table into a payload LUT over [lmin, lmax]; the
 * bounds come from stats rows, so a key outside them is left out and
 * reported in oob[0] rather than written */
__global__ void k_hash_to_lut(const long long *__restrict__ hk_,
                              const int32_t *__restrict__ hp_,
                              long long cap, int32_t *__restrict__ lut_,
                              long long lmin, long long lmax,
                              int32_t *__restrict__ oob_) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const long long key = ((const GAS long long *)(uintptr_t)hk_)[i];
  if (key == LLONG_MIN) return;
  if (key < lmin || key > lmax) {
    GAS int32_t *oob = (GAS int32_t *)(uintptr_t)oob_;
    atomicOr((int *)&oob[0], 1);
    return;
  }
  ((GAS int32_t *)(uintptr_t)lut_)[key - lmin] =
      ((const GAS int32_t *)(uintptr_t)hp_)[i];
}

extern "C" int sn_launch_join_build(const sn_dev_plan *plan,
                                    const sn_dev_plan *dev_plan,
                                    const sn_dev_batch *dev_batches,
                                    const sn_dev_tile *dev_tiles,
                                    int32_t ntiles, long long *hk,
                                    int32_t *hp, int cap_log2, int has_attr,
                                    int32_t *flags, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  {
    long long cap = 1ll << cap_log2;
    hipLaunchKernelGGL(k_fill_i64, dim3((unsigned)((cap + 255) / 256)),
                       dim3(256), 0, s, hk, cap, LLONG_MIN);
    /* payloads init to the INT32_MIN publication sentinel (two per i64) */
    hipLaunchKernelGGL(k_fill_i64, dim3((unsigned)((cap / 2 + 255) / 256)),
                       dim3(256), 0, s, (long long *)hp, cap / 2,
                       (long long)0x8000000080000000ull);
  }
  if (ntiles <= 0) return (int)hipGetLastError();
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  const size_t lds = sn_lds_join_build(plan->nused).total;
  if (lds > SN_LDS_LIMIT) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_join_build, dim3(grid), dim3(WG), lds, s,
                     *plan, dev_batches, dev_tiles, ntiles,
                     hk, hp, cap_log2, has_attr, flags);
  return (int)hipGetLastError();
}

extern "C" int sn_launch_hash_to_lut(const long long *hk, const int32_t *hp,
                                     long long cap, int32_t *lut,
                                     long long lmin, long long lmax,
                                     int32_t *oob, void *stream) {
  hipLaunchKernelGGL(k_hash_to_lut, dim3((unsigned)((cap + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, hk, hp, cap, lut, lmin,
                     lmax, oob);
  return (int)hipGetLastError();
}

/* compact the used hash-table rows into dense (key, accumulator-row) pairs
 * so the host reads back only the live groups, not the whole table */
__global__ void k_hash_compact(const long long *__restrict__ hk_,
                               const double *__restrict__ hacc_,
                               int cap, int naggs1,
                               long long *__restrict__ okeys,
                               double *__restrict__ orows,
                               int *__restrict__ counter) {
  const GAS long long *hk = (const GAS long long *)(uintptr_t)hk_;
  const GAS double *hacc = (const GAS double *)(uintptr_t)hacc_;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > cap) return;
  long long key;
  int used;
  if (i == cap) {                                   /* reserved sentinel-key row */
    key = SN_HASH_EMPTY;
    used = hacc[(size_t)cap * naggs1 + (naggs1 - 1)] != 0.0;
  } else {
    key = hk[i];
    used = key != SN_HASH_EMPTY;
  }
  if (!used) return;
  const int o = atomicAdd((int *)(uintptr_t)counter, 1);
  ((GAS long long *)(uintptr_t)okeys)[o] = key;
  GAS double *dst = (GAS double *)(uintptr_t)orows + (size_t)o * naggs1;
  for (int a = 0; a < naggs1; a++) dst[a] = hacc[(size_t)i * naggs1 + a];
}

extern "C" int sn_launch_hash_scan(const sn_dev_plan *plan,
                                   const sn_dev_plan *dev_plan,
                                   const sn_dev_batch *dev_batches,
                                   const sn_dev_tile *dev_tiles, int32_t ntiles,
                                   void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ntiles <= 0) return 0;
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  const size_t lds = sn_lds_hash(plan->nused).total;
  if (lds > SN_LDS_LIMIT) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grouped_hash, dim3(grid), dim3(WG), lds, s,
                     *plan, dev_plan, dev_batches, dev_tiles, ntiles);
  return (int)hipGetLastError();
}

extern "C" int sn_launch_hash_compact(const long long *hk, const double *hacc,
                                      int cap, int naggs1, long long *okeys,
                                      double *orows, int *counter,
                                      void *stream) {
  hipLaunchKernelGGL(k_hash_compact, dim3((cap + 1 + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, hk, hacc, cap, naggs1, okeys, orows,
                     counter);
  return (int)hipGetLastError();
}

/* ---- radix pass 2: per-partition aggregation in LDS ----
 * Pass 1 (the query-compiled scatter) partitioned the passing rows by
 * mix64(key) high bits into plan->precs.  Here one workgroup owns one
 * partition and aggregates its records into an LDS-RESIDENT open-address
 * table (the measured fix: a first version kept per-partition segments of
 * the global table — "L2-resident" probes still cost 6.9 ms on 60M rows
 * at 1 workgroup/partition, nearly the whole single-pass time, because
 * the streaming record reads evict the segments and the dependent L2
 * atomic chains sit at 8 waves/CU; LDS f64 atomics are the same pipe the
 * 5 TB/s dense grouped kernels run on).  The filled slots then compact
 * DIRECTLY from LDS into the (okeys, orows) result arrays — the global
 * hkeys table is never touched and k_hash_compact is skipped; only the
 * reserved sentinel-key row still lives in hacc[cap].  Fill counting and
 * the overflow flag keep the single-pass contract, so grow-and-retry is
 * unchanged. */
__global__ __launch_bounds__(WG, 1)
void k_radix_agg_lds(const sn_dev_plan *__restrict__ plan_g,
                     long long *__restrict__ okeys_,
                     double *__restrict__ orows_,
                     int *__restrict__ counter_) {
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  const GAS sn_dev_plan *P = (const GAS sn_dev_plan *)(uintptr_t)plan_g;
  const int naggs = P->naggs;
  const int na1 = naggs + 1;              /* radix requires pac == 0 */
  const int sub = P->radix;               /* partition shift (slots log2) */
  const int subcap = 1 << sub;
  const unsigned smask = (unsigned)subcap - 1;
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  long long *skeys = (long long *)lsm;
  double *sacc = (double *)(lsm + (size_t)subcap * 8);
  int *scnt = (int *)(lsm + (size_t)subcap * 8 + (size_t)subcap * na1 * 8);
  __shared__ int basew;

  int ops[12];                            /* SN_MAX_AGGS */
  double idents[12];
  for (int a = 0; a < naggs; a++) {
    ops[a] = P->aggs[a].op;
    idents[a] = acc_ident(ops[a]);
  }
  for (int i = tid; i < subcap; i += WG) {
    skeys[i] = SN_HASH_EMPTY;
    double *row = sacc + (size_t)i * na1;
    for (int a = 0; a < naggs; a++) row[a] = idents[a];
    row[na1 - 1] = 0.0;
  }
  __syncthreads();

  const int percap = P->percap;
  const int n = min(((const GAS int *)(uintptr_t)P->pcount)[p], percap);
  const GAS double *recs = (const GAS double *)(uintptr_t)P->precs +
                           (size_t)p * percap * (1 + naggs);
  GAS double *acc = (GAS double *)(uintptr_t)P->hacc;
  GAS int32_t *flags = (GAS int32_t *)(uintptr_t)P->hflags;
  const int cap = 1 << P->hcap_log2;

  for (int i = tid; i < n; i += WG) {
    const GAS double *rec = recs + (size_t)i * (1 + naggs);
    const long long key = __double_as_longlong(rec[0]);
    if (key == SN_HASH_EMPTY) {
      /* a REAL key of -1: reserved global row at cap (rare) */
      GAS double *row = acc + (size_t)cap * na1;
      for (int a = 0; a < naggs; a++) acc_cell(&row[a], ops[a], rec[1 + a]);
      (void)atomicAdd((double *)&row[na1 - 1], 1.0);
      continue;
    }
    /* (the compaction below counts the fill) */
    const int slot = hash_find_or_insert(skeys, smask, key, nullptr);
    if (slot < 0) { atomicOr((int *)flags, 1); continue; }   /* table full */
    double *row = sacc + (size_t)slot * na1;
    for (int a = 0; a < naggs; a++) acc_cell(&row[a], ops[a], rec[1 + a]);
    (void)atomicAdd(&row[na1 - 1], 1.0);
  }
  __syncthreads();

  /* compact straight from LDS: thread t owns slots [t*spt, (t+1)*spt);
   * block prefix-sum places each filled slot at one reserved output
   * range (ONE global counter add per block, and the filled-slot total
   * IS the insert count, so the fill counter costs one more add). */
  const int spt = subcap / WG;
  int mine = 0;
  for (int j = 0; j < spt; j++)
    mine += skeys[tid * spt + j] != SN_HASH_EMPTY;
  scnt[tid] = mine;
  __syncthreads();
  for (int off = 1; off < WG; off <<= 1) {        /* inclusive scan */
    const int u = tid >= off ? scnt[tid - off] : 0;
    __syncthreads();
    scnt[tid] += u;
    __syncthreads();
  }
  if (tid == WG - 1) {
    const int total = scnt[WG - 1];
    basew = total ? atomicAdd((int *)(uintptr_t)counter_, total) : 0;
    if (total) (void)atomicAdd((int *)(flags + 2), total);
  }
  __syncthreads();
  int o = basew + scnt[tid] - mine;
  GAS long long *okeys = (GAS long long *)(uintptr_t)okeys_;
  GAS double *orows = (GAS double *)(uintptr_t)orows_;
  for (int j = 0; j < spt; j++) {
    const int s = tid * spt + j;
    if (skeys[s] == SN_HASH_EMPTY) continue;
    okeys[o] = skeys[s];
    GAS double *dst = orows + (size_t)o * na1;
    const double *src = sacc + (size_t)s * na1;
    for (int a = 0; a < na1; a++) dst[a] = src[a];
    o++;
  }
}

/* fallback for accumulator rows too wide for the LDS table: per-partition
 * SEGMENTS of the global hkeys/hacc (compact + readback then run as in the
 * single-pass path) */
__global__ __launch_bounds__(WG, 2)
void k_radix_agg_glob(const sn_dev_plan *__restrict__ plan_g) {
  const GAS sn_dev_plan *P = (const GAS sn_dev_plan *)(uintptr_t)plan_g;
  const int naggs = P->naggs;
  const int na1 = naggs + 1;
  const int sub = P->radix;
  const int p = blockIdx.x;
  const int percap = P->percap;
  const GAS int *pcount = (const GAS int *)(uintptr_t)P->pcount;
  const int n = min(pcount[p], percap);
  const GAS double *recs = (const GAS double *)(uintptr_t)P->precs +
                           (size_t)p * percap * (1 + naggs);
  GAS long long *hk = (GAS long long *)(uintptr_t)P->hkeys;
  GAS double *acc = (GAS double *)(uintptr_t)P->hacc;
  GAS int32_t *flags = (GAS int32_t *)(uintptr_t)P->hflags;
  const int cap = 1 << P->hcap_log2;
  const int segbase = p << sub;
  const unsigned smask = (1u << sub) - 1;
  int ops[12];
  for (int a = 0; a < naggs; a++) ops[a] = P->aggs[a].op;

  for (int i = threadIdx.x; i < n; i += WG) {
    const GAS double *rec = recs + (size_t)i * (1 + naggs);
    const long long key = __double_as_longlong(rec[0]);
    int slot;
    if (key == SN_HASH_EMPTY) {
      slot = cap;                                   /* reserved row */
    } else {
      slot = hash_find_or_insert(hk + segbase, smask, key, flags + 2);
      if (slot < 0) { atomicOr((int *)flags, 1); continue; }  /* segment full */
      slot += segbase;
    }
    GAS double *row = acc + (size_t)slot * na1;
    for (int a = 0; a < naggs; a++) acc_cell(&row[a], ops[a], rec[1 + a]);
    (void)atomicAdd((double *)&row[na1 - 1], 1.0);
  }
}

extern "C" int sn_launch_radix_agg(const sn_dev_plan *plan,
                                   const sn_dev_plan *dev_plan,
                                   long long *okeys, double *orows,
                                   int *counter, void *stream) {
  const int npart = 1 << (plan->hcap_log2 - plan->radix);
  const int na1 = plan->naggs + 1;
  if (sn_radix_direct(plan->radix, na1)) {
    const size_t lds = sn_radix_lds_bytes(plan->radix, na1);
    hipLaunchKernelGGL(k_radix_agg_lds, dim3(npart), dim3(WG), lds,
                       (hipStream_t)stream, dev_plan, okeys, orows, counter);
  } else {
    hipLaunchKernelGGL(k_radix_agg_glob, dim3(npart), dim3(WG), 0,
                       (hipStream_t)stream, dev_plan);
  }
  return (int)hipGetLastError();
}

/* ---- device-side batch stats (f2: GPU batch building) ----
 * min/max over one raw fixed-width column (the ColumnStatsSchema bounds
 * ColumnEncoder tracks during encode, ColumnEncoding.scala:188-251),
 * accumulated into out[0]=min, out[1]=max with ord-encoded u64 atomics
 * (doubles) or native i64 atomics — async on the put stream, so ingest
 * never syncs per batch. */
__device__ __forceinline__ unsigned long long wave_umin(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y =
        (unsigned long long)__shfl_down((long long)x, off, 64);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ unsigned long long wave_umax(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y =
        (unsigned long long)__shfl_down((long long)x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}

/* omin slots memset to 0xFF (>= every encoding), omax to 0x00: f64 values
 * use the ord encoding, integers the sign-bias (v ^ 1<<63) — both
 * order-preserving into unsigned, so the memset identities work for all */
__global__ __launch_bounds__(256, 4)
void k_col_minmax(const void *__restrict__ body_, long long n, int kind,
                  unsigned long long *__restrict__ omin_,
                  unsigned long long *__restrict__ omax_) {
  GAS unsigned long long *omin = (GAS unsigned long long *)(uintptr_t)omin_;
  GAS unsigned long long *omax = (GAS unsigned long long *)(uintptr_t)omax_;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long emn = ~0ull, emx = 0ull;
  if (kind == SN_K_F64 || kind == SN_K_F32) {
    double mn = __longlong_as_double(0x7FF0000000000000ll);   /* +inf */
    double mx = -mn;
    bool any = false;
    if (kind == SN_K_F64) {
      const GAS double *b = (const GAS double *)(uintptr_t)body_;
      for (long long i = i0; i < n; i += stride) {
        const double v = b[i];
        mn = fmin(mn, v); mx = fmax(mx, v); any = true;
      }
    } else {
      const GAS float *b = (const GAS float *)(uintptr_t)body_;
      for (long long i = i0; i < n; i += stride) {
        const double v = (double)b[i];
        mn = fmin(mn, v); mx = fmax(mx, v); any = true;
      }
    }
    if (any) { emn = f64_ord(mn); emx = f64_ord(mx); }
  } else {
    long long mn = 0x7FFFFFFFFFFFFFFFll, mx = (long long)0x8000000000000000ll;
    bool any = false;
    if (kind == SN_K_I64) {
      const GAS long long *b = (const GAS long long *)(uintptr_t)body_;
      for (long long i = i0; i < n; i += stride) {
        const long long v = b[i];
        mn = v < mn ? v : mn; mx = v > mx ? v : mx; any = true;
      }
    } else if (kind == SN_K_I32) {
      const GAS int *b = (const GAS int *)(uintptr_t)body_;
      for (long long i = i0; i < n; i += stride) {
        const long long v = b[i];
        mn = v < mn ? v : mn; mx = v > mx ? v : mx; any = true;
      }
    } else {  /* I16 */
      const GAS short *b = (const GAS short *)(uintptr_t)body_;
      for (long long i = i0; i < n; i += stride) {
        const long long v = b[i];
        mn = v < mn ? v : mn; mx = v > mx ? v : mx; any = true;
      }
    }
    if (any) {
      emn = (unsigned long long)mn ^ 0x8000000000000000ull;
      emx = (unsigned long long)mx ^ 0x8000000000000000ull;
    }
  }
  emn = wave_umin(emn);
  emx = wave_umax(emx);
  if ((threadIdx.x & 63) == 0) {
    (void)atomicMin((unsigned long long *)omin, emn);
    (void)atomicMax((unsigned long long *)omax, emx);
  }
}

extern "C" int sn_launch_col_minmax(const void *body, long long n, int kind,
                                    unsigned long long *omin,
                                    unsigned long long *omax, void *stream) {
  long long blocks = (n + 256 * 16 - 1) / (256 * 16);
  if (blocks < 1) blocks = 1;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_col_minmax, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, body, n, kind, omin, omax);
  return (int)hipGetLastError();
}

/* ---- put-time f64 narrowing: 1-byte codes + a value dictionary ----
 * A low-cardinality double column (TPC-H l_quantity: 50 values, l_discount:
 * 11) scans from a num_rows-byte code array and a <= 256-entry dictionary
 * instead of its 8 B/row body.  Values are told apart by
 * their 64-bit PATTERN, so -0.0 / +0.0 and every NaN payload are entries of
 * their own and dict[code] gives back the exact input bits.
 *
 * Three launches, async on the ingest stream, no host sync:
 *   k_f64_distinct  every workgroup inserts its grid-stride slice into an
 *                   LDS open-address set, gives up once that holds more than
 *                   256 patterns, else merges it into the global set;
 *   k_f64_dict      one workgroup compacts and rank-sorts the global set
 *                   (ascending as unsigned integers) into dict[0..ndict) and
 *                   zeroes the rest, or writes ndict = -1 and zeroes it all;
 *   k_f64_encode    reads ndict on device, returns when it is negative, else
 *                   binary-searches an LDS copy of the dictionary per row.
 * The global set IS dict[0..256) (u64 view) and the flags live in *ndict, so
 * the launcher needs no workspace and nothing outside [codes, codes+n),
 * dict[0..256) and *ndict is ever written.  All 2^64 patterns are values, so
 * the empty-slot sentinel (all ones, itself a NaN payload) is tracked by a
 * flag instead of being stored. */
#define NARROW_MAX 256            /* dictionary entries == global set slots */
#define NARROW_LSLOTS 2048        /* LDS set: <= 256 + one 1024-row step */
#define NARROW_STEP 4             /* rows per lane per step */
#define NARROW_EMPTY (~0ull)
#define NARROW_F_OVERFLOW (1 << 30)
#define NARROW_F_HAS_EMPTY (1 << 29)

__global__ __launch_bounds__(WG, 4)
void k_f64_distinct(const double *__restrict__ body_, long long n,
                    double *__restrict__ dict_, int *__restrict__ ndict_) {
  __shared__ unsigned long long lset[NARROW_LSLOTS];
  __shared__ int lcount, lflags;
  const GAS unsigned long long *body =
      (const GAS unsigned long long *)(uintptr_t)body_;
  unsigned long long *gset = (unsigned long long *)dict_;
  const int tid = threadIdx.x;
  for (int i = tid; i < NARROW_LSLOTS; i += WG) lset[i] = NARROW_EMPTY;
  if (tid == 0) { lcount = 0; lflags = 0; }
  __syncthreads();
  const long long span = (long long)WG * NARROW_STEP;
  for (long long base = (long long)blockIdx.x * span; base < n;
       base += (long long)gridDim.x * span) {
    unsigned long long v[NARROW_STEP];
#pragma unroll
    for (int j = 0; j < NARROW_STEP; j++) {
      const long long i = base + tid + (long long)j * WG;
      v[j] = i < n ? body[i] : body[base];   /* base < n: a value of the slice */
    }
#pragma unroll
    for (int j = 0; j < NARROW_STEP; j++) {
      const unsigned long long key = v[j];
      if (key == NARROW_EMPTY) { atomicOr(&lflags, NARROW_F_HAS_EMPTY); continue; }
      /* the set holds at most 256 + 1024 of its 2048 slots, so a probe
       * always meets the key or an empty slot */
      unsigned h = (unsigned)mix64(key) & (NARROW_LSLOTS - 1);
      while (true) {
        unsigned long long k0 = lset[h];
        if (k0 == key) break;
        if (k0 == NARROW_EMPTY) {
          k0 = atomicCAS(&lset[h], NARROW_EMPTY, key);
          if (k0 == NARROW_EMPTY) { atomicAdd(&lcount, 1); break; }
          if (k0 == key) break;
        }
        h = (h + 1) & (NARROW_LSLOTS - 1);
      }
    }
    __syncthreads();
    if (lcount > NARROW_MAX) break;          /* uniform: lcount is settled */
    __syncthreads();                         /* before the next step's adds */
  }
  if (lcount > NARROW_MAX) {
    if (tid == 0) atomicOr(ndict_, NARROW_F_OVERFLOW);
    return;
  }
  if (tid == 0 && lflags) atomicOr(ndict_, lflags);
  for (int i = tid; i < NARROW_LSLOTS; i += WG) {
    const unsigned long long key = lset[i];
    if (key == NARROW_EMPTY) continue;
    unsigned h = (unsigned)mix64(key) & (NARROW_MAX - 1);
    int it = 0;
    for (; it < NARROW_MAX; it++) {
      /* a slot only ever goes from empty to its key, so a plain look first
       * is safe however stale, and spares the hot lines all but the first
       * workgroups' atomics (every workgroup brings the same few keys) */
      unsigned long long k0 = __hip_atomic_load(
          &gset[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k0 == NARROW_EMPTY) k0 = atomicCAS(&gset[h], NARROW_EMPTY, key);
      if (k0 == NARROW_EMPTY || k0 == key) break;
      h = (h + 1) & (NARROW_MAX - 1);
    }
    if (it == NARROW_MAX) atomicOr(ndict_, NARROW_F_OVERFLOW);   /* set full */
  }
}

__global__ __launch_bounds__(NARROW_MAX, 1)
void k_f64_dict(double *__restrict__ dict_, int *__restrict__ ndict_) {
  __shared__ unsigned long long keys[NARROW_MAX], sorted[NARROW_MAX];
  __shared__ int nvalid;
  unsigned long long *gset = (unsigned long long *)dict_;
  const int tid = threadIdx.x;
  const int flags = *ndict_;
  const unsigned long long key = gset[tid];
  keys[tid] = key;
  sorted[tid] = 0;
  if (tid == 0) nvalid = 0;
  __syncthreads();
  const int valid = key != NARROW_EMPTY;
  if (valid) atomicAdd(&nvalid, 1);
  /* distinct keys: the count of smaller ones is the sorted position */
  int rank = 0;
  for (int j = 0; j < NARROW_MAX; j++)
    rank += (keys[j] != NARROW_EMPTY) & (keys[j] < key);
  __syncthreads();
  const int has_empty = (flags & NARROW_F_HAS_EMPTY) != 0;
  const int total = nvalid + has_empty;
  const int fits = !(flags & NARROW_F_OVERFLOW) && total <= NARROW_MAX;
  if (fits) {
    if (valid) sorted[rank] = key;
    /* all ones is the largest pattern: it sorts last */
    if (has_empty && tid == 0) sorted[total - 1] = NARROW_EMPTY;
  }
  __syncthreads();
  gset[tid] = sorted[tid];
  if (tid == 0) *ndict_ = fits ? total : -1;
}

__global__ __launch_bounds__(WG, 4)
void k_f64_encode(const double *__restrict__ body_, long long n,
                  unsigned char *__restrict__ codes_,
                  const double *__restrict__ dict_,
                  const int *__restrict__ ndict_) {
  __shared__ unsigned long long sd[NARROW_MAX];
  const int nd = *ndict_;
  if (nd < 0) return;                        /* overflow: codes stay untouched */
  const GAS unsigned long long *body =
      (const GAS unsigned long long *)(uintptr_t)body_;
  GAS unsigned char *codes = (GAS unsigned char *)(uintptr_t)codes_;
  const int tid = threadIdx.x;
  sd[tid] = ((const unsigned long long *)dict_)[tid];
  __syncthreads();
  auto code_of = [&](unsigned long long key) {
    int pos = 0;                             /* entries [0, pos) are < key */
#pragma unroll
    for (int s = NARROW_MAX / 2; s > 0; s >>= 1) {
      const int p = pos + s;
      if (p <= nd && sd[p - 1] < key) pos = p;
    }
    return (unsigned)pos;
  };
  /* aligned code arrays (every arena block) store four codes per lane */
  const int packed = ((uintptr_t)codes_ & 3) == 0;
  const long long n4 = packed ? n / 4 : 0;
  const long long stride = (long long)gridDim.x * WG;
  for (long long g = (long long)blockIdx.x * WG + tid; g < n4; g += stride) {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) w |= code_of(body[g * 4 + j]) << (8 * j);
    ((GAS unsigned *)codes)[g] = w;
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * WG + tid; i < n;
       i += stride)
    codes[i] = (unsigned char)code_of(body[i]);
}

extern "C" int sn_launch_f64_narrow(const double *body, long long n,
                                    unsigned char *codes, double *dict,
                                    int *ndict, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipError_t rc = hipMemsetAsync(dict, 0xff, NARROW_MAX * 8, s);
  if (rc == hipSuccess) rc = hipMemsetAsync(ndict, 0, 4, s);
  if (rc != hipSuccess) return (int)rc;
  const long long span = (long long)WG * NARROW_STEP;
  long long blocks = (n + span - 1) / span;
  if (blocks > 1024) blocks = 1024;
  if (blocks > 0)
    hipLaunchKernelGGL(k_f64_distinct, dim3((unsigned)blocks), dim3(WG), 0, s,
                       body, n, dict, ndict);
  hipLaunchKernelGGL(k_f64_dict, dim3(1), dim3(NARROW_MAX), 0, s, dict, ndict);
  if (blocks > 0)
    hipLaunchKernelGGL(k_f64_encode, dim3((unsigned)blocks), dim3(WG), 0, s,
                       body, n, codes, dict, ndict);
  return (int)hipGetLastError();
}

/* ---- wave-cooperative LZ4 block decode (f1: compressed-upload ingest) ----
 * The reference wraps each column blob as ONE raw LZ4 block
 * (CompressionUtils.scala:132-160): the token chain is strictly
 * sequential, so lane 0 parses while all 64 lanes of the wave copy the
 * literal/match runs — wave lockstep makes the copy loop barrier-free.
 * Overlapping matches (offset < length) replicate periodically:
 * dst[i] = dst[start - off + i % off], every read landing before the
 * segment start.  One wave per blob; concurrency comes from decoding
 * many blobs in flight (one launch per put on the engine stream). */
__global__ __launch_bounds__(64, 8)
void k_lz4_decompress(const uint8_t *__restrict__ src_, long long slen,
                      uint8_t *__restrict__ dst_, long long dlen,
                      int32_t *__restrict__ err_) {
  const GAS uint8_t *src = (const GAS uint8_t *)(uintptr_t)src_;
  GAS uint8_t *dst = (GAS uint8_t *)(uintptr_t)dst_;
  GAS int32_t *err = (GAS int32_t *)(uintptr_t)err_;
  const int lane = threadIdx.x;
  long long ip = 0, op = 0;
  while (true) {
    /* lane 0 parses one sequence; broadcast (lit_src, lit_len, m_off,
     * m_len, next_ip); next_ip -2 = clean end, -3 = malformed */
    long long v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = -3;
    if (lane == 0) {
      if (ip >= slen) {
        v4 = -2;
      } else {
        const unsigned tok = src[ip++];
        long long ll = tok >> 4;
        if (ll == 15) {
          unsigned b;
          do { b = (ip < slen) ? src[ip++] : 0; ll += b; }
          while (b == 255 && ip < slen);
        }
        v0 = ip;                                /* literal source */
        v1 = ll;
        ip += ll;
        if (ip > slen || op + ll > dlen) {
          v4 = -3;
        } else if (ip == slen) {
          v4 = ip;                              /* final literals-only seq */
        } else if (ip + 2 > slen) {
          v4 = -3;
        } else {
          long long off = (long long)src[ip] | ((long long)src[ip + 1] << 8);
          ip += 2;
          long long ml = tok & 15;
          if (ml == 15) {
            unsigned b;
            do { b = (ip < slen) ? src[ip++] : 0; ml += b; }
            while (b == 255 && ip < slen);
          }
          ml += 4;
          if (off == 0 || off > op + ll || op + ll + ml > dlen) v4 = -3;
          else { v2 = off; v3 = ml; v4 = ip; }
        }
      }
    }
    v0 = __shfl(v0, 0, 64);
    v1 = __shfl(v1, 0, 64);
    v2 = __shfl(v2, 0, 64);
    v3 = __shfl(v3, 0, 64);
    v4 = __shfl(v4, 0, 64);
    if (v4 == -2) break;                        /* end of input */
    if (v4 == -3) { if (lane == 0 && err) err[0] = 1; return; }
    for (long long i = lane; i < v1; i += 64) dst[op + i] = src[v0 + i];
    op += v1;
    if (v3 > 0) {
      /* match copy: direct when the source window clears the segment,
       * periodic replication when it overlaps (off < len) — every read
       * lands strictly before the segment start either way */
      const long long mo = v2;
      for (long long i = lane; i < v3; i += 64)
        dst[op + i] = dst[op - mo + (mo >= v3 ? i : i % mo)];
      op += v3;
    }
    ip = v4;
  }
  if (lane == 0 && err) err[0] = (op == dlen) ? 0 : 2;
}

extern "C" int sn_launch_lz4_decompress(const void *src, long long slen,
                                        void *dst, long long dlen,
                                        int32_t *err, void *stream) {
  hipLaunchKernelGGL(k_lz4_decompress, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (const uint8_t *)src, slen,
                     (uint8_t *)dst, dlen, err);
  return (int)hipGetLastError();
}

/* fold per-block partial rows into the final output.
 * keyless: final[i] = sum_b scratch[b][i]  (NV = 2*NA_t+1, identical layout)
 * grouped: scratch rows are [slot][na1]; final is [slot][out_stride]
 * with rowcount at out_stride-1.  MIN/MAX cells (op from plan_g, NULL =
 * all-sum) hold the ord-u64 encoding in the scratch rows; they fold with
 * integer min/max and DECODE to plain doubles here. */
__device__ __forceinline__ double ord_f64(unsigned long long o) {
  unsigned long long b = (o & 0x8000000000000000ull)
      ? (o ^ 0x8000000000000000ull) : ~o;
  return __longlong_as_double((long long)b);
}

__global__ void k_reduce(const double *__restrict__ scratch, int nblocks,
                         int nv, double *__restrict__ out, int naggs1,
                         int out_stride,
                         const sn_dev_plan *__restrict__ plan_g) {
  /* one block per output value; 256 threads stride the partial rows */
  __shared__ double red[4];
  __shared__ unsigned long long redu[4];
  const GAS double *src = (const GAS double *)(uintptr_t)scratch;
  const int i = blockIdx.x;
  if (i >= nv) return;
  int op = 0;
  if (plan_g && naggs1 > 0) {
    const GAS sn_dev_plan *P = (const GAS sn_dev_plan *)(uintptr_t)plan_g;
    const int naggs = P->naggs;
    const int a = i % naggs1;
    if (a < naggs) op = P->aggs[a].op;
  }
  if (op != 0) {
    unsigned long long m = op == 1 ? ORD_MIN_IDENT : ORD_MAX_IDENT;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
      const unsigned long long v =
          (unsigned long long)__double_as_longlong(src[(size_t)b * nv + i]);
      m = op == 1 ? (v < m ? v : m) : (v > m ? v : m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o2 =
          (unsigned long long)__shfl_down((long long)m, off, 64);
      m = op == 1 ? (o2 < m ? o2 : m) : (o2 > m ? o2 : m);
    }
    if ((threadIdx.x & 63) == 0) redu[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; w++)
        m = op == 1 ? (redu[w] < redu[0] ? redu[w] : redu[0])
                    : (redu[w] > redu[0] ? redu[w] : redu[0]),
        redu[0] = m;
      const int slot = i / naggs1, a = i % naggs1;
      out[(size_t)slot * out_stride + (a < naggs1 - 1 ? a : out_stride - 1)] =
          ord_f64(redu[0]);
    }
    return;
  }
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
    s += src[(size_t)b * nv + i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0] + red[1] + red[2] + red[3];
    if (naggs1 == 0) {
      out[i] = t;
    } else {
      int slot = i / naggs1, a = i % naggs1;
      out[(size_t)slot * out_stride + (a < naggs1 - 1 ? a : out_stride - 1)] = t;
    }
  }
}

/* initialize a global accumulator's MIN/MAX cells to their identities
 * (host memset covers only the sum/count cells' zero) */
__global__ void k_acc_init(double *__restrict__ acc, long long rows,
                           int naggs, int na1,
                           const sn_dev_plan *__restrict__ plan_g) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * na1) return;
  const int a = (int)(i % na1);
  if (a >= naggs) return;
  const GAS sn_dev_plan *P = (const GAS sn_dev_plan *)(uintptr_t)plan_g;
  const int op = P->aggs[a].op;
  if (op == 0) return;
  ((GAS double *)(uintptr_t)acc)[i] = acc_ident(op);
}

extern "C" int sn_launch_acc_init(double *acc, long long rows, int naggs,
                                  int na1, const void *plan_dev,
                                  void *stream) {
  long long n = rows * na1;
  hipLaunchKernelGGL(k_acc_init, dim3((unsigned)((n + 255) / 256)), dim3(256),
                     0, (hipStream_t)stream, acc, rows, naggs, na1,
                     (const sn_dev_plan *)plan_dev);
  return (int)hipGetLastError();
}

/* put-time patch materialization: write value-only update patches straight
 * into the (null-free, fixed-width) device body so the batch scans clean.
 * Values are plain doubles (decode_delta widening) except INT64, whose
 * patch values travel as raw bits (exact beyond 2^53); the narrower integer
 * bodies take round-nearest, matching read_general's __double2ll_rn. */
__global__ void k_patch_apply(void *__restrict__ body,
                              const int32_t *__restrict__ pos,
                              const double *__restrict__ val, int n,
                              int kind) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = as_global(pos)[i];
  const double v = as_global(val)[i];
  switch (kind) {
    case SN_K_F64: ((GAS double *)(uintptr_t)body)[p] = v; break;
    case SN_K_F32: ((GAS float *)(uintptr_t)body)[p] = (float)v; break;
    case SN_K_I32: ((GAS int32_t *)(uintptr_t)body)[p] = (int32_t)__double2ll_rn(v); break;
    /* INT64 patch values are raw bits (exact beyond 2^53) */
    case SN_K_I64: ((GAS long long *)(uintptr_t)body)[p] = __double_as_longlong(v); break;
    case SN_K_I16: ((GAS int16_t *)(uintptr_t)body)[p] = (int16_t)__double2ll_rn(v); break;
  }
}

extern "C" int sn_launch_patch_apply(void *body, const int32_t *pos,
                                     const double *val, int n, int kind,
                                     void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_patch_apply, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, body, pos, val, n, kind);
  return (int)hipGetLastError();
}

extern "C" int sn_launch_reduce(const double *dev_scratch, int nblocks,
                                int nv, double *dev_out, int naggs1,
                                int out_stride, const void *plan_dev,
                                void *stream) {
  hipLaunchKernelGGL(k_reduce, dim3(nv), dim3(WG), 0, (hipStream_t)stream,
                     dev_scratch, nblocks, nv, dev_out, naggs1, out_stride,
                     (const sn_dev_plan *)plan_dev);
  return (int)hipGetLastError();
}

extern "C" int sn_launch_scan_agg(const sn_dev_plan *plan,
                                  const sn_dev_plan *dev_plan,
                                  const sn_dev_batch *dev_batches,
                                  const sn_dev_tile *dev_tiles, int32_t ntiles,
                                  double *dev_out, double *dev_scratch,
                                  void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const sn_dense_launch d = sn_dense_launch_of(plan, ntiles);
  if (d.lds > SN_LDS_LIMIT) return (int)hipErrorInvalidValue;
  const int grid = d.grid, ns = plan->nslots, na = plan->naggs;
  const size_t lds = (size_t)d.lds;
  const bool nc4 = plan->nused <= 4;
#define SCAN(K) hipLaunchKernelGGL((K), dim3(grid), dim3(WG), lds, s, *plan, \
        dev_plan, dev_batches, dev_tiles, ntiles, dev_scratch)
#define KL(A, NCv) SCAN((k_keyless<A, NCv>))
#define KG(S, NCv) SCAN((k_grouped<S, NCv>))
  switch (d.route) {
    case SN_ROUTE_KEYLESS:
      if (na <= 2) { if (nc4) KL(2, 4); else KL(2, 8); }
      else if (na <= 4) { if (nc4) KL(4, 4); else KL(4, 8); }
      else { if (nc4) KL(12, 4); else KL(12, 8); }
      break;
    case SN_ROUTE_GLOBAL:
      /* global f64 atomics into the (host-zeroed) scratch accumulator */
      SCAN(k_grouped_global);
      break;
    case SN_ROUTE_LDS:
      SCAN(k_grouped_lds);
      break;
    case SN_ROUTE_REG:
      /* (measured: an unstaged 3-waves/SIMD variant loses 20% — staging
       * beats occupancy for the grouped shape as well) */
      if (nc4) SCAN((k_grouped_reg<SN_REG_SLOTS, 6, 4>));
      else SCAN((k_grouped_reg<SN_REG_SLOTS, 6, 8>));
      break;
    default:
      if (ns <= 4) { if (nc4) KG(4, 4); else KG(4, 8); }
      else if (ns <= 8) { if (nc4) KG(8, 4); else KG(8, 8); }
      else { if (nc4) KG(16, 4); else KG(16, 8); }
      break;
  }
#undef KL
#undef KG
#undef SCAN
  hipLaunchKernelGGL(k_reduce, dim3(d.nv), dim3(WG), 0, s,
                     dev_scratch, sn_dense_rows(&d, 0), d.nv, dev_out,
                     d.naggs1, d.out_stride, dev_plan);
  return (int)hipGetLastError();
}

/* ================= exact DECIMAL aggregation =================
 * Fixed-point twin of the double aggregate path: a decimal column is an
 * INT64 column of unscaled values (the reference's 8-byte long decimals of
 * precision <= 18), so the decode front end above — convert_chunk,
 * alive_init, pred_sweeps and the raw-bit i64 LDS image — is reused as is
 * and deletes, deltas, nulls, RLE and stats skipping behave identically.
 * Clean full chunks take the same staged (software-pipelined) conversion.
 * Only the accumulate phase differs: factors are formed in int64, their
 * product in 128 bits with overflow detection, and sums accumulate in a
 * 192-bit two's-complement integer (three u64 limbs with carry) so no
 * reachable row count can wrap.  Integer addition is associative: results
 * are bit-identical across runs, grid sizes and atomic orderings.
 * No 128-bit division happens on the device (AVG divides on the host). */
typedef unsigned long long u64_t;
typedef __int128 i128_t;
typedef unsigned __int128 u128_t;

#define DEC_1E38_HI 0x4B3B4CA85A86C47Aull
#define DEC_1E38_LO 0x098A224000000000ull
#define DEC_SIGN 0x8000000000000000ull

/* (l2:l1:l0) += (p2:p1:p0), 192-bit add with carry */
__device__ __forceinline__ void acc192_add(u64_t &l0, u64_t &l1, u64_t &l2,
                                           u64_t p0, u64_t p1, u64_t p2) {
  const u64_t s0 = l0 + p0;
  const u64_t c0 = s0 < p0;
  const u64_t t1 = l1 + p1;
  u64_t c1 = t1 < p1;
  const u64_t s1 = t1 + c0;
  c1 += s1 < c0;              /* wraps only when t1 == ~0 and c0 == 1 */
  l0 = s0; l1 = s1; l2 = l2 + p2 + c1;
}

/* factor i of row r: add + mul * x in int64 (wrap-free for values within
 * the declared precision — proven by the host at submit) */
__device__ __forceinline__ long long dec_factor(const sn_dev_dec_agg &A, int i,
                                                const double *sval, int r) {
  const long long x =
      __double_as_longlong(sval[(size_t)A.c[i] * CHUNK + r]);
  return (long long)((u64_t)A.add[i] + (u64_t)A.mul[i] * (u64_t)x);
}

/* product of the row's factors as a two's-complement i128 (p1:p0).
 * Returns 1 when |product| >= 10^38 (or does not fit 128 bits): the row
 * then poisons its group to NULL instead of contributing. */
__device__ __forceinline__ int dec_product(const sn_dev_dec_agg &A,
                                           const double *sval, int r,
                                           u64_t *p0, u64_t *p1) {
  const u128_t lim = ((u128_t)DEC_1E38_HI << 64) | DEC_1E38_LO;
  const long long f0 = dec_factor(A, 0, sval, r);
  i128_t p = f0;
  if (A.nf >= 2) p = (i128_t)f0 * (i128_t)dec_factor(A, 1, sval, r);
  int ovf;
  if (A.nf >= 3) {
    /* |p| <= 2^126 here; multiply magnitudes limb-wise so the 128-bit
     * overflow is observable without a wider type */
    const long long f2 = dec_factor(A, 2, sval, r);
    const int neg = (p < 0) != (f2 < 0);
    const u128_t a = p < 0 ? (u128_t)0 - (u128_t)p : (u128_t)p;
    const u64_t b = f2 < 0 ? (u64_t)0 - (u64_t)f2 : (u64_t)f2;
    const u128_t hi = (u128_t)(u64_t)(a >> 64) * b;
    const u128_t lo = (u128_t)(u64_t)a * b;
    const u128_t hs = hi << 64;
    const u128_t m = hs + lo;
    ovf = ((u64_t)(hi >> 64) != 0) | (m < hs) | (m >= lim);
    p = neg ? (i128_t)((u128_t)0 - m) : (i128_t)m;
  } else {
    const u128_t a = p < 0 ? (u128_t)0 - (u128_t)p : (u128_t)p;
    ovf = a >= lim;
  }
  *p0 = (u64_t)(u128_t)p;
  *p1 = (u64_t)((u128_t)p >> 64);
  return ovf;
}

/* alive word of row r restricted to rows whose factor columns are all
 * non-null (Spark Sum/Average/Min/Max skip null inputs) */
__device__ __forceinline__ uint64_t dec_valid_word(const sn_dev_dec_agg &A,
                                                   uint64_t w, int clean,
                                                   const uint64_t *svalid,
                                                   int r) {
  if (!clean) {
    if (A.nf >= 1) w &= svalid[(size_t)A.c[0] * (CHUNK / 64) + (r >> 6)];
    if (A.nf >= 2) w &= svalid[(size_t)A.c[1] * (CHUNK / 64) + (r >> 6)];
    if (A.nf >= 3) w &= svalid[(size_t)A.c[2] * (CHUNK / 64) + (r >> 6)];
  }
  return w;
}

__device__ __forceinline__ u64_t dec_cell0_ident(int op) {
  return op == 1 ? ~0ull : 0ull;   /* MIN starts at the top, MAX/SUM at 0 */
}

/* combine accumulator (y2:y1:y0) into (x2:x1:x0): 192-bit sum with carry,
 * or min / max of the sign-biased cell 0 */
__device__ __forceinline__ void dec_fold(int op, u64_t &x0, u64_t &x1,
                                         u64_t &x2, u64_t y0, u64_t y1,
                                         u64_t y2) {
  if (op == 0) acc192_add(x0, x1, x2, y0, y1, y2);
  else if (op == 1) x0 = y0 < x0 ? y0 : x0;
  else x0 = y0 > x0 ? y0 : x0;
}

/* the decimal kernels' LDS: the shared layout with both plan mirrors */
__device__ __forceinline__ ScanLds dec_lds(char *smem, int nused,
                                           const sn_dev_plan *plan_g,
                                           const sn_dev_dec_plan *dec_g) {
  /* (the accumulator size does not move any offset) */
  const ScanLds S = scan_lds(smem, sn_lds_dec(nused, 0, 0), plan_g);
  lds_mirror((sn_dev_dec_plan *)S.plan2, dec_g);
  return S;
}

/* ---- keyless: per-lane register accumulators, reduced across the wave
 * with add-with-carry, block partial rows to scratch with plain stores
 * (the k_keyless -> k_reduce structure: same-address global atomics
 * serialize, see k_keyless) ---- */
template <int NA, int NC>
__global__ __launch_bounds__(WG, 1)
void k_dec_keyless(sn_dev_plan plan,
                   const sn_dev_plan *__restrict__ plan_g,
                   const sn_dev_dec_plan *__restrict__ dec_g,
                   const sn_dev_batch *__restrict__ batches,
                   const sn_dev_tile *__restrict__ tiles, int ntiles,
                   u64_t *__restrict__ out) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int npd = plan.npreds_d, npi = plan.npreds_i;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = dec_lds(smem, nused, plan_g, dec_g);
  const sn_dev_dec_plan *D = (const sn_dev_dec_plan *)S.plan2;
  __syncthreads();
  const int naggs = D->naggs;

  u64_t l0[NA], l1[NA], l2[NA];
  unsigned cnt[NA], ovf[NA];
  unsigned rcnt = 0;
#pragma unroll
  for (int a = 0; a < NA; a++) {
    l0[a] = a < naggs ? dec_cell0_ident(D->aggs[a].op) : 0ull;
    l1[a] = 0; l2[a] = 0; cnt[a] = 0; ovf[a] = 0;
  }

  /* (by-value captures: <12, 4> sits at 255 VGPRs with two waves per SIMD) */
  scan_tiles<NC, 1>(batches, tiles, ntiles, nused, S,
                    ROW_PHASE(=, &l0, &l1, &l2, &cnt, &ovf, &rcnt) {
      alive_init(S.salive, S.sdead, rows, clean);
      pred_sweeps(S.P, npd, npi, clean, S.sval, S.svalid, S.salive);
#pragma unroll
      for (int a = 0; a < NA; a++) {
        if (a >= naggs) break;
        const sn_dev_dec_agg A = D->aggs[a];
#pragma unroll 2
        for (int k = 0; k < CHUNK / WG; k++) {
          const int r = tid + k * WG;
          const uint64_t w =
              dec_valid_word(A, S.salive[r >> 6], clean, S.svalid, r);
          if (w == 0) continue;
          if (!((w >> (tid & 63)) & 1ull)) continue;
          cnt[a]++;
          if (A.op == 0) {
            u64_t p0, p1;
            if (dec_product(A, S.sval, r, &p0, &p1)) ovf[a]++;
            else acc192_add(l0[a], l1[a], l2[a], p0, p1,
                            (p1 & DEC_SIGN) ? ~0ull : 0ull);
          } else {
            const u64_t v = (u64_t)dec_factor(A, 0, S.sval, r) ^ DEC_SIGN;
            l0[a] = A.op == 1 ? (v < l0[a] ? v : l0[a]) : (v > l0[a] ? v : l0[a]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        rcnt += (unsigned)((S.salive[r >> 6] >> (tid & 63)) & 1ull);
      }
  });

  /* wave reduction with carries, then the 4 wave partials fold in LDS */
  const int RC = SN_DEC_ROW_CELLS(naggs);
  u64_t *wpart = (u64_t *)S.acc + RC;      /* [WG/64][RC] */
  const int wid = tid >> 6;
#pragma unroll
  for (int a = 0; a < NA; a++) {
    if (a >= naggs) break;
    const int op = D->aggs[a].op;
    u64_t x0 = l0[a], x1 = l1[a], x2 = l2[a];
    u64_t c = cnt[a], o = ovf[a];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64_t y0 = __shfl_down(x0, off, 64);
      const u64_t y1 = __shfl_down(x1, off, 64);
      const u64_t y2 = __shfl_down(x2, off, 64);
      c += __shfl_down(c, off, 64);
      o += __shfl_down(o, off, 64);
      dec_fold(op, x0, x1, x2, y0, y1, y2);
    }
    if ((tid & 63) == 0) {
      u64_t *cell = wpart + (size_t)wid * RC + a * SN_DEC_CELLS;
      cell[0] = x0; cell[1] = x1; cell[2] = x2; cell[3] = c; cell[4] = o;
    }
  }
  {
    u64_t rc = rcnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rc += __shfl_down(rc, off, 64);
    if ((tid & 63) == 0) wpart[(size_t)wid * RC + RC - 1] = rc;
  }
  __syncthreads();
  if (tid < naggs) {
    const int op = D->aggs[tid].op;
    const u64_t *c0 = wpart + tid * SN_DEC_CELLS;
    u64_t x0 = c0[0], x1 = c0[1], x2 = c0[2], c = c0[3], o = c0[4];
    for (int w = 1; w < WG / 64; w++) {
      const u64_t *cw = c0 + (size_t)w * RC;
      dec_fold(op, x0, x1, x2, cw[0], cw[1], cw[2]);
      c += cw[3]; o += cw[4];
    }
    u64_t *dst = out + (size_t)blockIdx.x * RC + tid * SN_DEC_CELLS;
    dst[0] = x0; dst[1] = x1; dst[2] = x2; dst[3] = c; dst[4] = o;
  } else if (tid == 64) {
    u64_t rc = 0;
    for (int w = 0; w < WG / 64; w++) rc += wpart[(size_t)w * RC + RC - 1];
    out[(size_t)blockIdx.x * RC + RC - 1] = rc;
  }
}

/* ---- grouped: dense slots (dictionary ids / stats-dense integer keys, the
 * slot derivation of k_grouped_lds) into a per-block LDS accumulator with
 * 64-bit LDS atomics; each limb's carry comes from the atomic's returned
 * old value, so the 192-bit sum is exact under any interleaving.  Limb
 * atomics whose addend is zero are skipped (small positive products touch
 * one limb).  Few-group shapes (Q1: 4 live groups) would serialize all 64
 * lanes of a wave on the same LDS address, so the accumulator is replicated
 * `copies` times (power of two, sn_dec_copies) and lane l updates copy
 * l % copies; the copies fold with carries in the single per-block flush. ---- */
template <int NC>
__global__ __launch_bounds__(WG, 1)
void k_dec_grouped(sn_dev_plan plan,
                   const sn_dev_plan *__restrict__ plan_g,
                   const sn_dev_dec_plan *__restrict__ dec_g,
                   const sn_dev_batch *__restrict__ batches,
                   const sn_dev_tile *__restrict__ tiles, int ntiles,
                   u64_t *__restrict__ out, int copies) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int ngroup = plan.ngroup;
  const int npd = plan.npreds_d, npi = plan.npreds_i;
  const int nslots = plan.nslots;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = dec_lds(smem, nused, plan_g, dec_g);
  const sn_dev_dec_plan *D = (const sn_dev_dec_plan *)S.plan2;
  __syncthreads();
  const int naggs = D->naggs;
  const int RC = SN_DEC_ROW_CELLS(naggs);
  const int NV = nslots * RC;
  u64_t *bacc = (u64_t *)S.acc;
  for (int i = tid; i < NV * copies; i += WG) {
    const int ci = i % RC;
    const int a = ci / SN_DEC_CELLS;
    bacc[i] = (ci < RC - 1 && ci % SN_DEC_CELLS == 0)
                  ? dec_cell0_ident(D->aggs[a].op) : 0ull;
  }
  __syncthreads();

  const int gc0 = plan.gcol[0], gc1 = plan.gcol[1];
  scan_tiles<NC, 1>(batches, tiles, ntiles, nused, S, ROW_PHASE(&) {
      alive_init(S.salive, S.sdead, rows, clean);
      pred_sweeps(S.P, npd, npi, clean, S.sval, S.svalid, S.salive);
      /* slot per row first (-1: dead), then aggregate-outer sweeps so each
       * aggregate's parameters are read from the LDS plan mirror once per
       * chunk, not once per row */
      int slots[CHUNK / WG];
      u64_t *const mybase = bacc + (size_t)(tid & (copies - 1)) * NV;
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        const int alive = (int)((S.salive[r >> 6] >> (tid & 63)) & 1ull);
        const int slot = dense_slot<int>(S.P, S.sval, ngroup, gc0, gc1, r);
        /* (a live row's slot is in range by construction; the bound keeps
         * a corrupt key from writing outside the accumulator) */
        slots[k] = (alive && (unsigned)slot < (unsigned)nslots) ? slot : -1;
        if (slots[k] >= 0)
          (void)atomicAdd(&mybase[(size_t)slots[k] * RC + RC - 1], 1ull);
      }
      for (int a = 0; a < naggs; a++) {
        const sn_dev_dec_agg A = D->aggs[a];
#pragma unroll
        for (int k = 0; k < CHUNK / WG; k++) {
          if (slots[k] < 0) continue;
          const int r = tid + k * WG;
          if (!((dec_valid_word(A, ~0ull, clean, S.svalid, r) >> (tid & 63)) & 1ull))
            continue;
          u64_t *cell = mybase + (size_t)slots[k] * RC + a * SN_DEC_CELLS;
          (void)atomicAdd(&cell[3], 1ull);
          if (A.op == 0) {
            u64_t p0, p1;
            if (dec_product(A, S.sval, r, &p0, &p1)) {
              (void)atomicAdd(&cell[4], 1ull);
            } else {
              const u64_t p2 = (p1 & DEC_SIGN) ? ~0ull : 0ull;
              u64_t c0 = 0;
              if (p0) {
                const u64_t old0 = atomicAdd(&cell[0], p0);
                c0 = (u64_t)(old0 + p0) < p0;
              }
              const u64_t a1 = p1 + c0;
              u64_t c1 = a1 < c0;     /* wraps only when p1 == ~0, c0 == 1 */
              if (a1) {
                const u64_t old1 = atomicAdd(&cell[1], a1);
                c1 += (u64_t)(old1 + a1) < a1;
              }
              const u64_t a2 = p2 + c1;
              if (a2) (void)atomicAdd(&cell[2], a2);
            }
          } else {
            const u64_t v = (u64_t)dec_factor(A, 0, S.sval, r) ^ DEC_SIGN;
            if (A.op == 1) (void)atomicMin(&cell[0], v);
            else (void)atomicMax(&cell[0], v);
          }
        }
      }
  });
  __syncthreads();
  /* flush: one thread per (slot, aggregate | rowcount) folds the copies */
  for (int i = tid; i < nslots * (naggs + 1); i += WG) {
    const int slot = i / (naggs + 1), a = i % (naggs + 1);
    u64_t *dst = out + (size_t)blockIdx.x * NV + (size_t)slot * RC;
    if (a == naggs) {
      u64_t rc = 0;
      for (int c = 0; c < copies; c++)
        rc += bacc[(size_t)c * NV + (size_t)slot * RC + RC - 1];
      dst[RC - 1] = rc;
      continue;
    }
    const int op = D->aggs[a].op;
    u64_t x0 = dec_cell0_ident(op), x1 = 0, x2 = 0, cn = 0, ov = 0;
    for (int c = 0; c < copies; c++) {
      const u64_t *cell =
          bacc + (size_t)c * NV + (size_t)slot * RC + a * SN_DEC_CELLS;
      dec_fold(op, x0, x1, x2, cell[0], cell[1], cell[2]);
      cn += cell[3]; ov += cell[4];
    }
    dst += a * SN_DEC_CELLS;
    dst[0] = x0; dst[1] = x1; dst[2] = x2; dst[3] = cn; dst[4] = ov;
  }
}

/* fold the per-block partial rows: one wave per (slot, aggregate) plus one
 * per slot rowcount; lanes stride the blocks, then reduce with carries */
__global__ __launch_bounds__(64)
void k_dec_reduce(const u64_t *__restrict__ scratch, int nblocks, int nslots,
                  const sn_dev_dec_plan *__restrict__ dec_g,
                  u64_t *__restrict__ out) {
  const GAS sn_dev_dec_plan *D = (const GAS sn_dev_dec_plan *)(uintptr_t)dec_g;
  const GAS u64_t *src = (const GAS u64_t *)(uintptr_t)scratch;
  const int naggs = D->naggs;
  const int RC = SN_DEC_ROW_CELLS(naggs);
  const size_t NV = (size_t)nslots * RC;
  const int slot = blockIdx.x / (naggs + 1);
  const int a = blockIdx.x % (naggs + 1);
  if (slot >= nslots) return;
  const int lane = threadIdx.x;
  if (a == naggs) {
    u64_t rc = 0;
    for (int b = lane; b < nblocks; b += 64)
      rc += src[(size_t)b * NV + (size_t)slot * RC + RC - 1];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rc += __shfl_down(rc, off, 64);
    if (lane == 0) out[(size_t)slot * RC + RC - 1] = rc;
    return;
  }
  const int op = D->aggs[a].op;
  u64_t x0 = dec_cell0_ident(op), x1 = 0, x2 = 0, c = 0, o = 0;
  for (int b = lane; b < nblocks; b += 64) {
    const GAS u64_t *cell =
        src + (size_t)b * NV + (size_t)slot * RC + a * SN_DEC_CELLS;
    dec_fold(op, x0, x1, x2, cell[0], cell[1], cell[2]);
    c += cell[3]; o += cell[4];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64_t y0 = __shfl_down(x0, off, 64);
    const u64_t y1 = __shfl_down(x1, off, 64);
    const u64_t y2 = __shfl_down(x2, off, 64);
    c += __shfl_down(c, off, 64);
    o += __shfl_down(o, off, 64);
    dec_fold(op, x0, x1, x2, y0, y1, y2);
  }
  if (lane == 0) {
    u64_t *dst = out + (size_t)slot * RC + a * SN_DEC_CELLS;
    dst[0] = x0; dst[1] = x1; dst[2] = x2; dst[3] = c; dst[4] = o;
  }
}

extern "C" int sn_launch_dec_scan(const sn_dev_plan *plan,
                                  const sn_dev_plan *dev_plan,
                                  const sn_dev_dec_plan *dec,
                                  const sn_dev_dec_plan *dev_dec,
                                  const sn_dev_batch *dev_batches,
                                  const sn_dev_tile *dev_tiles, int32_t ntiles,
                                  unsigned long long *dev_out,
                                  unsigned long long *dev_scratch,
                                  void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ntiles <= 0) return (int)hipErrorInvalidValue;
  const int grid = sn_balanced_grid(ntiles, SN_DEC_GRID_CAP);
  const int keyless = plan->ngroup == 0;
  const int ns = keyless ? 1 : plan->nslots;
  const int na = dec->naggs;
  if (ns < 1 || na < 0 || na > 12) return (int)hipErrorInvalidValue;
  if (sn_dec_lds_bytes(plan->nused, ns, na) > SN_LDS_LIMIT)
    return (int)hipErrorInvalidValue;
  const int copies = keyless ? 1 : sn_dec_copies(plan->nused, ns, na);
  const size_t lds = (size_t)sn_dec_lds_bytes(plan->nused, ns * copies, na);
  const bool nc4 = plan->nused <= 4;
#define KDK(A, NCv) hipLaunchKernelGGL((k_dec_keyless<A, NCv>), dim3(grid), \
        dim3(WG), lds, s, *plan, dev_plan, dev_dec, dev_batches, dev_tiles, \
        ntiles, dev_scratch)
#define KDG(NCv) hipLaunchKernelGGL((k_dec_grouped<NCv>), dim3(grid), \
        dim3(WG), lds, s, *plan, dev_plan, dev_dec, dev_batches, dev_tiles, \
        ntiles, dev_scratch, copies)
  if (keyless) {
    if (na <= 4) { if (nc4) KDK(4, 4); else KDK(4, 8); }
    else { if (nc4) KDK(12, 4); else KDK(12, 8); }
  } else {
    if (nc4) KDG(4); else KDG(8);
  }
#undef KDK
#undef KDG
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(k_dec_reduce, dim3(ns * (na + 1)), dim3(64), 0, s,
                     dev_scratch, grid, ns, dev_dec, dev_out);
  return (int)hipGetLastError();
}

/* ================= row-returning filter scan =================
 * SELECT cols WHERE preds [LIMIT n]: the scan front end and the predicate
 * sweeps of the aggregate kernels leave the per-chunk alive bitmap in LDS;
 * pass 1 keeps it (1 bit per row, plus a match count per tile), a one-block
 * scan turns the counts into output offsets, and pass 2 compacts each chunk's
 * alive rows into an LDS list and copies the projected columns out densely.
 * Row order is the scan order (tile, then row), so it is deterministic. */

/* ---- pass 1: only the predicate columns (slots [0, plan.nused)) are staged;
 * a join scan (JOIN = SN_MARK_INNER / SN_MARK_ANTI) stages the fact key among
 * them and ends its row phase with probe_alive ---- */
template <int NC, int JOIN>
__global__ __launch_bounds__(WG, 4)
void k_select_mark(sn_dev_plan plan,
                   const sn_dev_plan *__restrict__ plan_g,
                   const sn_dev_batch *__restrict__ batches,
                   const sn_dev_tile *__restrict__ tiles, int ntiles,
                   uint64_t *__restrict__ bitmap, int32_t *__restrict__ counts) {
  const int tid = threadIdx.x;
  const int nused = plan.nused;
  const int npd = plan.npreds_d, npi = plan.npreds_i;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScanLds S = scan_lds(smem, sn_lds_select(nused), plan_g);
  __syncthreads();
  /* scan_tiles hands the row phase no tile index: tiles start on multiples
   * of SN_TILE_ROWS, so a chunk at such a base opens this block's next tile */
  int t = (int)blockIdx.x - (int)gridDim.x;
  scan_tiles<NC, 1>(batches, tiles, ntiles, nused, S, ROW_PHASE(=, &t) {
      if ((base & (SN_TILE_ROWS - 1)) == 0) t += (int)gridDim.x;
      alive_init(S.salive, S.sdead, rows, clean);
      pred_sweeps(S.P, npd, npi, clean, S.sval, S.svalid, S.salive);
      if constexpr (JOIN != SN_MARK_NOJOIN)
        probe_alive<JOIN == SN_MARK_ANTI>(S.P, clean, S.sval, S.svalid,
                                          S.salive);
      /* each wave stores the words it owns (alive_init's ownership rule) */
      if ((tid & 63) == 0) {
        uint64_t *dst = bitmap + (size_t)t * SN_SEL_TILE_WORDS +
                        (size_t)((base & (SN_TILE_ROWS - 1)) / CHUNK) * (CHUNK / 64);
        int n = 0;
#pragma unroll
        for (int k = 0; k < CHUNK / WG; k++) {
          const int w = (tid + k * WG) >> 6;
          const uint64_t aw = S.salive[w];
          dst[w] = aw;
          n += __popcll(aw);
        }
        if (n) (void)atomicAdd(&counts[t], n);
      }
  });
}

extern "C" int sn_launch_select_mark(const sn_dev_plan *plan,
                                     const sn_dev_plan *dev_plan,
                                     const sn_dev_batch *dev_batches,
                                     const sn_dev_tile *dev_tiles,
                                     int32_t ntiles, uint64_t *bitmap,
                                     int32_t *counts, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ntiles <= 0 || plan->nused < 0 || plan->nused > SN_DEV_MAX_COLS)
    return (int)hipErrorInvalidValue;
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  const size_t lds = (size_t)sn_lds_select(plan->nused).total;
  if (plan->nused <= 4)
    hipLaunchKernelGGL((k_select_mark<4, SN_MARK_NOJOIN>), dim3(grid), dim3(WG),
                       lds, s, *plan, dev_plan, dev_batches, dev_tiles, ntiles,
                       bitmap, counts);
  else
    hipLaunchKernelGGL((k_select_mark<8, SN_MARK_NOJOIN>), dim3(grid), dim3(WG),
                       lds, s, *plan, dev_plan, dev_batches, dev_tiles, ntiles,
                       bitmap, counts);
  return (int)hipGetLastError();
}

extern "C" int sn_launch_select_mark_join(const sn_dev_plan *plan,
                                          const sn_dev_plan *dev_plan,
                                          const sn_dev_batch *dev_batches,
                                          const sn_dev_tile *dev_tiles,
                                          int32_t ntiles, int32_t mark,
                                          uint64_t *bitmap, int32_t *counts,
                                          void *stream) {
  hipStream_t s = (hipStream_t)stream;
  /* the key is staged: without a table, or with the key slot outside the
   * staged ones, the probe would read what pass 1 never wrote */
  if (ntiles <= 0 || plan->nused < 1 || plan->nused > SN_DEV_MAX_COLS ||
      (mark != SN_MARK_INNER && mark != SN_MARK_ANTI) || !plan->jkeys ||
      !plan->jpayload || plan->jcslot < 0 || plan->jcslot >= plan->nused ||
      plan->jcap_log2 < 1 || plan->jcap_log2 > 31)
    return (int)hipErrorInvalidValue;
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  const size_t lds = (size_t)sn_lds_select(plan->nused).total;
#define KSM(NCv, Jv) hipLaunchKernelGGL((k_select_mark<NCv, Jv>), dim3(grid), \
        dim3(WG), lds, s, *plan, dev_plan, dev_batches, dev_tiles, ntiles,    \
        bitmap, counts)
  if (mark == SN_MARK_INNER) {
    if (plan->nused <= 4) KSM(4, SN_MARK_INNER); else KSM(8, SN_MARK_INNER);
  } else {
    if (plan->nused <= 4) KSM(4, SN_MARK_ANTI); else KSM(8, SN_MARK_ANTI);
  }
#undef KSM
  return (int)hipGetLastError();
}

/* ---- exclusive scan of the tile counts: one block, WG counts per step with
 * the running total carried from step to step ---- */
__global__ __launch_bounds__(WG, 1)
void k_tile_offsets(const int32_t *__restrict__ counts, int n,
                    int64_t *__restrict__ offsets, int64_t *__restrict__ total) {
  __shared__ long long wsum[WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < n; base += WG) {
    const int i = base + tid;
    const long long v = i < n ? (long long)counts[i] : 0;
    long long x = v;                       /* inclusive scan within the wave */
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; w++) {
      const long long ws = wsum[w];
      before += w < wid ? ws : 0;
      all += ws;
    }
    if (i < n) offsets[i] = carry + before + x - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

extern "C" int sn_launch_tile_offsets(const int32_t *counts, int32_t n,
                                      int64_t *offsets, int64_t *total,
                                      void *stream) {
  if (n < 0 || !total || (n > 0 && (!counts || !offsets)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tile_offsets, dim3(1), dim3(WG), 0, (hipStream_t)stream,
                     counts, n, offsets, total);
  return (int)hipGetLastError();
}

/* ---- pass 2 ----
 * one projected value of source row `row` to output row `o`.  Everything the
 * switches test is uniform over the block (the batch's kind, the output
 * type), so they are scalar branches.  Values are copied, never recomputed:
 * f64 and f32 travel as their integer bit patterns. */
__device__ __forceinline__ void select_emit(const sn_dev_col &c, int direct,
                                            int otype, int row, void *val_,
                                            uint8_t *valid, long long o) {
  int ok = 1, gid = 0;
  long long vi = 0;          /* integer value, or the f64 bit pattern */
  unsigned fbits = 0;        /* f32 bit pattern */
  int have = 0;
  if (direct) {
    have = 1;
    switch (c.kind) {
      case SN_K_F64: vi = as_global((const long long *)c.body)[row]; break;
      case SN_K_F64C8:
        vi = as_global((const long long *)c.rle_vals)
            [as_global((const uint8_t *)c.body)[row]];
        break;
      case SN_K_I64: vi = as_global((const long long *)c.body)[row]; break;
      case SN_K_I32: vi = as_global((const int32_t *)c.body)[row]; break;
      case SN_K_F32: fbits = as_global((const unsigned *)c.body)[row]; break;
      case SN_K_I16: vi = as_global((const int16_t *)c.body)[row]; break;
      case SN_K_S8: vi = as_global((const int8_t *)c.body)[row]; break;
      case SN_K_U8: vi = as_global((const uint8_t *)c.body)[row] == 1; break;
      default: have = 0; break;
    }
  }
  if (!have) {
    double vd = 0.0;
    ok = read_general(c, row, &vd, &vi, &gid);
    if (otype == SN_TYPE_DOUBLE) vi = __double_as_longlong(vd);
    else if (otype == SN_TYPE_FLOAT) fbits = __float_as_uint((float)vd);
    else if (otype == SN_TYPE_STRING) vi = gid;
    if (!ok) { vi = 0; fbits = 0; }
  }
  switch (otype) {
    case SN_TYPE_DOUBLE: case SN_TYPE_INT64:
      ((long long *)val_)[o] = vi; break;
    case SN_TYPE_INT32: case SN_TYPE_STRING:
      ((int32_t *)val_)[o] = (int32_t)vi; break;
    case SN_TYPE_FLOAT: ((unsigned *)val_)[o] = fbits; break;
    case SN_TYPE_INT16: ((int16_t *)val_)[o] = (int16_t)vi; break;
    case SN_TYPE_INT8: ((int8_t *)val_)[o] = (int8_t)vi; break;
    case SN_TYPE_BOOL: ((uint8_t *)val_)[o] = (uint8_t)(vi != 0); break;
  }
  valid[o] = (uint8_t)ok;
}

/* the SN_SEL_DIM_ATTR projection of source row `row`: read the fact key the
 * way select_emit reads a value (so it is the key pass 1 probed: patches,
 * NULLs and run-length bodies included), look it up, store the attribute id.
 * A row that does not join (NULL or absent key) gets id 0, validity 0. */
__device__ __forceinline__ void select_emit_attr(const sn_dev_select &sel,
                                                 const sn_dev_col &c,
                                                 int direct, int row,
                                                 void *val_, uint8_t *valid,
                                                 long long o) {
  int ok = 1, have = 0;
  long long key = 0;
  if (direct) {
    have = 1;
    switch (c.kind) {
      case SN_K_I64: key = as_global((const long long *)c.body)[row]; break;
      case SN_K_I32: key = as_global((const int32_t *)c.body)[row]; break;
      default: have = 0; break;
    }
  }
  if (!have) {
    double vd = 0.0;
    int gid = 0;
    ok = read_general(c, row, &vd, &key, &gid);
  }
  int pay = -1;
  if (ok)
    pay = join_lookup((const GAS long long *)(uintptr_t)sel.jkeys,
                      (const GAS int32_t *)(uintptr_t)sel.jpayload,
                      (1u << sel.jcap_log2) - 1,
                      (const GAS int32_t *)(uintptr_t)sel.jlut, sel.jlut_min,
                      sel.jlut_max, key);
  ((int32_t *)val_)[o] = pay >= 0 ? pay : 0;
  valid[o] = (uint8_t)(pay >= 0);
}

/* ATTR = 0 is the gather of a scan without an attribute projection: the
 * lookup is compiled out, so plain selects keep their registers and speed */
template <int ATTR>
__global__ __launch_bounds__(WG, 4)
void k_select_gather(sn_dev_select sel,
                     const sn_dev_batch *__restrict__ batches,
                     const sn_dev_tile *__restrict__ tiles, int ntiles,
                     const uint64_t *__restrict__ bitmap,
                     const int32_t *__restrict__ counts,
                     const int64_t *__restrict__ offsets,
                     const int32_t *__restrict__ table_batch) {
  __shared__ uint64_t sword[CHUNK / 64];
  __shared__ int spfx[CHUNK / 64 + 1];
  __shared__ uint16_t slist[CHUNK];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long tile_off = offsets[t];
    if (counts[t] == 0 || tile_off >= sel.out_rows) continue;   /* uniform */
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int num_rows = b.num_rows;
    const int tile_end = min(tile.row_start + SN_TILE_ROWS, num_rows);
    const int direct = b.clean;
    const long long rowid_hi = (long long)table_batch[tile.batch] << 32;
    const uint64_t *tw = bitmap + (size_t)t * SN_SEL_TILE_WORDS;
    long long running = tile_off;
    for (int base = tile.row_start; base < tile_end && running < sel.out_rows;
         base += CHUNK) {
      if (tid < CHUNK / 64)
        sword[tid] = as_global(tw)[((base - tile.row_start) / CHUNK) *
                                   (CHUNK / 64) + tid];
      __syncthreads();
      if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < CHUNK / 64; w++) {
          spfx[w] = acc;
          acc += __popcll(sword[w]);
        }
        spfx[CHUNK / 64] = acc;
      }
      __syncthreads();
      /* rank of an alive row = alive rows before it in the chunk */
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        const uint64_t aw = sword[r >> 6];
        if ((aw >> lane) & 1ull)
          slist[spfx[r >> 6] + __popcll(aw & ((1ull << lane) - 1ull))] =
              (uint16_t)r;
      }
      __syncthreads();
      const int nalive = spfx[CHUNK / 64];
      for (int p = 0; p < sel.nproj; p++) {
        const int otype = sel.otype[p];
        void *val = sel.val[p];
        uint8_t *valid = sel.valid[p];
        if (otype == SN_SEL_ROWID) {
          for (int j = tid; j < nalive; j += WG) {
            const long long o = running + j;
            if (o >= sel.out_rows) break;
            ((long long *)val)[o] = rowid_hi | (long long)(base + slist[j]);
            valid[o] = 1;
          }
          continue;
        }
        if constexpr (ATTR) {
          if (otype == SN_SEL_DIM_ATTR) {
            const sn_dev_col &kc = b.cols[sel.jcslot];
            for (int j = tid; j < nalive; j += WG) {
              const long long o = running + j;
              const int row = base + slist[j];
              if (o >= sel.out_rows || row >= num_rows) break;
              select_emit_attr(sel, kc, direct, row, val, valid, o);
            }
            continue;
          }
        }
        const sn_dev_col &c = b.cols[sel.cslot[p]];
        for (int j = tid; j < nalive; j += WG) {
          const long long o = running + j;
          const int row = base + slist[j];
          if (o >= sel.out_rows || row >= num_rows) break;
          select_emit(c, direct, otype, row, val, valid, o);
        }
      }
      running += nalive;
      __syncthreads();       /* slist and sword are rewritten next chunk */
    }
  }
}

/* a DIM_ATTR projection needs the dimension descriptor (both gather launchers) */
static bool sel_join_ok(const sn_dev_select *sel) {
  for (int p = 0; p < sel->nproj; p++)
    if (sel->otype[p] == SN_SEL_DIM_ATTR &&
        (!sel->jkeys || !sel->jpayload || sel->jcslot < 0 ||
         sel->jcslot >= SN_DEV_MAX_COLS || sel->jcap_log2 < 1 ||
         sel->jcap_log2 > 31))
      return false;
  return true;
}
static bool sel_has_attr(const sn_dev_select *sel) {
  for (int p = 0; p < sel->nproj; p++)
    if (sel->otype[p] == SN_SEL_DIM_ATTR) return true;
  return false;
}

extern "C" int sn_launch_select_gather(const sn_dev_select *sel,
                                       const sn_dev_batch *dev_batches,
                                       const sn_dev_tile *dev_tiles,
                                       int32_t ntiles, const uint64_t *bitmap,
                                       const int32_t *counts,
                                       const int64_t *offsets,
                                       const int32_t *table_batch,
                                       void *stream) {
  if (ntiles <= 0 || sel->nproj < 1 || sel->nproj > SN_SEL_MAX_PROJ ||
      sel->out_rows <= 0 || !sel_join_ok(sel))
    return (int)hipErrorInvalidValue;
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  if (sel_has_attr(sel))
    hipLaunchKernelGGL(k_select_gather<1>, dim3(grid), dim3(WG), 0,
                       (hipStream_t)stream, *sel, dev_batches, dev_tiles,
                       ntiles, bitmap, counts, offsets, table_batch);
  else
    hipLaunchKernelGGL(k_select_gather<0>, dim3(grid), dim3(WG), 0,
                       (hipStream_t)stream, *sel, dev_batches, dev_tiles,
                       ntiles, bitmap, counts, offsets, table_batch);
  return (int)hipGetLastError();
}

/* ================= ordered row scan =================
 * SELECT cols WHERE preds ORDER BY key LIMIT k.  Pass 1 (k_select_mark) and
 * k_tile_offsets have left the alive bitmap and the tile counts.  A radix
 * select, 11 bits a pass from the top, finds the image T of the k-th smallest
 * key among the alive rows; the rows below T and the first `need` rows equal
 * to T (in scan order) are the result; one workgroup sorts them and the
 * gather projects them in that order.  Nothing is read back in between. */

/* the key of one row in two steps, so that a walk can issue the loads of
 * several rows before it needs the first value.  order_load reads the value
 * the way select_emit reads it: *vi the integer value, the f64 bit pattern or
 * the STRING's global id, *fbits the f32 pattern; returns 0 for a NULL. */
__device__ __forceinline__ int order_load(const sn_dev_order &od,
                                          const sn_dev_col &c, int direct,
                                          int row, long long *vi_,
                                          unsigned *fbits_) {
  int ok = 1, gid = 0, have = 0;
  long long vi = 0;
  unsigned fbits = 0;
  if (direct) {
    have = 1;
    switch (c.kind) {
      case SN_K_F64: vi = as_global((const long long *)c.body)[row]; break;
      case SN_K_F64C8:
        vi = as_global((const long long *)c.rle_vals)
            [as_global((const uint8_t *)c.body)[row]];
        break;
      case SN_K_I64: vi = as_global((const long long *)c.body)[row]; break;
      case SN_K_I32: vi = as_global((const int32_t *)c.body)[row]; break;
      case SN_K_F32: fbits = as_global((const unsigned *)c.body)[row]; break;
      case SN_K_I16: vi = as_global((const int16_t *)c.body)[row]; break;
      case SN_K_S8: vi = as_global((const int8_t *)c.body)[row]; break;
      case SN_K_U8: vi = as_global((const uint8_t *)c.body)[row] == 1; break;
      default: have = 0; break;
    }
  }
  if (!have) {
    double vd = 0.0;
    ok = read_general(c, row, &vd, &vi, &gid);
    if (od.dtype == SN_TYPE_DOUBLE) vi = __double_as_longlong(vd);
    else if (od.dtype == SN_TYPE_FLOAT) fbits = __float_as_uint((float)vd);
    else if (od.dtype == SN_TYPE_STRING) vi = gid;
  }
  *vi_ = vi;
  *fbits_ = fbits;
  return ok;
}

/* key image from order_load's outputs: the class, and through *key the u64
 * (0 for a NULL) */
__device__ __forceinline__ int order_image(const sn_dev_order &od, int ok,
                                           long long vi, unsigned fbits,
                                           unsigned long long *key) {
  if (!ok) { *key = 0; return od.null_cls; }
  if (od.dtype == SN_TYPE_STRING)
    vi = (unsigned)vi < (unsigned)od.nranks ? as_global(od.ranks)[(int)vi]
                                            : 0x7fffffff;
  *key = sn_order_image(od.dtype, vi, fbits, od.desc);
  return SN_ORD_CLS_VALUE;
}

/* The walks below take one 1,024-row chunk at a time: cw points at its 16
 * alive words, lane l of a wave owns bit l of word (tid + k * WG) >> 6.  All
 * four words are loaded first, then all four keys, and only then does anything
 * wait on a value: a block walks its tiles alone, so its pace is the number of
 * dependent load latencies per chunk (two this way, eight when each word and
 * each key is loaded where it is used). */
#define ORDER_CHUNK_LOADS()                                                  \
  uint64_t aw[CHUNK / WG];                                                   \
  long long vi[CHUNK / WG];                                                  \
  unsigned fb[CHUNK / WG];                                                   \
  int ok[CHUNK / WG], live[CHUNK / WG];                                      \
  _Pragma("unroll")                                                          \
  for (int k = 0; k < CHUNK / WG; k++) aw[k] = cw[(tid + k * WG) >> 6];      \
  _Pragma("unroll")                                                          \
  for (int k = 0; k < CHUNK / WG; k++) {                                     \
    const int row_ = base + tid + k * WG;                                    \
    live[k] = (int)((aw[k] >> lane) & 1ull) && row_ < tile_end;              \
    vi[k] = 0; fb[k] = 0; ok[k] = 0;                                         \
    if (live[k]) ok[k] = order_load(od, c, direct, row_, &vi[k], &fb[k]);    \
  }

/* ---- radix select, counting half: the next digit of every alive row whose
 * image still matches the prefix, into a per-block LDS histogram ---- */
__global__ __launch_bounds__(WG, 4)
void k_order_hist(sn_dev_order od, const sn_dev_batch *__restrict__ batches,
                  const sn_dev_tile *__restrict__ tiles, int ntiles,
                  const uint64_t *__restrict__ bitmap,
                  const int32_t *__restrict__ counts,
                  const sn_order_state *__restrict__ state,
                  unsigned long long *__restrict__ hist, int pass, int shift) {
  __shared__ unsigned shist[SN_ORD_HIST];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long prefix = 0, himask = 0;
  if (pass > 0) {
    /* T is a NULL class: no digit is left to decide (uniform) */
    if (state->cls != SN_ORD_CLS_VALUE) return;
    prefix = state->prefix;
    himask = ~0ull << (shift + SN_ORD_DIGIT_BITS);
  }
  for (int i = tid; i < SN_ORD_HIST; i += WG) shist[i] = 0;
  __syncthreads();
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (counts[t] == 0) continue;                               /* uniform */
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int tile_end = min(tile.row_start + SN_TILE_ROWS, b.num_rows);
    const int direct = b.clean;
    const sn_dev_col &c = b.cols[od.cslot];
    const uint64_t *tw = bitmap + (size_t)t * SN_SEL_TILE_WORDS;
    for (int base = tile.row_start; base < tile_end; base += CHUNK) {
      const uint64_t *cw = tw + ((base - tile.row_start) / CHUNK) * (CHUNK / 64);
      ORDER_CHUNK_LOADS();
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        if (aw[k] == 0) continue;                               /* uniform */
        int bin = -1;
        if (live[k]) {
          unsigned long long key;
          const int cls = order_image(od, ok[k], vi[k], fb[k], &key);
          const int digit = 1 + (int)((key >> shift) & (SN_ORD_BINS - 1));
          if (pass == 0)
            bin = cls == SN_ORD_CLS_VALUE ? digit
                : cls == SN_ORD_CLS_FIRST ? 0 : SN_ORD_BINS + 1;
          else if (cls == SN_ORD_CLS_VALUE && ((key ^ prefix) & himask) == 0)
            bin = digit;
        }
        /* the high digits of dates and prices put a whole wave in one bin:
         * the lanes that agree with the first active lane add once */
        const unsigned long long am = __ballot(bin >= 0);
        if (am) {
          const int leader = __ffsll((long long)am) - 1;
          const int b0 = __shfl(bin, leader, 64);
          const unsigned long long same = __ballot(bin == b0);
          if (lane == leader) atomicAdd(&shist[b0], (unsigned)__popcll(same));
          else if (bin >= 0 && bin != b0) atomicAdd(&shist[bin], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < SN_ORD_HIST; i += WG) {
    const unsigned v = shist[i];
    if (v) atomicAdd(&hist[i], (unsigned long long)v);
  }
}

/* ---- radix select, deciding half: one workgroup finds the bin in which the
 * running count reaches `need`, extends the prefix by its digit and leaves
 * the rank wanted inside that bin ---- */
__global__ __launch_bounds__(WG, 1)
void k_order_pick(const unsigned long long *__restrict__ hist,
                  sn_order_state *__restrict__ state, int pass, int shift,
                  int k_eff) {
  constexpr int PER = (SN_ORD_HIST + WG - 1) / WG;
  __shared__ long long wsum[WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (pass > 0 && state->cls != SN_ORD_CLS_VALUE) return;       /* uniform */
  const long long need = pass == 0 ? (long long)k_eff : state->need;
  const unsigned long long prefix = pass == 0 ? 0 : state->prefix;
  long long cnt[PER], mine = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int bin = tid * PER + i;
    cnt[i] = bin < SN_ORD_HIST ? (long long)hist[bin] : 0;
    mine += cnt[i];
  }
  long long x = mine;                       /* inclusive scan within the wave */
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();                 /* also: every thread has read the state */
  long long before = x - mine;
  for (int w = 0; w < wid; w++) before += wsum[w];
  /* the bin holding the row of 0-based rank need - 1: exactly one thread */
  if (before < need && need <= before + mine) {
    long long run = before;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (run < need && need <= run + cnt[i]) {
        const int bin = tid * PER + i;
        state->need = need - run;
        if (pass == 0) {
          state->cursor = 0;
          state->cls = bin == 0 ? SN_ORD_CLS_FIRST
                     : bin == SN_ORD_BINS + 1 ? SN_ORD_CLS_LAST
                     : SN_ORD_CLS_VALUE;
        }
        if (bin >= 1 && bin <= SN_ORD_BINS)
          state->prefix = prefix | ((unsigned long long)(bin - 1) << shift);
        else
          state->prefix = 0;
      }
      run += cnt[i];
    }
  }
}

/* rows of tile t equal to T, per tile */
__global__ __launch_bounds__(WG, 4)
void k_order_count(sn_dev_order od, const sn_dev_batch *__restrict__ batches,
                   const sn_dev_tile *__restrict__ tiles, int ntiles,
                   const uint64_t *__restrict__ bitmap,
                   const int32_t *__restrict__ counts,
                   const sn_order_state *__restrict__ state,
                   int32_t *__restrict__ eq_counts) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int tcls = state->cls;
  const unsigned long long tkey = state->prefix;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (counts[t] == 0) continue;                               /* uniform */
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int tile_end = min(tile.row_start + SN_TILE_ROWS, b.num_rows);
    const int direct = b.clean;
    const sn_dev_col &c = b.cols[od.cslot];
    const uint64_t *tw = bitmap + (size_t)t * SN_SEL_TILE_WORDS;
    int n = 0;                               /* this wave's equals (uniform) */
    for (int base = tile.row_start; base < tile_end; base += CHUNK) {
      const uint64_t *cw = tw + ((base - tile.row_start) / CHUNK) * (CHUNK / 64);
      ORDER_CHUNK_LOADS();
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        if (aw[k] == 0) continue;                               /* uniform */
        int eq = 0;
        if (live[k]) {
          unsigned long long key;
          const int cls = order_image(od, ok[k], vi[k], fb[k], &key);
          eq = cls == tcls && key == tkey;
        }
        n += __popcll(__ballot(eq));
      }
    }
    if (lane == 0 && n) (void)atomicAdd(&eq_counts[t], n);
  }
}

/* ---- candidates: every alive row below T, and the rows equal to T whose
 * scan-order rank among the equals is below `need` ---- */
__global__ __launch_bounds__(WG, 4)
void k_order_collect(sn_dev_order od, const sn_dev_batch *__restrict__ batches,
                     const sn_dev_tile *__restrict__ tiles, int ntiles,
                     const uint64_t *__restrict__ bitmap,
                     const int32_t *__restrict__ counts,
                     sn_order_state *__restrict__ state,
                     const int64_t *__restrict__ eq_offsets,
                     sn_order_ent *__restrict__ cand, int k_eff) {
  __shared__ uint64_t seq[CHUNK / 64];       /* the chunk's equal rows */
  const int tid = threadIdx.x, lane = tid & 63;
  const int tcls = state->cls;
  const unsigned long long tkey = state->prefix;
  const long long need = state->need;
  const unsigned long long below_lane = (1ull << lane) - 1ull;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (counts[t] == 0) continue;                               /* uniform */
    const sn_dev_tile tile = tiles[t];
    const sn_dev_batch &b = batches[tile.batch];
    const int tile_end = min(tile.row_start + SN_TILE_ROWS, b.num_rows);
    const int direct = b.clean;
    const sn_dev_col &c = b.cols[od.cslot];
    const uint64_t *tw = bitmap + (size_t)t * SN_SEL_TILE_WORDS;
    const unsigned long long pos_hi = (unsigned long long)tile.batch << 32;
    long long eq_run = eq_offsets[t];        /* equals before this chunk */
    for (int base = tile.row_start; base < tile_end; base += CHUNK) {
      const uint64_t *cw = tw + ((base - tile.row_start) / CHUNK) * (CHUNK / 64);
      unsigned long long key[CHUNK / WG], eqm[CHUNK / WG];
      int rel[CHUNK / WG];                   /* 0 above T, 1 below, 2 equal */
      int cl[CHUNK / WG];
      ORDER_CHUNK_LOADS();
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        key[k] = 0; rel[k] = 0; cl[k] = 0;
        if (live[k]) {
          cl[k] = order_image(od, ok[k], vi[k], fb[k], &key[k]);
          if (cl[k] < tcls || (cl[k] == tcls && key[k] < tkey)) rel[k] = 1;
          else if (cl[k] == tcls && key[k] == tkey) rel[k] = 2;
        }
        eqm[k] = __ballot(rel[k] == 2);
        if (lane == 0) seq[r >> 6] = eqm[k];
      }
      __syncthreads();
      long long chunk_eq = 0;
#pragma unroll
      for (int k = 0; k < CHUNK / WG; k++) {
        const int r = tid + k * WG;
        int take = rel[k] == 1;
        if (rel[k] == 2) {
          /* in-chunk rank by the word-popcount prefix, as k_select_gather */
          long long rank = eq_run + __popcll(eqm[k] & below_lane);
          for (int w = 0; w < (r >> 6); w++) rank += __popcll(seq[w]);
          take = rank < need;
        }
        const unsigned long long tm = __ballot(take);
        if (tm) {
          const int leader = __ffsll((long long)tm) - 1;
          int at = 0;
          if (lane == leader) at = atomicAdd(&state->cursor, __popcll(tm));
          at = __shfl(at, leader, 64);
          const int o = at + __popcll(tm & below_lane);
          if (take && o < k_eff) {           /* every store guarded by k_eff */
            sn_order_ent ent;
            ent.key = key[k];
            ent.cp = ((unsigned long long)cl[k] << 62) | pos_hi |
                     (unsigned long long)(unsigned)(base + r);
            cand[o] = ent;
          }
        }
      }
#pragma unroll
      for (int w = 0; w < CHUNK / 64; w++) chunk_eq += __popcll(seq[w]);
      eq_run += chunk_eq;
      __syncthreads();                       /* seq is rewritten next chunk */
    }
  }
}

extern "C" int sn_launch_order_select(const sn_dev_order *od,
                                      const sn_dev_batch *dev_batches,
                                      const sn_dev_tile *dev_tiles,
                                      int32_t ntiles, const uint64_t *bitmap,
                                      const int32_t *counts,
                                      sn_order_state *state,
                                      unsigned long long *hist,
                                      int32_t *eq_counts, int64_t *eq_offsets,
                                      int64_t *eq_total, sn_order_ent *cand,
                                      int32_t k_eff, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ntiles <= 0 || k_eff < 1 || k_eff > SN_ORDER_MAX_LIMIT ||
      od->npass < 1 || od->npass > SN_ORD_MAX_PASSES ||
      od->cslot < 0 || od->cslot >= SN_DEV_MAX_COLS)
    return (int)hipErrorInvalidValue;
  const int grid = sn_balanced_grid(ntiles, SN_GRID_CAP);
  for (int p = 0; p < od->npass; p++) {
    const int shift = SN_ORD_DIGIT_BITS * (od->npass - 1 - p);
    unsigned long long *h = hist + (size_t)p * SN_ORD_HIST;
    hipLaunchKernelGGL(k_order_hist, dim3(grid), dim3(WG), 0, s, *od,
                       dev_batches, dev_tiles, ntiles, bitmap, counts, state,
                       h, p, shift);
    hipLaunchKernelGGL(k_order_pick, dim3(1), dim3(WG), 0, s, h, state, p,
                       shift, k_eff);
  }
  hipLaunchKernelGGL(k_order_count, dim3(grid), dim3(WG), 0, s, *od,
                     dev_batches, dev_tiles, ntiles, bitmap, counts, state,
                     eq_counts);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  int rc = sn_launch_tile_offsets(eq_counts, ntiles, eq_offsets, eq_total, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_order_collect, dim3(grid), dim3(WG), 0, s, *od,
                     dev_batches, dev_tiles, ntiles, bitmap, counts, state,
                     eq_offsets, cand, k_eff);
  return (int)hipGetLastError();
}

/* ---- sort: one workgroup, a bitonic network over the next power of two of
 * entries in LDS (16 B each: 128 KiB at 8,192), padded with entries above
 * every real one ---- */
#define ORDER_SORT_WG 1024
__device__ __forceinline__ bool order_less(const sn_order_ent &a,
                                           const sn_order_ent &b) {
  const unsigned ca = (unsigned)(a.cp >> 62), cb = (unsigned)(b.cp >> 62);
  if (ca != cb) return ca < cb;
  if (a.key != b.key) return a.key < b.key;
  return a.cp < b.cp;
}

__global__ __launch_bounds__(ORDER_SORT_WG, 1)
void k_order_sort(sn_order_ent *__restrict__ ents, int n, int np2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  sn_order_ent *s = (sn_order_ent *)smem;
  const int tid = threadIdx.x;
  for (int i = tid; i < np2; i += ORDER_SORT_WG) {
    sn_order_ent e;
    e.key = ~0ull; e.cp = ~0ull;
    if (i < n) e = ents[i];
    s[i] = e;
  }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (np2 >> 1); t += ORDER_SORT_WG) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool up = (i & k) == 0;
        const sn_order_ent a = s[i], b = s[l];
        if (up ? order_less(b, a) : order_less(a, b)) { s[i] = b; s[l] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += ORDER_SORT_WG) ents[i] = s[i];
}

extern "C" int sn_launch_order_sort(sn_order_ent *ents, int32_t n,
                                    void *stream) {
  if (n < 0 || n > SN_ORDER_MAX_LIMIT || (n > 0 && !ents))
    return (int)hipErrorInvalidValue;
  if (n <= 1) return 0;
  int np2 = 2;
  while (np2 < n) np2 <<= 1;
  hipLaunchKernelGGL(k_order_sort, dim3(1), dim3(ORDER_SORT_WG),
                     (size_t)np2 * sizeof(sn_order_ent), (hipStream_t)stream,
                     ents, n, np2);
  return (int)hipGetLastError();
}

/* ---- ordered gather: output row j is candidate j.  The batch, and with it
 * select_emit's switches, now differs from lane to lane: divergence on at
 * most SN_ORDER_MAX_LIMIT rows.  ATTR as in k_select_gather ---- */
template <int ATTR>
__global__ __launch_bounds__(WG, 4)
void k_order_gather(sn_dev_select sel,
                    const sn_dev_batch *__restrict__ batches,
                    const sn_order_ent *__restrict__ cand,
                    const int32_t *__restrict__ table_batch) {
  const long long j = (long long)blockIdx.x * WG + threadIdx.x;
  if (j >= sel.out_rows) return;
  const unsigned long long pos = cand[j].cp & SN_ORD_POS_MASK;
  const int bi = (int)(pos >> 32), row = (int)(pos & 0xffffffffull);
  const sn_dev_batch &b = batches[bi];
  if (row >= b.num_rows) return;
  for (int p = 0; p < sel.nproj; p++) {
    const int otype = sel.otype[p];
    if (otype == SN_SEL_ROWID) {
      ((long long *)sel.val[p])[j] =
          ((long long)table_batch[bi] << 32) | (long long)row;
      sel.valid[p][j] = 1;
      continue;
    }
    if constexpr (ATTR) {
      if (otype == SN_SEL_DIM_ATTR) {
        select_emit_attr(sel, b.cols[sel.jcslot], b.clean, row, sel.val[p],
                         sel.valid[p], j);
        continue;
      }
    }
    select_emit(b.cols[sel.cslot[p]], b.clean, otype, row, sel.val[p],
                sel.valid[p], j);
  }
}

extern "C" int sn_launch_order_gather(const sn_dev_select *sel,
                                      const sn_dev_batch *dev_batches,
                                      const sn_order_ent *cand,
                                      const int32_t *table_batch,
                                      void *stream) {
  if (sel->nproj < 1 || sel->nproj > SN_SEL_MAX_PROJ || sel->out_rows <= 0 ||
      sel->out_rows > SN_ORDER_MAX_LIMIT || !sel_join_ok(sel))
    return (int)hipErrorInvalidValue;
  const int grid = (int)((sel->out_rows + WG - 1) / WG);
  if (sel_has_attr(sel))
    hipLaunchKernelGGL(k_order_gather<1>, dim3(grid), dim3(WG), 0,
                       (hipStream_t)stream, *sel, dev_batches, cand,
                       table_batch);
  else
    hipLaunchKernelGGL(k_order_gather<0>, dim3(grid), dim3(WG), 0,
                       (hipStream_t)stream, *sel, dev_batches, cand,
                       table_batch);
  return (int)hipGetLastError();
}
