/*
 * blob_format.h — the byte formats the put path accepts, as pure
 * bytes-in / values-out functions: no HIP, no engine state, no locks.
 *
 * Everything that reads a caller's bytes goes through BlobReader, which
 * refuses to step past the end of its buffer, so a truncated or corrupt blob
 * ends in SN_ERR_BADFORMAT here and never reaches a kernel.  Functions return
 * SN_* codes; the engine adds the column number and calls fail().
 *
 * Formats (SnappyData reference): column blob header ColumnEncoding.scala:
 * 37-53,764-832; dictionaries DictionaryEncoding.scala:85-160; var-width
 * strings Uncompressed.scala:117-160; run lengths RunLengthEncoding.scala:
 * 99-172; update deltas ColumnDeltaDecoder.scala:31-120; delete masks
 * ColumnDeleteDecoder.scala:24-55.
 */
#ifndef SN_BLOB_FORMAT_H
#define SN_BLOB_FORMAT_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/snappy_engine.h"

/* little-endian readers (host is LE) for bytes already proven in range */
static inline int32_t rd_i32(const uint8_t *p) { int32_t v; memcpy(&v, p, 4); return v; }
static inline int64_t rd_i64(const uint8_t *p) { int64_t v; memcpy(&v, p, 8); return v; }
static inline double  rd_f64(const uint8_t *p) { double v; memcpy(&v, p, 8); return v; }
static inline float   rd_f32(const uint8_t *p) { float v; memcpy(&v, p, 4); return v; }
static inline int16_t rd_i16(const uint8_t *p) { int16_t v; memcpy(&v, p, 2); return v; }

/* cursor over (p, len).  A read that would pass the end (or a negative size)
 * returns 0 / nullptr, leaves the cursor alone and clears `ok` for good, so a
 * parser checks `ok` once per section instead of once per field. */
struct BlobReader {
  const uint8_t *p;
  int64_t len, cur = 0;
  bool ok;
  BlobReader(const uint8_t *p_, int64_t len_)
      : p(p_), len(len_ < 0 ? 0 : len_), ok(p_ != nullptr) {}
  int64_t left() const { return len - cur; }
  const uint8_t *bytes(int64_t n) {
    if (!ok || n < 0 || n > left()) { ok = false; return nullptr; }
    const uint8_t *q = p + cur;
    cur += n;
    return q;
  }
  bool skip(int64_t n) { return bytes(n) != nullptr; }
  bool align8() { return skip(((cur + 7) & ~7ll) - cur); }
  int16_t i16() { const uint8_t *q = bytes(2); return q ? rd_i16(q) : 0; }
  int32_t i32() { const uint8_t *q = bytes(4); return q ? rd_i32(q) : 0; }
  int64_t i64() { const uint8_t *q = bytes(8); return q ? rd_i64(q) : 0; }
  /* n entries of w bytes each; n comes from the blob, so no n * w overflow */
  const uint8_t *array(int64_t n, int w) {
    if (n < 0 || n > left() / w) { ok = false; return nullptr; }
    return bytes(n * w);
  }
};

/* parsed column blob metadata (host view) */
struct ColMeta {
  int type_id = 0;               /* encoding */
  int64_t body_off = 0;          /* offset of fixed-width body / index array */
  int64_t null_off = 0;          /* offset of null words (0 if none) */
  int32_t num_null_words = 0;
  int32_t dict_n = 0;            /* dictionary entries (dict encodings) */
  std::vector<std::string> dict; /* string dictionary values */
  std::vector<int64_t> dict_i;   /* int dictionary values */
  std::vector<int32_t> local2global;  /* per-batch dict idx -> table-global id */
};

/* Raw Snappy block decompress (format_description.txt of google/snappy —
 * the raw block format snappy-java's Snappy.compress emits, which the
 * reference wraps as codec 2, CompressionCodecId.scala:31).  No libsnappy
 * is assumed, so the decoder is implemented here: varint32
 * uncompressed length, then literal (tag&3==0) and copy (1/2/4-byte
 * offset) elements; copies may overlap and run byte-by-byte. */
static int snappy_decompress(const uint8_t *src, int64_t slen,
                             std::vector<uint8_t> *out) {
  int64_t ip = 0;
  uint32_t ulen = 0;
  int shift = 0;
  while (ip < slen) {
    uint8_t b = src[ip++];
    ulen |= (uint32_t)(b & 0x7f) << shift;
    if (!(b & 0x80)) break;
    shift += 7;
    if (shift > 28) return -1;
  }
  out->resize(ulen);
  uint8_t *dst = out->data();
  uint32_t op = 0;
  while (ip < slen) {
    uint8_t tag = src[ip++];
    if ((tag & 3) == 0) {                        /* literal */
      uint32_t n = (uint32_t)(tag >> 2) + 1;
      if (n > 60) {
        int nb = (int)n - 60;
        if (ip + nb > slen) return -1;
        n = 0;
        for (int i = 0; i < nb; i++) n |= (uint32_t)src[ip + i] << (8 * i);
        n += 1;
        ip += nb;
      }
      if (ip + n > slen || (uint64_t)op + n > ulen) return -1;
      memcpy(dst + op, src + ip, n);
      ip += n; op += n;
    } else {                                     /* copy */
      uint32_t n, off;
      if ((tag & 3) == 1) {
        if (ip >= slen) return -1;
        n = ((uint32_t)(tag >> 2) & 7) + 4;
        off = ((uint32_t)(tag >> 5) << 8) | src[ip++];
      } else if ((tag & 3) == 2) {
        if (ip + 2 > slen) return -1;
        n = (uint32_t)(tag >> 2) + 1;
        off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8);
        ip += 2;
      } else {
        if (ip + 4 > slen) return -1;
        n = (uint32_t)(tag >> 2) + 1;
        off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8) |
              ((uint32_t)src[ip + 2] << 16) | ((uint32_t)src[ip + 3] << 24);
        ip += 4;
      }
      if (off == 0 || off > op || (uint64_t)op + n > ulen) return -1;
      for (uint32_t i = 0; i < n; i++) { dst[op] = dst[op - off]; op++; }
    }
  }
  return op == ulen ? 0 : -1;
}

/* the dictionary section [count][entries] of a column blob or a delta:
 * strings as [int32 size][bytes], INT32 / INT64 values fixed-width */
static int read_dictionary(BlobReader &r, sn_type_t dtype, int32_t *count,
                           std::vector<std::string> *strs,
                           std::vector<int64_t> *ints) {
  const int32_t n = *count = r.i32();
  if (!r.ok || n < 0) return SN_ERR_BADFORMAT;
  if (dtype == SN_TYPE_STRING) {
    if (n > r.left() / 4) return SN_ERR_BADFORMAT;     /* >= 4 bytes an entry */
    strs->reserve(n);
    for (int32_t i = 0; i < n; i++) {
      const int32_t sz = r.i32();
      const uint8_t *s = r.bytes(sz);
      if (!s) return SN_ERR_BADFORMAT;
      strs->emplace_back((const char *)s, (size_t)sz);
    }
    return SN_OK;
  }
  if (dtype != SN_TYPE_INT32 && dtype != SN_TYPE_INT64) return SN_ERR_UNSUPPORTED;
  const int w = dtype == SN_TYPE_INT64 ? 8 : 4;
  const uint8_t *v = r.array(n, w);
  if (!v) return SN_ERR_BADFORMAT;
  ints->reserve(n);
  for (int32_t i = 0; i < n; i++)
    ints->push_back(w == 8 ? rd_i64(v + (int64_t)i * 8) : rd_i32(v + (int64_t)i * 4));
  return SN_OK;
}

/* blob header parse: [typeId][nullBytes][null words], then for the dictionary
 * encodings [count][entries]; body_off is where the values / indices start */
static int parse_blob(const uint8_t *blob, int64_t len, sn_type_t dtype,
                      ColMeta *m) {
  BlobReader r(blob, len);
  m->type_id = r.i32();
  const int32_t null_bytes = r.i32();
  if (!r.ok || m->type_id < 0 || m->type_id > 4 || null_bytes < 0 ||
      (null_bytes & 7))
    return SN_ERR_BADFORMAT;
  if (null_bytes) {
    m->null_off = r.cur;
    m->num_null_words = null_bytes >> 3;
    if (!r.skip(null_bytes)) return SN_ERR_BADFORMAT;
  }
  if (m->type_id == SN_ENC_DICTIONARY || m->type_id == SN_ENC_BIG_DICTIONARY) {
    int rc = read_dictionary(r, dtype, &m->dict_n, &m->dict, &m->dict_i);
    if (rc != SN_OK) return rc;
  }
  m->body_off = r.cur;
  return SN_OK;
}

/* set bits of the blob's null words */
static int64_t count_nulls(const uint8_t *blob, const ColMeta &m) {
  int64_t n = 0;
  for (int32_t w = 0; w < m.num_null_words; w++)
    n += __builtin_popcountll(
        (unsigned long long)rd_i64(blob + m.null_off + (int64_t)w * 8));
  return n;
}

/* dictionary index i of an index array of 2-byte (unsigned) or 4-byte entries */
static inline int32_t dict_index(const uint8_t *body, int width, int64_t i) {
  return width == 2 ? (int32_t)(uint16_t)rd_i16(body + i * 2)
                    : rd_i32(body + i * 4);
}
static inline int dict_index_width(int type_id) {
  return type_id == SN_ENC_DICTIONARY ? 2 : 4;
}

/* a dictionary column carries exactly one index per NON-NULL row (padding
 * beyond is not data), each in [0, dict_n] — dict_n itself is the NULL
 * sentinel (DictionaryEncoding.scala:90).  *bad_at = ordinal of the first
 * index out of range, or -1 when the array is shorter than that. */
static int check_dict_indices(const uint8_t *blob, int64_t len,
                              const ColMeta &m, int32_t rows, int32_t dict_n,
                              int64_t *bad_at) {
  const int w = dict_index_width(m.type_id);
  const int64_t nidx = (int64_t)rows - count_nulls(blob, m);
  *bad_at = -1;
  BlobReader r(blob + m.body_off, len - m.body_off);
  const uint8_t *body = nidx > 0 ? r.array(nidx, w) : blob;
  if (!body) return SN_ERR_BADFORMAT;
  for (int64_t i = 0; i < nidx; i++) {
    const int32_t ix = dict_index(body, w, i);
    if (ix < 0 || ix > dict_n) { *bad_at = i; return SN_ERR_BADFORMAT; }
  }
  return SN_OK;
}

/* an UNCOMPRESSED body of `width`-byte values holds one per non-null row */
static int check_fixed_body(const uint8_t *blob, int64_t len, const ColMeta &m,
                            int32_t rows, int width) {
  const int64_t nn = (int64_t)rows - count_nulls(blob, m);
  return nn * width > len - m.body_off ? SN_ERR_BADFORMAT : SN_OK;
}

/* [typeId][nullBytes][null words] of a synthesized blob */
static void write_blob_header(std::vector<uint8_t> *out, int32_t type_id,
                              const void *nullw, int32_t null_bytes) {
  const uint8_t *t = (const uint8_t *)&type_id, *n = (const uint8_t *)&null_bytes;
  out->insert(out->end(), t, t + 4);
  out->insert(out->end(), n, n + 4);
  if (null_bytes)
    out->insert(out->end(), (const uint8_t *)nullw,
                (const uint8_t *)nullw + null_bytes);
}
static inline void write_i32(std::vector<uint8_t> *out, int32_t v) {
  const uint8_t *p = (const uint8_t *)&v;
  out->insert(out->end(), p, p + 4);
}

/* Var-width (non-dictionary) STRING bodies ([int32 size][bytes] per non-null
 * row, in row order) have no random-access layout a data-parallel kernel can
 * consume: re-encode as BIG_DICTIONARY, entries in first-occurrence order,
 * null words kept, so the dictionary machinery applies wholesale. */
static int transcode_strings(const uint8_t *blob, int64_t len, const ColMeta &m,
                             int32_t rows, std::vector<uint8_t> *out) {
  std::map<std::string, int32_t> didx;
  std::vector<const std::string *> dict;
  std::vector<int32_t> idx;
  const int64_t nn_rows = (int64_t)rows - count_nulls(blob, m);
  BlobReader r(blob, len);
  r.skip(m.body_off);
  if (nn_rows > r.left() / 4) return SN_ERR_BADFORMAT;
  idx.reserve(nn_rows > 0 ? (size_t)nn_rows : 0);
  int64_t dict_bytes = 0;
  for (int64_t i = 0; i < nn_rows; i++) {
    const int32_t sz = r.i32();
    const uint8_t *s = r.bytes(sz);
    if (!s) return SN_ERR_BADFORMAT;
    auto ins = didx.emplace(std::string((const char *)s, (size_t)sz),
                            (int32_t)dict.size());
    if (ins.second) { dict.push_back(&ins.first->first); dict_bytes += 4 + sz; }
    idx.push_back(ins.first->second);
  }
  const int32_t nb = m.num_null_words * 8;
  out->clear();
  out->reserve((size_t)(8 + nb + 4 + dict_bytes) + idx.size() * 4);
  write_blob_header(out, SN_ENC_BIG_DICTIONARY, blob + m.null_off, nb);
  write_i32(out, (int32_t)dict.size());
  for (const std::string *s : dict) {
    write_i32(out, (int32_t)s->size());
    out->insert(out->end(), s->begin(), s->end());
  }
  const uint8_t *ip = (const uint8_t *)idx.data();
  out->insert(out->end(), ip, ip + idx.size() * 4);
  return SN_OK;
}

/* Int-typed dictionary columns (DictionaryEncoding over int32/int64): write
 * the values out as a plain UNCOMPRESSED body so the scan runs the fixed-width
 * path.  Rows whose index is the NULL sentinel (== dict_n) are folded into the
 * synthesized null words.  *bad_at as in check_dict_indices. */
static int materialize_int_dict(const uint8_t *blob, int64_t len,
                                const ColMeta &m, sn_type_t dtype, int32_t rows,
                                std::vector<uint8_t> *out, int64_t *bad_at) {
  const int w = dict_index_width(m.type_id);
  const int vw = dtype == SN_TYPE_INT64 ? 8 : 4;
  const int32_t nwords = (rows + 63) >> 6;
  std::vector<uint64_t> nullw(nwords, 0);
  for (int32_t wi = 0; wi < m.num_null_words && wi < nwords; wi++)
    nullw[wi] = (uint64_t)rd_i64(blob + m.null_off + (int64_t)wi * 8);
  BlobReader r(blob, len);
  r.skip(m.body_off);
  std::vector<uint8_t> vals;
  vals.reserve((size_t)std::min<int64_t>(rows, r.left() / w) * vw);
  *bad_at = -1;
  int64_t ii = 0;                       /* index ordinal (one per non-null row) */
  for (int32_t row = 0; row < rows; row++) {
    if ((nullw[row >> 6] >> (row & 63)) & 1) continue;
    const int32_t ix = w == 2 ? (int32_t)(uint16_t)r.i16() : r.i32();
    if (!r.ok) return SN_ERR_BADFORMAT;
    if (ix < 0 || ix > m.dict_n) { *bad_at = ii; return SN_ERR_BADFORMAT; }
    ii++;
    if (ix == m.dict_n) { nullw[row >> 6] |= 1ull << (row & 63); continue; }
    const int64_t v = m.dict_i[ix];
    const int32_t v32 = (int32_t)v;
    const uint8_t *vp = vw == 8 ? (const uint8_t *)&v : (const uint8_t *)&v32;
    vals.insert(vals.end(), vp, vp + vw);
  }
  bool any_null = false;
  for (uint64_t wv : nullw) any_null |= wv != 0;
  out->clear();
  out->reserve(8 + (size_t)nwords * 8 + vals.size());
  write_blob_header(out, SN_ENC_UNCOMPRESSED, nullw.data(),
                    any_null ? nwords * 8 : 0);
  out->insert(out->end(), vals.begin(), vals.end());
  return SN_OK;
}

/* RLE body = [value][int32 run length] entries of `width`-byte values: one
 * (cumulative end, value) pair per run.  INT64 values keep their raw bits in
 * the double (i64_bits); narrower ones are widened numerically.  A trailing
 * partial entry is not data. */
static void extract_rle_runs(const uint8_t *blob, int64_t len, const ColMeta &m,
                             int width, bool i64_bits,
                             std::vector<int32_t> *ends,
                             std::vector<double> *vals) {
  BlobReader r(blob, len);
  r.skip(m.body_off);
  int32_t acc = 0;
  while (r.ok && r.left() >= width + 4) {
    const int64_t v = width == 2 ? r.i16() : width == 4 ? r.i32() : r.i64();
    acc = (int32_t)((uint32_t)acc + (uint32_t)r.i32());   /* wraps, no UB */
    ends->push_back(acc);
    double d = (double)v;
    if (i64_bits) memcpy(&d, &v, 8);
    vals->push_back(d);
  }
}

/* delete mask [int32 0][int32 numBaseRows][int32 n][n int32 positions] */
static int parse_delete_mask(const uint8_t *blob, int64_t len,
                             const uint8_t **pos, int32_t *n) {
  BlobReader r(blob, len);
  r.skip(8);
  *n = r.i32();
  *pos = r.array(*n, 4);
  return *pos ? SN_OK : SN_ERR_BADFORMAT;
}

/* one decoded update delta: entry i rewrites row pos[i].  Numeric columns
 * carry the value in val[i] (INT64: the RAW BITS, exact beyond 2^53, which
 * every consumer bitcasts back); string columns carry sidx[i], an index into
 * strs — the caller interns.  A null entry has isnull[i] = 1, val 0, sidx -1. */
struct DeltaRows {
  std::vector<int32_t> pos;
  std::vector<uint8_t> isnull;
  std::vector<double> val;
  std::vector<int32_t> sidx;
  std::vector<std::string> strs;
};

/* one UNCOMPRESSED fixed-width delta value at the cursor */
static int read_delta_value(BlobReader &r, sn_type_t dtype, double *v) {
  switch (dtype) {
    case SN_TYPE_DOUBLE: case SN_TYPE_INT64: {
      const int64_t b = r.i64(); memcpy(v, &b, 8); break; }
    case SN_TYPE_FLOAT: {
      const int32_t b = r.i32(); float f; memcpy(&f, &b, 4); *v = f; break; }
    case SN_TYPE_INT32: *v = (double)r.i32(); break;
    case SN_TYPE_INT16: *v = (double)r.i16(); break;
    default: return SN_ERR_UNSUPPORTED;
  }
  return r.ok ? SN_OK : SN_ERR_BADFORMAT;
}

/* delta blob = header with the null words over delta ENTRIES, [numBaseRows]
 * [numPositions][positions][pad to 8], then an UNCOMPRESSED or dictionary
 * body holding one value per non-null entry (deltas are bounded by
 * ColumnMaxDeltaRows, so this is O(10^4) host work per column). */
static int decode_delta(const uint8_t *blob, int64_t len, sn_type_t dtype,
                        DeltaRows *out) {
  BlobReader r(blob, len);
  const int type_id = r.i32();
  const int32_t null_bytes = r.i32();
  if (!r.ok || null_bytes < 0 || (null_bytes & 7)) return SN_ERR_BADFORMAT;
  const uint8_t *nullw = null_bytes ? r.bytes(null_bytes) : nullptr;
  r.skip(4);                                   /* numBaseRows */
  const int32_t npos = r.i32();
  const uint8_t *posp = r.array(npos, 4);
  r.align8();
  if (!r.ok || (nullw && npos > (int64_t)null_bytes * 8))
    return SN_ERR_BADFORMAT;
  const bool is_str = dtype == SN_TYPE_STRING;
  const bool dict_enc =
      type_id == SN_ENC_DICTIONARY || type_id == SN_ENC_BIG_DICTIONARY;
  int32_t dict_n = 0;
  std::vector<int64_t> dict_i;
  if (dict_enc) {
    int rc = read_dictionary(r, dtype, &dict_n, &out->strs, &dict_i);
    if (rc != SN_OK) return rc;
  } else if (type_id != SN_ENC_UNCOMPRESSED) {
    return SN_ERR_UNSUPPORTED;  /* RLE deltas not produced by this build */
  }
  const int iw = dict_index_width(type_id);
  for (int32_t i = 0; i < npos; i++) {
    bool nul = nullw && ((rd_i64(nullw + ((i >> 6) << 3)) >> (i & 63)) & 1);
    double v = 0.0;
    int32_t si = -1;
    if (nul) {
      /* no body bytes */
    } else if (dict_enc) {
      const int32_t idx = iw == 2 ? (int32_t)(uint16_t)r.i16() : r.i32();
      if (!r.ok || idx < 0 || idx > dict_n || (idx == dict_n && !is_str))
        return SN_ERR_BADFORMAT;
      if (idx == dict_n) nul = true;           /* the NULL sentinel */
      else if (is_str) si = idx;
      else if (dtype == SN_TYPE_INT64) memcpy(&v, &dict_i[idx], 8);
      else v = (double)dict_i[idx];
    } else if (is_str) {
      const int32_t sz = r.i32();
      const uint8_t *s = r.bytes(sz);
      if (!s) return SN_ERR_BADFORMAT;
      si = (int32_t)out->strs.size();
      out->strs.emplace_back((const char *)s, (size_t)sz);
    } else {
      int rc = read_delta_value(r, dtype, &v);
      if (rc != SN_OK) return rc;
    }
    out->pos.push_back(rd_i32(posp + (int64_t)i * 4));
    out->isnull.push_back(nul ? 1 : 0);
    out->val.push_back(v);
    out->sidx.push_back(si);
  }
  return SN_OK;
}

#endif
