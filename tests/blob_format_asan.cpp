/*
 * blob_format_asan.cpp — csrc/blob_format.h under AddressSanitizer and
 * UBSan, stand-alone: no engine, no HIP, no GPU.
 *
 * Builds one small valid blob of every kind the put path accepts, with its
 * own little-endian writers, and for each blob
 *   - decodes it untouched and compares with the values it was built from;
 *   - copies every proper prefix into a heap buffer of exactly that size
 *     (so one byte too far is a heap overflow the sanitizer reports) and
 *     decodes: each must be rejected, every blob here being minimal;
 *   - overwrites each 4-byte field of the header, positions and dictionary
 *     sections with -1, 0x7fffffff and the blob length in turn and decodes:
 *     accepted or rejected, the sanitizers must stay silent.
 * Prints per decoder how many inputs it saw, accepted and rejected.
 */
#include "../snappydata_amd/csrc/blob_format.h"

#include <cstdio>
#include <cstdlib>
#include <functional>

/* ---- writers: f32() also records the field's offset for the overwrite pass */
struct W {
  std::vector<uint8_t> v;
  std::vector<size_t> fields;
  void raw(const void *p, size_t n) {
    v.insert(v.end(), (const uint8_t *)p, (const uint8_t *)p + n);
  }
  void i16(int16_t x) { raw(&x, 2); }
  void i32(int32_t x) { raw(&x, 4); }
  void i64(int64_t x) { raw(&x, 8); }
  void f64(double x) { raw(&x, 8); }
  void f32(int32_t x) { fields.push_back(v.size()); i32(x); }
  void str(const std::string &s) { f32((int32_t)s.size()); raw(s.data(), s.size()); }
  void pad8() { while (v.size() & 7) v.push_back(0); }
};

/* a value of any column type: kind 'n'ull, 'i'nteger, 'd'ouble or 's'tring */
struct Val {
  char kind = 'n';
  bool null = true;
  int64_t i = 0;
  double d = 0;
  std::string s;
};
static Val N() { return Val(); }
static Val I(int64_t x) { Val v; v.kind = 'i'; v.null = false; v.i = x; return v; }
static Val D(double x) { Val v; v.kind = 'd'; v.null = false; v.d = x; return v; }
static Val S(const std::string &x) { Val v; v.kind = 's'; v.null = false; v.s = x; return v; }

static std::string dump(const std::vector<Val> &vals) {
  std::string o;
  char buf[64];
  for (const Val &v : vals) {
    if (v.kind == 'n') o += "N,";
    else if (v.kind == 's') o += "'" + v.s + "',";
    else if (v.kind == 'd') { snprintf(buf, sizeof buf, "%a,", v.d); o += buf; }
    else { snprintf(buf, sizeof buf, "%lld,", (long long)v.i); o += buf; }
  }
  return o;
}

static void put_header(W &w, int32_t type_id, const std::vector<Val> &vals,
                       bool bitset_nulls) {
  w.f32(type_id);
  bool any = false;
  for (const Val &v : vals) any |= v.null;
  if (!any || !bitset_nulls) { w.f32(0); return; }
  std::vector<uint64_t> words((vals.size() + 63) / 64, 0);
  for (size_t i = 0; i < vals.size(); i++)
    if (vals[i].null) words[i >> 6] |= 1ull << (i & 63);
  w.f32((int32_t)words.size() * 8);
  w.raw(words.data(), words.size() * 8);
}

static void put_fixed(W &w, sn_type_t dt, const Val &v) {
  switch (dt) {
    case SN_TYPE_INT16: w.i16((int16_t)v.i); break;
    case SN_TYPE_INT32: w.i32((int32_t)v.i); break;
    case SN_TYPE_INT64: w.i64(v.i); break;
    case SN_TYPE_DOUBLE: w.f64(v.d); break;
    default: w.v.push_back((uint8_t)v.i);
  }
}

/* the encoding body after the header; nulls in the bitset write nothing,
 * sentinel nulls (dictionary encodings, !bitset_nulls) write index == size */
static void put_body(W &w, int32_t enc, sn_type_t dt, const std::vector<Val> &vals,
                     bool bitset_nulls) {
  if (enc == SN_ENC_UNCOMPRESSED) {
    for (const Val &v : vals) {
      if (v.null) continue;
      if (dt == SN_TYPE_STRING) { w.i32((int32_t)v.s.size()); w.raw(v.s.data(), v.s.size()); }
      else put_fixed(w, dt, v);
    }
  } else if (enc == SN_ENC_RUNLENGTH) {
    std::vector<Val> nn;
    for (const Val &v : vals) if (!v.null) nn.push_back(v);
    for (size_t i = 0; i < nn.size();) {
      size_t j = i;
      while (j < nn.size() && nn[j].i == nn[i].i) j++;
      put_fixed(w, dt, nn[i]);
      w.i32((int32_t)(j - i));
      i = j;
    }
  } else if (enc == SN_ENC_BOOLEAN_BITSET) {
    std::vector<uint64_t> bits;
    size_t k = 0;
    for (const Val &v : vals) {
      if (v.null) continue;
      if ((k >> 6) >= bits.size()) bits.push_back(0);
      if (v.i) bits[k >> 6] |= 1ull << (k & 63);
      k++;
    }
    w.raw(bits.data(), bits.size() * 8);
  } else {                                    /* DICTIONARY / BIG_DICTIONARY */
    std::vector<const Val *> dict;
    std::vector<int32_t> idx;
    for (const Val &v : vals) {
      if (v.null) { if (!bitset_nulls) idx.push_back(-1); continue; }
      size_t j = 0;
      for (; j < dict.size(); j++)
        if (dict[j]->s == v.s && dict[j]->i == v.i) break;
      if (j == dict.size()) dict.push_back(&v);
      idx.push_back((int32_t)j);
    }
    w.f32((int32_t)dict.size());
    for (const Val *d : dict) {
      if (dt == SN_TYPE_STRING) w.str(d->s);
      else if (dt == SN_TYPE_INT32) w.f32((int32_t)d->i);
      else w.i64(d->i);
    }
    for (int32_t ix : idx) {
      if (ix < 0) ix = (int32_t)dict.size();
      if (enc == SN_ENC_DICTIONARY) w.i16((int16_t)ix); else w.i32(ix);
    }
  }
}

/* ---- decoders: blob -> values, through blob_format.h alone ---- */

static bool null_bit(const uint8_t *blob, const ColMeta &m, int64_t row) {
  if ((row >> 6) >= m.num_null_words) return false;
  return (rd_i64(blob + m.null_off + (row >> 6) * 8) >> (row & 63)) & 1;
}

static Val fixed_at(const uint8_t *body, sn_type_t dt, int64_t k) {
  switch (dt) {
    case SN_TYPE_INT16: return I(rd_i16(body + k * 2));
    case SN_TYPE_INT32: return I(rd_i32(body + k * 4));
    case SN_TYPE_INT64: return I(rd_i64(body + k * 8));
    case SN_TYPE_DOUBLE: return D(rd_f64(body + k * 8));
    default: return I(body[k]);
  }
}
static int width_of(sn_type_t dt) {
  return dt == SN_TYPE_INT16 ? 2 : dt == SN_TYPE_INT32 ? 4 :
         dt == SN_TYPE_INT64 || dt == SN_TYPE_DOUBLE ? 8 : 1;
}

static int decode_column(const uint8_t *blob, int64_t len, sn_type_t dt,
                         int32_t rows, std::vector<Val> *out) {
  ColMeta m;
  int rc = parse_blob(blob, len, dt, &m);
  if (rc != SN_OK) return rc;
  std::vector<uint8_t> synth;
  int64_t bad;
  const bool dict_enc = m.type_id == SN_ENC_DICTIONARY ||
                        m.type_id == SN_ENC_BIG_DICTIONARY;
  if (dt == SN_TYPE_STRING && m.type_id == SN_ENC_UNCOMPRESSED)
    rc = transcode_strings(blob, len, m, rows, &synth);
  else if (dict_enc && dt != SN_TYPE_STRING)
    rc = materialize_int_dict(blob, len, m, dt, rows, &synth, &bad);
  if (rc != SN_OK) return rc;
  if (!synth.empty()) {
    /* the re-encoded blob is decoded from an exact-size copy too */
    uint8_t *copy = (uint8_t *)malloc(synth.size());
    memcpy(copy, synth.data(), synth.size());
    rc = decode_column(copy, (int64_t)synth.size(), dt, rows, out);
    free(copy);
    return rc;
  }
  const uint8_t *body = blob + m.body_off;
  const int64_t nn = (int64_t)rows - count_nulls(blob, m);
  std::vector<int32_t> ends;
  std::vector<double> runs;
  if (m.type_id == SN_ENC_UNCOMPRESSED) {
    rc = check_fixed_body(blob, len, m, rows, width_of(dt));
  } else if (dict_enc) {
    rc = check_dict_indices(blob, len, m, rows, (int32_t)m.dict.size(), &bad);
  } else if (m.type_id == SN_ENC_RUNLENGTH) {
    extract_rle_runs(blob, len, m, width_of(dt), dt == SN_TYPE_INT64, &ends, &runs);
    /* the runs must cover the non-null rows, in increasing order */
    for (size_t i = 0; i < ends.size(); i++)
      if (ends[i] <= (i ? ends[i - 1] : 0)) rc = SN_ERR_BADFORMAT;
    if (nn > 0 && (ends.empty() || ends.back() < nn)) rc = SN_ERR_BADFORMAT;
  } else if (((nn + 63) >> 6) * 8 > len - m.body_off) {  /* BOOLEAN_BITSET */
    rc = SN_ERR_BADFORMAT;
  }
  if (rc != SN_OK) return rc;
  int64_t k = 0;
  size_t run = 0;
  for (int32_t r = 0; r < rows; r++) {
    if (null_bit(blob, m, r)) { out->push_back(N()); continue; }
    if (m.type_id == SN_ENC_UNCOMPRESSED) {
      out->push_back(fixed_at(body, dt, k));
    } else if (dict_enc) {
      int32_t ix = dict_index(body, dict_index_width(m.type_id), k);
      out->push_back(ix == (int32_t)m.dict.size() ? N() : S(m.dict[ix]));
    } else if (m.type_id == SN_ENC_RUNLENGTH) {
      while (ends[run] <= k) run++;
      int64_t bits;
      memcpy(&bits, &runs[run], 8);
      out->push_back(I(dt == SN_TYPE_INT64 ? bits : (int64_t)runs[run]));
    } else {
      out->push_back(I((rd_i64(body + (k >> 6) * 8) >> (k & 63)) & 1));
    }
    k++;
  }
  return SN_OK;
}

static int decode_mask(const uint8_t *blob, int64_t len, std::vector<Val> *out) {
  const uint8_t *pos;
  int32_t n;
  int rc = parse_delete_mask(blob, len, &pos, &n);
  for (int32_t i = 0; rc == SN_OK && i < n; i++)
    out->push_back(I(rd_i32(pos + (int64_t)i * 4)));
  return rc;
}

/* values interleaved as (position, value) pairs */
static int decode_delta_vals(const uint8_t *blob, int64_t len, sn_type_t dt,
                             std::vector<Val> *out) {
  DeltaRows d;
  int rc = decode_delta(blob, len, dt, &d);
  if (rc != SN_OK) return rc;
  for (size_t i = 0; i < d.pos.size(); i++) {
    int64_t bits;
    memcpy(&bits, &d.val[i], 8);
    out->push_back(I(d.pos[i]));
    if (d.isnull[i]) out->push_back(N());
    else if (dt == SN_TYPE_STRING) out->push_back(S(d.strs.at((size_t)d.sidx[i])));
    else if (dt == SN_TYPE_DOUBLE) out->push_back(D(d.val[i]));
    else out->push_back(I(dt == SN_TYPE_INT64 ? bits : (int64_t)d.val[i]));
  }
  return SN_OK;
}

/* the codec wrapper [int32 -2][int32 length][Snappy stream], as the engine's
 * unwrap stage reads it */
static int decode_snappy(const uint8_t *blob, int64_t len, std::vector<Val> *out) {
  BlobReader r(blob, len);
  const int32_t tag = r.i32(), ulen = r.i32();
  if (!r.ok || tag != -2 || ulen <= 0) return SN_ERR_BADFORMAT;
  std::vector<uint8_t> plain;
  if (snappy_decompress(blob + r.cur, r.left(), &plain) != 0 ||
      (int64_t)plain.size() != ulen)
    return SN_ERR_BADFORMAT;
  out->push_back(S(std::string(plain.begin(), plain.end())));
  return SN_OK;
}

/* ---- the cases ---- */

typedef std::function<int(const uint8_t *, int64_t, std::vector<Val> *)> Decoder;
struct Case {
  std::string name, decoder;
  W w;
  std::string expect;
  Decoder run;
};

static Case column_case(const char *name, int32_t enc, sn_type_t dt,
                        const std::vector<Val> &vals, bool bitset_nulls = true) {
  Case c;
  c.name = name;
  c.decoder = "column";
  put_header(c.w, enc, vals, bitset_nulls);
  put_body(c.w, enc, dt, vals, bitset_nulls);
  c.expect = dump(vals);
  const int32_t rows = (int32_t)vals.size();
  c.run = [dt, rows](const uint8_t *p, int64_t n, std::vector<Val> *o) {
    return decode_column(p, n, dt, rows, o);
  };
  return c;
}

static Case delta_case(const char *name, int32_t enc, sn_type_t dt,
                       const std::vector<int32_t> &pos,
                       const std::vector<Val> &vals, bool bitset_nulls = true) {
  Case c;
  c.name = name;
  c.decoder = "delta";
  put_header(c.w, enc, vals, bitset_nulls);
  c.w.f32(1000);
  c.w.f32((int32_t)pos.size());
  for (int32_t p : pos) c.w.f32(p);
  c.w.pad8();
  put_body(c.w, enc, dt, vals, bitset_nulls);
  std::vector<Val> ex;
  for (size_t i = 0; i < vals.size(); i++) {
    ex.push_back(I(pos[i]));
    ex.push_back(vals[i]);
  }
  c.expect = dump(ex);
  c.run = [dt](const uint8_t *p, int64_t n, std::vector<Val> *o) {
    return decode_delta_vals(p, n, dt, o);
  };
  return c;
}

static std::vector<Case> build_cases() {
  std::vector<Case> cs;
  std::vector<Val> ints, dbls, strs, runs, bools;
  for (int i = 0; i < 70; i++) {          /* 70 rows: two null words */
    const bool nul = i % 9 == 4 || i == 69;
    ints.push_back(nul ? N() : I((i % 5) * 1000 - 7));
    dbls.push_back(nul ? N() : D(i / 8.0 - 3));
    static const char *pool[] = { "bb", "a", "", "ccc" };
    strs.push_back(nul ? N() : S(pool[i % 4]));
    runs.push_back(nul ? N() : I(i / 20 - 1));
    bools.push_back(nul ? N() : I(i % 3 == 0));
  }
  const std::vector<Val> big = { I(5), I((1ll << 40) + 6), N(), I(-7), I(9) };
  cs.push_back(column_case("plain_i16", SN_ENC_UNCOMPRESSED, SN_TYPE_INT16, runs));
  cs.push_back(column_case("plain_i32", SN_ENC_UNCOMPRESSED, SN_TYPE_INT32, ints));
  cs.push_back(column_case("plain_i64", SN_ENC_UNCOMPRESSED, SN_TYPE_INT64, big));
  cs.push_back(column_case("plain_f64", SN_ENC_UNCOMPRESSED, SN_TYPE_DOUBLE, dbls));
  cs.push_back(column_case("plain_f64_nonull", SN_ENC_UNCOMPRESSED, SN_TYPE_DOUBLE,
                           { D(1.5), D(-2.25), D(0) }));
  cs.push_back(column_case("plain_string", SN_ENC_UNCOMPRESSED, SN_TYPE_STRING, strs));
  cs.push_back(column_case("rle_i16", SN_ENC_RUNLENGTH, SN_TYPE_INT16, runs));
  cs.push_back(column_case("rle_i32", SN_ENC_RUNLENGTH, SN_TYPE_INT32, runs));
  cs.push_back(column_case("rle_i64", SN_ENC_RUNLENGTH, SN_TYPE_INT64,
                           { I(1ll << 60), I(1ll << 60), N(), I(-3) }));
  cs.push_back(column_case("dict_string", SN_ENC_DICTIONARY, SN_TYPE_STRING, strs));
  cs.push_back(column_case("bigdict_string", SN_ENC_BIG_DICTIONARY, SN_TYPE_STRING, strs));
  cs.push_back(column_case("dict_string_sentinel", SN_ENC_DICTIONARY, SN_TYPE_STRING,
                           strs, false));
  cs.push_back(column_case("dict_i32", SN_ENC_DICTIONARY, SN_TYPE_INT32, ints));
  cs.push_back(column_case("bigdict_i32_sentinel", SN_ENC_BIG_DICTIONARY,
                           SN_TYPE_INT32, ints, false));
  cs.push_back(column_case("dict_i64", SN_ENC_DICTIONARY, SN_TYPE_INT64, big));
  cs.push_back(column_case("bigdict_i64", SN_ENC_BIG_DICTIONARY, SN_TYPE_INT64, big));
  cs.push_back(column_case("boolbitset", SN_ENC_BOOLEAN_BITSET, SN_TYPE_BOOL, bools));

  Case mask;
  mask.name = "delete_mask";
  mask.decoder = "delete_mask";
  mask.w.f32(0); mask.w.f32(1000); mask.w.f32(3);
  for (int32_t p : { 2, 40, 999 }) mask.w.f32(p);
  mask.expect = dump({ I(2), I(40), I(999) });
  mask.run = decode_mask;
  cs.push_back(mask);

  cs.push_back(delta_case("delta_plain_f64", SN_ENC_UNCOMPRESSED, SN_TYPE_DOUBLE,
                          { 1, 5, 9 }, { D(1.5), N(), D(-3) }));
  cs.push_back(delta_case("delta_plain_i64", SN_ENC_UNCOMPRESSED, SN_TYPE_INT64,
                          { 0, 7 }, { I((1ll << 55) + 1), I(-2) }));
  cs.push_back(delta_case("delta_plain_i16", SN_ENC_UNCOMPRESSED, SN_TYPE_INT16,
                          { 3 }, { I(-300) }));
  cs.push_back(delta_case("delta_plain_string", SN_ENC_UNCOMPRESSED, SN_TYPE_STRING,
                          { 1, 2, 3 }, { S("x"), N(), S("yz") }));
  cs.push_back(delta_case("delta_dict_string", SN_ENC_DICTIONARY, SN_TYPE_STRING,
                          { 1, 2, 3, 8 }, { S("x"), N(), S("yz"), S("x") }));
  cs.push_back(delta_case("delta_bigdict_string_sentinel", SN_ENC_BIG_DICTIONARY,
                          SN_TYPE_STRING, { 1, 2, 3 }, { S("x"), N(), S("yz") },
                          false));
  cs.push_back(delta_case("delta_dict_i32", SN_ENC_DICTIONARY, SN_TYPE_INT32,
                          { 4, 6, 7 }, { I(70), I(80), I(70) }));
  cs.push_back(delta_case("delta_bigdict_i64", SN_ENC_BIG_DICTIONARY, SN_TYPE_INT64,
                          { 4, 6 }, { I((1ll << 54) + 1), N() }));

  /* "abcabcabcabc!" + 70 x 'z': a literal, an overlapping 1-byte-offset copy,
   * a literal, a long literal with a length byte */
  Case sn;
  sn.name = "snappy";
  sn.decoder = "snappy";
  std::string plain = "abcabcabcabc!" + std::string(70, 'z');
  sn.w.f32(-2);
  sn.w.f32((int32_t)plain.size());
  sn.w.v.push_back((uint8_t)plain.size());                 /* varint 83 */
  sn.w.v.push_back((3 - 1) << 2); sn.w.raw("abc", 3);      /* literal 3 */
  sn.w.v.push_back(1 | ((9 - 4) << 2)); sn.w.v.push_back(3);  /* copy 9 off 3 */
  sn.w.v.push_back((1 - 1) << 2); sn.w.raw("!", 1);
  sn.w.v.push_back(60 << 2); sn.w.v.push_back(70 - 1);     /* literal, 1 length byte */
  sn.w.raw(std::string(70, 'z').data(), 70);
  sn.expect = dump({ S(plain) });
  sn.run = decode_snappy;
  cs.push_back(sn);
  return cs;
}

struct Tally { long seen = 0, accepted = 0, rejected = 0; };

/* decode an exact-size heap copy of (p, n) */
static int run_copy(const Case &c, const uint8_t *p, size_t n, Tally *t,
                    std::string *got) {
  uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(copy, p, n);
  std::vector<Val> out;
  /* a zero-length buffer is still a real pointer with nothing behind it */
  int rc = c.run(n ? copy : copy + 1, (int64_t)n, &out);
  free(copy);
  t->seen++;
  (rc == SN_OK ? t->accepted : t->rejected)++;
  if (got) *got = dump(out);
  return rc;
}

int main() {
  std::map<std::string, Tally> tally;
  int failures = 0;
  for (const Case &c : build_cases()) {
    Tally &t = tally[c.decoder];
    const std::vector<uint8_t> &v = c.w.v;
    std::string got;
    if (run_copy(c, v.data(), v.size(), &t, &got) != SN_OK || got != c.expect) {
      printf("FAIL %s: untouched blob decoded to [%s], built from [%s]\n",
             c.name.c_str(), got.c_str(), c.expect.c_str());
      failures++;
    }
    for (size_t n = 0; n < v.size(); n++)
      if (run_copy(c, v.data(), n, &t, nullptr) == SN_OK) {
        printf("FAIL %s: prefix %zu of %zu accepted\n", c.name.c_str(), n, v.size());
        failures++;
      }
    for (size_t off : c.w.fields)
      for (int32_t x : { -1, 0x7fffffff, (int32_t)v.size() }) {
        std::vector<uint8_t> m = v;
        memcpy(m.data() + off, &x, 4);
        run_copy(c, m.data(), m.size(), &t, nullptr);
      }
  }
  for (auto &kv : tally)
    printf("decoder %s seen %ld accepted %ld rejected %ld\n", kv.first.c_str(),
           kv.second.seen, kv.second.accepted, kv.second.rejected);
  printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
