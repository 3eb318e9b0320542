/*
 * jit_shapes.cpp — stand-alone host program that pins the query-compiled
 * kernel SOURCE (csrc/jit.cpp) over a fixed table of plan shapes.
 *
 * The generator is a pure host function, so "this jit.cpp emits the same
 * kernel text as another jit.cpp" is checkable without a GPU: build this
 * program against each and compare the per-shape hash lines.  Every source
 * is split at the first `extern "C" __global__`; the kernel part is hashed
 * (FNV-1a 64) and the prelude (typedefs, layout mirror, helpers — identical
 * for every shape) is printed once.
 *
 *   jit_shapes              one "<shape> <hash>" line per shape, then the prelude
 *   jit_shapes --compile    also compile every shape with hipRTC for gfx950;
 *                           exit 1 if any compile fails
 *   jit_shapes --dump NAME  print the full generated source of one shape
 *
 * The generator reads its SN_JIT_* environment once per process, so a shape
 * that names a variable runs in a child process of this same program
 * (--one NAME) with that variable set.
 */
#include "../snappydata_amd/csrc/jit.cpp"

#include <unistd.h>

namespace {

struct Shape {
  const char *name;
  sn_dev_plan p;
  int kinds[SN_DEV_MAX_COLS];
  int nslots, na_t, has_del;
  const char *env_name, *env_val;   /* NULL: default environment */
};

/* non-NULL markers: only the NULLness of a plan pointer shapes the source */
const int64_t *const PTR_KEYS = (const int64_t *)16;
const int32_t *const PTR_PAY = (const int32_t *)16;
const int32_t *const PTR_LUT = (const int32_t *)16;
const uint64_t *const PTR_BM = (const uint64_t *)16;

Shape blank(const char *name, int nslots, int na_t) {
  Shape s;
  memset(&s, 0, sizeof(s));
  s.name = name;
  s.nslots = nslots;
  s.na_t = na_t;
  s.p.nslots = nslots;
  return s;
}

void cols(Shape &s, std::initializer_list<int> kinds) {
  int c = 0;
  for (int k : kinds) {
    s.kinds[c] = k;
    if (k == SN_K_I64) s.p.i64_mask |= 1u << c;
    c++;
  }
  s.p.nused = c;
}

/* aggregate over up to three trivial (a=0, m=1) factors; op 0 sum, 1 min,
 * 2 max.  Unused factors carry the engine's (a=1, m=0, c=c0) filler. */
void agg(Shape &s, int op, std::initializer_list<int> factors) {
  sn_dev_agg &A = s.p.aggs[s.p.naggs++];
  int c[3] = { 0, 0, 0 }, n = 0;
  for (int f : factors) c[n++] = f;
  A.nf = n;
  A.op = op;
  A.c0 = c[0];
  A.c1 = n >= 2 ? c[1] : c[0];
  A.c2 = n >= 3 ? c[2] : c[0];
  A.a0 = n >= 1 ? 0.0 : 1.0; A.m0 = n >= 1 ? 1.0 : 0.0;
  A.a1 = n >= 2 ? 0.0 : 1.0; A.m1 = n >= 2 ? 1.0 : 0.0;
  A.a2 = n >= 3 ? 0.0 : 1.0; A.m2 = n >= 3 ? 1.0 : 0.0;
}

void pred_d(Shape &s, int cslot, double lo, double hi) {
  sn_dev_pred_d &P = s.p.preds_d[s.p.npreds_d++];
  P.lo = lo; P.hi = hi; P.cslot = cslot;
}

void pred_i(Shape &s, int cslot, int64_t lo, int64_t hi) {
  sn_dev_pred_i &P = s.p.preds_i[s.p.npreds_i++];
  P.lo = lo; P.hi = hi; P.cslot = cslot;
}

void inlist(Shape &s, int cslot) {
  auto &I = s.p.inp[s.p.npreds_in++];
  I.bm = PTR_BM; I.base = 3; I.nwords = 2; I.n = 5; I.cslot = cslot;
}

/* dense group keys (dictionary keys arrive premultiplied: base 0) */
void group(Shape &s, std::initializer_list<int> gcols, int gmul0) {
  int n = 0;
  for (int g : gcols) s.p.gcol[n++] = g;
  s.p.ngroup = n;
  s.p.gmul0 = gmul0;
}

/* broadcast-dimension join on column jcslot; lut_max < 0: hash chain only */
void join(Shape &s, int jcslot, int jmode, long long lut_min,
          long long lut_max) {
  s.p.jkeys = PTR_KEYS;
  s.p.jpayload = PTR_PAY;
  s.p.jcap_log2 = 12;
  s.p.jcslot = jcslot;
  s.p.jmode = jmode;
  if (lut_max >= lut_min) {
    s.p.jlut = PTR_LUT;
    s.p.jlut_min = lut_min;
    s.p.jlut_max = lut_max;
  }
}

void sparse(Shape &s, std::initializer_list<int> gcols, int radix) {
  group(s, gcols, 0);
  s.p.sparse = 1;
  s.p.hcap_log2 = 16;
  s.p.radix = radix;
}

Shape with_env(Shape s, const char *name, const char *env, const char *val) {
  s.name = name;
  s.env_name = env;
  s.env_val = val;
  return s;
}

std::vector<Shape> shape_table() {
  std::vector<Shape> t;

  /* ---- keyless register accumulators ---- */
  Shape q6 = blank("keyless_q6", 0, 2);
  cols(q6, { SN_K_F64, SN_K_F64, SN_K_F64, SN_K_F64 });
  pred_d(q6, 0, 8766.0, 9130.0);
  pred_d(q6, 1, 0.05, 0.07);
  pred_d(q6, 2, -1e300, 23.99);
  agg(q6, 0, { 3, 1 });
  agg(q6, 0, {});
  t.push_back(q6);

  Shape q6d = q6;
  q6d.name = "keyless_q6_del";
  q6d.has_del = 1;
  t.push_back(q6d);

  Shape kk = blank("keyless_all_kinds", 0, 8);
  cols(kk, { SN_K_I32, SN_K_F32, SN_K_I16, SN_K_I64, SN_K_DICT16, SN_K_DICT32 });
  pred_d(kk, 0, 10.0, 20.0);
  pred_i(kk, 3, -5, 1ll << 40);
  inlist(kk, 4);
  for (int c = 0; c < 6; c++) agg(kk, 0, { c });
  agg(kk, 0, { 3, 0, 2 });
  agg(kk, 0, {});
  t.push_back(kk);

  Shape kf = blank("keyless_factors", 0, 4);
  cols(kf, { SN_K_F64, SN_K_F64, SN_K_F64 });
  pred_d(kf, 1, 0.0, 1.0);
  agg(kf, 0, { 0, 1, 2 });          /* ep * (1 - disc) * (1 + tax) */
  kf.p.aggs[0].a1 = 1.0; kf.p.aggs[0].m1 = -1.0;
  kf.p.aggs[0].a2 = 1.0; kf.p.aggs[0].m2 = 1.0;
  agg(kf, 0, { 0, 1 });
  kf.p.aggs[1].a0 = 2.5; kf.p.aggs[1].m0 = 0.5;
  agg(kf, 0, { 2 });
  t.push_back(kf);

  /* keyless MIN/MAX: the grouped (pac) layout with one slot */
  Shape km = blank("keyless_minmax", 1, 4);
  cols(km, { SN_K_F64, SN_K_I32 });
  km.p.pac = 1;
  pred_d(km, 1, 0.0, 100.0);
  agg(km, 1, { 0 });
  agg(km, 2, { 0 });
  agg(km, 0, { 1 });
  t.push_back(km);

  /* ---- grouped register accumulators ---- */
  Shape q1 = blank("regs_q1", 6, 8);
  cols(q1, { SN_K_DICT16, SN_K_DICT16, SN_K_F64, SN_K_F64, SN_K_F64,
             SN_K_F64, SN_K_I32 });
  group(q1, { 0, 1 }, 1);
  pred_d(q1, 6, -1e300, 10471.0);
  agg(q1, 0, { 2 });
  agg(q1, 0, { 3 });
  agg(q1, 0, { 3, 4 });
  q1.p.aggs[2].a1 = 1.0; q1.p.aggs[2].m1 = -1.0;
  agg(q1, 0, { 3, 4, 5 });
  q1.p.aggs[3].a1 = 1.0; q1.p.aggs[3].m1 = -1.0;
  q1.p.aggs[3].a2 = 1.0; q1.p.aggs[3].m2 = 1.0;
  agg(q1, 0, { 4 });
  t.push_back(q1);

  Shape rm = blank("regs_minmax", 4, 4);
  cols(rm, { SN_K_I32, SN_K_F64 });
  rm.p.pac = 1;
  group(rm, { 0 }, 1);
  rm.p.gbase[0] = 7;
  agg(rm, 1, { 1 });
  agg(rm, 2, { 1 });
  agg(rm, 0, { 1 });
  t.push_back(rm);

  /* ---- wbin: per-16-lane LDS bins ---- */
  Shape wb = blank("wbin_8x2", 8, 2);
  cols(wb, { SN_K_I16, SN_K_F64, SN_K_F32 });
  group(wb, { 0 }, 1);
  wb.p.gbase[0] = -3;
  agg(wb, 0, { 1 });
  agg(wb, 0, { 2 });
  t.push_back(wb);

  /* ---- block LDS accumulator ---- */
  Shape ld = blank("lds_600", 600, 2);
  cols(ld, { SN_K_I32, SN_K_I32, SN_K_F64 });
  group(ld, { 0, 1 }, 30);
  ld.p.gbase[0] = 100; ld.p.gbase[1] = 1;
  pred_d(ld, 2, 0.0, 5.0);
  agg(ld, 0, { 2 });
  agg(ld, 0, { 2, 2 });
  t.push_back(ld);

  Shape lm = blank("lds_600_minmax", 600, 4);
  cols(lm, { SN_K_I32, SN_K_F64 });
  lm.p.pac = 1;
  group(lm, { 0 }, 1);
  agg(lm, 1, { 1 });
  agg(lm, 0, { 1 });
  agg(lm, 2, { 1 });
  t.push_back(lm);

  /* ---- XCD-privatised global accumulator ---- */
  Shape gl = blank("global_20000", 20000, 2);
  cols(gl, { SN_K_I32, SN_K_F64 });
  group(gl, { 0 }, 1);
  agg(gl, 0, { 1 });
  agg(gl, 0, {});
  t.push_back(gl);

  Shape gp = blank("global_20000_pac", 20000, 2);
  cols(gp, { SN_K_I32, SN_K_F64 });
  gp.p.pac = 1;
  group(gp, { 0 }, 1);
  agg(gp, 2, { 1 });
  agg(gp, 0, { 1 });
  t.push_back(gp);

  /* ---- join probes ---- */
  Shape jh = blank("join_hash_semi", 0, 2);
  cols(jh, { SN_K_I32, SN_K_F64 });
  join(jh, 0, 0, 0, -1);
  pred_d(jh, 1, 0.0, 10.0);
  agg(jh, 0, { 1 });
  agg(jh, 0, {});
  t.push_back(jh);

  Shape jhk = blank("join_hash_i64key", 0, 1);
  cols(jhk, { SN_K_I64 });
  join(jhk, 0, 0, 0, -1);
  agg(jhk, 0, {});
  t.push_back(jhk);

  /* star join: span far beyond the 100 KiB nibble LUT -> L2 probe via spay */
  Shape js = blank("join_spay_bigspan", 8, 2);
  cols(js, { SN_K_I32, SN_K_F64, SN_K_F64 });
  join(js, 0, 1, 1, 6000000);
  agg(js, 0, { 1 });
  agg(js, 0, { 1, 2 });
  t.push_back(js);
  t.push_back(with_env(js, "join_spay_bigspan_slut0", "SN_JIT_SLUT", "0"));

  Shape js16 = blank("join_spay_i16key", 0, 1);
  cols(js16, { SN_K_I16, SN_K_F64 });
  join(js16, 0, 0, -20000, 4000000);
  agg(js16, 0, { 1 });
  t.push_back(js16);

  Shape js64 = blank("join_spay_i64key", 0, 1);
  cols(js64, { SN_K_I64, SN_K_F64 });
  join(js64, 0, 0, 5, 3000000);
  agg(js64, 0, { 1 });
  t.push_back(js64);

  Shape jsf = blank("join_spay_f64key", 0, 1);
  cols(jsf, { SN_K_F64, SN_K_F64 });
  join(jsf, 0, 0, 5, 3000000);
  agg(jsf, 0, { 1 });
  t.push_back(jsf);

  Shape sl0 = blank("join_slut_semi", 0, 2);
  cols(sl0, { SN_K_I32, SN_K_F64 });
  join(sl0, 0, 0, 0, 19999);
  agg(sl0, 0, { 1 });
  agg(sl0, 0, {});
  t.push_back(sl0);
  /* the same small span with the nibble LUT switched off -> spay */
  t.push_back(with_env(sl0, "join_slut_semi_slut0", "SN_JIT_SLUT", "0"));

  Shape sl1 = blank("join_slut_attr", 8, 2);
  cols(sl1, { SN_K_I64, SN_K_F64 });
  join(sl1, 0, 1, 100, 50099);
  agg(sl1, 0, { 1 });
  agg(sl1, 0, {});
  t.push_back(sl1);

  Shape jc = blank("join_composite_factkey", 32, 2);
  cols(jc, { SN_K_I32, SN_K_I32, SN_K_F64 });
  join(jc, 0, 1, 0, 9999);
  jc.p.jslot_mul = 4;
  group(jc, { 1 }, 1);
  jc.p.gbase[0] = 1992;
  agg(jc, 0, { 2 });
  agg(jc, 0, {});
  t.push_back(jc);

  Shape jd = sl0;
  jd.name = "join_slut_semi_del";
  jd.has_del = 1;
  t.push_back(jd);

  Shape jsd = js;
  jsd.name = "join_spay_del";
  jsd.has_del = 1;
  t.push_back(jsd);

  /* ---- sparse hash aggregate ---- */
  Shape sp = blank("sparse_i64key", 0, 2);
  cols(sp, { SN_K_I64, SN_K_F64 });
  sparse(sp, { 0 }, 0);
  pred_d(sp, 1, 0.0, 1e9);
  agg(sp, 0, { 1 });
  agg(sp, 0, {});
  t.push_back(sp);

  Shape sp32 = blank("sparse_i32key", 0, 1);
  cols(sp32, { SN_K_I32, SN_K_F64 });
  sparse(sp32, { 0 }, 0);
  agg(sp32, 0, { 1 });
  t.push_back(sp32);

  Shape sp2 = blank("sparse_packed2x32", 0, 2);
  cols(sp2, { SN_K_I32, SN_K_I32, SN_K_F64 });
  sparse(sp2, { 0, 1 }, 0);
  agg(sp2, 0, { 2 });
  agg(sp2, 1, { 2 });
  t.push_back(sp2);

  Shape sr = blank("sparse_radix", 0, 2);
  cols(sr, { SN_K_I64, SN_K_F64, SN_K_F64 });
  sparse(sr, { 0 }, SN_RADIX_SUB_MIN);
  agg(sr, 0, { 1 });
  agg(sr, 0, { 1, 2 });
  t.push_back(sr);

  Shape srd = sr;
  srd.name = "sparse_radix_del";
  srd.has_del = 1;
  t.push_back(srd);

  t.push_back(with_env(sp, "sparse_i64key_spocc2", "SN_JIT_SPOCC", "2"));
  return t;
}

uint64_t fnv1a(const std::string &s, size_t from) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = from; i < s.size(); i++) {
    h ^= (uint8_t)s[i];
    h *= 1099511628211ull;
  }
  return h;
}

bool compile_gfx950(const Shape &s, const std::string &src) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "sn_jit.cu", 0, nullptr,
                          nullptr) != HIPRTC_SUCCESS) {
    fprintf(stderr, "%s: hiprtcCreateProgram failed\n", s.name);
    return false;
  }
  const char *opts[] = { "--offload-arch=gfx950", "-O3" };
  const bool ok = hiprtcCompileProgram(prog, 2, opts) == HIPRTC_SUCCESS;
  if (!ok) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    std::vector<char> log(lsz + 1, 0);
    if (lsz) hiprtcGetProgramLog(prog, log.data());
    fprintf(stderr, "%s: compile failed:\n%s\n", s.name, log.data());
  }
  hiprtcDestroyProgram(&prog);
  return ok;
}

const char KERNEL_MARK[] = "extern \"C\" __global__";

/* one shape in THIS process: print its line; returns false on failure */
bool run_shape(const Shape &s, bool compile, std::string *prelude) {
  const std::string src = gen_source(&s.p, s.kinds, s.nslots, s.na_t, s.has_del);
  const size_t cut = src.find(KERNEL_MARK);
  if (cut == std::string::npos) {
    fprintf(stderr, "%s: no kernel in the generated source\n", s.name);
    return false;
  }
  if (prelude) *prelude = src.substr(0, cut);
  printf("%s %016llx\n", s.name, (unsigned long long)fnv1a(src, cut));
  fflush(stdout);
  return !compile || compile_gfx950(s, src);
}

/* a shape that names an environment variable: same program, fresh process */
bool run_shape_in_child(const Shape &s, bool compile) {
  char exe[4096];
  const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
  if (n <= 0) { perror("readlink"); return false; }
  exe[n] = 0;
  fflush(stdout);
  setenv(s.env_name, s.env_val, 1);
  std::string cmd = std::string("'") + exe + "' --one " + s.name +
                    (compile ? " --compile" : "");
  const int rc = system(cmd.c_str());
  unsetenv(s.env_name);
  return rc == 0;
}

}  // namespace

int main(int argc, char **argv) {
  bool compile = false;
  const char *one = nullptr, *dump = nullptr;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--compile")) compile = true;
    else if (!strcmp(argv[i], "--one") && i + 1 < argc) one = argv[++i];
    else if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else { fprintf(stderr, "usage: %s [--compile] [--dump NAME]\n", argv[0]); return 2; }
  }
  const std::vector<Shape> table = shape_table();
  if (one || dump) {
    for (const Shape &s : table) {
      if (strcmp(s.name, one ? one : dump)) continue;
      if (one) return run_shape(s, compile, nullptr) ? 0 : 1;
      fputs(gen_source(&s.p, s.kinds, s.nslots, s.na_t, s.has_del).c_str(), stdout);
      return 0;
    }
    fprintf(stderr, "no such shape\n");
    return 2;
  }
  bool ok = true;
  std::string prelude;
  for (const Shape &s : table)
    ok &= s.env_name ? run_shape_in_child(s, compile)
                     : run_shape(s, compile, &prelude);
  printf("---- prelude ----\n%s", prelude.c_str());
  return ok ? 0 : 1;
}
