/*
 * jit_shapes_late.cpp — stand-alone host program over the query-compiled
 * kernel SOURCE (csrc/jit.cpp) for plan shapes with a late column
 * (SN_K_F64_LATE: an aggregate-only double column that the kernel reads in
 * the row phase, for the passing rows only, instead of staging it).
 *
 * jit_shapes.cpp and jit_shapes_narrow.cpp pin the shapes WITHOUT such a
 * column; this program covers the shapes with one.  No GPU is needed: hipRTC
 * compiles for gfx950 on any host.
 *
 *   jit_shapes_late              compile every shape with hipRTC for gfx950,
 *                                print "<shape> ok" per shape; exit 1 if a
 *                                compile fails
 *   jit_shapes_late --dump NAME  print the full generated source of a shape
 */
#include "../snappydata_amd/csrc/jit.cpp"

namespace {

struct Shape {
  const char *name;
  sn_dev_plan p;
  int kinds[SN_DEV_MAX_COLS];
  int nslots, na_t, has_del;
};

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
  for (int k : kinds) s.kinds[c++] = k;
  s.p.nused = c;
}

/* aggregate over up to three trivial (a=0, m=1) factors */
void agg(Shape &s, std::initializer_list<int> factors) {
  sn_dev_agg &A = s.p.aggs[s.p.naggs++];
  int c[3] = { 0, 0, 0 }, n = 0;
  for (int f : factors) c[n++] = f;
  A.nf = n;
  A.op = 0;
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

std::vector<Shape> shape_table() {
  std::vector<Shape> t;

  /* Q6: qty (codes), extendedprice (late), discount (codes), shipdate */
  Shape q6 = blank("late_keyless_q6", 0, 2);
  cols(q6, { SN_K_F64C8, SN_K_F64_LATE, SN_K_F64C8, SN_K_I32 });
  pred_d(q6, 3, 8766.0, 9130.0);
  pred_d(q6, 2, 0.05, 0.07);
  pred_d(q6, 0, -1e300, 23.99);
  agg(q6, { 1, 2 });
  agg(q6, {});
  t.push_back(q6);

  Shape q6d = q6;
  q6d.name = "late_keyless_q6_del";
  q6d.has_del = 1;
  t.push_back(q6d);

  /* the same over plain f64 predicate columns (SN_NARROW=0) */
  Shape q6f = q6;
  q6f.name = "late_keyless_q6_f64";
  q6f.kinds[0] = q6f.kinds[2] = SN_K_F64;
  t.push_back(q6f);

  /* SUM(a*b), both aggregate-only, one int predicate column */
  Shape two = blank("late_keyless_two", 0, 2);
  cols(two, { SN_K_I32, SN_K_F64_LATE, SN_K_F64_LATE });
  pred_d(two, 0, 8766.0, 9130.0);
  agg(two, { 1, 2 });
  agg(two, {});
  t.push_back(two);

  /* keyless MIN and MAX over a late column: MIN/MAX plans take the grouped
   * (pac) layout with one slot, register accumulators */
  Shape mm = blank("late_single_minmax", 1, 2);
  cols(mm, { SN_K_F64C8, SN_K_F64_LATE, SN_K_I32 });
  mm.p.pac = 1;
  pred_d(mm, 2, 8766.0, 9130.0);
  pred_d(mm, 0, 0.05, 0.07);
  agg(mm, { 1 });
  mm.p.aggs[0].op = 1;
  agg(mm, { 1 });
  mm.p.aggs[1].op = 2;
  agg(mm, { 1, 0 });
  t.push_back(mm);
  return t;
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

}  // namespace

int main(int argc, char **argv) {
  const char *dump = nullptr;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else { fprintf(stderr, "usage: %s [--dump NAME]\n", argv[0]); return 2; }
  }
  bool ok = true;
  for (const Shape &s : shape_table()) {
    const std::string src =
        gen_source(&s.p, s.kinds, s.nslots, s.na_t, s.has_del);
    if (dump) {
      if (strcmp(s.name, dump)) continue;
      fputs(src.c_str(), stdout);
      return 0;
    }
    const bool good = compile_gfx950(s, src);
    printf("%s %s\n", s.name, good ? "ok" : "FAILED");
    ok &= good;
  }
  if (dump) { fprintf(stderr, "no such shape\n"); return 2; }
  return ok ? 0 : 1;
}
