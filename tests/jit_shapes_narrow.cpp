/*
 * jit_shapes_narrow.cpp — stand-alone host program over the query-compiled
 * kernel SOURCE (csrc/jit.cpp) for plan shapes that read narrowed f64 columns
 * (SN_K_F64C8: 1-byte codes into a per-batch value dictionary).
 *
 * jit_shapes.cpp pins the text of every shape WITHOUT such a column; this
 * program covers the shapes with one, so the two tables never share a golden
 * file.  No GPU is needed: hipRTC compiles for gfx950 on any host.
 *
 *   jit_shapes_narrow              compile every shape with hipRTC for gfx950,
 *                                  print "<shape> ok" per shape; exit 1 if a
 *                                  compile fails
 *   jit_shapes_narrow --dump NAME  print the full generated source of a shape
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

  /* Q6: qty (codes), extendedprice (f64), discount (codes), shipdate */
  Shape q6 = blank("narrow_keyless_q6", 0, 2);
  cols(q6, { SN_K_F64C8, SN_K_F64, SN_K_F64C8, SN_K_I32 });
  pred_d(q6, 3, 8766.0, 9130.0);
  pred_d(q6, 2, 0.05, 0.07);
  pred_d(q6, 0, -1e300, 23.99);
  agg(q6, { 1, 2 });
  agg(q6, {});
  t.push_back(q6);

  Shape q6d = q6;
  q6d.name = "narrow_keyless_q6_del";
  q6d.has_del = 1;
  t.push_back(q6d);

  /* Q1: two DICT16 keys; qty, discount and tax narrowed, extendedprice not */
  Shape q1 = blank("narrow_regs_q1", 6, 8);
  cols(q1, { SN_K_DICT16, SN_K_DICT16, SN_K_F64C8, SN_K_F64, SN_K_F64C8,
             SN_K_F64C8, SN_K_I32 });
  q1.p.gcol[0] = 0; q1.p.gcol[1] = 1;
  q1.p.ngroup = 2;
  q1.p.gmul0 = 1;
  pred_d(q1, 6, -1e300, 10471.0);
  agg(q1, { 2 });
  agg(q1, { 3 });
  agg(q1, { 3, 4 });
  q1.p.aggs[2].a1 = 1.0; q1.p.aggs[2].m1 = -1.0;
  agg(q1, { 3, 4, 5 });
  q1.p.aggs[3].a1 = 1.0; q1.p.aggs[3].m1 = -1.0;
  q1.p.aggs[3].a2 = 1.0; q1.p.aggs[3].m2 = 1.0;
  agg(q1, { 4 });
  t.push_back(q1);
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
