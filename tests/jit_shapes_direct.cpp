/*
 * jit_shapes_direct.cpp — stand-alone host program over the query-compiled
 * kernel SOURCE (csrc/jit.cpp) for plan shapes whose late columns carry
 * SN_K_F64_LATE_DIRECT: the image-free keyless kernel of DESIGN.md §2d.
 *
 * jit_shapes_late.cpp pins the shapes with SN_K_F64_LATE; this program
 * covers the new tag, and can generate each shape with SN_K_F64_LATE in its
 * place, to show that the old tag's text did not move.  No GPU is needed:
 * hipRTC compiles for gfx950 on any host.
 *
 *   jit_shapes_direct                   compile every shape with hipRTC for
 *                                       gfx950, print "<shape> ok" per shape;
 *                                       exit 1 if a compile fails
 *   jit_shapes_direct --dump NAME       print the generated source of a shape
 *   jit_shapes_direct --late-twin NAME  the same plan, tag SN_K_F64_LATE
 *   jit_shapes_direct --code NAME FILE  write the shape's code object to FILE
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
  Shape q6 = blank("direct_keyless_q6", 0, 2);
  cols(q6, { SN_K_F64C8, SN_K_F64_LATE_DIRECT, SN_K_F64C8, SN_K_I32 });
  pred_d(q6, 3, 8766.0, 9130.0);
  pred_d(q6, 2, 0.05, 0.07);
  pred_d(q6, 0, -1e300, 23.99);
  agg(q6, { 1, 2 });
  agg(q6, {});
  t.push_back(q6);

  Shape q6d = q6;
  q6d.name = "direct_keyless_q6_del";
  q6d.has_del = 1;
  t.push_back(q6d);

  /* an int16 key with two range predicates, a narrowed predicate column */
  Shape i16 = blank("direct_keyless_i16", 0, 2);
  cols(i16, { SN_K_I16, SN_K_F64_LATE_DIRECT, SN_K_F64C8 });
  pred_d(i16, 0, -5.0, 300.0);
  pred_d(i16, 0, 7.0, 1e300);
  pred_d(i16, 2, 0.05, 0.07);
  agg(i16, { 1 });
  agg(i16, { 0, 1 });
  t.push_back(i16);

  /* SUM(a*b), both aggregate-only, one int predicate column */
  Shape two = blank("direct_keyless_two", 0, 2);
  cols(two, { SN_K_I32, SN_K_F64_LATE_DIRECT, SN_K_F64_LATE_DIRECT });
  pred_d(two, 0, 8766.0, 9130.0);
  agg(two, { 1, 2 });
  agg(two, {});
  t.push_back(two);

  /* a narrowed column that only an aggregate factor reads */
  Shape fac = blank("direct_keyless_factor", 0, 2);
  cols(fac, { SN_K_I32, SN_K_F64_LATE_DIRECT, SN_K_F64C8 });
  pred_d(fac, 0, 8766.0, 9130.0);
  agg(fac, { 1, 2 });
  agg(fac, {});
  t.push_back(fac);
  return t;
}

bool compile_gfx950(const Shape &s, const std::string &src,
                    std::vector<char> *code) {
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
  } else if (code) {
    size_t csz = 0;
    hiprtcGetCodeSize(prog, &csz);
    code->resize(csz);
    hiprtcGetCode(prog, code->data());
  }
  hiprtcDestroyProgram(&prog);
  return ok;
}

}  // namespace

int main(int argc, char **argv) {
  const char *dump = nullptr, *code_to = nullptr;
  bool twin = false;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else if (!strcmp(argv[i], "--late-twin") && i + 1 < argc)
      dump = argv[++i], twin = true;
    else if (!strcmp(argv[i], "--code") && i + 2 < argc)
      dump = argv[++i], code_to = argv[++i];
    else {
      fprintf(stderr, "usage: %s [--dump NAME | --late-twin NAME | "
                      "--code NAME FILE]\n", argv[0]);
      return 2;
    }
  }
  bool ok = true;
  for (Shape s : shape_table()) {
    if (dump && strcmp(s.name, dump)) continue;
    if (twin)
      for (int c = 0; c < s.p.nused; c++)
        if (s.kinds[c] == SN_K_F64_LATE_DIRECT) s.kinds[c] = SN_K_F64_LATE;
    const std::string src =
        gen_source(&s.p, s.kinds, s.nslots, s.na_t, s.has_del);
    if (code_to) {
      std::vector<char> code;
      if (!compile_gfx950(s, src, &code)) return 1;
      FILE *f = fopen(code_to, "wb");
      if (!f) { perror(code_to); return 1; }
      fwrite(code.data(), 1, code.size(), f);
      fclose(f);
      return 0;
    }
    if (dump) {
      fputs(src.c_str(), stdout);
      return 0;
    }
    const bool good = compile_gfx950(s, src, nullptr);
    printf("%s %s\n", s.name, good ? "ok" : "FAILED");
    ok &= good;
  }
  if (dump) { fprintf(stderr, "no such shape\n"); return 2; }
  return ok ? 0 : 1;
}
