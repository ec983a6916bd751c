// tests/cpp/msm_batch_test.cpp -- the C++ mirror's batched MSM (include/mlhip_driver.hpp: MultiScalarMulBatch,
// MultiScalarMulG2Batch, Mul2Batch) against the single-MSM calls it batches, with their length rules, on every curve.
// Driven by tests/test_msm_batch_cpp.py.  Needs a GPU.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "mlhip_driver.hpp"

using namespace mlhip_driver;

static int g_fail = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                \
      g_fail++;                                                             \
    }                                                                       \
  } while (0)

static const char* kNames[3] = {"BN254", "BLS12-381", "BLS12-377"};

template <class P>
static std::vector<P> slice(const std::vector<P>& v, size_t a, size_t b) {
  return std::vector<P>(v.begin() + a, v.begin() + b);
}

static void runG1(const Curve& c, uint64_t& st) {
  const G1 g = c.GenG1();
  std::vector<G1> pts;
  std::vector<Zr> zr;
  for (int i = 0; i < 24; i++) {
    pts.push_back(g.Mul(c.NewRandomZr(st)));
    zr.push_back(c.NewRandomZr(st));
  }
  pts[5] = c.NewG1();  // a point at infinity
  zr[6] = c.NewZrFromInt(0);
  // segment lengths 3, 0, 1, 7, 2 (more scalars than points: identity), 11 (holds the same pair twice)
  std::vector<std::vector<G1>> a = {slice(pts, 0, 3), {}, slice(pts, 3, 4), slice(pts, 4, 11), slice(pts, 11, 13), slice(pts, 13, 24)};
  std::vector<std::vector<Zr>> b = {slice(zr, 0, 3), {}, slice(zr, 3, 4), slice(zr, 4, 11), slice(zr, 11, 14), slice(zr, 13, 24)};
  a[5][3] = a[5][2];
  b[5][3] = b[5][2];
  std::vector<G1> got = c.MultiScalarMulBatch(a, b);
  EXPECT(got.size() == a.size());
  int same = 0;
  for (size_t i = 0; i < a.size() && i < got.size(); i++) same += got[i].Equals(c.MultiScalarMul(a[i], b[i])) ? 1 : 0;
  EXPECT(same == (int)a.size());
  EXPECT(got.size() == a.size() && got[1].IsInfinity() && got[4].IsInfinity() && !got[3].IsInfinity());
  bool threw = false;
  try {
    c.MultiScalarMulBatch({slice(pts, 0, 3)}, {slice(zr, 0, 2)});
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  EXPECT(c.MultiScalarMulBatch({}, {}).empty());
  std::vector<G1> gs = slice(pts, 0, 8), qs = slice(pts, 8, 16);
  std::vector<Zr> e = slice(zr, 0, 8), f = slice(zr, 8, 16);
  std::vector<G1> m2 = c.Mul2Batch(gs, e, qs, f);
  int ok2 = 0;
  for (size_t i = 0; i < gs.size() && i < m2.size(); i++) ok2 += m2[i].Equals(gs[i].Mul2(e[i], qs[i], f[i])) ? 1 : 0;
  EXPECT(ok2 == 8);
  printf("%s msm_batch_g1 %d/%d mul2_batch %d/8\n", kNames[c.id], same, (int)a.size(), ok2);
}

static void runG2(const Curve& c, const G2& h, uint64_t& st) {
  std::vector<G2> pts;
  std::vector<Zr> zr;
  for (int i = 0; i < 9; i++) {
    pts.push_back(h.Mul(c.NewRandomZr(st)));
    zr.push_back(c.NewRandomZr(st));
  }
  std::vector<std::vector<G2>> a = {slice(pts, 0, 2), slice(pts, 2, 9), {}, slice(pts, 0, 1)};
  std::vector<std::vector<Zr>> b = {slice(zr, 0, 2), slice(zr, 2, 9), slice(zr, 0, 1), slice(zr, 0, 1)};
  std::vector<G2> got = c.MultiScalarMulG2Batch(a, b);
  int same = 0;
  for (size_t i = 0; i < a.size() && i < got.size(); i++) same += got[i].Equals(c.MultiScalarMulG2(a[i], b[i])) ? 1 : 0;
  EXPECT(same == (int)a.size());
  EXPECT(got.size() == a.size() && got[2].IsInfinity());
  printf("%s msm_batch_g2 %d/%d\n", kNames[c.id], same, (int)a.size());
}

int main(int argc, char** argv) {
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 777 + id;
    runG1(c, st);
    if (id != MLHIP_CURVE_BLS12_377)
      runG2(c, c.GenG2(), st);
    else if (argc > 4)  // the G2 generator of BLS12-377 comes from the golden file (decimal coordinates)
      runG2(c, c.NewG2FromCoords(argv[1], argv[2], argv[3], argv[4]), st);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
