// tests/cpp/bases_batch_test.cpp -- the C++ mirror's batched MSM over resident bases (include/mlhip_driver.hpp:
// Bases::MultiScalarMulBatch, Bases::BatchTabled) against the MSMs it batches, with and without index lists, and its
// length and index rules, on every curve.  Driven by tests/test_bases_batch_cpp.py.  Needs a GPU.
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

static void run(const Curve& c, uint64_t& st) {
  const G1 g = c.GenG1();
  std::vector<G1> pts;
  std::vector<Zr> zr;
  for (int i = 0; i < 12; i++) pts.push_back(g.Mul(c.NewRandomZr(st)));
  for (int i = 0; i < 40; i++) zr.push_back(c.NewRandomZr(st));
  pts[4] = c.NewG1();  // a base at infinity
  Bases bases(c, pts);
  EXPECT(bases.BatchTabled() == 0);
  // positional: pair j of a segment takes base j
  std::vector<std::vector<Zr>> b = {slice(zr, 0, 3), {}, slice(zr, 3, 15), slice(zr, 15, 16)};
  std::vector<G1> got = bases.MultiScalarMulBatch(b);
  int same = 0;
  for (size_t i = 0; i < b.size() && i < got.size(); i++) same += got[i].Equals(bases.MultiScalarMul(b[i])) ? 1 : 0;
  EXPECT(got.size() == b.size() && got[1].IsInfinity());
  // indexed: repeated bases, the base at infinity, (B, s) beside (B, -s)
  std::vector<std::vector<uint32_t>> ix = {{11, 0, 11}, {}, {4, 4, 4, 1, 2, 3, 5, 6, 7, 8, 9, 10}, {7}};
  std::vector<std::vector<Zr>> b2 = b;
  b2[0][2] = c.NewZrFromInt(0).Minus(b2[0][0]);  // [s]B11 + [t]B0 + [-s]B11 = [t]B0
  std::vector<G1> got2 = bases.MultiScalarMulBatch(b2, &ix);
  int same2 = 0;
  for (size_t i = 0; i < b2.size() && i < got2.size(); i++) {
    std::vector<G1> a;
    for (uint32_t x : ix[i]) a.push_back(pts[x]);
    same2 += got2[i].Equals(c.MultiScalarMul(a, b2[i])) ? 1 : 0;
  }
  EXPECT(got2.size() == 4 && got2[0].Equals(pts[0].Mul(b2[0][1])));
  EXPECT(bases.BatchTabled() == 12);
  bool threw = false;
  try {
    bases.MultiScalarMulBatch({slice(zr, 0, 13)});
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    std::vector<std::vector<uint32_t>> bad = {{0, 12}};
    bases.MultiScalarMulBatch({slice(zr, 0, 2)}, &bad);
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    std::vector<std::vector<uint32_t>> bad = {{0}};
    bases.MultiScalarMulBatch({slice(zr, 0, 2)}, &bad);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  EXPECT(bases.MultiScalarMulBatch({}).empty());
  printf("%s bases_batch %d/%d indexed %d/%d\n", kNames[c.id], same, (int)b.size(), same2, (int)b2.size());
}

int main() {
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 991 + id;
    run(c, st);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
