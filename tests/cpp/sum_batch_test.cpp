// tests/cpp/sum_batch_test.cpp -- the C++ mirror's segmented point sums (include/mlhip_driver.hpp: SumG1Batch, SumG2Batch,
// Bases::SumBatch) against the single sums they batch (SumG1 / SumG2), on every curve.  Driven by tests/test_sum_batch_gpu.py.
// Needs a GPU.
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
  for (int i = 0; i < 40; i++) pts.push_back(g.Mul(c.NewRandomZr(st)));
  pts[5] = c.NewG1();  // a point at infinity
  G1 neg = pts[7];
  neg.Neg();
  // segment lengths 3, 0, 1, 21 (six slices of 4), 2 (P beside -P), 4 (one point four times), 40
  std::vector<std::vector<G1>> a = {slice(pts, 0, 3), {}, slice(pts, 3, 4), slice(pts, 4, 25), {pts[7], neg},
                                    {pts[9], pts[9], pts[9], pts[9]}, pts};
  std::vector<G1> got = c.SumG1Batch(a);
  EXPECT(got.size() == a.size());
  int same = 0;
  for (size_t i = 0; i < a.size() && i < got.size(); i++) same += got[i].Equals(c.SumG1(a[i])) ? 1 : 0;
  EXPECT(same == (int)a.size());
  EXPECT(got.size() == a.size() && got[1].IsInfinity() && got[4].IsInfinity() && !got[3].IsInfinity());
  EXPECT(c.SumG1Batch({}).empty());
  // the handle forms: index lists (a repeat, an index in two segments, an empty list) and leading lengths
  Bases bases(c, pts);
  const size_t tabled = bases.BatchTabled();
  std::vector<std::vector<uint32_t>> index = {{5, 9, 9, 39}, {}, {39, 0, 1, 2, 3, 4, 6, 7, 8}};
  std::vector<G1> bi = bases.SumBatch(index);
  int ok_index = 0;
  for (size_t i = 0; i < index.size() && i < bi.size(); i++) {
    std::vector<G1> l;
    for (uint32_t x : index[i]) l.push_back(pts[x]);
    ok_index += bi[i].Equals(c.SumG1(l)) ? 1 : 0;
  }
  EXPECT(ok_index == (int)index.size());
  std::vector<size_t> lengths = {0, 1, 9, 40};
  std::vector<G1> bl = bases.SumBatch(lengths);
  int ok_len = 0;
  for (size_t i = 0; i < lengths.size() && i < bl.size(); i++) ok_len += bl[i].Equals(c.SumG1(slice(pts, 0, lengths[i]))) ? 1 : 0;
  EXPECT(ok_len == (int)lengths.size());
  EXPECT(bases.BatchTabled() == tabled && tabled == 0);
  bool threw = false;
  try {
    bases.SumBatch(std::vector<std::vector<uint32_t>>{{40}});
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    bases.SumBatch(std::vector<size_t>{41});
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  printf("%s sum_batch_g1 %d/%d bases_index %d/%d bases_lengths %d/%d\n", kNames[c.id], same, (int)a.size(), ok_index,
         (int)index.size(), ok_len, (int)lengths.size());
}

static void runG2(const Curve& c, const G2& h, uint64_t& st) {
  std::vector<G2> pts;
  for (int i = 0; i < 11; i++) pts.push_back(h.Mul(c.NewRandomZr(st)));
  std::vector<std::vector<G2>> a = {slice(pts, 0, 2), slice(pts, 2, 11), {}, slice(pts, 0, 1), {pts[3], pts[3]}};
  std::vector<G2> got = c.SumG2Batch(a);
  int same = 0;
  for (size_t i = 0; i < a.size() && i < got.size(); i++) same += got[i].Equals(c.SumG2(a[i])) ? 1 : 0;
  EXPECT(same == (int)a.size());
  EXPECT(got.size() == a.size() && got[2].IsInfinity());
  printf("%s sum_batch_g2 %d/%d\n", kNames[c.id], same, (int)a.size());
}

int main(int argc, char** argv) {
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 4242 + id;
    runG1(c, st);
    if (id != MLHIP_CURVE_BLS12_377)
      runG2(c, c.GenG2(), st);
    else if (argc > 4)  // the G2 generator of BLS12-377 comes from the golden file (decimal coordinates)
      runG2(c, c.NewG2FromCoords(argv[1], argv[2], argv[3], argv[4]), st);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
