// tests/cpp/g2_prepared_test.cpp -- the C++ mirror's prepared G2 handles (include/mlhip_driver.hpp: G2Prepared) against the
// Pairing2 + FExp they replace, with and without an index, and their length and index rules, on every curve; and the raw
// C entry points mlhip_g2_prepared_create / _count / _destroy.  Driven by tests/test_g2_prepared_cpp.py.  Needs a GPU.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "mlhip_driver.hpp"

using namespace mlhip_driver;

static int g_fail = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail++;                                              \
    }                                                        \
  } while (0)

static const char* kNames[3] = {"BN254", "BLS12-381", "BLS12-377"};

static void run(const Curve& c, const G2& g, uint64_t& st) {
  const G1 g1 = c.GenG1();
  const G2 pk = g.Mul(c.NewRandomZr(st));
  G2Prepared prep(c, {g, pk, c.NewG2()});  // slot 2: the point at infinity
  EXPECT(prep.Count() == 3);
  std::vector<std::vector<G1>> proofs;
  for (int k = 0; k < 7; k++) proofs.push_back({g1.Mul(c.NewRandomZr(st)), g1.Mul(c.NewRandomZr(st))});
  proofs[3][1] = c.NewG1();  // a G1 argument at infinity
  std::vector<Gt> fused = prep.PairingBatch(proofs);
  std::vector<Gt> raw = prep.MillerLoopBatch(proofs);
  int same = 0;
  for (size_t k = 0; k < proofs.size() && k < fused.size() && k < raw.size(); k++) {
    const Gt want = c.FExp(c.Pairing2(g, pk, proofs[k][0], proofs[k][1]));
    same += (fused[k].Equals(want) && c.FExp(raw[k]).Equals(want)) ? 1 : 0;
  }
  EXPECT(same == (int)proofs.size());
  // an index: (pk, g) instead of (g, pk); and a pair against the point at infinity contributes 1
  std::vector<uint32_t> swap = {1, 0}, dead = {0, 2};
  std::vector<Gt> sw = prep.PairingBatch(proofs, &swap), dd = prep.PairingBatch(proofs, &dead);
  int same2 = 0;
  for (size_t k = 0; k < proofs.size() && k < sw.size() && k < dd.size(); k++) {
    same2 += sw[k].Equals(c.FExp(c.Pairing2(pk, g, proofs[k][0], proofs[k][1]))) ? 1 : 0;
    same2 += dd[k].Equals(c.FExp(c.Pairing(g, proofs[k][0]))) ? 1 : 0;
  }
  EXPECT(same2 == 2 * (int)proofs.size());
  bool threw = false;
  try {
    std::vector<uint32_t> bad = {0, 3};
    prep.PairingBatch(proofs, &bad);
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    std::vector<uint32_t> bad = {0};
    prep.PairingBatch(proofs, &bad);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  EXPECT(prep.PairingBatch({}).empty());
  // the C entry points the mirror does not reach
  mlhip_g2_prepared* h = nullptr;
  EXPECT(mlhip_g2_prepared_create(c.id, g.raw.data(), 0, &h) == MLHIP_EINVAL && h == nullptr);
  EXPECT(mlhip_g2_prepared_create(c.id, g.raw.data(), 1, &h) == 0 && h != nullptr);
  size_t m = 0;
  EXPECT(mlhip_g2_prepared_count(h, &m) == 0 && m == 1);
  Gt one = c.new_gt();
  EXPECT(mlhip_pairing_prepared(h, g1.raw.data(), nullptr, 2, 1, one.raw.data()) == MLHIP_EINVAL);
  EXPECT(mlhip_g2_prepared_destroy(h) == 0);
  printf("%s g2_prepared %d/%d indexed %d/%d\n", kNames[c.id], same, (int)proofs.size(), same2, 2 * (int)proofs.size());
}

// argv[1 .. 4]: the G2 generator of BLS12-377 in decimal coordinates (the mirror has none built in; from the golden file)
int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: g2_prepared_test x0 x1 y0 y1\n");
    return 2;
  }
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 4242 + id;
    run(c, id == MLHIP_CURVE_BLS12_377 ? c.NewG2FromCoords(argv[1], argv[2], argv[3], argv[4]) : c.GenG2(), st);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
