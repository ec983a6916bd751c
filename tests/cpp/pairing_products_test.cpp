// tests/cpp/pairing_products_test.cpp -- the C++ mirror's products of any length (include/mlhip_driver.hpp:
// Curve::MillerLoopProducts / PairingProducts, G2Prepared::MillerLoopBatch / PairingBatch with more than four pairs) on every
// curve: against the product of single pairings, against PairingProduct, with pairs at infinity, and the inline functions of
// include/mlhip_products.h on raw buffers.  Driven by tests/test_pairing_products_cpp.py.  Needs a GPU.
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

static void run(const Curve& c, const G2& g2gen, uint64_t& st) {
  const G1 g1gen = c.GenG1();
  const int K = 3, M = 7;  // 4 + 3 at four pairs a group, seven groups at one
  std::vector<std::vector<G1>> p(K);
  std::vector<std::vector<G2>> q(K);
  for (int k = 0; k < K; k++)
    for (int j = 0; j < M; j++) {
      p[k].push_back(g1gen.Mul(c.NewRandomZr(st)));
      q[k].push_back(g2gen.Mul(c.NewRandomZr(st)));
    }
  p[1][2] = c.NewG1();  // a G1 at infinity
  q[1][5] = c.NewG2();  // a G2 at infinity
  for (int j = 0; j < M; j++) p[2][j] = c.NewG1();  // a product of infinities only
  const std::vector<Gt> fused = c.PairingProducts(q, p), raw = c.MillerLoopProducts(q, p);
  EXPECT(fused.size() == (size_t)K && raw.size() == (size_t)K);
  int same = 0;
  for (int k = 0; k < K && (size_t)k < fused.size() && (size_t)k < raw.size(); k++) {
    const Gt want = c.PairingProduct(q[k], p[k]);  // one product, one final exponentiation
    same += (fused[k].Equals(want) && c.FExp(raw[k]).Equals(want)) ? 1 : 0;
  }
  EXPECT(same == K);
  Gt one = c.FExp(c.Pairing(c.NewG2(), g1gen));
  EXPECT(fused.size() == (size_t)K && fused[2].Equals(one));
  EXPECT(c.MillerLoopProducts({}, {}).empty() && c.PairingProducts({}, {}).empty());
  bool threw = false;
  try {
    c.MillerLoopProducts({q[0]}, {p[0], p[1]});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    std::vector<G1> shorter(p[1].begin(), p[1].begin() + 5);
    c.MillerLoopProducts({q[0], q[1]}, {p[0], shorter});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  // prepared: three points, seven pairs per product through an index with repeats
  G2Prepared prep(c, {q[0][0], q[0][1], q[0][2]});
  const std::vector<uint32_t> index = {2, 0, 1, 1, 0, 2, 2};
  std::vector<std::vector<G2>> expanded(K);
  for (int k = 0; k < K; k++)
    for (uint32_t x : index) expanded[k].push_back(q[0][x]);
  const std::vector<Gt> want = c.PairingProducts(expanded, p);
  const std::vector<Gt> pf = prep.PairingBatch(p, &index), pr = prep.MillerLoopBatch(p, &index);
  int same2 = 0;
  for (int k = 0; k < K && (size_t)k < pf.size() && (size_t)k < pr.size(); k++)
    same2 += (pf[k].Equals(want[k]) && c.FExp(pr[k]).Equals(want[k])) ? 1 : 0;
  EXPECT(same2 == K);
  threw = false;
  try {
    prep.PairingBatch(p);  // no index: seven pairs need seven prepared points
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  // the inline functions on raw buffers: a packed length of at most four is the plain call, a bad one is rejected
  Bytes b1, b2;
  for (int j = 0; j < 4; j++) {
    b1.insert(b1.end(), p[0][j].raw.begin(), p[0][j].raw.end());
    b2.insert(b2.end(), q[0][j].raw.begin(), q[0][j].raw.end());
  }
  Gt a = c.new_gt(), b = c.new_gt();
  EXPECT(mlhip_miller_loop_products(c.id, b1.data(), b2.data(), 4, 1, a.raw.data()) == 0);
  EXPECT(mlhip_miller_loop(c.id, b1.data(), b2.data(), 4, 1, b.raw.data()) == 0);
  EXPECT(a.raw == b.raw);
  EXPECT(mlhip_miller_loop_products(c.id, b1.data(), b2.data(), 0, 1, a.raw.data()) == MLHIP_EINVAL);
  EXPECT(mlhip_miller_loop_products(c.id, b1.data(), b2.data(), (size_t)1 << 32, 1, a.raw.data()) == MLHIP_EINVAL);
  EXPECT(mlhip_miller_loop(c.id, b1.data(), b2.data(), 7, 1, a.raw.data()) == MLHIP_EINVAL);
  EXPECT(a.raw == b.raw);
  printf("%s products %d/%d prepared %d/%d\n", kNames[c.id], same, K, same2, K);
}

// argv[1 .. 4]: the G2 generator of BLS12-377 in decimal coordinates (the mirror has none built in; from the golden file)
int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: pairing_products_test x0 x1 y0 y1\n");
    return 2;
  }
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 777 + id;
    run(c, id == MLHIP_CURVE_BLS12_377 ? c.NewG2FromCoords(argv[1], argv[2], argv[3], argv[4]) : c.GenG2(), st);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
