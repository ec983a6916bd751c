// tests/cpp/gt_exp_cyclo_test.cpp -- the C++ mirror's ExpBatchGt (include/mlhip_driver.hpp; mlhip_gt_exp_cyclo underneath)
// against Gt.Exp and ExpBatch on members of Gt, on every curve.  Driven by tests/test_gt_exp_cyclo_gpu.py.  Needs a GPU.
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

static void run(const Curve& c, const G2& g2, uint64_t& st) {
  const Gt gengt = c.FExp(c.Pairing(g2, c.GenG1()));
  Gt prod = gengt.Exp(c.NewRandomZr(st));
  prod.Mul(gengt);  // a product of members
  std::vector<Gt> gts = {gengt, prod, c.new_gt(), gengt, prod};
  std::vector<Zr> zs = {c.NewRandomZr(st), c.NewRandomZr(st), c.NewRandomZr(st), c.GroupOrder, c.NewZrFromInt(-1)};
  gts[2] = gengt.Exp(c.GroupOrder);  // 1
  std::vector<Gt> fast = c.ExpBatchGt(gts, zs), plain = c.ExpBatch(gts, zs);
  int same = 0;
  for (size_t i = 0; i < gts.size() && i < fast.size() && i < plain.size(); i++)
    same += (fast[i].Equals(plain[i]) && fast[i].Equals(gts[i].Exp(zs[i]))) ? 1 : 0;
  EXPECT(same == (int)gts.size());
  EXPECT(fast.size() == 5 && fast[2].IsUnity() && fast[3].IsUnity());
  Gt back = fast[4];
  back.Mul(prod);  // prod^-1 prod
  EXPECT(back.IsUnity());
  EXPECT(c.ExpBatchGt({}, {}).empty());
  bool threw = false;
  try {
    c.ExpBatchGt({gengt}, {});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  // the device form with null pointers: an argument error, nothing launched
  EXPECT(mlhip_gt_exp_cyclo_device(c.id, nullptr, nullptr, 0, 1, nullptr, nullptr) == MLHIP_EINVAL);
  printf("%s ExpBatchGt %d/%d\n", kNames[c.id], same, (int)gts.size());
}

// argv[1 .. 4]: the G2 generator of BLS12-377 in decimal coordinates (the mirror has none built in; from the golden file)
int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: gt_exp_cyclo_test x0 x1 y0 y1\n");
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
