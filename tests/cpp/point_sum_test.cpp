// tests/cpp/point_sum_test.cpp -- the C++ mirror's SumG1 / SumG2 (include/mlhip_driver.hpp) on every curve: the device
// route (MLHIP_SUM_DEVICE_MIN=1) against the host route (=0), against Add in a loop and against MultiScalarMul with unit
// scalars, on a list that holds a point at infinity, a repeated point and (G1) a point next to its negative.
// Driven by tests/test_point_sum_gpu.py.  Needs a GPU.
#include <cstdio>
#include <cstdlib>
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

template <class P, class SumFn, class MsmFn>
static int run(const Curve& c, std::vector<P> pts, const P& identity, SumFn sum, MsmFn msm) {
  P loop = identity;
  for (const P& p : pts) loop.Add(p);
  setenv("MLHIP_SUM_DEVICE_MIN", "1", 1);
  const P dev = sum(pts);
  const P dev1 = sum(std::vector<P>(pts.begin(), pts.begin() + 1));
  setenv("MLHIP_SUM_DEVICE_MIN", "0", 1);
  const P host = sum(pts);
  unsetenv("MLHIP_SUM_DEVICE_MIN");
  const P dflt = sum(pts);
  std::vector<Zr> ones(pts.size(), c.NewZrFromInt(1));
  int ok = 0;
  ok += dev.Equals(host) ? 1 : 0;
  ok += dev.Equals(loop) ? 1 : 0;
  ok += dev.Equals(msm(pts, ones)) ? 1 : 0;
  ok += dflt.Equals(host) ? 1 : 0;
  ok += dev1.Equals(pts[0]) ? 1 : 0;
  ok += sum(std::vector<P>()).IsInfinity() ? 1 : 0;
  EXPECT(ok == 6);
  EXPECT(!dev.IsInfinity());
  return ok;
}

int main(int argc, char** argv) {
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    uint64_t st = 4242 + id;
    const G1 g = c.GenG1();
    std::vector<G1> p1;
    for (int i = 0; i < 100; i++) p1.push_back(g.Mul(c.NewRandomZr(st)));
    p1[3] = c.NewG1();
    p1[40] = p1[7];
    p1[41] = p1[8];
    p1[41].Neg();
    const int ok1 = run<G1>(
        c, p1, c.NewG1(), [&](const std::vector<G1>& v) { return c.SumG1(v); },
        [&](const std::vector<G1>& v, const std::vector<Zr>& s) { return c.MultiScalarMul(v, s); });
    printf("%s sum_g1 %d/6\n", kNames[id], ok1);
    if (id == MLHIP_CURVE_BLS12_377 && argc <= 4) continue;
    // the G2 generator of BLS12-377 comes from the golden file (decimal coordinates)
    const G2 h = id == MLHIP_CURVE_BLS12_377 ? c.NewG2FromCoords(argv[1], argv[2], argv[3], argv[4]) : c.GenG2();
    std::vector<G2> p2;
    for (int i = 0; i < 70; i++) p2.push_back(h.Mul(c.NewRandomZr(st)));
    p2[0] = c.NewG2();
    p2[69] = p2[5];
    const int ok2 = run<G2>(
        c, p2, c.NewG2(), [&](const std::vector<G2>& v) { return c.SumG2(v); },
        [&](const std::vector<G2>& v, const std::vector<Zr>& s) { return c.MultiScalarMulG2(v, s); });
    printf("%s sum_g2 %d/6\n", kNames[id], ok2);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
