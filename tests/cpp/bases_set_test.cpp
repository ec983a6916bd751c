// tests/cpp/bases_set_test.cpp -- the C++ mirror's sets of resident bases (include/mlhip_driver.hpp: BasesG2, BasesSet) against
// the MSMs they share, and include/mlhip_bases_set.h through its C build (tests/cpp/bases_set_c.c).  Driven by
// tests/test_bases_set_cpp.py.  Needs a GPU.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "mlhip_driver.hpp"

using namespace mlhip_driver;

extern "C" {
int c_bases_set_create(mlhip_bases* const* members, size_t k, mlhip_bases** set);
int c_bases_set_route(mlhip_bases* set, int* info, int cap);
int c_group_set(void);
int c_msm_set_route(void);
}

static int g_fail = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                \
      g_fail++;                                                             \
    }                                                                       \
  } while (0)

static const char* kNames[3] = {"BN254", "BLS12-381", "BLS12-377"};

static void run(const Curve& c, uint64_t& st) {
  const G1 g = c.GenG1();
  const G2 h = c.GenG2();
  const size_t n = 24;
  std::vector<G1> p1, q1;
  std::vector<G2> p2;
  std::vector<Zr> zr;
  for (size_t i = 0; i < n; i++) {
    p1.push_back(g.Mul(c.NewRandomZr(st)));
    q1.push_back(g.Mul(c.NewRandomZr(st)));
    p2.push_back(h.Mul(c.NewRandomZr(st)));
    zr.push_back(c.NewRandomZr(st));
  }
  p1[3] = c.NewG1();  // bases at infinity
  p2[5] = c.NewG2();
  Bases a(c, p1), b1(c, q1);
  BasesG2 b2(c, p2);
  int same = 0;
  {
    BasesSet set(c);
    set.Add(a).Add(b2).Add(b1);
    BasesSet::Result r = set.MultiScalarMul(zr);
    EXPECT(r.g1.size() == 2 && r.g2.size() == 1);
    if (r.g1.size() == 2 && r.g2.size() == 1) {
      same += r.g1[0].Equals(c.MultiScalarMul(p1, zr)) ? 1 : 0;
      same += r.g1[1].Equals(c.MultiScalarMul(q1, zr)) ? 1 : 0;
      same += r.g2[0].Equals(c.MultiScalarMulG2(p2, zr)) ? 1 : 0;
      same += r.g1[0].Equals(a.MultiScalarMul(zr)) && r.g2[0].Equals(b2.MultiScalarMul(zr)) ? 1 : 0;
    }
    std::vector<int> route = set.Route();
    EXPECT(route.size() == 4 && route[0] == 3 && route[1] >= 1 && route[1] <= 3 && route[2] >= 1 && route[2] <= 3);
    // a prefix, and no scalars at all
    std::vector<Zr> few(zr.begin(), zr.begin() + 7);
    BasesSet::Result f = set.MultiScalarMul(few);
    same += f.g1.size() == 2 && f.g1[1].Equals(b1.MultiScalarMul(few)) ? 1 : 0;
    BasesSet::Result none = set.MultiScalarMul({});
    EXPECT(none.g1.size() == 2 && none.g2.size() == 1 && none.g1[0].IsInfinity() && none.g2[0].IsInfinity());
    bool threw = false;
    try {
      std::vector<Zr> many(zr);
      many.push_back(zr[0]);
      set.MultiScalarMul(many);
    } catch (const std::out_of_range&) {
      threw = true;
    }
    EXPECT(threw);
  }
  // the members outlive the set and still work
  same += a.MultiScalarMul(zr).Equals(c.MultiScalarMul(p1, zr)) ? 1 : 0;
  printf("%s BasesSet %d/6\n", kNames[c.id], same);
  EXPECT(same == 6);
}

int main() {
  uint64_t st = 0x5EED5E7;
  EXPECT(c_group_set() == 0x200 && c_msm_set_route() == 0x100);
  // the inline header as C: the argument rules that need no handle
  mlhip_bases* s = (mlhip_bases*)1;
  mlhip_bases* none[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  EXPECT(c_bases_set_create(none, 0, &s) == MLHIP_EINVAL && s == nullptr);
  EXPECT(c_bases_set_create(none, 5, &s) == MLHIP_EINVAL);
  EXPECT(c_bases_set_create(none, 2, &s) == MLHIP_EINVAL);
  EXPECT(mlhip_bases_set_create(none, 2, nullptr) == MLHIP_EINVAL);
  int info[4] = {0, 0, 0, 0};
  EXPECT(c_bases_set_route(nullptr, info, 4) == MLHIP_EINVAL && mlhip_bases_set_route(nullptr, info, -1) == MLHIP_EINVAL);
  try {
    for (int id : {MLHIP_CURVE_BN254, MLHIP_CURVE_BLS12_381}) {  // (the mirror has no built-in BLS12-377 G2 generator)
      Curve c(id);
      run(c, st);
    }
  } catch (const std::exception& e) {
    printf("FAIL exception: %s\n", e.what());
    g_fail++;
  }
  printf(g_fail ? "RESULT FAIL\n" : "RESULT OK\n");
  return g_fail ? 1 : 0;
}
