// tests/cpp/msm_bits_test.cpp -- the C++ mirror's short-scalar MSM (include/mlhip_driver.hpp: MultiScalarMulShort,
// MultiScalarMulG2Short) on every curve: against golden bytes the Python side computes with the oracle over the masked
// scalars (argv: bits, then one hex G1 point per curve), against the full-width calls when the scalars keep the promise,
// and with MultiScalarMul's length rules.  Driven by tests/test_msm_bits_cpp.py.  Needs a GPU.
#include <cstdio>
#include <cstdlib>
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
constexpr int N = 48, K0 = 12345, K1 = 77;

// scalar i of the shared vector: four 64-bit limbs from one multiplicative generator (the Python side runs the same one);
// the top limb is cleared so that every value is below every curve's r and needs no reduction
static void limbs_of(int i, uint64_t l[4]) {
  uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
  for (int k = 0; k < 4; k++) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    l[k] = x;
  }
  l[3] &= 0x0FFFFFFFFFFFFFFFull;
  if (i == 0) l[0] = l[1] = l[2] = l[3] = 0;
}

static std::string hex(const Bytes& b) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint8_t v : b) {
    s.push_back(d[v >> 4]);
    s.push_back(d[v & 15]);
  }
  return s;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: msm_bits_test <bits> <hex BN254> <hex BLS12-381> <hex BLS12-377>\n");
    return 2;
  }
  const int bits = atoi(argv[1]);
  for (int id = 0; id < 3; id++) {
    Curve c(id);
    const G1 g = c.GenG1();
    std::vector<G1> pts;
    std::vector<Zr> wide, kept;
    for (int i = 0; i < N; i++) {
      pts.push_back(g.Mul(c.NewZrFromInt(K0 + (int64_t)i * K1)));
      uint64_t l[4];
      limbs_of(i, l);
      wide.push_back(c.NewZrFromLimbs(l));  // breaks the promise: comes out masked
      uint64_t low[4] = {l[0], bits > 64 ? l[1] & ((bits >= 128 ? ~0ull : (1ull << (bits - 64)) - 1)) : 0, 0, 0};
      if (bits < 64) low[0] &= (1ull << bits) - 1;
      kept.push_back(c.NewZrFromLimbs(low));  // the same value masked by hand: keeps it
    }
    const G1 got = c.MultiScalarMulShort(pts, wide, bits);
    const bool golden = hex(got.raw) == argv[2 + id];
    EXPECT(golden);
    EXPECT(got.Equals(c.MultiScalarMul(pts, kept)));
    EXPECT(c.MultiScalarMulShort(pts, kept, bits).Equals(got));
    EXPECT(c.MultiScalarMulShort(pts, wide, 0).Equals(c.MultiScalarMul(pts, wide)));
    EXPECT(c.MultiScalarMulShort({}, {}, bits).IsInfinity());
    EXPECT(c.MultiScalarMulShort({pts[0]}, {wide[0], wide[1]}, bits).IsInfinity());
    bool threw = false;
    try {
      c.MultiScalarMulShort(pts, {wide[0]}, bits);
    } catch (const std::out_of_range&) {
      threw = true;
    }
    EXPECT(threw);
    bool g2ok = true;
    if (id != MLHIP_CURVE_BLS12_377) {  // (no built-in G2 generator for BLS12-377)
      const G2 h = c.GenG2();
      std::vector<G2> q;
      for (int i = 0; i < 9; i++) q.push_back(h.Mul(c.NewZrFromInt(3 + i)));
      std::vector<Zr> w9(wide.begin() + 1, wide.begin() + 10), k9(kept.begin() + 1, kept.begin() + 10);
      g2ok = c.MultiScalarMulG2Short(q, w9, bits).Equals(c.MultiScalarMulG2(q, k9)) && c.MultiScalarMulG2Short({}, {}, bits).IsInfinity();
      EXPECT(g2ok);
    }
    // the plan functions of include/mlhip_bits.h: the width round-trips, a bad width leaves the pointer null
    mlhip_msm_plan* plan = nullptr;
    int width = -1;
    EXPECT(mlhip_msm_plan_create_bits(id, MLHIP_GROUP_G1, 1000, 13, bits, &plan) == 0 && plan != nullptr);
    EXPECT(mlhip_msm_plan_scalar_bits(plan, &width) == 0 && width == bits);
    EXPECT(mlhip_msm_plan_destroy(plan) == 0);
    plan = reinterpret_cast<mlhip_msm_plan*>(&width);
    EXPECT(mlhip_msm_plan_create_bits(id, MLHIP_GROUP_G1, 1000, 13, 257, &plan) == MLHIP_EINVAL && plan == nullptr);
    EXPECT(mlhip_msm_plan_create(id, MLHIP_GROUP_G1, 1000, 13, &plan) == 0);
    EXPECT(mlhip_msm_plan_scalar_bits(plan, &width) == 0 && width > 250);  // full width: the curve's fr_bits
    EXPECT(mlhip_msm_plan_destroy(plan) == 0);
    printf("%s short_g1 golden %d g2 %d\n", kNames[id], golden ? 1 : 0, g2ok ? 1 : 0);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
