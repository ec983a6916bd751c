// tests/cpp/scalar_mul_subgroup_test.cpp -- the C++ mirror's MulBatchSubgroup (include/mlhip_driver.hpp) and the inline
// functions of include/mlhip_subgroup.h, compiled as C++ here and as C in scalar_mul_subgroup_c.c, against G1.Mul / G2.Mul and
// MulBatch on generators and their multiples, on every curve.  Driven by tests/test_scalar_mul_subgroup_cpp.py.  Needs a GPU.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "mlhip_driver.hpp"

using namespace mlhip_driver;

// include/mlhip_subgroup.h compiled as C (scalar_mul_subgroup_c.c)
extern "C" int c_scalar_mul_subgroup(int curve_id, int group, const void* points, size_t point_stride, const void* scalars,
                                     int scalars_mont, size_t n, void* out_affine);
extern "C" int c_scalar_mul_subgroup_device(int curve_id, int group, const void* d_points, size_t point_stride,
                                            const void* d_scalars, int scalars_mont, size_t n, void* d_out_affine, void* stream);
extern "C" int c_group_subgroup(int group);

static int g_fail = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail++;                                              \
    }                                                        \
  } while (0)

static const char* kNames[3] = {"BN254", "BLS12-381", "BLS12-377"};

template <class P>
static int run_group(const Curve& c, int group, const P& gen, uint64_t& st) {
  std::vector<P> pts = {gen, gen.Mul(c.NewRandomZr(st)), gen.Mul(c.NewZrFromInt(3)), gen, gen.Mul(c.NewRandomZr(st))};
  std::vector<Zr> zs = {c.NewRandomZr(st), c.NewRandomZr(st), c.NewZrFromInt(-1), c.GroupOrder, c.NewZrFromInt(1)};
  std::vector<P> fast = c.MulBatchSubgroup(pts, zs), plain = c.MulBatch(pts, zs);
  int same = 0;
  for (size_t i = 0; i < pts.size() && i < fast.size() && i < plain.size(); i++)
    same += (fast[i].Equals(plain[i]) && fast[i].Equals(pts[i].Mul(zs[i]))) ? 1 : 0;
  EXPECT(same == (int)pts.size());
  EXPECT(fast.size() == 5 && fast[3].IsInfinity() && fast[4].Equals(pts[4]));
  // the inline header as C and as C++ on the same bytes (scalars as the mirror packs them: one Zr is 32 bytes)
  const size_t size = gen.raw.size();
  std::vector<unsigned char> in, sc(32 * pts.size()), o1(size * pts.size()), o2(size * pts.size());
  for (auto& p : pts) in.insert(in.end(), p.raw.begin(), p.raw.end());
  for (size_t i = 0; i < zs.size(); i++) memcpy(sc.data() + 32 * i, zs[i].v.data(), 32);
  EXPECT(c_scalar_mul_subgroup(c.id, group, in.data(), 1, sc.data(), 0, pts.size(), o1.data()) == 0);
  EXPECT(mlhip_scalar_mul_subgroup(c.id, group, in.data(), 1, sc.data(), 0, pts.size(), o2.data()) == 0);
  EXPECT(o1 == o2);
  for (size_t i = 0; i < fast.size(); i++) EXPECT(memcmp(o1.data() + i * size, fast[i].raw.data(), size) == 0);
  return same;
}

static void run(const Curve& c, const G2& g2, uint64_t& st) {
  const int s1 = run_group<G1>(c, MLHIP_GROUP_G1, c.GenG1(), st);
  const int s2 = run_group<G2>(c, MLHIP_GROUP_G2, g2, st);
  EXPECT(c.MulBatchSubgroup(std::vector<G1>(), {}).empty() && c.MulBatchSubgroup(std::vector<G2>(), {}).empty());
  bool threw = false;
  try {
    c.MulBatchSubgroup(std::vector<G1>(1, c.GenG1()), {});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  // argument errors of the wrappers, in both languages: n = 0 does nothing; a group other than 1 or 2 and null pointers are
  // errors, nothing launched
  EXPECT(c_group_subgroup(1) == 0x101 && c_group_subgroup(2) == 0x102 && c_group_subgroup(3) == -1 && c_group_subgroup(0x101) == -1);
  EXPECT(MLHIP_GROUP_SUBGROUP(1) == 0x101 && MLHIP_GROUP_SUBGROUP(2) == 0x102 && MLHIP_GROUP_SUBGROUP(0) == -1);
  unsigned char buf[256] = {0};
  EXPECT(c_scalar_mul_subgroup(c.id, 1, nullptr, 1, nullptr, 0, 0, nullptr) == 0);
  EXPECT(mlhip_scalar_mul_subgroup_device(c.id, 2, nullptr, 1, nullptr, 0, 0, nullptr, nullptr) == 0);
  EXPECT(c_scalar_mul_subgroup(c.id, 3, buf, 1, buf, 0, 1, buf) == MLHIP_EINVAL);
  EXPECT(mlhip_scalar_mul_subgroup(c.id, 0x101, buf, 1, buf, 0, 1, buf) == MLHIP_EINVAL);
  EXPECT(c_scalar_mul_subgroup_device(c.id, 1, nullptr, 1, nullptr, 0, 1, nullptr, nullptr) == MLHIP_EINVAL);
  EXPECT(mlhip_scalar_mul_subgroup_device(c.id, 2, nullptr, 1, nullptr, 0, 1, nullptr, nullptr) == MLHIP_EINVAL);
  printf("%s MulBatchSubgroup G1 %d/5 G2 %d/5\n", kNames[c.id], s1, s2);
}

// argv[1 .. 4]: the G2 generator of BLS12-377 in decimal coordinates (the mirror has none built in; from the golden file)
int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: scalar_mul_subgroup_test x0 x1 y0 y1\n");
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
