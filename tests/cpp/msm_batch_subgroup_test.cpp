// tests/cpp/msm_batch_subgroup_test.cpp -- the C++ mirror's MultiScalarMulBatchSubgroup / MultiScalarMulG2BatchSubgroup
// (include/mlhip_driver.hpp) and the inline batched-MSM functions of include/mlhip_subgroup.h, compiled as C++ here and as C
// in msm_batch_subgroup_c.c, against the plain batch mirrors and single MultiScalarMul calls on multiples of the generators,
// on every curve.  Driven by tests/test_msm_batch_subgroup_cpp.py.  Needs a GPU.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "mlhip_driver.hpp"
#include "mlhip_subgroup.h"

using namespace mlhip_driver;

// include/mlhip_subgroup.h compiled as C (msm_batch_subgroup_c.c)
extern "C" int c_msm_batch_subgroup(int curve_id, int group, const void* points, const void* scalars, int scalars_mont,
                                    const uint64_t* offsets, size_t k, void* out_affine);
extern "C" int c_msm_batch_subgroup_device(int curve_id, int group, const void* d_points, const void* d_scalars, int scalars_mont,
                                           const uint64_t* offsets, size_t k, void* d_out_affine, void* stream);
extern "C" int c_curve_subgroup_points(int curve_id);

static int g_fail = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail++;                                              \
    }                                                        \
  } while (0)

static const char* kNames[3] = {"BN254", "BLS12-381", "BLS12-377"};

// segments of 3, 0, 1, 8 and 2 pairs, and one with more scalars than points (the identity): how many of the six agree with the
// plain batch mirror and (the used ones) with a single MultiScalarMul
template <class P, class Fast, class Plain, class Single>
static int run_group(const Curve& c, int group, const P& gen, uint64_t& st, Fast fast_fn, Plain plain_fn, Single single_fn) {
  std::vector<P> pts;
  for (int i = 0; i < 11; i++) pts.push_back(gen.Mul(c.NewRandomZr(st)));
  pts.push_back(gen);
  std::vector<Zr> zs;
  for (int i = 0; i < 9; i++) zs.push_back(c.NewRandomZr(st));
  zs.push_back(c.NewZrFromInt(-1));
  zs.push_back(c.GroupOrder);
  zs.push_back(c.NewZrFromInt(1));
  auto cut = [](const auto& v, size_t a, size_t b) { return std::vector<typename std::decay<decltype(v)>::type::value_type>(v.begin() + a, v.begin() + b); };
  std::vector<std::vector<P>> a = {cut(pts, 0, 3), {}, cut(pts, 3, 4), cut(pts, 4, 12), cut(pts, 0, 2), cut(pts, 5, 7)};
  std::vector<std::vector<Zr>> b = {cut(zs, 0, 3), {}, cut(zs, 3, 4), cut(zs, 4, 12), cut(zs, 0, 2), cut(zs, 5, 8)};
  std::vector<P> fast = fast_fn(a, b), plain = plain_fn(a, b);
  int same = 0;
  for (size_t i = 0; i < a.size() && i < fast.size() && i < plain.size(); i++) {
    const bool used = a[i].size() == b[i].size();
    same += (fast[i].Equals(plain[i]) && (used ? fast[i].Equals(single_fn(a[i], b[i])) : fast[i].IsInfinity())) ? 1 : 0;
  }
  EXPECT(same == (int)a.size());
  EXPECT(fast.size() == 6 && fast[1].IsInfinity() && fast[5].IsInfinity());
  // the inline header as C and as C++ on the bytes of the first five segments (one Zr is 32 bytes)
  const size_t size = gen.raw.size();
  std::vector<unsigned char> in, sc;
  std::vector<uint64_t> offsets(1, 0);
  for (size_t i = 0; i < 5; i++) {
    for (auto& p : a[i]) in.insert(in.end(), p.raw.begin(), p.raw.end());
    for (auto& z : b[i]) {
      auto l = z.abi_limbs();
      sc.insert(sc.end(), (const unsigned char*)l.data(), (const unsigned char*)l.data() + 32);
    }
    offsets.push_back(offsets.back() + a[i].size());
  }
  std::vector<unsigned char> o1(size * 5), o2(size * 5);
  const int mont = c.scalars_mont ? 1 : 0;
  EXPECT(c_msm_batch_subgroup(c.id, group, in.data(), sc.data(), mont, offsets.data(), 5, o1.data()) == 0);
  EXPECT(mlhip_msm_batch_subgroup(c.id, group, in.data(), sc.data(), mont, offsets.data(), 5, o2.data()) == 0);
  EXPECT(o1 == o2);
  for (size_t i = 0; i < 5 && i < fast.size(); i++) EXPECT(memcmp(o1.data() + i * size, fast[i].raw.data(), size) == 0);
  return same;
}

static void run(const Curve& c, const G2& g2, uint64_t& st) {
  typedef std::vector<std::vector<G1>> L1;
  typedef std::vector<std::vector<G2>> L2;
  typedef std::vector<std::vector<Zr>> LZ;
  const int s1 = run_group<G1>(
      c, MLHIP_GROUP_G1, c.GenG1(), st, [&](const L1& a, const LZ& b) { return c.MultiScalarMulBatchSubgroup(a, b); },
      [&](const L1& a, const LZ& b) { return c.MultiScalarMulBatch(a, b); },
      [&](const std::vector<G1>& a, const std::vector<Zr>& b) { return c.MultiScalarMul(a, b); });
  const int s2 = run_group<G2>(
      c, MLHIP_GROUP_G2, g2, st, [&](const L2& a, const LZ& b) { return c.MultiScalarMulG2BatchSubgroup(a, b); },
      [&](const L2& a, const LZ& b) { return c.MultiScalarMulG2Batch(a, b); },
      [&](const std::vector<G2>& a, const std::vector<Zr>& b) { return c.MultiScalarMulG2(a, b); });
  EXPECT(c.MultiScalarMulBatchSubgroup({}, {}).empty() && c.MultiScalarMulG2BatchSubgroup({}, {}).empty());
  bool threw = false;
  try {
    c.MultiScalarMulBatchSubgroup(L1(1, std::vector<G1>(2, c.GenG1())), LZ(1, std::vector<Zr>(1, c.NewZrFromInt(1))));
  } catch (const std::out_of_range&) {
    threw = true;
  }
  EXPECT(threw);
  threw = false;
  try {
    c.MultiScalarMulG2BatchSubgroup(L2(1), LZ());
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  // the macro and the argument errors of the wrappers, in both languages: k = 0 does nothing; a curve id other than 0, 1, 2
  // (a flagged one included), a bad group, malformed offsets and null pointers are errors, nothing launched
  EXPECT(c_curve_subgroup_points(0) == 0x100 && c_curve_subgroup_points(1) == 0x101 && c_curve_subgroup_points(2) == 0x102);
  EXPECT(c_curve_subgroup_points(3) == -1 && c_curve_subgroup_points(-1) == -1 && c_curve_subgroup_points(0x101) == -1);
  EXPECT(MLHIP_CURVE_SUBGROUP_POINTS(2) == 0x102 && MLHIP_CURVE_SUBGROUP_POINTS(7) == -1);
  unsigned char buf[256] = {0};
  const uint64_t one[2] = {0, 1}, bad[2] = {1, 1};
  EXPECT(c_msm_batch_subgroup(c.id, 1, nullptr, nullptr, 0, one, 0, nullptr) == 0);
  EXPECT(mlhip_msm_batch_subgroup_device(c.id, 2, nullptr, nullptr, 0, one, 0, nullptr, nullptr) == 0);
  EXPECT(c_msm_batch_subgroup(3, 1, buf, buf, 0, one, 1, buf) == MLHIP_EINVAL);
  EXPECT(mlhip_msm_batch_subgroup(MLHIP_CURVE_SUBGROUP_POINTS(c.id), 1, buf, buf, 0, one, 1, buf) == MLHIP_EINVAL);
  EXPECT(c_msm_batch_subgroup(c.id, 3, buf, buf, 0, one, 1, buf) == MLHIP_EINVAL);
  EXPECT(mlhip_msm_batch_subgroup(c.id, 1, buf, buf, 0, bad, 1, buf) == MLHIP_EINVAL);
  EXPECT(c_msm_batch_subgroup_device(c.id, 1, nullptr, nullptr, 0, one, 1, nullptr, nullptr) == MLHIP_EINVAL);
  EXPECT(mlhip_msm_batch_subgroup_device(c.id, 2, nullptr, nullptr, 0, one, 1, nullptr, nullptr) == MLHIP_EINVAL);
  for (unsigned char v : buf) EXPECT(v == 0);
  printf("%s MultiScalarMulBatchSubgroup G1 %d/6 G2 %d/6\n", kNames[c.id], s1, s2);
}

// argv[1 .. 4]: the G2 generator of BLS12-377 in decimal coordinates (the mirror has none built in; from the golden file)
int main(int argc, char** argv) {
  if (argc < 5) {
    printf("usage: msm_batch_subgroup_test x0 x1 y0 y1\n");
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
