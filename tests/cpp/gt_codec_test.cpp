// tests/cpp/gt_codec_test.cpp -- the C++ mirror's Gt.Inverse, NewGtFromBytes and the batch forms NewGtFromBytesBatch /
// GtBytesBatch / IsInSubGroupBatch / InverseBatch (include/mlhip_driver.hpp) on a handful of the cases of
// tests/gt_codec_cases.py, which tests/test_gt_codec_cpp.py writes to a text file: one line per case,
//     <curve id> <label> <status with the check> <wire, hex> <in-memory value, hex | -> <in-memory inverse, hex | ->
// Needs a GPU.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
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

struct Case {
  std::string label;
  int status;
  Bytes wire, value, inverse;  // value / inverse empty: a malformed encoding
};

static Bytes unhex(const std::string& h) {
  Bytes b;
  if (h == "-") return b;
  for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
  return b;
}

static void run(const Curve& c, const std::vector<Case>& cases) {
  std::vector<Bytes> blobs;
  for (auto& k : cases) blobs.push_back(k.wire);
  std::vector<unsigned char> st, st0;
  std::vector<Gt> checked = c.NewGtFromBytesBatch(blobs, st), plain = c.NewGtFromBytesBatch(blobs, st0, false);
  std::vector<Gt> good;
  std::vector<Bytes> good_wire, good_inv;
  std::vector<bool> good_member;
  int ok = 0;
  for (size_t i = 0; i < cases.size(); i++) {
    const Case& k = cases[i];
    const bool malformed = k.value.empty();
    bool fine = st[i] == k.status && st0[i] == (malformed ? 1 : 0);
    fine = fine && checked[i].raw == (k.status == 0 ? k.value : Bytes(c.gt_bytes, 0));
    fine = fine && plain[i].raw == (malformed ? Bytes(c.gt_bytes, 0) : k.value);
    bool threw = false;
    try {
      Gt g = c.NewGtFromBytes(k.wire);  // no subgroup check, as gnark's SetBytes
      fine = fine && g.raw == k.value && g.ToBytes() == k.wire;
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    fine = fine && threw == malformed;
    if (!malformed) {
      good.push_back(plain[i]);
      good_wire.push_back(k.wire);
      good_inv.push_back(k.inverse);
      good_member.push_back(k.status == 0);
      Gt inv = plain[i];
      inv.Inverse();
      fine = fine && inv.raw == k.inverse;
      inv.Mul(plain[i]);
      fine = fine && (k.label == "zero" ? inv.raw == Bytes(c.gt_bytes, 0) : inv.IsUnity());
    }
    if (!fine) printf("FAIL %s %s\n", kNames[c.id], k.label.c_str());
    ok += fine ? 1 : 0;
  }
  EXPECT(ok == (int)cases.size());
  EXPECT(c.GtBytesBatch(good) == good_wire);
  EXPECT(c.IsInSubGroupBatch(good) == good_member);
  std::vector<Gt> inv = c.InverseBatch(good);
  EXPECT(inv.size() == good.size());
  for (size_t i = 0; i < inv.size() && i < good.size(); i++) EXPECT(inv[i].raw == good_inv[i]);
  // empty batches, a wrong length, and the device forms with null pointers: argument errors, nothing launched
  std::vector<unsigned char> none;
  EXPECT(c.NewGtFromBytesBatch({}, none).empty() && c.GtBytesBatch({}).empty() && c.IsInSubGroupBatch({}).empty() && c.InverseBatch({}).empty());
  bool threw = false;
  try {
    c.NewGtFromBytes(Bytes(c.gt_bytes - 1, 0));
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  EXPECT(mlhip_gt_from_bytes_device(c.id, nullptr, 1, 1, nullptr, nullptr, nullptr) == MLHIP_EINVAL);
  EXPECT(mlhip_gt_to_bytes_device(c.id, nullptr, 1, nullptr, nullptr) == MLHIP_EINVAL);
  EXPECT(mlhip_gt_is_member_device(c.id, nullptr, 1, nullptr, nullptr) == MLHIP_EINVAL);
  EXPECT(mlhip_gt_inverse_device(c.id, nullptr, 1, nullptr, nullptr) == MLHIP_EINVAL);
  printf("%s gt_codec %d/%d\n", kNames[c.id], ok, (int)cases.size());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: gt_codec_test cases.txt\n");
    return 2;
  }
  std::vector<Case> cases[3];
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    int id;
    Case k;
    std::string w, v, iv;
    if (!(ls >> id >> k.label >> k.status >> w >> v >> iv) || id < 0 || id > 2) continue;
    k.wire = unhex(w);
    k.value = unhex(v);
    k.inverse = unhex(iv);
    cases[id].push_back(k);
  }
  for (int id = 0; id < 3; id++) {
    EXPECT(!cases[id].empty());
    Curve c(id);
    run(c, cases[id]);
  }
  printf(g_fail ? "RESULT FAIL %d\n" : "RESULT OK\n", g_fail);
  return g_fail ? 1 : 0;
}
