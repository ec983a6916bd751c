// api_bases.hip -- resident bases (mlhip_bases_* of include/mlhip.h): an uploaded point table with its plan, on one device
// or cut into shards over several, and the batched MSMs over it.  No kernels here.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "mlhip_rt.h"
#include "msm_body.h"

using namespace mlhip;
using namespace mlhip_rt;

struct mlhip_bases {
  mlhip_msm_plan* plan = nullptr;
  void *d_pts = nullptr, *d_sc = nullptr;
  size_t n = 0, ptsz = 0;
  int curve = 0, group = 0, device = 0;
  hipStream_t stream = nullptr;  // own non-blocking stream (see PoolEntry)
  std::mutex mu;  // one MSM at a time per handle: the plan and the scalar buffer are shared state
  mlhip_bases_batch_tables batch;  // mlhip_bases_msm_batch's per-base tables: built by the first batch call that wants them
  // a table spread over several devices: contiguous shards, shard r = bases [lo[r], lo[r + 1]) on devs[r]
  std::vector<mlhip_bases*> shards;
  std::vector<size_t> lo;
  std::vector<int> devs;
  // a SET of handles (mlhip_bases_set_create): 1 .. 4 single-device handles of one curve on one device, NOT owned; n is the
  // smallest member's count, ptsz the bytes of all results back to back.  No plan, no points, no stream of its own: a set
  // call runs on its first member's stream (host scalars) or the caller's (device scalars).
  std::vector<mlhip_bases*> members;
  int route[4] = {0, 0, 0, 0};  // how the set's last MSM ran (mlhip_bases_set_route), written under mu
};


namespace {
// Shifted-base tables for a table of n resident bases (msm_fold.h)?  They cost Wd rows per base (112 B a row for a 48-byte
// field: 1.5 GB for 2^20 BLS12-381 G1 bases) and ~60 ms per 2^20 bases to build, and pay from the first few MSMs on.
//   MLHIP_BASES_TABLES = 0: never; = 1: always (any size: what the tests use); unset: for tables of at least 2^10 bases
//   created with window_c = 0 (an explicit window width asks for that Pippenger geometry) that fit a quarter of the free memory.
//   MLHIP_FOLD_WINDOW = c: the digit width (default by size, see below); MLHIP_FOLD_TILE_LOG2 = t: tiles of 2^t bases (20).
bool bases_want_tables(int group, size_t n, int window_c, int fr_bits, size_t ptsz, int* c_out, size_t* tile_out) {
  const char* e = getenv("MLHIP_BASES_TABLES");
  const bool forced = e && e[0] == '1';
  if (e && e[0] == '0') return false;
  // (G2 was measured from 2^20 bases down to 2^17 only: its small tables stay plain)
  if (!forced && (n < ((size_t)1 << (group == MLHIP_GROUP_G1 ? 10 : 17)) || window_c != 0)) return false;
  int lg_tile = 20;
  if (const char* t = getenv("MLHIP_FOLD_TILE_LOG2")) {
    const int v = atoi(t);
    if (v >= 4 && v <= 24) lg_tile = v;
  }
  size_t tile = (size_t)1 << lg_tile;
  if (n < tile) tile = n;
  int c = 0;
  if (const char* w = getenv("MLHIP_FOLD_WINDOW")) c = atoi(w);
  // 20 bits (13 digits for a 253-255-bit group order) at every size from 2^16 on: narrower digits mean more of them and, in
  // the even digit layout, most of the 2^(c-1) buckets half-used -- same-box runs (profiles/r04_fold.txt), BLS12-381 G1,
  // resident scalars, c = 18 / 19 / 20 against the plain table: 2^17 1.11 / 0.83 / 0.80 (0.90) ms, 2^18 1.68 / 1.10 / 1.02
  // (1.19), 2^19 - / 1.61 / 1.50 (1.75), 2^20 5.15 / 3.10 / 2.75 (3.16).  Below 2^16 bases an MSM is latency, not work -- the
  // reduction's dependent chains grow with the bucket count, the accumulation's with the entries per bucket -- and what the
  // tables save is mostly the host tail's 256 doublings (0.14 ms): 13 / 14 / 16 bits from 2^10 / 2^12 / 2^13 bases:
  // 2^10 0.35 (plain 0.49) ms, 2^11 0.39 (0.52), 2^12 0.46 (0.56), 2^14 0.57 (0.67), 2^15 0.70 (0.72), 2^16 at 20 bits 0.75 (0.81)
  if (c < 5 || c > 20) c = n < ((size_t)1 << 12) ? 13 : n < ((size_t)1 << 13) ? 14 : n < ((size_t)1 << 16) ? 16 : 20;
  const size_t tiles = (n + tile - 1) / tile;
  const size_t rows = tiles * (size_t)msm_num_windows(fr_bits, c) * tile;
  if (!forced) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    // carry-free rows: at most 5/4 of the boundary form's bytes a coordinate (10 x 4 B for a 32-byte field, 14 x 4 B for a 48-byte
    // one); a G1 row may be a Niels triple (three coordinates instead of two); + one tile of boundary-form rows during the build
    const size_t row_bytes = group == MLHIP_GROUP_G1 ? ptsz / 2 * 3 * 5 / 4 : ptsz * 5 / 4;
    if (rows * row_bytes + (size_t)msm_num_windows(fr_bits, c) * tile * ptsz > free_b / 4) return false;
  }
  *c_out = c;
  *tile_out = tile;
  return true;
}

// window_c may carry MLHIP_WINDOW_DEVICE_RESULT (mlhip_bases_create / _create_device pass it on; the shards of a device
// list never have it): the handle's plan is then a device-result plan.  What is left is a plain width: a scalar-width
// packing is a width above 20.
int bases_create_single(int curve, int group, const void* points, size_t n, int window_c, size_t ptsz,
                               mlhip_bases** out, bool points_on_device = false) {
  const bool device_result = window_c > 0 && (window_c & MLHIP_WINDOW_DEVICE_RESULT);
  if (device_result) window_c &= ~MLHIP_WINDOW_DEVICE_RESULT;
  int rc = ensure_device();
  if (rc) return rc;
  mlhip_bases* b = new mlhip_bases();
  b->device = call_device();
  b->curve = curve;
  b->group = group;
  b->n = n;
  b->ptsz = ptsz;
  const CurveOps* ops = curve_ops(curve);  // (every caller has checked the id)
  {
    int fold_c = 0;
    size_t fold_tile = 0;
    if (bases_want_tables(group, n, window_c, ops->fr_bits, ptsz, &fold_c, &fold_tile)) {
      if (plan_create_ex(curve, group, n, fold_c, fold_tile, &b->plan, 0, device_result) != 0) b->plan = nullptr;  // (the plain plan below)
    }
  }
  rc = b->plan ? 0 : plan_create_ex(curve, group, n, window_c, 0, &b->plan, 0, device_result);
  if (!rc && (hipMalloc(&b->d_pts, n * b->ptsz) != hipSuccess || hipMalloc(&b->d_sc, n * 32) != hipSuccess))
    rc = mlhip_rt::fail(MLHIP_ENOMEM, "hipMalloc of the bases failed");
  if (!rc && hipMemcpy(b->d_pts, points, n * b->ptsz, points_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) != hipSuccess)
    rc = mlhip_rt::fail(MLHIP_EHIP, "upload of the bases failed");
  if (!rc && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
    rc = mlhip_rt::fail(MLHIP_EHIP, "hipStreamCreate failed");
  if (rc) {
    mlhip_bases_destroy(b);
    return rc;
  }
  b->plan->points_static = true;  // the buffer is ours and never rewritten: convert it on the first MSM only
  // BLS12-377 G1: a table whose every point is in the prime-order subgroup (what an SRS is; checked here, once, on the
  // device: on the curve and phi(P) = [-x^2]P) has its buckets summed in twisted Edwards coordinates (ed28.h)
  if (ops->g1_count_outside_subgroup && group == MLHIP_GROUP_G1) {
    const char* e = getenv("MLHIP_EDWARDS");
    if (!(e && e[0] == '0')) {
      uint32_t* d_bad = nullptr;
      uint32_t bad = 1;
      if (hipMalloc(&d_bad, 4) == hipSuccess) {
        if (hipMemsetAsync(d_bad, 0, 4, b->stream) == hipSuccess &&
            ops->g1_count_outside_subgroup(b->d_pts, n, d_bad, b->stream) == 0 &&
            hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, b->stream) == hipSuccess &&
            hipStreamSynchronize(b->stream) == hipSuccess) {
          b->plan->trust_subgroup = bad == 0;
          if (bad == 0) plan_reserve_edwards(b->plan);
        }
        (void)hipFree(d_bad);
      }
    }
  }
  if (b->plan->fold) {
    // the shifted-base table, in the form the plan will read (after the subgroup check: Niels triples or Weierstrass rows).
    // If it cannot be built (memory), the handle falls back to a plain plan over the uploaded bases.
    rc = ops->plan_fold_build(b->plan, b->d_pts, n, b->stream);
    if (!rc && hipStreamSynchronize(b->stream) != hipSuccess) rc = MLHIP_EHIP;
    if (rc) {
      (void)hipGetLastError();
      const bool trusted = b->plan->trust_subgroup;
      mlhip_msm_plan_destroy(b->plan);
      b->plan = nullptr;
      rc = plan_create_ex(curve, group, n, window_c, 0, &b->plan, 0, device_result);
      if (rc) {
        mlhip_bases_destroy(b);
        return rc;
      }
      b->plan->points_static = true;
      b->plan->trust_subgroup = trusted;
      if (trusted) plan_reserve_edwards(b->plan);
    }
  }
  *out = b;
  return 0;
}

int bases_create_on(const std::vector<int>& devs, int curve, int group, const void* points, size_t n, int window_c,
                           size_t ptsz, mlhip_bases** out) {
  mlhip_bases* b = new mlhip_bases();
  b->curve = curve;
  b->group = group;
  b->n = n;
  b->ptsz = ptsz;
  b->devs = devs;
  b->shards.assign(devs.size(), nullptr);
  b->lo.assign(devs.size() + 1, n);
  int rc = run_on_devices(devs, n, [&](size_t r, size_t lo, size_t hi) {
    b->lo[r] = lo;
    return bases_create_single(curve, group, (const char*)points + lo * ptsz, hi - lo, window_c, ptsz, &b->shards[r]);
  });
  if (rc) {
    std::string msg = mlhip_last_error();
    mlhip_bases_destroy(b);
    return mlhip_rt::fail(rc, msg);
  }
  *out = b;
  return 0;
}

// the checks of a batch over a handle that need its size: every index below n (base_index given), or every segment at most n
// pairs long (not given); *need = 1 + the largest base any pair reads (0: every segment is empty)
int check_bases_batch_index(const mlhip_bases* b, const uint32_t* base_index, const uint64_t* offsets, size_t k,
                                   size_t* need) {
  size_t most = 0;
  if (base_index) {
    for (uint64_t i = 0; i < offsets[k]; i++) {
      if (base_index[i] >= b->n) return mlhip_rt::fail(MLHIP_EINVAL, "bases msm batch: base index out of range");
      most = std::max<size_t>(most, (size_t)base_index[i] + 1);
    }
  } else {
    for (size_t s = 0; s < k; s++) {
      const uint64_t m = offsets[s + 1] - offsets[s];
      if (m > b->n) return mlhip_rt::fail(MLHIP_EINVAL, "bases msm batch: a segment is longer than the handle's bases");
      most = std::max<size_t>(most, (size_t)m);
    }
  }
  *need = most;
  return 0;
}

// mlhip_bases_msm / _msm_device on a single-device handle whose mutex the caller holds, arguments checked, n != 0
int bases_msm_locked(mlhip_bases* b, const void* scalars, int scalars_mont, size_t n, void* out_affine) {
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  {
    // after the first MSM (which leaves the converted copy of the bases) large calls stream their scalars
    const mlhip_msm_plan* p = b->plan;
    const int segments = stream_segments(p->group, n, p);
    if (segments > 1 && p->points_static && p->conv_src == b->d_pts && n <= p->conv_n) {
      int rc = plan_stream(b->plan, b->d_pts, b->d_sc, nullptr, scalars, scalars_mont, n, segments, b->stream);
      return rc ? rc : mlhip_msm_finish(b->plan, out_affine, nullptr);
    }
  }
  if (hipMemcpy(b->d_sc, scalars, n * 32, hipMemcpyHostToDevice) != hipSuccess)
    return mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy of MSM scalars failed");
  return mlhip_msm_run(b->plan, b->d_pts, b->d_sc, scalars_mont, n, b->stream, out_affine, nullptr);
}

int bases_msm_device_locked(mlhip_bases* b, const void* d_scalars, int scalars_mont, size_t n, void* stream, void* out_affine) {
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  return mlhip_msm_run(b->plan, b->d_pts, d_scalars, scalars_mont, n, stream, out_affine, nullptr);
}

bool is_set(const mlhip_bases* b) { return !b->members.empty(); }

int reject_set(const mlhip_bases* b, const char* who) {
  if (!is_set(b)) return 0;
  return mlhip_rt::fail(MLHIP_EINVAL, std::string(who) + ": the handle is a set of handles (mlhip_bases_set_create); batches run on its members");
}

SetGeometry set_geometry(const mlhip_msm_plan* p) {
  SetGeometry g;
  g.fold = p->fold;
  g.c = p->c;
  g.Wd = p->Wd;
  g.fold_tile = p->fold_tile;
  g.W = p->W;
  g.M = p->M;
  g.bits = p->bits;
  g.can_train = plan_can_train(p);
  return g;
}

// mlhip_bases_msm (d_scalars null) / mlhip_bases_msm_device (scalars null) on a set: every member's MSM over the same first n
// scalars, the affine results back to back in member order.  Every member's mutex is held, taken in address order.
//   shared route (msm_set.h: set_share): the members are put into classes of equal plan geometry; the host scalars are
//   uploaded ONCE, into the first member's scalar buffer, by the first class -- segment by segment as that member's own
//   mlhip_bases_msm would --, and the later classes read that copy (the first class's stream has waited for every segment);
//   a class of two or more members sorts every tile once (plan_train), a class of one runs its handle's own launch; the
//   classes are queued one after another on one stream and finished -- host tails -- in that order.
//   per-member route: exactly what each member's own call does, in member order.
int set_msm(mlhip_bases* set, const void* scalars, const void* d_scalars, int mont, size_t n, void* stream, void* out_affine) {
  const bool device_form = scalars == nullptr;
  const int k = (int)set->members.size();
  if (n > set->n) return mlhip_rt::fail(MLHIP_EINVAL, "more scalars than the resident bases of the set's smallest member");
  int tables = 1;
  for (mlhip_bases* m : set->members) tables &= m->plan->fold ? 1 : 0;
  if (n == 0) {
    memset(out_affine, 0, set->ptsz);
    std::lock_guard<std::mutex> lk(set->mu);
    const int r[4] = {k, 0, 0, tables};
    memcpy(set->route, r, sizeof(r));
    return 0;
  }
  if (!scalars && !d_scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (hipSetDevice(set->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  std::lock_guard<std::mutex> lk(set->mu);
  std::vector<mlhip_bases*> by_address(set->members);
  std::sort(by_address.begin(), by_address.end(), std::less<mlhip_bases*>());
  std::vector<std::unique_lock<std::mutex>> held;
  for (mlhip_bases* m : by_address) held.emplace_back(m->mu);
  size_t out_off[MLHIP_SET_MAX_MEMBERS + 1] = {0};
  for (int i = 0; i < k; i++) out_off[i + 1] = out_off[i] + set->members[i]->ptsz;
  char* out = (char*)out_affine;
  if (!set_share(n, device_form)) {
    for (int i = 0; i < k; i++) {
      mlhip_bases* m = set->members[i];
      int rc = device_form ? bases_msm_device_locked(m, d_scalars, mont, n, stream, out + out_off[i])
                           : bases_msm_locked(m, scalars, mont, n, out + out_off[i]);
      if (rc) return rc;
    }
    const int r[4] = {k, k, device_form ? 0 : k, tables};
    memcpy(set->route, r, sizeof(r));
    return 0;
  }
  SetGeometry g[MLHIP_SET_MAX_MEMBERS];
  int cls[MLHIP_SET_MAX_MEMBERS];
  for (int i = 0; i < k; i++) g[i] = set_geometry(set->members[i]->plan);
  const int n_cls = set_classes(g, k, cls);
  hipStream_t st = device_form ? (hipStream_t)stream : set->members[0]->stream;
  void* dsc = device_form ? const_cast<void*>(d_scalars) : set->members[0]->d_sc;
  bool uploaded = device_form;
  int uploads = 0, rc = 0, queued = 0;
  int order[MLHIP_SET_MAX_MEMBERS];  // the members as their launches were queued
  for (int c = 0; c < n_cls && !rc; c++) {
    mlhip_msm_plan* plans[MLHIP_SET_MAX_MEMBERS];
    void* dpts[MLHIP_SET_MAX_MEMBERS];
    int m = 0;
    for (int i = 0; i < k; i++)
      if (cls[i] == c) {
        plans[m] = set->members[i]->plan;
        dpts[m] = set->members[i]->d_pts;
        order[queued + m] = i;
        m++;
      }
    const void* hs = uploaded ? nullptr : scalars;
    mlhip_msm_plan* p = plans[0];
    if (m >= 2) {
      const int K = set_class_tiles(g[order[queued]], p->group == MLHIP_GROUP_G1, hs != nullptr, n);
      rc = plan_train(plans, dpts, m, dsc, hs, mont, n, K, st);
    } else if (hs) {
      // a class of one that brings the scalars: as its own mlhip_bases_msm (streamed once the converted copy is there)
      const int segments = stream_segments(p->group, n, p);
      if (segments > 1 && p->points_static && p->conv_src == dpts[0] && n <= p->conv_n) {
        rc = plan_stream(p, dpts[0], dsc, nullptr, hs, mont, n, segments, st);
      } else {
        if (hipMemcpy(dsc, hs, n * 32, hipMemcpyHostToDevice) != hipSuccess)
          rc = mlhip_rt::fail(MLHIP_EHIP, "hipMemcpy of MSM scalars failed");
        if (!rc) rc = mlhip_msm_launch(p, dpts[0], dsc, mont, n, st);
      }
    } else {
      rc = mlhip_msm_launch(p, dpts[0], dsc, mont, n, st);
    }
    if (hs) {
      uploads++;
      uploaded = true;
    }
    if (!rc) queued += m;
  }
  for (int q = 0; q < queued && !rc; q++) rc = mlhip_msm_finish(set->members[order[q]]->plan, out + out_off[order[q]], nullptr);
  if (rc) {  // whatever is still queued may read the caller's scalars: let it drain, and leave every member usable
    const std::string msg = mlhip_last_error();
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    for (mlhip_bases* m : set->members) m->plan->pending = false;
    return mlhip_rt::fail(rc, msg);
  }
  const int r[4] = {k, n_cls, uploads, tables};
  memcpy(set->route, r, sizeof(r));
  return 0;
}

// mlhip_bases_create with group = MLHIP_GROUP_SET (include/mlhip_bases_set.h: mlhip_bases_set_create); *set is null
int set_create(mlhip_bases* const* members, size_t k, mlhip_bases** set) {
  if (k == 0 || k > MLHIP_SET_MAX_MEMBERS) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: a set has 1 .. 4 members");
  if (!members) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: null member list");
  for (size_t i = 0; i < k; i++) {
    if (!members[i]) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: null member");
    for (size_t j = 0; j < i; j++)
      if (members[j] == members[i]) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: a handle is listed twice");
  }
  size_t n = 0, ptsz = 0;
  for (size_t i = 0; i < k; i++) {
    const mlhip_bases* m = members[i];
    if (is_set(m)) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: a set cannot be a member of a set");
    if (!m->shards.empty()) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: a member is spread over several devices");
    if (!m->plan || m->plan->device_result)
      return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: a device-result handle cannot be a member (its result stays in device memory)");
    if (m->curve != members[0]->curve) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: the members are of different curves");
    if (m->device != members[0]->device) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_create: the members live on different devices");
    n = i == 0 ? m->n : std::min(n, m->n);
    ptsz += m->ptsz;
  }
  mlhip_bases* b = new mlhip_bases();
  b->members.assign(members, members + k);
  b->curve = members[0]->curve;
  b->device = members[0]->device;
  b->n = n;
  b->ptsz = ptsz;
  *set = b;
  return 0;
}

// mlhip_bases_msm with scalars = NULL and scalars_mont = MLHIP_MSM_SET_ROUTE (mlhip_bases_set_route): entries written
int set_route(mlhip_bases* set, int* info, size_t cap) {
  if (!is_set(set)) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_set_route: the handle is not a set (mlhip_bases_set_create)");
  std::lock_guard<std::mutex> lk(set->mu);
  const int m = (int)std::min<size_t>(cap, 4);
  for (int i = 0; i < m; i++) info[i] = set->route[i];
  return m;
}

}  // namespace

extern "C" {

int mlhip_bases_destroy(mlhip_bases* b) {
  if (!b) return 0;
  if (is_set(b)) {  // the members are not owned
    delete b;
    return 0;
  }
  for (mlhip_bases* sh : b->shards) mlhip_bases_destroy(sh);
  if (b->shards.empty()) {
    (void)hipSetDevice(b->device);
    if (b->d_pts) (void)hipFree(b->d_pts);
    if (b->d_sc) (void)hipFree(b->d_sc);
    if (b->batch.buf) (void)hipFree(b->batch.buf);
    if (b->plan) mlhip_msm_plan_destroy(b->plan);
    if (b->stream) (void)hipStreamDestroy(b->stream);
  }
  delete b;
  return 0;
}

int mlhip_bases_create(int curve, int group, const void* points, size_t n, int window_c, mlhip_bases** out) {
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  *out = nullptr;
  if (group == MLHIP_GROUP_SET) return set_create((mlhip_bases* const*)points, n, out);  // (curve and window_c: the members')
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (!points || n == 0) return mlhip_rt::fail(MLHIP_EINVAL, "bases need at least one point");
  // (a device-result handle stays on the calling thread's device: its result is a pointer on that device)
  const bool device_result = window_c > 0 && (window_c & MLHIP_WINDOW_DEVICE_RESULT);
  if (!device_result) {
    const std::vector<int> devs = spread_devices(n, false);
    if (!devs.empty()) return bases_create_on(devs, curve, group, points, n, window_c, ptsz, out);
  }
  return bases_create_single(curve, group, points, n, window_c, ptsz, out);
}

int mlhip_bases_create_device(int curve, int group, const void* d_points, size_t n, int window_c, mlhip_bases** out) {
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  *out = nullptr;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (!d_points || n == 0) return mlhip_rt::fail(MLHIP_EINVAL, "bases need at least one point");
  return bases_create_single(curve, group, d_points, n, window_c, ptsz, out, true);
}

int mlhip_bases_create_multi(int curve, int group, const int* devices, int n_devices, const void* points, size_t n,
                             int window_c, mlhip_bases** out) {
  if (!out) return mlhip_rt::fail(MLHIP_EINVAL, "null output pointer");
  *out = nullptr;
  const CurveOps* ops = curve_ops(curve);
  if (!ops) return mlhip_rt::fail(MLHIP_EINVAL, "unknown curve id");
  const size_t ptsz = ops->point_size(group);
  if (!ptsz) return mlhip_rt::fail(MLHIP_EINVAL, "group must be 1 (G1) or 2 (G2)");
  if (!points || n == 0) return mlhip_rt::fail(MLHIP_EINVAL, "bases need at least one point");
  if (window_c > 0 && (window_c & MLHIP_WINDOW_DEVICE_RESULT))
    return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_create_multi: MLHIP_WINDOW_DEVICE_RESULT is for handles on one device");
  if (n_devices < 1 || n_devices > 64 || !devices) return mlhip_rt::fail(MLHIP_EINVAL, "device list: 1 .. 64 entries");
  std::vector<int> devs(devices, devices + n_devices);
  for (int d : devs)
    if (d < 0 || d >= MLHIP_MAX_DEVICES) return mlhip_rt::fail(MLHIP_EINVAL, "device list: index out of range (0 .. 63)");
  if (devs.size() > n) devs.resize(n);
  return bases_create_on(devs, curve, group, points, n, window_c, ptsz, out);
}

int mlhip_bases_checked_subgroup(mlhip_bases* b) {
  if (!b) return 0;
  if (is_set(b)) {
    for (mlhip_bases* m : b->members)
      if (!mlhip_bases_checked_subgroup(m)) return 0;
    return 1;
  }
  if (!b->shards.empty()) {
    for (mlhip_bases* s : b->shards)
      if (!s || !mlhip_bases_checked_subgroup(s)) return 0;
    return 1;
  }
  return b->plan && b->plan->trust_subgroup ? 1 : 0;
}

int mlhip_bases_msm(mlhip_bases* b, const void* scalars, int scalars_mont, size_t n, void* out_affine) {
  if (!b || !out_affine) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (!scalars && scalars_mont == MLHIP_MSM_SET_ROUTE) return set_route(b, (int*)out_affine, n);
  if (is_set(b)) {
    if (n && !scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
    return set_msm(b, scalars, nullptr, scalars_mont, n, nullptr, out_affine);
  }
  if (b->plan && b->plan->device_result)
    return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_msm: a device-result handle leaves its result in device memory; use mlhip_bases_msm_device");
  if (n > b->n) return mlhip_rt::fail(MLHIP_EINVAL, "more scalars than resident bases");
  if (n == 0) {
    memset(out_affine, 0, b->ptsz);
    return 0;
  }
  if (!scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (!b->shards.empty()) {
    // every device adds up its part of the first n bases; the partial sums meet on the host (see msm_multi)
    const size_t D = b->shards.size();
    std::vector<char> partial(D * b->ptsz, 0);
    int rc = run_on_devices(b->devs, D, [&](size_t r, size_t, size_t) {
      const size_t lo = b->lo[r], hi = std::min(b->lo[r + 1], n);
      if (lo >= hi) return 0;  // this shard's bases lie beyond the call's scalars: identity
      return mlhip_bases_msm(b->shards[r], (const char*)scalars + lo * 32, scalars_mont, hi - lo, &partial[r * b->ptsz]);
    });
    if (rc) return rc;
    return host_group_sum(b->curve, b->group, partial.data(), D, out_affine);
  }
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  std::lock_guard<std::mutex> lk(b->mu);
  return bases_msm_locked(b, scalars, scalars_mont, n, out_affine);
}

int mlhip_bases_msm_device(mlhip_bases* b, const void* d_scalars, int scalars_mont, size_t n, void* stream, void* out_affine) {
  if (!b || !out_affine) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (is_set(b)) {
    if (n && !d_scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
    return set_msm(b, nullptr, d_scalars, scalars_mont, n, stream, out_affine);
  }
  if (!b->shards.empty()) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_msm_device: the handle is spread over several devices");
  if (n > b->n) return mlhip_rt::fail(MLHIP_EINVAL, "more scalars than resident bases");
  // (a device-result handle: out_affine is a device pointer, written in stream order -- the all-zero point too -- and the
  // call returns once everything is queued: the mutex covers the enqueue only)
  const bool device_result = b->plan->device_result;
  if (n == 0 && !device_result) {
    memset(out_affine, 0, b->ptsz);
    return 0;
  }
  if (n && !d_scalars) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  std::lock_guard<std::mutex> lk(b->mu);
  return mlhip_msm_run(b->plan, b->d_pts, d_scalars, scalars_mont, n, stream, out_affine, nullptr);
}

int mlhip_bases_msm_batch_device(mlhip_bases* b, const void* d_scalars, int scalars_mont, const uint32_t* base_index,
                                 const uint64_t* offsets, size_t k, void* stream, void* d_out_affine) {
  if (!b) return mlhip_rt::fail(MLHIP_EINVAL, "null handle");
  if (int rc_set = reject_set(b, "mlhip_bases_msm_batch")) return rc_set;
  bool unit = false;
  int rc = take_unit_scalars(scalars_mont, d_scalars, &unit);
  if (rc) return rc;
  rc = check_batch_offsets(offsets, k);
  if (rc) return rc;
  if (k == 0) return 0;
  if (!b->shards.empty()) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_msm_batch: the handle is spread over several devices");
  size_t need = 0;
  rc = check_bases_batch_index(b, base_index, offsets, k, &need);
  if (rc) return rc;
  if (!d_out_affine || (offsets[k] && !d_scalars && !unit)) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  std::lock_guard<std::mutex> lk(b->mu);
  // plain sums (msm_sum_batch.h) read the handle's points only: the batch tables are neither built nor read
  if (unit) return curve_ops(b->curve)->sum_batch(b->group, b->d_pts, true, base_index, offsets, k, d_out_affine, (hipStream_t)stream);
  return curve_ops(b->curve)->bases_batch(b->group, &b->batch, b->d_pts, b->n, d_scalars, scalars_mont, base_index, offsets, k, need,
                                          d_out_affine, (hipStream_t)stream);
}

int mlhip_bases_msm_batch(mlhip_bases* b, const void* scalars, int scalars_mont, const uint32_t* base_index, const uint64_t* offsets,
                          size_t k, void* out_affine) {
  if (!b) return mlhip_rt::fail(MLHIP_EINVAL, "null handle");
  if (int rc_set = reject_set(b, "mlhip_bases_msm_batch")) return rc_set;
  bool unit = false;
  int rc = take_unit_scalars(scalars_mont, scalars, &unit);
  if (rc) return rc;
  rc = check_batch_offsets(offsets, k);
  if (rc) return rc;
  if (k == 0) return 0;
  if (!b->shards.empty()) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_msm_batch: the handle is spread over several devices");
  size_t need = 0;
  rc = check_bases_batch_index(b, base_index, offsets, k, &need);
  if (rc) return rc;
  const size_t n = offsets[k];
  if (!out_affine || (n && !scalars && !unit)) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  // the call's scratch comes from the process's device (HostCall); a handle made there before a later mlhip_init moved it
  // elsewhere has to be driven through the device form
  if (b->device != call_device()) return mlhip_rt::fail(MLHIP_EINVAL, "mlhip_bases_msm_batch: the handle lives on another device");
  if (hipSetDevice(b->device) != hipSuccess) return mlhip_rt::fail(MLHIP_EHIP, "hipSetDevice failed");
  HostCall hc;
  hc.reserve((unit ? 0 : n * 32) + k * b->ptsz);
  void* ds = unit ? nullptr : hc.up(scalars, n * 32);
  void* dout = hc.dev(k * b->ptsz);
  if (hc.rc) return hc.rc;
  rc = mlhip_bases_msm_batch_device(b, ds, scalars_mont, base_index, offsets, k, hc.l.st, dout);
  if (rc) return rc;
  return hc.down(out_affine, dout, k * b->ptsz);
}

int mlhip_bases_batch_tabled(mlhip_bases* b, size_t* n_tabled) {
  if (!b || !n_tabled) return mlhip_rt::fail(MLHIP_EINVAL, "null pointer");
  if (int rc_set = reject_set(b, "mlhip_bases_batch_tabled")) return rc_set;
  if (!b->shards.empty()) {
    *n_tabled = 0;
    return 0;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  *n_tabled = b->batch.n_tabled;
  return 0;
}

mlhip_msm_plan* mlhip_bases_plan(mlhip_bases* b) { return b && b->shards.empty() ? b->plan : nullptr; }

}  // extern "C"
