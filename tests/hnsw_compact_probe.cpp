// hnsw_compact_probe.cpp -- test infrastructure (tests/test_gpu_hnsw_compact_kernel.py): K11c, the compaction of an HNSW
// slab and its mirror (vt_hnsw.hip: launch_hnsw_compact), launched on the caller's hand-made mirror.  Built into
// libvt_hnsw_compact_probe.so from that unit and this file alone; the product library never sees it.
//
// The entry points take and return host arrays, own their device buffers for the length of the call and return the
// hipError_t as an int.  Everything the kernel will index with is checked against the caller's sizes first, and so is
// every list entry a clamped count reaches: one that names no row of the old slab is hipErrorInvalidValue, nothing
// launched (the guard for it is there to keep a read inside the table; it is not for a test to lean on).  Every output
// buffer starts as 0xA5 bytes, so a word the launch did not write shows.
#include "vt_device.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct Dev {  // the call's device buffers and its stream, released on every way out
  std::vector<void *> bufs;
  hipStream_t stream = nullptr;
  hipError_t err = hipSuccess;
  Dev() { err = hipStreamCreate(&stream); }
  ~Dev() {
    for (void *p : bufs) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
  // `bytes` of device memory (at least 16) filled with `fill`, then the first `copy` bytes from `src` if given
  template <typename T>
  T *get(size_t bytes, int fill, const void *src = nullptr, size_t copy = 0) {
    if (err != hipSuccess) return nullptr;
    void *p = nullptr;
    const size_t room = bytes < 16 ? 16 : bytes;
    if ((err = hipMalloc(&p, room)) != hipSuccess) return nullptr;
    bufs.push_back(p);
    if ((err = hipMemset(p, fill, room)) != hipSuccess) return nullptr;
    if (src && copy && (err = hipMemcpy(p, src, copy, hipMemcpyHostToDevice)) != hipSuccess) return nullptr;
    return static_cast<T *>(p);
  }
  bool back(void *dst, const void *src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return err == hipSuccess;
  }
  bool sync() {
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    return err == hipSuccess;
  }
};

// every entry a (clamped) count reaches names a row of the old slab
bool list_in_table(const uint32_t *list, uint32_t lim, uint32_t old_rows) {
  const uint32_t cnt = std::min(list[0], lim);
  for (uint32_t k = 1; k <= cnt; ++k)
    if (list[k] >= old_rows) return false;
  return true;
}

// the plan and the old mirror agree on every size the kernels index with
bool shapes_hold(const uint32_t *adj0, const uint32_t *level, const uint32_t *upoff, const uint32_t *upper, uint32_t old_rows,
                 uint64_t old_upper, uint32_t stride, uint32_t m, uint32_t m0, const uint32_t *src, const uint32_t *new_upoff,
                 uint32_t rows, uint64_t new_upper) {
  if (stride == 0 || stride % 4 || m == 0 || m0 < m || m0 > 2048 || old_rows == 0 || old_rows >= (1u << 24) || rows > old_rows ||
      old_upper > (1u << 28) || new_upper > old_upper)
    return false;
  uint64_t at = 0;
  for (uint32_t i = 0; i < rows; ++i) {
    const uint32_t s = src[i];
    if (s >= old_rows || (i && s <= src[i - 1]) || new_upoff[i] != at) return false;
    const uint64_t words = (uint64_t)level[s] * (m + 1);
    if (level[s] > 64 || (uint64_t)upoff[s] + words > old_upper) return false;
    if (!list_in_table(adj0 + (size_t)s * (m0 + 1), m0, old_rows)) return false;
    for (uint32_t l = 0; l < level[s]; ++l)
      if (!list_in_table(upper + upoff[s] + (size_t)l * (m + 1), m, old_rows)) return false;
    at += words;
  }
  return at == new_upper;
}

}  // namespace

extern "C" {

uint32_t vthc_guards() { return vt::kHnswCompactGuards; }
uint32_t vthc_no_row() { return vt::kHnswNoRow; }

// launch_hnsw_compact over a hand-made mirror.  X[old_rows][stride], adj0[old_rows][m0 + 1], level[old_rows],
// upoff[old_rows], upper[old_upper]; src[rows] ascending, new_upoff[rows] the running sum of level * (m + 1), new_upper its
// end.  Out: outX[rows][stride], out_adj0[rows][m0 + 1], out_level[rows], out_upoff[rows], out_upper[new_upper],
// remap[old_rows], status[vthc_guards()].
int vthc_compact(const float *X, const uint32_t *adj0, const uint32_t *level, const uint32_t *upoff, const uint32_t *upper,
                 uint32_t old_rows, uint64_t old_upper, uint32_t stride, uint32_t m, uint32_t m0, const uint32_t *src,
                 const uint32_t *new_upoff, uint32_t rows, uint64_t new_upper, float *outX, uint32_t *out_adj0, uint32_t *out_level,
                 uint32_t *out_upoff, uint32_t *out_upper, uint32_t *remap, uint32_t *status) {
  if (!shapes_hold(adj0, level, upoff, upper, old_rows, old_upper, stride, m, m0, src, new_upoff, rows, new_upper))
    return hipErrorInvalidValue;
  Dev dv;
  const size_t xb = (size_t)old_rows * stride * 4, ab = (size_t)old_rows * (m0 + 1) * 4, rb = (size_t)old_rows * 4;
  const size_t nxb = (size_t)rows * stride * 4, nab = (size_t)rows * (m0 + 1) * 4, nrb = (size_t)rows * 4;
  vt::HnswCompactArgs a{};
  a.X = dv.get<float>(xb, 0, X, xb);
  a.adj0 = dv.get<uint32_t>(ab, 0, adj0, ab);
  a.level = dv.get<uint32_t>(rb, 0, level, rb);
  a.upoff = dv.get<uint32_t>(rb, 0, upoff, rb);
  a.upper = dv.get<uint32_t>((size_t)old_upper * 4, 0, upper, (size_t)old_upper * 4);
  a.old_rows = old_rows;
  a.old_upper = old_upper;
  a.stride = stride;
  a.m = m;
  a.m0 = m0;
  a.src = dv.get<uint32_t>(nrb, 0, src, nrb);
  a.new_upoff = dv.get<uint32_t>(nrb, 0, new_upoff, nrb);
  a.rows = rows;
  a.new_upper = new_upper;
  a.remap = dv.get<uint32_t>(rb, 0xA5);
  a.outX = dv.get<float>(nxb, 0xA5);
  a.out_adj0 = dv.get<uint32_t>(nab, 0xA5);
  a.out_level = dv.get<uint32_t>(nrb, 0xA5);
  a.out_upoff = dv.get<uint32_t>(nrb, 0xA5);
  a.out_upper = dv.get<uint32_t>((size_t)new_upper * 4, 0xA5);
  a.status = dv.get<uint32_t>(vt::kHnswCompactGuards * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  if ((dv.err = vt::launch_hnsw_compact(a, dv.stream)) != hipSuccess) return dv.err;
  if (!dv.sync()) return dv.err;
  dv.back(outX, a.outX, nxb) && dv.back(out_adj0, a.out_adj0, nab) && dv.back(out_level, a.out_level, nrb) &&
      dv.back(out_upoff, a.out_upoff, nrb) && dv.back(out_upper, a.out_upper, (size_t)new_upper * 4) &&
      dv.back(remap, a.remap, rb) && dv.back(status, a.status, vt::kHnswCompactGuards * 4);
  return dv.err;
}

// The measurement of DESIGN 5: a slab of old_rows rows of `stride` floats, every other row live, every list full and
// naming live rows, one row in four with upper-layer lists; `reps` compactions timed with HIP events beside `reps`
// device-to-device copies of the same number of live bytes (rows and both list arrays), the fastest of each in
// milliseconds.  status_or: the guards' words of all runs, or-ed (0).
int vthc_time(uint32_t old_rows, uint32_t stride, uint32_t m, uint32_t m0, uint32_t reps, float *compact_ms, float *copy_ms,
              unsigned long long *live_bytes, uint32_t *status_or) {
  if (old_rows < 2 || old_rows > (1u << 22) || stride == 0 || stride % 4 || stride > 4096 || m == 0 || m0 < m || m0 > 256 || reps == 0 ||
      reps > 100)
    return hipErrorInvalidValue;
  const uint32_t rows = (old_rows + 1) / 2;
  std::vector<uint32_t> level(old_rows), upoff(old_rows), adj0((size_t)old_rows * (m0 + 1)), src(rows), new_upoff(rows), upper;
  auto fill = [&](uint32_t *list, uint32_t r, uint32_t lim) {
    list[0] = lim;
    for (uint32_t k = 1; k <= lim; ++k) list[k] = (uint32_t)(((uint64_t)r + 2ull * k * 977) % old_rows) & ~1u;
  };
  uint64_t nu = 0;
  for (uint32_t r = 0; r < old_rows; ++r) {
    level[r] = (r % 8 == 0) + (r % 32 == 0) + (r % 128 == 0);
    upoff[r] = (uint32_t)upper.size();
    upper.resize(upper.size() + (size_t)level[r] * (m + 1));
    for (uint32_t l = 0; l < level[r]; ++l) fill(upper.data() + upoff[r] + (size_t)l * (m + 1), r, m);
    fill(adj0.data() + (size_t)r * (m0 + 1), r, m0);
    if (r % 2 == 0) {
      src[r / 2] = r;
      new_upoff[r / 2] = (uint32_t)nu;
      nu += (uint64_t)level[r] * (m + 1);
    }
  }
  const uint64_t old_upper = upper.size();
  if (!shapes_hold(adj0.data(), level.data(), upoff.data(), upper.data(), old_rows, old_upper, stride, m, m0, src.data(),
                   new_upoff.data(), rows, nu))
    return hipErrorInvalidValue;
  Dev dv;
  const size_t xb = (size_t)old_rows * stride * 4, ab = adj0.size() * 4, rb = (size_t)old_rows * 4;
  const size_t nxb = (size_t)rows * stride * 4, nab = (size_t)rows * (m0 + 1) * 4, nrb = (size_t)rows * 4;
  vt::HnswCompactArgs a{};
  a.X = dv.get<float>(xb, 0x3C);
  a.adj0 = dv.get<uint32_t>(ab, 0, adj0.data(), ab);
  a.level = dv.get<uint32_t>(rb, 0, level.data(), rb);
  a.upoff = dv.get<uint32_t>(rb, 0, upoff.data(), rb);
  a.upper = dv.get<uint32_t>((size_t)old_upper * 4, 0, upper.data(), (size_t)old_upper * 4);
  a.old_rows = old_rows;
  a.old_upper = old_upper;
  a.stride = stride;
  a.m = m;
  a.m0 = m0;
  a.src = dv.get<uint32_t>(nrb, 0, src.data(), nrb);
  a.new_upoff = dv.get<uint32_t>(nrb, 0, new_upoff.data(), nrb);
  a.rows = rows;
  a.new_upper = nu;
  a.remap = dv.get<uint32_t>(rb, 0xA5);
  a.outX = dv.get<float>(nxb, 0xA5);
  a.out_adj0 = dv.get<uint32_t>(nab, 0xA5);
  a.out_level = dv.get<uint32_t>(nrb, 0xA5);
  a.out_upoff = dv.get<uint32_t>(nrb, 0xA5);
  a.out_upper = dv.get<uint32_t>((size_t)nu * 4, 0xA5);
  a.status = dv.get<uint32_t>(vt::kHnswCompactGuards * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if ((dv.err = hipEventCreate(&e0)) != hipSuccess) return dv.err;
  if ((dv.err = hipEventCreate(&e1)) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return dv.err;
  }
  float best_c = 1e30f, best_m = 1e30f;
  uint32_t fired[vt::kHnswCompactGuards], all = 0;
  for (uint32_t r = 0; r <= reps && dv.err == hipSuccess; ++r) {  // (run 0 warms up)
    float ms = 0.0f;
    (void)hipEventRecord(e0, dv.stream);
    dv.err = vt::launch_hnsw_compact(a, dv.stream);
    (void)hipEventRecord(e1, dv.stream);
    if (!dv.sync()) break;
    if ((dv.err = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) break;
    if (r) best_c = std::min(best_c, ms);
    if (!dv.back(fired, a.status, sizeof fired)) break;
    for (uint32_t g = 0; g < vt::kHnswCompactGuards; ++g) all |= fired[g] << g;
    // what the slab's growth path copies for as many live rows: rows, layer-0 lists, level, offsets, upper-layer lists
    (void)hipEventRecord(e0, dv.stream);
    (void)hipMemcpyAsync(a.outX, a.X, nxb, hipMemcpyDeviceToDevice, dv.stream);
    (void)hipMemcpyAsync(a.out_adj0, a.adj0, nab, hipMemcpyDeviceToDevice, dv.stream);
    (void)hipMemcpyAsync(a.out_level, a.level, nrb, hipMemcpyDeviceToDevice, dv.stream);
    (void)hipMemcpyAsync(a.out_upoff, a.upoff, nrb, hipMemcpyDeviceToDevice, dv.stream);
    dv.err = hipMemcpyAsync(a.out_upper, a.upper, (size_t)nu * 4, hipMemcpyDeviceToDevice, dv.stream);
    (void)hipEventRecord(e1, dv.stream);
    if (!dv.sync()) break;
    if ((dv.err = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) break;
    if (r) best_m = std::min(best_m, ms);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *compact_ms = best_c;
  *copy_ms = best_m;
  *live_bytes = (unsigned long long)(nxb + nab + 2 * nrb + nu * 4);
  *status_or = all;
  return dv.err;
}

}  // extern "C"
