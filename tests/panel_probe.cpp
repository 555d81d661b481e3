// panel_probe.cpp -- test infrastructure (tests/test_gpu_panel_kernels.py): the three kernels that walk the slab in row
// panels (csrc/vt_panel.cuh) -- K1p (vt_prefix_multi.hip), K6bm and K6b (vt_cosine.hip) -- launched one at a time on the
// caller's own arrays, so that a test can read back what no search returns: every sample cell, every tile maximum, every
// listed (key, row, raw), every count, the status word.  Built into libvt_panel_probe.so from vt_cosine.o,
// vt_prefix_multi.o and this file alone; the product library never sees it.
//
// As tests/batch_probe.cpp: every entry point takes and returns host arrays, owns its device buffers for the length of the
// call (hipMalloc, blocking copies, one stream, a synchronise before the copies back) and returns the hipError_t as an int.
// Everything a kernel will index is checked against the caller's lengths first: hipErrorInvalidValue, nothing launched.
// Output buffers are filled with 0xA5 before the launch: a write outside the contract shows.
#define VT_ENV_IMPLEMENTATION  // (this library's own copy of the settings table: csrc/vt_env.h)
#include "vt_env.h"
#include "vt_device.h"

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

constexpr uint32_t kMaxD = 4096, kMaxRows = 1u << 20, kMaxBlocks = 1024, kMaxCap = 1u << 16;
enum { kK1p = 0, kK6bm = 1 };
enum { kSweep = 0, kDense = 1, kMaxima = 2 };

// X holds n rows `stride` floats apart; a walk reads whole 32-float panels of a row's first d floats, 16 bytes at a time
bool rows_ok(const float *X, uint64_t x_floats, uint64_t stride, uint32_t n, uint32_t d) {
  return X && n >= 1 && n <= kMaxRows && d >= 1 && d <= kMaxD && stride % 4 == 0 && stride >= vt::padded_dim(d) && stride <= 2 * kMaxD &&
         x_floats >= (uint64_t)n * stride;
}

// f64_dot(q, q) over the first d coordinates, sequentially (distances.rs:179-185): what the host hands K6b and K6bm
double seq_qq(const float *q, uint32_t d) {
  double qq = 0.0;
  for (uint32_t j = 0; j < d; ++j) qq += (double)q[j] * (double)q[j];
  return qq;
}

void split(const std::vector<vt::Payload> &pay, uint32_t *rows, uint32_t *raw_bits) {
  for (size_t i = 0; i < pay.size(); ++i) {
    rows[i] = pay[i].row;
    std::memcpy(&raw_bits[i], &pay[i].raw, 4);
  }
}

}  // namespace

extern "C" {

uint32_t vpp_group_max() { return vt::kGroupSweepMax; }
uint32_t vpp_padded_dim(uint32_t d) { return vt::padded_dim(d); }
size_t vpp_group_lds_bytes() { return vt::group_sweep_lds_bytes(); }
int vpp_group_blocks_per_cu(int metric) { return vt::group_sweep_blocks_per_cu(metric); }

// One launch of a group's sweep: launch_prefix_multi (kernel 0) or launch_cosine_scan_multi (kernel 1) in sweep mode
// (mode 0), dense mode (1) or dense mode with tile maxima (2).  Lengths are in elements of the array they belong to.
// Q is [8][q_stride] f32 (all eight rows: K1p reads them whatever nq is); for kernel 1 the probe makes of it what the host
// makes: the prefixes as f64, [8][padded_dim(d)], rows >= nq zero, and qq[].  Sweep mode: cand_count is zeroed before the
// launch as the host does; cand_keys / cand_rows / cand_raw ([8][cand_cap]) come back over their 0xA5 fill.  Dense modes:
// sample[8][sample_rows] likewise.  *status is the device's status word after the launch (0 before it).
struct VppGroup {
  int32_t kernel, mode, metric, order;
  uint32_t n, d, nq, q_stride, sample_stride, sample_rows, cand_cap, blocks;
  const float *X;
  uint64_t x_floats, stride;
  const float *Q;
  uint64_t q_floats;
  const uint32_t *id_rank;  // null: the key's low word is the row
  uint64_t rank_len;
  const float *tau;
  uint64_t tau_len;
  float *sample;
  uint64_t sample_len;
  uint64_t *cand_keys;
  uint32_t *cand_rows, *cand_raw;
  uint64_t cand_len;
  uint32_t *cand_count;
  uint64_t count_len;
  int32_t *status;
};

int vpp_group(const VppGroup *p) {
  constexpr uint32_t G = vt::kGroupSweepMax;
  if (!p || (p->kernel != kK1p && p->kernel != kK6bm) || p->mode < kSweep || p->mode > kMaxima || !p->status) return hipErrorInvalidValue;
  if (!rows_ok(p->X, p->x_floats, p->stride, p->n, p->d) || p->nq < 1 || p->nq > G || p->blocks < 1 || p->blocks > kMaxBlocks)
    return hipErrorInvalidValue;
  // K1p reads whole 8-float chunks of all eight query rows; the overflow recovery reads d floats of a query's row
  if (!p->Q || p->q_stride % 8 != 0 || p->q_stride < (p->d + 7) / 8 * 8 || p->q_stride > 2 * kMaxD || p->q_floats != (uint64_t)G * p->q_stride)
    return hipErrorInvalidValue;
  if (p->id_rank && p->rank_len < p->n) return hipErrorInvalidValue;
  const bool dense = p->mode != kSweep;
  const uint64_t tiles_all = ((uint64_t)p->n + 63) / 64;
  if (dense) {
    // a cell is written only below sample_rows, whatever the launch walks: the test may give fewer
    if (p->sample_stride < 1 || p->sample_stride > tiles_all || p->sample_rows < 1 || !p->sample || p->sample_len != (uint64_t)G * p->sample_rows)
      return hipErrorInvalidValue;
  } else if (!p->tau || p->tau_len != G || !p->cand_count || p->count_len != G || p->cand_cap < 1 || p->cand_cap > kMaxCap || !p->cand_keys ||
             !p->cand_rows || !p->cand_raw || p->cand_len != (uint64_t)G * p->cand_cap) {
    return hipErrorInvalidValue;
  }
  Dev dv;
  vt::GroupSweepArgs a{};
  a.X = dv.get<float>(p->x_floats * 4, 0, p->X, p->x_floats * 4);
  a.stride = p->stride;
  a.Q = dv.get<float>(p->q_floats * 4, 0, p->Q, p->q_floats * 4);
  a.q_stride = p->q_stride;
  if (p->kernel == kK6bm) {
    const uint32_t ldq = vt::padded_dim(p->d);
    std::vector<double> qd((size_t)G * ldq, 0.0);
    for (uint32_t i = 0; i < p->nq; ++i) {
      const float *q = p->Q + (size_t)i * p->q_stride;
      for (uint32_t j = 0; j < p->d; ++j) qd[(size_t)i * ldq + j] = (double)q[j];
      a.qq[i] = seq_qq(q, p->d);
    }
    a.Qd = dv.get<double>(qd.size() * 8, 0, qd.data(), qd.size() * 8);
  }
  if (p->id_rank) a.id_rank = dv.get<uint32_t>(p->rank_len * 4, 0, p->id_rank, p->rank_len * 4);
  a.n = p->n;
  a.d = p->d;
  a.nq = p->nq;
  a.metric = p->metric;
  a.order = p->order;
  a.status = dv.get<int>(4, 0);
  if (dense) {
    a.sample = dv.get<float>(p->sample_len * 4, 0xA5);
    a.sample_stride = p->sample_stride;
    a.sample_rows = p->sample_rows;
    a.sample_maxima = p->mode == kMaxima ? 1u : 0u;
  } else {
    a.tau = dv.get<float>(p->tau_len * 4, 0, p->tau, p->tau_len * 4);
    a.cand_keys = dv.get<uint64_t>(p->cand_len * 8, 0xA5);
    a.cand_pay = dv.get<vt::Payload>(p->cand_len * 8, 0xA5);
    a.cand_count = dv.get<uint32_t>(p->count_len * 4, 0);
    a.cand_cap = p->cand_cap;
  }
  if (dv.err != hipSuccess) return dv.err;
  dv.err = p->kernel == kK1p ? vt::launch_prefix_multi(a, p->blocks, dv.stream) : vt::launch_cosine_scan_multi(a, p->blocks, dv.stream);
  if (!dv.sync()) return dv.err;
  if (!dv.back(p->status, a.status, 4)) return dv.err;
  if (dense) {
    dv.back(p->sample, a.sample, p->sample_len * 4);
  } else {
    std::vector<vt::Payload> pay(p->cand_len);
    if (dv.back(p->cand_keys, a.cand_keys, p->cand_len * 8) && dv.back(pay.data(), a.cand_pay, p->cand_len * 8) &&
        dv.back(p->cand_count, a.cand_count, p->count_len * 4))
      split(pay, p->cand_rows, p->cand_raw);
  }
  return dv.err;
}

// One launch of launch_cosine_scan (K6b) over X[n][stride]'s first d columns against q[q_floats] (padded with zeros to
// padded_dim(d)).  List mode (key_out null): part_keys / part_rows / part_raw [blocks][k] come back over their 0xA5 fill.
// Key-column mode: key_out[n] likewise.  *status as above.
int vpp_cosine_scan(const float *X, uint64_t x_floats, uint64_t stride, uint32_t n, uint32_t d, const float *q, uint64_t q_floats,
                    const uint32_t *id_rank, uint64_t rank_len, uint32_t k, int has_lo, uint64_t lo_key, uint32_t blocks, uint64_t *part_keys,
                    uint32_t *part_rows, uint32_t *part_raw, uint64_t part_len, uint64_t *key_out, uint64_t key_len, int32_t *status) {
  if (!rows_ok(X, x_floats, stride, n, d) || !q || q_floats != vt::padded_dim(d) || (id_rank && rank_len < n) || k < 1 ||
      k > (uint32_t)vt::kMaxFusedK || vt::cosine_scan_lds_bytes(d, k) == 0 || blocks < 1 || blocks > kMaxBlocks || !status)
    return hipErrorInvalidValue;
  if (key_out ? key_len < n : (!part_keys || !part_rows || !part_raw || part_len != (uint64_t)blocks * k)) return hipErrorInvalidValue;
  Dev dv;
  vt::CosineScanArgs a{};
  a.X = dv.get<float>(x_floats * 4, 0, X, x_floats * 4);
  a.stride = stride;
  a.q = dv.get<float>(q_floats * 4, 0, q, q_floats * 4);
  a.qq = seq_qq(q, d);
  if (id_rank) a.id_rank = dv.get<uint32_t>(rank_len * 4, 0, id_rank, rank_len * 4);
  a.n = n;
  a.d = d;
  a.k = k;
  a.lo_key = lo_key;
  a.has_lo = has_lo;
  a.status = dv.get<int>(4, 0);
  // (the list buffers exist in key-column mode too: the kernel is handed what the host hands it)
  const uint64_t slots = (uint64_t)blocks * k;
  a.part_keys = dv.get<uint64_t>(slots * 8, 0xA5);
  a.part_pay = dv.get<vt::Payload>(slots * 8, 0xA5);
  if (key_out) a.key_out = dv.get<uint64_t>(key_len * 8, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_cosine_scan(a, blocks, dv.stream);
  if (!dv.sync()) return dv.err;
  if (!dv.back(status, a.status, 4)) return dv.err;
  if (key_out) {
    dv.back(key_out, a.key_out, key_len * 8);
  } else {
    std::vector<vt::Payload> pay(slots);
    if (dv.back(part_keys, a.part_keys, slots * 8) && dv.back(pay.data(), a.part_pay, slots * 8)) split(pay, part_rows, part_raw);
  }
  return dv.err;
}

}  // extern "C"
