// hnsw_stage_probe.cpp -- test infrastructure (tests/test_gpu_hnsw_stage_kernels.py): K15, the two scoring kernels behind
// an HNSW collection's staged searches (vt_hnsw_stage.hip: launch_hnsw_stage_bits, launch_hnsw_stage_score), launched on
// the caller's hand-made slab.  Built into libvt_hnsw_stage_probe.so from that unit and this file alone; the product
// library never sees it.
//
// The entry points take and return host arrays, own their device buffers for the length of the call and return the
// hipError_t as an int.  Everything a kernel will index with is checked against the caller's sizes first: a list entry
// that names no row of the slab is hipErrorInvalidValue, nothing launched (the kernel's guard for it is there to keep a
// read inside the slab; it is not for a test to lean on).  The key and payload columns are `extra` entries longer than
// the kernel's contract and start as 0xA5 bytes, as does the query's pad: a word the launch should not have written, or
// read, shows.
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

bool slab_holds(uint32_t rows, uint32_t stride, uint32_t d) {
  return d >= 1 && d <= (1u << 16) && stride % 4 == 0 && stride >= d && stride <= d + 64 && rows <= (1u << 20);
}

}  // namespace

extern "C" {

uint32_t vths_no_row() { return vt::kHnswNoRow; }
unsigned long long vths_empty_key() { return vt::kEmptyKey; }
uint32_t vths_lds_dim() { return vt::kHnswLdsDim; }

// K15b over X[rows][stride] with id_rank[rows] and the query q[d].  Out: keys / pay [rows + extra].
int vths_bits(const float *X, uint32_t rows, uint32_t stride, uint32_t d, const uint32_t *id_rank, const float *q, uint32_t extra,
              unsigned long long *keys, vt::Payload *pay) {
  if (!slab_holds(rows, stride, d) || extra > 4096) return hipErrorInvalidValue;
  std::vector<uint64_t> qw(vt::hnsw_stage_qword_count(d));
  vt::hnsw_stage_qwords(q, d, qw.data());
  Dev dv;
  const size_t xb = (size_t)rows * stride * 4, n = (size_t)rows + extra;
  vt::HnswStageBitsArgs a{};
  a.X = dv.get<float>(xb, 0, X, xb);
  a.stride = stride;
  a.d = d;
  a.rows = rows;
  a.id_rank = dv.get<uint32_t>((size_t)rows * 4, 0, id_rank, (size_t)rows * 4);
  a.qwords = dv.get<uint64_t>(qw.size() * 8, 0, qw.data(), qw.size() * 8);
  a.keys = dv.get<uint64_t>(n * 8, 0xA5);
  a.pay = dv.get<vt::Payload>(n * 8, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  if ((dv.err = vt::launch_hnsw_stage_bits(a, dv.stream)) != hipSuccess) return dv.err;
  if (!dv.sync()) return dv.err;
  dv.back(keys, a.keys, n * 8) && dv.back(pay, a.pay, n * 8);
  return dv.err;
}

// K15p over the same slab on the prefix p: every row (list null, n == rows) or the n rows of list[].  Out: keys / pay
// [n + extra] and the status word (0 before the launch).
int vths_score(const float *X, uint32_t rows, uint32_t stride, uint32_t d, uint32_t p, const float *q, const uint32_t *id_rank,
               const uint32_t *list, uint32_t n, int metric, int order, uint32_t extra, unsigned long long *keys, vt::Payload *pay,
               int *status) {
  if (!slab_holds(rows, stride, d) || p == 0 || p > d || extra > 4096 || n > (1u << 20) || (!list && n != rows) ||
      order < 0 || order > 3)
    return hipErrorInvalidValue;
  for (uint32_t i = 0; list && i < n; ++i)
    if (list[i] >= rows) return hipErrorInvalidValue;
  double qq = 0.0;
  for (uint32_t j = 0; j < p; ++j) qq += (double)q[j] * (double)q[j];
  Dev dv;
  const size_t xb = (size_t)rows * stride * 4, m = (size_t)n + extra;
  vt::HnswStageScoreArgs a{};
  a.X = dv.get<float>(xb, 0, X, xb);
  a.stride = stride;
  a.d = d;
  a.rows = rows;
  a.p = p;
  a.q = dv.get<float>((size_t)stride * 4, 0xA5, q, (size_t)d * 4);
  a.qq = qq;
  a.id_rank = dv.get<uint32_t>((size_t)rows * 4, 0, id_rank, (size_t)rows * 4);
  a.list = list ? dv.get<uint32_t>((size_t)n * 4, 0, list, (size_t)n * 4) : nullptr;
  a.n = n;
  a.metric = metric;
  a.order = order;
  a.keys = dv.get<uint64_t>(m * 8, 0xA5);
  a.pay = dv.get<vt::Payload>(m * 8, 0xA5);
  a.status = dv.get<int>(4, 0);
  if (dv.err != hipSuccess) return dv.err;
  if ((dv.err = vt::launch_hnsw_stage_score(a, dv.stream)) != hipSuccess) return dv.err;
  if (!dv.sync()) return dv.err;
  dv.back(keys, a.keys, m * 8) && dv.back(pay, a.pay, m * 8) && dv.back(status, a.status, 4);
  return dv.err;
}

}  // extern "C"
