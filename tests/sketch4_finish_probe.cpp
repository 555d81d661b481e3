// sketch4_finish_probe.cpp -- test infrastructure (tests/test_gpu_sketch4_finish_kernels.py), beside sketch4_probe.cpp: the
// kernel that finishes K1n's chain, launched on the caller's own arrays -- the gathered K1 in filter mode
// (vt_scan_filter.hip).  Built into libvt_sketch4_finish_probe.so from that unit and this file alone; the product library
// never sees it.
//
// Every entry point takes and returns host arrays, owns its device buffers for the length of the call and returns the
// hipError_t as an int.  Every size a kernel will index with is checked against the caller's buffer lengths first:
// hipErrorInvalidValue, nothing launched.  The words a launch wants zeroed arrive as the search delivers them: in a copy
// from the host queued in front of the launch.
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

const uint32_t kZeros[vt::kScanFilterSyncWords] = {};

}  // namespace

extern "C" {

uint32_t vtpf_filter_cap() { return vt::kScanFilterCap; }
uint32_t vtpf_delivered() { return vt::kScanFilterDelivered; }

// launch_scan_filter over the rows list[0 .. min(dev_count, cap)) of X, `runs` times on the same buffers: only the
// sync words are zeroed, by a copy queued in front of each launch.  X[x_floats]: n_rows rows `stride` floats apart, every
// entry of list[cap] below n_rows; q: d floats; id_rank: n_rows words or null.  info_in[4] is what the collect would have
// left; the result block starts as 0xA5 bytes before every run.  Per run r: head[r] = {status, count} as the block holds
// them, keys[r][k], rows[r][k], raws[r][k] (the entries, 0xA5 where none was written), info[r][4], survivors[r] (the
// count word).
int vtpf_filter(const float *X, size_t x_floats, size_t stride, uint32_t n_rows, const float *q, uint32_t d, int metric, int order,
                const uint32_t *id_rank, const uint32_t *list, uint32_t cap, uint32_t dev_count, uint32_t hi_word, uint32_t k,
                uint32_t blocks, uint32_t runs, const uint32_t *info_in, uint32_t *head, unsigned long long *keys, uint32_t *rows,
                uint32_t *raws, uint32_t *info, uint32_t *survivors, int *status_word) {
  if (d == 0 || d > vt::kSketchMaxDim || k == 0 || k > (uint32_t)vt::kSmallK || cap == 0 || blocks == 0 || blocks > 4096 || runs == 0 ||
      n_rows == 0)
    return hipErrorInvalidValue;
  const size_t ld = ((size_t)d + 63) / 64 * 64;
  if (stride < ld || stride % 4 || (size_t)n_rows * stride > x_floats) return hipErrorInvalidValue;
  for (uint32_t i = 0; i < cap; ++i)
    if (list[i] >= n_rows) return hipErrorInvalidValue;
  std::vector<float> qpad(ld, 0.0f);
  std::memcpy(qpad.data(), q, (size_t)d * sizeof(float));
  Dev dv;
  vt::ScanArgs a{};
  a.X = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  a.stride = stride;
  a.q = dv.get<float>(ld * sizeof(float), 0, qpad.data(), ld * sizeof(float));
  a.id_rank = id_rank ? dv.get<uint32_t>((size_t)n_rows * 4, 0, id_rank, (size_t)n_rows * 4) : nullptr;
  a.gather = dv.get<uint32_t>((size_t)cap * 4, 0, list, (size_t)cap * 4);
  a.gather_stride = 1;
  a.n = cap;
  a.d = d;
  a.metric = metric;
  a.order = order;
  a.k = k;
  a.status = dv.get<int>(4, 0);
  a.batch_counts = dv.get<uint32_t>(4, 0, &dev_count, 4);
  a.batch_cap = cap;
  a.hi_word = dv.get<uint32_t>(4, 0, &hi_word, 4);
  a.surv_keys = dv.get<uint64_t>((size_t)vt::kScanFilterCap * 8, 0xA5);
  a.surv_pay = dv.get<vt::Payload>((size_t)vt::kScanFilterCap * 8, 0xA5);
  a.surv_cap = vt::kScanFilterCap;
  a.fsync = dv.get<uint32_t>(sizeof kZeros, 0xA5);
  a.out = dv.get<vt::ResultBlock>(sizeof(vt::ResultBlock), 0xA5);
  a.info = dv.get<uint32_t>(16, 0, info_in, 16);
  if (dv.err != hipSuccess) return dv.err;
  std::vector<vt::ResultBlock> hb(1);
  for (uint32_t r = 0; r < runs; ++r) {
    if ((dv.err = hipMemsetAsync(a.out, 0xA5, sizeof(vt::ResultBlock), dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemcpyAsync(a.info, info_in, 16, hipMemcpyHostToDevice, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemcpyAsync(a.fsync, kZeros, sizeof kZeros, hipMemcpyHostToDevice, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = vt::launch_scan_filter(a, blocks, dv.stream)) != hipSuccess) return dv.err;
    if (!dv.sync()) return dv.err;
    if (!dv.back(hb.data(), a.out, sizeof(vt::ResultBlock))) return dv.err;
    head[2 * r] = (uint32_t)hb[0].status;
    head[2 * r + 1] = hb[0].count;
    for (uint32_t j = 0; j < k; ++j) {
      keys[(size_t)r * k + j] = hb[0].e[j].key;
      rows[(size_t)r * k + j] = hb[0].e[j].row;
      std::memcpy(raws + (size_t)r * k + j, &hb[0].e[j].raw, 4);
    }
    dv.back(info + 4 * r, a.info, 16) && dv.back(survivors + r, a.fsync, 4) && dv.back(status_word + r, a.status, 4);
    if (dv.err != hipSuccess) return dv.err;
  }
  return dv.err;
}

}  // extern "C"
