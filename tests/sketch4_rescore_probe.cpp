// sketch4_rescore_probe.cpp -- test infrastructure (tests/test_gpu_sketch4_rescore_kernels.py), beside
// sketch4_finish_probe.cpp: K1n's last link, the kernel that rescores the candidates straight from the pass's lists
// (vt_sketch4_rescore.hip), launched on the caller's hand-made lists.  Built into libvt_sketch4_rescore_probe.so from that
// unit and this file alone; the product library never sees it.
//
// The entry point takes and returns host arrays, owns its device buffers for the length of the call and returns the
// hipError_t as an int.  Every size the kernel will index with is checked against the caller's buffer lengths first:
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

uint32_t vtpr_filter_cap() { return vt::kScanFilterCap; }
uint32_t vtpr_delivered() { return vt::kScanFilterDelivered; }
uint32_t vtpr_block_lists() { return vt::kSketch4BlockLists; }
// (0: the launcher does not take rows of d dimensions)
size_t vtpr_lds_bytes(uint32_t d, uint32_t kp) { return vt::sketch4_rescore_lds_bytes(d, kp); }

// launch_sketch4_rescore on `blocks` blocks over hand-made lists, `runs` times on the same buffers: only the sync words are
// zeroed, by a copy queued in front of each launch.  X[x_floats]: n_rows rows `stride` floats apart; q: d floats; id_rank:
// n_rows words or null.  hi_words and pay_rows hold [blocks * kSketch4BlockLists][kp] slots: a slot's key(hi) word
// (0xffffffff: empty) and its row, below n_rows in every live slot (an empty slot's row is anything: the kernel loads it
// and must not use it).  kt: the refine's word.  info and the result block start as 0xA5 bytes before every run.  Per run
// r: head[r] = {status, count} as the block holds them, keys[r][k], rows[r][k], raws[r][k] (the entries, 0xA5 where none
// was written), info[r][4], words[r] = {survivor count, overflow / fail word}, status_word[r] (the device's status word
// after the run).
int vtpr_rescore(const float *X, size_t x_floats, size_t stride, uint32_t n_rows, const float *q, uint32_t d, int metric, int order,
                 const uint32_t *id_rank, const uint32_t *hi_words, const uint32_t *pay_rows, uint32_t blocks, uint32_t kp, uint32_t kt,
                 uint32_t k, uint32_t cap, uint32_t runs, uint32_t *head, unsigned long long *keys, uint32_t *rows, uint32_t *raws,
                 uint32_t *info, uint32_t *words, int *status_word) {
  if (d == 0 || d > vt::kSketchMaxDim || k == 0 || k > (uint32_t)vt::kSmallK || kp == 0 || kp > (uint32_t)vt::kSmallK || blocks == 0 ||
      blocks > 4096 || runs == 0 || n_rows == 0)
    return hipErrorInvalidValue;
  const size_t ld = ((size_t)d + 63) / 64 * 64;
  if (stride < ld || stride % 4 || (size_t)n_rows * stride > x_floats) return hipErrorInvalidValue;
  const size_t slots = (size_t)blocks * vt::kSketch4BlockLists * kp;
  std::vector<vt::Payload> pay(slots);
  for (size_t i = 0; i < slots; ++i) {
    if (hi_words[i] != 0xffffffffu && pay_rows[i] >= n_rows) return hipErrorInvalidValue;
    pay[i].row = pay_rows[i];
    pay[i].raw = 0.0f;
  }
  std::vector<float> qpad(ld, 0.0f);
  std::memcpy(qpad.data(), q, (size_t)d * sizeof(float));
  Dev dv;
  vt::Sketch4RescoreArgs a{};
  vt::ScanArgs &f = a.s;
  f.X = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  f.stride = stride;
  f.q = dv.get<float>(ld * sizeof(float), 0, qpad.data(), ld * sizeof(float));
  f.id_rank = id_rank ? dv.get<uint32_t>((size_t)n_rows * 4, 0, id_rank, (size_t)n_rows * 4) : nullptr;
  f.n = n_rows;
  f.d = d;
  f.metric = metric;
  f.order = order;
  f.k = k;
  f.status = dv.get<int>(4, 0);
  f.hi_word = dv.get<uint32_t>(4, 0, &kt, 4);
  f.surv_keys = dv.get<uint64_t>((size_t)vt::kScanFilterCap * 8, 0xA5);
  f.surv_pay = dv.get<vt::Payload>((size_t)vt::kScanFilterCap * 8, 0xA5);
  f.surv_cap = vt::kScanFilterCap;
  f.fsync = dv.get<uint32_t>(sizeof kZeros, 0xA5);
  f.out = dv.get<vt::ResultBlock>(sizeof(vt::ResultBlock), 0xA5);
  f.info = dv.get<uint32_t>(16, 0xA5);
  a.hi_words = dv.get<uint32_t>(slots * 4, 0xFF, hi_words, slots * 4);
  a.pay = dv.get<vt::Payload>(slots * sizeof(vt::Payload), 0xA5, pay.data(), slots * sizeof(vt::Payload));
  a.kp = kp;
  a.cap = cap;
  if (dv.err != hipSuccess) return dv.err;
  std::vector<vt::ResultBlock> hb(1);
  for (uint32_t r = 0; r < runs; ++r) {
    if ((dv.err = hipMemsetAsync(f.out, 0xA5, sizeof(vt::ResultBlock), dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemsetAsync(f.info, 0xA5, 16, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemsetAsync(f.status, 0, 4, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemcpyAsync(f.fsync, kZeros, sizeof kZeros, hipMemcpyHostToDevice, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = vt::launch_sketch4_rescore(a, blocks, dv.stream)) != hipSuccess) return dv.err;
    if (!dv.sync()) return dv.err;
    if (!dv.back(hb.data(), f.out, sizeof(vt::ResultBlock))) return dv.err;
    head[2 * r] = (uint32_t)hb[0].status;
    head[2 * r + 1] = hb[0].count;
    for (uint32_t j = 0; j < k; ++j) {
      keys[(size_t)r * k + j] = hb[0].e[j].key;
      rows[(size_t)r * k + j] = hb[0].e[j].row;
      std::memcpy(raws + (size_t)r * k + j, &hb[0].e[j].raw, 4);
    }
    dv.back(info + 4 * r, f.info, 16) && dv.back(words + 2 * r, f.fsync, 8) && dv.back(status_word + r, f.status, 4);
    if (dv.err != hipSuccess) return dv.err;
  }
  return dv.err;
}

}  // extern "C"
