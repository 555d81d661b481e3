// sketch4_best_probe.cpp -- test infrastructure (tests/test_gpu_sketch4_best_kernels.py), beside sketch4_probe.cpp and
// sketch4_rescore_probe.cpp: K1n's threshold from each list's best rows -- the 4-bit pass asked for its lists'
// best words (vt_sketch_nibble.hip) and the rescoring kernel handed such words in place of a threshold
// (vt_sketch4_rescore.hip), each launched on the caller's own arrays.  Built into libvt_sketch4_best_probe.so from those two
// units and this file alone; the product library never sees it.
//
// Every entry point takes and returns host arrays, owns its device buffers for the length of the call and returns the
// hipError_t as an int.  Every size a kernel will index with is checked against the caller's buffer lengths first:
// hipErrorInvalidValue, nothing launched.
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

uint32_t vtbp_block_lists() { return vt::kSketch4BlockLists; }
uint32_t vtbp_best_rows() { return vt::kSketch4BestRows; }
uint32_t vtbp_max_words() { return vt::kSketch4BestMaxWords; }
uint32_t vtbp_max_k() { return vt::kSketch4BestMaxK; }
uint32_t vtbp_delivered() { return vt::kScanFilterDelivered; }

// launch_sketch4_scan with `blocks` blocks and lists of k over an image of n rows, as sketch4_probe.cpp's vtp4_scan has it,
// and -- want_best -- asked for the lists' best words: X[x_floats] holds the n rows `stride` floats apart, q the query (d
// floats), order the reduce order.  keys, pay ({row, raw bits}), lo_words and hi_words come back as [lists][k] and best as
// [lists][vtbp_best_rows()], lists = blocks * vtbp_block_lists(), all pre-filled with 0xA5 (without want_best `best` comes
// back as that).
int vtbp_scan(const unsigned char *img, size_t img_bytes, uint32_t n, uint32_t d, int metric, const uint32_t *id_rank,
              const unsigned char *qimg, size_t qimg_bytes, const float *t, double qn, double eta, double kerr, uint32_t k,
              uint32_t blocks, const float *X, size_t x_floats, size_t stride, const float *q, int order, int want_best,
              unsigned long long *keys, uint32_t *pay, uint32_t *lo_words, uint32_t *hi_words, uint32_t *best) {
  if (d == 0 || d > vt::kSketchMaxDim || n == 0 || k == 0 || blocks == 0 || blocks > 4096 || !lo_words || !hi_words || !best)
    return hipErrorInvalidValue;
  const uint32_t ld8 = vt::sketch_ld8(d);
  const size_t ld = vt::padded_dim(d);
  if (img_bytes != vt::sketch4_bytes(n, d) || qimg_bytes != 3 * (size_t)ld8 / 2) return hipErrorInvalidValue;
  if (stride < ld || stride % 4 || (size_t)n * stride > x_floats) return hipErrorInvalidValue;
  const size_t lists = (size_t)blocks * vt::kSketch4BlockLists, slots = lists * k;
  std::vector<float> qpad(ld, 0.0f);
  std::memcpy(qpad.data(), q, (size_t)d * sizeof(float));
  Dev dv;
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0, img, img_bytes);
  unsigned char *dQ = dv.get<unsigned char>(qimg_bytes, 0, qimg, qimg_bytes);
  uint32_t *dR = id_rank ? dv.get<uint32_t>((size_t)n * 4, 0, id_rank, (size_t)n * 4) : nullptr;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0xA5);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0xA5);
  uint32_t *dLo = dv.get<uint32_t>(slots * 4, 0xA5), *dHi = dv.get<uint32_t>(slots * 4, 0xA5);
  uint32_t *dB = dv.get<uint32_t>(lists * vt::kSketch4BestRows * 4, 0xA5);
  vt::Sketch6ScanArgs a{};
  a.img = dI;
  a.id_rank = dR;
  a.qimg = reinterpret_cast<const uint32_t *>(dQ);
  a.n = n;
  a.d = d;
  a.ld8 = ld8;
  a.metric = metric;
  for (int j = 0; j < vt::kSketch6Levels; ++j) a.t[j] = t[j];
  a.qn = qn;
  a.eta = eta;
  a.kerr = kerr;
  a.k = k;
  a.part_keys = dK;
  a.part_pay = dP;
  a.lo_words = dLo;
  a.hi_words = dHi;
  if (want_best) {
    a.best_words = dB;
    a.X = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
    a.stride = stride;
    a.q = dv.get<float>(ld * sizeof(float), 0, qpad.data(), ld * sizeof(float));
    a.order = order;
  }
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_sketch4_scan(a, blocks, dv.stream);
  if (dv.sync())
    dv.back(keys, dK, slots * 8) && dv.back(pay, dP, slots * 8) && dv.back(lo_words, dLo, slots * 4) && dv.back(hi_words, dHi, slots * 4) &&
        dv.back(best, dB, lists * vt::kSketch4BestRows * 4);
  return dv.err;
}

// launch_sketch4_rescore handed best[best_count] in place of a threshold word, as sketch4_rescore_probe.cpp's vtpr_rescore
// launches it on a word: the same arrays in, the same out, per run r, and kt_out[r] = the word block 0 published (0xA5A5A5A5
// before every run).
int vtbp_rescore(const float *X, size_t x_floats, size_t stride, uint32_t n_rows, const float *q, uint32_t d, int metric, int order,
                 const uint32_t *id_rank, const uint32_t *hi_words, const uint32_t *pay_rows, uint32_t blocks, uint32_t kp,
                 const uint32_t *best, uint32_t best_count, uint32_t k, uint32_t cap, uint32_t runs, uint32_t *head,
                 unsigned long long *keys, uint32_t *rows, uint32_t *raws, uint32_t *info, uint32_t *words, int *status_word,
                 uint32_t *kt_out) {
  if (d == 0 || d > vt::kSketchMaxDim || k == 0 || k > (uint32_t)vt::kSmallK || kp == 0 || kp > (uint32_t)vt::kSmallK || blocks == 0 ||
      blocks > 4096 || runs == 0 || n_rows == 0 || best_count == 0 || best_count > (1u << 20))
    return hipErrorInvalidValue;
  const size_t ld = vt::padded_dim(d);
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
  a.best_words = dv.get<uint32_t>((size_t)best_count * 4, 0xA5, best, (size_t)best_count * 4);
  a.best_count = best_count;
  a.kt_out = dv.get<uint32_t>(4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  std::vector<vt::ResultBlock> hb(1);
  for (uint32_t r = 0; r < runs; ++r) {
    if ((dv.err = hipMemsetAsync(f.out, 0xA5, sizeof(vt::ResultBlock), dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemsetAsync(f.info, 0xA5, 16, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = hipMemsetAsync(a.kt_out, 0xA5, 4, dv.stream)) != hipSuccess) return dv.err;
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
    dv.back(info + 4 * r, f.info, 16) && dv.back(words + 2 * r, f.fsync, 8) && dv.back(status_word + r, f.status, 4) &&
        dv.back(kt_out + r, a.kt_out, 4);
    if (dv.err != hipSuccess) return dv.err;
  }
  return dv.err;
}

}  // extern "C"
