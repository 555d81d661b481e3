// sketch4_probe.cpp -- test infrastructure (tests/test_gpu_sketch4_kernels.py), as sketch_probe.cpp is for the other three
// sketches: K1n's builders and pass (vt_sketch_nibble.hip) and the chain behind it with the exact threshold (vt_sketch.hip:
// sketch_thresh_kernel filing slots, sketch_refine_kernel, sketch_collect_kernel taking the published word) launched one
// at a time on the caller's own arrays.  Built into libvt_sketch4_probe.so from those two units and this file alone; the
// product library never sees it.
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

}  // namespace

extern "C" {

size_t vtp4_image_bytes(uint32_t rows, uint32_t d) { return vt::sketch4_bytes(rows, d); }
uint32_t vtp4_thresh_blocks(uint32_t lists, uint32_t kp) { return vt::sketch_thresh_blocks(lists, kp); }
uint32_t vtp4_block_lists() { return vt::kSketch4BlockLists; }

// launch_sketch4_build over X[x_floats] (rows `stride` floats apart) into an image of rows_img rows pre-filled with 0xA5;
// *max_norm is the f64's bits, in and out.
int vtp4_build(const float *X, size_t x_floats, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, unsigned char *img,
               size_t img_bytes, unsigned long long *max_norm) {
  if (d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows || n_src > rows_img ||
      img_bytes != vt::sketch4_bytes(rows_img, d) || (n_src && (size_t)(n_src - 1) * stride + d > x_floats))
    return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_sketch4_build(dX, stride, n_src, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch4_rows: the rows of list[count] of X patched into the caller's image (in and out).
int vtp4_rows(const float *X, size_t x_floats, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
              unsigned char *img, size_t img_bytes, unsigned long long *max_norm) {
  if (d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows || img_bytes != vt::sketch4_bytes(rows_img, d))
    return hipErrorInvalidValue;
  for (uint32_t i = 0; i < count; ++i)
    if (list[i] < rows_img && (size_t)list[i] * stride + d > x_floats) return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  uint32_t *dL = dv.get<uint32_t>((size_t)count * 4, 0, list, (size_t)count * 4);
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5, img, img_bytes);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_sketch4_rows(dX, stride, dL, count, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch4_scan with `blocks` blocks and lists of k over an image of n rows.  qimg: the query's levels as the pass
// reads them ([3][ld8 / 8] dwords of nibbles), t: their three scales.  keys, pay ({row, raw bits}), lo_words and hi_words
// come back as [blocks * vtp4_block_lists()][k], pre-filled with 0xA5.
int vtp4_scan(const unsigned char *img, size_t img_bytes, uint32_t n, uint32_t d, int metric, const uint32_t *id_rank,
              const unsigned char *qimg, size_t qimg_bytes, const float *t, double qn, double eta, double kerr, uint32_t k,
              uint32_t blocks, unsigned long long *keys, uint32_t *pay, uint32_t *lo_words, uint32_t *hi_words) {
  if (d == 0 || d > vt::kSketchMaxDim || n == 0 || k == 0 || blocks == 0 || blocks > 4096 || !lo_words || !hi_words)
    return hipErrorInvalidValue;
  const uint32_t ld8 = vt::sketch_ld8(d);
  if (img_bytes != vt::sketch4_bytes(n, d) || qimg_bytes != 3 * (size_t)ld8 / 2) return hipErrorInvalidValue;
  const size_t slots = (size_t)blocks * vt::kSketch4BlockLists * k;
  Dev dv;
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0, img, img_bytes);
  unsigned char *dQ = dv.get<unsigned char>(qimg_bytes, 0, qimg, qimg_bytes);
  uint32_t *dR = id_rank ? dv.get<uint32_t>((size_t)n * 4, 0, id_rank, (size_t)n * 4) : nullptr;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0xA5);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0xA5);
  uint32_t *dLo = dv.get<uint32_t>(slots * 4, 0xA5), *dHi = dv.get<uint32_t>(slots * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
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
  dv.err = vt::launch_sketch4_scan(a, blocks, dv.stream);
  if (dv.sync())
    dv.back(keys, dK, slots * 8) && dv.back(pay, dP, slots * 8) && dv.back(lo_words, dLo, slots * 4) && dv.back(hi_words, dHi, slots * 4);
  return dv.err;
}

// launch_sketch_thresh (filing slots), launch_sketch_refine, launch_sketch_collect (taking the refined word) over
// [lists][kp] word arrays and payloads ({row, -}), `runs` times on the same buffers; sync[] and the threshold word start as
// garbage and are never touched between the runs.  X[x_floats]: the rows the payloads name, `stride` floats apart, every
// payload row below n_rows; q: the query, d floats.  Per run r: parts[r][tb * k], slots[r][tb * k], kt[r], picked[r][k],
// rows[r][cap], count[r], info[r][4].
int vtp4_certify(const uint32_t *lo_words, const uint32_t *hi_words, const uint32_t *pay, uint32_t lists, uint32_t kp, uint32_t k,
                 uint32_t cap, const float *X, size_t x_floats, size_t stride, uint32_t n_rows, const float *q, uint32_t d, int metric,
                 int order, uint32_t runs, uint32_t *parts, uint32_t *slots, uint32_t *kt, uint32_t *picked, uint32_t *rows,
                 uint32_t *count, uint32_t *info) {
  if (lists == 0 || kp == 0 || k == 0 || cap == 0 || runs == 0 || (size_t)lists * kp > (1u << 24) || d == 0 || d > vt::kSketchMaxDim)
    return hipErrorInvalidValue;
  const size_t nslots = (size_t)lists * kp, tb = vt::sketch_thresh_blocks(lists, kp);
  const size_t ld = ((size_t)d + 63) / 64 * 64;  // padded_dim: the refine kernel reads whole padded rows
  if (stride < ld || stride % 4 || n_rows == 0 || (size_t)n_rows * stride > x_floats) return hipErrorInvalidValue;
  for (size_t i = 0; i < nslots; ++i)
    if (lo_words[i] != 0xffffffffu && pay[2 * i] >= n_rows) return hipErrorInvalidValue;
  std::vector<float> qpad(ld, 0.0f);
  std::memcpy(qpad.data(), q, (size_t)d * sizeof(float));
  Dev dv;
  vt::SketchSpreadArgs a{};
  a.lo_words = dv.get<uint32_t>(nslots * 4, 0, lo_words, nslots * 4);
  a.hi_words = dv.get<uint32_t>(nslots * 4, 0, hi_words, nslots * 4);
  a.pay = dv.get<vt::Payload>(nslots * 8, 0, pay, nslots * 8);
  a.lists = lists;
  a.kp = kp;
  a.k = k;
  a.cap = cap;
  a.parts = dv.get<uint32_t>(tb * k * 4, 0xA5);
  a.live = dv.get<uint32_t>(tb * 4, 0xA5);
  a.slots = dv.get<uint32_t>(tb * k * 4, 0xA5);
  a.sync = dv.get<uint32_t>(16, 0xA5);
  a.rows = dv.get<uint32_t>((size_t)cap * 4, 0xA5);
  a.count = dv.get<uint32_t>(4, 0xA5);
  a.info = dv.get<uint32_t>(16, 0xA5);
  uint32_t *dKt = dv.get<uint32_t>(4, 0xA5), *dPicked = dv.get<uint32_t>((size_t)k * 4, 0xA5);
  vt::SketchRefineArgs ra{};
  ra.parts = a.parts;
  ra.slots = a.slots;
  ra.live = a.live;
  ra.thresh_blocks = (uint32_t)tb;
  ra.k = k;
  ra.pay = a.pay;
  ra.slots_total = (uint32_t)nslots;
  ra.X = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  ra.stride = stride;
  ra.q = dv.get<float>(ld * sizeof(float), 0, qpad.data(), ld * sizeof(float));
  ra.d = d;
  ra.metric = metric;
  ra.order = order;
  ra.kt_out = dKt;
  ra.picked = dPicked;
  a.kt_word = dKt;
  if (dv.err != hipSuccess) return dv.err;
  for (uint32_t r = 0; r < runs; ++r) {
    if ((dv.err = vt::launch_sketch_thresh(a, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = vt::launch_sketch_refine(ra, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = vt::launch_sketch_collect(a, dv.stream)) != hipSuccess) return dv.err;
    if (!dv.sync()) return dv.err;
    dv.back(parts + r * tb * k, a.parts, tb * k * 4) && dv.back(slots + r * tb * k, a.slots, tb * k * 4) && dv.back(kt + r, dKt, 4) &&
        dv.back(picked + (size_t)r * k, dPicked, (size_t)k * 4) && dv.back(rows + (size_t)r * cap, a.rows, (size_t)cap * 4) &&
        dv.back(count + r, a.count, 4) && dv.back(info + 4 * r, a.info, 16);
    if (dv.err != hipSuccess) return dv.err;
  }
  return dv.err;
}

}  // extern "C"
