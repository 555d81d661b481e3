// sketch_probe.cpp -- test infrastructure (tests/test_gpu_sketch_kernels.py): the sketch builders, the four sketch passes
// and the spread certification (vt_sketch.hip, vt_sketch_nibble.hip) launched one at a time on the caller's own
// arrays, so that a test can read back what no search returns: a sketch image, a row's interval words, Kt and the candidate
// set.  Built into libvt_sketch_probe.so from those two units and this file alone; the product library never sees it.
//
// Every entry point takes and returns host arrays, owns its device buffers for the length of the call (hipMalloc, blocking
// copies, one stream, a synchronise before the copies back) and returns the hipError_t as an int.  The launchers are called
// as host/vt_sketchsearch.h calls them; what that file computes on the way (the query's levels, the norms) is an input here.
// Every size a kernel will index with is checked against the caller's buffer lengths first: hipErrorInvalidValue, nothing
// launched.
#include "vt_device.h"

#include "host/vt_sketch5.h"

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

size_t image_bytes(int width, uint32_t rows, uint32_t d) {
  return width == 8   ? vt::sketch_bytes(rows, d)
         : width == 6 ? vt::sketch6_bytes(rows, d)
         : width == 5 ? vt::sketch5_bytes(rows, d)
                      : vt::sketch4_bytes(rows, d);
}
bool known(int width) { return width == 8 || width == 6 || width == 5 || width == 4; }
uint32_t block_lists(int width) { return width == 4 ? vt::kSketch4BlockLists : 1; }  // lists a block of the pass leaves

}  // namespace

extern "C" {

size_t vtp_image_bytes(int width, uint32_t rows, uint32_t d) { return known(width) ? image_bytes(width, rows, d) : 0; }
uint32_t vtp_thresh_blocks(uint32_t lists, uint32_t kp) { return vt::sketch_thresh_blocks(lists, kp); }
uint32_t vtp_block_lists(int width) { return known(width) ? block_lists(width) : 0; }

// launch_sketch*_build over X[x_floats] (rows `stride` floats apart) into an image of rows_img rows pre-filled with 0xA5;
// *max_norm is the f64's bits, in and out.
int vtp_build(int width, const float *X, size_t x_floats, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d,
              unsigned char *img, size_t img_bytes, unsigned long long *max_norm) {
  if (!known(width) || d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows || n_src > rows_img ||
      img_bytes != image_bytes(width, rows_img, d) || (n_src && (size_t)(n_src - 1) * stride + d > x_floats))
    return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  auto launch = width == 8   ? vt::launch_sketch_build
                : width == 6 ? vt::launch_sketch6_build
                : width == 5 ? vt::launch_sketch5_build
                             : vt::launch_sketch4_build;
  dv.err = launch(dX, stride, n_src, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch*_rows: the rows of list[count] of X patched into the caller's image (in and out).
int vtp_rows(int width, const float *X, size_t x_floats, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img,
             uint32_t d, unsigned char *img, size_t img_bytes, unsigned long long *max_norm) {
  if (!known(width) || d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows ||
      img_bytes != image_bytes(width, rows_img, d))
    return hipErrorInvalidValue;
  for (uint32_t i = 0; i < count; ++i)
    if (list[i] < rows_img && (size_t)list[i] * stride + d > x_floats) return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  uint32_t *dL = dv.get<uint32_t>((size_t)count * 4, 0, list, (size_t)count * 4);
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5, img, img_bytes);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  auto launch = width == 8   ? vt::launch_sketch_rows
                : width == 6 ? vt::launch_sketch6_rows
                : width == 5 ? vt::launch_sketch5_rows
                             : vt::launch_sketch4_rows;
  dv.err = launch(dX, stride, dL, count, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch*_scan with `blocks` blocks and lists of k over an image of n rows.  qimg: the query's levels as the pass
// reads them (width 8: [2][ld8] int8; else [3][ld8 / 8] dwords of nibbles), t: their scales (2 or 3).  keys, pay
// ({row, raw bits}) and, for the nibble widths, lo_words and hi_words come back as [blocks * vtp_block_lists(width)][k],
// pre-filled with 0xA5.  (Width 4 reads neither c3 nor w3.)
int vtp_scan(int width, const unsigned char *img, size_t img_bytes, uint32_t n, uint32_t d, int metric, const uint32_t *id_rank,
             const unsigned char *qimg, size_t qimg_bytes, const float *t, double qn, double eta, double kerr, double c3, double w3,
             uint32_t k, uint32_t blocks, unsigned long long *keys, uint32_t *pay, uint32_t *lo_words, uint32_t *hi_words) {
  if (!known(width) || d == 0 || d > vt::kSketchMaxDim || n == 0 || k == 0 || blocks == 0 || blocks > 4096) return hipErrorInvalidValue;
  const uint32_t ld8 = vt::sketch_ld8(d);
  if (img_bytes != image_bytes(width, n, d) || qimg_bytes != (width == 8 ? 2 * (size_t)ld8 : 3 * (size_t)ld8 / 2))
    return hipErrorInvalidValue;
  if (width != 8 && (!lo_words || !hi_words)) return hipErrorInvalidValue;
  const size_t slots = (size_t)blocks * block_lists(width) * k;
  Dev dv;
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0, img, img_bytes);
  unsigned char *dQ = dv.get<unsigned char>(qimg_bytes, 0, qimg, qimg_bytes);
  uint32_t *dR = id_rank ? dv.get<uint32_t>((size_t)n * 4, 0, id_rank, (size_t)n * 4) : nullptr;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0xA5);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0xA5);
  uint32_t *dLo = dv.get<uint32_t>(slots * 4, 0xA5), *dHi = dv.get<uint32_t>(slots * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  if (width == 8) {
    vt::SketchScanArgs a{};
    a.img = dI;
    a.id_rank = dR;
    a.qimg = reinterpret_cast<const int8_t *>(dQ);
    a.n = n;
    a.d = d;
    a.nch = ld8 / 16;
    a.metric = metric;
    a.t1 = t[0];
    a.t2 = t[1];
    a.qn = qn;
    a.eta = eta;
    a.kerr = kerr;
    a.k = k;
    a.part_keys = dK;
    a.part_pay = dP;
    dv.err = vt::launch_sketch_scan(a, blocks, dv.stream);
  } else {
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
    a.c3 = c3;
    a.w3 = w3;
    a.k = k;
    a.part_keys = dK;
    a.part_pay = dP;
    a.lo_words = dLo;
    a.hi_words = dHi;
    auto launch = width == 6 ? vt::launch_sketch6_scan : width == 5 ? vt::launch_sketch5_scan : vt::launch_sketch4_scan;
    dv.err = launch(a, blocks, dv.stream);
  }
  if (dv.sync() && dv.back(keys, dK, slots * 8) && dv.back(pay, dP, slots * 8) && width != 8)
    dv.back(lo_words, dLo, slots * 4) && dv.back(hi_words, dHi, slots * 4);
  return dv.err;
}

// launch_sketch_thresh then launch_sketch_collect over [lists][kp] word arrays and payloads, `runs` times on the same
// buffers; sync[] starts as sync_prefill[4] and is never touched between the runs.  Per run r: parts[r][tb * k],
// live[r][tb] (tb = vtp_thresh_blocks), rows[r][cap], count[r], info[r][4], sync[r][4] as the run left them.  rows[] and
// parts[] start as 0xA5 bytes.
int vtp_certify(const uint32_t *lo_words, const uint32_t *hi_words, const uint32_t *pay, uint32_t lists, uint32_t kp, uint32_t k,
                uint32_t cap, const uint32_t *sync_prefill, uint32_t runs, uint32_t *parts, uint32_t *live, uint32_t *rows,
                uint32_t *count, uint32_t *info, uint32_t *sync) {
  if (lists == 0 || kp == 0 || k == 0 || cap == 0 || runs == 0 || (size_t)lists * kp > (1u << 24)) return hipErrorInvalidValue;
  const size_t slots = (size_t)lists * kp, tb = vt::sketch_thresh_blocks(lists, kp);
  Dev dv;
  vt::SketchSpreadArgs a{};
  a.lo_words = dv.get<uint32_t>(slots * 4, 0, lo_words, slots * 4);
  a.hi_words = dv.get<uint32_t>(slots * 4, 0, hi_words, slots * 4);
  a.pay = dv.get<vt::Payload>(slots * 8, 0, pay, slots * 8);
  a.lists = lists;
  a.kp = kp;
  a.k = k;
  a.cap = cap;
  a.parts = dv.get<uint32_t>(tb * k * 4, 0xA5);
  a.live = dv.get<uint32_t>(tb * 4, 0xA5);
  a.sync = dv.get<uint32_t>(16, 0, sync_prefill, 16);
  a.rows = dv.get<uint32_t>((size_t)cap * 4, 0xA5);
  a.count = dv.get<uint32_t>(4, 0xA5);
  a.info = dv.get<uint32_t>(16, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  for (uint32_t r = 0; r < runs; ++r) {
    if ((dv.err = vt::launch_sketch_thresh(a, dv.stream)) != hipSuccess) return dv.err;
    if ((dv.err = vt::launch_sketch_collect(a, dv.stream)) != hipSuccess) return dv.err;
    if (!dv.sync()) return dv.err;
    dv.back(parts + r * tb * k, a.parts, tb * k * 4) && dv.back(live + r * tb, a.live, tb * 4) &&
        dv.back(rows + (size_t)r * cap, a.rows, (size_t)cap * 4) && dv.back(count + r, a.count, 4) &&
        dv.back(info + 4 * r, a.info, 16) && dv.back(sync + 4 * r, a.sync, 16);
    if (dv.err != hipSuccess) return dv.err;
  }
  return dv.err;
}

// ---- the host side's own query image (header-only: host/vt_sketch6.h, vt_sketch5.h) -----------------------------------
uint32_t vtp_level_words(uint32_t d) { return vt_host::sketch6_level_words(d); }
void vtp_query_levels(const float *q, uint32_t d, uint32_t *img, double *resid, float *t, double *ee) {
  vt_host::sketch6_query_levels(q, d, img, resid, t, ee);
}
void vtp_level_sums(const uint32_t *level, uint32_t lw, long long *pos, long long *neg, long long *l1) {
  int64_t p = 0, n = 0, l = 0;
  vt_host::sketch6_level_sums(level, lw, &p, &n, &l);
  *pos = p;
  *neg = n;
  *l1 = l;
}
void vtp_level_bound5(const uint32_t *level, uint32_t lw, float t, double *c, double *w) {
  vt_host::sketch5_level_bound(level, lw, t, c, w);
}

}  // extern "C"
