// sketch_l2_probe.cpp -- test infrastructure (tests/test_gpu_sketch_l2_kernels.py): the int8 sketch's builders with and
// without xx, its pass in either metric family and its one-block tail (vt_sketch.hip) launched one at a time on the
// caller's own arrays, so that a test can read back what no search returns: a sketch image, a row's two words, the tail's
// outcome, candidate set and rescored block.  Built into libvt_sketch_l2_probe.so from vt_sketch.o and this file alone; the
// product library never sees it.
//
// Every entry point takes and returns host arrays, owns its device buffers for the length of the call (hipMalloc, blocking
// copies, one stream, a synchronise before the copies back) and returns the hipError_t as an int.  The launchers are called
// as host/vt_sketchsearch.h calls them; what that file computes on the way (the query's levels, the norms) is an input here.
// Every size a kernel will index with is checked against the caller's buffer lengths first: hipErrorInvalidValue, nothing
// launched.
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

size_t vtl_image_bytes(uint32_t rows, uint32_t d) { return vt::sketch_bytes(rows, d); }

// launch_sketch_build (with_xx = 0) or launch_sketch_build_xx over X[x_floats] (rows `stride` floats apart) into an image of
// rows_img rows pre-filled with 0xA5; *max_norm is the f64's bits, in and out.
int vtl_build(int with_xx, const float *X, size_t x_floats, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d,
              unsigned char *img, size_t img_bytes, unsigned long long *max_norm) {
  if (d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows || n_src > rows_img ||
      img_bytes != vt::sketch_bytes(rows_img, d) || (n_src && (size_t)(n_src - 1) * stride + d > x_floats))
    return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = (with_xx ? vt::launch_sketch_build_xx : vt::launch_sketch_build)(dX, stride, n_src, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch_rows / launch_sketch_rows_xx: the rows of list[count] of X patched into the caller's image (in and out).
int vtl_rows(int with_xx, const float *X, size_t x_floats, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img,
             uint32_t d, unsigned char *img, size_t img_bytes, unsigned long long *max_norm) {
  if (d == 0 || d > vt::kSketchMaxDim || rows_img % vt::kSketchTileRows || img_bytes != vt::sketch_bytes(rows_img, d))
    return hipErrorInvalidValue;
  for (uint32_t i = 0; i < count; ++i)
    if (list[i] < rows_img && (size_t)list[i] * stride + d > x_floats) return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * sizeof(float), 0, X, x_floats * sizeof(float));
  uint32_t *dL = dv.get<uint32_t>((size_t)count * 4, 0, list, (size_t)count * 4);
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0xA5, img, img_bytes);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_norm, 8);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = (with_xx ? vt::launch_sketch_rows_xx : vt::launch_sketch_rows)(dX, stride, dL, count, rows_img, d, dI, dM, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_bytes) && dv.back(max_norm, dM, 8);
  return dv.err;
}

// launch_sketch_scan with `blocks` blocks and lists of k over an image of n rows, in `metric` (either family).  qimg: the
// query's two int8 levels [2][ld8], t: their scales.  keys and pay ({row, raw bits}) come back as [blocks][k], pre-filled
// with 0xA5.
int vtl_scan(const unsigned char *img, size_t img_bytes, uint32_t n, uint32_t d, int metric, const uint32_t *id_rank,
             const unsigned char *qimg, size_t qimg_bytes, const float *t, double qn, double eta, double kerr, double qq_lo,
             double qq_hi, uint32_t k, uint32_t blocks, unsigned long long *keys, uint32_t *pay) {
  if (d == 0 || d > vt::kSketchMaxDim || n == 0 || k == 0 || blocks == 0 || blocks > 4096) return hipErrorInvalidValue;
  const uint32_t ld8 = vt::sketch_ld8(d);
  if (img_bytes != vt::sketch_bytes(n, d) || qimg_bytes != 2 * (size_t)ld8) return hipErrorInvalidValue;
  const size_t slots = (size_t)blocks * k;
  Dev dv;
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0, img, img_bytes);
  unsigned char *dQ = dv.get<unsigned char>(qimg_bytes, 0, qimg, qimg_bytes);
  uint32_t *dR = id_rank ? dv.get<uint32_t>((size_t)n * 4, 0, id_rank, (size_t)n * 4) : nullptr;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0xA5);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
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
  a.qq_lo = qq_lo;
  a.qq_hi = qq_hi;
  a.k = k;
  a.part_keys = dK;
  a.part_pay = dP;
  dv.err = vt::launch_sketch_scan(a, blocks, dv.stream);
  if (dv.sync()) dv.back(keys, dK, slots * 8) && dv.back(pay, dP, slots * 8);
  return dv.err;
}

// launch_sketch_tail over [lists][kp] keys and payloads as a pass left them.  X[n_rows][stride] are the f32 rows (stride a
// multiple of 64 floats, at least padded_dim(d)), q the query padded with zeros to padded_dim(d) floats.  Back come rows[cap]
// (pre-filled with 0xA5), *count, info[4], the device's status word after the launch, and the result block as
// {status, count} in res_head[2] and res_keys / res_rows / res_raw [k].
int vtl_tail(const unsigned long long *keys, const uint32_t *pay, uint32_t lists, uint32_t kp, uint32_t k, uint32_t cap,
             const float *X, size_t stride, uint32_t n_rows, const float *q, const uint32_t *id_rank, uint32_t d, int metric,
             int order, uint32_t *rows, uint32_t *count, uint32_t *info, int *status_after, int *res_head,
             unsigned long long *res_keys, uint32_t *res_rows, float *res_raw) {
  if (lists == 0 || kp == 0 || k == 0 || k > kp || k > (uint32_t)vt::kMaxFusedK || cap == 0 || d == 0 || d > vt::kSketchMaxDim ||
      n_rows == 0 || (size_t)lists * kp > (1u << 22))
    return hipErrorInvalidValue;
  const uint32_t ld = vt::padded_dim(d);
  if (stride % vt::kRowAlign || stride < ld) return hipErrorInvalidValue;
  const size_t slots = (size_t)lists * kp;
  for (size_t i = 0; i < slots; ++i)  // every row the tail may load lies in X
    if (keys[i] != vt::kEmptyKey && pay[2 * i] >= n_rows) return hipErrorInvalidValue;
  Dev dv;
  vt::SketchTailArgs a{};
  a.keys = dv.get<uint64_t>(slots * 8, 0, keys, slots * 8);
  a.pay = dv.get<vt::Payload>(slots * 8, 0, pay, slots * 8);
  a.lists = lists;
  a.kp = kp;
  a.k = k;
  a.cap = cap;
  a.rows = dv.get<uint32_t>((size_t)cap * 4, 0xA5);
  a.count = dv.get<uint32_t>(4, 0xA5);
  a.info = dv.get<uint32_t>(16, 0xA5);
  a.X = dv.get<float>((size_t)n_rows * stride * 4, 0, X, (size_t)n_rows * stride * 4);
  a.stride = stride;
  a.q = dv.get<float>((size_t)ld * 4, 0, q, (size_t)ld * 4);
  a.id_rank = id_rank ? dv.get<uint32_t>((size_t)n_rows * 4, 0, id_rank, (size_t)n_rows * 4) : nullptr;
  a.d = d;
  a.metric = metric;
  a.order = order;
  a.status = dv.get<int>(4, 0);
  a.out = dv.get<vt::ResultBlock>(sizeof(vt::ResultBlock), 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_sketch_tail(a, dv.stream);
  if (!dv.sync()) return dv.err;
  std::vector<vt::ResultBlock> res(1);
  if (!(dv.back(rows, a.rows, (size_t)cap * 4) && dv.back(count, a.count, 4) && dv.back(info, a.info, 16) &&
        dv.back(status_after, a.status, 4) && dv.back(res.data(), a.out, sizeof(vt::ResultBlock))))
    return dv.err;
  res_head[0] = res[0].status;
  res_head[1] = (int)res[0].count;
  for (uint32_t i = 0; i < k; ++i) {
    res_keys[i] = res[0].e[i].key;
    res_rows[i] = res[0].e[i].row;
    res_raw[i] = res[0].e[i].raw;
  }
  return dv.err;
}

}  // extern "C"
