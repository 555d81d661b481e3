// sketch_batch_probe.cpp -- test infrastructure (tests/test_gpu_sketch_batch_kernels.py): K1qm's group pass
// (vt_sketch_batch.hip) and group tail (vt_sketch.hip) launched on the caller's own arrays beside the lone pass and the lone
// tail they must agree with, so that a test can read back what no search returns: every query's lists, and every tail
// block's outcome, candidate rows and rescored block.  Built into libvt_sketch_batch_probe.so from vt_sketch.o,
// vt_sketch_batch.o and this file alone; the product library never sees it.
//
// As tests/sketch_l2_probe.cpp: every entry point takes and returns host arrays, owns its device buffers for the length of
// the call (hipMalloc, blocking copies, one stream, a synchronise before the copies back) and returns the hipError_t as an
// int.  Every size a kernel will index with is checked against the caller's buffer lengths first: hipErrorInvalidValue,
// nothing launched.
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

size_t vtb_image_bytes(uint32_t rows, uint32_t d) { return vt::sketch_bytes(rows, d); }
uint32_t vtb_compiled_group(uint32_t ng) { return vt::sketch_scan_multi_group(ng); }
size_t vtb_multi_lds_bytes(uint32_t d, uint32_t k, uint32_t group) { return vt::sketch_scan_multi_lds_bytes(d, k, group); }

// launch_sketch_build (with_xx = 0) or launch_sketch_build_xx over X[x_floats] (rows `stride` floats apart) into an image of
// rows_img rows pre-filled with 0xA5; *max_norm is the f64's bits, in and out.
int vtb_build(int with_xx, const float *X, size_t x_floats, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d,
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

// The group pass and, on the same device image, the lone pass for each query of the group.  qimg: [ng][2][ld8] (the probe
// pads it to the compiled group with zero images, as the host does); par: [ng][7] doubles {t1, t2, qn, eta, kerr, qq_lo,
// qq_hi} (t1 and t2 are floats widened).  multi_keys / multi_pay come back as [ng][blocks][k], lone_keys / lone_pay as
// [ng][lone_blocks][k] ({row, raw bits} payloads), all pre-filled with 0xA5.  lone_blocks = 0: the group pass alone.
int vtb_scan_both(const unsigned char *img, size_t img_bytes, uint32_t n, uint32_t d, int metric, const uint32_t *id_rank,
                  const unsigned char *qimg, size_t qimg_bytes, uint32_t ng, const double *par, uint32_t k, uint32_t blocks,
                  uint32_t lone_blocks, unsigned long long *multi_keys, uint32_t *multi_pay, unsigned long long *lone_keys,
                  uint32_t *lone_pay) {
  if (d == 0 || d > vt::kSketchMaxDim || n == 0 || k == 0 || k > (uint32_t)vt::kSmallK || blocks == 0 || blocks > 4096 ||
      lone_blocks > 4096 || ng < 2 || ng > (uint32_t)vt::kSketchMultiMax)
    return hipErrorInvalidValue;
  const uint32_t ld8 = vt::sketch_ld8(d), group = vt::sketch_scan_multi_group(ng);
  if (img_bytes != vt::sketch_bytes(n, d) || qimg_bytes != (size_t)ng * 2 * ld8 || !vt::sketch_scan_multi_lds_bytes(d, k, group))
    return hipErrorInvalidValue;
  const size_t slots = (size_t)ng * blocks * k, lone_slots = (size_t)ng * lone_blocks * k;
  Dev dv;
  unsigned char *dI = dv.get<unsigned char>(img_bytes, 0, img, img_bytes);
  unsigned char *dQ = dv.get<unsigned char>((size_t)group * 2 * ld8, 0, qimg, qimg_bytes);
  uint32_t *dR = id_rank ? dv.get<uint32_t>((size_t)n * 4, 0, id_rank, (size_t)n * 4) : nullptr;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0xA5);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0xA5);
  uint64_t *dLK = dv.get<uint64_t>(lone_slots * 8, 0xA5);
  vt::Payload *dLP = dv.get<vt::Payload>(lone_slots * 8, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  vt::SketchScanMultiArgs a{};
  a.img = dI;
  a.id_rank = dR;
  a.qimg = reinterpret_cast<const int8_t *>(dQ);
  a.n = n;
  a.d = d;
  a.nch = ld8 / 16;
  a.ng = ng;
  a.metric = metric;
  a.k = k;
  a.part_keys = dK;
  a.part_pay = dP;
  for (uint32_t g = 0; g < ng; ++g) {
    const double *p = par + 7 * g;
    a.t1[g] = (float)p[0];
    a.t2[g] = (float)p[1];
    a.qn[g] = p[2];
    a.eta[g] = p[3];
    a.kerr[g] = p[4];
    a.qq_lo[g] = p[5];
    a.qq_hi[g] = p[6];
  }
  dv.err = vt::launch_sketch_scan_multi(a, blocks, dv.stream);
  for (uint32_t g = 0; g < ng && lone_blocks && dv.err == hipSuccess; ++g) {
    vt::SketchScanArgs l{};
    l.img = dI;
    l.id_rank = dR;
    l.qimg = reinterpret_cast<const int8_t *>(dQ) + (size_t)g * 2 * ld8;
    l.n = n;
    l.d = d;
    l.nch = ld8 / 16;
    l.metric = metric;
    l.t1 = a.t1[g];
    l.t2 = a.t2[g];
    l.qn = a.qn[g];
    l.eta = a.eta[g];
    l.kerr = a.kerr[g];
    l.qq_lo = a.qq_lo[g];
    l.qq_hi = a.qq_hi[g];
    l.k = k;
    l.part_keys = dLK + (size_t)g * lone_blocks * k;
    l.part_pay = dLP + (size_t)g * lone_blocks * k;
    dv.err = vt::launch_sketch_scan(l, lone_blocks, dv.stream);
  }
  if (dv.sync())
    dv.back(multi_keys, dK, slots * 8) && dv.back(multi_pay, dP, slots * 8) && dv.back(lone_keys, dLK, lone_slots * 8) &&
        dv.back(lone_pay, dLP, lone_slots * 8);
  return dv.err;
}

// launch_sketch_tail_group over [ng][lists][kp] keys and payloads (group = 1) or launch_sketch_tail once per query on that
// query's slice (group = 0): the two must leave the same arrays.  X[n_rows][stride] are the f32 rows, q [ng][stride] the
// queries padded with zeros.  Back come, per query: rows[cap] (pre-filled with 0xA5), count, info[4], the status word after
// the launch, and the result block as {status, count} in res_head[2] and res_keys / res_rows / res_raw [k].
int vtb_tail(int group, const unsigned long long *keys, const uint32_t *pay, uint32_t ng, uint32_t lists, uint32_t kp, uint32_t k,
             uint32_t cap, const float *X, size_t stride, uint32_t n_rows, const float *q, const uint32_t *id_rank, uint32_t d,
             int metric, int order, uint32_t *rows, uint32_t *count, uint32_t *info, int *status_after, int *res_head,
             unsigned long long *res_keys, uint32_t *res_rows, float *res_raw) {
  if (lists == 0 || kp == 0 || k == 0 || k > kp || k > (uint32_t)vt::kMaxFusedK || cap == 0 || d == 0 || d > vt::kSketchMaxDim ||
      n_rows == 0 || ng == 0 || ng > (uint32_t)vt::kSketchMultiMax || (size_t)ng * lists * kp > (1u << 22))
    return hipErrorInvalidValue;
  const uint32_t ld = vt::padded_dim(d);
  if (stride % vt::kRowAlign || stride < ld) return hipErrorInvalidValue;
  const size_t slots = (size_t)ng * lists * kp;
  for (size_t i = 0; i < slots; ++i)  // every row a tail block may load lies in X
    if (keys[i] != vt::kEmptyKey && pay[2 * i] >= n_rows) return hipErrorInvalidValue;
  Dev dv;
  vt::SketchTailArgs a{};
  a.keys = dv.get<uint64_t>(slots * 8, 0, keys, slots * 8);
  a.pay = dv.get<vt::Payload>(slots * 8, 0, pay, slots * 8);
  a.lists = lists;
  a.kp = kp;
  a.k = k;
  a.cap = cap;
  a.rows = dv.get<uint32_t>((size_t)ng * cap * 4, 0xA5);
  a.count = dv.get<uint32_t>((size_t)ng * 4, 0xA5);
  a.info = dv.get<uint32_t>((size_t)ng * 16, 0xA5);
  a.X = dv.get<float>((size_t)n_rows * stride * 4, 0, X, (size_t)n_rows * stride * 4);
  a.stride = stride;
  a.q = dv.get<float>((size_t)ng * stride * 4, 0, q, (size_t)ng * stride * 4);
  a.id_rank = id_rank ? dv.get<uint32_t>((size_t)n_rows * 4, 0, id_rank, (size_t)n_rows * 4) : nullptr;
  a.d = d;
  a.metric = metric;
  a.order = order;
  a.status = dv.get<int>((size_t)ng * 4, 0);
  a.out = dv.get<vt::ResultBlock>((size_t)ng * sizeof(vt::ResultBlock), 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  if (group) {
    dv.err = vt::launch_sketch_tail_group(a, ng, stride, dv.stream);
  } else {
    for (uint32_t g = 0; g < ng && dv.err == hipSuccess; ++g) {
      vt::SketchTailArgs b = a;
      b.keys += (size_t)g * lists * kp;
      b.pay += (size_t)g * lists * kp;
      b.rows += (size_t)g * cap;
      b.count += g;
      b.info += 4 * g;
      b.q += (size_t)g * stride;
      b.status += g;
      b.out += g;
      dv.err = vt::launch_sketch_tail(b, dv.stream);
    }
  }
  if (!dv.sync()) return dv.err;
  std::vector<vt::ResultBlock> res(ng);
  if (!(dv.back(rows, a.rows, (size_t)ng * cap * 4) && dv.back(count, a.count, (size_t)ng * 4) && dv.back(info, a.info, (size_t)ng * 16) &&
        dv.back(status_after, a.status, (size_t)ng * 4) && dv.back(res.data(), a.out, (size_t)ng * sizeof(vt::ResultBlock))))
    return dv.err;
  for (uint32_t g = 0; g < ng; ++g) {
    res_head[2 * g] = res[g].status;
    res_head[2 * g + 1] = (int)res[g].count;
    for (uint32_t i = 0; i < k; ++i) {
      res_keys[(size_t)g * k + i] = res[g].e[i].key;
      res_rows[(size_t)g * k + i] = res[g].e[i].row;
      res_raw[(size_t)g * k + i] = res[g].e[i].raw;
    }
  }
  return dv.err;
}

}  // extern "C"
