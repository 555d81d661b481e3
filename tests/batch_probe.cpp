// batch_probe.cpp -- test infrastructure (tests/test_gpu_batch_kernels.py): the matrix-core nomination kernels -- K2
// (vt_batch.hip), K2b (vt_batch_bf16.hip), K2s (vt_batch_shadow.hip) -- and the small kernels around them (query and row
// images, row norms, the two threshold kernels, the batched select) launched one at a time on the caller's own arrays, so
// that a test can read back what no search returns: every score, every nominated row, every count.  Built into
// libvt_batch_probe.so from vt_batch.o, vt_batch_bf16.o, vt_batch_shadow.o and this file alone; the product library never
// sees it.  The certificate's margin (host/vt_batchbound.h) is exported beside them: the tests take their tolerances from the
// function batch_group_finish judges with.
//
// As tests/sketch_batch_probe.cpp: every entry point takes and returns host arrays, owns its device buffers for the length
// of the call (hipMalloc, blocking copies, one stream, a synchronise before the copies back) and returns the hipError_t as
// an int.  Everything a kernel will index is checked against the caller's lengths first: hipErrorInvalidValue, nothing
// launched.  Output buffers are filled with 0xA5 before the launch: a write outside the contract shows.
#define VT_ENV_IMPLEMENTATION  // (this library's own copy of the settings table: csrc/vt_env.h -- K2s reads its ring depth there)
#include "vt_env.h"
#include "vt_device.h"
#include "host/vt_batchbound.h"

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

constexpr uint32_t kMaxLd = 4096, kMaxRows = 1u << 20, kMaxBlocks = 4096;
enum { kK2 = 0, kK2b = 1, kK2s = 2 };
enum { kPass = 0, kDense = 1, kMaxima = 2 };

bool ld_ok(uint32_t ld) { return ld >= 64 && ld <= kMaxLd && ld % 64 == 0; }
bool pad_ok(int kernel, uint32_t nq_pad) {
  return nq_pad == 64 || nq_pad == 128 || nq_pad == 256 || (kernel == kK2 && nq_pad == 32);
}
// X holds `rows` rows `stride` floats apart, each at least ld floats long and 256-B aligned
bool rows_ok(const float *X, size_t x_floats, size_t stride, uint32_t rows, uint32_t ld) {
  return X && rows >= 1 && rows <= kMaxRows && stride >= ld && stride % vt::kRowAlign == 0 && stride <= kMaxLd &&
         x_floats >= (size_t)rows * stride;
}
uint32_t tile_rows_of(int kernel) {
  return kernel == kK2 ? vt::batch_rows_per_block(32) : kernel == kK2b ? vt::batch_bf16_rows_per_block() : vt::batch_shadow_rows_per_block();
}

}  // namespace

extern "C" {

// ---- sizes and the margin ---------------------------------------------------------------------------------------------
uint32_t vbp_rows_per_block(int kernel) { return tile_rows_of(kernel); }
size_t vbp_q_image_bytes(int kernel, uint32_t ld) { return kernel == kK2b ? vt::batch_bf16_image_bytes(ld) : vt::batch_shadow_image_bytes(ld); }
size_t vbp_shadow_elems(uint32_t rows, uint32_t ld) { return vt::shadow_elems(rows, ld); }
size_t vbp_shadow_index(uint32_t row, uint32_t col, uint32_t ld) { return vt::shadow_index(row, col, ld); }
uint32_t vbp_sample_groups(uint32_t tiles) { return vt::batch_shadow_sample_groups(tiles); }
uint32_t vbp_bf16_pad(uint32_t nq) { return vt::batch_bf16_pad(nq); }
double vbp_eps(int l2_family, int bf16, uint32_t d, double qnorm, double xnorm) {
  return vt_host::batch_eps(l2_family != 0, bf16 != 0, d, qnorm, xnorm);
}
void vbp_bf16_terms(int l2_family, uint32_t d, double qnorm, double xnorm, double *out3) {
  const vt_host::BatchBf16Terms t = vt_host::batch_bf16_terms(l2_family != 0, d, qnorm, xnorm);
  out3[0] = t.rounding;
  out3[1] = t.accumulation;
  out3[2] = t.flush;
}
int vbp_magnitudes_ok(int bf16, double qnorm, double xnorm) { return vt_host::batch_magnitudes_ok(bf16 != 0, qnorm, xnorm) ? 1 : 0; }

// ---- images -----------------------------------------------------------------------------------------------------------
// launch_batch_q_image (kernel = 1) or launch_batch_q_image16 (kernel = 2) over Q[nq_pad][ld] into an image of
// vbp_q_image_bytes(kernel, ld) bytes.
int vbp_q_image(int kernel, const float *Q, size_t q_floats, uint32_t ld, uint32_t nq_pad, unsigned char *image, size_t image_bytes) {
  if ((kernel != kK2b && kernel != kK2s) || !ld_ok(ld) || !pad_ok(kernel, nq_pad) || !Q || q_floats != (size_t)nq_pad * ld || !image ||
      image_bytes != vbp_q_image_bytes(kernel, ld))
    return hipErrorInvalidValue;
  Dev dv;
  float *dQ = dv.get<float>(q_floats * 4, 0, Q, q_floats * 4);
  unsigned char *dI = dv.get<unsigned char>(image_bytes, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = kernel == kK2b ? vt::launch_batch_q_image(dQ, ld, nq_pad, dI, dv.stream) : vt::launch_batch_q_image16(dQ, ld, nq_pad, dI, dv.stream);
  if (dv.sync()) dv.back(image, dI, image_bytes);
  return dv.err;
}

// launch_shadow_build: rows [0, rows_src) of X into an image of rows_img rows (img_elems = rows_img * ld bf16 elements).
int vbp_shadow_build(const float *X, size_t x_floats, size_t stride, uint32_t rows_src, uint32_t rows_img, uint32_t ld,
                     unsigned short *img, size_t img_elems) {
  if (!ld_ok(ld) || rows_img == 0 || rows_img > kMaxRows || rows_img % vt::batch_shadow_rows_per_block() || rows_src > rows_img || !img ||
      img_elems != (size_t)rows_img * ld || (rows_src && !rows_ok(X, x_floats, stride, rows_src, ld)))
    return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * 4, 0, X, x_floats * 4);
  unsigned short *dI = dv.get<unsigned short>(img_elems * 2, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_shadow_build(dX, stride, rows_src, rows_img, ld, dI, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_elems * 2);
  return dv.err;
}

// launch_shadow_rows: the rows of list[count] (each below n_rows) patched into img (in and out).
int vbp_shadow_rows(const float *X, size_t x_floats, size_t stride, const uint32_t *list, uint32_t count, uint32_t n_rows, uint32_t ld,
                    unsigned short *img, size_t img_elems) {
  if (!ld_ok(ld) || !rows_ok(X, x_floats, stride, n_rows, ld) || !img || img_elems != vt::shadow_elems(n_rows, ld) || (count && !list) ||
      count > kMaxRows)
    return hipErrorInvalidValue;
  for (uint32_t i = 0; i < count; ++i)
    if (list[i] >= n_rows) return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * 4, 0, X, x_floats * 4);
  uint32_t *dL = dv.get<uint32_t>((size_t)count * 4, 0, list, (size_t)count * 4);
  unsigned short *dI = dv.get<unsigned short>(img_elems * 2, 0, img, img_elems * 2);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_shadow_rows(dX, stride, dL, count, ld, dI, dv.stream);
  if (dv.sync()) dv.back(img, dI, img_elems * 2);
  return dv.err;
}

// ---- row norms --------------------------------------------------------------------------------------------------------
// launch_row_sqnorms (list = null) or launch_row_sqnorms_rows over X[n][stride]'s first d columns; xnorm2[xnorm_len] and
// *max_bits (the f64 maximum's bit pattern) are in and out.
int vbp_row_sqnorms(const float *X, size_t x_floats, size_t stride, uint32_t n, uint32_t d, const uint32_t *list, uint32_t count,
                    float *xnorm2, size_t xnorm_len, unsigned long long *max_bits) {
  if (d == 0 || d > kMaxLd || n == 0 || n > kMaxRows || !X || stride < d || x_floats < (size_t)(n - 1) * stride + d || !xnorm2 ||
      xnorm_len < n || !max_bits || count > kMaxRows)
    return hipErrorInvalidValue;
  for (uint32_t i = 0; list && i < count; ++i)
    if (list[i] >= n) return hipErrorInvalidValue;
  Dev dv;
  float *dX = dv.get<float>(x_floats * 4, 0, X, x_floats * 4);
  float *dN = dv.get<float>(xnorm_len * 4, 0, xnorm2, xnorm_len * 4);
  unsigned long long *dM = dv.get<unsigned long long>(8, 0, max_bits, 8);
  uint32_t *dL = list ? dv.get<uint32_t>((size_t)count * 4, 0, list, (size_t)count * 4) : nullptr;
  if (dv.err != hipSuccess) return dv.err;
  dv.err = list ? vt::launch_row_sqnorms_rows(dX, stride, dL, count, d, dN, dM, dv.stream) : vt::launch_row_sqnorms(dX, stride, n, d, dN, dM, dv.stream);
  if (dv.sync()) dv.back(xnorm2, dN, xnorm_len * 4) && dv.back(max_bits, dM, 8);
  return dv.err;
}

// ---- the scores -------------------------------------------------------------------------------------------------------
// One launch of launch_batch_scores (kernel 0), launch_batch_scores_bf16 (1) or launch_batch_scores_shadow (2) in pass mode
// (mode 0) or dense mode (1), or of launch_batch_sample_maxima_shadow (kernel 2, mode 2).  Lengths are in elements of the
// array they belong to.  Pass mode: cand_count is zeroed before the launch as the host does, cand ({score, row} pairs,
// [nq_pad][cand_cap]) comes back over its 0xA5 fill.  Dense / maxima: sample[nq_pad][sample_rows] likewise.
struct VbpScores {
  int32_t kernel, mode;
  uint32_t ld, nq_pad, n, n_total, sample_stride, blocks, stages, sample_rows, cand_cap, pad_;
  const float *X;                // kernels 0 and 1: [n_total][stride]
  uint64_t x_floats, stride;
  const unsigned short *shadow;  // kernel 2: vbp_shadow_elems(n_total, ld) elements
  uint64_t shadow_elems;
  const float *Q;                // kernel 0: [nq_pad][ld]
  uint64_t q_floats;
  const unsigned char *qimage;   // kernels 1 and 2: vbp_q_image_bytes(kernel, ld) bytes
  uint64_t qimage_bytes;
  const float *xnorm2;           // null: dot family
  uint64_t xnorm_len;
  float *sample;
  uint64_t sample_len;
  const float *tau;
  uint64_t tau_len;
  uint32_t *cand;
  uint64_t cand_len;             // in {score, row} pairs
  uint32_t *cand_count;
  uint64_t count_len;
};

int vbp_scores(const VbpScores *p) {
  if (!p || p->kernel < kK2 || p->kernel > kK2s || p->mode < kPass || p->mode > kMaxima || (p->mode == kMaxima && p->kernel != kK2s))
    return hipErrorInvalidValue;
  const bool dense = p->mode != kPass;
  if (!ld_ok(p->ld) || !pad_ok(p->kernel, p->nq_pad) || p->n_total < 1 || p->n_total > kMaxRows || p->n < 1 || p->n > kMaxRows ||
      p->blocks < 1 || p->blocks > kMaxBlocks)
    return hipErrorInvalidValue;
  // every tile the launch visits starts below n_total (K2 and K2b clamp their loads to n_total - 1 RELATIVE to the tile's
  // first row; K2s reads the tile's KiBs of an image of round_up(n_total, 256) rows)
  const uint32_t tile_rows = tile_rows_of(p->kernel);
  const uint64_t tiles = ((uint64_t)p->n + tile_rows - 1) / tile_rows;
  const uint64_t tile_step = dense ? p->sample_stride : 1;
  if (tile_step < 1 || (tiles - 1) * tile_step * tile_rows >= p->n_total) return hipErrorInvalidValue;
  if (p->kernel == kK2s) {
    if (!p->shadow || p->shadow_elems != vt::shadow_elems(p->n_total, p->ld) || (p->stages != 4 && p->stages != 5)) return hipErrorInvalidValue;
  } else if (!rows_ok(p->X, p->x_floats, p->stride, p->n_total, p->ld)) {
    return hipErrorInvalidValue;
  }
  if (p->kernel == kK2) {
    if (!p->Q || p->q_floats != (uint64_t)p->nq_pad * p->ld) return hipErrorInvalidValue;
  } else if (!p->qimage || p->qimage_bytes != vbp_q_image_bytes(p->kernel, p->ld)) {
    return hipErrorInvalidValue;
  }
  // the epilogues read 16 or 32 norms from any sub-tile that starts below n_total
  if (p->xnorm2 && p->xnorm_len < ((uint64_t)p->n_total + 255) / 256 * 256) return hipErrorInvalidValue;
  if (dense) {
    const uint64_t slots = p->mode == kMaxima ? vt::batch_shadow_sample_groups((uint32_t)tiles) : tiles * tile_rows;
    if (!p->sample || p->sample_rows < slots || p->sample_len != (uint64_t)p->nq_pad * p->sample_rows) return hipErrorInvalidValue;
  } else {
    if (!p->tau || p->tau_len != p->nq_pad || !p->cand_count || p->count_len != p->nq_pad || p->cand_cap < 1 || !p->cand ||
        p->cand_len != (uint64_t)p->nq_pad * p->cand_cap)
      return hipErrorInvalidValue;
  }
  Dev dv;
  vt::BatchScoreArgs a{};
  if (p->kernel == kK2s) {
    a.Xshadow = dv.get<unsigned short>(p->shadow_elems * 2, 0, p->shadow, p->shadow_elems * 2);
  } else {
    a.X = dv.get<float>(p->x_floats * 4, 0, p->X, p->x_floats * 4);
    a.stride = p->stride;
  }
  if (p->kernel == kK2) a.Q = dv.get<float>(p->q_floats * 4, 0, p->Q, p->q_floats * 4);
  else a.Qimage = dv.get<unsigned char>(p->qimage_bytes, 0, p->qimage, p->qimage_bytes);
  a.ld = p->ld;
  a.nq_pad = p->nq_pad;
  a.n = p->n;
  a.n_total = p->n_total;
  a.stages = p->stages;
  if (p->xnorm2) a.xnorm2 = dv.get<float>(p->xnorm_len * 4, 0, p->xnorm2, p->xnorm_len * 4);
  if (dense) {
    a.sample_stride = p->sample_stride;
    a.sample = dv.get<float>(p->sample_len * 4, 0xA5);
    a.sample_rows = p->sample_rows;
  } else {
    a.tau = dv.get<float>(p->tau_len * 4, 0, p->tau, p->tau_len * 4);
    a.cand = dv.get<vt::BatchCand>(p->cand_len * 8, 0xA5);
    a.cand_count = dv.get<uint32_t>(p->count_len * 4, 0);
    a.cand_cap = p->cand_cap;
  }
  if (dv.err != hipSuccess) return dv.err;
  if (p->mode == kMaxima) dv.err = vt::launch_batch_sample_maxima_shadow(a, p->blocks, dv.stream);
  else if (p->kernel == kK2) dv.err = vt::launch_batch_scores(a, dense, p->blocks, dv.stream);
  else if (p->kernel == kK2b) dv.err = vt::launch_batch_scores_bf16(a, dense, p->blocks, dv.stream);
  else dv.err = vt::launch_batch_scores_shadow(a, dense, p->blocks, dv.stream);
  if (!dv.sync()) return dv.err;
  if (dense) dv.back(p->sample, a.sample, p->sample_len * 4);
  else dv.back(p->cand, a.cand, p->cand_len * 8) && dv.back(p->cand_count, a.cand_count, p->count_len * 4);
  return dv.err;
}

// ---- thresholds -------------------------------------------------------------------------------------------------------
// launch_sample_tau (groups = 0) or launch_sample_tau_groups (groups = 1) over sample[nq][sample_rows]; tau[nq] comes back
// over its 0xA5 fill.
int vbp_sample_tau(int groups, const float *sample, size_t sample_len, uint32_t sample_rows, uint32_t nq, uint32_t nq_real, uint32_t rank,
                   float *tau) {
  // sample_tau_kernel keeps 64 values per thread of 1 024 in registers; sample_tau_groups_kernel 32 per lane of a wave
  const uint32_t most = groups ? 2048u : 65536u;
  if (!sample || !tau || sample_rows < 1 || sample_rows > most || nq < 1 || nq > 4096 || nq_real > nq || rank < 1 ||
      sample_len != (size_t)nq * sample_rows)
    return hipErrorInvalidValue;
  Dev dv;
  float *dS = dv.get<float>(sample_len * 4, 0, sample, sample_len * 4);
  float *dT = dv.get<float>((size_t)nq * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = groups ? vt::launch_sample_tau_groups(dS, sample_rows, nq, nq_real, rank, dT, dv.stream)
                  : vt::launch_sample_tau(dS, sample_rows, nq, nq_real, rank, dT, dv.stream);
  if (dv.sync()) dv.back(tau, dT, (size_t)nq * 4);
  return dv.err;
}

// ---- the batched select -----------------------------------------------------------------------------------------------
// launch_batch_select over keys / pay [nq][m] ({row, raw bits} payloads): out_keys / out_rows / out_raw [nq][k] and
// out_count[nq] come back over a 0xA5 fill.  with_export: the BatchExport words too -- cand_count[nq] and tau[nq] (tau may be
// null) are copied to cand_count_out / tau_out (0xA5-filled first), status_in goes to *status_out and *status_after is the
// device's status word after the launch.
int vbp_batch_select(const unsigned long long *keys, const uint32_t *pay, uint32_t nq, uint32_t m, uint32_t k, unsigned long long *out_keys,
                     uint32_t *out_rows, uint32_t *out_raw, uint32_t *out_count, int with_export, const uint32_t *cand_count, const float *tau,
                     int status_in, uint32_t *cand_count_out, uint32_t *tau_out, int *status_out, int *status_after) {
  if (!keys || !pay || nq < 1 || nq > 4096 || m < 1 || m > 4096 || k < 1 || k > 4096 || !out_keys || !out_rows || !out_raw || !out_count ||
      (with_export && (!cand_count || !cand_count_out || !tau_out || !status_out || !status_after)))
    return hipErrorInvalidValue;
  const size_t slots = (size_t)nq * m, outs = (size_t)nq * k;
  Dev dv;
  uint64_t *dK = dv.get<uint64_t>(slots * 8, 0, keys, slots * 8);
  vt::Payload *dP = dv.get<vt::Payload>(slots * 8, 0, pay, slots * 8);
  vt::Entry *dO = dv.get<vt::Entry>(outs * sizeof(vt::Entry), 0xA5);
  uint32_t *dC = dv.get<uint32_t>((size_t)nq * 4, 0xA5);
  vt::BatchExport ex{};
  if (with_export) {
    ex.cand_count = dv.get<uint32_t>((size_t)nq * 4, 0, cand_count, (size_t)nq * 4);
    ex.cand_count_out = dv.get<uint32_t>((size_t)nq * 4, 0xA5);
    ex.tau = tau ? dv.get<float>((size_t)nq * 4, 0, tau, (size_t)nq * 4) : nullptr;
    ex.tau_out = dv.get<float>((size_t)nq * 4, 0xA5);
    ex.status = dv.get<int>(4, 0, &status_in, 4);
    ex.status_out = dv.get<int>(4, 0xA5);
  }
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_batch_select(dK, dP, nq, m, k, dO, dC, dv.stream, with_export ? &ex : nullptr);
  if (!dv.sync()) return dv.err;
  std::vector<vt::Entry> res(outs);
  if (!(dv.back(res.data(), dO, outs * sizeof(vt::Entry)) && dv.back(out_count, dC, (size_t)nq * 4))) return dv.err;
  for (size_t i = 0; i < outs; ++i) {
    out_keys[i] = res[i].key;
    out_rows[i] = res[i].row;
    std::memcpy(&out_raw[i], &res[i].raw, 4);
  }
  if (with_export)
    dv.back(cand_count_out, ex.cand_count_out, (size_t)nq * 4) && dv.back(tau_out, ex.tau_out, (size_t)nq * 4) &&
        dv.back(status_out, ex.status_out, 4) && dv.back(status_after, ex.status, 4);
  return dv.err;
}

}  // extern "C"
