// select_probe.cpp -- test infrastructure (tests/test_gpu_select_kernels.py): the selection kernels of csrc/vt_select.hip
// (K3) -- the one-block radix select in its five launch forms, the spread select, the list sort, the cross-shard merge, the
// radix k-th passes and their collect -- launched one at a time on the caller's own arrays, so that a test can read back
// what no search returns: every byte of a result block, every listed (key, row, raw), every count, the status word.  Built
// into libvt_select_probe.so from vt_select.o and this file alone; the product library never sees it.
//
// As tests/panel_probe.cpp: every entry point takes and returns host arrays, owns its device buffers for the length of the
// call (hipMalloc, blocking copies, one stream, a synchronise before the copies back) and returns the hipError_t as an int.
// Everything a kernel will index is checked against the caller's lengths first: hipErrorInvalidValue, nothing launched.
// (What the launchers themselves refuse -- k = 0, k above the form's limit, a stride too narrow, a misaligned column, a
// pass out of range -- is left to them: the probe hands it on, and the launcher's answer comes back.)
// Output buffers are filled with 0xA5 before the launch: a write outside the contract shows.
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

constexpr uint64_t kMaxKeys = 1u << 20;
constexpr uint32_t kMaxQueries = 64, kMaxBlocks = 1024, kMaxWorld = 64;
constexpr uint32_t kHeaderBytes = 16;  // a result block's {status, count, pad[2]}

// the (row, raw) columns a test hands over as two u32 arrays, as the kernels read them
std::vector<vt::Payload> join(const uint32_t *rows, const uint32_t *raw_bits, uint64_t len) {
  std::vector<vt::Payload> pay(len ? len : 1);
  for (uint64_t i = 0; i < len; ++i) {
    pay[i].row = rows[i];
    std::memcpy(&pay[i].raw, &raw_bits[i], 4);
  }
  return pay;
}

void split(const std::vector<vt::Payload> &pay, uint32_t *rows, uint32_t *raw_bits) {
  for (size_t i = 0; i < pay.size(); ++i) {
    rows[i] = pay[i].row;
    std::memcpy(&raw_bits[i], &pay[i].raw, 4);
  }
}

// a key list and its payload columns of `len` entries, of which a launch reads `need`
bool list_ok(const uint64_t *keys, const uint32_t *rows, const uint32_t *raw, uint64_t len, uint64_t need) {
  return keys && rows && raw && len >= 1 && len <= kMaxKeys && need <= len;
}

}  // namespace

extern "C" {

uint32_t vsp_max_fused_k() { return (uint32_t)vt::kMaxFusedK; }
uint32_t vsp_sel_list_max() { return vt::kSelListMax; }
uint32_t vsp_sel_two_level_min() { return vt::kSelTwoLevelMin; }
uint32_t vsp_sel_groups() { return vt::kSelGroups; }
uint32_t vsp_radix_bins() { return vt::kRadixBins; }
uint32_t vsp_result_block_bytes() { return (uint32_t)sizeof(vt::ResultBlock); }
int vsp_status_retry() { return vt::kStatusRetry; }

// launch_select on keys / rows / raw[len], of which the launch is told `m`.  m_dev (null or one word): the list length
// decided on the device.  two_level != 0: the scratch lists are handed over, so that m >= kSelTwoLevelMin takes the
// two-level form; 0: scratch null, one level whatever m is.  status_io (null: dev_status null): the device's status word,
// *status_io before the launch, read back after it.  out[out_bytes] (out_bytes >= sizeof(ResultBlock)): the result block
// and whatever lies behind it, over its 0xA5 fill.
int vsp_select(const uint64_t *keys, const uint32_t *rows, const uint32_t *raw, uint64_t len, uint32_t m, uint32_t k, uint64_t lo_key,
               int has_lo, const uint32_t *m_dev, int two_level, int32_t *status_io, unsigned char *out, uint64_t out_bytes) {
  // (a block has room for kMaxFusedK entries: whatever k the launcher accepts fits)
  if (!list_ok(keys, rows, raw, len, m) || !out || out_bytes < sizeof(vt::ResultBlock) || out_bytes > (1u << 20)) return hipErrorInvalidValue;
  const std::vector<vt::Payload> pay = join(rows, raw, len);
  Dev dv;
  const uint64_t *dk = dv.get<uint64_t>(len * 8, 0, keys, len * 8);
  const vt::Payload *dp = dv.get<vt::Payload>(len * 8, 0, pay.data(), len * 8);
  const uint32_t *dm = m_dev ? dv.get<uint32_t>(4, 0, m_dev, 4) : nullptr;
  int *ds = status_io ? dv.get<int>(4, 0, status_io, 4) : nullptr;
  unsigned char *dout = dv.get<unsigned char>(out_bytes, 0xA5);
  const size_t slots = (size_t)vt::kSelGroups * vt::kMaxFusedK;
  uint64_t *sk = two_level ? dv.get<uint64_t>(slots * 8, 0xA5) : nullptr;
  vt::Payload *sp = two_level ? dv.get<vt::Payload>(slots * 8, 0xA5) : nullptr;
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_select(dk, dp, m, k, lo_key, has_lo, ds, reinterpret_cast<vt::ResultBlock *>(dout), sk, sp, dv.stream, dm);
  if (!dv.sync()) return dv.err;
  if (ds && !dv.back(status_io, ds, 4)) return dv.err;
  dv.back(out, dout, out_bytes);
  return dv.err;
}

// launch_select_list: the k <= kSelListMax best of keys[0 .. min(m, *m_dev)), unsorted and padded, into out_keys / out_rows /
// out_raw[out_len] (out_len >= k: what lies past k must keep its fill).
int vsp_select_list(const uint64_t *keys, const uint32_t *rows, const uint32_t *raw, uint64_t len, uint32_t m, const uint32_t *m_dev,
                    uint32_t k, uint64_t *out_keys, uint32_t *out_rows, uint32_t *out_raw, uint64_t out_len) {
  if (!list_ok(keys, rows, raw, len, m) || !out_keys || !out_rows || !out_raw || out_len < k || out_len > kMaxKeys) return hipErrorInvalidValue;
  const std::vector<vt::Payload> pay = join(rows, raw, len);
  Dev dv;
  const uint64_t *dk = dv.get<uint64_t>(len * 8, 0, keys, len * 8);
  const vt::Payload *dp = dv.get<vt::Payload>(len * 8, 0, pay.data(), len * 8);
  const uint32_t *dm = m_dev ? dv.get<uint32_t>(4, 0, m_dev, 4) : nullptr;
  uint64_t *ok = dv.get<uint64_t>(out_len * 8, 0xA5);
  vt::Payload *op = dv.get<vt::Payload>(out_len * 8, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_select_list(dk, dp, m, dm, k, ok, op, dv.stream);
  if (!dv.sync()) return dv.err;
  std::vector<vt::Payload> got(out_len);
  if (dv.back(out_keys, ok, out_len * 8) && dv.back(got.data(), op, out_len * 8)) split(got, out_rows, out_raw);
  return dv.err;
}

// launch_select_queries (m_dev null) or launch_select_lists (m_dev[nq]; spread on or off): nq lists `m` keys apart in
// keys / rows / raw[len], the blocks out_stride bytes apart in out[out_bytes].
int vsp_select_many(const uint64_t *keys, const uint32_t *rows, const uint32_t *raw, uint64_t len, uint32_t nq, uint32_t m,
                    const uint32_t *m_dev, int spread, uint32_t k, unsigned char *out, uint64_t out_bytes, uint32_t out_stride) {
  if (nq < 1 || nq > kMaxQueries || m < 1 || !list_ok(keys, rows, raw, len, (uint64_t)nq * m) || !out || out_bytes > (1u << 22) ||
      out_bytes < (uint64_t)nq * out_stride || out_stride < kHeaderBytes + (uint64_t)k * sizeof(vt::Entry))
    return hipErrorInvalidValue;
  const std::vector<vt::Payload> pay = join(rows, raw, len);
  Dev dv;
  const uint64_t *dk = dv.get<uint64_t>(len * 8, 0, keys, len * 8);
  const vt::Payload *dp = dv.get<vt::Payload>(len * 8, 0, pay.data(), len * 8);
  const uint32_t *dm = m_dev ? dv.get<uint32_t>((size_t)nq * 4, 0, m_dev, (size_t)nq * 4) : nullptr;
  unsigned char *dout = dv.get<unsigned char>(out_bytes, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = m_dev ? vt::launch_select_lists(dk, dp, nq, m, dm, k, dout, out_stride, dv.stream, spread != 0)
                 : vt::launch_select_queries(dk, dp, nq, m, k, dout, out_stride, dv.stream);
  if (!dv.sync()) return dv.err;
  dv.back(out, dout, out_bytes);
  return dv.err;
}

// launch_sort_list on keys / rows / raw[len], told `m`: head[2] = {status, count} and out[out_entries] entries of 16 bytes
// come back over their fill; *status_io as in vsp_select.
int vsp_sort_list(const uint64_t *keys, const uint32_t *rows, const uint32_t *raw, uint64_t len, uint32_t m, int32_t *status_io,
                  uint32_t *head, unsigned char *out, uint64_t out_entries) {
  if (!list_ok(keys, rows, raw, len, m) || !status_io || !head || !out || out_entries < m || out_entries > kMaxKeys) return hipErrorInvalidValue;
  const std::vector<vt::Payload> pay = join(rows, raw, len);
  Dev dv;
  const uint64_t *dk = dv.get<uint64_t>(len * 8, 0, keys, len * 8);
  const vt::Payload *dp = dv.get<vt::Payload>(len * 8, 0, pay.data(), len * 8);
  int *ds = dv.get<int>(4, 0, status_io, 4);
  vt::BigResultHeader *dh = dv.get<vt::BigResultHeader>(sizeof(vt::BigResultHeader), 0xA5);
  vt::Entry *de = dv.get<vt::Entry>(out_entries * sizeof(vt::Entry), 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_sort_list(dk, dp, m, ds, dh, de, dv.stream);
  if (!dv.sync()) return dv.err;
  if (dv.back(status_io, ds, 4) && dv.back(head, dh, sizeof(vt::BigResultHeader))) dv.back(out, de, out_entries * sizeof(vt::Entry));
  return dv.err;
}

// launch_merge_blocks over `world` result blocks block_bytes apart in blocks[blocks_len]: out[sizeof(ResultBlock)] and
// out_shard[shard_len] come back over their fill.  A block is read up to its k-th entry whatever its count says.
int vsp_merge_blocks(const unsigned char *blocks, uint64_t blocks_len, uint32_t world, uint32_t k, uint32_t block_bytes, unsigned char *out,
                     uint64_t out_bytes, uint32_t *out_shard, uint64_t shard_len) {
  if (!blocks || world < 1 || world > kMaxWorld || block_bytes % 16 || block_bytes < kHeaderBytes + (uint64_t)k * sizeof(vt::Entry) ||
      blocks_len < (uint64_t)world * block_bytes || !out || out_bytes != sizeof(vt::ResultBlock) || !out_shard || shard_len < k ||
      shard_len > 2 * (uint64_t)vt::kMaxFusedK)
    return hipErrorInvalidValue;
  Dev dv;
  const unsigned char *db = dv.get<unsigned char>(blocks_len, 0, blocks, blocks_len);
  unsigned char *dout = dv.get<unsigned char>(out_bytes, 0xA5);
  uint32_t *dsh = dv.get<uint32_t>(shard_len * 4, 0xA5);
  if (dv.err != hipSuccess) return dv.err;
  dv.err = vt::launch_merge_blocks(db, world, k, block_bytes, reinterpret_cast<vt::ResultBlock *>(dout), dsh, dv.stream);
  if (!dv.sync()) return dv.err;
  if (dv.back(out, dout, out_bytes)) dv.back(out_shard, dsh, shard_len * 4);
  return dv.err;
}

// The exact k-th key of the column keys[n] and the list of what lies at or below it: launch_radix_pass for pass = 0 ..
// passes - 1 (passes 3 or 6), then launch_radix_collect, on `blocks` blocks.  hist is zeroed as the host zeroes it;
// list_count holds garbage, which pass 0 must clear.  key_offset: the column starts that many keys into its buffer (1: a
// misaligned pointer, for the launcher to refuse).  raw (null or [n]): the payload column's raw bits (its rows are garbage:
// the collect writes positions).  only_pass >= 0: that one launch_radix_pass alone and its answer.  list_keys / list_rows /
// list_raw[list_len] (list_len >= cap), *count and *status come back; hist_out (null or [passes * kRadixBins]) too.
int vsp_radix(const uint64_t *keys, uint32_t n, uint32_t key_offset, uint32_t k, int passes, uint32_t blocks, uint32_t cap, const uint32_t *raw,
              int only_pass, uint64_t *list_keys, uint32_t *list_rows, uint32_t *list_raw, uint64_t list_len, uint32_t *count, int32_t *status,
              uint32_t *hist_out) {
  if (!keys || n < 1 || n > kMaxKeys || key_offset > 1 || (passes != 3 && passes != 6) || blocks < 1 || blocks > kMaxBlocks || cap < 1 ||
      !list_keys || !list_rows || !list_raw || list_len < cap || list_len > kMaxKeys || !count || !status)
    return hipErrorInvalidValue;
  Dev dv;
  vt::RadixArgs a{};
  uint64_t *col = dv.get<uint64_t>(((size_t)n + 2) * 8, 0xFF);
  if (col && dv.err == hipSuccess) dv.err = hipMemcpy(col + key_offset, keys, (size_t)n * 8, hipMemcpyHostToDevice);
  a.keys = col + key_offset;
  a.n = n;
  a.k = k;
  const size_t bins = (size_t)passes * vt::kRadixBins;
  a.hist = dv.get<uint32_t>(bins * 4, 0);
  a.list_count = dv.get<uint32_t>(4, 0xA5);
  a.list_keys = dv.get<uint64_t>(list_len * 8, 0xA5);
  a.list_pay = dv.get<vt::Payload>(list_len * 8, 0xA5);
  a.cap = cap;
  a.status = dv.get<int>(4, 0);
  if (raw) {
    std::vector<vt::Payload> pay(n);
    for (uint32_t i = 0; i < n; ++i) {
      pay[i].row = 0xDEAD0000u + i;
      std::memcpy(&pay[i].raw, &raw[i], 4);
    }
    a.pay_col = dv.get<vt::Payload>((size_t)n * 8, 0, pay.data(), (size_t)n * 8);
  }
  a.passes = passes;
  if (dv.err != hipSuccess) return dv.err;
  if (only_pass >= 0) {
    dv.err = vt::launch_radix_pass(a, only_pass, blocks, dv.stream);
  } else {
    for (int pass = 0; pass < passes && dv.err == hipSuccess; ++pass) dv.err = vt::launch_radix_pass(a, pass, blocks, dv.stream);
    if (dv.err == hipSuccess) dv.err = vt::launch_radix_collect(a, blocks, dv.stream);
  }
  if (dv.err != hipSuccess) {  // refused: nothing was launched (a pass is refused before the first launch or not at all)
    (void)hipStreamSynchronize(dv.stream);
    return dv.err;
  }
  if (!dv.sync()) return dv.err;
  std::vector<vt::Payload> got(list_len);
  if (dv.back(list_keys, a.list_keys, list_len * 8) && dv.back(got.data(), a.list_pay, list_len * 8) && dv.back(count, a.list_count, 4) &&
      dv.back(status, a.status, 4)) {
    split(got, list_rows, list_raw);
    if (hist_out) dv.back(hist_out, a.hist, bins * 4);
  }
  return dv.err;
}

}  // extern "C"
