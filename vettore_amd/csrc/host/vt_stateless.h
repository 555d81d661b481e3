// vt_stateless.h -- the entry points without an index handle: one session per device, handed out locked; the two-slot
// staged upload that MaxSim (vt_maxsim.h) and MUVERA (vt_muvera.h) feed their kernels through; and the four dense
// helpers themselves (vector_top_k, binary_top_k, normalize_l2, compress_sign_bits).
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
#pragma once

namespace {

// Two pinned staging blocks, two device buffers and a copy stream: a call's chunks go up through slots 0, 1, 0, ...
// while the consumer stream works on the slot before.  Each of the four ordering rules is one operation below; rules 1
// and 2 bind a slot once it has been used in the current call.  The buffers grow and stay, whichever family calls next.
struct UploadRing {
  hipStream_t copy = nullptr;
  hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  PinnedBuf<float> hX[2];
  PinnedBuf<uint32_t> hOff[2];
  DevBuf<float> dX[2];
  DevBuf<uint32_t> dOff[2];
  // The start of a call: stream and events on first use; then no upload of an earlier call (one that failed between two
  // chunks) is in flight and no slot counts as used.
  int open() {
    if (!copy) VT_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      if (!copied[b]) VT_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
      if (!consumed[b]) VT_HIP(hipEventCreateWithFlags(&consumed[b], hipEventDisableTiming));
      used[b] = false;
    }
    VT_HIP(hipStreamSynchronize(copy));
    return VT_OK;
  }
  // Rule 1: the host fills staging block b (hX[b], hOff[b]: once this returns) only after its previous upload is done.
  int reserve(int b, size_t floats, size_t offsets) {
    if (used[b]) VT_HIP(hipEventSynchronize(copied[b]));
    VT_TRY(hX[b].ensure(std::max<size_t>(floats, 1)));
    VT_TRY(hOff[b].ensure(offsets));
    VT_TRY(dX[b].ensure(std::max<size_t>(floats, 1)));
    return dOff[b].ensure(offsets);
  }
  // Rule 2: the copy stream overwrites device buffers b only after the consumer is done with what they held.
  int send(int b, size_t floats, size_t offsets) {
    if (used[b]) VT_HIP(hipStreamWaitEvent(copy, consumed[b], 0));
    VT_HIP(hipMemcpyAsync(dX[b].p, hX[b].p, floats * sizeof(float), hipMemcpyHostToDevice, copy));
    VT_HIP(hipMemcpyAsync(dOff[b].p, hOff[b].p, offsets * sizeof(uint32_t), hipMemcpyHostToDevice, copy));
    VT_HIP(hipEventRecord(copied[b], copy));
    used[b] = true;
    return VT_OK;
  }
  // Rule 3: before the consumer's first kernel that reads slot b.  Rule 4: after its last one.
  int wait_ready(int b, hipStream_t consumer) { VT_HIP(hipStreamWaitEvent(consumer, copied[b], 0)); return VT_OK; }
  int mark_consumed(int b, hipStream_t consumer) { VT_HIP(hipEventRecord(consumed[b], consumer)); return VT_OK; }
  ~UploadRing() {
    if (!copy) return;  // (no event without the stream)
    (void)hipStreamSynchronize(copy);
    for (hipEvent_t e : {copied[0], copied[1], consumed[0], consumed[1]})
      if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(copy);
  }
};

// What the consumers keep on the device besides the ring -- MaxSim (K9): per slot the norms and the running sums between
// query panels, per call the query, ranks, keys and first device error; MUVERA (K10): a call's table and slot lists, a chunk's rows.
struct MaxSimState {
  DevBuf<double> dNorm[2], dQNorm;
  DevBuf<float> dTotal[2], dQ;
  DevBuf<int> dStatus[2];
  DevBuf<uint32_t> dRank;
  DevBuf<uint64_t> dKeys;
  DevBuf<vt::Payload> dPay;
  DevBuf<unsigned long long> dFirst;
  PinnedBuf<unsigned long long> hFirst;
};
struct MuveraState {
  DevBuf<float> dTable, dFull, dFinal;
  DevBuf<uint32_t> dCounts, dSlotOff, dSlotList;
  DevBuf<int> dStatus;
  PinnedBuf<int> hStatus;
};

// Prepare rows (K14, vt_prepare.h): two chunks in flight, each with a pinned block and a device buffer for its rows
// (normalized in place on the device, so the block that went up is the block that comes down) and the same for its sign
// words; a stream per direction beside the context's; the first-refused word.  Everything grows and stays.
struct PrepareState {
  hipStream_t up = nullptr, down = nullptr;
  hipEvent_t uploaded[2] = {nullptr, nullptr}, computed[2] = {nullptr, nullptr}, landed[2] = {nullptr, nullptr};
  PinnedBuf<float> hX[2];
  PinnedBuf<uint64_t> hW[2];
  DevBuf<float> dX[2];
  DevBuf<uint64_t> dW[2];
  DevBuf<uint32_t> dFirst;
  PinnedBuf<uint32_t> hFirst;
  int open() {
    if (!up) VT_HIP(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    if (!down) VT_HIP(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b)
      for (hipEvent_t *e : {&uploaded[b], &computed[b], &landed[b]})
        if (!*e) VT_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    // nothing of an earlier call (one that failed between two chunks) is in flight
    VT_HIP(hipStreamSynchronize(up));
    VT_HIP(hipStreamSynchronize(down));
    VT_TRY(dFirst.ensure(1));
    return hFirst.ensure(1);
  }
  ~PrepareState() {
    for (hipStream_t s : {up, down})
      if (s) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : {uploaded[0], uploaded[1], computed[0], computed[1], landed[0], landed[1]})
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {up, down})
      if (s) (void)hipStreamDestroy(s);
  }
};

// What the stateless calls keep on one device (the ring and the states after the context: gone before its stream).
struct Stateless {
  Ctx ctx;
  UploadRing ring;
  MaxSimState maxsim;
  MuveraState muvera;
  PrepareState prepare;
  // (vector_top_k, binary_top_k, normalize_l2 and compress_sign_bits still allocate and free their own buffers per call)
};

// One session per device, one lock over all of them: a lease is the only way to a session and holds the lock while it lives.
struct StatelessLease { std::unique_lock<std::mutex> held; Stateless *s = nullptr; };
std::mutex g_stateless_mu;
std::unordered_map<int, std::unique_ptr<Stateless>> g_stateless;
int stateless_lease(int device, StatelessLease *out) {
  std::unique_lock<std::mutex> held(g_stateless_mu);
  std::unique_ptr<Stateless> &slot = g_stateless[device];
  if (!slot) {
    auto s = std::make_unique<Stateless>();
    VT_TRY(s->ctx.init(device));
    slot = std::move(s);
  }
  *out = StatelessLease{std::move(held), slot.get()};
  return slot->ctx.bind();
}

// Where the reference, walking a batch in order, stops: the smallest i whose check(i) is not VT_OK (`count` when there
// is none) and, in *status, what that row answered.  (On a large call the longest host step, so it is split over
// threads; the earliest failing row wins whichever thread finds it.  Below the grain it is the serial loop.)
template <class Check>
size_t first_refused(size_t count, Check check, int *status) {
  std::atomic<size_t> first_bad{count};
  parallel_for(count, 512, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi && i < first_bad.load(std::memory_order_relaxed); ++i)
      if (check(i) != VT_OK) {
        size_t cur = first_bad.load();
        while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {
        }
        break;
      }
  });
  const size_t good = first_bad.load();
  *status = good < count ? check(good) : VT_OK;
  return good;
}

// id_rank for an ad-hoc batch of ids (ties between equal ids: input order).
void ranks_for_ids(const char *ids, const size_t *id_off, size_t count, std::vector<uint32_t> &rank) {
  std::vector<uint32_t> order(count);
  for (size_t i = 0; i < count; ++i) order[i] = (uint32_t)i;
  auto view = [&](uint32_t i) { return std::pair<const char *, size_t>(ids + id_off[i], id_off[i + 1] - id_off[i]); };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    auto x = view(a), y = view(b);
    const size_t m = std::min(x.second, y.second);
    const int c = m ? std::memcmp(x.first, y.first, m) : 0;
    if (c) return c < 0;
    return x.second < y.second;
  });
  rank.resize(count);
  for (size_t i = 0; i < count; ++i) rank[order[i]] = (uint32_t)i;
}

int hits_from_batch(const char *ids, const size_t *id_off, const std::vector<vt::Entry> &entries, vt_hits **out) {
  auto h = std::make_unique<vt_hits>();
  for (const auto &e : entries) {
    h->ids.emplace_back(ids + id_off[e.row], id_off[e.row + 1] - id_off[e.row]);
    h->raw.push_back(e.raw);
    h->rank_key.push_back(rank_key_of(e.key));
  }
  *out = h.release();
  return VT_OK;
}

int vector_top_k(int device, size_t count, const char *ids, const size_t *id_off, const float *values, const size_t *value_off,
                 const float *query, size_t nq, int metric_code, size_t dimensions, size_t limit, vt_hits **out) {
  // nifs.rs:158-161: metric decode first, then search.rs:38-73
  if (metric_code < VT_L2 || metric_code > VT_JACCARD) return VT_ERR_UNKNOWN_METRIC;
  if (dimensions == 0 || dimensions > nq) return VT_ERR_PREFIX;
  VT_TRY(validate_finite(query, dimensions));
  // the reference walks the batch in order and stops at the first error;
  // rows before the first invalid one may still overflow and win the race
  int first_error = VT_OK;
  const size_t good = first_refused(count, [&](size_t i) {
    return dimensions > value_off[i + 1] - value_off[i] ? VT_ERR_DIMENSION : validate_finite(values + value_off[i], dimensions);
  }, &first_error);
  if (dimensions > 0x7fffffffu || vt::scan_lds_bytes((uint32_t)dimensions, 1) == 0)
    return fail(VT_ERR_UNSUPPORTED, "prefix dimension exceeds what the scan kernel stages in LDS");
  if (count > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 rows");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  std::vector<vt::Entry> entries;
  if (good > 0) {
    const uint32_t d = (uint32_t)dimensions, ld = vt::padded_dim(d);
    const uint32_t n = (uint32_t)good;
    const uint32_t cap = round_up_u32(n, vt::kTileRows);
    std::vector<float> packed((size_t)cap * ld, 0.0f);
    for (size_t i = 0; i < good; ++i) std::memcpy(&packed[i * ld], values + value_off[i], (size_t)d * sizeof(float));
    std::vector<uint32_t> rank;
    ranks_for_ids(ids, id_off, good, rank);
    DevBuf<float> dX;
    DevBuf<uint32_t> dRank;
    VT_TRY(dX.ensure(packed.size()));
    VT_TRY(dRank.ensure(n));
    VT_HIP(hipMemcpyAsync(dX.p, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, c.stream));
    VT_HIP(hipMemcpyAsync(dRank.p, rank.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    uint32_t qnz = 0;
    VT_TRY(upload_query(c, query, dimensions, &qnz));
    const size_t want = first_error == VT_OK ? limit : (size_t)1;  // only the overflow flag matters then
    const RowSet rows{dX.p, ld, dRank.p, n, metric_code, default_order()};
    if (metric_code == VT_COSINE) {
      VT_TRY(c.ensure_cand_lists(n));
      VT_HIP(vt::launch_cosine_rerank(cosine_rerank_args(rows, c, d), c.stream));
      // limit == 0 still has to surface "metric overflow": select one
      VT_TRY(collect_from_keys(c, c.dCandKeys.p, c.dCandPay.p, n, std::max<size_t>(want, 1), entries));
    } else {
      vt::ScanArgs j = scan_args(rows, c, d);
      j.q_nonzero = qnz;
      // limit == 0 still has to surface "metric overflow": scan for one hit
      VT_TRY(run_scan(c, j, std::max<size_t>(want, 1), entries, false));
    }
    if (limit == 0) entries.clear();
  }
  if (first_error != VT_OK) return first_error;
  return hits_from_batch(ids, id_off, entries, out);
}

int binary_top_k(int device, size_t count, const char *ids, const size_t *id_off, const uint64_t *words, const size_t *word_off,
                 const uint64_t *query, size_t nq, size_t dimensions, size_t limit, vt_hits **out) {
  // search.rs:82-84: the query is validated against itself first
  const size_t W = (dimensions + 63) / 64;
  if (dimensions == 0) return VT_ERR_DIMS_POSITIVE;
  if (nq != W) return VT_ERR_DIMENSION;
  for (size_t i = 0; i < count; ++i)
    if (word_off[i + 1] - word_off[i] != W) return VT_ERR_DIMENSION;
  if (count == 0 || limit == 0) return empty_hits(out);
  if (count > 0xFFFFFFF0ull || dimensions > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  const uint32_t n = (uint32_t)count;
  // K4 reads the tiled layout: [tile of 64 rows][word pair][row][2]
  const uint32_t pairs = (uint32_t)((W + 1) / 2);
  std::vector<uint64_t> packed(vt::hamming_matrix_words(n, (uint32_t)W), 0);
  for (size_t i = 0; i < count; ++i)
    for (size_t w = 0; w < W; ++w) packed[vt::hamming_word_index((uint32_t)i, (uint32_t)w, pairs)] = words[word_off[i] + w];
  std::vector<uint32_t> rank;
  ranks_for_ids(ids, id_off, count, rank);
  DevBuf<uint64_t> dBits, dQ;
  DevBuf<uint32_t> dRank;
  VT_TRY(dBits.ensure(packed.size()));
  std::vector<uint64_t> qwords(2 * (size_t)pairs, 0);  // (K4 reads whole word pairs: an odd count is padded with a zero word)
  std::copy(query, query + W, qwords.begin());
  VT_TRY(dQ.ensure(qwords.size()));
  VT_TRY(dRank.ensure(n));
  VT_HIP(hipMemcpyAsync(dBits.p, packed.data(), packed.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemcpyAsync(dQ.p, qwords.data(), qwords.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
  VT_HIP(hipMemcpyAsync(dRank.p, rank.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
  std::vector<vt::Entry> entries;
  VT_TRY(run_hamming(c, dBits.p, dQ.p, dRank.p, n, (uint32_t)dimensions, limit, entries, false));
  return hits_from_batch(ids, id_off, entries, out);
}

int normalize_l2(int device, size_t count, size_t d, const float *in, float *out) {
  // distances.rs:350-361: finiteness first
  VT_TRY(validate_finite(in, count * d));
  if (count == 0 || d == 0) return VT_OK;
  if (count > 0xFFFFFFF0ull || d > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  DevBuf<float> dIn, dOut;
  VT_TRY(dIn.ensure(count * d));
  VT_TRY(dOut.ensure(count * d));
  VT_HIP(hipMemcpyAsync(dIn.p, in, count * d * sizeof(float), hipMemcpyHostToDevice, c.stream));
  VT_HIP(vt::launch_normalize_l2(dIn.p, (uint32_t)count, (uint32_t)d, dOut.p, c.stream));
  VT_HIP(hipMemcpyAsync(out, dOut.p, count * d * sizeof(float), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  return VT_OK;
}

int compress_sign_bits(int device, size_t count, size_t d, const float *in, uint64_t *out) {
  if (count == 0 || d == 0) return VT_OK;
  if (count > 0xFFFFFFF0ull || d > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  const size_t W = (d + 63) / 64;
  DevBuf<float> dIn;
  DevBuf<uint64_t> dOut;
  VT_TRY(dIn.ensure(count * d));
  VT_TRY(dOut.ensure(count * W));
  VT_HIP(hipMemcpyAsync(dIn.p, in, count * d * sizeof(float), hipMemcpyHostToDevice, c.stream));
  VT_HIP(vt::launch_sign_pack(dIn.p, d, (uint32_t)count, (uint32_t)d, dOut.p, 0, c.stream));
  VT_HIP(hipMemcpyAsync(out, dOut.p, count * W * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  return VT_OK;
}

}  // namespace
