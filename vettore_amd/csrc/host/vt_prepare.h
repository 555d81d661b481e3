// vt_prepare.h -- prepare rows (K14): what Collection.prepare_embedding does per record (collection.ex:921-946 --
// validate, normalize in one of the four modes of distances.rs:350-410, take the sign bits of the result) for a batch.
// The host form streams its rows through the session's pooled buffers in chunks; the device form runs the kernel on
// rows that already live in HBM.  vt_normalize_zscore / vt_normalize_minmax are the host form without words.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
#pragma once

namespace {

static_assert(VT_NORM_NONE == vt::kPrepNone && VT_NORM_L2 == vt::kPrepL2 && VT_NORM_ZSCORE == vt::kPrepZscore &&
              VT_NORM_MINMAX == vt::kPrepMinmax, "the ABI's modes are the kernel's");

constexpr size_t kPrepareChunkBytes = (size_t)32 << 20;  // rows per chunk: this many bytes of them, at least one row

// (the one place the chunk size can be shrunk, and only in the hooks build: the chunk-boundary test)
inline size_t prepare_chunk_rows(size_t d) {
  const long forced = vt::env::get(vt::env::TEST_PREPARE_CHUNK_ROWS);
  if (forced > 0) return (size_t)forced;
  return std::max<size_t>(1, kPrepareChunkBytes / (d * sizeof(float)));
}

// The host form.  Order: mode, then finiteness of every row on the host (status 3 and the smallest refused row, nothing
// written, no device touched), then the chunks.  Chunk k goes through slot k % 2:
//   host copy into the slot's pinned block -> upload (stream `up`) -> kernel, in place (the context's stream) ->
//   download into the same pinned block (stream `down`) -> host copy out,
// and the host copy out of chunk k happens only when slot k % 2 is needed again (or at the end), so that chunk k + 1
// uploads while chunk k computes and chunk k - 1 comes down.
int prepare_rows(int device, int mode, size_t count, size_t d, const float *in, float *out, uint64_t *words,
                 size_t *first_bad) {
  if (mode < VT_NORM_NONE || mode > VT_NORM_MINMAX) return VT_ERR_ARGUMENT;
  if (first_bad) *first_bad = count;
  int refused_with = VT_OK;
  const size_t good = first_refused(count, [&](size_t i) { return validate_finite(in + i * d, d); }, &refused_with);
  if (good < count) {
    if (first_bad) *first_bad = good;
    return refused_with;
  }
  if (count == 0 || d == 0) return VT_OK;
  if (count > 0xFFFFFFF0ull || d > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  PrepareState &p = lease.s->prepare;
  VT_TRY(p.open());
  const size_t W = (d + 63) / 64;
  const size_t chunk = std::min(prepare_chunk_rows(d), count);
  VT_HIP(hipMemsetAsync(p.dFirst.p, 0xff, sizeof(uint32_t), c.stream));

  size_t begin[2] = {0, 0}, rows_in[2] = {0, 0};  // what each slot holds
  // chunk in slot b has landed in its pinned block: hand it to the caller
  auto drain = [&](int b) -> int {
    if (rows_in[b] == 0) return VT_OK;
    VT_HIP(hipEventSynchronize(p.landed[b]));
    const size_t r0 = begin[b], nr = rows_in[b];
    parallel_for(nr * d, (size_t)1 << 18, [&](size_t lo, size_t hi) {
      std::memcpy(out + r0 * d + lo, p.hX[b].p + lo, (hi - lo) * sizeof(float));
    });
    if (words) std::memcpy(words + r0 * W, p.hW[b].p, nr * W * sizeof(uint64_t));
    rows_in[b] = 0;
    return VT_OK;
  };
  int k = 0;
  for (size_t r0 = 0; r0 < count; r0 += chunk, ++k) {
    const int b = k & 1;
    const size_t nr = std::min(chunk, count - r0);
    VT_TRY(drain(b));
    VT_TRY(p.hX[b].ensure(chunk * d));
    VT_TRY(p.dX[b].ensure(chunk * d));
    if (words) {
      VT_TRY(p.hW[b].ensure(chunk * W));
      VT_TRY(p.dW[b].ensure(chunk * W));
    }
    parallel_for(nr * d, (size_t)1 << 18, [&](size_t lo, size_t hi) {
      std::memcpy(p.hX[b].p + lo, in + r0 * d + lo, (hi - lo) * sizeof(float));
    });
    VT_HIP(hipMemcpyAsync(p.dX[b].p, p.hX[b].p, nr * d * sizeof(float), hipMemcpyHostToDevice, p.up));
    VT_HIP(hipEventRecord(p.uploaded[b], p.up));
    VT_HIP(hipStreamWaitEvent(c.stream, p.uploaded[b], 0));
    vt::PrepareArgs a{};
    a.in = p.dX[b].p;
    a.ld_in = d;
    a.out = p.dX[b].p;
    a.ld_out = d;
    a.words = words ? p.dW[b].p : nullptr;
    a.first_refused = p.dFirst.p;
    a.n = (uint32_t)nr;
    a.d = (uint32_t)d;
    VT_HIP(vt::launch_prepare_rows(a, mode, c.stream));
    VT_HIP(hipEventRecord(p.computed[b], c.stream));
    VT_HIP(hipStreamWaitEvent(p.down, p.computed[b], 0));
    VT_HIP(hipMemcpyAsync(p.hX[b].p, p.dX[b].p, nr * d * sizeof(float), hipMemcpyDeviceToHost, p.down));
    if (words) VT_HIP(hipMemcpyAsync(p.hW[b].p, p.dW[b].p, nr * W * sizeof(uint64_t), hipMemcpyDeviceToHost, p.down));
    VT_HIP(hipEventRecord(p.landed[b], p.down));
    begin[b] = r0;
    rows_in[b] = nr;
  }
  // the older chunk first
  VT_TRY(drain(k & 1));
  VT_TRY(drain((k + 1) & 1));
  // (the host has checked every row: the kernel refuses none)
  VT_HIP(hipMemcpyAsync(p.hFirst.p, p.dFirst.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  if (*p.hFirst.p != vt::kPrepNoRow) return fail(VT_ERR_DEVICE, "prepare rows: the kernel refused a row the host accepted");
  return VT_OK;
}

// The device form: rows in this device's HBM, validated where they lie.  Returns after its work has finished.
int prepare_device_rows(int device, int mode, size_t count, size_t d, size_t ld_in, const void *in, size_t ld_out,
                        void *out, void *words, size_t *first_bad) {
  if (mode < VT_NORM_NONE || mode > VT_NORM_MINMAX) return VT_ERR_ARGUMENT;
  if (first_bad) *first_bad = count;
  if (count == 0 || d == 0) return VT_OK;
  if (!in || !out || ld_in < d || ld_out < d) return VT_ERR_ARGUMENT;
  if (in == out && ld_in != ld_out) return VT_ERR_ARGUMENT;
  if (count > 0xFFFFFFF0ull || d > 0x7fffffffu) return fail(VT_ERR_UNSUPPORTED, "batch too large");
  StatelessLease lease;
  VT_TRY(stateless_lease(device, &lease));
  Ctx &c = lease.s->ctx;
  PrepareState &p = lease.s->prepare;
  VT_TRY(p.open());
  VT_HIP(hipDeviceSynchronize());  // the producer may have used another stream
  VT_HIP(hipMemsetAsync(p.dFirst.p, 0xff, sizeof(uint32_t), c.stream));
  vt::PrepareArgs a{};
  a.in = static_cast<const float *>(in);
  a.ld_in = ld_in;
  a.out = static_cast<float *>(out);
  a.ld_out = ld_out;
  a.words = static_cast<uint64_t *>(words);
  a.first_refused = p.dFirst.p;
  a.n = (uint32_t)count;
  a.d = (uint32_t)d;
  VT_HIP(vt::launch_prepare_rows(a, mode, c.stream));
  VT_HIP(hipMemcpyAsync(p.hFirst.p, p.dFirst.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  VT_HIP(hipStreamSynchronize(c.stream));
  if (*p.hFirst.p != vt::kPrepNoRow) {
    if (first_bad) *first_bad = *p.hFirst.p;
    return VT_ERR_NON_FINITE;
  }
  return VT_OK;
}

}  // namespace
