// vt_muvera.h -- muvera_encode_query / muvera_encode_document (muvera.rs:26-106) for a batch of vector sets:
// validation on the host in the reference's order, the encoding on the device (K10, vt_muvera.hip) in chunks of
// sets bounded by a byte budget.
// Part of vt_index.cpp's translation unit (included there, in this order, exactly once).
//
// A chunk's vectors are copied into one of the upload ring's two staging blocks (UploadRing, vt_stateless.h) and uploaded
// into one of its two device buffers (every vector of a valid set has the configured length: a set is one run of `values`);
// chunk k + 1 is staged and uploaded while chunk k is encoded and its rows come back.  The weights and signs depend
// on the configuration alone: one table per call, and one list of input indices per count-sketch slot.
#pragma once

namespace {

constexpr size_t kMuveraChunkBytes = 256u << 20;      // default budget of a chunk (vt_debug_set muvera_chunk_bytes)
constexpr size_t kMuveraMaxOutput = 16777216;         // MAX_OUTPUT_DIMENSIONS, muvera.rs:23
constexpr size_t kMuveraMaxTable = (size_t)1 << 28;   // floats of weights and signs (1 GiB)

struct MuveraConfig {
  size_t d, R, k;
  uint64_t seed;
  size_t pd, final_dim;
  bool final_some;  // Some(final_dim), Some(0) included
};

// muvera.rs:81-95: the configuration on its own
int muvera_check_config(const MuveraConfig &m) {
  if (m.d == 0) return VT_ERR_MUVERA_DIMENSION;
  if (m.R == 0) return VT_ERR_MUVERA_REPETITIONS;
  if (m.k >= 31) return VT_ERR_MUVERA_SIMHASH;
  if (m.pd == 0) return VT_ERR_MUVERA_PROJECTION;
  if (m.final_some && m.final_dim == 0) return VT_ERR_MUVERA_FINAL;
  return VT_OK;
}
// muvera.rs:29-42: the sizes (a valid configuration).  (counts_size, :45-48, cannot overflow once output_size is
// within the limit: it is output_size / projection_dimension.)
int muvera_check_sizes(const MuveraConfig &m, size_t *out_size, size_t *fde_dim) {
  const size_t partitions = (size_t)1 << m.k;
  size_t rep = 0, total = 0;
  if (__builtin_mul_overflow(partitions, m.pd, &rep) || __builtin_mul_overflow(m.R, rep, &total)) return VT_ERR_FDE_OVERFLOW;
  const size_t final_size = m.final_some ? m.final_dim : total;
  if (total > kMuveraMaxOutput || final_size > kMuveraMaxOutput) return VT_ERR_FDE_LIMIT;
  *out_size = total;
  *fde_dim = final_size;
  return VT_OK;
}
// muvera.rs:96-104 for one non-empty set: every length first, then every value
int muvera_check_set(const float *values, const size_t *value_off, size_t v0, size_t v1, size_t d) {
  for (size_t v = v0; v < v1; ++v)
    if (value_off[v + 1] - value_off[v] != d) return VT_ERR_DIMENSION;
  return validate_finite(values + value_off[v0], (v1 - v0) * d);
}

// count_sketch's slot and sign of every input index (muvera.rs:187-192), as one list of indices per slot in
// increasing order: off[final_dim + 1], list[out_size] (bit 31: sign -1).
void muvera_slot_lists(uint64_t seed, size_t out_size, size_t final_dim, std::vector<uint32_t> &off, std::vector<uint32_t> &list) {
  std::vector<uint32_t> slot(out_size);
  parallel_for(out_size, (size_t)1 << 16, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t s = vt::muvera_hash4(seed, 0x9E3779B97F4A7C15ull, i, 0) % final_dim;
      const uint32_t neg = (uint32_t)(vt::muvera_hash4(seed, 0xD1B54A32D192ED03ull, i, s) & 1);
      slot[i] = (uint32_t)s | (neg << 31);
    }
  });
  off.assign(final_dim + 1, 0);
  for (size_t i = 0; i < out_size; ++i) ++off[(slot[i] & 0x7fffffffu) + 1];
  for (size_t s = 0; s < final_dim; ++s) off[s + 1] += off[s];
  std::vector<uint32_t> at(off.begin(), off.end() - 1);
  list.resize(out_size);
  for (size_t i = 0; i < out_size; ++i) list[at[slot[i] & 0x7fffffffu]++] = (uint32_t)i | (slot[i] & 0x80000000u);
}

// encode (muvera.rs:26-74) of `count` sets; `out` is [count][fde dimension].  A set that fails keeps a zero row.
// Returns the first failing set's status when the caller has no place for statuses (or asks for one set: the NIF).
int muvera_encode(int device, int mode, size_t count, const size_t *set_vec_off, const float *values, const size_t *value_off,
                  const MuveraConfig &m, float *out, int *set_status) {
  size_t out_size = 0, fde = 0;
  std::vector<int> st(count, VT_OK);
  if (count == 1) {
    // the reference's order for one set: empty, the configuration, lengths, values, sizes
    if (set_vec_off[0] == set_vec_off[1]) return VT_ERR_EMPTY_SET;
    VT_TRY(muvera_check_config(m));
    VT_TRY(muvera_check_set(values, value_off, set_vec_off[0], set_vec_off[1], m.d));
    VT_TRY(muvera_check_sizes(m, &out_size, &fde));
  } else {
    // a batch: what depends on the configuration alone fails the call, the rest is the set's own
    VT_TRY(muvera_check_config(m));
    VT_TRY(muvera_check_sizes(m, &out_size, &fde));
    parallel_for(count, 512, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const size_t v0 = set_vec_off[i], v1 = set_vec_off[i + 1];
        st[i] = v0 == v1 ? VT_ERR_EMPTY_SET : muvera_check_set(values, value_off, v0, v1, m.d);
      }
    });
  }
  if (count == 0) return VT_OK;
  if (!out) return VT_ERR_ARGUMENT;  // (only now: a refused configuration has no row length to allocate for)
  const bool report_first = !set_status || count == 1;
  auto refused = [](int s) { return s != VT_OK; };
  const size_t first_bad = std::find_if(st.begin(), st.end(), refused) - st.begin();
  // without a place for statuses only the sets before the first refused one can change the answer (an earlier
  // "encoding overflow" comes first)
  const size_t todo = report_first ? first_bad : count;
  const size_t valid = std::count(st.begin(), st.begin() + todo, VT_OK);

  if (valid > 0) {
    if (m.d > vt::kMuveraMaxDim) return fail(VT_ERR_UNSUPPORTED, "vector dimension exceeds what the MUVERA kernel stages in LDS");
    const bool identity = m.pd == m.d;
    const size_t C = m.k + (identity ? 0 : m.pd);
    const size_t table_floats = m.R * m.d * C;
    if (table_floats > kMuveraMaxTable) return fail(VT_ERR_UNSUPPORTED, "MUVERA weight table exceeds 1 GiB");
    StatelessLease lease;
    VT_TRY(stateless_lease(device, &lease));
    Ctx &c = lease.s->ctx;
    UploadRing &ring = lease.s->ring;
    MuveraState &P = lease.s->muvera;
    VT_TRY(ring.open());

    vt::MuveraArgs a = muvera_args(m.d, m.R, m.k, m.pd, mode, out_size);
    const bool global_counts = mode == 1 && ((size_t)1 << m.k) > vt::kMuveraLdsPartitions;
    if (table_floats) {
      VT_TRY(P.dTable.ensure(table_floats));
      VT_HIP(vt::launch_muvera_table(m.seed, a.R, a.d, a.k, a.C, P.dTable.p, c.stream));
      a.table = P.dTable.p;
    }
    std::vector<uint32_t> slot_off, slot_list;
    if (m.final_some) {
      muvera_slot_lists(m.seed, out_size, m.final_dim, slot_off, slot_list);
      VT_TRY(P.dSlotOff.ensure(slot_off.size()));
      VT_TRY(P.dSlotList.ensure(std::max<size_t>(slot_list.size(), 1)));
      VT_HIP(hipMemcpyAsync(P.dSlotOff.p, slot_off.data(), slot_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
      VT_HIP(hipMemcpyAsync(P.dSlotList.p, slot_list.data(), slot_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
      VT_HIP(hipStreamSynchronize(c.stream));  // (the lists leave scope with the call, but pageable copies return early)
    }

    // chunks of sets [cut[k], cut[k + 1]): the intermediate rows, the counts and the vectors within the budget
    const long forced = vt::env::get(vt::env::MUVERA_CHUNK_BYTES);
    const size_t budget = std::min<size_t>(forced > 0 ? (size_t)forced : kMuveraChunkBytes, (size_t)4 << 30);
    const size_t set_bytes = (out_size + (m.final_some ? fde : 0) + (global_counts ? out_size / m.pd : 0)) * sizeof(float);
    const size_t vec_bytes = m.d * sizeof(float);
    const size_t max_sets = std::max<size_t>(1, 0x7fffffffull / a.groups);
    std::vector<size_t> cut{0};
    for (size_t i0 = 0; i0 < todo;) {
      size_t i1 = i0, bytes = 0;
      while (i1 < todo && i1 - i0 < max_sets) {
        const size_t add = set_bytes + (st[i1] == VT_OK ? (set_vec_off[i1 + 1] - set_vec_off[i1]) * vec_bytes : 0);
        if (i1 > i0 && bytes + add > budget) break;
        bytes += add;
        ++i1;
      }
      cut.push_back(i1);
      i0 = i1;
    }
    const size_t nchunks = cut.size() - 1;

    // vectors and offsets of chunk k into staging block k & 1, and on their way to the device
    auto stage = [&](size_t k) -> int {
      const int b = (int)(k & 1);
      const size_t i0 = cut[k], i1 = cut[k + 1];
      size_t rows = 0;
      for (size_t i = i0; i < i1; ++i)
        if (st[i] == VT_OK) rows += set_vec_off[i + 1] - set_vec_off[i];
      if (rows > 0xFFFFFFF0ull) return fail(VT_ERR_UNSUPPORTED, "more than 2^32-16 vectors in one chunk of sets");
      VT_TRY(ring.reserve(b, rows * m.d, i1 - i0 + 1));
      size_t at = 0;
      for (size_t i = i0; i < i1; ++i) {
        ring.hOff[b].p[i - i0] = (uint32_t)at;
        if (st[i] != VT_OK) continue;
        const size_t n = set_vec_off[i + 1] - set_vec_off[i];
        const float *src = values + value_off[set_vec_off[i]];
        float *dst = ring.hX[b].p + at * m.d;
        parallel_for(n * m.d, (size_t)1 << 20, [&](size_t lo, size_t hi) { std::memcpy(dst + lo, src + lo, (hi - lo) * sizeof(float)); });
        at += n;
      }
      ring.hOff[b].p[i1 - i0] = (uint32_t)at;
      return ring.send(b, rows * m.d, i1 - i0 + 1);
    };

    VT_TRY(stage(0));
    for (size_t k = 0; k < nchunks; ++k) {
      const int b = (int)(k & 1);
      const size_t i0 = cut[k], nsets = cut[k + 1] - i0;
      VT_TRY(P.dFull.ensure(nsets * out_size));
      VT_TRY(P.dStatus.ensure(nsets));
      VT_TRY(P.hStatus.ensure(nsets));
      VT_TRY(ring.wait_ready(b, c.stream));
      VT_HIP(hipMemsetAsync(P.dFull.p, 0, nsets * out_size * sizeof(float), c.stream));
      VT_HIP(hipMemsetAsync(P.dStatus.p, 0, nsets * sizeof(int), c.stream));
      a.counts = nullptr;
      if (global_counts) {
        const size_t words = nsets * (out_size / m.pd);
        VT_TRY(P.dCounts.ensure(words));
        VT_HIP(hipMemsetAsync(P.dCounts.p, 0, words * sizeof(uint32_t), c.stream));
        a.counts = P.dCounts.p;
      }
      a.X = ring.dX[b].p;
      a.set_off = ring.dOff[b].p;
      a.nsets = (uint32_t)nsets;
      a.full = P.dFull.p;
      a.status = P.dStatus.p;
      if (vt::muvera_lds_bytes(a) > 160u * 1024) return fail(VT_ERR_UNSUPPORTED, "MUVERA: the vector and the partition counts exceed the LDS");
      VT_HIP(vt::launch_muvera_encode(a, c.stream));
      const float *rows = P.dFull.p;
      if (m.final_some) {
        VT_TRY(P.dFinal.ensure(nsets * fde));
        VT_HIP(vt::launch_muvera_sketch(P.dFull.p, out_size, a.nsets, (uint32_t)fde, P.dSlotOff.p, P.dSlotList.p, P.dFinal.p,
                                        P.dStatus.p, c.stream));
        rows = P.dFinal.p;
      }
      VT_TRY(ring.mark_consumed(b, c.stream));    // (the last kernel that reads slot b is behind this)
      if (k + 1 < nchunks) VT_TRY(stage(k + 1));  // (the other slot, while this chunk is encoded)
      VT_HIP(hipMemcpyAsync(out + i0 * fde, rows, nsets * fde * sizeof(float), hipMemcpyDeviceToHost, c.stream));
      VT_HIP(hipMemcpyAsync(P.hStatus.p, P.dStatus.p, nsets * sizeof(int), hipMemcpyDeviceToHost, c.stream));
      VT_HIP(hipStreamSynchronize(c.stream));  // (for the host's read of the rows and the statuses, not for the ring)
      for (size_t i = 0; i < nsets; ++i)
        if (st[i0 + i] == VT_OK && P.hStatus.p[i] != 0) st[i0 + i] = P.hStatus.p[i];
    }
  }
  // a set that failed, on the host or on the device, and every set that was not reached: a zero row
  for (size_t i = 0; i < count; ++i)
    if (i >= todo || st[i] != VT_OK) std::memset(out + i * fde, 0, fde * sizeof(float));

  if (set_status) std::memcpy(set_status, st.data(), count * sizeof(int));
  const auto bad = std::find_if(st.begin(), st.end(), refused);  // (after the device's statuses: maybe an earlier set)
  return report_first && bad != st.end() ? *bad : VT_OK;
}

}  // namespace
