// K1 instantiations in filter mode (vt_scan.cuh, FILTER): the gathered scan of ONE query's candidate rows that keeps the
// rows whose rank word is <= a word on the device and finishes the search itself -- K1n's last link.  Dot in
// the default lane order, as vt_scan_gather.hip has it, and the run-time-order form, as vt_scan_general.hip has it for the
// other orders and for a query too long for LDS; the small candidate buffer's shape (k <= kSmallK), padded or not.
#include "vt_scan.cuh"

namespace vt {
namespace dev {
hipError_t launch_scan_filter_t(const ScanDev &sd, uint32_t blocks, size_t lds, hipStream_t s) {
  const bool padded = (sd.a.d % kRowAlign) != 0;
  if (sd.p.q_global) return launch_scan_t<-1, -1, kCapSmall, true, true, true, true>(sd, blocks, lds, s, 1);
  if (sd.a.order == kDefaultReduceOrder) {
    if (padded) return launch_scan_t<OP_DOT, kDefaultReduceOrder, kCapSmall, true, true, false, true>(sd, blocks, lds, s, 1);
    return launch_scan_t<OP_DOT, kDefaultReduceOrder, kCapSmall, true, false, false, true>(sd, blocks, lds, s, 1);
  }
  if (padded) return launch_scan_t<-1, -1, kCapSmall, true, true, false, true>(sd, blocks, lds, s, 1);
  return launch_scan_t<-1, -1, kCapSmall, true, false, false, true>(sd, blocks, lds, s, 1);
}
}  // namespace dev

using namespace dev;

hipError_t launch_scan_filter(const ScanArgs &a, uint32_t blocks, hipStream_t s) {
  ScanDev sd;
  sd.a = a;
  // (8-row tiles, as launch_scan_batch takes them: a candidate list spreads over more waves)
  if (!make_scan_shape(a.d, a.batch_cap, &sd.p, 8)) return hipErrorInvalidValue;
  sd.p.tile_floats = sd.p.tr * (uint32_t)a.stride;
  // the waves' panels and the query; no candidate buffers.  The finish keeps kScanFilterCap keys and payloads in static
  // LDS beside them (16 KiB): a query that leaves no room for those stays in global memory, as launch_scan_batch has it.
  const size_t panels = (size_t)kWavesPerBlock * sd.p.tr * sd.p.ss * sizeof(float);
  size_t lds = panels + (size_t)sd.p.ld * sizeof(float);
  if (lds > kMaxLds - 20 * 1024) {
    sd.p.q_global = 1;
    lds = panels;
  }
  if (blocks == 0 || a.k == 0 || a.k > (uint32_t)kSmallK || a.stride < sd.p.ld || !a.gather || !a.batch_counts ||
      metric_op(a.metric) != OP_DOT || a.key_out || !a.hi_word || !a.surv_keys || !a.surv_pay || a.surv_cap == 0 ||
      a.surv_cap > kScanFilterCap || !a.fsync || !a.out || !a.info || !a.status)
    return hipErrorInvalidValue;
  return launch_scan_filter_t(sd, blocks, lds, s);
}
}  // namespace vt
