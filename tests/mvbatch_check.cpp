// mvbatch_check.cpp -- drives the batch planner of the resident multi-vector store (vettore_amd/csrc/host/vt_mvbatch.h,
// plain C++) from stdin, for tests/test_mv_batch.py; built there with AddressSanitizer and UBSan.
// One batch per line: `capacity pass own_panel nsets count...`.  The answer is one line:
//   P first_set/sets/desc0/ndesc ... D set/info ... S set ...
// and `ok` after the last batch.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../vettore_amd/csrc/host/vt_mvbatch.h"

int main() {
  std::string line;
  vt_host::MvBatchPlan plan;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t capacity = 0, pass = 0;
    int own = 0;
    size_t nsets = 0;
    if (!(in >> capacity >> pass >> own >> nsets)) return 2;
    std::vector<uint32_t> counts(nsets);
    for (auto &c : counts)
      if (!(in >> c)) return 2;
    // (an exactly sized heap block: a read past the last count is an ASan report)
    vt_host::mv_batch_plan(counts.data(), nsets, capacity, pass, own != 0, &plan);
    std::printf("P");
    for (const auto &p : plan.panels) std::printf(" %u/%u/%u/%u", p.first_set, p.sets, p.desc0, p.ndesc);
    std::printf(" D");
    for (const auto &d : plan.desc) std::printf(" %u/%u", d.set, d.info);
    std::printf(" S");
    for (uint32_t s : plan.single) std::printf(" %u", s);
    std::printf("\n");
  }
  std::printf("ok\n");
  return 0;
}
