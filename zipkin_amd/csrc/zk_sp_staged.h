// zk_sp_staged.h — what zk_sp_traces leaves in the span store's staging, for the library's joint kernels
// (zk_an.hip's k_an_adjust). Internal: not part of the C ABI.
#pragma once
#include <stdint.h>

#include "zkspans.h"

namespace zk {

// The staging of the handle's last zk_sp_traces that ran its passes (the call ends synchronised, so a kernel
// on another stream of the same device may read it): the heads of the asked ids, and every trace's merged
// spans and (span, service) pairs behind the trace's own row base. All device pointers are NULL, and total
// is 0, when no pass has run. Valid until the handle's next lookup, observe, compact, expire or reset.
struct SpStagedTraces {
    int device = 0;
    const zk_sp_trace* heads = nullptr;        // [ZK_SP_MAX_IDS], the asked order
    const zk_sp_span* spans = nullptr;         // [total]
    const uint32_t* services = nullptr;        // [total]
    const unsigned long long* base = nullptr;  // [n], the row base of each asked id (device)
    const uint64_t* base_host = nullptr;       // the same on the host
    uint64_t total = 0;                        // the staged rows of the last call
};

int sp_device(const zk_sp* h);
void sp_staged_traces(const zk_sp* h, SpStagedTraces* out);

}  // namespace zk
