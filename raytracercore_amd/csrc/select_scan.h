// select_scan.h -- what the compacting selection passes share (api_adaptive.hip holds it: rt_adaptive_select_device;
// api_probe_list.hip: rt_probe_select_device): the per-device temporary memory, one ballot mask and one count
// per block of 64 candidates, and the exclusive scan over the counts.  A pass is
//     SelectPass pass;  select_begin(name, n_blocks, stream, pass)
//     its count kernel (pass.S->masks, pass.S->counts), select_scan, its write kernel
//     select_end(pass, stream)
// and holds the scratch's lock from begin until `pass` goes out of scope.
#pragma once

#include <mutex>

#include "rt_scene.h"

namespace rtc {

// The passes' temporary memory, the library's own, one per device: a mask and a count per block.
// Calls on one device share it, so a call on another stream than the last is ordered after it.
struct SelectScratch {
    unsigned long long* masks = nullptr;
    unsigned int* counts = nullptr;
    size_t blocks = 0;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool any = false;
};
struct SelectPass {
    std::unique_lock<std::mutex> lock;
    SelectScratch* S = nullptr;
};

// The current device's scratch, grown to n_blocks, with `stream` ordered after the last pass on it.
// name: the entry point, for messages.  RT_OK / RT_ERR_ARG (device index out of range) / RT_ERR_HIP.
int select_begin(const char* name, size_t n_blocks, hipStream_t stream, SelectPass& pass);
// Exclusive scan of pass.S->counts[0 .. n_blocks), in place; *d_total gets their sum.
void select_scan(SelectPass& pass, int n_blocks, unsigned int* d_total, hipStream_t stream);
// After the pass's last launch: the launches' status, and the event the next pass waits for.
int select_end(SelectPass& pass, hipStream_t stream);

} // namespace rtc
