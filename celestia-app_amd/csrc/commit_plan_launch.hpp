// commit_plan_launch.hpp -- the launches of commit_plan.hip and the two of
// blobtx_check.hip that dagpu_proposal_check_device enqueues
// (commit_plan_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "commit_plan.hpp"

namespace dagpu {

// cp_reduce, cp_scan, cp_fill
hipError_t launch_commit_plan(const CpArgs& a, hipStream_t s);
// bt_tie over the rows up to a.blob_base[n] (device memory); owner: two words per row
hipError_t launch_bt_tie_counted(const BtArgs& a, uint32_t* owner, uint64_t capacity, uint32_t grid_cap,
                                 hipStream_t s);
// pv_fold over the rows up to a.blob_base[n], then pv_finish
hipError_t launch_verdict(const PvArgs& a, uint64_t capacity, uint32_t grid_cap, hipStream_t s);
// blobtx_check.hip: bt_validate (one lane per tx) and bt_finish (one per block)
hipError_t launch_bt_validate(const BtArgs& a, hipStream_t s);
hipError_t launch_bt_finish(const BtArgs& a, hipStream_t s);

}  // namespace dagpu
