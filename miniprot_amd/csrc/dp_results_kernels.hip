// dp_results_kernels.hip -- a DP round's result records and the offsets of its dense CIGAR pool on the device (MPA_GPU_ROUND2=1; DESIGN.md
// section 4.12): the stages of dp_results_core.h, each called by 256-lane workgroups with the planner's team (dp_plan_kernels.hip: scans in
// wave registers, the four waves' totals through LDS, the workgroup sums carried by one workgroup in the middle).  Included by dp_exec.hip,
// which enqueues them, k_cigar_gather and one download behind the round's last kernel and in front of the round's one wait.
// Bookkeeping next to resident DP workgroups: no dynamic LDS, the team's 192 bytes of static LDS, one lane per call.  Plain vector stores.
#pragma once
#include "dp_plan_kernels.hip"
#include "dp_results_core.h"

namespace mpa {

__global__ __launch_bounds__(256) void k_dpr_sums(DpResDev R) { MPA_DPP_TEAM(); dpr_sums(tm, R, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpr_mid(DpResDev R) { MPA_DPP_TEAM(); dpr_mid(tm, R); }                      // one workgroup
__global__ __launch_bounds__(256) void k_dpr_offsets(DpResDev R) { MPA_DPP_TEAM(); dpr_offsets(tm, R, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpr_records(DpResDev R) { MPA_DPP_TEAM(); dpr_records(tm, R, (int64_t)blockIdx.x); }

} // namespace mpa
