// dp_plan_kernels.hip -- the planner of a DP round on the device: the stages of dp_plan_core.h, each called by
// 256-lane workgroups.  Included by dp_exec.hip, whose dev_dp_plan() launches them around two radix sorts.  Bookkeeping next to resident
// DP workgroups: no dynamic LDS, 192 bytes of static LDS for the workgroup scan, one lane per call or per unit.
#pragma once
#include "dp_plan_core.h"

namespace mpa {

// a workgroup as the team of the stages: scans in wave registers, the four waves' totals through LDS
struct TeamWG {
	static const int W = 256;
	int64_t *lds;                                // [4][DPP_NSUM]
	__device__ int rank() const { return (int)threadIdx.x; }
	__device__ void sync() const { __syncthreads(); }
	template<int K> __device__ void exscan(DpVec<K> &v, DpVec<K> &total) const
	{
		static_assert(K <= DPP_NSUM, "the team's LDS holds DPP_NSUM sums per wave");
		const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
		DpVec<K> inc = v;
		for (int d = 1; d < 64; d <<= 1)
			for (int k = 0; k < K; ++k) {
				const long long o = __shfl_up((long long)inc.v[k], (unsigned)d, 64);
				if (lane >= d) inc.v[k] += o;
			}
		__syncthreads();                            // (the previous scan's totals have been read)
		if (lane == 63) for (int k = 0; k < K; ++k) lds[wave * K + k] = inc.v[k];
		__syncthreads();
		for (int k = 0; k < K; ++k) {
			int64_t before = 0, tot = 0;
			for (int w = 0; w < W / 64; ++w) { const int64_t x = lds[w * K + k]; before += w < wave ? x : 0, tot += x; }
			v.v[k] = inc.v[k] - v.v[k] + before, total.v[k] = tot;
		}
	}
	__device__ void add(int64_t *dst, int64_t v) const
	{
		long long s = v;
		for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
		if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)dst, (unsigned long long)s);
	}
	__device__ void flag(int64_t *dst, int64_t bits) const { atomicOr((unsigned long long*)dst, (unsigned long long)bits); }
};

#define MPA_DPP_TEAM() MPA_SHORT_KERNEL(); __shared__ int64_t team_lds[(TeamWG::W / 64) * DPP_NSUM]; const TeamWG tm{ team_lds }

__global__ __launch_bounds__(256) void k_dpp_classify(DpDevPlan D) { MPA_DPP_TEAM(); dpp_classify(tm, D, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpp_sums(DpDevPlan D) { MPA_DPP_TEAM(); dpp_sums(tm, D, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpp_mid(DpDevPlan D) { MPA_DPP_TEAM(); dpp_mid(tm, D); }                   // one workgroup
__global__ __launch_bounds__(256) void k_dpp_layout(DpDevPlan D) { MPA_DPP_TEAM(); dpp_layout(tm, D, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpp_units(DpDevPlan D) { MPA_DPP_TEAM(); dpp_units(tm, D, (int64_t)blockIdx.x); }
__global__ __launch_bounds__(256) void k_dpp_units_out(DpDevPlan D) { MPA_DPP_TEAM(); dpp_units_out(tm, D, (int64_t)blockIdx.x); }

} // namespace mpa
