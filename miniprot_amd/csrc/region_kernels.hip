// region_kernels.hip -- main chains to refinement windows on the device (row a17 of DESIGN.md section 1; DESIGN.md section 4.6;
// MPA_GPU_REGIONS=1), included by seed_run.hip, whose chain tail launches them.  The code itself is regions_core.h, the one source
// the host model runs too; this file is its device team and the kernels around it.
//   k_regions      one wavefront per query, four queries per workgroup: the query's main chains where k_chain_extract left them ->
//                  its selected regions (fixed-size records), their refinement limits and their number
//   k_region_pack  the records and limits of every query into pinned host memory
// No LDS: the digit tables of the sort (3 KB per query) live in global memory next to the rest of the query's scratch, which is
// carved from the number of its chains.  No capacity.  Plain vector stores only.

namespace mpa {

#define REGIONS_WAVES 4                                   /* queries per workgroup */

struct RegionsWave : CoopWave {                           // the team of regions_core.h on the device: one wavefront
	static __device__ __forceinline__ int32_t sum(int32_t v)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		return __builtin_amdgcn_readfirstlane(v);                     // (the same on every lane: a scalar from here on)
	}
};

struct RegionsArgs {
	const int64_t *first;            // [n_prob] where the extraction left query q's chains: a + first[q], u + first[q]
	const uint64_t *a, *u;
	const int64_t *nu;               // [n_prob] chains of query q
	const int64_t *offu;             // [n_prob + 1] their prefix: where query q's records, limits and scratch lie
	const uint32_t *bo;              // [p.n_vid + 1]
	RegionsParams p;
	RegionRec *tmp, *out;            // [total chains]
	uint64_t *ext, *cov;
	Pair64 *key;
	SortRange *stack;                // query q at offu[q] / 64 + 5 q
	uint32_t *hist;                  // 768 per query
	int32_t *prim, *ctl, *n_reg;     // ctl: 2 per query; n_reg[n_prob]: the result's length
};

// (the budget of DESIGN.md section 5 (3) for a kernel next to three resident k_dp_round workgroups: 64 registers, no scratch)
__global__ __launch_bounds__(64 * REGIONS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_regions(RegionsArgs x, int32_t n_prob)
{
	MPA_SHORT_KERNEL();
	// (the wave's number through readfirstlane: the query's offsets and everything derived from them stay scalar)
	const int32_t q = (int32_t)blockIdx.x * REGIONS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (q >= n_prob) return;
	const int64_t n = x.nu[q];
	if (n <= 0 || n > INT32_MAX) { if ((threadIdx.x & 63) == 0) x.n_reg[q] = 0; return; }
	const int64_t o = x.offu[q], f = x.first[q];
	const RegionsScratch S{ x.tmp + o, x.key + o, x.stack + (o / 64 + 5 * (int64_t)q), x.hist + 768 * (int64_t)q, x.prim + o, x.cov + o, x.ctl + 2 * (int64_t)q };
	const int32_t k = regions_core<RegionsWave>(x.p, x.bo, x.u + f, (int32_t)n, x.a + f, S, x.out + o, x.ext + o);
	if ((threadIdx.x & 63) == 0) x.n_reg[q] = k;
}

// the regions of every query, where its chains' prefix puts them; dst may be pinned host memory.  A record is four 16-byte words
__global__ __launch_bounds__(256) void k_region_pack(const int64_t *offu, const int32_t *n_reg, const RegionRec *src, const uint64_t *ext, RegionRec *dst, uint64_t *ext_dst,
                                                     int32_t *n_dst)
{
	MPA_SHORT_KERNEL();
	const int32_t q = blockIdx.x;
	const int64_t o = offu[q];
	const int32_t n = n_reg[q];
	const uint4 *s4 = (const uint4*)(src + o);
	uint4 *d4 = (uint4*)(dst + o);
	for (int32_t i = threadIdx.x; i < 4 * n; i += 256) d4[i] = s4[i];
	for (int32_t i = threadIdx.x; i < n; i += 256) ext_dst[o + i] = ext[o + i];
	if (threadIdx.x == 0) n_dst[q] = n;
}

} // namespace mpa
