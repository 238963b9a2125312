// stats_kernels.hip -- the statistics pass over the finished alignments of a mini-batch on the device (row a16 of DESIGN.md section 1;
// DESIGN.md section 4.5), included by stats_run.hip.  The code itself is aln_stats_core.h, the one source the host model runs too;
// this file is its device team, its genome reader and the kernel around them.
//   k_aln_stats   one wavefront per alignment, four alignments per workgroup: dist_stop / dist_start, the statistics of the CIGAR
//                 walk and the exon / stop-codon features, written where the host's download finds them
//   k_aln_cs      the same shape for the cs:Z: difference strings (MPA_GPU_CS=1; the code is aln_cs_core.h)
//   k_aln_rows    the same shape for the residue rows of --aln / --trans (MPA_GPU_ROWS=1; the code is aln_rows_core.h)
// The tables (codon table, aa20, substitution matrix: 804 bytes) are the workgroup's only LDS.  No capacity: the CIGAR is read 64
// words at a time, runs of any length are strided over the lanes, features go straight to their slots in global memory.

namespace mpa {

#define STATS_WAVES 4                                     /* alignments per workgroup */

struct StatsWave : CoopWave {                             // the team of aln_stats_core.h on the device: one wavefront
	static __device__ __forceinline__ int32_t sum(int32_t v)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		return __builtin_amdgcn_readfirstlane(v);                     // (the same on every lane: a scalar from here on)
	}
	static __device__ __forceinline__ uint32_t bcast(uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); }   // (k is wave-uniform)
	static __device__ __forceinline__ int32_t scan32(int32_t v, int32_t *total)
	{
		int32_t inc = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const int32_t w = __shfl_up(inc, o); if (lane() >= o) inc += w; }
		*total = __builtin_amdgcn_readlane(inc, 63);                  // (a scalar: the write position stays one)
		return inc - v;
	}
};

// the strand of one alignment in the resident 4-bit genome; outside the contig a position reads as N
struct StatsGenome {
	const uint8_t *seq;
	int64_t off, len;
	int rev;
	__device__ __forceinline__ uint32_t base(int64_t x) const { return x < 0 || x >= len ? 4u : strand_base(seq, off, len, rev, x); }
};

// (64 registers, no scratch, 804 bytes of LDS: next to three resident k_dp_round workgroups a SIMD has 128 registers left,
// DESIGN.md section 5 (3))
__global__ __launch_bounds__(64 * STATS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_aln_stats(const AlnStatsJob *jobs, int32_t n_jobs, const uint8_t *tabs,
                                                                                                       AlnStatsParams p, const uint8_t *text, const uint32_t *cig,
                                                                                                       const uint8_t *seq, const int64_t *ctg_off, const int64_t *ctg_len,
                                                                                                       AlnStatsOut *out, AlnFeat *feat)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[(ALN_TAB_BYTES + 15) & ~15];
	for (int i = (int)threadIdx.x; i < ALN_TAB_BYTES; i += 64 * STATS_WAVES) tab[i] = tabs[i];
	__syncthreads();
	// (the wave's number through readfirstlane: the job record, the contig and everything the walk derives from them stay scalar)
	const int32_t j = (int32_t)blockIdx.x * STATS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (j >= n_jobs) return;
	const AlnStatsJob J = jobs[j];
	const StatsGenome g{ seq, ctg_off[J.vid >> 1], ctg_len[J.vid >> 1], J.vid & 1 };
	const AlnStatsOut o = aln_stats_core<StatsWave>(J, p, tab, text, cig, g, feat);
	if ((threadIdx.x & 63) == 0) out[j] = o;
}

// The cs:Z: body of every alignment (aln_cs_core.h): the same jobs, tables, text and CIGAR pool, one wavefront
// per alignment writing into its own slot [slot_off[j], slot_off[j + 1]) of `slots` (sized by aln_cs_bound() on the host) with
// plain byte stores, and its length to out[j].  The table block is the only LDS (the matrix part is not read).
__global__ __launch_bounds__(64 * STATS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_aln_cs(const AlnStatsJob *jobs, int32_t n_jobs, const uint8_t *tabs,
                                                                                                    const uint8_t *text, const uint32_t *cig, const uint8_t *seq,
                                                                                                    const int64_t *ctg_off, const int64_t *ctg_len, const int64_t *slot_off,
                                                                                                    AlnCsOut *out, char *slots)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[(ALN_TAB_BYTES + 15) & ~15];
	for (int i = (int)threadIdx.x; i < ALN_TAB_BYTES; i += 64 * STATS_WAVES) tab[i] = tabs[i];
	__syncthreads();
	const int32_t j = (int32_t)blockIdx.x * STATS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (j >= n_jobs) return;
	const AlnStatsJob J = jobs[j];
	const StatsGenome g{ seq, ctg_off[J.vid >> 1], ctg_len[J.vid >> 1], J.vid & 1 };
	const AlnCsOut o = aln_cs_core<StatsWave>(J, tab, text, cig, g, slots + slot_off[j]);
	if ((threadIdx.x & 63) == 0) out[j] = o;
}

// The residue rows of every alignment (aln_rows_core.h): the same jobs, tables, text and CIGAR pool, one
// wavefront per alignment writing the four rows and the STA bytes into its own slot [slot_off[j], slot_off[j + 1]) of `slots` (sized
// by aln_rows_slot() on the host, exactly) with plain byte stores, and its record to out[j].  Only the bases that are printed are
// read from the resident genome.  The table block is the only LDS.
__global__ __launch_bounds__(64 * STATS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_aln_rows(const AlnStatsJob *jobs, int32_t n_jobs, const uint8_t *tabs,
                                                                                                      AlnRowsParams p, const uint8_t *text, const uint32_t *cig,
                                                                                                      const uint8_t *seq, const int64_t *ctg_off, const int64_t *ctg_len,
                                                                                                      const int64_t *slot_off, AlnRowsOut *out, char *slots)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[(ALN_TAB_BYTES + 15) & ~15];
	for (int i = (int)threadIdx.x; i < ALN_TAB_BYTES; i += 64 * STATS_WAVES) tab[i] = tabs[i];
	__syncthreads();
	const int32_t j = (int32_t)blockIdx.x * STATS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (j >= n_jobs) return;
	const AlnStatsJob J = jobs[j];
	const StatsGenome g{ seq, ctg_off[J.vid >> 1], ctg_len[J.vid >> 1], J.vid & 1 };
	const AlnRowsOut o = aln_rows_core<StatsWave>(J, p, tab, text, cig, g, slots + slot_off[j]);
	if ((threadIdx.x & 63) == 0) out[j] = o;
}

} // namespace mpa
