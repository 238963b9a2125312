// dev_common.h -- what more than one device unit of the library needs on the DEVICE side: the few __forceinline__ helpers that several
// kernel files use, and the plain structs that cross from the host drivers into kernel arguments of another unit's helper.  Every
// unit (dev_ctx.h includes this) sees the same text, and nothing here has a definition that could exist twice in the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chain_core.h"

namespace mpa {

struct U32ToU64 { __host__ __device__ uint64_t operator()(uint32_t x) const { return (uint64_t)x; } };   // scan inputs of 32-bit counts as 64-bit sums

// the chain forward pass (k_chain_fwd, k_chain_fwd_wave: seed_exec.hip) as its host entry takes it (chain_fwd_launch, dev_ctx.h): the
// parameters (an entry of the list of long runs: LongRun, chain_core.h)
struct PreParams { int32_t max_dist_x, max_dist_y, bw, max_skip, max_iter, kmer, bbit, is_spliced, max_dblock; float coef_log; };

// base of the strand-oriented contig at strand-local position x (ntseq.c:89-106 folded into addressing; the scans of refine_kernels.hip and index_kernels.hip)
__device__ __forceinline__ uint32_t strand_base(const uint8_t *seq, int64_t off, int64_t len, int rev, int64_t x)
{
	int64_t p = rev ? off + len - 1 - x : off + x;
	uint32_t b = (seq[p >> 1] >> ((p & 1) * 4)) & 0xf;
	return rev && b < 4 ? 3 - b : b;
}

// Sixteen consecutive bases of the packed genome as the nibbles of one word: nibble j = the base at genome position
// p_first + dir * j (dir = +1 / -1), complemented (3 - b for the codes below 4) when `comp`.  Three aligned words cover them;
// positions outside the genome buffer (which is padded by 16 bytes) read as garbage -- the caller masks what it does not own.
__device__ __forceinline__ uint64_t packed_window16(const uint8_t *seq, int64_t l_seq, int64_t p_first, int dir, int comp)
{
	const int64_t lo = dir > 0 ? p_first : p_first - 15;
	const int64_t seq_bytes = (l_seq + 1) >> 1, amax = (seq_bytes + 4) & ~(int64_t)3;
	int64_t a0 = (lo >> 1) & ~(int64_t)3;
	a0 = a0 < 0 ? 0 : a0 > amax ? amax : a0;
	const uint32_t *wp = (const uint32_t*)(seq + a0);
	const uint32_t W0 = wp[0], W1 = wp[1], W2 = wp[2];
	const int64_t n0 = lo - 2 * a0;                                // first nibble (0..7 unless the address was clamped)
	const uint64_t lo64 = (uint64_t)W0 | (uint64_t)W1 << 32;
	uint64_t nib;
	if (n0 >= 0 && n0 <= 7) nib = n0 ? (lo64 >> (4 * n0)) | ((uint64_t)W2 << (64 - 4 * n0)) : lo64;
	else if (n0 < 0 && n0 >= -15) nib = lo64 << (4 * (-n0));
	else nib = 0;
	if (dir < 0) {                                                 // descending: reverse the sixteen nibbles
		nib = ((nib & 0x0f0f0f0f0f0f0f0fULL) << 4) | ((nib >> 4) & 0x0f0f0f0f0f0f0f0fULL);
		nib = __builtin_bswap64(nib);
	}
	if (comp) {                                                    // minus strand: complement the codes below 4 (3 - b = b ^ 3)
		const uint64_t m = ~((nib >> 2) | (nib >> 3)) & 0x1111111111111111ULL;
		nib ^= m * 3;
	}
	return nib;
}

__device__ __forceinline__ uint32_t d_hash32_mask(uint32_t key, uint32_t mask)     // mp_hash32_mask (sketch.c:7-16)
{
	key = (key + ~(key << 15)) & mask;
	key ^= key >> 10;
	key = (key + (key << 3)) & mask;
	key ^= key >> 6;
	key = (key + ~(key << 11)) & mask;
	key ^= key >> 16;
	return key;
}

// the refinement scan and the index scan (refine_kernels.hip, index_kernels.hip) walk a strand in chunks of the same size and
// translate codons through the same table
struct RefineTab { uint8_t t[64]; };                  // codon -> reduced residue (ns_tab_codon13), 0xff for a stop codon
#define REFINE_CHUNK 2048

// MPA_TIMING=2 stamps of k_chain_extract (CoopWave::mark_time / note): DEFINED in seed_exec.hip, the unit of the one kernel that
// stamps; the other user of CoopWave (k_gs32) calls neither, so its unit never refers to them
extern __device__ long long *g_extract_prof;
extern __device__ int g_extract_prof_n;

// the team's fast scratch memory: 2 KB of LDS per wavefront (k_chain_extract is one wavefront per workgroup).  Round 6: 8 KB -> 2 KB.
// With the 5 KB of digit tables a wave then takes 7.2 KB, so that LDS allows the five waves per SIMD the 85 VGPRs do (8 KB: three), all
// 4 000 problems of a launch are resident at once and a wave's footprint next to the DP round's workgroups is half of what it was:
// lone launch 11.9 -> 10.6 ms, stream +5 % (3 of 3 interleaved repeats; 512 words: the same; profiles/r06_experiments.txt).  Buckets
// that do not fit are walked in place, as before.
#ifndef EXTRACT_STAGE_WORDS
#define EXTRACT_STAGE_WORDS 256
#endif
// (DYNAMIC LDS: with a static array the compiler knows that LDS allows three waves per SIMD and lets the registers grow to 512 / 3 --
// 166 VGPRs, a wave that fits next to no DP workgroup's waves; with the size hidden, amdgpu_waves_per_eu below is what it allocates for)
#define EXTRACT_LDS_BYTES (EXTRACT_STAGE_WORDS * 8 + 1280 * 4)
__device__ __forceinline__ uint64_t *g_extract_stage()
{
	extern __shared__ __attribute__((aligned(16))) uint64_t mpa_extract_lds[];
	return mpa_extract_lds;
}

// the team of chain_core.h on the device: the 64 lanes of one wavefront
struct CoopWave {
	static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & 63); }
	static __device__ __forceinline__ int width() { return 64; }
	// lanes of one wave share their L1: ordering their global / LDS accesses needs no cache action, only completion + a barrier
	static __device__ __forceinline__ void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
	static __device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
	static __device__ __forceinline__ int rank(uint64_t m) { return __popcll(m & ((1ull << lane()) - 1ull)); }
	static __device__ __forceinline__ int popc(uint64_t m) { return __popcll(m); }
	static __device__ __forceinline__ int32_t reduce_max(int32_t v)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { const int32_t w = __shfl_xor(v, o); v = w > v ? w : v; }
		return v;
	}
	static __device__ __forceinline__ bool any(bool p) { return __ballot(p) != 0; }
	static __device__ __forceinline__ void count(uint32_t *slot) { atomicAdd(slot, 1u); }
	static __device__ __forceinline__ void atomic_min(int32_t *slot, int32_t v) { atomicMin(slot, v); }
	static __device__ __forceinline__ int64_t scan_excl(int64_t v, int64_t *total)
	{
		int64_t inc = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const int64_t w = __shfl_up(inc, o); if (lane() >= o) inc += w; }
		*total = __shfl(inc, 63);
		return inc - v;
	}
	static __device__ __forceinline__ int64_t scan_max_excl(int64_t v, int64_t *total)
	{
		int64_t inc = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) { const int64_t w = __shfl_up(inc, o); if (lane() >= o && w > inc) inc = w; }
		*total = __shfl(inc, 63);
		const int64_t below = __shfl_up(inc, 1);
		return lane() ? below : INT64_MIN;
	}
	static __device__ __forceinline__ void digit_rank(int d, bool have, int *rank, int *cnt)
	{
		unsigned long long eq = __ballot(have);                  // lanes that take part and hold the same 8-bit digit: eight ballots
#pragma unroll
		for (int b = 0; b < 8; ++b) { const unsigned long long m = __ballot((d >> b) & 1); eq &= ((d >> b) & 1) ? m : ~m; }
		*rank = __popcll(eq & ((1ull << lane()) - 1ull)), *cnt = __popcll(eq);
	}
	static __device__ __forceinline__ int first_unset(uint64_t m) { return m == ~0ull ? 64 : __ffsll((long long)~m) - 1; }
	static __device__ __forceinline__ int lowest(uint64_t m) { return __ffsll((long long)m) - 1; }
	static __device__ __forceinline__ uint64_t *scratch(int64_t *cap) { *cap = EXTRACT_STAGE_WORDS; return g_extract_stage(); }
	static __device__ __forceinline__ void mark_time(int k) { if (g_extract_prof && (int)blockIdx.x < g_extract_prof_n && lane() == 0) g_extract_prof[(int64_t)blockIdx.x * 16 + k] = (long long)wall_clock64(); }
	static __device__ __forceinline__ void note(int k, int64_t v) { if (g_extract_prof && (int)blockIdx.x < g_extract_prof_n && lane() == 0) g_extract_prof[(int64_t)blockIdx.x * 16 + 8 + k] = (long long)v; }
};

} // namespace mpa
