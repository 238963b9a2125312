// sketch_exec.hip -- the first stage of mp_map() on the device (SURVEY.md kernel K5; map.c:126-170, sketch.c:18-38), included by
// seed_run.hip behind seed_exec.hip.  For a whole mini-batch (driver: dev_sketch_jobs in seed_run.hip):
//   k_sketch_count   per query: the protein sketch (modimizers of the reduced-alphabet k-mers), the occurrence count of every
//                    sketched seed (ki[b + 1] - ki[b], empty buckets included), the boxplot cut-off of mp_cal_max_occ from the
//                    25 % / 75 % order statistics of those counts, and how many seeds / anchors the cut-off keeps
//   k_offsets2       (seed_exec.hip) exclusive prefixes of the two per-query counts: qfirst[] (anchors), jfirst[] (jobs)
//   k_sketch_emit    the kept seeds of every query in ascending query position as SeedJobDev records, dense across queries, written
//                    where k_seed_sift reads them
// One wavefront per query, four queries per workgroup.  Nothing rolls: the lane of position i builds the k-mer that ENDS at i from
// its k <= 7 residues.  The counts of a query never leave global memory: what pass 1 writes per position (count, or -1 where no
// seed ends; bucket) is read back by the lane that wrote it, 1.4 KB for a typical protein and resident in the L2 for any.  The order
// statistics are therefore not a sort but a selection: sorted[i] is the largest v with #(counts < v) <= i, found bit by bit
// from the highest set bit of the query's largest count (12 passes at genome scale), both quantiles in the same pass.  That keeps
// the kernel at 256 bytes of LDS (the residue table) and frees it of any capacity: a query of any length is sketched here.
// A query is handed to the host (flag = 1, no jobs) only where the device cannot restate the host's arithmetic: a bucket of more
// than 2^31 - 1 occurrences, or a cut-off whose double leaves the int32 range (the x86 conversion and the GPU's differ there).

namespace mpa {

struct SketchParams { int64_t n_bucket, n_kb; int32_t kmer, mod_bit, max_occ, pad; };

#define SKETCH_WAVES 4                                    /* queries per workgroup */

__device__ __forceinline__ uint32_t sketch_wave_sum(uint32_t v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

// the seed that ends at position i, if one does: all of the last `kmer` residues valid (a stop or an unknown residue resets the
// run, host_core.cpp sketch_protein) and the hash selected by the modimizer mask
__device__ __forceinline__ bool sketch_seed_at(const uint8_t *seq, int32_t i, const uint8_t *tab, const SketchParams &p, uint32_t *bucket)
{
	if (i < p.kmer - 1) return false;
	uint32_t word = 0, bad = 0;
	for (int32_t k = p.kmer - 1; k >= 0; --k) {
		const uint32_t c = tab[seq[i - k]];
		bad |= c >= 14u ? 1u : 0u;
		word = word << 4 | (c & 15u);
	}
	if (bad) return false;
	const uint32_t mask = (1u << (4 * p.kmer)) - 1u;
	const uint32_t h = d_hash32_mask(word, mask);
	if (h & ((1u << p.mod_bit) - 1u)) return false;
	*bucket = h >> p.mod_bit;
	return true;
}

// (64 registers: next to three resident k_dp_round workgroups a SIMD has 128 left)
__global__ __launch_bounds__(64 * SKETCH_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_sketch_count(const uint8_t *text, const int64_t *q_off, int32_t n_query,
                                                                                                          const uint8_t *aa13, const int64_t *ki, SketchParams p, int32_t *pcnt,
                                                                                                          uint32_t *pbkt, int64_t *n_anchor, int64_t *n_kept, int32_t *max_occ,
                                                                                                          int32_t *flag)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[256];
	tab[threadIdx.x] = aa13[threadIdx.x];
	__syncthreads();
	const int lane = (int)(threadIdx.x & 63);
	const int32_t q = (int32_t)blockIdx.x * SKETCH_WAVES + (int32_t)(threadIdx.x >> 6);
	if (q >= n_query) return;
	const int64_t o = q_off[q];
	const int32_t len = (int32_t)(q_off[q + 1] - o);
	const uint8_t *seq = text + o;
	int32_t *cnt = pcnt + o;
	uint32_t *bkt = pbkt + o;
	// ---- pass 1: seeds and their counts
	uint32_t n_seed = 0, vmax = 0, big = 0;
	for (int32_t i = lane; i < len; i += 64) {
		uint32_t b = 0;
		int32_t c = -1;
		if (sketch_seed_at(seq, i, tab, p, &b)) {
			const int64_t st = ki[b], en = (int64_t)b + 1 < p.n_bucket ? ki[b + 1] : p.n_kb;
			const int64_t d = en - st;
			if (d > 0x7fffffffLL || d < 0) big = 1u, c = 0x7fffffff;
			else c = (int32_t)d;
			++n_seed;
			vmax = (uint32_t)c > vmax ? (uint32_t)c : vmax;
		}
		cnt[i] = c, bkt[i] = b;
	}
	n_seed = sketch_wave_sum(n_seed);
	big = __ballot(big != 0u) ? 1u : 0u;
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) { const uint32_t w = __shfl_xor(vmax, s); vmax = w > vmax ? w : vmax; }
	// ---- the cut-off (mp_cal_max_occ, map.c:126-141), in double like the host
	int32_t mo = p.max_occ, fl = (int32_t)big;
	if (!fl && n_seed >= 8u) {
		const uint32_t i25 = (uint32_t)(int64_t)((double)n_seed * .25 + .499), i75 = (uint32_t)(int64_t)((double)n_seed * .75 + .499);
		uint32_t a25 = 0, a75 = 0;
		for (int bit = 31 - __clz((int)(vmax | 1u)); bit >= 0; --bit) {
			const uint32_t t25 = a25 | 1u << bit, t75 = a75 | 1u << bit;
			uint32_t c25 = 0, c75 = 0;
			for (int32_t i = lane; i < len; i += 64) {
				const int32_t c = cnt[i];
				if (c >= 0) c25 += (uint32_t)c < t25 ? 1u : 0u, c75 += (uint32_t)c < t75 ? 1u : 0u;
			}
			c25 = sketch_wave_sum(c25), c75 = sketch_wave_sum(c75);
			if (c25 <= i25) a25 = t25;
			if (c75 <= i75) a75 = t75;
		}
		const double v = (double)a75 + (double)(a75 - a25) * 1.5 + 10.;
		if (!(v < 2147483648.0)) fl = 1;
		else { const int32_t cut = (int32_t)v; mo = cut < mo ? cut : mo; }
	}
	// ---- what the cut-off keeps
	uint32_t nk = 0;
	int64_t na = 0;
	if (!fl)
		for (int32_t i = lane; i < len; i += 64) {
			const int32_t c = cnt[i];
			if (c > 0 && c <= mo) ++nk, na += (int64_t)c;
		}
	nk = sketch_wave_sum(nk);
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) na += __shfl_xor(na, s);
	if (lane == 0) n_anchor[q] = na, n_kept[q] = (int64_t)nk, max_occ[q] = mo, flag[q] = fl;
}

// the kept seeds as the sift's jobs: dst = the running anchor offset, the bucket rides in `pad` (the host rebuilds its seed list
// from a download with it: mpa_dbg_seed_jobs)
__global__ __launch_bounds__(64 * SKETCH_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_sketch_emit(const int64_t *q_off, int32_t n_query, const int64_t *ki,
                                                                                                         const int32_t *pcnt, const uint32_t *pbkt, const int64_t *qfirst,
                                                                                                         const int64_t *jfirst, const int32_t *max_occ, const int32_t *flag,
                                                                                                         SeedJobDev *jobs)
{
	MPA_SHORT_KERNEL();
	const int lane = (int)(threadIdx.x & 63);
	const int32_t q = (int32_t)blockIdx.x * SKETCH_WAVES + (int32_t)(threadIdx.x >> 6);
	if (q >= n_query || flag[q]) return;
	const int64_t o = q_off[q], j1 = jfirst[q + 1];
	const int32_t len = (int32_t)(q_off[q + 1] - o), mo = max_occ[q];
	int64_t j = jfirst[q], dst = qfirst[q];
	for (int32_t base = 0; base < len && j < j1; base += 64) {
		const int32_t i = base + lane;
		const int32_t c = i < len ? pcnt[o + i] : -1;
		const bool keep = c > 0 && c <= mo;
		const unsigned long long m = __ballot(keep);
		if (!m) continue;
		int64_t inc = keep ? (int64_t)c : 0;
#pragma unroll
		for (int s = 1; s < 64; s <<= 1) { const int64_t w = __shfl_up(inc, s); if (lane >= s) inc += w; }
		const int64_t total = __shfl(inc, 63);
		if (keep) {
			const uint32_t b = pbkt[o + i];
			const int64_t at = j + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
			if (at < j1) jobs[at] = SeedJobDev{ ki[b], dst + inc - (int64_t)c, c, i, q, (int32_t)b };   // (at < j1 always: the count pass kept the same seeds)
		}
		j += (int64_t)__popcll(m), dst += total;
	}
}

} // namespace mpa
