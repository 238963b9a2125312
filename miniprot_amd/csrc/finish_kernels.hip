// finish_kernels.hip -- the aligned regions of a batch to its flat result on the device (MPA_GPU_FINISH=1),
// included by stats_run.hip, whose dev_finish() launches them.  The code itself is finish_core.h, the one source the host model runs
// too; this file is its device team and the kernels around it.
//   k_finish_fill    (behind the walks) one lane per record: the statistics, cs length and rows width of its alignment from the walks'
//                    out records, where they lie, into the record
//   k_finish_rank    one wavefront per query: its records -> rank order, the ranking's fields and the query's counts.  The query's
//                    working records and sort keys lie in LDS up to FINISH_LDS_REGS = 64 regions (13 KB; the sort is then the
//                    reference's insertion sort); a larger query works in HBM scratch carved from the number of its regions, digit
//                    tables included.  No query is refused for its size.
//   k_finish_scan    the exclusive prefix of the counts over the batch: one workgroup, FINISH_SCAN queries per step and a carry; a copy
//                    goes to the pinned block
//   k_finish_gather  one workgroup per query, one wavefront per kept hit at a time: the hit record and the copies of its words,
//                    features and text into the dense arrays, lane-strided.  The arrays are pinned host memory: only what the result
//                    holds crosses the bus, and nothing has to be sized on the host before the call's one wait
// Plain vector stores only.

namespace mpa {

#define FINISH_SCAN 256                                   /* queries per step of k_finish_scan (its workgroup) */
#define FINISH_GATHER_WAVES 4                             /* hits a workgroup of k_finish_gather copies side by side */

struct FinishWave : CoopWave {                            // the team of finish_core.h on the device: one wavefront
	static __device__ __forceinline__ int64_t sum64(int64_t v)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		return v;
	}
};

struct FinishArgs {
	const int64_t *first;            // [n_query + 1] the queries' records
	const FinRec *rec;
	const int32_t *big;              // [n_query] a query of more than FINISH_LDS_REGS regions: its number among those, else -1
	FinParams p;
	FinOut *out;                     // [n_rec] kept hits by rank, query q at first[q]
	FinCounts *cnt, *off;            // [n_query], [n_query + 1]
	// HBM scratch of the large queries: per record at first[q], per query at big[q]
	FinRank *tmp, *r;
	Pair64 *key;
	SortRange *stack;                // query q at first[q] / 64 + 8 big[q]
	uint32_t *hist;                  // 768 per large query
	int32_t *prim, *ctl;
	uint64_t *cov;
};

__global__ __launch_bounds__(256) void k_finish_fill(FinRec *rec, int64_t n_rec, const AlnStatsOut *st, const AlnCsOut *cs, const AlnRowsOut *rows, int32_t show_trans)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n_rec) finish_fill_core(rec[i], st, cs, rows, show_trans);
}

__global__ __launch_bounds__(64) void k_finish_rank(FinishArgs x, int32_t n_query)
{
	MPA_SHORT_KERNEL();
	__shared__ FinRank s_tmp[FINISH_LDS_REGS], s_r[FINISH_LDS_REGS];
	__shared__ Pair64 s_key[FINISH_LDS_REGS];
	__shared__ int32_t s_prim[FINISH_LDS_REGS], s_ctl[2];
	__shared__ uint64_t s_cov[FINISH_LDS_REGS];
	const int32_t q = (int32_t)blockIdx.x;
	if (q >= n_query) return;
	const int64_t f = x.first[q], n = x.first[q + 1] - f;
	if (n > INT32_MAX) return;                            // (dev_finish refuses such a table)
	static_assert(FINISH_LDS_REGS <= 64, "an LDS-sized query takes sort_pairs_by_x_core's insertion sort: no stack, no digit tables");
	FinScratch S{ s_tmp, s_r, s_key, nullptr, nullptr, s_prim, s_cov, s_ctl };
	if (n > FINISH_LDS_REGS) {
		const int64_t b = x.big[q];
		S = FinScratch{ x.tmp + f, x.r + f, x.key + f, x.stack + (f / 64 + 8 * b), x.hist + 768 * b, x.prim + f, x.cov + f, x.ctl + 2 * b };
	}
	finish_rank_core<FinishWave>(x.p, x.rec + f, (int32_t)n, S, x.out + f, x.cnt + q);
}

__global__ __launch_bounds__(FINISH_SCAN) void k_finish_scan(const FinCounts *cnt, int32_t n_query, FinCounts *off, FinCounts *host_off)
{
	MPA_SHORT_KERNEL();
	__shared__ int64_t s_tot[FINISH_SCAN / 64][8];
	const int t = (int)threadIdx.x, wave = t >> 6;
	int64_t carry[7] = { 0, 0, 0, 0, 0, 0, 0 };
	for (int32_t base = 0; base < n_query; base += FINISH_SCAN) {
		const int32_t q = base + t;
		const bool have = q < n_query;
		const FinCounts c = have ? cnt[q] : FinCounts{ 0, 0, 0, 0, 0, 0, 0, 0 };
		const int64_t v[7] = { c.hit, c.cigar, c.feat, c.cs, c.rows, c.n_cs, c.n_rows };
		int64_t e[7];
#pragma unroll
		for (int k = 0; k < 7; ++k) {
			int64_t total;
			e[k] = CoopWave::scan_excl(v[k], &total);
			if ((t & 63) == 0) s_tot[wave][k] = total;
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 7; ++k) {
			int64_t below = 0, all = 0;
#pragma unroll
			for (int w = 0; w < FINISH_SCAN / 64; ++w) { const int64_t s = s_tot[w][k]; below += w < wave ? s : 0, all += s; }
			e[k] += carry[k] + below, carry[k] += all;
		}
		if (have) off[q] = host_off[q] = FinCounts{ e[0], e[1], e[2], e[3], e[4], e[5], e[6], 0 };
		__syncthreads();
	}
	if (t == 0) off[n_query] = host_off[n_query] = FinCounts{ carry[0], carry[1], carry[2], carry[3], carry[4], carry[5], carry[6], 0 };
}

__global__ __launch_bounds__(64 * FINISH_GATHER_WAVES) void k_finish_gather(FinishArgs x, int32_t n_query, const uint32_t *words, const void *feats, const char *cs_text,
                                                                           const char *rows_text, FinDst dst)
{
	MPA_SHORT_KERNEL();
	const int32_t q = (int32_t)blockIdx.x;
	if (q >= n_query) return;
	const FinCounts at = x.off[q];
	const int64_t f = x.first[q], k = x.off[q + 1].hit - at.hit;
	for (int64_t j = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6)); j < k; j += FINISH_GATHER_WAVES) {
		const FinOut o = x.out[f + j];
		finish_gather_core<FinishWave>(q, x.rec[f + o.src], o, at.hit + j, at, words, feats, cs_text, rows_text, dst);
	}
}

} // namespace mpa
