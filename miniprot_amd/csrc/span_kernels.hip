// span_kernels.hip -- the accepted spans between the DP rounds and the region CIGARs behind them on the device (MPA_GPU_SPANS=1;
// DESIGN.md section 4.10), included by stats_run.hip behind stats_kernels.hip: the walk kernels and these share pools, and no unit
// launches another's kernels.  The code itself is spans_core.h, the one source the host model runs too; this file is its device team
// and the kernels around it.
//   k_spans        one lane per plan: spans_accept, the plan's round-2 tasks counted and numbered inside its workgroup, the
//                  workgroup's sum
//   k_spans_emit   one lane per plan: the sums of the workgroups before its own added (the host's order: query-major, plans in
//                  order, left before right), records and tasks written densely where one download finds them
//   k_assemble     one wavefront per plan, four plans per workgroup: spans_assemble into the plan's slot of the CIGAR pool
//   k_task_bounds  (MPA_GPU_ROUND2=1) one lane per round-2 task: the three bounds the device planner sizes by (dp_results_core.h), a
//                  wave reduction and one vector atomic per wave and bound
// (MPA_GPU_ROUND1=1) the three kernels chained behind a DP round inside its one wait take a guard: the round's
// hand-off error word and its results header.  Either one non-zero: no result record and no genome byte is read, and the task count is 0.
// The tables (804 bytes) and the workgroup scan's four wave totals are k_spans' only LDS.  No capacity.  Plain vector stores only.

namespace mpa {

#define SPANS_BLOCK 256                                   /* plans per workgroup of k_spans / k_spans_emit */

struct SpansWave : StatsWave {};                          // the team of spans_core.h on the device: one wavefront

struct SpansArgs {
	const SpansPlan *plan;
	int32_t n_plan;
	const mpa_dp_rst_t *rst1;
	const uint8_t *text, *tabs, *seq;
	const int64_t *ctg_off, *ctg_len;
	SpansParams p;
	SpanRec *rec;                        // [n_plan] task numbers local to the plan
	mpa_dp_task_t *tmp;                  // [2 n_plan] plan i's tasks at 2 i
	int32_t *excl;                       // [n_plan] tasks of the plans before it in its workgroup
	int32_t *bsum;                       // [workgroups] tasks of the workgroup
	const int32_t *g_err = nullptr;      // (nullable) the round's hand-off error word and the bad-call word of its results header: when
	const int64_t *g_bad = nullptr;      // either is non-zero nobody wrote the records at rst1
};

// the guard of a chained step: plain loads, stream-ordered behind the round that wrote the words
__device__ __forceinline__ bool spans_guarded(const int32_t *g_err, const int64_t *g_bad)
{
	return (g_err && *g_err != 0) || (g_bad && *g_bad != 0);
}

__global__ __launch_bounds__(SPANS_BLOCK) void k_spans(SpansArgs x)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[(ALN_TAB_BYTES + 15) & ~15];
	__shared__ int32_t wsum[SPANS_BLOCK / 64];
	for (int i = (int)threadIdx.x; i < ALN_TAB_BYTES; i += SPANS_BLOCK) tab[i] = x.tabs[i];
	__syncthreads();
	const int32_t i = (int32_t)(blockIdx.x * SPANS_BLOCK + threadIdx.x);
	int32_t n = 0;
	if (i < x.n_plan && !spans_guarded(x.g_err, x.g_bad)) {
		const SpansPlan P = x.plan[i];
		const StatsGenome g{ x.seq, x.ctg_off[P.vid >> 1], x.ctg_len[P.vid >> 1], (int)(P.vid & 1) };
		n = spans_accept(x.p, P, x.rst1, g, tab, x.text, x.rec[i], x.tmp + 2 * (int64_t)i);   // (straight into global memory: no private copy)
	}
	int32_t total;
	const int32_t below = SpansWave::scan32(n, &total);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
	__syncthreads();
	int32_t before = 0, all = 0;
	for (int w = 0; w < SPANS_BLOCK / 64; ++w) { before += w < (int)(threadIdx.x >> 6) ? wsum[w] : 0; all += wsum[w]; }
	if (i < x.n_plan) x.excl[i] = before + below;
	if (threadIdx.x == 0) x.bsum[blockIdx.x] = all;
}

// head: int32 n_task at dst; rec_dst[n_plan]; task_dst[at most 2 n_plan], dense
__global__ __launch_bounds__(SPANS_BLOCK) void k_spans_emit(SpansArgs x, int32_t *head, SpanRec *rec_dst, mpa_dp_task_t *task_dst)
{
	MPA_SHORT_KERNEL();
	__shared__ int32_t wsum[SPANS_BLOCK / 64];
	int32_t part = 0;
	for (int32_t b = (int32_t)threadIdx.x; b < (int32_t)blockIdx.x; b += SPANS_BLOCK) part += x.bsum[b];
	part = SpansWave::sum(part);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = part;
	__syncthreads();
	int32_t base = 0;
	for (int w = 0; w < SPANS_BLOCK / 64; ++w) base += wsum[w];
	const int32_t i = (int32_t)(blockIdx.x * SPANS_BLOCK + threadIdx.x);
	if (spans_guarded(x.g_err, x.g_bad)) {                                 // (uniform: k_spans wrote no record and counted no task)
		if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) head[0] = 0;
		return;
	}
	if (i < x.n_plan) {
		// (the record as ten 8-byte words, then the two task numbers over it: no private copy of the record)
		const int32_t t0 = base + x.excl[i], lt = x.rec[i].left.task, rt = x.rec[i].right.task;
		const uint64_t *src = (const uint64_t*)(x.rec + i);
		uint64_t *dst = (uint64_t*)(rec_dst + i);
#pragma unroll
		for (int w = 0; w < (int)(sizeof(SpanRec) / 8); ++w) dst[w] = src[w];
		int32_t n = 0;
		if (lt >= 0) rec_dst[i].left.task = lt + t0, ++n;
		if (rt >= 0) rec_dst[i].right.task = rt + t0, ++n;
		for (int32_t k = 0; k < n; ++k) task_dst[t0 + k] = x.tmp[2 * (int64_t)i + k];
	}
	if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) head[0] = base + x.bsum[blockIdx.x];
}

// out[3], zero before the launch: prep chunks, largest nl, largest al of task[0, *n_task); the grid covers the list's capacity
__global__ __launch_bounds__(SPANS_BLOCK) void k_task_bounds(const mpa_dp_task_t *task, const int32_t *n_task, int64_t *out, const int32_t *g_err, const int64_t *g_bad)
{
	MPA_SHORT_KERNEL();
	if (spans_guarded(g_err, g_bad)) return;                               // (a chained step behind a round that failed: out stays zero)
	const int64_t i = (int64_t)blockIdx.x * SPANS_BLOCK + threadIdx.x;
	DpTaskBounds b{ 0, 0, 0 };
	if (i < (int64_t)*n_task) b = dp_task_bounds_of(task[i].nl, task[i].al);
	for (int d = 32; d > 0; d >>= 1) {
		const DpTaskBounds o{ (int64_t)__shfl_xor((long long)b.prep, d, 64), (int64_t)__shfl_xor((long long)b.max_nl, d, 64), (int64_t)__shfl_xor((long long)b.max_al, d, 64) };
		dp_task_bounds_join(b, o);
	}
	if ((threadIdx.x & 63) == 0 && (b.prep | b.max_nl | b.max_al)) {       // (all three are >= 0)
		atomicAdd((unsigned long long*)out, (unsigned long long)b.prep);
		atomicMax((unsigned long long*)out + 1, (unsigned long long)b.max_nl);
		atomicMax((unsigned long long*)out + 2, (unsigned long long)b.max_al);
	}
}

struct AsmArgs {
	const SpansPlan *plan;
	const SpanRec *rec;
	int32_t n_plan;
	const SegRec *gap;
	const mpa_dp_rst_t *rst1, *rst2;
	const uint32_t *pool1, *pool2;
	const int64_t *slot_off;             // [n_plan + 1]
	uint32_t *cig;                       // the pool of the assembled CIGARs
	AsmRec *out;
};

__global__ __launch_bounds__(64 * STATS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_assemble(AsmArgs x)
{
	MPA_SHORT_KERNEL();
	const int32_t j = (int32_t)blockIdx.x * STATS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (j >= x.n_plan) return;
	const int64_t o = x.slot_off[j];
	AsmRec A = spans_assemble<SpansWave>(x.plan[j], x.rec[j], x.gap, x.rst1, x.pool1, x.rst2, x.pool2, x.cig + o);
	A.cig_off = o;
	if ((threadIdx.x & 63) == 0) x.out[j] = A;
}

} // namespace mpa
