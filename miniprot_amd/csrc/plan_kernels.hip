// plan_kernels.hip -- refinement chains to regions, alignment plans, round-1 DP tasks and gap segments on the device (the part of
// rows a11 / a12 of DESIGN.md section 1 between the refinement and DP round 1; MPA_GPU_PLANS=1), included by seed_run.hip behind region_kernels.hip: the chain
// tail of that unit launches them for the refinement.  The code itself is plans_core.h, the one source the host model runs too; this
// file is its device team, its genome reader and the kernels around it.
//   k_plans      one wavefront per query, four queries per workgroup: the chains of the query's refinement windows where
//                k_chain_extract left them -> its regions, plans, tasks and segments (fixed-size records) and their numbers
//   k_plan_pack  the kept records and the counts of every query into pinned host memory
// The tables (codon table, aa20, substitution matrix: 804 bytes) are the workgroup's only LDS; the digit tables of the region order
// live in global memory next to the rest of the query's scratch, which is carved from its windows and anchors.  No capacity.  Plain
// vector stores only.

namespace mpa {

#define PLANS_WAVES 4                                     /* queries per workgroup */

struct PlansWave : RegionsWave {};                        // the team of plans_core.h on the device: one wavefront

// one strand of the resident 4-bit genome; outside the contig a position reads as N
struct PlansStrand {
	const uint8_t *seq;
	int64_t off, len;
	int rev;
	__device__ __forceinline__ uint32_t base(int64_t x) const { return x < 0 || x >= len ? 4u : strand_base(seq, off, len, rev, x); }
};
struct PlansGenome {
	const uint8_t *seq;
	const int64_t *ctg_off, *ctg_len;
	__device__ __forceinline__ int64_t off(int32_t c) const { return ctg_off[c]; }
	__device__ __forceinline__ int64_t len(int32_t c) const { return ctg_len[c]; }
	__device__ __forceinline__ PlansStrand strand(uint32_t vid) const { return PlansStrand{ seq, ctg_off[vid >> 1], ctg_len[vid >> 1], (int)(vid & 1) }; }
};

// Query q has the windows [win0[q], win0[q + 1]); window w's chains and anchors lie at u / a + first[w] (where the extraction left
// them), offa[] is the prefix of the windows' extracted anchors.  With w0 = win0[q] and a0 = offa[w0], everything of the query that
// is sized by its windows lies at w0, everything sized by its anchors at a0, its tasks at 4 w0 + a0.
struct PlansArgs {
	const int64_t *first, *nu, *offa;
	const uint64_t *u;
	uint64_t *a;
	const PlansWindow *win;
	const int64_t *win0, *q_off;         // [n_query + 1] first window; first residue in text
	const uint8_t *text, *tabs;
	PlansGenome g;
	PlansParams p;
	RegionRec *tmp;
	Pair64 *key;
	SortRange *stack;                    // query q at w0 / 64 + 5 q
	uint32_t *hist;                      // 768 per query
	int32_t *prim, *flag, *list, *ctl;   // ctl: 2 per query
	uint64_t *cov, *ext;
	int64_t *aoff;
	RegionRec *reg;
	PlanRec *plan;
	mpa_dp_task_t *task;
	SegRec *seg;
	PlansCounts *cnt;                    // [n_query]
};

// (the budget of DESIGN.md section 5 (3) for a kernel next to three resident k_dp_round workgroups: 64 registers, no scratch)
__global__ __launch_bounds__(64 * PLANS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_plans(PlansArgs x, int32_t n_query)
{
	MPA_SHORT_KERNEL();
	__shared__ uint8_t tab[(ALN_TAB_BYTES + 15) & ~15];
	for (int i = (int)threadIdx.x; i < ALN_TAB_BYTES; i += 64 * PLANS_WAVES) tab[i] = x.tabs[i];
	__syncthreads();
	// (the wave's number through readfirstlane: the query's offsets and everything derived from them stay scalar)
	const int32_t q = (int32_t)blockIdx.x * PLANS_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	if (q >= n_query) return;
	const int64_t w0 = x.win0[q], n = x.win0[q + 1] - w0;
	PlansCounts c{ 0, 0, 0, 0 };
	if (n > 0 && n <= INT32_MAX) {
		const int64_t a0 = x.offa[w0];
		const PlansQuery Q{ (int32_t)n, q, (int32_t)(x.q_off[q + 1] - x.q_off[q]), x.win + w0, x.first + w0, x.first + w0, x.nu + w0, x.u, x.a, x.text + x.q_off[q] };
		const PlansScratch S{ x.tmp + w0, x.key + w0, x.stack + (w0 / 64 + 5 * (int64_t)q), x.hist + 768 * (int64_t)q, x.prim + w0, x.cov + w0, x.ext + w0, x.aoff + w0,
		                      x.flag + a0, x.list + a0, x.ctl + 2 * (int64_t)q };
		c = plans_core<PlansWave>(x.p, Q, x.g, tab, S, x.reg + w0, x.plan + w0, x.task + (4 * w0 + a0), x.seg + a0);
	}
	if ((threadIdx.x & 63) == 0) x.cnt[q] = c;
}

// the kept records of every query, where its windows and anchors put them; the destinations may be pinned host memory.  Every
// record is a whole number of 8-byte words
__global__ __launch_bounds__(256) void k_plan_pack(const int64_t *win0, const int64_t *offa, const PlansCounts *cnt, const RegionRec *reg, const PlanRec *plan,
                                                   const mpa_dp_task_t *task, const SegRec *seg, RegionRec *reg_dst, PlanRec *plan_dst, mpa_dp_task_t *task_dst, SegRec *seg_dst,
                                                   PlansCounts *cnt_dst)
{
	MPA_SHORT_KERNEL();
	const int32_t q = blockIdx.x;
	const int64_t w0 = win0[q], a0 = offa[w0];
	const PlansCounts c = cnt[q];
	auto copy = [](const void *src, void *dst, int64_t words) {
		const uint64_t *s = (const uint64_t*)src;
		uint64_t *d = (uint64_t*)dst;
		for (int64_t i = threadIdx.x; i < words; i += 256) d[i] = s[i];
	};
	copy(reg + w0, reg_dst + w0, (int64_t)c.n_reg * (int64_t)(sizeof(RegionRec) / 8));
	copy(plan + w0, plan_dst + w0, (int64_t)c.n_plan * (int64_t)(sizeof(PlanRec) / 8));
	copy(task + (4 * w0 + a0), task_dst + (4 * w0 + a0), (int64_t)c.n_task * (int64_t)(sizeof(mpa_dp_task_t) / 8));
	copy(seg + a0, seg_dst + a0, (int64_t)c.n_seg * (int64_t)(sizeof(SegRec) / 8));
	if (threadIdx.x == 0) cnt_dst[q] = c;
}
static_assert(sizeof(RegionRec) % 8 == 0 && sizeof(PlanRec) % 8 == 0 && sizeof(mpa_dp_task_t) % 8 == 0 && sizeof(SegRec) % 8 == 0, "k_plan_pack copies 8-byte words");

} // namespace mpa
