// host_batch.h -- the state of a batch in the stage machine (mpa_batch_*) and what its host files share: host_plan.cpp (stage A: seeding,
// planning, round-1 tasks), host_align.cpp (the steps between "DP results arrive" and "regions ranked"), host_map.cpp (the stage
// machine), host_pipeline.cpp (the stream), host_pool.cpp (the worker pools) and host_hooks.cpp (the test hooks of stage A).
// Host-only: no device unit includes it.
#pragma once
#include <cstdlib>
#include <functional>
#include <memory>
#include "host_core.h"

namespace mpa {

struct Segment {                     // one mp_align_seq() call (align.c:62-80)
	int32_t ne0, ne1, ae0, ae1;      // window-relative nt span (w.r.t. vs0) and protein span
	int32_t task = -1;               // DP task index within its round, -1 = ungapped shortcut
	int32_t score = 0;
	std::vector<uint32_t> cigar;     // filled when the DP result arrives
};

struct AlignPlan {                   // the state of one mp_align() call
	int32_t reg = -1;
	int64_t as = 0, ae = 0, vs0 = 0, vs1 = 0;
	int32_t i0 = 0, as1 = 0;
	int32_t t_left = -1, t_left2 = -1, t_right = -1, t_right2 = -1;
	int32_t l_nt = 0, l_aa = 0, r_nt = 0, r_aa = 0;
	int64_t mid_ve = 0;              // r->ve / r->qe after the gap-patching loop
	int32_t mid_qe = 0;
	bool has_right = false;
	Segment left_span, right_span;   // the spans accepted by the two extensions, re-aligned with traceback (round 3)
	bool has_left_span = false, has_right_span = false;
	bool l_rep = false, r_rep = false;   // the terminal-exon repeat of that side counted (MPA_SPANS_DUMP)
	int32_t n_merged = 0;            // segment boundaries that merged two words into one (MPA_SPANS_DUMP)
	std::vector<Segment> gaps;       // gaps between consecutive kept anchors: independent of the extensions (round 1)
};

struct QueryState {
	int32_t qid = 0, qlen = 0;
	const char *seq = nullptr;
	std::vector<Region> regs;
	std::vector<AlignPlan> plans;
	std::vector<uint64_t> seeds;         // kept seeds (query position << 32 | index bucket), ascending; only between the seeding sub-stages
	std::vector<uint64_t> ext_refine;    // per region: window extension limits of the refinement (between the planning sub-stages)
	int32_t n_chains = 0;                // main chains of the query before the selection (MPA_REGIONS_DUMP)
	int64_t win0 = 0;                    // first refinement window of this query in the batch's list (device refinement)
	int64_t n_anchor = 0;                // anchors those seeds expand to
	bool seeds_ready = false;            // seeds / n_anchor / max_occ are the host's (stage_seeds has run); false after a device sketch: built when the host anchor stage asks
	int32_t max_occ = 0;                 // the occurrence cut-off in force for this query (stage_seeds)
	std::vector<mpa_dp_task_t> local1;   // this query's round-1 DP tasks (plan fields index into it)
	int64_t base1 = 0;                   // where local1 starts in the batch's round-1 task array
};

} // namespace mpa

struct mpa_batch_s {
	const mpa_idx_s *mi = nullptr;
	mpa_mapopt_t opt;
	mpa_dpopt_t dpopt;
	mpa_qbatch_t q;
	int n_threads = 1;
	int round = 0;                   // 0: before round 1; 1, 2: tasks of that round are out (extensions + gaps; accepted spans); 4: done
	std::vector<mpa::QueryState> qs;
	std::vector<mpa_dp_task_t> tasks;
	bool seeded_on_device = false;   // between the two seeding phases: `sparse` holds the device's pre-chain result
	mpa::PrechainSparse sparse;
	// between the host half of seeding (sketch, lookup, cut-off: batch_sketch_phase) and its device half: the kept seeds of every
	// query as occurrence lists (one job per seed) and the first anchor of every query; empty = the batch is seeded on the host
	std::vector<mpa::SeedJob> seed_jobs;
	std::vector<int64_t> seed_qfirst;
	bool dev_sketch = false;         // MPA_GPU_SKETCH: the sketch phase built the shell only, the seeder runs the sketch on the device first
	mpa_ctx_t *dp_ctx = nullptr;     // the context that runs this batch's DP rounds (run_dp_rounds), null for a caller that drives the stage machine itself
	int64_t dp_n_pool = 0;           // ... and the words of the CIGAR pool its last mpa_dp_run left there
	// MPA_GPU_SPANS (1 or model) between the rounds: how round 1 was taken (0 host, 1 shared core, 2 device), the round-1 results and
	// their CIGAR pool kept for the step behind round 2 (the pool is the executor's own block on the device path: run_dp_rounds hands
	// it over instead of freeing it), and where k_assemble left every plan's words on the device (empty: not there)
	int spans_src = 0;
	bool spans_want_pool = false;
	std::vector<mpa_dp_rst_t> sp_rst1;
	uint32_t *sp_pool1 = nullptr;
	std::vector<int64_t> sp_cig_off;
	// MPA_GPU_ROUND2: what the device step between the rounds left for a resident round 2 (d_tasks null: nothing);
	// whether round 2 ran that way -- its dense pool is then on dp_ctx (dp_n_pool words) and not with the host -- and its records there
	mpa::DpResidentIn r2_in;
	bool r2_resident = false;
	const mpa_dp_rst_t *r2_rst_dev = nullptr;
	// MPA_GPU_ROUND1: round 1 ran with the step between the rounds chained into its submission -- r1_io is what the
	// step left (taken by spans_take_round1 in place of a device call, then cleared), and round 1's dense pool (r1_n_pool words) is on dp_ctx
	// in the spans step's pool and not with the host: sp_pool1 stays null until a fallback fetches the words
	bool r1_prefetched = false, r1_resident = false;
	mpa::SpansIO r1_io;
	int64_t r1_n_pool = 0;
	// MPA_GPU_FINISH (1 or model): the batch's flat result when the step behind the walks ranked and laid it out
	// (null: stage_finish ranked the regions and mpa_batch_finish flattens them), and where its cs bodies came from (Region::cs_src)
	std::unique_ptr<mpa_result_s> flat;
	int flat_cs_src = 0;
	// MPA_GPU_FORMAT=1: the batch's query names, handed over by the stream pipeline before the DP stage when it
	// will want the batch's text (null: nobody formats this batch, or not on the device)
	const char *const *fmt_names = nullptr;
	~mpa_batch_s() { free(sp_pool1); }
};

// The query side of the device refinement: the query's k-mers (packed word, index of the last residue) grouped by word -- in
// ascending hash order, positions ascending inside a group, as the pairing of map.c:53-79 meets them in the sorted list.
// (Outside the namespace, where it was: the library's default visibility exports a few std::vector<QueryGroups> members under that name.)
struct QueryGroups { std::vector<uint32_t> gword, gcount, qpos; };

namespace mpa {

// What crosses between the files (internal to the library: hidden, so the dynamic symbol table does not grow):
#define MPA_HOST_LOCAL __attribute__((visibility("hidden")))
// host_map.cpp -> host_align.cpp: round 1 in / round 2 out, and the last round in (CIGARs, statistics, cs strings and rows, ranking)
MPA_HOST_LOCAL int spans_take_round1(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool);
MPA_HOST_LOCAL int take_round3(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool);
// ... and (MPA_GPU_ROUND1=1) round 1 itself with the step behind it in one submission; declined: *why, or the last error
MPA_HOST_LOCAL int spans_round1_resident(mpa_batch_s *b, mpa_ctx_t *ctx, const mpa_dpopt_t *dpopt, int64_t n, const mpa_dp_task_t *tasks, mpa_dp_rst_t *rst, int64_t *n_pool, const char **why);
// host_align.cpp -> host_plan.cpp: plan_round1 makes the gap segments with it, take_round1_emit_round2 the accepted spans
MPA_HOST_LOCAL void make_segment(mpa_batch_s *b, const QueryState &qs, const Region &r, const AlignPlan &pl, int32_t ne0, int32_t ne1, int32_t ae0, int32_t ae1,
                                 int32_t qi, int32_t pi, std::vector<mpa_dp_task_t> &tasks, Segment &s);
// host_pipeline.cpp -> host_map.cpp: the DP rounds of a planned batch on a device context
MPA_HOST_LOCAL int run_dp_rounds(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_qbatch_t *q, mpa_batch_s *b);

// host_map.cpp, host_pipeline.cpp, host_hooks.cpp -> host_plan.cpp: the phases of stage A.  sketch (host: seeds of every query and the
// seed jobs) -> device seed (anchors, pre-chain, main chain; false = error) -> plan (windows, refinement, plans, round-1 tasks)
MPA_HOST_LOCAL mpa_batch_s *batch_shell(const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads);
MPA_HOST_LOCAL mpa_batch_s *batch_sketch_phase(bool have_device, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads);
MPA_HOST_LOCAL void batch_host_seeds(mpa_batch_s *b, bool have_device);
MPA_HOST_LOCAL bool batch_device_seed_phase(mpa_ctx_t *seed_ctx, mpa_batch_s *b, bool want_chains, SeedHold *hold, double *sketch_ms = nullptr, bool for_planner = false);
MPA_HOST_LOCAL mpa_batch_s *batch_seed_phase(mpa_ctx_t *seed_ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, bool want_chains = true, SeedHold *hold = nullptr, bool for_planner = false);
MPA_HOST_LOCAL void batch_plan_phase(mpa_batch_s *b, mpa_ctx_t *rctx);
MPA_HOST_LOCAL mpa_batch_s *batch_begin_impl(mpa_ctx_t *seed_ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads);
MPA_HOST_LOCAL void emit_round1(mpa_batch_s *b);
struct MPA_HOST_LOCAL SeedModeScope { int keep; explicit SeedModeScope(int m); ~SeedModeScope(); };   // forces MPA_GPU_SEED for the calling thread over a scope (the mpa_dbg_* hooks, for their own call)
// host_hooks.cpp -> host_plan.cpp: the per-query steps that the test hooks of stage A call one by one
enum SeedRoute { SEED_ON_HOST = 0, SEED_PRECHAIN, SEED_DIRECT };
MPA_HOST_LOCAL SeedRoute seed_route(const mpa_mapopt_t &opt, const mpa_idxopt_t &io);
MPA_HOST_LOCAL void stage_seeds(mpa_batch_s *b, QueryState &qs);
MPA_HOST_LOCAL void stage_anchors_host(mpa_batch_s *b, QueryState &qs, std::vector<uint64_t> &a);
MPA_HOST_LOCAL void stage_anchors_from_device(mpa_batch_s *b, QueryState &qs, const PrechainSparse &ps, std::vector<uint64_t> &a);
MPA_HOST_LOCAL void query_words(const char *aa, int32_t l_aa, int32_t k, std::vector<uint32_t> &w);
MPA_HOST_LOCAL void query_groups(const char *aa, int32_t l_aa, int32_t k, QueryGroups &out);
MPA_HOST_LOCAL void gather_query_groups(const QueryGroups *per, int64_t n_q, RefineGroupsHost &G);
// mp_refine_reg (map.c:32-111): re-seed the region's window with all 5-mers at base resolution, re-chain
// The query side of the refinement seeding, built once per query: its k-mers sorted by hash and a bitmap over the
// hash space (2^(4k) bits; one per worker thread, reused) with the query's hashes set.
struct RefineQuery {
	std::vector<uint64_t> qk;
	std::vector<uint64_t> *filter = nullptr;
	int32_t kmer = 0;
	static std::vector<uint64_t> &thread_filter(int32_t kmer) {
		static thread_local std::vector<uint64_t> f;
		const size_t words = ((size_t)1 << (4 * kmer)) / 64 + 1;
		if (f.size() < words) f.assign(words, 0);
		return f;
	}
	std::vector<uint32_t> words;                      // packed k-mer words of the query (bitmap keys)
	RefineQuery(const char *aa, int32_t l_aa, int32_t k, bool want_filter = true) : kmer(k) {
		sketch_protein(aa, l_aa, k, 0, qk);
		sort_u64(qk.data(), qk.data() + qk.size());
		if (k <= 6 && want_filter) {
			filter = &thread_filter(k);
			const uint8_t *aa13 = tab_aa13();
			const uint32_t mask = (1U << 4 * k) - 1;
			uint32_t w = 0;
			for (int32_t i = 0, run = 0; i < l_aa; ++i) {
				const uint32_t c = aa13[(uint8_t)aa[i]];
				if (c >= 14) { run = 0, w = 0; continue; }
				w = (w << 4 | c) & mask;
				if (++run >= k) words.push_back(w), (*filter)[w >> 6] |= 1ULL << (w & 63);
			}
		}
	}
	~RefineQuery() { if (filter) for (uint32_t w : words) (*filter)[w >> 6] = 0; }
};
MPA_HOST_LOCAL void refine_region_pairs(const mpa_idx_s *mi, const mpa_mapopt_t &opt, const RefineQuery &rq, const Region &r, int32_t extl, int32_t extr, const uint64_t *dev_hits, int64_t n_dev_hits, std::vector<uint64_t> &a);
static inline ChainParams refine_chain_params(const mpa_mapopt_t &opt)
{
	return ChainParams{ opt.max_intron, opt.max_gap, opt.bw, opt.max_chn_max_skip, opt.max_chn_iter, opt.min_chn_cnt, opt.min_chn_sc,
	                    opt.chn_coef_log, !(opt.flag & MPA_MF_NO_SPLICE), opt.kmer2, 0 };
}
static inline ChainParams main_chain_params(const mpa_idx_s *mi, const mpa_mapopt_t &opt)
{
	return ChainParams{ opt.max_intron, opt.max_gap, opt.bw, opt.max_chn_max_skip, opt.max_chn_iter, opt.min_chn_cnt, opt.min_chn_sc,
	                    opt.chn_coef_log, !(opt.flag & MPA_MF_NO_SPLICE), mi->opt.kmer, mi->opt.bbit };
}

// The calling thread's worker pool (host_pool.cpp); the pool, its lane and its share of the threads are set by the stream pipeline's
// stage threads for themselves
MPA_HOST_LOCAL void parallel_run(int n_threads, int64_t n, const std::function<void(int64_t)> &fn);
MPA_HOST_LOCAL void pool_stage_enter(int lane, int thread_div, const char *label);
MPA_HOST_LOCAL void pool_stage_leave();
template<typename F> static void parallel_for(int n_threads, int64_t n, F fn)
{
	std::function<void(int64_t)> f = fn;
	parallel_run(n_threads, n, f);
}

// A step that has a device twin and a model behind a knob (MPA_GPU_REGIONS, _PLANS, _STATS, _CS, _ROWS, _SPANS): 0 / unset = the host
// functions; 1 = on the device; model = the host instance of the device's code with a team of one (the *_core.h headers: the CPU tests)
enum StepMode { STEP_HOST = 0, STEP_DEVICE, STEP_MODEL };
static inline StepMode step_mode(const char *env_name)
{
	const char *e = getenv(env_name);                   // (read per call: the tests flip it)
	if (!e || !*e) return STEP_HOST;
	if (!strcmp(e, "model")) return STEP_MODEL;
	return atoi(e) != 0 ? STEP_DEVICE : STEP_HOST;
}

// host_align.cpp -> host_finish.cpp (MPA_GPU_FINISH=model): ranking and flat result of the batch through finish_core.h on the host, into b->flat
MPA_HOST_LOCAL bool batch_finish_model(mpa_batch_s *b);

static inline uint8_t codon_aa(const uint8_t *nt)
{
	return nt[0] > 3 || nt[1] > 3 || nt[2] > 3 ? 21 : tab_codon()[nt[0] << 4 | nt[1] << 2 | nt[2]];
}

// the packed genome as the shared cores read it on the host: strand_base() of dev_common.h in plain C++
struct StatsGenomeHost {
	const uint8_t *seq;
	int64_t off, len;
	int rev;
	uint32_t base(int64_t x) const
	{
		if (x < 0 || x >= len) return 4;
		const int64_t p = rev ? off + len - 1 - x : off + x;
		const uint32_t c = (seq[p >> 1] >> ((p & 1) * 4)) & 0xf;
		return rev && c < 4 ? 3 - c : c;
	}
};
static inline StatsGenomeHost genome_strand(const mpa_idx_s *mi, uint32_t vid)
{
	const Contig &c = mi->ctg[vid >> 1];
	return StatsGenomeHost{ mi->seq.data(), c.off, c.len, (int)(vid & 1) };
}

// the fixed-size records of the shared cores into the host's state and back.  Region::a stays empty; a shortcut segment gets its
// one-word CIGAR, a DP segment's words are left as they are
static inline void region_from_rec(Region &x, const RegionRec &y)
{
	x.off = y.off, x.cnt = y.cnt, x.id = y.id, x.parent = y.parent, x.n_sub = y.n_sub, x.subsc = y.subsc, x.chn_sc = y.chn_sc, x.chn_sc_ungap = y.chn_sc_ungap;
	x.vid = y.vid, x.qs = y.qs, x.qe = y.qe, x.vs = y.vs, x.ve = y.ve, x.split = y.split;
}
static inline void segment_from_rec(Segment &s, const SegRec &z)
{
	s.ne0 = z.ne0, s.ne1 = z.ne1, s.ae0 = z.ae0, s.ae1 = z.ae1, s.task = z.task, s.score = z.score;
	if (z.task < 0) s.cigar.assign(1, (uint32_t)(z.ae1 - z.ae0) << 4);
}
static inline SegRec rec_of_segment(const Segment &s) { return SegRec{ s.ne0, s.ne1, s.ae0, s.ae1, s.task, s.score }; }

} // namespace mpa
