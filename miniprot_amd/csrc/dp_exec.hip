// dp_exec.hip -- host-side executor of the batched spliced DP: the implementation of mpa_dp_run().
//
// A batch of ns_global_gs16b() calls (nasw.h:135; call sites align.c:73,288,293,322,327) is planned on the host (dp_plan.cpp: classes,
// order, pool layout, waves, traceback chunks, the round's unit list -- nothing of it needs the device; with MPA_GPU_DPPLAN=1 the same
// plan is made by the kernels of dp_plan_kernels.hip, dev_dp_plan() below, and the uploads of what they wrote are skipped) and then enqueued as
//   1. one upload from a pinned staging block, k_prep_rows / k_prep_prof (per-row records + query profiles, written once to HBM),
//   2. ONE k_dp_round launch for every DP unit of the round: the extension calls of every class up to 1024 columns, the packed
//      sweeps of the checkpointed traceback and the plain traceback sweeps of the first traceback chunk, costliest unit first
//      (MPA_DP_POOL=1: the units go to the resident workers of the device's pool, k_dp_worker, instead),
//   3. next to it on side streams: k_ext_huge (MPA_DP_HUGE_WG=1: and k_ext_huge_wg, one wave per column block, for the calls of four
//      blocks or more) + k_ext_replay (wider calls, and whatever the int16 sweeps may not take), k_lite_wide, k_lite_w8
//      (129..256-column checkpointed calls), the 512/1024-thread traceback classes, the anti-diagonal prototype, and (MPA_DP_MB_WG=1)
//      k_glob_mb_wg, one wave per column block, over the T_MB traceback calls, whose units in the round then find no call,
//   4. k_backtrack per traceback chunk (chunks after the first: stand-alone k_glob_* launches, serial), k_walk for the
//      checkpointed calls, one download, one host wait, k_cigar_gather (MPA_GPU_ROUND2=1, a batch's round 2 from tasks that are on the
//      device: the result records and the dense pool's offsets by the kernels of dp_results_kernels.hip and the gather in front of
//      that one wait, the dense pool left on the device -- dp_run_resident() below),
// bracketed by HIP events (mpa_dp_last_stats feeds bench.py's roofline record).  mpa_dp_run_impl is that list of phases.  There is no
// CPU fallback here by design.  This unit holds the DP only (kernels: dp_kernels.hip -- what k_dp_round and k_dp_worker execute -- and,
// behind it, the launches of phases 1, 3 and 4 in dp_prep_kernels.hip, dp_lite_wide.hip, dp_huge_kernels.hip and
// dp_traceback_kernels.hip; dp_antidiag.hip, gs32_exec.hip); the context and its pools are dev_ctx.hip, the other stages seed_run.hip,
// refine_run.hip and index_run.hip.
#include <rocprim/device/device_radix_sort.hpp>
#include "dev_ctx.h"
#include "dp_kernels.hip"
#include "dp_prep_kernels.hip"
#include "dp_lite_wide.hip"
#include "dp_huge_kernels.hip"
#include "dp_traceback_kernels.hip"
#include "dp_antidiag.hip"
#include "dp_plan_kernels.hip"
#include "dp_results_kernels.hip"

namespace mpa {

template<int NW> static hipError_t launch_glob_wide(const GlobArgs &a, int n_groups, hipStream_t s, bool wide_ge = false)
{
	const size_t lds = GLOB_WIDE_LDS(NW);
	if (wide_ge) hipLaunchKernelGGL((k_glob_wide<NW, true>), dim3(n_groups), dim3(NW * 64), lds, s, a);
	else hipLaunchKernelGGL((k_glob_wide<NW, false>), dim3(n_groups), dim3(NW * 64), lds, s, a);
	return hipGetLastError();
}

// traceback classes T_16, T_32, T_64 (16/32/64 lanes) and T_MB (block-major, > 1024 columns) in one launch; a.waves = whole array
// (the traceback chunks after the first, which do not ride in the round's launch)
static hipError_t launch_glob_narrow(const GlobArgs &a, const int *first, const int *cnt, hipStream_t s, bool wide_ge = false)
{
	const size_t lds = GLOB_NARROW_LDS;
	NarrowMap m{};
	const int cls[4] = { T_16, T_32, T_64, T_MB };
	int total = 0;
	for (int k = 0; k < 4; ++k) m.first[k] = first[cls[k]], m.cnt[k] = cnt[cls[k]], total += cnt[cls[k]];
	if (wide_ge) hipLaunchKernelGGL(k_glob_narrow<true>, dim3((unsigned)total), dim3(64), lds, s, a, m);
	else hipLaunchKernelGGL(k_glob_narrow<false>, dim3((unsigned)total), dim3(64), lds, s, a, m);
	return hipGetLastError();
}

} // namespace mpa

namespace mpa {
// ---- DP worker pool: host side (the kernels and the protocol are in dp_kernels.hip, "The DP worker pool")
// MPA_DP_POOL=1 selects the pool; the default is one k_dp_round launch per round.  Measured (profiles/r05_experiments.txt): with
// identical sweep code the pool is level with the launches on the DP-bound config 5 (1.05-1.14 M against 1.09 M residues/s), 5-10 %
// behind on config 3 (19.4-19.8 M against 20.0-21.9 M) and a third behind on config 2 (17-ms batches: arming, the second host
// round trip and the L2 write-back weigh).  The hardware's workgroup dispatcher already IS a work-conserving queue across the
// launches in flight -- a slot that a finished unit frees goes to the oldest pending workgroup of ANY launch -- so what the pool
// adds (units taken wave by wave, a bounded DP population) buys no throughput here, and its round latency is longer because the
// rounds in flight share the workers instead of being served in order of arrival.
static bool dp_pool_enabled()
{
	static const bool on = [] { const char *e = getenv("MPA_DP_POOL"); return e && atoi(e) != 0; }();
	return on;
}
// resident worker workgroups the pool admits (MPA_DP_WORKERS).  The workers ask for a fifth of a CU's LDS plus a little, so four
// fit per CU (1 024 on the chip); the default keeps three per CU busy and leaves the fourth slot to the workgroups that arrive,
// find the pool full and leave -- and registers and LDS to the seeding kernels of the batches behind.
static int dp_pool_budget()
{
	static const int b = [] { const char *e = getenv("MPA_DP_WORKERS"); const int v = e ? atoi(e) : 768; return v < 1 ? 1 : v; }();
	return b;
}
// MPA_DP_TRACE=<file>: every unit of every round appends "slot generation unit kind priority start end" (100-MHz device ticks);
// tools/dp_trace.py turns that into resident units over time
static const char *dp_trace_path()
{
	static const char *p = [] { const char *e = getenv("MPA_DP_TRACE"); return e && *e ? e : (const char*)nullptr; }();
	return p;
}
// the calling context's slot, done word and worker stream (created on its first round); the device's pool on the first of all
static int pool_attach(mpa_ctx_t *ctx)
{
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	std::lock_guard<std::mutex> g(root->worker.pool_mu);
	if (!root->worker.dp_pool) {
		DpPool *p = nullptr;
		HIP_TRY(hipMalloc((void**)&p, sizeof(DpPool)));
		HIP_TRY(hipMemset(p, 0, sizeof(DpPool)));
		const int32_t budget = dp_pool_budget();
		HIP_TRY(hipMemcpy(&p->ctl.budget, &budget, 4, hipMemcpyHostToDevice));
		const int32_t acq = [] { const char *e = getenv("MPA_DP_ACQUIRE"); return e ? atoi(e) : 2; }();
		HIP_TRY(hipMemcpy(&p->ctl.acquire_mode, &acq, 4, hipMemcpyHostToDevice));
		HIP_TRY(hipEventCreate(&root->worker.pool_base));
		HIP_TRY(hipEventRecord(root->worker.pool_base, root->stream));
		root->worker.dp_pool = p;
	}
	if (ctx->worker.dp_slot < 0) {
		if (root->worker.pool_slots >= MPA_DP_SLOTS) { set_error("more than " + std::to_string(MPA_DP_SLOTS) + " contexts of one device run DP rounds"); return MPA_ERR_UNSUPPORTED; }
		HIP_TRY(hipHostMalloc((void**)&ctx->worker.dp_done, 64, hipHostMallocDefault));
		*(volatile int32_t*)ctx->worker.dp_done = 0;
		HIP_TRY(hipStreamCreateWithFlags(&ctx->worker.worker_stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&ctx->worker.arm_ev, hipEventDisableTiming));
		ctx->worker.dp_slot = root->worker.pool_slots++;
	}
	return MPA_OK;
}
// durations of the context's worker launches that have ended (wait: of all of them -- only when no round is pending anywhere, the
// workers then leave within microseconds) into the context's totals and the device's interval list
void pool_harvest(mpa_ctx_t *ctx, bool wait)
{
	if (ctx->worker.wl_busy.empty()) return;
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	(void)hipSetDevice(ctx->device);
	if (wait) (void)wait_stream(ctx, ctx->worker.worker_stream);
	size_t keep = 0;
	for (size_t k = 0; k < ctx->worker.wl_busy.size(); ++k) {
		WorkerBufs::WorkerLaunch w = ctx->worker.wl_busy[k];
		float a = 0, b = 0;
		if (hipEventQuery(w.e1) == hipSuccess && hipEventElapsedTime(&a, root->worker.pool_base, w.e0) == hipSuccess && hipEventElapsedTime(&b, root->worker.pool_base, w.e1) == hipSuccess) {
			ctx->total.ms_round += (double)(b - a), ctx->total.launches_round++;
			{ std::lock_guard<std::mutex> g(root->worker.pool_mu); root->worker.pool_iv.emplace_back(a, b); }
			ctx->worker.wl_free.push_back(w);
		} else ctx->worker.wl_busy[keep++] = w;
	}
	(void)hipGetLastError();
	ctx->worker.wl_busy.resize(keep);
}
// A round for the pool: the round's arguments (ha: pinned) and units into the lane's slot of the device's pool, the slot armed in
// stream order behind everything the round reads, the lane's workers launched (a worker takes any lane's units: their stream is
// never waited for by a round -- a round is complete when its last unit says so in pinned memory).  The unit list is in
// ctx->round.units already: whole-workgroup units [0, n_group), then the one-wave units.  *gen: what pool_wait_round waits for.
static int pool_launch_round(mpa_ctx_t *ctx, hipStream_t s, const ExtArgs &ea, const ExtWideArgs &wa, const GlobArgs &ga, DpRoundArgs *ha,
                             size_t n_units, size_t n_group, size_t round_lds, unsigned int *gen)
{
	int rc;
	if ((rc = pool_attach(ctx))) return rc;
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	DpPool *pool = root->worker.dp_pool;
	int n_slots;
	{ std::lock_guard<std::mutex> g(root->worker.pool_mu); n_slots = root->worker.pool_slots; }
	ha->ea = ea, ha->wa = wa, ha->ga = ga, ha->units = ctx->round.units.as<DpUnit>(), ha->n_group = (int32_t)n_group, ha->pad_ = 0;
	HIP_TRY(hipMemcpyAsync(&pool->args[ctx->worker.dp_slot], ha, sizeof(DpRoundArgs), hipMemcpyHostToDevice, s));
	long long *d_trace = nullptr;
	if (dp_trace_path()) {
		if ((rc = ctx->worker.dp_trace.ensure(n_units * 16))) return rc;
		HIP_TRY(hipMemsetAsync(ctx->worker.dp_trace.p, 0, n_units * 16, s));
		d_trace = ctx->worker.dp_trace.as<long long>();
	}
	*gen = ++ctx->worker.dp_gen;
	hipLaunchKernelGGL(k_dp_arm, dim3(1), dim3(1), 0, s, pool, ctx->worker.dp_slot, (int)n_group, (int)(n_units - n_group), *gen, ctx->worker.dp_done, d_trace);
	HIP_TRY(hipGetLastError());
	// The workers go out on the lane's own stream (what follows the round on that stream then also waits for this launch's
	// workers to run out of units of ANY lane; measured level with a stream of their own, 19.6 against 19.7 M residues/s).
	// MPA_DP_WORKER_STREAM=1: a worker stream per lane -- one more stream per lane for HIP to deal hardware queues to, and
	// when that stream lands on a queue another context's long kernels use, every round waits for them (the evidence run of
	// round 5 measured 6.5 M residues/s that way: profiles/r05_experiments.txt).
	static const bool own_stream = [] { const char *e = getenv("MPA_DP_WORKER_STREAM"); return e && atoi(e) != 0; }();
	hipStream_t ws = own_stream ? ctx->worker.worker_stream : s;
	if (own_stream) {
		HIP_TRY(hipEventRecord(ctx->worker.arm_ev, s));
		HIP_TRY(hipStreamWaitEvent(ws, ctx->worker.arm_ev, 0));
	}
	WorkerBufs::WorkerLaunch wl;
	if (!ctx->worker.wl_free.empty()) wl = ctx->worker.wl_free.back(), ctx->worker.wl_free.pop_back();
	else { HIP_TRY(hipEventCreate(&wl.e0)); HIP_TRY(hipEventCreate(&wl.e1)); }
	HIP_TRY(ensure_dynamic_lds((const void*)k_dp_worker, ctx->device, round_lds));
	static const int launch_cap = [] { const char *e = getenv("MPA_DP_LAUNCH_WORKERS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : dp_pool_budget(); }();
	// a workgroup serves one workgroup unit at a time, or four one-wave units side by side
	const unsigned grid = (unsigned)std::min<size_t>(n_group + (n_units - n_group + 3) / 4, (size_t)launch_cap);
	HIP_TRY(hipEventRecord(wl.e0, ws));
	hipLaunchKernelGGL(k_dp_worker, dim3(grid), dim3(256), round_lds, ws, pool, ctx->worker.dp_slot, n_slots);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(wl.e1, ws));
	ctx->worker.wl_busy.push_back(wl);
	return MPA_OK;
}
// the round is complete when the last of its units has stored the round's generation into the lane's pinned word
static int pool_wait_round(mpa_ctx_t *ctx, hipStream_t s, unsigned int gen, const DpUnit *units, size_t n_units)
{
	volatile int32_t *d = ctx->worker.dp_done;
	const double t0 = now_ms();
	for (int polls = 0; (unsigned int)*d != gen; ++polls) {
		if (polls >= 8) { struct timespec ts = { 0, 100000L }; nanosleep(&ts, nullptr); }
		if ((polls & 1023) == 1023) {
			if (now_ms() - t0 > 120000.0) { set_error("DP worker pool: a round did not complete within two minutes"); return MPA_ERR_HIP; }
			const hipError_t e = hipStreamQuery(s);                            // (a fault in a worker kernel shows up here, not in the word)
			if (e != hipSuccess && e != hipErrorNotReady) { set_error(std::string("DP worker launch: ") + hipGetErrorString(e)); return MPA_ERR_HIP; }
		}
	}
	hipLaunchKernelGGL(k_l2_writeback, dim3(128), dim3(64), 0, s);       // the units' results out of the L2s, before anything enqueued behind reads them
	HIP_TRY(hipGetLastError());
	if (const char *path = dp_trace_path()) {                             // (debug) one line per unit: who ran when
		std::vector<long long> tr(2 * n_units);
		HIP_TRY(hipMemcpy(tr.data(), ctx->worker.dp_trace.p, n_units * 16, hipMemcpyDeviceToHost));
		static std::mutex tmu;
		std::lock_guard<std::mutex> g(tmu);
		if (FILE *f = fopen(path, "a")) {
			for (size_t k = 0; k < n_units; ++k)
				fprintf(f, "%d\t%u\t%zu\t%d\t%d\t%lld\t%lld\n", ctx->worker.dp_slot, gen, k, units[k].kind, units[k].prio, tr[2 * k], tr[2 * k + 1]);
			fclose(f);
		}
	}
	return MPA_OK;
}
// time during which at least one worker launch of the device was running
static double pool_union_ms(mpa_ctx_s *root, bool reset)
{
	std::lock_guard<std::mutex> g(root->worker.pool_mu);
	std::vector<std::pair<float, float>> iv = root->worker.pool_iv;
	if (reset) root->worker.pool_iv.clear();
	std::sort(iv.begin(), iv.end());
	double sum = 0, lo = 0, hi = -1;
	for (auto &x : iv) {
		if (hi < 0) { lo = x.first, hi = x.second; continue; }
		if (x.first <= hi) { hi = std::max<double>(hi, x.second); continue; }
		sum += hi - lo, lo = x.first, hi = x.second;
	}
	if (hi >= 0) sum += hi - lo;
	return sum;
}
} // namespace mpa

extern "C" {

void mpa_dp_last_stats(const mpa_ctx_t *ctx, mpa_dp_stats_t *st) { *st = ctx->stats; }
void mpa_dp_total_stats(mpa_ctx_t *ctx, mpa_dp_stats_t *st, int reset)
{
	pool_harvest(ctx, true);
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	const double u = pool_union_ms(root, reset != 0);
	if (st) *st = ctx->total, st->ms_round_union = u;
	if (reset) ctx->total = mpa_dp_stats_t();
}

#define MPA_RETRY_NO_SPLIT (-100)   /* internal: repeat the round without split extension calls */

// A round from device-resident tasks: what goes in, what the phases count, where the device's result records are.
struct Resident {
	DpResidentIn in;
	DpResidentRec rec;
	const int32_t *d_gids = nullptr;            // the sorted traceback calls where the device planner left them
	const mpa_dp_rst_t *d_rst = nullptr;
	const int64_t *d_head = nullptr;            // ... and their header
	// (MPA_GPU_ROUND1, section 4.15) round 1: in.d_tasks is null and the tasks go up with the planner's upload; the step between the rounds
	// is chained behind the results kernels (chain: what the caller staged for it; cdev: where it wants records and dense pool)
	const SpansChain *chain = nullptr;
	mpa_idx_s *chain_mi = nullptr;
	SpansChainDev cdev;
	int64_t plan_up = 0;                        // the planner's upload, for the record's parts
	const char *who() const { return chain ? "round 1 resident" : "round 2 resident"; }
};

// What the phases of one mpa_dp_run() call share: the plan, the staging blocks, the kernels' argument structs, which side streams
// carry what, and the event times collected so far.
struct DpRun {
	mpa_ctx_t *ctx;
	hipStream_t s;
	DpPlan &plan;
	DpPlanKnobs kn;
	const mpa_dp_task_t *in;                    // the caller's array (null for a resident round)
	struct Resident *rz = nullptr;              // (MPA_GPU_ROUND2) a round from device-resident tasks: results assembled on the device
	size_t dn_res = 0;                          // ... where its header and result records land in the download block
	char *hup = nullptr, *hdn = nullptr;        // pinned staging: host -> device (plan.up), device -> host (plan.dn)
	DpConst dc;
	ExtArgs ea;
	ExtWideArgs wa;
	GlobArgs ga;
	GlobWave *d_hw = nullptr;                   // the huge calls' waves and list, behind their keys
	int32_t *d_hlist = nullptr;
	struct Launch { int side; bool is_ext; };
	std::vector<Launch> launches;               // side-stream launches so far (side = index of the stream and of its event pair)
	int l12_side = -1;                          // ... the one of the T_LITE_W4 sweep
	int l13_side = -1;                          // ... and of the T_LITE_W8 sweep
	bool round_launched = false;
	bool pool_pending = false;                  // (worker pool) a round is armed and not yet known to be complete ...
	unsigned int pool_gen = 0;                  // ... its generation
	int64_t pool_n = 0;                         // words of the dense CIGAR pool
	bool mb_wg = false;                         // (MPA_DP_MB_WG, not with the worker pool) the T_MB traceback calls on k_glob_mb_wg, next to the round
	float ms_glob = 0, ms_bt = 0;
	bool glob_timed = false;                    // ev[3..5] hold a chunk's sweep and walk not yet added to ms_glob / ms_bt
	double t_mark = 0;
	void mark(const char *what) { const double t = now_ms(); timing_note(what, t - t_mark); t_mark = t; }   // (MPA_TIMING: wall clock between marks)
	hipEvent_t ev_round(int k) const { return ctx->lev[2 * (mpa_ctx_s::kSide - 1) + k]; }                    // the last event pair times the round's launch
	int side_slot(int k) const { return (k + ctx->side_off) % ctx->side_cap; }                               // (side_cap > 0) the stream plan caps a lane's side streams: launches beyond the cap share them in turn
	hipStream_t side_stream(int k) const { hipStream_t st = ctx->side_cap > 0 ? ctx->side[side_slot(k)] : nullptr; return st ? st : s; }
	void add_chunk_times() { float a = 0, b = 0; (void)hipEventElapsedTime(&a, ctx->ev[3], ctx->ev[4]); (void)hipEventElapsedTime(&b, ctx->ev[4], ctx->ev[5]); ms_glob += a, ms_bt += b; }
};

// fork: the next side stream (created when first used), waiting for fork_ev, its start event recorded
static hipStream_t begin_side(DpRun &R, bool is_ext)
{
	mpa_ctx_t *ctx = R.ctx;
	const int k = (int)R.launches.size();
	// (side streams are created when first used: HIP deals hardware queues to streams in creation order, and sixteen idle side
	// streams per context pushed the main streams of later contexts onto queues that other contexts' long kernels were using)
	// (how many a lane may have and in which priority class is the stream plan's: stream_plan.h; none: the lane's own stream)
	if (ctx->side_cap > 0) {
		hipStream_t &slot = ctx->side[R.side_slot(k)];
		if (!slot && create_stream_in_class(&slot, ctx->side_cls) != hipSuccess) { (void)hipGetLastError(); slot = nullptr; }
	}
	hipStream_t st = R.side_stream(k);
	(void)hipStreamWaitEvent(st, ctx->fork_ev, 0);
	(void)hipEventRecord(ctx->lev[2 * k], st);
	R.launches.push_back(DpRun::Launch{ k, is_ext });
	return st;
}
static void end_side(DpRun &R) { const int k = R.launches.back().side; (void)hipEventRecord(R.ctx->lev[2 * k + 1], R.side_stream(k)); }

// a resident round's results pool (ctx->round.cigoff): ResLayout, dev_layout.h
static ResLayout res_layout(size_t n, size_t n_glob) { return ResLayout(n, n_glob, (size_t)dp_blocks((int64_t)n_glob, TeamWG::W)); }
// round.list: the calls of a traceback chunk, then its GlobWave[] in the next 64-byte section (dp_tb_chunks and the device planner put
// them there); round.wlist: the calls the walk takes, then the walk's block counter
static GlobWave *round_list_waves(mpa_ctx_t *ctx, size_t n_calls) { Carve c(64); c.take<int32_t>(n_calls); return Piece<GlobWave>{ c.at, 0 }.in(ctx->round.list.p); }
static unsigned long long *round_wlist_blocks(mpa_ctx_t *ctx, size_t n_lite) { Carve c(64); c.take<int32_t>(n_lite); return Piece<unsigned long long>{ c.at, 1 }.in(ctx->round.wlist.p); }
// (the word behind it counts the blocks of k_walk_w8 alone: the pool's 128 bytes of slack hold both)

// ---- 2. pools and staging at the sizes the plan asks for
static int dp_size_pools(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	const DpPlan::Pools &z = R.plan.sz;
	int rc;
	if ((rc = ctx->round.tasks.ensure(z.tasks)) || (rc = ctx->round.chunks.ensure(z.chunks)) || (rc = ctx->round.qseq.ensure(z.qseq)) || (rc = ctx->round.rec.ensure(z.rec)) || (rc = ctx->round.prof.ensure(z.prof)) ||
	    (rc = ctx->round.waves.ensure(z.waves)) || (rc = ctx->round.extout.ensure(z.extout)) || (rc = ctx->round.tb.ensure(z.tb)) || (rc = ctx->round.cig.ensure(z.cig)) || (rc = ctx->round.ncig.ensure(z.ncig)) ||
	    (rc = ctx->round.lite.ensure(z.lite)) || (rc = ctx->round.ckpt.ensure(z.ckpt)) || (rc = ctx->round.wlist.ensure(z.wlist)) || (rc = ctx->round.score.ensure(z.score)) || (rc = ctx->round.rowkey.ensure(z.rowkey)) ||
	    (rc = ctx->round.bnd.ensure(z.bnd)) || (rc = ctx->round.hkey.ensure(z.hkey)) || (rc = ctx->round.list.ensure(z.list)))
		return rc;
	// Everything the device needs from the host goes through ONE pinned staging buffer (plan.up), so that no copy is
	// staged by the runtime and the host never waits for one: a DP round is enqueued in one go and waited for once.
	if ((rc = ctx->round.h_up.ensure(R.plan.up.end + 256))) return rc;
	R.hup = ctx->round.h_up.as<char>();
	if (R.rz) {
		// the dense pool at the plan's bound, the sum of cig_cap (its size is not known before the wait); offsets | offsets by call | block
		// sums | header | result records in one pool; the download block with room for header and records
		const ResLayout L = res_layout((size_t)R.plan.cnt.n, R.plan.glob_ids.size());
		Carve dc(64); dc.take<char>(R.plan.dn.end), R.dn_res = dc.at;        // (behind the plan's own sections, in a 64-byte section of its own)
		// (round 1: the dense pool is the spans step's sp_pool1, sized by dev_spans_chain_prepare -- round 2 overwrites cigd)
		if ((!R.rz->chain && (rc = ctx->round.cigd.ensure((size_t)R.plan.cig_total * 4 + 16))) || (rc = ctx->round.cigoff.ensure(L.end)) || (rc = ctx->round.h_down.ensure(R.dn_res + L.down_bytes()))) return rc;
	}
	return MPA_OK;
}

// ---- 3. staging filled; uploads, memsets and the prep kernels enqueued
static int dp_upload_and_prep(DpRun &R, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	char *hup = R.hup;
	const size_t b_tasks = sizeof(DTask) * P.cnt.n, b_chunks = sizeof(PrepChunk) * P.cnt.n_prep, b_waves = sizeof(ExtWave) * P.cnt.n_ewaves;
	const bool up = !P.on_device;                                         // (a plan made on the device: tasks, prep chunks and waves are in their pools)
	if (up) memcpy(hup + P.up.tasks, P.tasks.data(), b_tasks);
	if (up) memcpy(hup + P.up.chunks, P.prep.data(), b_chunks);
	memcpy(hup + P.up.q, q->seqs + q->q_off[0], (size_t)P.q_bytes);
	if (up) memcpy(hup + P.up.waves, P.ewaves.data(), b_waves);
	R.mark("    dp: buffers");
	if (up) HIP_TRY(hipMemcpyAsync(ctx->round.tasks.p, hup + P.up.tasks, b_tasks, hipMemcpyHostToDevice, s));
	if (up) HIP_TRY(hipMemcpyAsync(ctx->round.chunks.p, hup + P.up.chunks, b_chunks, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(ctx->round.qseq.p, hup + P.up.q, P.q_bytes, hipMemcpyHostToDevice, s));
	if (up && b_waves) HIP_TRY(hipMemcpyAsync(ctx->round.waves.p, hup + P.up.waves, b_waves, hipMemcpyHostToDevice, s));
	// (k_prep_rows writes every row of every call; only the padding the kernels prefetch behind the last call is cleared)
	HIP_TRY(hipMemsetAsync((char*)ctx->round.rec.p + (size_t)(P.rec_total - P.rec_pad) * 4, 0, (size_t)P.rec_pad * 4, s));
	if (P.n_wide_groups) HIP_TRY(hipMemsetAsync(ctx->round.rowkey.p, 0, (size_t)(P.n_wide_groups * 2 * P.key_stride * 4), s));
	// split classes: boundary granules, then the per-group completion counters and the error flag; all zero before the launch (a granule's tag is row + 1)
	if (P.n_split) {
		int rc;
		if ((rc = ctx->round.xg.ensure(P.sz.xg))) return rc;
		HIP_TRY(hipMemsetAsync(ctx->round.xg.p, 0, P.xg_bytes + P.xg_tail, s));
	}
	// extension calls wider than 1024 columns: keys (zeroed), then one GlobWave and one list entry per call
	if (!P.huge_ids.empty()) {
		const size_t n_huge = P.huge_ids.size();
		HIP_TRY(hipMemsetAsync(ctx->round.hkey.p, 0, (size_t)P.hkey_total * 8, s));
		Carve kc(16), tail(1);                                             // hkey: the keys in a 16-byte section | waves | list, packed
		kc.take<uint64_t>((size_t)P.hkey_total), tail.skip(kc.at);
		R.d_hw = tail.take<GlobWave>(n_huge).in(ctx->round.hkey.p), R.d_hlist = tail.take<int32_t>(n_huge).in(ctx->round.hkey.p);
		HIP_TRY(hipMemcpyAsync(R.d_hw, P.huge_waves.data(), sizeof(GlobWave) * n_huge, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(R.d_hlist, P.huge_ids.data(), 4 * n_huge, hipMemcpyHostToDevice, s));
		HIP_TRY(wait_stream(ctx, s));                  // (pageable sources; the calls are rare)
	}

	DevTables tabs;
	memcpy(tabs.aa20, tab_aa20(), 256);
	memcpy(tabs.codon, tab_codon(), 64);
	memcpy(tabs.mat, opt->mat, 484);
	DpConst &dc = R.dc;
	dc.go = opt->go, dc.ge = opt->ge, dc.fs = opt->fs, dc.xdrop = opt->xdrop, dc.end_bonus = opt->end_bonus;
	for (int k = 0; k < 6; ++k) dc.sp[k] = opt->sp[k];
	dc.sp_null_bonus = opt->sp_null_bonus;
	dc.wide_ge = P.wide_ge ? 1 : 0;
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, mi->dev[ctx->device]->spsc, mi->l_seq };

	// per-row records and profiles
	// (measured, round 4: putting these two on a high-priority stream of their own gives every DP lane a second active hardware
	// queue, and with ten more queues in use the round kernels are time-sliced: 41 -> 72 ms per launch.  They stay in the lane's
	// own queue; MPA_SHORT_KERNEL raises their wave priority instead.)
	HIP_TRY(hipEventRecord(ctx->ev[0], s));
	if (P.cnt.n_prep)
		hipLaunchKernelGGL(k_prep_rows, dim3((unsigned)P.cnt.n_prep), dim3(256), 0, s, dg, ctx->round.tasks.as<DTask>(), ctx->round.chunks.as<PrepChunk>(), ctx->round.rec.as<uint32_t>(), dc, tabs);
	hipLaunchKernelGGL(k_prep_prof, dim3((unsigned)P.cnt.n), dim3(256), 0, s, ctx->round.tasks.as<DTask>(), ctx->round.qseq.as<char>(), ctx->round.prof.as<int16_t>(), tabs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(ctx->ev[1], s));
	R.mark("    dp: uploads + prep enqueued");

	// the kernels' arguments
	ExtArgs &ea = R.ea;
	ea.tasks = ctx->round.tasks.as<DTask>(), ea.rec = ctx->round.rec.as<uint32_t>(), ea.prof = ctx->round.prof.as<int16_t>(), ea.out = ctx->round.extout.as<ExtOut>();
	ea.c = dc, ea.pen = P.pen;
	ea.lite = ctx->round.lite.as<uint32_t>(), ea.ckpt = ctx->round.ckpt.as<uint32_t>(), ea.score = ctx->round.score.as<int32_t>();
	ea.waves = ctx->round.waves.as<ExtWave>();
	ExtWideArgs &wa = R.wa;
	wa.tasks = ea.tasks, wa.rec = ea.rec, wa.prof = ea.prof, wa.out = ea.out, wa.c = dc, wa.pen = P.pen, wa.key_stride = P.key_stride;
	wa.xg = P.n_split ? ctx->round.xg.as<unsigned long long>() : nullptr;
	wa.done = P.n_split ? (int32_t*)((char*)ctx->round.xg.p + P.xg_bytes) : nullptr;
	wa.ticket = P.n_split ? wa.done + P.n_split : nullptr;
	wa.err = P.n_split ? wa.ticket + P.n_split : nullptr;
	wa.waves = ctx->round.waves.as<ExtWave>();                // absolute descriptor indices: the rowkey slot of group g is g - first wide group
	wa.rowkey = ctx->round.rowkey.as<uint32_t>() - (int64_t)P.ext[X_W2].first * 2 * P.key_stride;
	GlobArgs &ga = R.ga;
	ga.tasks = ctx->round.tasks.as<DTask>(), ga.rec = ctx->round.rec.as<uint32_t>(), ga.prof = ctx->round.prof.as<int16_t>();
	ga.tb = ctx->round.tb.as<uint16_t>(), ga.bnd = ctx->round.bnd.as<int4>(), ga.score = ctx->round.score.as<int32_t>(), ga.c = dc, ga.rowkey64 = nullptr, ga.waves = nullptr;
	return MPA_OK;
}

// ---- 4. what runs next to the round on side streams: the anti-diagonal prototype, the huge calls, the T_LITE_W4 sweep
static int dp_side_launches(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	// fork: every side launch waits for the prep kernels, so the long single-wave tails overlap instead of adding up
	HIP_TRY(hipEventRecord(ctx->fork_ev, R.s));
	if (ctx->antidiag && P.ext[X_32].cnt > 0) {                        // (measurement) the 32-column class on the anti-diagonal prototype, one wave per block
		hipStream_t st = begin_side(R, true);
		hipLaunchKernelGGL(k_ext_antidiag, dim3((unsigned)P.ext[X_32].cnt), dim3(64), EXT_ANTIDIAG_LDS, st, R.ea, P.ext[X_32].first);
		HIP_TRY(hipGetLastError());
		end_side(R);
		ctx->stats.launches_ext++;
	}
	if (!P.huge_ids.empty()) {                                         // block-major sweep with the traceback kernel's arithmetic, then the replay
		const unsigned n_huge = (unsigned)P.huge_ids.size();
		GlobArgs ha;
		ha.tasks = ctx->round.tasks.as<DTask>(), ha.waves = R.d_hw, ha.rec = ctx->round.rec.as<uint32_t>(), ha.prof = ctx->round.prof.as<int16_t>();
		ha.tb = nullptr, ha.bnd = ctx->round.bnd.as<int4>(), ha.score = nullptr, ha.c = R.dc, ha.rowkey64 = ctx->round.hkey.as<unsigned long long>();
		// MPA_DP_HUGE_WG: calls of hwg::MIN_BLOCKS column blocks or more on k_ext_huge_wg (one wave per block, no hand-off between
		// workgroups: a repeated round and the worker pool take it too); both kernels go over the same list and each returns at
		// once for the other's calls.  A kernel without a call in the list is not launched.
		int64_t *lh = ctx->last_huge;                                   // (zero: mpa_dp_run_impl)
		for (int32_t id : P.huge_ids) {
			const int32_t nblk = hwg::n_blocks(P.tasks[id].ncol);
			if (ctx->knobs.huge_wg && hwg::takes_wg(P.tasks[id].ncol)) ++lh[1], lh[2] += nblk, lh[3] += hwg::n_pass(nblk);
			else ++lh[0];
		}
		if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: huge calls: %lld on one wave, %lld on workgroups (%lld blocks, %lld passes)\n", (long long)lh[0], (long long)lh[1], (long long)lh[2], (long long)lh[3]);
		const int32_t wg_min = ctx->knobs.huge_wg ? hwg::MIN_BLOCKS : 0;
		hipStream_t st = begin_side(R, true);
		if (lh[0]) {
			if (P.wide_ge) hipLaunchKernelGGL(k_ext_huge<true>, dim3(n_huge), dim3(64), GLOB_NARROW_LDS, st, ha, wg_min);
			else hipLaunchKernelGGL(k_ext_huge<false>, dim3(n_huge), dim3(64), GLOB_NARROW_LDS, st, ha, wg_min);
			HIP_TRY(hipGetLastError());
		}
		if (lh[1]) {
			if (P.wide_ge) hipLaunchKernelGGL(k_ext_huge_wg<true>, dim3(n_huge), dim3(hwg::W * 64), 0, st, ha);
			else hipLaunchKernelGGL(k_ext_huge_wg<false>, dim3(n_huge), dim3(hwg::W * 64), 0, st, ha);
			HIP_TRY(hipGetLastError());
		}
		hipLaunchKernelGGL(k_ext_replay, dim3(n_huge), dim3(64), 0, st, ctx->round.tasks.as<DTask>(), R.d_hlist, (int32_t)n_huge,
		                   ctx->round.hkey.as<unsigned long long>(), ctx->round.extout.as<ExtOut>(), R.dc, P.pen);
		HIP_TRY(hipGetLastError());
		end_side(R);
		ctx->stats.launches_ext++;
	}
	// the packed sweep of the 129..256-column checkpointed class (unit kind U_LITE_W4): a 256-thread launch of its own next to the
	// round, on a side stream (at most two are taken at this point, by the launches above); the walk waits for it
	if (P.lite_w4.cnt > 0) {
		hipStream_t st = begin_side(R, false);
		hipLaunchKernelGGL(k_lite_wide, dim3((unsigned)P.lite_w4.cnt), dim3(MPA_LITE_WIDE_WAVES * 64), 0, st, R.ea, P.lite_w4.first);
		HIP_TRY(hipGetLastError());
		end_side(R), R.l12_side = R.launches.back().side;
		ctx->stats.launches_glob++;
	}
	// ... and of the 257..512-column checkpointed class (U_LITE_W8): a 512-thread launch on a side stream of its own, next to k_lite_wide
	if (P.lite_w8.cnt > 0) {
		hipStream_t st = begin_side(R, false);
		hipLaunchKernelGGL(k_lite_w8, dim3((unsigned)P.lite_w8.cnt), dim3(MPA_LITE_W8_WAVES * 64), 0, st, R.ea, P.lite_w8.first);
		HIP_TRY(hipGetLastError());
		end_side(R), R.l13_side = R.launches.back().side;
		ctx->stats.launches_glob++;
		ctx->last_w8[2] += P.lite_w8.cnt;
	}
	return MPA_OK;
}

// Workgroups of the round kernel per CU, enforced through the LDS it asks for (MPA_DP_WG_PER_CU, default 3).  Round 6: the
// kernel takes 124 VGPRs (the asm rows of ext_narrow keep the whole DP state of eight calls in registers and nothing is
// spilled), so three workgroups hold 372 of each SIMD's 512 registers -- what four workgroups of the 95-register kernel of
// rounds 4-5 held (384) -- and the seeding kernels of the next batches stay co-resident.  One more workgroup than wanted must
// NOT fit; what is left of the LDS stays free for the seeding kernels.
static size_t dp_round_lds()
{
	static const size_t round_lds = [] {
		const char *e = getenv("MPA_DP_WG_PER_CU");
		int want = e ? atoi(e) : 3;
		if (want < 1) want = 1;
		if (want > 4) want = 4;
		const size_t pad = (((size_t)160 * 1024 / (want + 1)) + 256) & ~(size_t)255;
		return pad > DP_ROUND_LDS ? pad : DP_ROUND_LDS;
	}();
	return round_lds;
}

// every DP unit of the round (dp_plan_units, built straight into the staging block) in ONE k_dp_round launch on the context's main stream -- or handed to the worker pool;
// d_gw: the first traceback chunk's waves when they ride in the round
static int dp_launch_round(DpRun &R, GlobWave *d_gw)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	DpUnit *units = (DpUnit*)(R.hup + P.up.units);          // (pinned: the copy below needs no wait)
	int rc;
	if (!P.on_device && (rc = dp_plan_units(P, R.kn, units))) { set_error(P.err); return rc; }   // (on the device: the list is in ctx->round.units, its length in the plan)
	const size_t n_units = P.n_units;
	if (n_units == 0) return MPA_OK;
	static const bool show_top = [] { const char *e = getenv("MPA_DP_TOP"); return e && atoi(e) != 0; }();
	if (show_top && !P.on_device) fputs(dp_plan_top(P, R.kn).c_str(), stderr);
	if ((rc = ctx->round.units.ensure(P.sz.units))) return rc;
	if (!P.on_device) HIP_TRY(hipMemcpyAsync(ctx->round.units.p, units, P.sz.units, hipMemcpyHostToDevice, s));
	R.ga.waves = d_gw;
	const size_t round_lds = dp_round_lds();
	if (dp_pool_enabled()) {
		if ((rc = pool_launch_round(ctx, s, R.ea, R.wa, R.ga, (DpRoundArgs*)(R.hup + P.up.args), n_units, P.n_group, round_lds, &R.pool_gen))) return rc;
		R.pool_pending = true;
	} else {
		if (round_lds > 48 * 1024) HIP_TRY(ensure_dynamic_lds((const void*)k_dp_round, ctx->device, round_lds));
		HIP_TRY(hipEventRecord(R.ev_round(0), s));
		hipLaunchKernelGGL(k_dp_round, dim3((unsigned)n_units), dim3(256), round_lds, s, R.ea, R.wa, R.ga, ctx->round.units.as<DpUnit>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(R.ev_round(1), s));
	}
	R.round_launched = true;
	ctx->stats.launches_ext++;
	return MPA_OK;
}

// launch, then (worker pool) wait until the round's units are done
static int dp_round(DpRun &R, GlobWave *d_gw, const char *what)
{
	int rc;
	if ((rc = dp_launch_round(R, d_gw)) != MPA_OK) return rc;
	R.mark(what);
	if (R.pool_pending) {
		if ((rc = pool_wait_round(R.ctx, R.s, R.pool_gen, (const DpUnit*)(R.hup + R.plan.up.units), R.plan.n_units)) != MPA_OK) return rc;
		R.pool_pending = false;
	}
	if (dp_pool_enabled()) R.mark("    dp: round (units done)");
	return MPA_OK;
}

// one stand-alone launch of a chunk's plain traceback sweep: T_16, T_32, T_64 and T_MB share one ("narrow", cls < 0), every wide class has its own
// (MPA_DP_MB_WG: T_MB leaves the narrow launch and, cls == T_MB, has k_glob_mb_wg over the tail of the chunk's call list d_list)
static hipError_t launch_glob_class(DpRun &R, const DpTbChunk &r, GlobWave *d_gw, const int32_t *d_list, int cls, hipStream_t st)
{
	GlobArgs &ga = R.ga;
	const bool wide_ge = R.plan.wide_ge;
	if (cls == T_MB) {
		const unsigned n_mb = (unsigned)r.cls[T_MB].cnt;
		const int32_t *mbl = d_list + (r.n_list - n_mb);
		if (wide_ge) hipLaunchKernelGGL(k_glob_mb_wg<true>, dim3(n_mb), dim3(hwg::W * 64), 0, st, ga, mbl);
		else hipLaunchKernelGGL(k_glob_mb_wg<false>, dim3(n_mb), dim3(hwg::W * 64), 0, st, ga, mbl);
		return hipGetLastError();
	}
	if (cls < 0) {
		int first[8], cnt[8];
		for (int c = 0; c < 8; ++c) first[c] = r.cls[c].first, cnt[c] = r.cls[c].cnt;
		if (R.mb_wg) cnt[T_MB] = 0;                                        // (k_glob_mb_wg's, above)
		ga.waves = d_gw;
		return launch_glob_narrow(ga, first, cnt, st, wide_ge);
	}
	ga.waves = d_gw + r.cls[cls].first;
	switch (cls) {
	case T_W2: return launch_glob_wide<2>(ga, r.cls[cls].cnt, st, wide_ge);
	case T_W4: return launch_glob_wide<4>(ga, r.cls[cls].cnt, st, wide_ge);
	case T_W8: return launch_glob_wide<8>(ga, r.cls[cls].cnt, st, wide_ge);
	default: return launch_glob_wide<16>(ga, r.cls[cls].cnt, st, wide_ge);
	}
}

// ---- 5. the chunks of the plain traceback sweep, each followed by k_backtrack; the round's launch rides with the first
static int dp_tb_chunks(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	char *hup = R.hup;
	int rc;
	for (size_t ri = 0; ri < P.chunks.size(); ++ri) {
		if (!P.on_device) dp_plan_chunk_waves(P, ri);
		const DpTbChunk &r = P.chunks[ri];
		if (ri > 0) {                                                    // later chunks reuse the traceback buffer (and its staging): join everything first
			for (auto &l : R.launches) (void)hipStreamWaitEvent(s, ctx->lev[2 * l.side + 1], 0);
			HIP_TRY(wait_stream(ctx, s));
			R.add_chunk_times();                                           // (the previous chunk's sweep and walk)
		}
		int32_t *d_list = ctx->round.list.as<int32_t>();
		GlobWave *d_gw = round_list_waves(ctx, P.cnt.n);
		const bool in_round = ri == 0 && P.round_has_glob;
		// the chunk's T_MB calls: one per wave, the last class of the chunk's waves and so the tail of its call list.  MPA_DP_MB_WG: they are
		// k_glob_mb_wg's (a device plan with such a call was declined: dev_dp_plan)
		const int n_mb = r.cls[T_MB].cnt, n_mb_wg = R.mb_wg ? n_mb : 0;
		ctx->last_mb[0] += n_mb - n_mb_wg, ctx->last_mb[1] += n_mb_wg;
		for (int k = 0; k < n_mb_wg; ++k) {
			const int32_t nblk = hwg::n_blocks(P.tasks[r.list[r.n_list - n_mb_wg + k]].ncol);
			ctx->last_mb[2] += nblk, ctx->last_mb[3] += hwg::n_pass(nblk);
		}
		if (!P.on_device) {
			memcpy(hup + P.up.list, r.list.data(), r.n_list * 4);
			memcpy(hup + P.up.gw, r.waves.data(), r.n_waves * sizeof(GlobWave));
			// in the round their U_GLOB_MB units stay (the plan and k_dp_round are what they are without the knob) and find no call:
			// glob_narrow returns at once for an empty wave of no rows, having written nothing
			if (in_round)
				for (int k = 0; k < n_mb_wg; ++k) { GlobWave &g = ((GlobWave*)(hup + P.up.gw))[r.cls[T_MB].first + k]; g.task[0] = -1, g.max_nl = 0; }
			HIP_TRY(hipMemcpyAsync(d_list, hup + P.up.list, r.n_list * 4, hipMemcpyHostToDevice, s));
			HIP_TRY(hipMemcpyAsync(d_gw, hup + P.up.gw, r.n_waves * sizeof(GlobWave), hipMemcpyHostToDevice, s));
		}
		R.mark("    dp: traceback lists enqueued");
		R.ga.tb = ctx->round.tb.as<uint16_t>();
		HIP_TRY(hipEventRecord(ctx->ev[3], s));
		// every launch on its own stream (next to the extension classes in the first chunk); the walk needs them all
		HIP_TRY(hipEventRecord(ctx->fork_ev, s));
		const size_t first_glob_launch = R.launches.size();
		const int order[6] = { T_MB, T_W16, T_W8, T_W4, T_W2, -1 };      // (T_MB: k_glob_mb_wg over the chunk's T_MB calls, the longest of these launches)
		for (int cls : order) {
			if (in_round && cls < T_W8) continue;                            // (only the 512/1024-thread traceback classes and k_glob_mb_wg keep their own launch)
			const int cnt = cls == T_MB ? n_mb_wg : cls >= 0 ? r.cls[cls].cnt : r.cls[T_16].cnt + r.cls[T_32].cnt + r.cls[T_64].cnt + n_mb - n_mb_wg;
			if (!cnt) continue;
			if ((int)R.launches.size() >= mpa_ctx_s::kSide - 1) {            // out of side streams (the last event pair times the round's launch): main stream
				HIP_TRY(launch_glob_class(R, r, d_gw, d_list, cls, s));
			} else {
				hipStream_t st = begin_side(R, false);
				HIP_TRY(launch_glob_class(R, r, d_gw, d_list, cls, st));
				end_side(R);
			}
			ctx->stats.launches_glob++;
		}
		if (in_round) {                                        // (behind the 512/1024-thread classes' own launches: with the worker pool the host waits here)
			ctx->stats.launches_glob++;
			if ((rc = dp_round(R, d_gw, "    dp: units up, round launched")) != MPA_OK) return rc;
		}
		for (size_t k = first_glob_launch; k < R.launches.size(); ++k) (void)hipStreamWaitEvent(s, ctx->lev[2 * R.launches[k].side + 1], 0);
		HIP_TRY(hipEventRecord(ctx->ev[4], s));
		hipLaunchKernelGGL(k_backtrack, dim3((unsigned)r.n_list), dim3(64), 0, s, ctx->round.tasks.as<DTask>(), d_list, (int32_t)r.n_list,
		                   ctx->round.tb.as<uint16_t>(), ctx->round.cig.as<uint32_t>(), ctx->round.ncig.as<int32_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(ctx->ev[5], s));
		R.glob_timed = true;                                              // (ev[3..5] are read after the next wait)
	}
	if (!R.round_launched && (rc = dp_round(R, nullptr, "    dp: (round without traceback launched)")) != MPA_OK) return rc;
	const int64_t *lm = ctx->last_mb;                                   // (zero: mpa_dp_run_impl)
	if (timing_on() && lm[0] + lm[1] > 0)
		fprintf(stderr, "[mpa-timing]   dp: block-major traceback calls: %lld on one wave, %lld on workgroups (%lld blocks, %lld passes)\n", (long long)lm[0], (long long)lm[1], (long long)lm[2], (long long)lm[3]);
	return MPA_OK;
}

// ---- 6. the walk of the checkpointed traceback: behind the round that swept its calls
static int dp_walk(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	if (!P.n_lite) return MPA_OK;
	if (!P.on_device) {
		memcpy(R.hup + P.up.wl, P.glob_ids.data() + P.n_reg_glob, 4 * P.n_lite);
		HIP_TRY(hipMemcpyAsync(ctx->round.wlist.p, R.hup + P.up.wl, 4 * P.n_lite, hipMemcpyHostToDevice, s));
	}
	WalkArgs wk;
	wk.ga = R.ga, wk.ga.waves = nullptr, wk.list = ctx->round.wlist.as<int32_t>(), wk.n_list = (int32_t)P.n_lite;
	wk.lite = ctx->round.lite.as<uint32_t>(), wk.ckpt = ctx->round.ckpt.as<uint32_t>(), wk.cig = ctx->round.cig.as<uint32_t>(), wk.n_cigar = ctx->round.ncig.as<int32_t>();
	wk.n_blocks = round_wlist_blocks(ctx, P.n_lite);
	HIP_TRY(hipMemsetAsync(wk.n_blocks, 0, 16, s));                     // (and the word of k_walk_w8's blocks behind it)
	// (the list is sorted by class: one launch per class, with the LDS that class's block of direction words needs)
	size_t at = 0;
	for (int cls = T_LITE16; cls <= T_LITE_W4; ++cls) {
		const size_t n_c = (size_t)P.walk_cnt[cls - T_LITE16];
		if (n_c == 0) continue;
		wk.list = ctx->round.wlist.as<int32_t>() + at, wk.n_list = (int32_t)n_c;
		if (cls == T_LITE_W4) {                                            // behind their own sweep; more LDS than a launch gets unasked
			if (R.l12_side >= 0) (void)hipStreamWaitEvent(s, ctx->lev[2 * R.l12_side + 1], 0);
			HIP_TRY(ensure_dynamic_lds((const void*)k_walk, ctx->device, WALK_LDS(256)));
		}
		hipLaunchKernelGGL(k_walk, dim3((unsigned)n_c), dim3(64), WALK_LDS(lite_columns(cls)), s, wk);
		at += n_c;
	}
	if (P.walk_cnt_w8 > 0) {                                             // the sixth list: T_LITE_W8, behind its own sweep, on a kernel of its own
		HIP_TRY(hipGetLastError());
		wk.list = ctx->round.wlist.as<int32_t>() + at, wk.n_list = P.walk_cnt_w8, wk.n_blocks += 1;
		if (R.l13_side >= 0) (void)hipStreamWaitEvent(s, ctx->lev[2 * R.l13_side + 1], 0);
		HIP_TRY(ensure_dynamic_lds((const void*)k_walk_w8, ctx->device, WALK_LDS(lite_columns(T_LITE_W8))));
		hipLaunchKernelGGL(k_walk_w8, dim3((unsigned)P.walk_cnt_w8), dim3(64), WALK_LDS(lite_columns(T_LITE_W8)), s, wk);
	}
	HIP_TRY(hipGetLastError());
	ctx->stats.launches_glob++;
	return MPA_OK;
}

// ---- 6'. (a resident round) behind the round's last kernel and in front of its one wait: the dense pool's offsets scanned over the sorted
// traceback calls, every call's result record, the CIGARs gathered from the device's own offsets, header and records into the download
// block.  The dense pool stays in ctx->round.cigd.
static int dp_results_enqueue(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	const size_t n = P.cnt.n, n_glob = P.glob_ids.size();
	const ResLayout L = res_layout(n, n_glob);
	static_assert(DPR_NHEAD * 8 <= 64, "the header has 64 bytes of the pool");
	char *X = ctx->round.cigoff.as<char>();
	DpResDev D;
	D.n = (int64_t)n, D.n_glob = (int64_t)n_glob, D.tasks = ctx->round.tasks.as<DTask>(), D.gids = R.rz->d_gids;
	D.eo = ctx->round.extout.as<ExtOut>(), D.sc = ctx->round.score.as<int32_t>(), D.nc = ctx->round.ncig.as<int32_t>();
	D.off = L.off.in(X), D.call_off = L.call_off.in(X), D.bsum = L.bsum.in(X), D.head = L.head.in(X), D.rst = L.rst.in(X);
	HIP_TRY(hipMemsetAsync(D.head, 0, L.head.bytes(), s));
	const dim3 wg(TeamWG::W), g_glob((unsigned)dp_blocks((int64_t)n_glob, TeamWG::W)), g_calls((unsigned)dp_blocks((int64_t)n, TeamWG::W));
	if (n_glob) {
		hipLaunchKernelGGL(k_dpr_sums, g_glob, wg, 0, s, D);
		hipLaunchKernelGGL(k_dpr_mid, dim3(1), wg, 0, s, D);
		hipLaunchKernelGGL(k_dpr_offsets, g_glob, wg, 0, s, D);
	}
	hipLaunchKernelGGL(k_dpr_records, g_calls, wg, 0, s, D);
	// (round 1, section 4.15: the words go straight into the spans step's pool, which outlives round 2, and the records into the rst1 section
	// of its block, where k_spans reads them now and k_assemble behind round 2)
	uint32_t *dense = R.rz->chain ? R.rz->cdev.d_pool1 : ctx->round.cigd.as<uint32_t>();
	if (n_glob) hipLaunchKernelGGL(k_cigar_gather, dim3((unsigned)n_glob), dim3(64), 0, s, ctx->round.tasks.as<DTask>(), D.gids, D.off, (int32_t)n_glob,
	                               ctx->round.ncig.as<int32_t>(), ctx->round.cig.as<uint32_t>(), dense);
	HIP_TRY(hipGetLastError());
	if (R.rz->chain) HIP_TRY(hipMemcpyAsync(R.rz->cdev.d_rst1, D.rst, sizeof(mpa_dp_rst_t) * n, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(R.hdn + R.dn_res, L.head.in(X), L.down_bytes(), hipMemcpyDeviceToHost, s));
	R.rz->d_rst = D.rst, R.rz->d_head = D.head, R.rz->rec.bytes_down += (int64_t)L.down_bytes();
	return MPA_OK;
}

// ---- 7. join the side streams; results into pinned memory behind the last kernel (extension outputs, traceback scores and
// CIGAR lengths, hand-off error flag, the walk's block count); the one wait of the round; kernel times
static int dp_join_and_download(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	const size_t n = P.cnt.n;
	for (auto &l : R.launches) (void)hipStreamWaitEvent(s, ctx->lev[2 * l.side + 1], 0);
	HIP_TRY(hipEventRecord(ctx->ev[2], s));
	int rc;
	if ((rc = ctx->round.h_down.ensure(P.dn.end))) return rc;
	char *hdn = R.hdn = ctx->round.h_down.as<char>();
	*(int32_t*)(hdn + P.dn.err) = 0;
	if (R.rz) { if ((rc = dp_results_enqueue(R))) return rc; }           // (resident: the records come down instead of what they are made from)
	else if (P.cnt.n_ext) HIP_TRY(hipMemcpyAsync(hdn + P.dn.eo, ctx->round.extout.p, sizeof(ExtOut) * n, hipMemcpyDeviceToHost, s));
	if (P.cnt.n_glob && !R.rz) {
		HIP_TRY(hipMemcpyAsync(hdn + P.dn.sc, ctx->round.score.p, n * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(hdn + P.dn.nc, ctx->round.ncig.p, n * 4, hipMemcpyDeviceToHost, s));
	}
	if (P.n_split) HIP_TRY(hipMemcpyAsync(hdn + P.dn.err, R.wa.err, 4, hipMemcpyDeviceToHost, s));
	((unsigned long long*)(hdn + P.dn.wb))[0] = 0, ((unsigned long long*)(hdn + P.dn.wb))[1] = 0;
	if (R.rz) R.rz->rec.bytes_down += (P.n_split ? 4 : 0) + (P.n_lite ? 8 : 0);
	if (P.n_lite) HIP_TRY(hipMemcpyAsync(hdn + P.dn.wb, round_wlist_blocks(ctx, P.n_lite), P.walk_cnt_w8 > 0 ? 16 : 8, hipMemcpyDeviceToHost, s));
	// (MPA_GPU_ROUND1, section 4.15) the step between the rounds, by its own unit's enqueue function: its kernels read the records in place
	// and are guarded by the words the host checks behind the wait -- a hand-off that timed out, a call outside its slot
	if (R.rz && R.rz->chain) {
		int64_t down = 0;
		if ((rc = dev_spans_chain_enqueue(ctx, R.rz->chain_mi, *R.rz->chain, P.n_split ? R.wa.err : nullptr, R.rz->d_head + DPR_H_BAD, &R.rz->rec.chained_launches, &down))) return rc;
		R.rz->rec.bytes_down += down;
	}
	R.mark("    dp: round enqueued");
	HIP_TRY(wait_stream(ctx, s));
	R.mark("    dp: round (wait)");
	if (R.glob_timed) R.add_chunk_times();
	float ms_ext_sum = 0;                                                 // sum of the per-launch durations of the extension kernels
	if (R.round_launched && !dp_pool_enabled()) {
		(void)hipEventElapsedTime(&ms_ext_sum, R.ev_round(0), R.ev_round(1));
		ctx->stats.ms_round = ms_ext_sum, ctx->stats.launches_round = 1;
	}
	if (dp_pool_enabled()) pool_harvest(ctx, false);                    // (worker launches that have ended: into the context's totals)
	for (auto &l : R.launches) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ctx->lev[2 * l.side], ctx->lev[2 * l.side + 1]);
		if (l.is_ext) ms_ext_sum += ms;
		else if (l.side == R.l12_side || l.side == R.l13_side) R.ms_glob += ms;   // (the 129..256- and 257..512-column packed sweeps: traceback sweeps like the chunks')
	}
	ctx->stats.ms_ext = ms_ext_sum;
	return MPA_OK;
}

// ---- 8. the real CIGARs gathered into a dense pool on the device (the slots were sized for the worst case, nl+al+4 words each:
// only that goes over PCIe); the caller's result records
static int dp_assemble(DpRun &R, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	const size_t n_glob = P.glob_ids.size();
	const ExtOut *eo = (const ExtOut*)(R.hdn + P.dn.eo);
	const int32_t *sc = (const int32_t*)(R.hdn + P.dn.sc), *nc = (const int32_t*)(R.hdn + P.dn.nc);
	int64_t &pool_n = R.pool_n;
	int64_t *dense_off = (int64_t*)(R.hup + P.up.off);                    // (the staging buffer's earlier sections have been consumed)
	for (size_t g = 0; g < n_glob; ++g) dense_off[g] = pool_n, pool_n += nc[P.glob_ids[g]];
	uint32_t *pool = (uint32_t*)malloc((size_t)(pool_n > 0 ? pool_n : 1) * 4);
	if (pool_n > 0) {
		int rc;
		Carve oc(1);                                                       // cigoff, packed: every call's offset into the dense pool | the calls
		const auto c_off = oc.take<int64_t>(n_glob); const auto c_ids = oc.take<int32_t>(n_glob);
		if ((rc = ctx->round.cigd.ensure((size_t)pool_n * 4)) || (rc = ctx->round.cigoff.ensure(oc.at + 64)) || (rc = ctx->round.h_pool.ensure((size_t)pool_n * 4))) { free(pool); return rc; }
		int64_t *d_off = c_off.in(ctx->round.cigoff.p); int32_t *d_ids = c_ids.in(ctx->round.cigoff.p);
		memcpy(R.hup + P.up.ids, P.glob_ids.data(), n_glob * 4);
		HIP_TRY(hipMemcpyAsync(d_off, dense_off, n_glob * 8, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(d_ids, R.hup + P.up.ids, n_glob * 4, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(k_cigar_gather, dim3((unsigned)n_glob), dim3(64), 0, s, ctx->round.tasks.as<DTask>(), d_ids, d_off, (int32_t)n_glob,
		                   ctx->round.ncig.as<int32_t>(), ctx->round.cig.as<uint32_t>(), ctx->round.cigd.as<uint32_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(ctx->round.h_pool.p, ctx->round.cigd.p, (size_t)pool_n * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		memcpy(pool, ctx->round.h_pool.p, (size_t)pool_n * 4);
	}
	std::vector<int64_t> off_of(P.cnt.n, 0);
	for (size_t k = 0; k < n_glob; ++k) off_of[P.glob_ids[k]] = dense_off[k];
	for (size_t k = 0; k < P.cnt.n; ++k) {
		const mpa_dp_task_t &t = R.in[k];                                  // (mode and shape: the caller's own record; the rule: dp_results_core.h)
		rst[k] = dp_result_of(t.flag, t.nl, t.al, (int64_t)k, eo, sc, nc, off_of[k]);
	}
	if (cigar_pool) *cigar_pool = pool; else free(pool);
	if (n_pool) *n_pool = pool_n;
	return MPA_OK;
}

// ---- 9. statistics: the plan's counts, cells and bytes, the event times, the context's totals
static void dp_statistics(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	mpa_dp_stats_t &st = ctx->stats;
	if (!R.plan.on_device) dp_plan_stats(R.plan);                        // (on the device: sums of the classify stage, in the plan already)
	const mpa_dp_stats_t &ps = R.plan.stats;
	st.n_ext = ps.n_ext, st.n_glob = ps.n_glob, st.cells_ext = ps.cells_ext, st.cells_glob = ps.cells_glob, st.rows_prep = ps.rows_prep;
	st.alg_bytes_ext = ps.alg_bytes_ext, st.alg_bytes_glob = ps.alg_bytes_glob + 4 * R.pool_n;   // (+ the CIGARs' own words)
	st.n_ckpt = ps.n_ckpt, st.cells_ckpt = ps.cells_ckpt, st.n_ckpt_wide = ps.n_ckpt_wide, st.cells_ckpt_wide = ps.cells_ckpt_wide;
	st.cells_ext_round = ps.cells_ext_round, st.cells_glob_round = ps.cells_glob_round;
	// (k_walk's blocks and, counted apart for mpa_dbg_dp_last_w8, k_walk_w8's)
	ctx->last_w8[3] = (int64_t)((const unsigned long long*)(R.hdn + R.plan.dn.wb))[1];
	st.walk_blocks = (int64_t)((const unsigned long long*)(R.hdn + R.plan.dn.wb))[0] + ctx->last_w8[3];
	float ms = 0;
	(void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); st.ms_prep = ms;
	st.ms_glob = R.ms_glob, st.ms_backtrack = R.ms_bt;
	timing_note("    dp: GPU prep kernels", st.ms_prep);
	timing_note("    dp: GPU round kernel", st.ms_round);
	timing_note("    dp: GPU walk", R.ms_bt);
	{ float w = 0; (void)hipEventElapsedTime(&w, ctx->ev[0], ctx->ev[2]); st.ms_total = w; }   // wall time of the whole batch on the device
	mpa_dp_stats_t &t = ctx->total;
	t.n_ext += st.n_ext, t.n_glob += st.n_glob, t.cells_ext += st.cells_ext, t.cells_glob += st.cells_glob, t.rows_prep += st.rows_prep;
	t.alg_bytes_ext += st.alg_bytes_ext, t.alg_bytes_glob += st.alg_bytes_glob;
	t.n_ckpt += st.n_ckpt, t.cells_ckpt += st.cells_ckpt, t.walk_blocks += st.walk_blocks;
	t.n_ckpt_wide += st.n_ckpt_wide, t.cells_ckpt_wide += st.cells_ckpt_wide;
	t.ms_prep += st.ms_prep, t.ms_ext += st.ms_ext, t.ms_glob += st.ms_glob, t.ms_backtrack += st.ms_backtrack, t.ms_total += st.ms_total;
	t.launches_ext += st.launches_ext, t.launches_glob += st.launches_glob;
	t.cells_ext_round += st.cells_ext_round, t.cells_glob_round += st.cells_glob_round, t.ms_round += st.ms_round, t.launches_round += st.launches_round;
}

// MPA_DP_MB_WG as the executor applies it: off with the worker pool, like MPA_DP_LITE_WIDE, MPA_DP_LITE_W8 and MPA_DP_SPLIT_WIDE
static bool dp_mb_wg(const mpa_ctx_t *ctx) { return ctx->knobs.mb_wg && !dp_pool_enabled(); }

// the executor's knobs as the planner takes them (the environment: read when the context was created, or once per process)
static DpPlanKnobs dp_plan_knobs(const mpa_ctx_t *ctx)
{
	static const bool ext_dual = [] { const char *e = getenv("MPA_DP_EXT_DUAL"); return !e || atoi(e) != 0; }();
	static const bool unit_prio = [] { const char *e = getenv("MPA_DP_PRIO"); return !e || atoi(e) != 0; }();   // (MPA_DP_PRIO=0: measurement)
	DpPlanKnobs kn;
	kn.lite_min = ctx->knobs.lite_min, kn.lite_wide = ctx->knobs.lite_wide, kn.no_split = ctx->no_split, kn.antidiag = ctx->antidiag, kn.pool = dp_pool_enabled();
	kn.split_wide = ctx->knobs.split_wide && !kn.pool && !kn.no_split;
	kn.lite_w8 = ctx->knobs.lite_w8 && !kn.pool;
	kn.ext_dual = ext_dual, kn.unit_prio = unit_prio, kn.tb_budget = (int64_t)ctx->knobs.tb_budget;
	return kn;
}

// ---- 1'. the plan of the round made on the device (MPA_GPU_DPPLAN=1)
// Pools the planner writes are sized before its result is known, from n and one pass over the caller's array; one upload (raw tasks |
// query offsets | contig lengths when the caller has them on the host only), the stages of dp_plan_core.h around two radix sorts, one
// download (header | sorted traceback calls), one wait.  d_ctg_len: the resident index's contig lengths, or nullptr: h_ctg_len go up.
// MPA_OK: *head and *gids point into the context's pinned block, tasks / chunks / waves / list (calls, then GlobWave[] at the
// executor's offset) / units / wlist hold the plan.  MPA_ERR_UNSUPPORTED: declined (the last error says why), nothing the host planner
// needs was touched.
static int dev_dp_plan_run(mpa_ctx_t *ctx, hipStream_t s, const int64_t *d_ctg_len, const int64_t *h_ctg_len, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt,
                           const DpPlanKnobs &kn, int64_t n, const mpa_dp_task_t *in, const DpDevHead **head, const int32_t **gids, size_t *bytes_up, size_t *bytes_down,
                           Resident *rz = nullptr)
{
	if (const char *why = dp_plan_device_declines(opt, kn, n)) { set_error(std::string("device DP plan: ") + why); return MPA_ERR_UNSUPPORTED; }
	if (q->n_seq < 0 || n_ctg < 0) { set_error("device DP plan: no queries or contigs"); return MPA_ERR_UNSUPPORTED; }
	const size_t N = (size_t)n, U = (size_t)dp_units_bound(n, kn.split_wide != 0), nb = (size_t)dp_blocks(n, TeamWG::W);
	// what goes up, in one block (rz: the tasks are read where they are -- no task bytes are staged or uploaded; a resident round 1 has
	// them on the host, and they go up here as with MPA_GPU_DPPLAN=1)
	const bool tasks_up = !rz || !rz->in.d_tasks;
	Carve up;
	const auto u_raw = up.take_if<mpa_dp_task_t>(tasks_up, N); const auto u_qoff = up.take<int64_t>((size_t)q->n_seq + 1), u_ctg = up.take_if<int64_t>(!d_ctg_len, (size_t)n_ctg);
	const size_t up_end = up.at;
	tl_alloc_failed = false;
	auto declined_alloc = [](int rc) { if (tl_alloc_failed) { tl_alloc_failed = false; return (int)MPA_ERR_UNSUPPORTED; } return rc; };
	int rc;
	if ((rc = ctx->planner.h_dpp_up.ensure(up_end + 256))) return MPA_ERR_UNSUPPORTED;
	char *hup = ctx->planner.h_dpp_up.as<char>();
	if (tasks_up) memcpy(u_raw.in(hup), in, u_raw.bytes());
	int64_t max_nl = tasks_up ? 0 : rz->in.max_nl, max_al = tasks_up ? 0 : rz->in.max_al;
	const int64_t prep_bound = tasks_up ? dp_plan_prep_bound(u_raw.in((const char*)hup), n, &max_nl, &max_al) : rz->in.prep_bound;
	if (prep_bound < 0 || prep_bound > (int64_t)N << 21) { set_error("device DP plan: impossible bounds of the task list"); return MPA_ERR_UNSUPPORTED; }
	if (!dp_unit_costs_fit(max_nl, max_al)) { set_error("device DP plan: unit costs that do not fit the sort key"); return MPA_ERR_UNSUPPORTED; }
	memcpy(u_qoff.in(hup), q->q_off, u_qoff.bytes());
	if (!d_ctg_len && n_ctg > 0) memcpy(u_ctg.in(hup), h_ctg_len, u_ctg.bytes());
	// scratch: the upload block, keys, block sums, units, header | sorted traceback calls (one download), the sorts' own
	size_t tmp_calls = 0, tmp_units = 0;
	HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_calls, (uint64_t*)nullptr, (uint64_t*)nullptr, N, 0u, (unsigned)MPA_DPPLAN_KEY_BITS, s));
	HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_units, (uint64_t*)nullptr, (uint64_t*)nullptr, U, 0u, 64u, s));
	Carve carve;
	const auto x_up = carve.take<char>(up_end); const auto x_key = carve.take<uint64_t>(N), x_skey = carve.take<uint64_t>(N); const auto x_bsum = carve.take<DpSums>(nb); const auto x_ubuf = carve.take<DpUnit>(U);
	const auto x_ukey = carve.take<uint64_t>(U), x_uskey = carve.take<uint64_t>(U); const auto x_head = carve.take<DpDevHead>(1); const auto x_gids = carve.take<int32_t>(N); const auto x_tmp = carve.take<char>(std::max(tmp_calls, tmp_units), 16);
	const Piece<int32_t> h_gids{ x_gids.off - x_head.off, N };          // header | sorted traceback calls: one download, the header at 0
	const size_t down_bytes = h_gids.end();
	// the executor's pools at their bounds (size_buffers() asks for no more once the plan is known: nothing the planner wrote moves)
	if ((rc = ctx->planner.dpp.ensure(carve.at)) || (rc = ctx->round.tasks.ensure(sizeof(DTask) * N)) || (rc = ctx->round.chunks.ensure(sizeof(PrepChunk) * ((size_t)prep_bound + 1))) ||
	    (rc = ctx->round.waves.ensure(sizeof(ExtWave) * (N + 16))) || (rc = ctx->round.list.ensure(N * 4 + 128 + sizeof(GlobWave) * (N + 1))) ||
	    (rc = ctx->round.units.ensure(sizeof(DpUnit) * U)) || (rc = ctx->round.wlist.ensure(N * 4 + 128)))
		return declined_alloc(rc);
	if ((rc = ctx->planner.h_dpp_down.ensure(down_bytes + 256))) return MPA_ERR_UNSUPPORTED;
	char *X = ctx->planner.dpp.as<char>();
	DpDevPlan D;
	D.n = n, D.n_ubound = (int64_t)U, D.n_ctg = n_ctg, D.n_seq = q->n_seq, D.opt = dp_plan_opt(opt), D.kn = kn;
	const char *dup = x_up.in(X);
	D.raw = tasks_up ? u_raw.in(dup) : rz->in.d_tasks, D.q_off = u_qoff.in(dup), D.ctg_len = d_ctg_len ? d_ctg_len : u_ctg.in(dup);
	D.tasks = ctx->round.tasks.as<DTask>(), D.chunks = ctx->round.chunks.as<PrepChunk>(), D.waves = ctx->round.waves.as<ExtWave>(), D.list = ctx->round.list.as<int32_t>();
	D.gw = round_list_waves(ctx, N);
	D.units = ctx->round.units.as<DpUnit>(), D.wlist = ctx->round.wlist.as<int32_t>();
	D.key = x_key.in(X), D.skey = x_skey.in(X), D.bsum = x_bsum.in(X), D.ubuf = x_ubuf.in(X);
	D.ukey = x_ukey.in(X), D.uskey = x_uskey.in(X), D.head = x_head.in(X), D.gids = x_gids.in(X);
	HIP_TRY(hipMemcpyAsync(x_up.in(X), hup, up_end, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(D.head, 0, sizeof(DpDevHead), s));
	const dim3 g_calls((unsigned)nb), g_units((unsigned)dp_blocks((int64_t)U, TeamWG::W)), wg(TeamWG::W);
	hipLaunchKernelGGL(k_dpp_classify, g_calls, wg, 0, s, D);
	HIP_TRY(rocprim::radix_sort_keys(x_tmp.in(X), tmp_calls, D.key, D.skey, N, 0u, (unsigned)MPA_DPPLAN_KEY_BITS, s));
	hipLaunchKernelGGL(k_dpp_sums, g_calls, wg, 0, s, D);
	hipLaunchKernelGGL(k_dpp_mid, dim3(1), wg, 0, s, D);
	hipLaunchKernelGGL(k_dpp_layout, g_calls, wg, 0, s, D);
	hipLaunchKernelGGL(k_dpp_units, g_units, wg, 0, s, D);
	HIP_TRY(rocprim::radix_sort_keys(x_tmp.in(X), tmp_units, D.ukey, D.uskey, U, 0u, 64u, s));
	hipLaunchKernelGGL(k_dpp_units_out, g_units, wg, 0, s, D);
	HIP_TRY(hipGetLastError());
	char *hdn = ctx->planner.h_dpp_down.as<char>();
	HIP_TRY(hipMemcpyAsync(hdn, x_head.in(X), down_bytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	*head = (const DpDevHead*)hdn, *gids = h_gids.in((const char*)hdn);
	*bytes_up = up_end, *bytes_down = down_bytes;
	if (rz) rz->d_gids = D.gids, rz->rec.task_bytes_up = (int64_t)(u_qoff.off - u_raw.off);
	return MPA_OK;
}

// the round's plan from the device planner: MPA_OK (plan.on_device), MPA_ERR_UNSUPPORTED when it declines, else an error
static int dev_dp_plan(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, const DpPlanKnobs &kn, int64_t n, const mpa_dp_task_t *in, DpPlan &plan,
                       size_t *bytes_up, size_t *bytes_down, Resident *rz = nullptr)
{
	const DpDevHead *head = nullptr;
	const int32_t *gids = nullptr;
	int rc = dev_dp_plan_run(ctx, ctx->stream, mi->dev[ctx->device]->ctg_len, nullptr, (int32_t)mi->ctg.size(), q, opt, kn, n, in, &head, &gids, bytes_up, bytes_down, rz);
	if (rc != MPA_OK) return rc;
	if ((rc = dp_plan_from_head(*head, gids, q, opt, kn, sizeof(DpRoundArgs), plan))) set_error("device DP plan: " + plan.err);
	// MPA_DP_MB_WG: k_glob_mb_wg's calls leave the round through the host's copy of the chunk's descriptors, which a device plan does not have
	else if (dp_mb_wg(ctx) && !plan.chunks.empty() && plan.chunks[0].cls[T_MB].cnt > 0) {
		plan = DpPlan();
		set_error("device DP plan: a block-major traceback call (T_MB) with MPA_DP_MB_WG");
		rc = MPA_ERR_UNSUPPORTED;
	}
	return rc;
}
// MPA_GPU_DPPLAN, read per call
static bool dp_plan_on_device() { const char *e = getenv("MPA_GPU_DPPLAN"); return e && atoi(e) != 0; }

static int mpa_dp_run_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q,
               int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool, Resident *rz = nullptr)
{
	if (cigar_pool) *cigar_pool = nullptr;
	if (n_pool) *n_pool = 0;
	if (!ctx) { set_error("no device context"); return MPA_ERR_NO_DEVICE; }
	if (ctx->device >= mpa_idx_s::kMaxDevices || !mi->dev[ctx->device]) { set_error("index is not resident on this context's device (call mpa_idx_to_device)"); return MPA_ERR_ARG; }
	ctx->stats = mpa_dp_stats_t();
	if (n <= 0) return MPA_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	const double t_begin = now_ms();
	int rc;
	// 1. plan
	DpPlan plan;
	DpPlanKnobs kn = dp_plan_knobs(ctx);
	bool planned = false;
	const int64_t waits0 = ctx->n_waits;
	if (rz) {                                                   // (MPA_GPU_ROUND2=1) planned from the tasks in place, or not run here at all
		size_t b_up = 0, b_down = 0;
		tl_alloc_failed = false;
		if ((rc = dev_dp_plan(ctx, mi, opt, q, kn, n, in, plan, &b_up, &b_down, rz)) != MPA_OK) return rc;   // (in: null for round 2, whose tasks are in place)
		planned = true;
		rz->rec.plan_waits = ctx->n_waits - waits0, rz->rec.bytes_up = (int64_t)b_up, rz->rec.bytes_down = (int64_t)b_down, rz->plan_up = (int64_t)b_up;
		timing_note("  dp: plan on device", now_ms() - t_begin);
		if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: plan on device: %zu bytes up, %zu bytes down\n", b_up, b_down);
	} else if (dp_plan_on_device()) {                                  // (MPA_GPU_DPPLAN=1) the planner's stages on the device; declined: the host planner, as without the knob
		size_t b_up = 0, b_down = 0;
		rc = dev_dp_plan(ctx, mi, opt, q, kn, n, in, plan, &b_up, &b_down);
		if (rc == MPA_OK) {
			planned = true;
			timing_note("  dp: plan on device", now_ms() - t_begin);
			if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: plan on device: %zu bytes up, %zu bytes down\n", b_up, b_down);
		} else if (rc != MPA_ERR_UNSUPPORTED) return rc;
		else if (timing_on()) fprintf(stderr, "[mpa-timing]   device DP plan declined (%s): planned on the host\n", mpa_last_error());
	}
	if (!planned) {
		if ((rc = dp_plan(in, n, mi->ctg.empty() ? nullptr : &mi->ctg[0].len, sizeof(mi->ctg[0]), (int32_t)mi->ctg.size(), q, opt, kn, sizeof(DpRoundArgs), plan))) { set_error(plan.err); return rc; }
		timing_note("  dp: classify/sort/layout", now_ms() - t_begin);
	}
	// X_SPLIT8 / X_SPLIT12 groups need 7 / 11 boundaries of key_stride granules each: a granule pool that cannot grow that far declines
	// them -- the round is planned again with those calls on k_ext_huge (same results), before anything of it is enqueued
	if (kn.split_wide && plan.ext_wide[0].cnt + plan.ext_wide[1].cnt > 0) {
		tl_alloc_failed = false;
		if (ctx->round.xg.ensure(plan.sz.xg)) {
			tl_alloc_failed = false;
			if (rz) { set_error(std::string(rz->who()) + ": the boundary pool of the 2048/3072-column extension classes cannot grow"); return MPA_ERR_UNSUPPORTED; }
			if (timing_on()) fprintf(stderr, "[mpa-timing]   2048/3072-column extension classes declined (%zu bytes of boundary granules): those calls on the one-wave int32 sweep\n", plan.sz.xg);
			kn.split_wide = 0;
			if ((rc = dp_plan(in, n, mi->ctg.empty() ? nullptr : &mi->ctg[0].len, sizeof(mi->ctg[0]), (int32_t)mi->ctg.size(), q, opt, kn, sizeof(DpRoundArgs), plan))) { set_error(plan.err); return rc; }
		}
	}
	memcpy(ctx->last_ext_calls, plan.ext_calls, sizeof(ctx->last_ext_calls));
	memset(ctx->last_huge, 0, sizeof(ctx->last_huge));
	memset(ctx->last_mb, 0, sizeof(ctx->last_mb));
	memset(ctx->last_w8, 0, sizeof(ctx->last_w8));
	for (size_t k = plan.n_reg_glob; k < plan.glob_ids.size() && !plan.on_device; ++k) {      // (a plan made on the device holds no call of the class)
		const DTask &t = plan.tasks[plan.glob_ids[k]];
		if (t.cls == T_LITE_W8) ++ctx->last_w8[0], ctx->last_w8[1] += (int64_t)(t.nl > 2 ? t.nl - 2 : 0) * t.ncol;
	}
	if (timing_on() && ctx->last_w8[0] > 0)
		fprintf(stderr, "[mpa-timing]   dp: %lld traceback calls of 257..512 columns checkpointed, in %d eight-wave groups\n", (long long)ctx->last_w8[0], plan.lite_w8.cnt);
	if (timing_on() && plan.ext_wide[0].cnt + plan.ext_wide[1].cnt > 0)
		fprintf(stderr, "[mpa-timing]   dp: %d + %d groups of the 2048- / 3072-column extension classes (8 / 12 workgroups each), %lld boundaries\n", plan.ext_wide[0].cnt, plan.ext_wide[1].cnt, (long long)plan.n_bound);
	DpRun R{ ctx, ctx->stream, plan, kn, in };
	R.t_mark = now_ms();
	R.rz = rz;
	R.mb_wg = dp_mb_wg(ctx) && !plan.on_device;                 // (a device plan with a T_MB call was declined under the knob: dev_dp_plan)
	const int64_t waits1 = ctx->n_waits;
	rc = dp_size_pools(R);                                      // 2. pools and staging
	if (rc && rz) { tl_alloc_failed = false; return MPA_ERR_UNSUPPORTED; }   // (resident: a pool or pinned block that cannot grow declines, before anything of the round is launched)
	if (rz) rz->rec.bytes_up += plan.q_bytes;                   // (the queries' residues: the round's only upload)
	// (MPA_GPU_ROUND1, section 4.15) the step between the rounds staged before round 1 is launched: its block up without the record section,
	// its pools sized -- sp_pool1 at the plan's bound of the dense pool, whose real size is not known before the wait
	if (!rc && rz && rz->chain) {
		tl_alloc_failed = false;
		if ((rc = dev_spans_chain_prepare(ctx, rz->chain_mi, *rz->chain, plan.cig_total, rz->cdev)) != MPA_OK) { tl_alloc_failed = false; return rc; }
		rz->rec.bytes_up += rz->cdev.bytes_up;
	}
	if (rc ||
	    (rc = dp_upload_and_prep(R, mi, opt, q)) ||            // 3. uploads, memsets, prep
	    (rc = dp_side_launches(R)) ||                          // 4. next to the round: anti-diagonal, huge, T_LITE_W4 sweep
	    (rc = dp_tb_chunks(R)) ||                              // 5. traceback chunks with the round's launch
	    (rc = dp_walk(R)) ||                                   // 6. walk
	    (rc = dp_join_and_download(R)))                        // 7. join, download, the one wait
		return rc;
	// a boundary hand-off that never arrived (bounded spin in the kernel): the producer workgroup was running (it drew its
	// ticket first) but made no progress for seconds -- a stalled hardware queue under oversubscription.  Nothing of this round
	// has been handed to the caller yet: mpa_dp_run() repeats it with those calls on the one-wave path (k_ext_huge, same bits).
	static const bool test_fail = [] { const char *e = getenv("MPA_TEST_HANDOFF_FAIL"); return e && atoi(e) != 0; }();
	if (*(const int32_t*)(R.hdn + plan.dn.err) || (test_fail && plan.n_split && !ctx->no_split)) {
		if (rz) { set_error(std::string(rz->who()) + ": a column-block hand-off timed out, the round is repeated by mpa_dp_run"); return MPA_ERR_UNSUPPORTED; }
		set_error("k_ext_wide_split: a column-block hand-off between workgroups timed out"); return MPA_RETRY_NO_SPLIT;
	}
	timing_note("  dp: upload+kernels (wall)", now_ms() - t_begin);
	const double t_res = now_ms();
	if (rz) {                                                   // 8'. the records are down already; the dense pool stays on the device
		const int64_t *head = (const int64_t*)(R.hdn + R.dn_res);
		if (head[DPR_H_BAD] || head[DPR_H_POOL] < 0 || head[DPR_H_POOL] > plan.cig_total) { set_error(std::string(rz->who()) + ": a traceback call's CIGAR length is outside its slot"); return MPA_ERR_HIP; }
		R.pool_n = head[DPR_H_POOL];
		memcpy(rst, R.hdn + R.dn_res + 64, sizeof(mpa_dp_rst_t) * (size_t)n);
		if (n_pool) *n_pool = R.pool_n;
		rz->rec.round_waits = ctx->n_waits - waits1;
		if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: %s: %lld up, %lld down, %lld wait\n", rz->who(), (long long)rz->rec.bytes_up, (long long)rz->rec.bytes_down, (long long)rz->rec.round_waits);
	} else if ((rc = dp_assemble(R, rst, cigar_pool, n_pool))) return rc;   // 8. CIGAR gather, results
	timing_note("  dp: download+assemble", now_ms() - t_res);
	dp_statistics(R);                                           // 9.
	return MPA_OK;
}

int mpa_dp_run(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q,
               int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] {
		int rc = mpa_dp_run_impl(ctx, mi, opt, q, n, in, rst, cigar_pool, n_pool);
		if (rc == MPA_RETRY_NO_SPLIT) {
			ctx->no_split = true, ++ctx->handoff_retries;
			rc = mpa_dp_run_impl(ctx, mi, opt, q, n, in, rst, cigar_pool, n_pool);
			ctx->no_split = false;
			if (rc == MPA_RETRY_NO_SPLIT) rc = MPA_ERR_HIP;
		}
		return rc;
	});
}

} // extern "C"

namespace mpa {
int dp_run_resident(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const DpResidentIn &in, mpa_dp_rst_t *rst, int64_t *n_pool,
                    const mpa_dp_rst_t **d_rst, DpResidentRec *rec)
{
	if (!in.d_tasks || n <= 0) { set_error("round 2 resident: no tasks on the device"); return MPA_ERR_UNSUPPORTED; }
	Resident rz;
	rz.in = in;
	const int rc = mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_dp_run_impl(ctx, mi, opt, q, n, nullptr, rst, nullptr, n_pool, &rz); });
	if (d_rst) *d_rst = rc == MPA_OK ? rz.d_rst : nullptr;
	if (rec) *rec = rz.rec;
	return rc;
}
// n_pool words of a dense pool of the context (src: cigd, or the spans step's sp_pool1) into a malloc'ed block, in a wait of its own
static int dp_fetch_pool_from(mpa_ctx_t *ctx, const CtxPool &src, int64_t n_pool, uint32_t **pool)
{
	*pool = nullptr;
	if (n_pool < 0 || (size_t)n_pool * 4 > src.cap) { set_error("dp_fetch_pool: no dense CIGAR pool of that size on this context"); return MPA_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	uint32_t *p = (uint32_t*)malloc((size_t)(n_pool > 0 ? n_pool : 1) * 4);
	if (!p) { set_error("out of host memory"); return MPA_ERR_HIP; }
	if (n_pool > 0) {
		int rc;
		if ((rc = ctx->round.h_pool.ensure((size_t)n_pool * 4))) { free(p); return rc; }
		if (hipMemcpyAsync(ctx->round.h_pool.p, src.p, (size_t)n_pool * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || wait_stream(ctx, ctx->stream) != hipSuccess) {
			free(p), set_error("dp_fetch_pool: the download failed"); return MPA_ERR_HIP;
		}
		memcpy(p, ctx->round.h_pool.p, (size_t)n_pool * 4);
	}
	*pool = p;
	return MPA_OK;
}
int dp_fetch_pool(mpa_ctx_t *ctx, int64_t n_pool, uint32_t **pool) { return dp_fetch_pool_from(ctx, ctx->round.cigd, n_pool, pool); }
int dp_fetch_pool1(mpa_ctx_t *ctx, int64_t n_pool, uint32_t **pool) { return dp_fetch_pool_from(ctx, ctx->spans.sp_pool1, n_pool, pool); }

// (MPA_GPU_ROUND1=1) round 1 from the caller's table with the step between the rounds chained into its submission
int dp_run_round1_chained(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *tasks, const SpansChain &c,
                          mpa_dp_rst_t *rst, int64_t *n_pool, SpansIO &io, DpResidentRec *rec, int64_t *parts)
{
	if (n_pool) *n_pool = 0;
	if (!ctx || !tasks || n <= 0 || c.n_rst1 != n) { set_error("round 1 resident: no context, no tasks, or a staged block of another size"); return MPA_ERR_UNSUPPORTED; }
	Resident rz;
	rz.chain = &c, rz.chain_mi = const_cast<mpa_idx_s*>(mi);
	int64_t words = 0;
	int rc = mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_dp_run_impl(ctx, mi, opt, q, n, tasks, rst, nullptr, &words, &rz); });
	if (rc == MPA_OK) rc = dev_spans_chain_collect(ctx, c, words, io);    // (behind the round's wait and its checks: nothing is enqueued)
	if (n_pool && rc == MPA_OK) *n_pool = words;
	if (rec) *rec = rz.rec;
	if (parts) parts[0] = rz.plan_up, parts[1] = q->q_off[q->n_seq] - q->q_off[0], parts[2] = rz.cdev.bytes_up, parts[3] = rz.cdev.rst1_bytes;
	return rc;
}
} // namespace mpa

extern "C" {

int64_t mpa_dp_handoff_retries(const mpa_ctx_t *ctx) { return ctx ? ctx->handoff_retries : 0; }
void mpa_dbg_antidiag(mpa_ctx_t *ctx, int on) { if (ctx) ctx->antidiag = on != 0; }
int64_t mpa_dbg_dp_plan(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                        const int64_t *knobs, void *buf, int64_t cap)
{
	return mpa::guarded<int64_t>(MPA_ERR_HIP, [&]() -> int64_t {
		DpPlanKnobs kn;
		kn.lite_min = (int32_t)knobs[0], kn.lite_wide = (int32_t)knobs[1], kn.no_split = (int32_t)knobs[2], kn.antidiag = (int32_t)knobs[3], kn.pool = (int32_t)knobs[4];
		kn.ext_dual = (int32_t)knobs[5], kn.unit_prio = (int32_t)knobs[6], kn.tb_budget = knobs[7];
		const mpa_qbatch_t q{ n_seq, nullptr, q_off };
		DpPlan plan;
		int64_t r = dp_plan(tasks, n, ctg_len, sizeof(int64_t), n_ctg, &q, opt, kn, sizeof(DpRoundArgs), plan);
		if (r == MPA_OK) r = dp_plan_serialize(plan, kn, buf, cap);
		if (r < 0) set_error(plan.err);
		return r;
	});
}

} // extern "C"

namespace mpa {
size_t dp_round_args_bytes() { return sizeof(DpRoundArgs); }
void dp_last_ext_calls(const mpa_ctx_t *ctx, int64_t ext_calls[16]) { memcpy(ext_calls, ctx->last_ext_calls, sizeof(ctx->last_ext_calls)); }
void dp_last_huge(const mpa_ctx_t *ctx, int64_t out[4]) { memcpy(out, ctx->last_huge, sizeof(ctx->last_huge)); }
void dp_last_mb(const mpa_ctx_t *ctx, int64_t out[4]) { memcpy(out, ctx->last_mb, sizeof(ctx->last_mb)); }
void dp_last_w8(const mpa_ctx_t *ctx, int64_t out[4]) { memcpy(out, ctx->last_w8, sizeof(ctx->last_w8)); }
// mpa_dbg_dp_plan_device on a context (dpplan_dbg.cpp): the device planner on a task table, then every section it left in the pools
// downloaded into a plan's vectors and serialised as mpa_dbg_dp_plan does.  1: declined (the last error says why).
int64_t dev_dp_plan_dbg(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *in,
                        const DpPlanKnobs &kn, void *buf, int64_t cap, bool wide)
{
	HIP_TRY(hipSetDevice(ctx->device));
	const DpDevHead *head = nullptr;
	const int32_t *gids = nullptr;
	size_t b_up = 0, b_down = 0;
	int rc = dev_dp_plan_run(ctx, ctx->stream, nullptr, ctg_len, n_ctg, q, opt, kn, n, in, &head, &gids, &b_up, &b_down);
	if (rc == MPA_ERR_UNSUPPORTED) return 1;
	if (rc != MPA_OK) return rc;
	DpPlan P;
	if ((rc = dp_plan_from_head(*head, gids, q, opt, kn, sizeof(DpRoundArgs), P))) { set_error("device DP plan: " + P.err); return rc == MPA_ERR_UNSUPPORTED ? 1 : rc; }
	const DpDevHead H = *head;
	std::vector<DpUnit> units((size_t)H.n_units);
	std::vector<int32_t> wl((size_t)H.n_lite);
	P.tasks.resize((size_t)H.n), P.prep.resize((size_t)H.n_prep), P.ewaves.resize((size_t)H.n_ewaves);
	auto down = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
	HIP_TRY(down(P.tasks.data(), ctx->round.tasks.p, sizeof(DTask) * P.tasks.size()));
	HIP_TRY(down(P.prep.data(), ctx->round.chunks.p, sizeof(PrepChunk) * P.prep.size()));
	HIP_TRY(down(P.ewaves.data(), ctx->round.waves.p, sizeof(ExtWave) * P.ewaves.size()));
	HIP_TRY(down(units.data(), ctx->round.units.p, sizeof(DpUnit) * units.size()));
	HIP_TRY(down(wl.data(), ctx->round.wlist.p, 4 * wl.size()));
	if (!P.chunks.empty()) {
		DpTbChunk &r = P.chunks[0];
		r.list.resize(r.n_list), r.waves.resize(r.n_waves);
		HIP_TRY(down(r.list.data(), ctx->round.list.p, 4 * r.n_list));
		HIP_TRY(down(r.waves.data(), round_list_waves(ctx, (size_t)H.n), sizeof(GlobWave) * r.n_waves));
		for (size_t k = 0; k < r.n_list; ++k) if (r.list[k] != P.glob_ids[k]) { set_error("device DP plan: the chunk's call list is not the sorted order"); return MPA_ERR_HIP; }
	}
	for (size_t k = 0; k < wl.size(); ++k) if (wl[k] != P.glob_ids[P.n_reg_glob + k]) { set_error("device DP plan: the walk list is not the sorted order"); return MPA_ERR_HIP; }
	return dp_plan_write(P, units, buf, cap, wide);
}
// mpa_dbg_dp_run_resident on a context (round2_dbg.cpp): the tasks into a device pool, their bounds reduced there, the resident round, then
// the explicit fetch of the dense pool.  rec: the hook's int64 record (mpamd_dbg.h).  1: declined (the last error says why).
int dev_dp_run_resident_dbg(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst,
                            uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec)
{
	HIP_TRY(hipSetDevice(ctx->device));
	int rc;
	if ((rc = ctx->spans.sp_out.ensure(sizeof(mpa_dp_task_t) * (size_t)n + 64))) return rc;
	HIP_TRY(hipMemcpy(ctx->spans.sp_out.p, in, sizeof(mpa_dp_task_t) * (size_t)n, hipMemcpyHostToDevice));
	DpResidentIn ri;
	if ((rc = dev_task_bounds(ctx, ctx->spans.sp_out.as<mpa_dp_task_t>(), n, ri))) return rc;
	rec[7] = ri.prep_bound, rec[8] = ri.max_nl, rec[9] = ri.max_al;
	DpResidentRec rr;
	int64_t words = 0;
	rc = dp_run_resident(ctx, mi, opt, q, n, ri, rst, &words, nullptr, &rr);
	rec[0] = rr.plan_waits, rec[1] = rr.round_waits, rec[2] = rr.bytes_up, rec[3] = rr.task_bytes_up, rec[4] = rr.bytes_down, rec[5] = rr.pool_bytes_down;
	if (rc == MPA_ERR_UNSUPPORTED) return 1;
	if (rc != MPA_OK) return rc;
	if ((rc = dp_fetch_pool(ctx, words, cigar_pool))) return rc;
	rec[6] = 4 * words, rec[10] = words;
	if (n_pool) *n_pool = words;
	return MPA_OK;
}
} // namespace mpa

#include "gs32_exec.hip"
