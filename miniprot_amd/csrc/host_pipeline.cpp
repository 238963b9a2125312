// host_pipeline.cpp -- the stream: several mini-batches in flight on one device (mpa_map_batches, mpa_map_batches_claim) and one job
// over the devices of a process (mpa_map_batches_multi).  Who may start which batch when is host_pipeline.h, which knows nothing of
// the device; this file makes the device contexts and gives the scheduler its stage bodies.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include "host_batch.h"
#include "stream_plan.h"
#pragma GCC visibility push(hidden)   // (the scheduler is internal to the library: the dynamic symbol table does not grow)
#include "host_pipeline.h"
#pragma GCC visibility pop

using namespace mpa;

// MPA_TRACE=1: one line per pipeline event of mpa_map_batches() with a time stamp (ms since the call began) -- tools/gantt.py
// turns them into a per-stage timeline
static double g_trace_t0 = 0;
static bool trace_on() { static int on = -1; if (on < 0) { const char *e = getenv("MPA_TRACE"); on = e && *e && *e != '0'; } return on != 0; }
static void trace(const char *stage, int32_t batch, const char *what)
{
	if (trace_on()) fprintf(stderr, "[mpa-trace] %10.3f %-8s batch %3d %s\n", now_ms() - g_trace_t0, stage, batch, what);
}

// wall-clock microseconds and calls of the stream pipeline's stages since the last reset (mpa_stage_clocks): 0 seeding, 1 planning,
// 2 DP rounds of a batch (all of them, host round trips included), 3 output (flatten + text), 4 sketch (host half of seeding)
static std::atomic<int64_t> g_stage_us[5], g_stage_n[5];
namespace mpa {
struct StageClock {
	int k; double t0;
	explicit StageClock(int k_) : k(k_), t0(now_ms()) {}
	~StageClock() { g_stage_us[k] += (int64_t)((now_ms() - t0) * 1000.0), ++g_stage_n[k]; }
};
} // namespace mpa

// MPA_DP_LANES, MPA_PLANNERS, MPA_SEEDERS (read per call)
static int stream_knob(const char *name, int dflt, int lo, int hi)
{
	int v = dflt;
	if (const char *e = getenv(name)) v = atoi(e);
	return std::max(lo, std::min(v, hi));
}

extern "C" {

// Several mini-batches as a software pipeline: [sketch of batch k+2] | [seeding of batch k+1] | [planning] | [DP rounds of batch k on
// the GPU] | [flatten + format batch k-1].  Each stage thread drives its own worker-pool lane.
// claim != nullptr: the job's batches are handed out by the caller -- claim(user) returns the index (into batches[]) of the next
// batch this call should map, or -1 when the job has none left -- so that several callers (one process per GPU) can share one
// job and each takes work as fast as it gets through it (the kt_for work stealing of map.c:264-271, between processes).
// results / text / text_len are then in CLAIM order, order[j] says which batch slot j holds, *n_mapped how many there are.
static int mpa_map_batches_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, int32_t n_batches, const mpa_qbatch_t *batches,
                    const char *const *const *names, int n_threads, mpa_result_t **results, int64_t *id_io, char **text, int64_t *text_len,
                    mpa_claim_fn claim = nullptr, void *claim_user = nullptr, int32_t *n_mapped = nullptr, int32_t *order = nullptr, int pipe = 0)
{
	const int lane0 = 24 * (pipe & 7);                    // worker-pool lanes of this pipeline (several pipelines of one process: one per device)
	for (int32_t k = 0; k < n_batches; ++k) { results[k] = nullptr; if (text) text[k] = nullptr; if (text_len) text_len[k] = 0; }
	if (!ctx) { set_error("mpa_map_batches needs a device context: the DP has no CPU fallback"); return MPA_ERR_NO_DEVICE; }
	if (names && (!text || !text_len || !id_io)) { set_error("mpa_map_batches: names given without text/text_len/id_io"); return MPA_ERR_ARG; }
	g_trace_t0 = now_ms();
	struct Work { mpa_batch_t *b = nullptr; mpa_qbatch_t q{}; };   // slot k of the scheduler: the batch's state and its queries
	std::vector<Work> work((size_t)n_batches);
	if (n_mapped) *n_mapped = 0;
	// DP lanes = batches in their DP rounds at the same time.  A round is one k_dp_round launch (one hardware queue), so four
	// lanes fit next to the seeding streams; measured at config 3 (20 000 proteins in 10 batches, two planners, two seeders):
	// 3 lanes 0.91 s, 4 lanes 0.865 s; with one planner and one seeder the host stages bound the stream (1.00 s, any lane count)
	// round 3 (both chaining rounds on the device, sleeping waits: the host stages no longer bound the stream): 5 lanes 93.5 ms per
	// 4 000-protein step, 4 lanes 99.8, 6 lanes 100-112 (config 3, 20 steps)
	const int n_lanes = stream_knob("MPA_DP_LANES", 5, 1, 8);
	const int n_plan = stream_knob("MPA_PLANNERS", 4, 1, 6), n_seed = stream_knob("MPA_SEEDERS", 3, 1, 4);   // (what they are: below)
	// The streams of all these contexts share the process's hardware queues (GPU_MAX_HW_QUEUES per priority class): which context's
	// stream is created when and in which class is stream_plan.h.  MPA_STREAM_PLAN=0 (and the legacy layout's own knobs MPA_PRIO_MAIN,
	// MPA_PRIO_SEED): every context a normal main stream, seeders and planners a high one on top, sixteen side streams per lane.
	{
		const int layout = getenv("MPA_PRIO_MAIN") || getenv("MPA_PRIO_SEED") ? (int)SL_LEGACY : stream_layout_of(getenv("MPA_STREAM_PLAN"));
		if (const int rc = ctx_apply_stream_plan(ctx, n_lanes, n_seed, n_plan, layout)) return rc;
	}
	std::vector<mpa_ctx_t*> lane_ctx((size_t)n_lanes, ctx);
	for (int d = 1; d < n_lanes; ++d) if (!(lane_ctx[d] = ctx_sibling(ctx, d))) return MPA_ERR_HIP;
	for (int d = 0; d < n_lanes; ++d) ctx_set_role(ctx, lane_ctx[d], 0);
	// HIP maps streams to its hardware queues by creation order; with 17 streams per context the first side streams of the
	// third context land on the queues of the second one's (measured, rocprofv3 queue ids), three further on they do not
	if (n_lanes > 2) ctx_set_side_offset(lane_ctx[2], 3);
	// Planners: the planning stage (pre-chain extraction, chaining, refinement, plans) is memory-bound host work that gains
	// nothing from more than ~32 threads, so two batches are planned side by side with half the threads each
	// (MPA_PLANNERS, default 2).  The seeder's own streams and buffers, one set per batch that can be between seeding and
	// the end of planning: the result of batch k is consumed while batches k+1 .. are on the device.
	// (round 3: with the whole refinement on the device a planner mostly waits for it -- three of them, a third of the threads each)
	// (round 5, once the contexts' idle side streams no longer took hardware queues away: four planners and three seeders, +5 %)
	// Seeders: the device-seeding stage of a batch is mostly waiting for its kernels, which share the GPU with the DP rounds in
	// flight; two batches are seeded side by side (MPA_SEEDERS, default 2)
	// Depth of the pipeline.  A seeding context is busy from the start of a batch's seeding to the end of its planning, and a
	// planned batch waits for a DP lane: seeding of batch k waits for the plan of batch k - n_seed_ctx, the plan of batch k for
	// the end of the DP of batch k - (lanes + planners).  Deeper coupling was measured to change nothing (rounds 2-3).
	// Device contexts (streams + pools): one per seeder and one per planner.  What a seeded batch leaves for its planner is pinned
	// host memory only (SeedHold): n_seed_ctx holders, one per batch that can be between the start of seeding and the end of planning.
	const int n_seed_ctx = n_plan + n_seed;
	std::vector<mpa_ctx_t*> seed_dev((size_t)n_seed, nullptr), plan_dev((size_t)n_plan, nullptr);
	for (int k = 0; k < n_seed; ++k) if (!(seed_dev[k] = ctx_sibling(ctx, n_lanes + k))) return MPA_ERR_HIP;
	for (int k = 0; k < n_plan; ++k) if (!(plan_dev[k] = ctx_sibling(ctx, n_lanes + n_seed + k))) return MPA_ERR_HIP;
	for (int k = 0; k < n_seed; ++k) ctx_set_role(ctx, seed_dev[k], 1);
	for (int k = 0; k < n_plan; ++k) ctx_set_role(ctx, plan_dev[k], 2);
	std::vector<SeedHold*> hold((size_t)n_seed_ctx, nullptr);
	for (int k = 0; k < n_seed_ctx; ++k) hold[k] = ctx_seed_hold(ctx, k);
	static const char *const kSeedName[4] = { "seed0", "seed1", "seed2", "seed3" };
	static const char *const kPlanName[6] = { "plan0", "plan1", "plan2", "plan3", "plan4", "plan5" };
	static const char *const kLaneName[8] = { "dp0", "dp1", "dp2", "dp3", "dp4", "dp5", "dp6", "dp7" };

	StreamStages st;
	int32_t next_own = 0;                                 // (without a claim function) the next batch
	st.claim = [&]() -> int32_t { return claim ? claim(claim_user) : (next_own < n_batches ? next_own++ : -1); };
	st.last_error = [] { return std::string(mpa_last_error()); };
	// every stage thread: its own worker pool, a share of the threads (stages with light host work take a fraction), its CPU time under a label
	st.thread = [&](StreamStage s, int i, const std::function<void()> &loop) {
		static const char *const kPool[5] = { "sketch: worker pool", "seeding: worker pool", "planning: worker pool", "DP lanes: worker pool", "output: worker pool" };
		static const char *const kSpan[5] = { "sketch: stage thread", "seeding: stage thread (waits for the device)", "planning: stage thread (serial parts + waits)",
			"DP lanes: lane thread (round bookkeeping + waits)", "output: stage thread (flatten + format)" };
		const int lane[5] = { 20, 10 + i, 14 + i, 2 + i, 1 };
		pool_stage_enter(lane0 + lane[s], s == STREAM_PLAN ? n_plan : 4, kPool[s]);
		{ CpuSpan cs(kSpan[s]); loop(); }
		pool_stage_leave();                                // (lane 0 of the DP stage is the caller's thread)
	};
	// Sketch: the host half of seeding (protein sketch, bucket lookup, occurrence cut-off, seed jobs: ~27 ms per 4 000 proteins), so
	// that the seeders' stage is device work only -- it was the stage that bounded the stream (141 ms of wall per batch on two
	// seeders, round 4)
	st.sketch = [&](int32_t k, int32_t g) {
		work[k].q = batches[g];
		trace("sketch", k, "begin");
		{ StageClock sc(4); work[k].b = batch_sketch_phase(true, mi, opt, &work[k].q, n_threads); }
		if (work[k].b && names && format_knob() == 1) work[k].b->fmt_names = names[g];   // (MPA_GPU_FORMAT=1: the DP lane's last call writes the text)
		trace("sketch", k, "end");
		return work[k].b ? MPA_OK : MPA_ERR_ARG;
	};
	st.seed = [&](int sd, int32_t k, int h) {
		trace(kSeedName[sd], k, "begin");
		bool ok;
		double sketch_ms = 0;
		{ StageClock sc(0); ok = batch_device_seed_phase(seed_dev[sd], work[k].b, true, hold[h], &sketch_ms, true); }
		// (clock [4] is the sketch stage wherever it ran: with MPA_GPU_SKETCH its time inside this phase moves over from clock [0])
		if (sketch_ms > 0) g_stage_us[4] += (int64_t)(sketch_ms * 1000.0), g_stage_us[0] -= (int64_t)(sketch_ms * 1000.0);
		trace(kSeedName[sd], k, "end");
		return ok ? MPA_OK : MPA_ERR_HIP;
	};
	st.plan = [&](int pl, int32_t k) {
		trace(kPlanName[pl], k, "begin");
		{ StageClock sc(1); batch_plan_phase(work[k].b, plan_dev[pl]); }
		trace(kPlanName[pl], k, "end");
	};
	// DP lanes: a lane drives the DP rounds of a batch on its own device context (streams + buffers).  The rounds of one batch are
	// dominated by the tails of a few very long DP calls, during which the GPU is nearly idle; the next batch's rounds fill that space.
	st.dp = [&](int d, int32_t k) {
		trace(kLaneName[d], k, "begin");
		int rc;
		{ StageClock sc(2); rc = run_dp_rounds(lane_ctx[d], mi, &work[k].q, work[k].b); }
		trace(kLaneName[d], k, "end");
		return rc;
	};
	st.finish = [&](int32_t k, int32_t g, int32_t j) {
		trace("finish", k, "begin");
		StageClock sc(3);
		mpa_result_t *r = mpa_batch_finish(work[k].b);
		work[k].b = nullptr;
		char *t = nullptr;
		int64_t tl = 0;
		// (batches finish in input order: the hit ids run on.  MPA_GPU_FORMAT=1: the text came down with the result and is patched with the id)
		if (names && (tl = format_take_text(r, work[k].q.n_seq, id_io, &t)) < 0) tl = mpa_format_output(mi, opt, &work[k].q, names[g], r, id_io, &t);
		if (r) r->fmt_n_out = -1, std::string().swap(r->fmt_text), std::vector<int64_t>().swap(r->fmt_id_at);
		results[j] = r;
		if (names) text[j] = t, text_len[j] = tl;
		trace("finish", k, "end");
	};
	StreamResult res;
	run_stream(StreamShape{ n_batches, n_lanes, n_seed, n_plan, MPA_ERR_ARG, MPA_ERR_HIP }, st, res);
	ctx_absorb_sibling_stats(ctx);
	cpu_report_and_reset("mpa_map_batches", now_ms() - g_trace_t0);
	if (res.rc == MPA_OK) {
		if (n_mapped) *n_mapped = res.n_mapped;
		if (order) std::copy(res.order.begin(), res.order.end(), order);
	}
	if (res.rc != MPA_OK) {
		for (Work &w : work) delete w.b;
		for (int32_t k = 0; k < n_batches; ++k) {
			delete results[k], results[k] = nullptr;
			if (text && text[k]) free(text[k]), text[k] = nullptr;
		}
		set_error(res.err);
	}
	return res.rc;
}

void mpa_stage_clocks(double ms[5], int64_t calls[5], int reset)
{
	for (int k = 0; k < 5; ++k) {
		if (ms) ms[k] = (double)g_stage_us[k].load() / 1000.0;
		if (calls) calls[k] = g_stage_n[k].load();
		if (reset) g_stage_us[k] = 0, g_stage_n[k] = 0;
	}
}

int mpa_map_batches(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, int32_t n_batches, const mpa_qbatch_t *batches,
                    const char *const *const *names, int n_threads, mpa_result_t **results, int64_t *id_io, char **text, int64_t *text_len)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_map_batches_impl(ctx, mi, opt, n_batches, batches, names, n_threads, results, id_io, text, text_len); });
}

int mpa_map_batches_claim(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, int32_t n_batches, const mpa_qbatch_t *batches,
                          const char *const *const *names, int n_threads, mpa_result_t **results, int64_t *id_io, char **text, int64_t *text_len,
                          mpa_claim_fn claim, void *user, int32_t *n_mapped, int32_t *order)
{
	if (!claim || !n_mapped || !order) { set_error("mpa_map_batches_claim: claim, n_mapped and order are required"); return MPA_ERR_ARG; }
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_map_batches_impl(ctx, mi, opt, n_batches, batches, names, n_threads, results, id_io, text, text_len, claim, user, n_mapped, order); });
}

// One job over the GPUs of ONE process: the kt_for of mp_map_file (map.c:264-271, 291) across devices.  A pipeline per device
// context, each claiming the job's next mini-batch from one atomic counter whenever it has room (a faster or less loaded GPU
// maps more of the job); no data-path exchange between them -- the index is resident on every device, the results come back
// to the host anyway.  PAF text is formatted inside the pipelines; GFF3 / GTF text needs the running hit id of the whole file
// (map.c:306), so those jobs are formatted afterwards, in input order, from the exclusive prefix sum of mpa_result_n_output().
static int mpa_map_batches_multi_impl(int n_ctx, mpa_ctx_t *const *ctxs, mpa_idx_t *mi, const mpa_mapopt_t *opt, int32_t n_batches, const mpa_qbatch_t *batches,
                                      const char *const *const *names, int n_threads, mpa_result_t **results, int64_t *id_io, char **text, int64_t *text_len)
{
	if (n_ctx <= 0 || !ctxs) { set_error("mpa_map_batches_multi: no device context"); return MPA_ERR_NO_DEVICE; }
	if (n_ctx > 8) { set_error("mpa_map_batches_multi: at most eight device contexts"); return MPA_ERR_ARG; }
	if (names && (!text || !text_len || !id_io)) { set_error("mpa_map_batches_multi: names given without text/text_len/id_io"); return MPA_ERR_ARG; }
	for (int p = 0; p < n_ctx; ++p) {
		if (!ctxs[p]) { set_error("mpa_map_batches_multi: null context"); return MPA_ERR_NO_DEVICE; }
		const int rc = dev_upload_index(ctxs[p], mi);
		if (rc != MPA_OK) return rc;
	}
	if (n_ctx == 1) return mpa_map_batches_impl(ctxs[0], mi, opt, n_batches, batches, names, n_threads, results, id_io, text, text_len);
	for (int32_t k = 0; k < n_batches; ++k) { results[k] = nullptr; if (text) text[k] = nullptr; if (text_len) text_len[k] = 0; }
	const bool needs_ids = names && (opt->flag & (MPA_MF_GFF | MPA_MF_GTF));
	struct Pipe {
		std::vector<mpa_result_t*> res;
		std::vector<char*> text;
		std::vector<int64_t> tlen;
		std::vector<int32_t> order;
		int32_t n_mapped = 0;
		int64_t id = 0;
		int rc = MPA_OK;
		std::string err;
	};
	std::vector<Pipe> pipes((size_t)n_ctx);
	std::atomic<int32_t> next{0};
	struct Claim { std::atomic<int32_t> *next; int32_t n; };
	Claim cl{ &next, n_batches };
	auto claim = [](void *u) -> int32_t { Claim *c = (Claim*)u; const int32_t k = c->next->fetch_add(1); return k < c->n ? k : -1; };
	const int threads_each = std::max(1, n_threads / n_ctx);
	std::vector<std::thread> th;
	for (int p = 0; p < n_ctx; ++p) {
		Pipe &P = pipes[(size_t)p];
		P.res.assign((size_t)n_batches, nullptr), P.text.assign((size_t)n_batches, nullptr), P.tlen.assign((size_t)n_batches, 0), P.order.assign((size_t)n_batches, -1);
		th.emplace_back([&, p] {
			Pipe &Q = pipes[(size_t)p];
			Q.rc = mpa::guarded<int>(MPA_ERR_HIP, [&] {
				return mpa_map_batches_impl(ctxs[p], mi, opt, n_batches, batches, needs_ids ? nullptr : names, threads_each, Q.res.data(), &Q.id, needs_ids ? nullptr : Q.text.data(),
				                            needs_ids ? nullptr : Q.tlen.data(), claim, &cl, &Q.n_mapped, Q.order.data(), p);
			});
			if (Q.rc != MPA_OK) { Q.err = mpa_last_error(); next.store(n_batches); }   // (a failed pipeline ends the job for the others too)
		});
	}
	for (auto &t : th) t.join();
	int rc = MPA_OK;
	for (Pipe &P : pipes) if (P.rc != MPA_OK && rc == MPA_OK) rc = P.rc, set_error(P.err);
	for (Pipe &P : pipes)
		for (int32_t j = 0; j < P.n_mapped; ++j) {
			const int32_t k = P.order[(size_t)j];
			if (rc == MPA_OK && k >= 0 && k < n_batches) {
				results[k] = P.res[(size_t)j];
				if (names && !needs_ids) text[k] = P.text[(size_t)j], text_len[k] = P.tlen[(size_t)j];
			} else { delete P.res[(size_t)j]; if (P.text[(size_t)j]) free(P.text[(size_t)j]); }
		}
	if (rc != MPA_OK) {
		for (int32_t k = 0; k < n_batches; ++k) { delete results[k], results[k] = nullptr; if (text && text[k]) free(text[k]), text[k] = nullptr; }
		return rc;
	}
	for (int32_t k = 0; k < n_batches; ++k) if (!results[k]) { set_error("mpa_map_batches_multi: a batch was not mapped"); return MPA_ERR_HIP; }
	if (needs_ids) {
		std::vector<int64_t> id0((size_t)n_batches + 1, *id_io);
		for (int32_t k = 0; k < n_batches; ++k) id0[(size_t)k + 1] = id0[(size_t)k] + mpa_result_n_output(opt, &batches[k], results[k]);
		for (int32_t k = 0; k < n_batches; ++k) {               // (mpa_format_output threads its own parallel region over the queries)
			int64_t id = id0[(size_t)k];
			text_len[k] = mpa_format_output(mi, opt, &batches[k], names[k], results[k], &id, &text[k]);
		}
		*id_io = id0[(size_t)n_batches];
	} else if (names) {
		for (int32_t k = 0; k < n_batches; ++k) *id_io += mpa_result_n_output(opt, &batches[k], results[k]);
	}
	return MPA_OK;
}

int mpa_map_batches_multi(int n_ctx, mpa_ctx_t *const *ctxs, mpa_idx_t *mi, const mpa_mapopt_t *opt, int32_t n_batches, const mpa_qbatch_t *batches,
                          const char *const *const *names, int n_threads, mpa_result_t **results, int64_t *id_io, char **text, int64_t *text_len)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_map_batches_multi_impl(n_ctx, ctxs, mi, opt, n_batches, batches, names, n_threads, results, id_io, text, text_len); });
}

} // extern "C"
