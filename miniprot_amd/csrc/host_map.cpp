// host_map.cpp -- the batched replacement of mp_map() (map.c:143-240) and mp_align() (align.c:239-342).
//
// The reference maps one protein per thread from seeding to CIGAR.  Here a whole batch of proteins moves
// through the pipeline stage by stage so that every spliced-DP call of the batch can be issued to the GPU
// together:
//
//   stage A (host, threaded over queries)   sketch -> index lookup -> sort -> pre-chain -> chain ->
//                                           regions -> refine (k=5 re-seeding + re-chaining) -> select ->
//                                           extension limits -> per-region alignment plan
//   DP round 1 (GPU)   left + right extensions of every region            ns_global_gs16b EXT_LEFT/EXT_RIGHT
//                      + every gap between kept anchors with traceback (they do not depend on the extensions,
//                        so they run concurrently with the long extension windows)
//   DP round 2 (GPU)   the io_end retries of align.c:290-296,324-330
//   DP round 3 (GPU)   the two spans accepted by the extensions, with traceback
//   stage B (host, threaded)                CIGAR assembly, mp_extra_* statistics, final ranking
//
// The object is a plain stage machine (mpa_batch_*): it hands out DP tasks and takes DP results, and does
// not care who executes them.  mpa_map_batch() drives it with the HIP executor; the CPU-only tests drive
// it with the oracle to check the host logic against the reference's output.
// This file: the stage machine's C ABI (mpa_batch_*, mpa_result_*) and the blocking call mpa_map_batch() with the DP rounds of a batch.
//   host_plan.cpp      stage A: seeding, chaining, refinement, plans and round-1 tasks, on the host and by way of the device
//   host_align.cpp     what happens to the DP results: accepted spans, CIGARs, statistics, cs strings and residue rows, final ranking
//   host_pipeline.cpp  the stream: mpa_map_batches*, several batches in flight; its scheduler is host_pipeline.h
//   host_pool.cpp      the worker pools that parallel_for() runs on
//   host_hooks.cpp     the mpa_dbg_* test hooks of stage A
#include <algorithm>
#include <cstring>
#include "host_batch.h"

using namespace mpa;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

static mpa_batch_t *mpa_batch_begin_impl(const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads)
{
	return batch_begin_impl(nullptr, mi, opt, q, n_threads);
}

mpa_batch_t *mpa_batch_begin(const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads)
{
	return mpa::guarded<mpa_batch_t *>(nullptr, [&] { return mpa_batch_begin_impl(mi, opt, q, n_threads); });
}

int64_t mpa_batch_dp_tasks(mpa_batch_t *b, const mpa_dp_task_t **tasks, mpa_dpopt_t *opt)
{
	if (opt) *opt = b->dpopt;
	*tasks = nullptr;
	if (b->round == 0) {
		double t0 = now_ms();
		emit_round1(b);
		timing_note("emit round 1", now_ms() - t0);
		b->round = 1;
		if (b->tasks.empty()) { const int rc = take_round3(b, nullptr, nullptr); if (rc != MPA_OK) return rc; b->round = 4; }   // nothing to align at all
	}
	// (round 2 without tasks: every accepted span took the ungapped shortcut)
	if (b->round == 2 && b->tasks.empty()) { const int rc = take_round3(b, nullptr, nullptr); if (rc != MPA_OK) return rc; b->round = 4; }
	if (b->round >= 4) { *tasks = nullptr; return 0; }
	*tasks = b->tasks.data();
	return (int64_t)b->tasks.size();
}

static int mpa_batch_dp_results_impl(mpa_batch_t *b, const mpa_dp_rst_t *rst, const uint32_t *cigar_pool)
{
	double t0 = now_ms();
	if (b->round == 1) { const int rc = spans_take_round1(b, rst, cigar_pool); if (rc != MPA_OK) return rc; b->round = 2; timing_note("take 1 / emit 2", now_ms() - t0); }
	else if (b->round == 2) {
		const int rc = take_round3(b, rst, cigar_pool);
		if (rc != MPA_OK) return rc;
		b->round = 4; b->tasks.clear(); timing_note("take 2 + finish", now_ms() - t0);
	}
	else { set_error("mpa_batch_dp_results called out of sequence"); return MPA_ERR_ARG; }
	return MPA_OK;
}

int mpa_batch_dp_results(mpa_batch_t *b, const mpa_dp_rst_t *rst, const uint32_t *cigar_pool)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_batch_dp_results_impl(b, rst, cigar_pool); });
}

static mpa_result_t *mpa_batch_finish_impl(mpa_batch_t *b)
{
	double t_fin = now_ms();
	if (b->flat) {                                           // (MPA_GPU_FINISH: the step behind the walks laid the result out already)
		mpa_result_s *res = b->flat.release();
		res->n_seq = (int32_t)b->qs.size();
		parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t i) { b->qs[i] = QueryState(); });
		delete b;
		timing_note("batch_finish (flatten)", now_ms() - t_fin);
		return res;
	}
	mpa_result_s *res = new mpa_result_s();
	res->n_seq = (int32_t)b->qs.size();
	res->hit_off.assign(b->qs.size() + 1, 0);
	for (size_t qi = 0; qi < b->qs.size(); ++qi) {
		QueryState &qs = b->qs[qi];
		res->hit_off[qi] = (int64_t)res->hits.size();
		for (const Region &r : qs.regs) {
			mpa_hit_t h;
			memset(&h, 0, sizeof(h));
			h.qid = qs.qid, h.id = r.id, h.parent = r.parent, h.n_sub = r.n_sub, h.subsc = r.subsc, h.cnt = r.cnt;
			h.n_exon = r.n_exon, h.chn_sc = r.chn_sc, h.chn_sc_ungap = r.chn_sc_ungap, h.vid = r.vid;
			h.qs = r.qs, h.qe = r.qe, h.vs = r.vs, h.ve = r.ve, h.has_aln = r.aligned;
			h.dp_score = r.dp_score, h.dp_max = r.dp_max, h.dp_max2 = r.dp_max2, h.blen = r.blen, h.n_fs = r.n_fs, h.n_stop = r.n_stop;
			h.dist_stop = r.dist_stop, h.dist_start = r.dist_start, h.n_iden = r.n_iden, h.n_plus = r.n_plus;
			h.n_cigar = (int32_t)r.cigar.size(), h.n_feat = (int32_t)r.feat.size();
			h.cigar_off = (int64_t)res->cigars.size(), h.feat_off = (int64_t)res->feats.size();
			res->cigars.insert(res->cigars.end(), r.cigar.begin(), r.cigar.end());
			for (const Feat &f : r.feat) {
				mpa_feat_t o;
				memset(&o, 0, sizeof(o));
				o.vs = f.vs, o.ve = f.ve, o.qs = f.qs, o.qe = f.qe, o.type = f.type, o.phase = f.phase, o.n_fs = f.n_fs, o.n_stop = f.n_stop;
				o.score = f.score, o.n_iden = f.n_iden, o.blen = f.blen;
				memcpy(o.donor, f.donor, 2), memcpy(o.acceptor, f.acceptor, 2);
				res->feats.push_back(o);
			}
			if (r.cs_src) {                                    // the cs body that came with the region (MPA_GPU_CS): one entry per hit from here on
				res->cs.resize(res->hits.size(), mpa_result_s::CsRef{ 0, 0, 0 });
				res->cs.push_back(mpa_result_s::CsRef{ (int64_t)res->cs_text.size(), (int32_t)r.cs.size(), 1 });
				res->cs_text += r.cs;
			}
			if (r.rows_src) {                                  // its residue rows the same way (MPA_GPU_ROWS)
				res->rows.resize(res->hits.size(), mpa_result_s::RowsRef{ 0, 0, 0, 0 });
				res->rows.push_back(mpa_result_s::RowsRef{ (int64_t)res->rows_text.size(), r.rows_w, r.rows_sta, 1 });
				res->rows_text += r.rows;
			}
			res->hits.push_back(h);
		}
	}
	if (!res->cs.empty()) res->cs.resize(res->hits.size(), mpa_result_s::CsRef{ 0, 0, 0 });
	if (!res->rows.empty()) res->rows.resize(res->hits.size(), mpa_result_s::RowsRef{ 0, 0, 0, 0 });
	res->hit_off[b->qs.size()] = (int64_t)res->hits.size();
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t i) { b->qs[i] = QueryState(); });   // free per-query state in parallel
	delete b;
	timing_note("batch_finish (flatten)", now_ms() - t_fin);
	return res;
}

mpa_result_t *mpa_batch_finish(mpa_batch_t *b)
{
	return mpa::guarded<mpa_result_t *>(nullptr, [&] { return mpa_batch_finish_impl(b); });
}

int64_t mpa_result_n_hit(const mpa_result_t *r) { return (int64_t)r->hits.size(); }
const mpa_hit_t *mpa_result_hits(const mpa_result_t *r) { return r->hits.data(); }
const int64_t *mpa_result_hit_off(const mpa_result_t *r) { return r->hit_off.data(); }
const uint32_t *mpa_result_cigars(const mpa_result_t *r) { return r->cigars.data(); }
const mpa_feat_t *mpa_result_feats(const mpa_result_t *r) { return r->feats.data(); }
void mpa_result_destroy(mpa_result_t *r) { delete r; }

} // extern "C"

// one (sub-)batch through the stage machine with the HIP executor
int mpa::run_dp_rounds(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_qbatch_t *q, mpa_batch_t *b)
{
	const mpa_dp_task_t *tasks;
	mpa_dpopt_t dpopt;
	int64_t n;
	std::vector<mpa_dp_rst_t> rst;
	b->dp_ctx = ctx;                 // (MPA_GPU_STATS=1: the statistics pass behind the last round runs there too)
	while ((n = mpa_batch_dp_tasks(b, &tasks, &dpopt)) != 0) {
		if (n < 0) return (int)n;                // (a device statistics call behind a round without tasks failed)
		uint32_t *pool = nullptr;
		int64_t n_pool = 0;
		rst.resize((size_t)n);
		double t0 = now_ms();
		int rc = MPA_ERR_UNSUPPORTED;
		// (MPA_GPU_ROUND2=1) round 2 planned from the tasks the device step between the rounds left in place, its records and dense pool
		// assembled on the device: no pool comes back.  Declined: the round runs through mpa_dp_run as always
		if (b->round == 2 && round2_knob()) {
			if (b->spans_src != 2 || !b->r2_in.d_tasks) set_error("the step between the rounds did not run on the device");
			else rc = dp_run_resident(ctx, mi, &dpopt, q, n, b->r2_in, rst.data(), &n_pool, &b->r2_rst_dev, nullptr);
			if (rc == MPA_OK) b->r2_resident = true;
			else if (rc != MPA_ERR_UNSUPPORTED) return rc;
			else if (timing_on()) fprintf(stderr, "[mpa-timing]   round 2 resident declined (%s): mpa_dp_run\n", mpa_last_error());
		}
		// (MPA_GPU_ROUND1=1) round 1 planned on the device from the batch's tasks, its records and dense pool assembled there and the step
		// between the rounds chained behind them, inside the round's one wait: no pool comes back, and spans_take_round1 finds the step's
		// outputs with the batch.  Declined: mpa_dp_run and the step as always
		if (b->round == 1 && round1_knob()) {
			const char *why = nullptr;
			rc = spans_round1_resident(b, ctx, &dpopt, n, tasks, rst.data(), &n_pool, &why);
			if (rc != MPA_OK && rc != MPA_ERR_UNSUPPORTED) return rc;
			if (rc != MPA_OK && timing_on()) fprintf(stderr, "[mpa-timing]   round 1 resident declined (%s): mpa_dp_run\n", why ? why : mpa_last_error());
		}
		if (rc == MPA_ERR_UNSUPPORTED) rc = mpa_dp_run(ctx, mi, &dpopt, q, n, tasks, rst.data(), &pool, &n_pool);
		timing_note("mpa_dp_run (total)", now_ms() - t0);
		if (rc != MPA_OK) { free(pool); return rc; }
		b->dp_n_pool = n_pool;           // (MPA_GPU_SPANS=1: the round's dense pool is still on the context)
		rc = mpa_batch_dp_results(b, rst.data(), pool);
		if (b->spans_want_pool) b->sp_pool1 = pool, pool = nullptr, b->spans_want_pool = false;   // (round 1's words stay with the batch: a declined step behind round 2 reads them)
		free(pool);
		if (rc != MPA_OK) return rc;
	}
	return MPA_OK;
}

static int run_batch_on(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, mpa_result_t **out)
{
	*out = nullptr;
	mpa_batch_t *b = batch_begin_impl(ctx, mi, opt, q, n_threads);
	if (!b) return MPA_ERR_ARG;
	const int rc = run_dp_rounds(ctx, mi, q, b);
	if (rc != MPA_OK) { delete b; return rc; }
	*out = mpa_batch_finish(b);
	return MPA_OK;
}

extern "C" {

static int mpa_map_batch_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, mpa_result_t **out)
{
	*out = nullptr;
	if (!ctx) { set_error("mpa_map_batch needs a device context: the DP has no CPU fallback"); return MPA_ERR_NO_DEVICE; }
	return run_batch_on(ctx, mi, opt, q, n_threads, out);
}

int mpa_map_batch(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, mpa_result_t **out)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_map_batch_impl(ctx, mi, opt, q, n_threads, out); });
}

} // extern "C"
