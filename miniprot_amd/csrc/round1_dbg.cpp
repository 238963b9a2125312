// round1_dbg.cpp -- mpa_dbg_round1_chain (include/mpamd_dbg.h), the test hook of MPA_GPU_ROUND1: a round-1 task
// table and the plans it belongs to through one submission -- the step's block staged and sent up without its record section, the round
// planned on the device and run with its records and dense pool assembled there, k_spans / k_spans_emit / k_task_bounds chained behind
// the results kernels, one wait (dp_run_round1_chained of dp_exec.hip) -- and then the explicit fetch of the dense pool.  Built into
// libmpamd_dbg.so: the C ABI of libmpamd.so stays what it was.
#include <cstring>
#include "mpa_internal.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

extern "C" int mpa_dbg_round1_chain(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_dpopt_t *dpopt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans_v,
                                    int32_t n_seg, const void *segs_v, int64_t n, const mpa_dp_task_t *tasks, mpa_dp_rst_t *rst, void *span_rec, mpa_dp_task_t *tasks2, int32_t *n_task,
                                    int64_t *bounds, uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&]() -> int {
		if (cigar_pool) *cigar_pool = nullptr;
		if (n_pool) *n_pool = 0;
		if (n_task) *n_task = 0;
		const SpansPlan *plan = (const SpansPlan*)plans_v;
		const SegRec *seg = (const SegRec*)segs_v;
		if (!ctx || !mi || !opt || !dpopt || !q || n_plan <= 0 || !plan || n_seg < 0 || (n_seg > 0 && !seg) || n <= 0 || !tasks || !rst || !span_rec || !tasks2 || !n_task || !bounds ||
		    !cigar_pool || !n_pool || !rec) { set_error("mpa_dbg_round1_chain: missing arguments"); return MPA_ERR_ARG; }
		for (int k = 0; k < MPA_DBG_ROUND1_REC; ++k) rec[k] = 0;
		bounds[0] = bounds[1] = bounds[2] = 0;
		// every index the step follows that does not depend on the round's results, as mpa_dbg_spans checks it
		const int64_t text_bytes = q->q_off[q->n_seq] - q->q_off[0];
		for (int32_t j = 0; j < n_plan; ++j) {
			const SpansPlan &P = plan[j];
			const PlanRec &pl = P.pl;
			auto t_ok = [&](int32_t t, bool must) { return t < 0 ? !must && t == -1 : (int64_t)P.base1 + t < n; };
			if (P.base1 < 0 || !t_ok(pl.t_left, true) || !t_ok(pl.t_left2, false) || !t_ok(pl.t_right, pl.has_right != 0) || !t_ok(pl.t_right2, false) || pl.n_gap < 0 || pl.gap0 < 0 ||
			    (int64_t)pl.gap0 + pl.n_gap > n_seg || (P.vid >> 1) >= mi->ctg.size() || P.qlen < 0 || P.q_off < 0 || P.q_off + P.qlen > text_bytes || pl.as1 < 0 || pl.as1 > P.qlen ||
			    pl.mid_qe < 0 || pl.mid_qe > P.qlen) { set_error("mpa_dbg_round1_chain: a plan that points outside its inputs"); return MPA_ERR_ARG; }
			// (an extension is no longer than the protein slice its task hands to the DP: what mpa_dbg_spans checks on the results)
			for (int32_t t : { pl.t_left, pl.t_left2 }) if (t >= 0 && tasks[P.base1 + t].al > pl.as1) { set_error("mpa_dbg_round1_chain: a left extension task longer than its protein slice"); return MPA_ERR_ARG; }
			for (int32_t t : { pl.t_right, pl.t_right2 }) if (t >= 0 && tasks[P.base1 + t].al > P.qlen - pl.mid_qe) { set_error("mpa_dbg_round1_chain: a right extension task longer than its protein slice"); return MPA_ERR_ARG; }
			for (int32_t g = 0; g < pl.n_gap; ++g) {
				const SegRec &x = seg[pl.gap0 + g];
				if (x.task < -1 || (x.task >= 0 && (int64_t)P.base1 + x.task >= n)) { set_error("mpa_dbg_round1_chain: a gap segment without a task"); return MPA_ERR_ARG; }
			}
		}
		SpansIO io;
		int rc = dev_spans_stage(ctx, n_plan, n_seg, n, text_bytes, io);
		if (rc == MPA_ERR_UNSUPPORTED) return MPA_DBG_ROUND1_DECLINED;
		if (rc != MPA_OK) return rc;
		memcpy(io.plan, plan, (size_t)n_plan * sizeof(SpansPlan));
		if (n_seg > 0) memcpy(io.seg, seg, (size_t)n_seg * sizeof(SegRec));
		if (text_bytes > 0) memcpy(io.text, q->seqs + q->q_off[0], (size_t)text_bytes);
		const SpansChain c{ SpansParams{ opt->kmer2, opt->max_ext, opt->io, opt->asize }, opt->mat, n_plan, n_seg, n, text_bytes, true };
		DpResidentRec rr;
		int64_t words = 0, parts[4] = { 0, 0, 0, 0 };
		rc = dp_run_round1_chained(ctx, mi, dpopt, q, n, tasks, c, rst, &words, io, &rr, parts);
		rec[0] = rr.plan_waits, rec[1] = rr.round_waits, rec[2] = rr.bytes_up, rec[3] = rr.task_bytes_up, rec[4] = rr.bytes_down, rec[5] = rr.pool_bytes_down, rec[6] = rr.chained_launches;
		rec[7] = parts[0], rec[8] = parts[1], rec[9] = parts[2], rec[10] = parts[3];
		if (rc == MPA_ERR_UNSUPPORTED) return MPA_DBG_ROUND1_DECLINED;
		if (rc != MPA_OK) return rc;
		memcpy(span_rec, io.rec, (size_t)n_plan * sizeof(SpanRec));
		if (io.n_task > 0) memcpy(tasks2, io.task, (size_t)io.n_task * sizeof(mpa_dp_task_t));
		*n_task = io.n_task;
		bounds[0] = io.r2.prep_bound, bounds[1] = io.r2.max_nl, bounds[2] = io.r2.max_al;
		if ((rc = dp_fetch_pool1(ctx, words, cigar_pool)) != MPA_OK) return rc;
		rec[11] = 4 * words;
		*n_pool = words;
		return MPA_OK;
	});
}

// mpa_dbg_spans_guard: the step between the rounds alone, on the device, under guard words that say the round behind it failed (err: the
// hand-off error word, bad: the bad-call word of the results header; at least one non-zero -- with both zero the step is mpa_dbg_spans).
// The kernels must read none of rst1[] (the caller may pass records no round wrote) and leave a task count and bounds of 0.
extern "C" int mpa_dbg_spans_guard(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans_v, int32_t n_seg,
                                   const void *segs_v, int64_t n_rst1, const mpa_dp_rst_t *rst1, int32_t err, int64_t bad, int32_t *n_task, int64_t *bounds)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&]() -> int {
		if (!ctx || !mi || !opt || !q || n_plan <= 0 || !plans_v || n_seg < 0 || (n_seg > 0 && !segs_v) || n_rst1 <= 0 || !rst1 || !n_task || !bounds) { set_error("mpa_dbg_spans_guard: missing arguments"); return MPA_ERR_ARG; }
		if (err == 0 && bad == 0) { set_error("mpa_dbg_spans_guard: both guard words are zero (that is mpa_dbg_spans)"); return MPA_ERR_ARG; }
		const int64_t text_bytes = q->q_off[q->n_seq] - q->q_off[0];
		SpansIO io;
		int rc = dev_spans_stage(ctx, n_plan, n_seg, n_rst1, text_bytes, io);
		if (rc != MPA_OK) return rc;
		memcpy(io.plan, plans_v, (size_t)n_plan * sizeof(SpansPlan));
		if (n_seg > 0) memcpy(io.seg, segs_v, (size_t)n_seg * sizeof(SegRec));
		memcpy(io.rst1, rst1, (size_t)n_rst1 * sizeof(mpa_dp_rst_t));
		if (text_bytes > 0) memcpy(io.text, q->seqs + q->q_off[0], (size_t)text_bytes);
		const SpansChain c{ SpansParams{ opt->kmer2, opt->max_ext, opt->io, opt->asize }, opt->mat, n_plan, n_seg, n_rst1, text_bytes, true };
		if ((rc = dev_spans_round1_guarded(ctx, const_cast<mpa_idx_s*>(mi), c, err, bad, io)) != MPA_OK) return rc;
		*n_task = io.n_task;
		bounds[0] = io.r2.prep_bound, bounds[1] = io.r2.max_nl, bounds[2] = io.r2.max_al;
		return MPA_OK;
	});
}
