// spans_dbg.cpp -- mpa_dbg_spans (include/mpamd_dbg.h), the test hook of MPA_GPU_SPANS: hand-made plans through the two steps of DESIGN.md
// section 4.10, on the device (dev_spans_* of stats_run.hip) or through the shared core on the host (spans_core.h).  It is built into a
// library of its own, libmpamd_dbg.so next to libmpamd.so, which it links against: the C ABI of libmpamd.so stays what it was.
#include <cstring>
#include <vector>
#include "mpa_internal.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

namespace {
// the packed genome as the shared core reads it on the host (StatsGenomeHost of host_batch.h)
struct GenomeHost {
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
}

extern "C" {

// Test hook of MPA_GPU_SPANS (mpamd.h): hand-made plans through both steps, on the device (ctx) or through the shared core (ctx == NULL)
static int mpa_dbg_spans_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans_v, int32_t n_seg,
                              const void *segs_v, int64_t n_rst1, const mpa_dp_rst_t *rst1, const uint32_t *pool1, int64_t n_pool1, int64_t n_rst2, const mpa_dp_rst_t *rst2,
                              const uint32_t *pool2, int64_t n_pool2, void *span_rec, mpa_dp_task_t *tasks, int32_t *n_task, void *asm_rec, uint32_t *cigar, int64_t cigar_cap)
{
	const SpansPlan *plan = (const SpansPlan*)plans_v;
	const SegRec *seg = (const SegRec*)segs_v;
	SpanRec *rec = (SpanRec*)span_rec;
	AsmRec *arec = (AsmRec*)asm_rec;
	if (!mi || !opt || !q || n_plan <= 0 || !plan || n_seg < 0 || n_rst1 <= 0 || !rst1 || n_pool1 < 0 || !rec || !tasks || !n_task) { set_error("mpa_dbg_spans: missing arguments"); return MPA_ERR_ARG; }
	// every index the two steps follow, checked here once for both paths
	const int64_t text_bytes = q->q_off[q->n_seq] - q->q_off[0];
	auto pool_ok = [](const mpa_dp_rst_t &o, int64_t n_pool) { return o.n_cigar >= 0 && o.cigar_off >= 0 && o.cigar_off + o.n_cigar <= n_pool; };
	for (int64_t k = 0; k < n_rst1; ++k) if (!pool_ok(rst1[k], n_pool1)) { set_error("mpa_dbg_spans: a round-1 result outside its pool"); return MPA_ERR_ARG; }
	for (int32_t j = 0; j < n_plan; ++j) {
		const SpansPlan &P = plan[j];
		const PlanRec &pl = P.pl;
		auto t_ok = [&](int32_t t, bool must) { return t < 0 ? !must && t == -1 : (int64_t)P.base1 + t < n_rst1; };
		if (P.base1 < 0 || !t_ok(pl.t_left, true) || !t_ok(pl.t_left2, false) || !t_ok(pl.t_right, pl.has_right != 0) || !t_ok(pl.t_right2, false) || pl.n_gap < 0 || pl.gap0 < 0 ||
		    (int64_t)pl.gap0 + pl.n_gap > n_seg || (P.vid >> 1) >= mi->ctg.size() || P.qlen < 0 || P.q_off < 0 || P.q_off + P.qlen > text_bytes || pl.as1 < 0 || pl.as1 > P.qlen ||
		    pl.mid_qe < 0 || pl.mid_qe > P.qlen) { set_error("mpa_dbg_spans: a plan that points outside its inputs"); return MPA_ERR_ARG; }
		const mpa_dp_rst_t *mine = rst1 + P.base1;
		for (int32_t t : { pl.t_left, pl.t_left2 }) if (t >= 0 && (mine[t].aa_len < 0 || spans_ext_aa(mine[t]) > pl.as1 || mine[t].nt_len < 0)) { set_error("mpa_dbg_spans: a left extension longer than its protein slice"); return MPA_ERR_ARG; }
		for (int32_t t : { pl.t_right, pl.t_right2 }) if (t >= 0 && (mine[t].aa_len < 0 || spans_ext_aa(mine[t]) > P.qlen - pl.mid_qe || mine[t].nt_len < 0)) { set_error("mpa_dbg_spans: a right extension longer than its protein slice"); return MPA_ERR_ARG; }
		for (int32_t g = 0; g < pl.n_gap; ++g) {
			const SegRec &x = seg[pl.gap0 + g];
			if (x.task < -1 || (x.task >= 0 && (int64_t)P.base1 + x.task >= n_rst1)) { set_error("mpa_dbg_spans: a gap segment without a result"); return MPA_ERR_ARG; }
		}
	}
	const SpansParams p{ opt->kmer2, opt->max_ext, opt->io, opt->asize };
	const int64_t t0 = q->q_off[0];
	std::vector<int64_t> slot((size_t)n_plan + 1, 0);
	auto check_round2 = [&](int32_t nt) {
		if (nt > n_rst2 || (nt > 0 && (!rst2 || !pool2)) || !arec || !cigar) { set_error("mpa_dbg_spans: fewer round-2 results than round-2 tasks"); return MPA_ERR_ARG; }
		for (int32_t k = 0; k < nt; ++k) if (!pool_ok(rst2[k], n_pool2)) { set_error("mpa_dbg_spans: a round-2 result outside its pool"); return MPA_ERR_ARG; }
		for (int32_t j = 0; j < n_plan; ++j) {
			int64_t n = 0;
			for (int32_t s = 0; s < spans_n_seg(plan[j], rec[j]); ++s) n += spans_seg_words(plan[j], rec[j], seg, rst1, rst2, s);
			slot[(size_t)j + 1] = slot[(size_t)j] + n;
		}
		if (slot[(size_t)n_plan] > cigar_cap) { set_error("mpa_dbg_spans: the CIGAR buffer is too small"); return MPA_ERR_ARG; }
		return MPA_OK;
	};
	if (!ctx) {
		uint8_t tab[ALN_TAB_BYTES];
		memcpy(tab + ALN_TAB_CODON, tab_codon(), 64), memcpy(tab + ALN_TAB_AA20, tab_aa20(), 256), memcpy(tab + ALN_TAB_MAT, opt->mat, 484);
		int32_t nt = 0;
		for (int32_t j = 0; j < n_plan; ++j) {
			const Contig &c = mi->ctg[plan[j].vid >> 1];
			const GenomeHost g{ mi->seq.data(), c.off, c.len, (int)(plan[j].vid & 1) };
			mpa_dp_task_t t[2];
			const int32_t n = spans_accept(p, plan[j], rst1, g, tab, (const uint8_t*)q->seqs + t0, rec[j], t);
			if (rec[j].left.task >= 0) rec[j].left.task += nt;
			if (rec[j].right.task >= 0) rec[j].right.task += nt;
			for (int32_t k = 0; k < n; ++k) tasks[nt++] = t[k];
		}
		*n_task = nt;
		if (n_rst2 < 0) return MPA_OK;
		const int rc = check_round2(nt);
		if (rc != MPA_OK) return rc;
		for (int32_t j = 0; j < n_plan; ++j) {
			arec[j] = spans_assemble<SpansSerial>(plan[j], rec[j], seg, rst1, pool1, rst2, pool2, cigar + slot[(size_t)j]);
			arec[j].cig_off = slot[(size_t)j];
		}
		return MPA_OK;
	}
	SpansIO io;
	int rc = dev_spans_stage(ctx, n_plan, n_seg, n_rst1, text_bytes, io);
	if (rc != MPA_OK) return rc;
	memcpy(io.plan, plan, (size_t)n_plan * sizeof(SpansPlan));
	if (n_seg > 0) memcpy(io.seg, seg, (size_t)n_seg * sizeof(SegRec));
	memcpy(io.rst1, rst1, (size_t)n_rst1 * sizeof(mpa_dp_rst_t));
	if (text_bytes > 0) memcpy(io.text, q->seqs + t0, (size_t)text_bytes);
	static const uint32_t none = 0;
	rc = dev_spans_round1(ctx, const_cast<mpa_idx_s*>(mi), p, opt->mat, n_plan, n_seg, n_rst1, text_bytes, pool1 ? pool1 : &none, n_pool1, io);
	if (rc != MPA_OK) return rc;
	memcpy(rec, io.rec, (size_t)n_plan * sizeof(SpanRec));
	if (io.n_task > 0) memcpy(tasks, io.task, (size_t)io.n_task * sizeof(mpa_dp_task_t));
	*n_task = io.n_task;
	if (n_rst2 < 0) return MPA_OK;
	if ((rc = check_round2(io.n_task)) != MPA_OK) return rc;
	SpansAsmIO ao;
	if ((rc = dev_spans_asm_stage(ctx, n_plan, io.n_task, ao)) != MPA_OK) return rc;
	if (io.n_task > 0) memcpy(ao.rst2, rst2, (size_t)io.n_task * sizeof(mpa_dp_rst_t));
	memcpy(ao.slot_off, slot.data(), ((size_t)n_plan + 1) * 8);
	if ((rc = dev_spans_assemble(ctx, n_plan, io.n_task, pool2 ? pool2 : &none, pool2 ? n_pool2 : 0, ao)) != MPA_OK) return rc;
	memcpy(arec, ao.rec, (size_t)n_plan * sizeof(AsmRec));
	if (slot[(size_t)n_plan] > 0) memcpy(cigar, ao.cigar, (size_t)slot[(size_t)n_plan] * 4);
	return MPA_OK;
}

int mpa_dbg_spans(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans, int32_t n_seg, const void *segs,
                  int64_t n_rst1, const mpa_dp_rst_t *rst1, const uint32_t *pool1, int64_t n_pool1, int64_t n_rst2, const mpa_dp_rst_t *rst2, const uint32_t *pool2,
                  int64_t n_pool2, void *span_rec, mpa_dp_task_t *tasks, int32_t *n_task, void *asm_rec, uint32_t *cigar, int64_t cigar_cap)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] {
		return mpa_dbg_spans_impl(ctx, mi, opt, q, n_plan, plans, n_seg, segs, n_rst1, rst1, pool1, n_pool1, n_rst2, rst2, pool2, n_pool2, span_rec, tasks, n_task, asm_rec, cigar,
		                          cigar_cap);
	});
}

} // extern "C"
