// stats_run.hip -- the device unit of the steps behind the DP rounds.
// The walks over the finished alignments (kernels: stats_kernels.hip): statistics and exon features (MPA_GPU_STATS=1, k_aln_stats, code:
// aln_stats_core.h), cs:Z: difference strings (MPA_GPU_CS=1, k_aln_cs, aln_cs_core.h) and --aln / --trans
// residue rows (MPA_GPU_ROWS=1, k_aln_rows, aln_rows_core.h; section 4.9).  One call takes any of the three: take_round3() of
// host_align.cpp fills one pinned block (tables | jobs | cs slot offsets | rows slot offsets | CIGAR words | the batch's protein text;
// the offset sections only for the walks asked for) through dev_aln_walks_stage(), dev_aln_walks() sends it up, launches up to three
// kernels on the context that ran the batch's DP rounds, takes one pinned block down for each (statistics: per-alignment records |
// features; cs: lengths | slots; rows: records | slots) and waits once.  The pools (st_in, st_out, cs_out, rows_out and their staging)
// are grow-only and allocated by the first call that asks for them: a run that never sets a knob holds none of them.
// MPA_GPU_SPANS=1 (kernels k_spans, k_spans_emit, k_assemble: span_kernels.hip; code: spans_core.h) puts the
// host step between the DP rounds and the one behind them here: dev_spans_stage() / dev_spans_round1() and dev_spans_asm_stage() /
// dev_spans_assemble().  The CIGAR pool k_assemble writes (sp_cig) stays on the device until the context's next call, and
// dev_aln_walks() reads it in place of an uploaded one when the caller says so (dev_cig).
#include "dev_ctx.h"
#include "spans_core.h"
#include "dp_results_core.h"
#include "stats_kernels.hip"
#include "span_kernels.hip"

namespace mpa {

namespace {
struct StatsLayout {
	size_t off_jobs, off_slot, off_rslot, off_cig, off_text, up_bytes, off_feat, down_bytes, off_body, cs_down_bytes, off_rbody, rows_down_bytes;
	// slot_bytes < 0: no cs strings; rows_bytes < 0: no residue rows (the block that goes up is then what it was without them)
	explicit StatsLayout(const AlnWalkSizes &z)
	{
		auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
		off_jobs = 1024;                                                   // (the tables take ALN_TAB_BYTES of the first KB)
		off_slot = off_jobs + up16((size_t)z.n_jobs * sizeof(AlnStatsJob));
		off_rslot = off_slot + (z.slot_bytes >= 0 ? up16((size_t)(z.n_jobs + 1) * 8) : 0);
		off_cig = off_rslot + (z.rows_bytes >= 0 ? up16((size_t)(z.n_jobs + 1) * 8) : 0);
		off_text = off_cig + up16((size_t)z.n_cigar * 4);
		up_bytes = off_text + up16((size_t)z.text_bytes) + 16;
		off_feat = up16((size_t)z.n_jobs * sizeof(AlnStatsOut));
		down_bytes = off_feat + (size_t)(z.n_feat > 0 ? z.n_feat : 0) * sizeof(AlnFeat) + 16;
		off_body = up16((size_t)z.n_jobs * sizeof(AlnCsOut));
		cs_down_bytes = off_body + (size_t)(z.slot_bytes > 0 ? z.slot_bytes : 0) + 16;
		off_rbody = up16((size_t)z.n_jobs * sizeof(AlnRowsOut));
		rows_down_bytes = off_rbody + (size_t)(z.rows_bytes > 0 ? z.rows_bytes : 0) + 16;
	}
};
static_assert(ALN_TAB_BYTES <= 1024, "the tables share the first KB of the staging block");
}

// The pinned blocks of a call for any non-empty subset of the walks, the one that goes up for the caller to fill: jobs, CIGAR words,
// text and, next to the jobs, cs.slot_off[n_jobs + 1] / rows.slot_off[n_jobs + 1].  z.n_feat < 0: no statistics (the statistics stay
// on the host and no feature slots come down); z.slot_bytes = the sum of the alignments' aln_cs_bound() (< 0: no cs strings);
// z.rows_bytes = the sum of their aln_rows_slot() (< 0: no rows).  MPA_ERR_UNSUPPORTED: no memory for it
int dev_aln_walks_stage(mpa_ctx_t *ctx, const AlnWalkSizes &z, AlnStatsIO &io, AlnCsIO &cs, AlnRowsIO &rows)
{
	io = AlnStatsIO(), cs = AlnCsIO(), rows = AlnRowsIO();
	if (z.n_jobs <= 0 || z.n_jobs > (int64_t)1 << 28) { set_error("GPU alignment statistics / cs strings / residue rows: no alignments, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const StatsLayout L(z);
	if (ctx->walks.h_stats_up.ensure(L.up_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (z.slot_bytes >= 0 && ctx->walks.h_cs_down.ensure(L.cs_down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (z.rows_bytes >= 0 && ctx->walks.h_rows_down.ensure(L.rows_down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (z.n_feat >= 0 && ctx->walks.h_stats_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->walks.h_stats_up.as<char>();
	io.jobs = (AlnStatsJob*)(hu + L.off_jobs), io.cigar = (uint32_t*)(hu + L.off_cig), io.text = hu + L.off_text;
	if (z.slot_bytes >= 0) cs.slot_off = (int64_t*)(hu + L.off_slot);
	if (z.rows_bytes >= 0) rows.slot_off = (int64_t*)(hu + L.off_rslot);
	return MPA_OK;
}

// The walks asked for over the z.n_jobs alignments staged in io / cs / rows, on ctx: the tables into the staged block, one upload, the
// launches (statistics: k_aln_stats; cs: k_aln_cs; rows: k_aln_rows), their downloads and one wait.  Afterwards io.out / io.feat hold
// the statistics, cs.out[j].len bytes lie at cs.body + cs.slot_off[j], and rows.out[j] describes the slot at rows.body +
// rows.slot_off[j] as aln_rows_core.h lays it out -- all of it pinned memory of the context, valid until its next call.
// MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller keeps the host's walks.
int dev_aln_walks(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const AlnRowsParams &rp, const int8_t *mat, const AlnWalkSizes &z, AlnStatsIO &io, AlnCsIO &cs,
                  AlnRowsIO &rows, bool dev_cig)
{
	const StatsLayout L(z);
	const int64_t n_jobs = z.n_jobs;
	const bool stats = z.n_feat >= 0, cs_on = z.slot_bytes >= 0, rows_on = z.rows_bytes >= 0;
	if (dev_cig && !ctx->spans.sp_cig.p) { set_error("dev_aln_walks: no assembled CIGAR pool on this context"); return MPA_ERR_ARG; }
	if (p.asize < 1 || p.asize * p.asize > 484) { set_error("GPU alignment statistics: a substitution matrix of more than 22 x 22"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	const DeviceIndex *d = mi->dev[ctx->device];
	if (L.up_bytes > ctx->walks.h_stats_up.cap || (stats && L.down_bytes > ctx->walks.h_stats_down.cap) || (cs_on && L.cs_down_bytes > ctx->walks.h_cs_down.cap) ||
	    (rows_on && L.rows_down_bytes > ctx->walks.h_rows_down.cap)) {
		set_error("dev_aln_walks: the staging block was not sized for this call");
		return MPA_ERR_ARG;
	}
	tl_alloc_failed = false;
	if (ctx->walks.st_in.ensure(L.up_bytes) != MPA_OK || (stats && ctx->walks.st_out.ensure(L.down_bytes) != MPA_OK) || (cs_on && ctx->walks.cs_out.ensure(L.cs_down_bytes) != MPA_OK) ||
	    (rows_on && ctx->walks.rows_out.ensure(L.rows_down_bytes) != MPA_OK))
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *hu = ctx->walks.h_stats_up.as<char>();
	aln_tables_fill((uint8_t*)hu, mat, (size_t)(p.asize * p.asize));
	HIP_TRY(hipMemcpyAsync(ctx->walks.st_in.p, hu, L.up_bytes - 16, hipMemcpyHostToDevice, s));
	const char *din = ctx->walks.st_in.as<char>();
	const uint32_t *dcig = dev_cig ? ctx->spans.sp_cig.as<uint32_t>() : (const uint32_t*)(din + L.off_cig);   // (MPA_GPU_SPANS=1: where k_assemble left the words)
	const unsigned nwg = (unsigned)((n_jobs + STATS_WAVES - 1) / STATS_WAVES);
	if (stats) {
		char *dout = ctx->walks.st_out.as<char>();
		hipLaunchKernelGGL(k_aln_stats, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din, p,
		                   (const uint8_t*)(din + L.off_text), dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (AlnStatsOut*)dout, (AlnFeat*)(dout + L.off_feat));
		HIP_TRY(hipGetLastError());
		char *hd = ctx->walks.h_stats_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.down_bytes - 16, hipMemcpyDeviceToHost, s));
		io.out = (const AlnStatsOut*)hd, io.feat = (const AlnFeat*)(hd + L.off_feat);
	}
	if (cs_on) {
		char *dout = ctx->walks.cs_out.as<char>();
		hipLaunchKernelGGL(k_aln_cs, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din,
		                   (const uint8_t*)(din + L.off_text), dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (const int64_t*)(din + L.off_slot), (AlnCsOut*)dout, dout + L.off_body);
		HIP_TRY(hipGetLastError());
		char *hd = ctx->walks.h_cs_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.cs_down_bytes - 16, hipMemcpyDeviceToHost, s));
		cs.out = (const AlnCsOut*)hd, cs.body = hd + L.off_body;
	}
	if (rows_on) {
		char *dout = ctx->walks.rows_out.as<char>();
		hipLaunchKernelGGL(k_aln_rows, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din, rp,
		                   (const uint8_t*)(din + L.off_text), dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (const int64_t*)(din + L.off_rslot), (AlnRowsOut*)dout, dout + L.off_rbody);
		HIP_TRY(hipGetLastError());
		char *hd = ctx->walks.h_rows_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.rows_down_bytes - 16, hipMemcpyDeviceToHost, s));
		rows.out = (const AlnRowsOut*)hd, rows.body = hd + L.off_rbody;
	}
	HIP_TRY(wait_stream(ctx, s));
	return MPA_OK;
}

// ---- MPA_GPU_SPANS=1 ------------------------------------------------------------------------------------------------------------
namespace {
static const size_t SPANS_HEAD_BYTES = 32;
struct SpansLayout {
	size_t off_plan, off_seg, off_rst1, off_text, up_bytes;                  // sp_in / h_sp_up (the tables take the first KB)
	size_t off_tmp, off_excl, off_bsum, mid_bytes;                            // sp_mid (records with local numbers at 0)
	size_t off_rec, off_task, down_bytes;                                     // sp_out / h_sp_down (the task count at 0, the tasks' three bounds as int64 at 8)
	unsigned blocks;
	SpansLayout(int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes)
	{
		auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
		blocks = (unsigned)((n_plan + SPANS_BLOCK - 1) / SPANS_BLOCK);
		off_plan = 1024;
		off_seg = off_plan + up16((size_t)n_plan * sizeof(SpansPlan));
		off_rst1 = off_seg + up16((size_t)n_seg * sizeof(SegRec));
		off_text = off_rst1 + up16((size_t)n_rst1 * sizeof(mpa_dp_rst_t));
		up_bytes = off_text + up16((size_t)text_bytes) + 16;
		off_tmp = up16((size_t)n_plan * sizeof(SpanRec));
		off_excl = off_tmp + up16((size_t)n_plan * 2 * sizeof(mpa_dp_task_t));
		off_bsum = off_excl + up16((size_t)n_plan * 4);
		mid_bytes = off_bsum + up16((size_t)blocks * 4) + 16;
		off_rec = SPANS_HEAD_BYTES;
		off_task = off_rec + up16((size_t)n_plan * sizeof(SpanRec));
		down_bytes = off_task + (size_t)n_plan * 2 * sizeof(mpa_dp_task_t) + 16;
	}
};
struct AsmLayout {
	size_t off_slot, off_pool2, up_bytes, rec_bytes;
	AsmLayout(int64_t n_plan, int64_t n_rst2, int64_t n_pool2)
	{
		auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
		off_slot = up16((size_t)n_rst2 * sizeof(mpa_dp_rst_t));
		off_pool2 = off_slot + up16((size_t)(n_plan + 1) * 8);
		up_bytes = off_pool2 + up16((size_t)n_pool2 * 4) + 16;
		rec_bytes = up16((size_t)n_plan * sizeof(AsmRec));
	}
};
static_assert(sizeof(SpansPlan) % 8 == 0 && sizeof(SpanRec) % 8 == 0 && sizeof(AsmRec) % 8 == 0, "records in 16-byte aligned sections");
}

int dev_spans_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes, SpansIO &io)
{
	io = SpansIO();
	if (n_plan <= 0 || n_plan > (int64_t)1 << 28 || n_seg < 0 || n_rst1 <= 0) { set_error("GPU spans: no plans, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const SpansLayout L(n_plan, n_seg, n_rst1, text_bytes);
	if (ctx->spans.h_sp_up.ensure(L.up_bytes) != MPA_OK || ctx->spans.h_sp_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->spans.h_sp_up.as<char>();
	io.plan = (SpansPlan*)(hu + L.off_plan), io.seg = (SegRec*)(hu + L.off_seg), io.rst1 = (mpa_dp_rst_t*)(hu + L.off_rst1), io.text = hu + L.off_text;
	return MPA_OK;
}

int dev_spans_round1(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansParams &p, const int8_t *mat, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes,
                     const uint32_t *pool1, int64_t n_pool1, SpansIO &io)
{
	ctx->spans.sp_keep.n_plan = -1;
	if (p.asize < 1 || p.asize * p.asize > 484) { set_error("GPU spans: a substitution matrix of more than 22 x 22"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	const DeviceIndex *d = mi->dev[ctx->device];
	const SpansLayout L(n_plan, n_seg, n_rst1, text_bytes);
	if (L.up_bytes > ctx->spans.h_sp_up.cap || L.down_bytes > ctx->spans.h_sp_down.cap) { set_error("dev_spans_round1: the staging block was not sized for this call"); return MPA_ERR_ARG; }
	if (n_pool1 < 0 || (!pool1 && n_pool1 > 0 && (size_t)n_pool1 * 4 > ctx->round.cigd.cap)) { set_error("dev_spans_round1: no round-1 CIGAR pool of that size on this context"); return MPA_ERR_ARG; }
	tl_alloc_failed = false;
	if (ctx->spans.sp_in.ensure(L.up_bytes) != MPA_OK || ctx->spans.sp_mid.ensure(L.mid_bytes) != MPA_OK || ctx->spans.sp_out.ensure(L.down_bytes) != MPA_OK ||
	    ctx->spans.sp_pool1.ensure((size_t)n_pool1 * 4 + 16) != MPA_OK)
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *hu = ctx->spans.h_sp_up.as<char>();
	aln_tables_fill((uint8_t*)hu, mat, (size_t)(p.asize * p.asize));
	HIP_TRY(hipMemcpyAsync(ctx->spans.sp_in.p, hu, L.up_bytes - 16, hipMemcpyHostToDevice, s));
	// the round-1 pool stays: round 2 overwrites cigd
	if (n_pool1 > 0) HIP_TRY(hipMemcpyAsync(ctx->spans.sp_pool1.p, pool1 ? (const void*)pool1 : ctx->round.cigd.p, (size_t)n_pool1 * 4, pool1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
	const char *din = ctx->spans.sp_in.as<char>();
	char *mid = ctx->spans.sp_mid.as<char>(), *dout = ctx->spans.sp_out.as<char>();
	SpansArgs a;
	a.plan = (const SpansPlan*)(din + L.off_plan), a.n_plan = (int32_t)n_plan, a.rst1 = (const mpa_dp_rst_t*)(din + L.off_rst1);
	a.text = (const uint8_t*)(din + L.off_text), a.tabs = (const uint8_t*)din, a.seq = (const uint8_t*)d->seq, a.ctg_off = d->ctg_off, a.ctg_len = d->ctg_len;
	a.p = p, a.rec = (SpanRec*)mid, a.tmp = (mpa_dp_task_t*)(mid + L.off_tmp), a.excl = (int32_t*)(mid + L.off_excl), a.bsum = (int32_t*)(mid + L.off_bsum);
	hipLaunchKernelGGL(k_spans, dim3(L.blocks), dim3(SPANS_BLOCK), 0, s, a);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_spans_emit, dim3(L.blocks), dim3(SPANS_BLOCK), 0, s, a, (int32_t*)dout, (SpanRec*)(dout + L.off_rec), (mpa_dp_task_t*)(dout + L.off_task));
	HIP_TRY(hipGetLastError());
	const bool want_r2 = round2_knob();                  // (MPA_GPU_ROUND2=1) the bounds of the tasks just written, for the planner of round 2
	if (want_r2) {
		HIP_TRY(hipMemsetAsync(dout + 8, 0, 24, s));
		hipLaunchKernelGGL(k_task_bounds, dim3((unsigned)((2 * n_plan + SPANS_BLOCK - 1) / SPANS_BLOCK)), dim3(SPANS_BLOCK), 0, s, (const mpa_dp_task_t*)(dout + L.off_task), (const int32_t*)dout,
		                   (int64_t*)(dout + 8));
		HIP_TRY(hipGetLastError());
	}
	char *hd = ctx->spans.h_sp_down.as<char>();
	HIP_TRY(hipMemcpyAsync(hd, dout, L.down_bytes - 16, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	io.n_task = *(const int32_t*)hd, io.rec = (const SpanRec*)(hd + L.off_rec), io.task = (const mpa_dp_task_t*)(hd + L.off_task);
	io.r2 = DpResidentIn();
	if (want_r2) { const int64_t *bd = (const int64_t*)(hd + 8); io.r2.d_tasks = (const mpa_dp_task_t*)(dout + L.off_task), io.r2.prep_bound = bd[0], io.r2.max_nl = bd[1], io.r2.max_al = bd[2]; }
	if (io.n_task < 0 || io.n_task > 2 * n_plan) { set_error("dev_spans_round1: an impossible task count"); return MPA_ERR_HIP; }
	ctx->spans.sp_keep.off_plan = L.off_plan, ctx->spans.sp_keep.off_seg = L.off_seg, ctx->spans.sp_keep.off_rst1 = L.off_rst1, ctx->spans.sp_keep.n_plan = n_plan, ctx->spans.sp_keep.n_pool1 = n_pool1;
	return MPA_OK;
}

int dev_spans_asm_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_rst2, SpansAsmIO &io)
{
	io = SpansAsmIO();
	if (n_plan <= 0 || n_plan != ctx->spans.sp_keep.n_plan || n_rst2 < 0) { set_error("GPU spans: the plans of this batch are not on the device"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const AsmLayout L(n_plan, n_rst2, 0);
	if (ctx->spans.h_sp_up2.ensure(L.up_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->spans.h_sp_up2.as<char>();
	io.rst2 = (mpa_dp_rst_t*)hu, io.slot_off = (int64_t*)(hu + L.off_slot);
	return MPA_OK;
}

int dev_spans_assemble(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_rst2, const uint32_t *pool2, int64_t n_pool2, SpansAsmIO &io, const mpa_dp_rst_t *d_rst2)
{
	if (n_plan <= 0 || n_plan != ctx->spans.sp_keep.n_plan) { set_error("dev_spans_assemble: the plans of this batch are not on the device"); return MPA_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	const AsmLayout L0(n_plan, n_rst2, 0), L(n_plan, n_rst2, pool2 ? n_pool2 : 0);
	if (L0.up_bytes > ctx->spans.h_sp_up2.cap || !io.slot_off) { set_error("dev_spans_assemble: the staging block was not sized for this call"); return MPA_ERR_ARG; }
	if (n_pool2 < 0 || (!pool2 && n_pool2 > 0 && (size_t)n_pool2 * 4 > ctx->round.cigd.cap)) { set_error("dev_spans_assemble: no round-2 CIGAR pool of that size on this context"); return MPA_ERR_ARG; }
	const int64_t n_words = io.slot_off[n_plan];
	if (n_words < 0) { set_error("dev_spans_assemble: negative slot offsets"); return MPA_ERR_ARG; }
	const size_t down_bytes = L.rec_bytes + (size_t)n_words * 4 + 16;
	if (ctx->spans.h_sp_down2.ensure(down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	tl_alloc_failed = false;
	if (ctx->spans.sp_in2.ensure(L.up_bytes) != MPA_OK || ctx->spans.sp_asm.ensure(L.rec_bytes + 16) != MPA_OK || ctx->spans.sp_cig.ensure((size_t)n_words * 4 + 16) != MPA_OK)
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *din2 = ctx->spans.sp_in2.as<char>();
	// (d_rst2: round 2's records are on the device already, where the round's own kernels wrote them -- only the slot offsets go up)
	const size_t up_from = d_rst2 ? L0.off_slot : 0;
	HIP_TRY(hipMemcpyAsync(din2 + up_from, ctx->spans.h_sp_up2.as<char>() + up_from, L0.up_bytes - 16 - up_from, hipMemcpyHostToDevice, s));
	if (pool2 && n_pool2 > 0) HIP_TRY(hipMemcpyAsync(din2 + L.off_pool2, pool2, (size_t)n_pool2 * 4, hipMemcpyHostToDevice, s));
	const char *din = ctx->spans.sp_in.as<char>();
	AsmArgs a;
	a.plan = (const SpansPlan*)(din + ctx->spans.sp_keep.off_plan), a.rec = (const SpanRec*)(ctx->spans.sp_out.as<char>() + SPANS_HEAD_BYTES), a.n_plan = (int32_t)n_plan;
	a.gap = (const SegRec*)(din + ctx->spans.sp_keep.off_seg), a.rst1 = (const mpa_dp_rst_t*)(din + ctx->spans.sp_keep.off_rst1), a.rst2 = d_rst2 ? d_rst2 : (const mpa_dp_rst_t*)din2;
	a.pool1 = ctx->spans.sp_pool1.as<uint32_t>(), a.pool2 = pool2 ? (const uint32_t*)(din2 + L.off_pool2) : ctx->round.cigd.as<uint32_t>();
	a.slot_off = (const int64_t*)(din2 + L.off_slot), a.cig = ctx->spans.sp_cig.as<uint32_t>(), a.out = ctx->spans.sp_asm.as<AsmRec>();
	hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n_plan + STATS_WAVES - 1) / STATS_WAVES)), dim3(64 * STATS_WAVES), 0, s, a);
	HIP_TRY(hipGetLastError());
	char *hd = ctx->spans.h_sp_down2.as<char>();
	HIP_TRY(hipMemcpyAsync(hd, ctx->spans.sp_asm.p, (size_t)n_plan * sizeof(AsmRec), hipMemcpyDeviceToHost, s));
	if (n_words > 0) HIP_TRY(hipMemcpyAsync(hd + L.rec_bytes, ctx->spans.sp_cig.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	io.rec = (const AsmRec*)hd, io.cigar = (const uint32_t*)(hd + L.rec_bytes);
	return MPA_OK;
}

// the bounds of a task list that is on the device, by the kernel dev_spans_round1 launches for MPA_GPU_ROUND2 (the hook's way to it)
int dev_task_bounds(mpa_ctx_t *ctx, const mpa_dp_task_t *d_tasks, int64_t n, DpResidentIn &out)
{
	out = DpResidentIn();
	if (n <= 0 || n > (int64_t)1 << 28) { set_error("dev_task_bounds: no tasks, or too many for one launch"); return MPA_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (ctx->spans.sp_mid.ensure(64) != MPA_OK) return MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	int64_t h[4] = { 0, 0, 0, 0 };                       // bounds[3] | the count
	*(int32_t*)(h + 3) = (int32_t)n;
	HIP_TRY(hipMemcpyAsync(ctx->spans.sp_mid.p, h, sizeof h, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_task_bounds, dim3((unsigned)((n + SPANS_BLOCK - 1) / SPANS_BLOCK)), dim3(SPANS_BLOCK), 0, s, d_tasks, (const int32_t*)(ctx->spans.sp_mid.as<int64_t>() + 3), ctx->spans.sp_mid.as<int64_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, ctx->spans.sp_mid.p, 24, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	out.d_tasks = d_tasks, out.prep_bound = h[0], out.max_nl = h[1], out.max_al = h[2];
	return MPA_OK;
}

} // namespace mpa
