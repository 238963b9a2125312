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
// host step between the DP rounds and the one behind them here: dev_spans_stage() / dev_spans_round1() (MPA_GPU_ROUND1=1, section 4.15: the
// dev_spans_chain_*() parts of it, behind a resident round 1 inside that round's wait) and dev_spans_asm_stage() /
// dev_spans_assemble().  The CIGAR pool k_assemble writes (sp_cig) stays on the device until the context's next call, and
// dev_aln_walks() reads it in place of an uploaded one when the caller says so (dev_cig).
// MPA_GPU_FINISH=1 (kernels k_finish_rank, k_finish_scan, k_finish_gather: finish_kernels.hip; code: finish_core.h; DESIGN.md section
// 4.13) puts the final ranking of the batch's aligned regions and the layout of its flat result here: dev_finish_stage() / dev_finish().
// MPA_GPU_FORMAT (kernels k_format_size, k_format_scan, k_format_write: format_kernels.hip; code: format_core.h)
// writes the output text of a flat result: dev_format_stage() / dev_format().
#include "dev_ctx.h"
#include "spans_core.h"
#include "dp_results_core.h"
#include "stats_kernels.hip"
#include "span_kernels.hip"
#include "finish_kernels.hip"
#include "format_kernels.hip"

namespace mpa {

// (the layouts of the blocks: StatsLayout, SpansLayout, AsmLayout, FinishLayout, FormatLayout in dev_layout.h)

// the finish step's parts (below), which dev_aln_walks runs behind its own kernels
struct FinishSrc { const uint32_t *words; const void *feats; const char *cs_text, *rows_text; const AlnStatsOut *st; const AlnCsOut *cs; const AlnRowsOut *rows; int32_t show_trans; };
static int finish_prepare(mpa_ctx_t *ctx, const FinishSizes &z);
static int finish_launch(mpa_ctx_t *ctx, const FinParams &p, const FinishSizes &z, const FinishSrc *src);
static int finish_collect(mpa_ctx_t *ctx, const FinishSizes &z, int64_t waits, FinishFlat &flat);
// ... and the format step's (further below), behind the finish step's in the same call
static int format_prepare(mpa_ctx_t *ctx, const FormatSizes &z);
static int format_launch(mpa_ctx_t *ctx, const FmtOpt &o, const FormatSizes &z, const FinishSizes *fin, const FinishSrc *src);
static int format_collect(mpa_ctx_t *ctx, const FormatSizes &z, int64_t waits, FormatOut &out);

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
	io.jobs = L.jobs.in(hu), io.cigar = L.cig.in(hu), io.text = L.text.in(hu);
	if (z.slot_bytes >= 0) cs.slot_off = L.slot.in(hu);
	if (z.rows_bytes >= 0) rows.slot_off = L.rslot.in(hu);
	return MPA_OK;
}

// The walks asked for over the z.n_jobs alignments staged in io / cs / rows, on ctx: the tables into the staged block, one upload, the
// launches (statistics: k_aln_stats; cs: k_aln_cs; rows: k_aln_rows), their downloads and one wait.  Afterwards io.out / io.feat hold
// the statistics, cs.out[j].len bytes lie at cs.body + cs.slot_off[j], and rows.out[j] describes the slot at rows.body +
// rows.slot_off[j] as aln_rows_core.h lays it out -- all of it pinned memory of the context, valid until its next call.
// MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller keeps the host's walks.
int dev_aln_walks(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const AlnRowsParams &rp, const int8_t *mat, const AlnWalkSizes &z, AlnStatsIO &io, AlnCsIO &cs,
                  AlnRowsIO &rows, bool dev_cig, FinishResident *fin, FormatResident *fmt)
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
	// (MPA_GPU_FINISH=1) ranking and flat result behind the walks' kernels, in front of the call's one wait: what the walks leave is
	// read where it lies and is not downloaded.  Whatever can decline does so here, before anything is launched
	if (fin && !stats) { set_error("dev_aln_walks: the finish step needs the statistics in the same call"); return MPA_ERR_ARG; }
	if (fin) { const int rc = finish_prepare(ctx, fin->z); if (rc != MPA_OK) return rc; }
	if (fmt && !fin) { set_error("dev_aln_walks: the format step needs the finish step in the same call"); return MPA_ERR_ARG; }
	if (fmt) { const int rc = format_prepare(ctx, fmt->z); if (rc != MPA_OK) return rc; }
	const int64_t waits0 = ctx->n_waits.load();
	hipStream_t s = ctx->stream;
	char *hu = ctx->walks.h_stats_up.as<char>();
	aln_tables_fill(L.tabs.in(hu), mat, (size_t)(p.asize * p.asize));
	HIP_TRY(hipMemcpyAsync(ctx->walks.st_in.p, hu, L.up_bytes - 16, hipMemcpyHostToDevice, s));
	const char *din = ctx->walks.st_in.as<char>();
	const uint8_t *dtext = (const uint8_t*)L.text.in(din);
	const uint32_t *dcig = dev_cig ? ctx->spans.sp_cig.as<uint32_t>() : L.cig.in(din);   // (MPA_GPU_SPANS=1: where k_assemble left the words)
	const unsigned nwg = (unsigned)((n_jobs + STATS_WAVES - 1) / STATS_WAVES);
	if (stats) {
		char *dout = ctx->walks.st_out.as<char>();
		hipLaunchKernelGGL(k_aln_stats, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, L.jobs.in(din), (int32_t)n_jobs, L.tabs.in(din), p,
		                   dtext, dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   L.out.in(dout), L.feat.in(dout));
		HIP_TRY(hipGetLastError());
		const char *hd = ctx->walks.h_stats_down.as<char>();
		if (!fin) HIP_TRY(hipMemcpyAsync(ctx->walks.h_stats_down.p, dout, L.down_bytes - 16, hipMemcpyDeviceToHost, s));
		io.out = L.out.in(hd), io.feat = L.feat.in(hd);
	}
	if (cs_on) {
		char *dout = ctx->walks.cs_out.as<char>();
		hipLaunchKernelGGL(k_aln_cs, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, L.jobs.in(din), (int32_t)n_jobs, L.tabs.in(din),
		                   dtext, dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   L.slot.in(din), L.cs_out.in(dout), L.body.in(dout));
		HIP_TRY(hipGetLastError());
		const char *hd = ctx->walks.h_cs_down.as<char>();
		if (!fin) HIP_TRY(hipMemcpyAsync(ctx->walks.h_cs_down.p, dout, L.cs_down_bytes - 16, hipMemcpyDeviceToHost, s));
		cs.out = L.cs_out.in(hd), cs.body = L.body.in(hd);
	}
	if (rows_on) {
		char *dout = ctx->walks.rows_out.as<char>();
		hipLaunchKernelGGL(k_aln_rows, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, L.jobs.in(din), (int32_t)n_jobs, L.tabs.in(din), rp,
		                   dtext, dcig, (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   L.rslot.in(din), L.rows_out.in(dout), L.rbody.in(dout));
		HIP_TRY(hipGetLastError());
		const char *hd = ctx->walks.h_rows_down.as<char>();
		if (!fin) HIP_TRY(hipMemcpyAsync(ctx->walks.h_rows_down.p, dout, L.rows_down_bytes - 16, hipMemcpyDeviceToHost, s));
		rows.out = L.rows_out.in(hd), rows.body = L.rbody.in(hd);
	}
	if (fin) {
		const char *d_st = ctx->walks.st_out.as<char>(), *d_cs = cs_on ? ctx->walks.cs_out.as<char>() : nullptr, *d_rows = rows_on ? ctx->walks.rows_out.as<char>() : nullptr;
		const FinishSrc src{ dcig, (const void*)L.feat.in(d_st), cs_on ? L.body.in(d_cs) : nullptr, rows_on ? L.rbody.in(d_rows) : nullptr, L.out.in(d_st),
		                     cs_on ? L.cs_out.in(d_cs) : nullptr, rows_on ? L.rows_out.in(d_rows) : nullptr, rp.show_trans };
		int rc = finish_launch(ctx, fin->p, fin->z, &src);
		if (rc != MPA_OK) return rc;
		if (fmt && (rc = format_launch(ctx, fmt->o, fmt->z, &fin->z, &src)) != MPA_OK) return rc;   // (MPA_GPU_FORMAT=1) the text, behind the gather
		io.out = nullptr, io.feat = nullptr, cs.out = nullptr, cs.body = nullptr, rows.out = nullptr, rows.body = nullptr;   // (not downloaded)
	}
	HIP_TRY(wait_stream(ctx, s));
	if (fmt) { fmt->out = FormatOut(); const int rc = format_collect(ctx, fmt->z, ctx->n_waits.load() - waits0, fmt->out); if (rc != MPA_OK) return rc; }
	if (fin) return finish_collect(ctx, fin->z, ctx->n_waits.load() - waits0, fin->flat);
	return MPA_OK;
}

// ---- MPA_GPU_SPANS=1 ------------------------------------------------------------------------------------------------------------
static size_t spans_blocks(int64_t n_plan) { return (size_t)((n_plan + SPANS_BLOCK - 1) / SPANS_BLOCK); }   // workgroups of k_spans / k_spans_emit

int dev_spans_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes, SpansIO &io)
{
	io = SpansIO();
	if (n_plan <= 0 || n_plan > (int64_t)1 << 28 || n_seg < 0 || n_rst1 <= 0) { set_error("GPU spans: no plans, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const SpansLayout L(n_plan, n_seg, n_rst1, text_bytes, spans_blocks(n_plan));
	if (ctx->spans.h_sp_up.ensure(L.up_bytes) != MPA_OK || ctx->spans.h_sp_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->spans.h_sp_up.as<char>();
	io.plan = L.plan.in(hu), io.seg = L.seg.in(hu), io.rst1 = L.rst1.in(hu), io.text = L.text.in(hu);
	return MPA_OK;
}

// The three parts of the step between the rounds, as for the finish step.  spans_prepare: the pools sized, the tables filled and the staged
// block sent up -- everything that can decline, before anything is launched (with_rst1 false: the round-1 records are written on the
// device behind it, so their section of the block stays out of the upload, which is then the two pieces around it).  spans_launch: k_spans,
// k_spans_emit and, with MPA_GPU_ROUND2=1, k_task_bounds on the context's stream, then the step's download; it does not wait.
// spans_collect, behind the caller's wait: the task count checked, io filled, what dev_spans_assemble reads kept.
static SpansLayout spans_layout(const SpansChain &c) { return SpansLayout(c.n_plan, c.n_seg, c.n_rst1, c.text_bytes, spans_blocks(c.n_plan)); }

static int spans_prepare(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, int64_t pool_words, bool with_rst1, int64_t *bytes_up)
{
	ctx->spans.sp_keep.n_plan = -1;
	if (c.p.asize < 1 || c.p.asize * c.p.asize > 484) { set_error("GPU spans: a substitution matrix of more than 22 x 22"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	const SpansLayout L = spans_layout(c);
	if (L.up_bytes > ctx->spans.h_sp_up.cap || L.down_bytes > ctx->spans.h_sp_down.cap) { set_error("dev_spans_round1: the staging block was not sized for this call"); return MPA_ERR_ARG; }
	tl_alloc_failed = false;
	if (ctx->spans.sp_in.ensure(L.up_bytes) != MPA_OK || ctx->spans.sp_mid.ensure(L.mid_bytes) != MPA_OK || ctx->spans.sp_out.ensure(L.down_bytes) != MPA_OK ||
	    ctx->spans.sp_pool1.ensure((size_t)pool_words * 4 + 16) != MPA_OK)
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *hu = ctx->spans.h_sp_up.as<char>(), *din = ctx->spans.sp_in.as<char>();
	aln_tables_fill(L.tabs.in(hu), c.mat, (size_t)(c.p.asize * c.p.asize));
	if (with_rst1) {
		HIP_TRY(hipMemcpyAsync(din, hu, L.up_bytes - 16, hipMemcpyHostToDevice, s));
		if (bytes_up) *bytes_up = (int64_t)(L.up_bytes - 16);
	} else {                                             // tables | plans | gap segments, then the text: the records' section is the device's
		const size_t head = L.seg.end(), tail = L.text.bytes();
		HIP_TRY(hipMemcpyAsync(din, hu, head, hipMemcpyHostToDevice, s));
		if (tail) HIP_TRY(hipMemcpyAsync(din + L.text.off, hu + L.text.off, tail, hipMemcpyHostToDevice, s));
		if (bytes_up) *bytes_up = (int64_t)(head + tail);
	}
	return MPA_OK;
}

static int spans_launch(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, const int32_t *g_err, const int64_t *g_bad, int64_t *launches, int64_t *bytes_down)
{
	const DeviceIndex *d = mi->dev[ctx->device];
	const SpansLayout L = spans_layout(c);
	hipStream_t s = ctx->stream;
	const char *din = ctx->spans.sp_in.as<char>();
	char *mid = ctx->spans.sp_mid.as<char>(), *dout = ctx->spans.sp_out.as<char>();
	SpansArgs a;
	a.plan = L.plan.in(din), a.n_plan = (int32_t)c.n_plan, a.rst1 = L.rst1.in(din);
	a.text = (const uint8_t*)L.text.in(din), a.tabs = L.tabs.in(din), a.seq = (const uint8_t*)d->seq, a.ctg_off = d->ctg_off, a.ctg_len = d->ctg_len;
	a.p = c.p, a.rec = L.mid_rec.in(mid), a.tmp = L.tmp.in(mid), a.excl = L.excl.in(mid), a.bsum = L.bsum.in(mid);
	a.g_err = g_err, a.g_bad = g_bad;
	const dim3 grid((unsigned)L.bsum.n);
	hipLaunchKernelGGL(k_spans, grid, dim3(SPANS_BLOCK), 0, s, a);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_spans_emit, grid, dim3(SPANS_BLOCK), 0, s, a, L.n_task.in(dout), L.rec.in(dout), L.task.in(dout));
	HIP_TRY(hipGetLastError());
	int64_t n_launch = 2;
	if (c.want_r2) {                                     // (MPA_GPU_ROUND2=1) the bounds of the tasks just written, for the planner of round 2
		HIP_TRY(hipMemsetAsync(L.bounds.in(dout), 0, L.bounds.bytes(), s));
		hipLaunchKernelGGL(k_task_bounds, dim3((unsigned)((2 * c.n_plan + SPANS_BLOCK - 1) / SPANS_BLOCK)), dim3(SPANS_BLOCK), 0, s, (const mpa_dp_task_t*)L.task.in(dout), (const int32_t*)L.n_task.in(dout),
		                   L.bounds.in(dout), g_err, g_bad);
		HIP_TRY(hipGetLastError());
		++n_launch;
	}
	HIP_TRY(hipMemcpyAsync(ctx->spans.h_sp_down.p, dout, L.down_bytes - 16, hipMemcpyDeviceToHost, s));
	if (launches) *launches = n_launch;
	if (bytes_down) *bytes_down = (int64_t)(L.down_bytes - 16);
	return MPA_OK;
}

static int spans_collect(mpa_ctx_t *ctx, const SpansChain &c, int64_t n_pool1, SpansIO &io)
{
	const SpansLayout L = spans_layout(c);
	const char *hd = ctx->spans.h_sp_down.as<char>();
	char *dout = ctx->spans.sp_out.as<char>();
	io.n_task = *L.n_task.in(hd), io.rec = L.rec.in(hd), io.task = L.task.in(hd);
	io.r2 = DpResidentIn();
	if (c.want_r2) { const int64_t *bd = L.bounds.in(hd); io.r2.d_tasks = L.task.in(dout), io.r2.prep_bound = bd[0], io.r2.max_nl = bd[1], io.r2.max_al = bd[2]; }
	if (io.n_task < 0 || io.n_task > 2 * c.n_plan) { set_error("dev_spans_round1: an impossible task count"); return MPA_ERR_HIP; }
	ctx->spans.sp_keep = SpanBufs::SpansKeep{ L.plan, L.seg, L.rst1, L.rec, c.n_plan, n_pool1 };
	return MPA_OK;
}

int dev_spans_round1(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansParams &p, const int8_t *mat, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes,
                     const uint32_t *pool1, int64_t n_pool1, SpansIO &io)
{
	const SpansChain c{ p, mat, n_plan, n_seg, n_rst1, text_bytes, round2_knob() };
	ctx->spans.sp_keep.n_plan = -1;
	if (n_pool1 < 0 || (!pool1 && n_pool1 > 0 && (size_t)n_pool1 * 4 > ctx->round.cigd.cap)) { set_error("dev_spans_round1: no round-1 CIGAR pool of that size on this context"); return MPA_ERR_ARG; }
	int rc = spans_prepare(ctx, mi, c, n_pool1, true, nullptr);
	if (rc != MPA_OK) return rc;
	hipStream_t s = ctx->stream;
	// the round-1 pool stays: round 2 overwrites cigd
	if (n_pool1 > 0) HIP_TRY(hipMemcpyAsync(ctx->spans.sp_pool1.p, pool1 ? (const void*)pool1 : ctx->round.cigd.p, (size_t)n_pool1 * 4, pool1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
	if ((rc = spans_launch(ctx, mi, c, nullptr, nullptr, nullptr, nullptr)) != MPA_OK) return rc;
	HIP_TRY(wait_stream(ctx, s));
	return spans_collect(ctx, c, n_pool1, io);
}

// ---- MPA_GPU_ROUND1=1: the same step chained behind a resident round 1 (dp_exec.hip), inside the round's one wait.
// dev_spans_chain_prepare, before the round is launched: the block staged through dev_spans_stage goes up without its record section and
// sp_pool1 is sized at pool_words, the plan's bound of the dense pool; dev says where the round's kernels put records and words.
// dev_spans_chain_enqueue, behind the round's results kernels: the step's kernels under the guard (g_err, g_bad: the round's hand-off
// error word and the bad-call word of its results header) and its download.  dev_spans_chain_collect, behind the wait.
int dev_spans_chain_prepare(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, int64_t pool_words, SpansChainDev &dev)
{
	dev = SpansChainDev();
	if (c.n_plan <= 0 || c.n_rst1 <= 0 || pool_words < 0) { set_error("dev_spans_chain_prepare: no plans, no calls or a negative pool"); return MPA_ERR_ARG; }
	const int rc = spans_prepare(ctx, mi, c, pool_words, false, &dev.bytes_up);
	if (rc != MPA_OK) return rc;
	const SpansLayout L = spans_layout(c);
	dev.d_rst1 = L.rst1.in(ctx->spans.sp_in.as<char>()), dev.d_pool1 = ctx->spans.sp_pool1.as<uint32_t>();
	dev.block_bytes = (int64_t)(L.up_bytes - 16), dev.rst1_bytes = (int64_t)(L.text.off - L.seg.end());
	return MPA_OK;
}
int dev_spans_chain_enqueue(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, const int32_t *g_err, const int64_t *g_bad, int64_t *launches, int64_t *bytes_down)
{
	return spans_launch(ctx, mi, c, g_err, g_bad, launches, bytes_down);
}
int dev_spans_chain_collect(mpa_ctx_t *ctx, const SpansChain &c, int64_t n_pool1, SpansIO &io)
{
	if (n_pool1 < 0 || (size_t)n_pool1 * 4 > ctx->spans.sp_pool1.cap) { set_error("dev_spans_chain_collect: no round-1 CIGAR pool of that size on this context"); return MPA_ERR_ARG; }
	return spans_collect(ctx, c, n_pool1, io);
}
// (the hook mpa_dbg_spans_guard) the step on a staged block that holds its records, under guard words the caller chooses: err and bad go
// into a pool of the context and the kernels get pointers to them, as a chained step gets the round's.  No CIGAR pool is kept
int dev_spans_round1_guarded(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, int32_t err, int64_t bad, SpansIO &io)
{
	int rc = spans_prepare(ctx, mi, c, 0, true, nullptr);
	if (rc != MPA_OK) return rc;
	if (ctx->spans.sp_in2.ensure(64) != MPA_OK) return MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	Carve gc(8);                                         // the error word | the bad-call word
	const auto p_err = gc.take<int32_t>(1); const auto p_bad = gc.take<int64_t>(1);
	int64_t h[2] = { 0, 0 };
	*p_err.in(h) = err, *p_bad.in(h) = bad;
	HIP_TRY(hipMemcpyAsync(ctx->spans.sp_in2.p, h, sizeof h, hipMemcpyHostToDevice, s));
	if ((rc = spans_launch(ctx, mi, c, p_err.in((const void*)ctx->spans.sp_in2.p), p_bad.in((const void*)ctx->spans.sp_in2.p), nullptr, nullptr)) != MPA_OK) return rc;
	HIP_TRY(wait_stream(ctx, s));
	return spans_collect(ctx, c, 0, io);
}

int dev_spans_asm_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_rst2, SpansAsmIO &io)
{
	io = SpansAsmIO();
	if (n_plan <= 0 || n_plan != ctx->spans.sp_keep.n_plan || n_rst2 < 0) { set_error("GPU spans: the plans of this batch are not on the device"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const AsmLayout L(n_plan, n_rst2, 0);
	if (ctx->spans.h_sp_up2.ensure(L.up_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->spans.h_sp_up2.as<char>();
	io.rst2 = L.rst2.in(hu), io.slot_off = L.slot.in(hu);
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
	const Piece<uint32_t> h_cig = L.cigar((size_t)n_words);
	const size_t down_bytes = h_cig.end() + 16;
	if (ctx->spans.h_sp_down2.ensure(down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	tl_alloc_failed = false;
	if (ctx->spans.sp_in2.ensure(L.up_bytes) != MPA_OK || ctx->spans.sp_asm.ensure(L.rec_bytes + 16) != MPA_OK || ctx->spans.sp_cig.ensure((size_t)n_words * 4 + 16) != MPA_OK)
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *din2 = ctx->spans.sp_in2.as<char>();
	// (d_rst2: round 2's records are on the device already, where the round's own kernels wrote them -- only the slot offsets go up)
	const size_t up_from = d_rst2 ? L0.slot.off : 0;
	HIP_TRY(hipMemcpyAsync(din2 + up_from, ctx->spans.h_sp_up2.as<char>() + up_from, L0.up_bytes - 16 - up_from, hipMemcpyHostToDevice, s));
	if (pool2 && n_pool2 > 0) HIP_TRY(hipMemcpyAsync(L.pool2.in(din2), pool2, (size_t)n_pool2 * 4, hipMemcpyHostToDevice, s));
	const char *din = ctx->spans.sp_in.as<char>(), *in2 = din2, *dout1 = ctx->spans.sp_out.as<char>();
	AsmArgs a;
	const SpanBufs::SpansKeep &K = ctx->spans.sp_keep;       // (what dev_spans_round1 left in sp_in and sp_out)
	a.plan = K.plan.in(din), a.rec = K.rec.in(dout1), a.n_plan = (int32_t)n_plan;
	a.gap = K.seg.in(din), a.rst1 = K.rst1.in(din), a.rst2 = d_rst2 ? d_rst2 : L.rst2.in(in2);
	a.pool1 = ctx->spans.sp_pool1.as<uint32_t>(), a.pool2 = pool2 ? L.pool2.in(in2) : ctx->round.cigd.as<uint32_t>();
	a.slot_off = L.slot.in(in2), a.cig = ctx->spans.sp_cig.as<uint32_t>(), a.out = ctx->spans.sp_asm.as<AsmRec>();
	hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n_plan + STATS_WAVES - 1) / STATS_WAVES)), dim3(64 * STATS_WAVES), 0, s, a);
	HIP_TRY(hipGetLastError());
	char *hd = ctx->spans.h_sp_down2.as<char>();
	HIP_TRY(hipMemcpyAsync(L.rec.in(hd), ctx->spans.sp_asm.p, L.rec.bytes(), hipMemcpyDeviceToHost, s));
	if (n_words > 0) HIP_TRY(hipMemcpyAsync(h_cig.in(hd), ctx->spans.sp_cig.p, h_cig.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	io.rec = L.rec.in(hd), io.cigar = h_cig.in(hd);
	return MPA_OK;
}

// ---- MPA_GPU_FINISH=1 -----------------------------------------------------------------------------------------------------------
static bool finish_sizes_ok(const FinishSizes &z)
{
	const int64_t lim = (int64_t)1 << 40;
	return z.n_query > 0 && z.n_query < INT32_MAX && z.n_rec > 0 && z.n_rec <= (int64_t)1 << 28 && z.n_big >= 0 && z.n_big <= z.n_query && z.in_words >= 0 && z.in_words < lim && z.in_feat >= 0 &&
	       z.in_feat < lim && z.in_cs >= 0 && z.in_cs < lim && z.in_rows >= 0 && z.in_rows < lim && z.out_words >= 0 && z.out_words < lim && z.out_feat >= 0 && z.out_feat < lim && z.out_cs >= 0 &&
	       z.out_cs < lim && z.out_rows >= 0 && z.out_rows < lim;
}

int dev_finish_stage(mpa_ctx_t *ctx, const FinishSizes &z, FinishTables &t)
{
	t = FinishTables();
	if (!finish_sizes_ok(z)) { set_error("GPU finish: no aligned regions, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const FinishLayout L(z);
	if (ctx->finish.h_fin_up.ensure(L.up_bytes) != MPA_OK || ctx->finish.h_fin_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->finish.h_fin_up.as<char>();
	t.first = L.first.in(hu), t.rec = L.rec.in(hu), t.words = L.words.in(hu), t.feats = L.in_feat.in(hu), t.cs_text = L.in_cs.in(hu), t.rows_text = L.in_rows.in(hu);
	return MPA_OK;
}

// The three parts of a call.  finish_prepare: the staged first[] checked, the large queries numbered, the pools sized -- everything that
// can decline, before anything is launched.  finish_launch: the staged block up (behind the walks only first | big | records: `src` says
// where the walks left the rest, and k_finish_fill completes the records from their out records), then rank, scan and gather on the
// context's stream; scan and gather write the pinned block directly.  finish_collect, behind the caller's wait: the flat arrays.

static int finish_prepare(mpa_ctx_t *ctx, const FinishSizes &z)
{
	if (!finish_sizes_ok(z)) { set_error("dev_finish: no aligned regions, or too many for one launch"); return MPA_ERR_ARG; }
	const FinishLayout L(z);
	if (L.up_bytes > ctx->finish.h_fin_up.cap || L.down_bytes > ctx->finish.h_fin_down.cap) { set_error("dev_finish: the staging block was not sized for this call"); return MPA_ERR_ARG; }
	char *hu = ctx->finish.h_fin_up.as<char>();
	const int64_t *first = L.first.in(hu);
	int32_t *big = L.big.in(hu);
	int64_t nb = 0;
	if (first[0] != 0 || first[z.n_query] != z.n_rec) { set_error("dev_finish: first[] does not span the records"); return MPA_ERR_ARG; }
	for (int64_t q = 0; q < z.n_query; ++q) {
		const int64_t n = first[q + 1] - first[q];
		if (n < 0 || n > INT32_MAX) { set_error("dev_finish: first[] is not ascending"); return MPA_ERR_ARG; }
		big[q] = n > FINISH_LDS_REGS ? (int32_t)nb++ : -1;
	}
	if (nb != z.n_big) { set_error("dev_finish: n_big is not the number of large queries"); return MPA_ERR_ARG; }
	tl_alloc_failed = false;
	if (ctx->finish.fin_in.ensure(L.up_bytes) != MPA_OK || ctx->finish.fin_mid.ensure(L.mid_bytes) != MPA_OK) return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	return MPA_OK;
}

static int finish_launch(mpa_ctx_t *ctx, const FinParams &p, const FinishSizes &z, const FinishSrc *src)
{
	const FinishLayout L(z);
	hipStream_t s = ctx->stream;
	char *din = ctx->finish.fin_in.as<char>(), *mid = ctx->finish.fin_mid.as<char>(), *hd = ctx->finish.h_fin_down.as<char>();
	HIP_TRY(hipMemcpyAsync(din, ctx->finish.h_fin_up.p, src ? L.rec.end() : L.up_bytes - 16, hipMemcpyHostToDevice, s));
	if (src) {
		hipLaunchKernelGGL(k_finish_fill, dim3((unsigned)((z.n_rec + 255) / 256)), dim3(256), 0, s, L.rec.in(din), z.n_rec, src->st, src->cs, src->rows, src->show_trans);
		HIP_TRY(hipGetLastError());
	}
	FinishArgs a;
	a.first = L.first.in(din), a.rec = L.rec.in(din), a.big = L.big.in(din), a.p = p, a.out = L.out.in(mid), a.cnt = L.cnt.in(mid), a.off = L.off.in(mid);
	a.tmp = L.tmp.in(mid), a.r = L.r.in(mid), a.key = L.key.in(mid), a.stack = L.stack.in(mid), a.hist = L.hist.in(mid), a.prim = L.prim.in(mid), a.ctl = L.ctl.in(mid), a.cov = L.cov.in(mid);
	// (pinned host memory, written by the kernels: what the result holds is what crosses the bus)
	const FinDst dst{ L.hits.in(hd), L.cigars.in(hd), L.feats.in(hd), L.cs.in(hd), L.cs_text.in(hd), L.rows.in(hd), L.rows_text.in(hd) };
	const int32_t nq = (int32_t)z.n_query;
	hipLaunchKernelGGL(k_finish_rank, dim3((unsigned)nq), dim3(64), 0, s, a, nq);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_finish_scan, dim3(1), dim3(FINISH_SCAN), 0, s, (const FinCounts*)a.cnt, nq, a.off, L.h_off.in(hd));
	HIP_TRY(hipGetLastError());
	if (src) hipLaunchKernelGGL(k_finish_gather, dim3((unsigned)nq), dim3(64 * FINISH_GATHER_WAVES), 0, s, a, nq, src->words, src->feats, src->cs_text, src->rows_text, dst);
	else hipLaunchKernelGGL(k_finish_gather, dim3((unsigned)nq), dim3(64 * FINISH_GATHER_WAVES), 0, s, a, nq, (const uint32_t*)L.words.in(din), (const void*)L.in_feat.in(din), (const char*)L.in_cs.in(din), (const char*)L.in_rows.in(din), dst);
	HIP_TRY(hipGetLastError());
	return MPA_OK;
}

static int finish_collect(mpa_ctx_t *ctx, const FinishSizes &z, int64_t waits, FinishFlat &flat)
{
	const FinishLayout L(z);
	const char *hd = ctx->finish.h_fin_down.as<char>();
	flat.off = L.h_off.in(hd), flat.hits = L.hits.in(hd), flat.cs = L.cs.in(hd), flat.rows = L.rows.in(hd), flat.cigars = L.cigars.in(hd), flat.feats = L.feats.in(hd);
	flat.cs_text = L.cs_text.in(hd), flat.rows_text = L.rows_text.in(hd);
	const FinCounts &tot = flat.off[z.n_query];
	if (tot.hit < 0 || tot.hit > z.n_rec || tot.cigar < 0 || tot.cigar > z.out_words || tot.feat < 0 || tot.feat > z.out_feat || tot.cs < 0 || tot.cs > z.out_cs || tot.rows < 0 || tot.rows > z.out_rows) {
		set_error("dev_finish: impossible counts");
		return MPA_ERR_HIP;
	}
	// what the kernels wrote into the pinned block: the prefix, a hit record and two references per hit, and the dense arrays at their real length
	flat.bytes_down = (int64_t)L.h_off.bytes() + tot.hit * (int64_t)(sizeof(mpa_hit_t) + sizeof(FinCsRef) + sizeof(FinRowsRef)) + 4 * tot.cigar + (int64_t)sizeof(mpa_feat_t) * tot.feat + tot.cs + tot.rows;
	int64_t *last = ctx->finish.last;
	last[0] = z.n_query, last[1] = z.n_rec, last[2] = tot.hit, last[3] = flat.bytes_down, last[4] = z.n_big, last[5] = waits;
	return MPA_OK;
}

int dev_finish(mpa_ctx_t *ctx, const FinParams &p, const FinishSizes &z, FinishFlat &flat)
{
	flat = FinishFlat();
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = finish_prepare(ctx, z);
	if (rc != MPA_OK) return rc;
	const int64_t waits0 = ctx->n_waits.load();
	if ((rc = finish_launch(ctx, p, z, nullptr)) != MPA_OK) return rc;
	HIP_TRY(wait_stream(ctx, ctx->stream));
	return finish_collect(ctx, z, ctx->n_waits.load() - waits0, flat);
}

int dev_finish_last(const mpa_ctx_t *ctx, int64_t out[6])
{
	if (!ctx || !out) { set_error("dev_finish_last: missing arguments"); return MPA_ERR_ARG; }
	for (int k = 0; k < 6; ++k) out[k] = ctx->finish.last[k];
	return MPA_OK;
}

// ---- MPA_GPU_FORMAT -------------------------------------------------------------------------------------------------------------
static bool format_sizes_ok(const FormatSizes &z)
{
	const int64_t lim = (int64_t)1 << 40;
	return z.n_query > 0 && z.n_query < INT32_MAX && z.n_hit >= 0 && z.n_hit <= (int64_t)1 << 28 && z.n_words >= 0 && z.n_words < lim && z.n_feat >= 0 && z.n_feat < lim && z.cs_bytes >= 0 &&
	       z.cs_bytes < lim && z.rows_bytes >= 0 && z.rows_bytes < lim && z.qname_bytes >= 0 && z.qname_bytes < lim && z.n_ctg > 0 && z.n_ctg < INT32_MAX && z.cname_bytes >= 0 &&
	       z.cname_bytes < lim && z.text_cap >= 0 && z.text_cap < lim && z.id_cap >= 0 && z.id_cap < lim && z.n_place >= 0 && z.n_place <= (int64_t)1 << 28;
}

int dev_format_stage(mpa_ctx_t *ctx, const FormatSizes &z, FormatTables &t)
{
	t = FormatTables();
	if (!format_sizes_ok(z)) { set_error("GPU format: no queries, or too many hits for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const FormatLayout L(z);
	if (ctx->format.h_fmt_up.ensure(L.up_bytes) != MPA_OK || ctx->format.h_fmt_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->format.h_fmt_up.as<char>();
	t.hit_off = L.hit_off.in(hu), t.q_off = L.q_off.in(hu), t.qname_off = L.qname_off.in(hu), t.cname_off = L.cname_off.in(hu), t.clen = L.clen.in(hu), t.hits = L.hits.in(hu);
	t.cs = z.has_cs ? L.cs.in(hu) : nullptr, t.rows = z.has_rows ? L.rows.in(hu) : nullptr, t.feats = L.feats.in(hu), t.cigars = L.cigars.in(hu);
	t.cs_text = L.cs_text.in(hu), t.rows_text = L.rows_text.in(hu), t.qname = L.qname.in(hu), t.cname = L.cname.in(hu);
	return MPA_OK;
}

// The three parts of a call, as for the finish step.  format_prepare: the pools sized -- what can decline, before anything is launched.
// format_launch: the staged block up, then size, scan and write on the context's stream; scan and write store into the pinned block.
// `fin` (inside dev_aln_walks): the hits are read where the finish step of the same call left them, and only the names went up.
// format_collect, behind the caller's wait: the totals, and whether the kernels wrote the text.
static int format_prepare(mpa_ctx_t *ctx, const FormatSizes &z)
{
	if (!format_sizes_ok(z)) { set_error("dev_format: no queries, or too many hits for one launch"); return MPA_ERR_ARG; }
	const FormatLayout L(z);
	if (L.up_bytes > ctx->format.h_fmt_up.cap || L.down_bytes > ctx->format.h_fmt_down.cap) { set_error("dev_format: the staging block was not sized for this call"); return MPA_ERR_ARG; }
	tl_alloc_failed = false;
	if (ctx->format.fmt_in.ensure(L.up_bytes) != MPA_OK || ctx->format.fmt_mid.ensure(L.mid_bytes) != MPA_OK) return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	return MPA_OK;
}

static int format_launch(mpa_ctx_t *ctx, const FmtOpt &o, const FormatSizes &z, const FinishSizes *fin, const FinishSrc *src)
{
	const FormatLayout L(z);
	hipStream_t s = ctx->stream;
	char *din = ctx->format.fmt_in.as<char>(), *mid = ctx->format.fmt_mid.as<char>(), *hd = ctx->format.h_fmt_down.as<char>();
	*L.head.in(hd) = FmtCounts{ 0, 0, 0, -1 };           // (what the host reads if the scan never ran)
	HIP_TRY(hipMemcpyAsync(din, ctx->format.h_fmt_up.p, L.up_bytes - 16, hipMemcpyHostToDevice, s));
	FmtSrc S;
	S.hits = L.hits.in(din), S.hit_off = L.hit_off.in(din), S.cigars = L.cigars.in(din), S.feats = L.feats.in(din);
	S.cs = z.has_cs ? L.cs.in(din) : nullptr, S.cs_text = L.cs_text.in(din), S.rows = z.has_rows ? L.rows.in(din) : nullptr, S.rows_text = L.rows_text.in(din);
	S.q_off = L.q_off.in(din), S.qname = L.qname.in(din), S.qname_off = L.qname_off.in(din), S.cname = L.cname.in(din), S.cname_off = L.cname_off.in(din), S.clen = L.clen.in(din);
	if (fin) {                                           // (what finish_launch set up in fin_in / fin_mid, and what the walks left)
		const FinishLayout F(*fin);
		const char *fin_in = ctx->finish.fin_in.as<char>(), *fin_mid = ctx->finish.fin_mid.as<char>();
		S.hits = nullptr, S.hit_off = nullptr, S.cs = nullptr, S.rows = nullptr;
		S.rec = F.rec.in(fin_in), S.first = F.first.in(fin_in), S.out = F.out.in(fin_mid), S.fin_off = F.off.in(fin_mid);
		S.cigars = src->words, S.feats = (const mpa_feat_t*)src->feats, S.cs_text = src->cs_text, S.rows_text = src->rows_text;
	}
	const int32_t nq = (int32_t)z.n_query;
	hipLaunchKernelGGL(k_format_size, dim3((unsigned)nq), dim3(64), 0, s, o, S, nq, L.at.in(mid), L.cnt.in(mid));
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_format_scan, dim3(1), dim3(FORMAT_SCAN), 0, s, (const FmtCounts*)L.cnt.in(mid), nq, L.off.in(mid), L.head.in(hd));
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_format_write, dim3((unsigned)nq), dim3(64 * FORMAT_WRITE_WAVES), 0, s, o, S, nq, (const FmtAt*)L.at.in(mid), (const FmtCounts*)L.off.in(mid), L.text.in(hd), z.text_cap,
	                   L.id_at.in(hd), z.id_cap);
	HIP_TRY(hipGetLastError());
	return MPA_OK;
}

static int format_collect(mpa_ctx_t *ctx, const FormatSizes &z, int64_t waits, FormatOut &out)
{
	const FormatLayout L(z);
	const char *hd = ctx->format.h_fmt_down.as<char>();
	out.tot = *L.head.in(hd);
	if (out.tot.bad < 0 || out.tot.bytes < 0 || out.tot.ids < 0 || out.tot.n_out < 0 || out.tot.n_out > z.n_place) { set_error("dev_format: impossible counts"); return MPA_ERR_HIP; }
	out.declined = format_decline_reason(out.tot, z.text_cap, z.id_cap) != nullptr;
	out.text = L.text.in(hd), out.id_at = L.id_at.in(hd);
	int64_t *last = ctx->format.last;
	last[0] = z.n_query, last[1] = out.tot.n_out, last[2] = out.tot.bytes, last[3] = out.tot.ids, last[4] = waits, last[5] = out.declined;
	return MPA_OK;
}

int dev_format(mpa_ctx_t *ctx, const FmtOpt &o, const FormatSizes &z, FormatOut &out)
{
	out = FormatOut();
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = format_prepare(ctx, z);
	if (rc != MPA_OK) return rc;
	const int64_t waits0 = ctx->n_waits.load();
	if ((rc = format_launch(ctx, o, z, nullptr, nullptr)) != MPA_OK) return rc;
	HIP_TRY(wait_stream(ctx, ctx->stream));
	return format_collect(ctx, z, ctx->n_waits.load() - waits0, out);
}

int dev_format_last(const mpa_ctx_t *ctx, int64_t out[6])
{
	if (!ctx || !out) { set_error("dev_format_last: missing arguments"); return MPA_ERR_ARG; }
	for (int k = 0; k < 6; ++k) out[k] = ctx->format.last[k];
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
	Carve hc(8);                                         // bounds[3] | the count
	const auto p_bounds = hc.take<int64_t>(3); const auto p_n = hc.take<int32_t>(1);
	int64_t h[4] = { 0, 0, 0, 0 };
	*p_n.in(h) = (int32_t)n;
	HIP_TRY(hipMemcpyAsync(ctx->spans.sp_mid.p, h, sizeof h, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_task_bounds, dim3((unsigned)((n + SPANS_BLOCK - 1) / SPANS_BLOCK)), dim3(SPANS_BLOCK), 0, s, d_tasks, (const int32_t*)p_n.in(ctx->spans.sp_mid.p), p_bounds.in(ctx->spans.sp_mid.p), (const int32_t*)nullptr, (const int64_t*)nullptr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, ctx->spans.sp_mid.p, p_bounds.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	out.d_tasks = d_tasks, out.prep_bound = h[0], out.max_nl = h[1], out.max_al = h[2];
	return MPA_OK;
}

} // namespace mpa
