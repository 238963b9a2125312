// stats_run.hip -- the device unit of the alignment statistics (MPA_GPU_STATS=1; kernel: stats_kernels.hip, code: aln_stats_core.h).
// take_round3() of host_map.cpp fills one pinned block (tables | jobs | CIGAR words | the batch's protein text) through
// dev_aln_stats_stage(), dev_aln_stats() sends it up, launches k_aln_stats on the context that ran the batch's DP rounds, takes one
// pinned block down (per-alignment records | features) and waits once.  The pools (st_in, st_out and their staging) are grow-only and
// allocated on first use: a run that never sets the knob holds none of them.
// MPA_GPU_CS=1 (kernel k_aln_cs, code: aln_cs_core.h) goes the same way through dev_aln_walks_stage() / dev_aln_walks():
// the block that goes up gains the slot offsets (tables | jobs | slot offsets | CIGAR words | protein text), one more pinned block
// comes down (lengths | slots: cs_out and its staging), and when the statistics run on the device too the two kernels share the
// upload and the wait.
// MPA_GPU_ROWS=1 (kernel k_aln_rows, code: aln_rows_core.h) is the third of the kind: dev_aln_walks_stage() /
// dev_aln_walks() take any of statistics, cs strings and residue rows in one call -- one upload (tables | jobs | cs slot offsets | rows
// slot offsets | CIGAR words | protein text), up to three launches, one pinned block down each, one wait.  The rows' block (records |
// slots: rows_out and its staging) is allocated by the first call that asks for rows.
#include "dev_ctx.h"
#include "stats_kernels.hip"

namespace mpa {

namespace {
struct StatsLayout {
	size_t off_jobs, off_slot, off_rslot, off_cig, off_text, up_bytes, off_feat, down_bytes, off_body, cs_down_bytes, off_rbody, rows_down_bytes;
	// slot_bytes < 0: no cs strings; rows_bytes < 0: no residue rows (the block that goes up is then what it was without them)
	StatsLayout(int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat, int64_t slot_bytes = -1, int64_t rows_bytes = -1)
	{
		auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
		off_jobs = 1024;                                                   // (the tables take ALN_TAB_BYTES of the first KB)
		off_slot = off_jobs + up16((size_t)n_jobs * sizeof(AlnStatsJob));
		off_rslot = off_slot + (slot_bytes >= 0 ? up16((size_t)(n_jobs + 1) * 8) : 0);
		off_cig = off_rslot + (rows_bytes >= 0 ? up16((size_t)(n_jobs + 1) * 8) : 0);
		off_text = off_cig + up16((size_t)n_cigar * 4);
		up_bytes = off_text + up16((size_t)text_bytes) + 16;
		off_feat = up16((size_t)n_jobs * sizeof(AlnStatsOut));
		down_bytes = off_feat + (size_t)n_feat * sizeof(AlnFeat) + 16;
		off_body = up16((size_t)n_jobs * sizeof(AlnCsOut));
		cs_down_bytes = off_body + (size_t)(slot_bytes > 0 ? slot_bytes : 0) + 16;
		off_rbody = up16((size_t)n_jobs * sizeof(AlnRowsOut));
		rows_down_bytes = off_rbody + (size_t)(rows_bytes > 0 ? rows_bytes : 0) + 16;
	}
};
static_assert(ALN_TAB_BYTES <= 1024, "the tables share the first KB of the staging block");
}

// the pinned block of a call, for the caller to fill: jobs, CIGAR words and text.  MPA_ERR_UNSUPPORTED: no memory for it
int dev_aln_stats_stage(mpa_ctx_t *ctx, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat, AlnStatsIO &io)
{
	io = AlnStatsIO();
	if (n_jobs <= 0 || n_jobs > (int64_t)1 << 28) { set_error("GPU alignment statistics: no alignments, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const StatsLayout L(n_jobs, n_cigar, text_bytes, n_feat);
	if (ctx->h_stats_up.ensure(L.up_bytes) != MPA_OK || ctx->h_stats_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->h_stats_up.as<char>();
	io.jobs = (AlnStatsJob*)(hu + L.off_jobs), io.cigar = (uint32_t*)(hu + L.off_cig), io.text = hu + L.off_text;
	return MPA_OK;
}

// What dev_aln_stats() and dev_aln_walks() share: the tables into the staged block, one upload, the launches asked for (stats:
// k_aln_stats; cs: k_aln_cs; rows: k_aln_rows), their downloads and one wait.
static int stats_walks_run(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const int8_t *mat, int64_t n_jobs, const StatsLayout &L, bool stats, AlnStatsIO &io, AlnCsIO *cs,
                           const AlnRowsParams *rp = nullptr, AlnRowsIO *rows = nullptr)
{
	if (p.asize < 1 || p.asize * p.asize > 484) { set_error("GPU alignment statistics: a substitution matrix of more than 22 x 22"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	const DeviceIndex *d = mi->dev[ctx->device];
	if (L.up_bytes > ctx->h_stats_up.cap || (stats && L.down_bytes > ctx->h_stats_down.cap) || (cs && L.cs_down_bytes > ctx->h_cs_down.cap) ||
	    (rows && L.rows_down_bytes > ctx->h_rows_down.cap)) {
		set_error("dev_aln_stats: the staging block was not sized for this call");
		return MPA_ERR_ARG;
	}
	tl_alloc_failed = false;
	if (ctx->st_in.ensure(L.up_bytes) != MPA_OK || (stats && ctx->st_out.ensure(L.down_bytes) != MPA_OK) || (cs && ctx->cs_out.ensure(L.cs_down_bytes) != MPA_OK) ||
	    (rows && ctx->rows_out.ensure(L.rows_down_bytes) != MPA_OK))
		return tl_alloc_failed ? MPA_ERR_UNSUPPORTED : MPA_ERR_HIP;
	hipStream_t s = ctx->stream;
	char *hu = ctx->h_stats_up.as<char>();
	memcpy(hu + ALN_TAB_CODON, tab_codon(), 64);
	memcpy(hu + ALN_TAB_AA20, tab_aa20(), 256);
	memset(hu + ALN_TAB_MAT, 0, 484);
	memcpy(hu + ALN_TAB_MAT, mat, (size_t)(p.asize * p.asize));
	HIP_TRY(hipMemcpyAsync(ctx->st_in.p, hu, L.up_bytes - 16, hipMemcpyHostToDevice, s));
	const char *din = ctx->st_in.as<char>();
	const unsigned nwg = (unsigned)((n_jobs + STATS_WAVES - 1) / STATS_WAVES);
	if (stats) {
		char *dout = ctx->st_out.as<char>();
		hipLaunchKernelGGL(k_aln_stats, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din, p,
		                   (const uint8_t*)(din + L.off_text), (const uint32_t*)(din + L.off_cig), (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (AlnStatsOut*)dout, (AlnFeat*)(dout + L.off_feat));
		HIP_TRY(hipGetLastError());
		char *hd = ctx->h_stats_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.down_bytes - 16, hipMemcpyDeviceToHost, s));
		io.out = (const AlnStatsOut*)hd, io.feat = (const AlnFeat*)(hd + L.off_feat);
	}
	if (cs) {
		char *dout = ctx->cs_out.as<char>();
		hipLaunchKernelGGL(k_aln_cs, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din,
		                   (const uint8_t*)(din + L.off_text), (const uint32_t*)(din + L.off_cig), (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (const int64_t*)(din + L.off_slot), (AlnCsOut*)dout, dout + L.off_body);
		HIP_TRY(hipGetLastError());
		char *hd = ctx->h_cs_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.cs_down_bytes - 16, hipMemcpyDeviceToHost, s));
		cs->out = (const AlnCsOut*)hd, cs->body = hd + L.off_body;
	}
	if (rows) {
		char *dout = ctx->rows_out.as<char>();
		hipLaunchKernelGGL(k_aln_rows, dim3(nwg), dim3(64 * STATS_WAVES), 0, s, (const AlnStatsJob*)(din + L.off_jobs), (int32_t)n_jobs, (const uint8_t*)din, *rp,
		                   (const uint8_t*)(din + L.off_text), (const uint32_t*)(din + L.off_cig), (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len,
		                   (const int64_t*)(din + L.off_rslot), (AlnRowsOut*)dout, dout + L.off_rbody);
		HIP_TRY(hipGetLastError());
		char *hd = ctx->h_rows_down.as<char>();
		HIP_TRY(hipMemcpyAsync(hd, dout, L.rows_down_bytes - 16, hipMemcpyDeviceToHost, s));
		rows->out = (const AlnRowsOut*)hd, rows->body = hd + L.off_rbody;
	}
	HIP_TRY(wait_stream(ctx, s));
	return MPA_OK;
}

// The statistics and features of the n_jobs alignments staged in io, on ctx.  io.out / io.feat point into pinned memory of the
// context afterwards, valid until its next call.  MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller runs the host stage.
int dev_aln_stats(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const int8_t *mat, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat,
                  AlnStatsIO &io)
{
	return stats_walks_run(ctx, mi, p, mat, n_jobs, StatsLayout(n_jobs, n_cigar, text_bytes, n_feat), true, io, nullptr);
}

// The same for a call that writes cs strings, residue rows or both: slot_bytes = the sum of the alignments' aln_cs_bound() (< 0: no cs
// strings), rows_bytes = the sum of their aln_rows_slot() (< 0: no rows); cs.slot_off[n_jobs + 1] and rows.slot_off[n_jobs + 1] are the
// caller's to fill next to the jobs.  n_feat < 0: the statistics stay on the host and the block carries no feature slots.
int dev_aln_walks_stage(mpa_ctx_t *ctx, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat, int64_t slot_bytes, int64_t rows_bytes, AlnStatsIO &io, AlnCsIO &cs,
                        AlnRowsIO &rows)
{
	io = AlnStatsIO(), cs = AlnCsIO(), rows = AlnRowsIO();
	if (n_jobs <= 0 || n_jobs > (int64_t)1 << 28 || (slot_bytes < 0 && rows_bytes < 0)) { set_error("GPU cs strings / residue rows: no alignments, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const StatsLayout L(n_jobs, n_cigar, text_bytes, n_feat < 0 ? 0 : n_feat, slot_bytes, rows_bytes);
	if (ctx->h_stats_up.ensure(L.up_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (slot_bytes >= 0 && ctx->h_cs_down.ensure(L.cs_down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (rows_bytes >= 0 && ctx->h_rows_down.ensure(L.rows_down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (n_feat >= 0 && ctx->h_stats_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->h_stats_up.as<char>();
	io.jobs = (AlnStatsJob*)(hu + L.off_jobs), io.cigar = (uint32_t*)(hu + L.off_cig), io.text = hu + L.off_text;
	if (slot_bytes >= 0) cs.slot_off = (int64_t*)(hu + L.off_slot);
	if (rows_bytes >= 0) rows.slot_off = (int64_t*)(hu + L.off_rslot);
	return MPA_OK;
}

// The cs bodies of the n_jobs alignments staged in io / cs on ctx -- cs.out[j].len bytes at cs.body + cs.slot_off[j] -- their residue
// rows -- rows.out[j] and the slot at rows.body + rows.slot_off[j], laid out as aln_rows_core.h says -- and, with n_feat >= 0, their
// statistics as dev_aln_stats() leaves them, behind one upload and one wait.  All of it is pinned memory of the context, valid until
// its next call.  MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller keeps the host's walks.
int dev_aln_walks(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const AlnRowsParams &rp, const int8_t *mat, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes,
                  int64_t n_feat, int64_t slot_bytes, int64_t rows_bytes, AlnStatsIO &io, AlnCsIO &cs, AlnRowsIO &rows)
{
	return stats_walks_run(ctx, mi, p, mat, n_jobs, StatsLayout(n_jobs, n_cigar, text_bytes, n_feat < 0 ? 0 : n_feat, slot_bytes, rows_bytes), n_feat >= 0, io,
	                       slot_bytes >= 0 ? &cs : nullptr, &rp, rows_bytes >= 0 ? &rows : nullptr);
}

} // namespace mpa
