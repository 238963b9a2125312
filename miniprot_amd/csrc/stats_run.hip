// stats_run.hip -- the device unit of the alignment statistics (MPA_GPU_STATS=1; kernel: stats_kernels.hip, code: aln_stats_core.h).
// take_round3() of host_map.cpp fills one pinned block (tables | jobs | CIGAR words | the batch's protein text) through
// dev_aln_stats_stage(), dev_aln_stats() sends it up, launches k_aln_stats on the context that ran the batch's DP rounds, takes one
// pinned block down (per-alignment records | features) and waits once.  The pools (st_in, st_out and their staging) are grow-only and
// allocated on first use: a run that never sets the knob holds none of them.
// MPA_GPU_CS=1 (kernel k_aln_cs, code: aln_cs_core.h) goes the same way through dev_aln_cs_stage() / dev_aln_cs():
// the block that goes up gains the slot offsets (tables | jobs | slot offsets | CIGAR words | protein text), one more pinned block
// comes down (lengths | slots: cs_out and its staging), and when the statistics run on the device too the two kernels share the
// upload and the wait.
#include "dev_ctx.h"
#include "stats_kernels.hip"

namespace mpa {

namespace {
struct StatsLayout {
	size_t off_jobs, off_slot, off_cig, off_text, up_bytes, off_feat, down_bytes, off_body, cs_down_bytes;
	// slot_bytes < 0: no cs strings (the block that goes up is then what it was without them)
	StatsLayout(int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat, int64_t slot_bytes = -1)
	{
		auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
		off_jobs = 1024;                                                   // (the tables take ALN_TAB_BYTES of the first KB)
		off_slot = off_jobs + up16((size_t)n_jobs * sizeof(AlnStatsJob));
		off_cig = off_slot + (slot_bytes >= 0 ? up16((size_t)(n_jobs + 1) * 8) : 0);
		off_text = off_cig + up16((size_t)n_cigar * 4);
		up_bytes = off_text + up16((size_t)text_bytes) + 16;
		off_feat = up16((size_t)n_jobs * sizeof(AlnStatsOut));
		down_bytes = off_feat + (size_t)n_feat * sizeof(AlnFeat) + 16;
		off_body = up16((size_t)n_jobs * sizeof(AlnCsOut));
		cs_down_bytes = off_body + (size_t)(slot_bytes > 0 ? slot_bytes : 0) + 16;
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

// What dev_aln_stats() and dev_aln_cs() share: the tables into the staged block, one upload, the launches asked for (stats: k_aln_stats;
// cs: k_aln_cs), their downloads and one wait.
static int stats_cs_run(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const int8_t *mat, int64_t n_jobs, const StatsLayout &L, bool stats, AlnStatsIO &io, AlnCsIO *cs)
{
	if (p.asize < 1 || p.asize * p.asize > 484) { set_error("GPU alignment statistics: a substitution matrix of more than 22 x 22"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	const DeviceIndex *d = mi->dev[ctx->device];
	if (L.up_bytes > ctx->h_stats_up.cap || (stats && L.down_bytes > ctx->h_stats_down.cap) || (cs && L.cs_down_bytes > ctx->h_cs_down.cap)) {
		set_error("dev_aln_stats: the staging block was not sized for this call");
		return MPA_ERR_ARG;
	}
	tl_alloc_failed = false;
	if (ctx->st_in.ensure(L.up_bytes) != MPA_OK || (stats && ctx->st_out.ensure(L.down_bytes) != MPA_OK) || (cs && ctx->cs_out.ensure(L.cs_down_bytes) != MPA_OK))
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
	HIP_TRY(wait_stream(ctx, s));
	return MPA_OK;
}

// The statistics and features of the n_jobs alignments staged in io, on ctx.  io.out / io.feat point into pinned memory of the
// context afterwards, valid until its next call.  MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller runs the host stage.
int dev_aln_stats(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const int8_t *mat, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat,
                  AlnStatsIO &io)
{
	return stats_cs_run(ctx, mi, p, mat, n_jobs, StatsLayout(n_jobs, n_cigar, text_bytes, n_feat), true, io, nullptr);
}

// The same for a call that writes cs strings: slot_bytes = the sum of the alignments' aln_cs_bound(); cs.slot_off[n_jobs + 1] is the
// caller's to fill next to the jobs.  n_feat < 0: the statistics stay on the host and the block carries no feature slots.
int dev_aln_cs_stage(mpa_ctx_t *ctx, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat, int64_t slot_bytes, AlnStatsIO &io, AlnCsIO &cs)
{
	io = AlnStatsIO(), cs = AlnCsIO();
	if (n_jobs <= 0 || n_jobs > (int64_t)1 << 28 || slot_bytes < 0) { set_error("GPU cs strings: no alignments, or too many for one launch"); return MPA_ERR_UNSUPPORTED; }
	if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); return MPA_ERR_HIP; }
	const StatsLayout L(n_jobs, n_cigar, text_bytes, n_feat < 0 ? 0 : n_feat, slot_bytes);
	if (ctx->h_stats_up.ensure(L.up_bytes) != MPA_OK || ctx->h_cs_down.ensure(L.cs_down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	if (n_feat >= 0 && ctx->h_stats_down.ensure(L.down_bytes) != MPA_OK) return MPA_ERR_UNSUPPORTED;
	char *hu = ctx->h_stats_up.as<char>();
	io.jobs = (AlnStatsJob*)(hu + L.off_jobs), io.cigar = (uint32_t*)(hu + L.off_cig), io.text = hu + L.off_text;
	cs.slot_off = (int64_t*)(hu + L.off_slot);
	return MPA_OK;
}

// The cs bodies of the n_jobs alignments staged in io / cs on ctx -- cs.out[j].len bytes at cs.body + cs.slot_off[j], pinned memory
// of the context, valid until its next call -- and, with n_feat >= 0, their statistics as dev_aln_stats() leaves them, behind one
// upload and one wait.  MPA_ERR_UNSUPPORTED: a pool could not grow -- the caller keeps the host's put_cs (and statistics).
int dev_aln_cs(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const int8_t *mat, int64_t n_jobs, int64_t n_cigar, int64_t text_bytes, int64_t n_feat,
               int64_t slot_bytes, AlnStatsIO &io, AlnCsIO &cs)
{
	return stats_cs_run(ctx, mi, p, mat, n_jobs, StatsLayout(n_jobs, n_cigar, text_bytes, n_feat < 0 ? 0 : n_feat, slot_bytes), n_feat >= 0, io, &cs);
}

} // namespace mpa
