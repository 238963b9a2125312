// seed_run.hip -- host drivers of the seeding stage on the device: the sketch (dev_sketch_jobs; kernels in sketch_exec.hip), the sift
// and both chaining rounds behind the pre-chain (dev_prechain_forward) or without one (dev_seed_direct), the forward pass of mp_chain
// for the host's chains (dev_chain_forward), and the chain tail that these routes and the refinement (refine_run.hip) share.  The
// unit of the sift and chain kernels (seed_exec.hip): nothing else launches them.
#include "dev_ctx.h"
#include "seed_exec.hip"
#include "sketch_exec.hip"
#include "region_kernels.hip"
#include "plan_kernels.hip"

namespace mpa {
// ---- the chain tail (declared in dev_ctx.h): the forward pass of mp_chain, the extraction and the packed download, as every
// device chaining route runs them
PreParams pre_params(const ChainParams &cp)
{
	PreParams pp;
	pp.max_dist_x = std::max(cp.max_dist_x, cp.bw), pp.max_dist_y = cp.max_dist_y;
	if (pp.max_dist_y < cp.bw && !cp.is_spliced) pp.max_dist_y = cp.bw;
	pp.bw = cp.bw, pp.max_skip = cp.max_skip, pp.max_iter = cp.max_iter, pp.kmer = cp.kmer, pp.bbit = cp.bbit;
	pp.is_spliced = cp.is_spliced, pp.coef_log = cp.coef_log, pp.max_dblock = pp.max_dist_x >> cp.bbit;
	return pp;
}

int chain_fwd_launch(hipStream_t s, const uint64_t *a, int64_t n, const int64_t *first, const int64_t *cnt, int32_t n_prob, const PreParams &pp, int32_t serial_run,
                     const ChainFwdBufs &b)
{
	const unsigned nblk = (unsigned)((n + 255) / 256);
	hipLaunchKernelGGL(k_seed_fill, dim3(nblk), dim3(256), 0, s, n, pp.kmer, b.f, b.pred, b.mark, b.flag);
	hipLaunchKernelGGL(k_chain_fwd, dim3(nblk), dim3(256), 0, s, a, n, first, cnt, n_prob, pp, b.f, b.pred, b.mark, serial_run, b.runs, b.n_runs, (unsigned int)b.long_cap);
	hipLaunchKernelGGL(k_chain_fwd_wave, dim3((unsigned)std::min<size_t>(b.long_cap, 65536)), dim3(64), 0, s, a, (const LongRun*)b.runs, (const unsigned int*)b.n_runs,
	                   (unsigned int)b.long_cap, pp, b.f, b.pred, b.mark);
	HIP_TRY(hipGetLastError());
	return MPA_OK;
}

// MPA_TIMING=2 (debug): per-phase wall clock of the extraction kernel, averaged over the problems of the launch
static bool extract_prof_on()
{
	static const bool prof = [] { const char *e = getenv("MPA_TIMING"); return e && atoi(e) >= 2; }();
	return prof;
}
static int extract_prof_begin(hipStream_t s, size_t NQ, long long *&d_prof)
{
	HIP_TRY(hipMalloc((void**)&d_prof, NQ * 128 + 64));
	HIP_TRY(hipMemsetAsync(d_prof, 0, NQ * 128, s));
	const int n_prof = (int)NQ;
	HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof_n), &n_prof, sizeof(n_prof), 0, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof), &d_prof, sizeof(d_prof), 0, hipMemcpyHostToDevice, s));
	return MPA_OK;
}
static int extract_prof_end(mpa_ctx_t *ctx, hipStream_t s, size_t NQ, long long *&d_prof, const char *what)
{
	std::vector<long long> h(NQ * 16);
	HIP_TRY(hipMemcpyAsync(h.data(), d_prof, NQ * 128, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	double sum[4] = { 0, 0, 0, 0 }, sub[4] = { 0, 0, 0, 0 }, mx = 0;
	int64_t cnt = 0, cnt2 = 0;
	std::vector<std::pair<double, size_t>> by_time;
	for (size_t q = 0; q < NQ; ++q) {
		const long long *t = &h[q * 16];
		if (!t[4] || !t[0]) continue;
		for (int k = 0; k < 4; ++k) sum[k] += (double)(t[k + 1] - t[k]) * 1e-5;   // 100 MHz ticks -> ms
		mx = std::max(mx, (double)(t[4] - t[0]) * 1e-5), ++cnt;
		by_time.emplace_back((double)(t[4] - t[0]) * 1e-5, q);
		if (t[5] && t[6] && t[7]) {                            // the two-level sort replay: its parts (stamps 5-7 lie between 0 and 1)
			sub[0] += (double)(t[5] - t[0]) * 1e-5, sub[1] += (double)(t[6] - t[5]) * 1e-5;
			sub[2] += (double)(t[7] - t[6]) * 1e-5, sub[3] += (double)(t[1] - t[7]) * 1e-5, ++cnt2;
		}
	}
	fprintf(stderr, "[mpa-extract-prof] %s: %lld problems; mean ms: sort replay %.2f, trees %.2f, extraction %.2f, output %.2f; slowest problem %.2f ms\n", what, (long long)cnt,
	        sum[0] / std::max<int64_t>(cnt, 1), sum[1] / std::max<int64_t>(cnt, 1), sum[2] / std::max<int64_t>(cnt, 1), sum[3] / std::max<int64_t>(cnt, 1), mx);
	if (cnt2) fprintf(stderr, "[mpa-extract-prof]   two-level replay (%lld problems): level-1 placement %.2f, level-1 walk %.2f, merge %.2f, level 2 %.2f ms\n", (long long)cnt2,
	                  sub[0] / cnt2, sub[1] / cnt2, sub[2] / cnt2, sub[3] / cnt2);
	if (!by_time.empty()) {                                   // the distribution, and what the slowest problems look like
		std::sort(by_time.begin(), by_time.end());
		const size_t n = by_time.size();
		fprintf(stderr, "[mpa-extract-prof]   problem ms: p50 %.2f p90 %.2f p99 %.2f max %.2f\n", by_time[n / 2].first, by_time[n * 9 / 10].first, by_time[n * 99 / 100].first, by_time[n - 1].first);
		for (size_t k = 0; k < std::min<size_t>(n, 6); ++k) {
			const size_t q = by_time[n - 1 - k].second;
			const long long *t = &h[q * 16];
			fprintf(stderr, "[mpa-extract-prof]   slow #%zu: %.2f ms (replay %.2f [lvl2 %.2f] trees %.2f extraction %.2f output %.2f); view %lld, non-roots %lld, high scores %lld, largest level-2 bucket %lld, merged %lld\n", k,
			        by_time[n - 1 - k].first, (double)(t[1] - t[0]) * 1e-5, t[7] ? (double)(t[1] - t[7]) * 1e-5 : 0.0, (double)(t[2] - t[1]) * 1e-5, (double)(t[3] - t[2]) * 1e-5, (double)(t[4] - t[3]) * 1e-5,
			        t[8], t[9], t[10], t[11], t[12]);
		}
		const size_t q = by_time[n / 2].second;
		const long long *t = &h[q * 16];
		fprintf(stderr, "[mpa-extract-prof]   median problem: view %lld, non-roots %lld, high scores %lld, largest level-2 bucket %lld, merged %lld\n", t[8], t[9], t[10], t[11], t[12]);
	}
	long long *none = nullptr;
	HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof), &none, sizeof(none), 0, hipMemcpyHostToDevice, s));
	HIP_TRY(wait_stream(ctx, s));
	HIP_TRY(hipDeviceSynchronize());                   // (debug facility: an extraction launched by another context may still be stamping into the buffer)
	(void)hipFree(d_prof), d_prof = nullptr;
	return MPA_OK;
}

int chain_extract_launch(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, const ChainParams &p, int32_t n_prob, int32_t set_only,
                         const char *prof_label)
{
	ExtractArgs xa;
	xa.first = v.first, xa.cnt = v.cnt, xa.ntot_first = v.ntot_first;
	xa.v_pos = v.v_pos, xa.v_f = v.v_f, xa.v_pred = v.v_pred, xa.v_a = v.v_a;
	xa.mark = c.mark.in(X), xa.order = c.order.in(X), xa.ends = c.ends.in(X), xa.tail8 = c.tail8.in(X);
	xa.items = c.items.in(X), xa.moved = c.moved.in(X), xa.merged = c.merged.in(X);
	xa.kept = c.kept.in(X), xa.stack = c.stack.in(X);
	xa.a_out = c.out_a.in(X), xa.u_out = c.out_u.in(X), xa.n_a = c.na.in(X), xa.n_u = c.nu.in(X);
	xa.status = c.status.in(X), xa.p = p, xa.set_only = set_only;
	const bool prof = prof_label && extract_prof_on();
	long long *d_prof = nullptr;
	int rc;
	if (prof && (rc = extract_prof_begin(s, (size_t)n_prob, d_prof))) return rc;
	hipLaunchKernelGGL(k_chain_extract, dim3((unsigned)n_prob), dim3(64), EXTRACT_LDS_BYTES, s, xa, n_prob);
	HIP_TRY(hipGetLastError());
	if (prof && (rc = extract_prof_end(ctx, s, (size_t)n_prob, d_prof, prof_label))) return rc;
	return MPA_OK;
}

// The regions of every problem behind its main-chain extraction (MPA_GPU_REGIONS=1): k_regions reads the chains where the extraction
// left them in X, k_region_pack puts records, limits and counts into the holder's pinned block.  Everything is laid out by the prefix
// of the chain counts (h_offu, on the device at c.offu), which the caller has just downloaded: a query keeps at most as many regions
// as it has chains.  MPA_ERR_UNSUPPORTED: a pool or the pinned block could not grow -- nothing was launched, the caller packs the chains.
static int regions_tail(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, int32_t n_prob, SeedHold &H, int64_t tot_u, RegionsTail &rt)
{
	SeedBufs &B = ctx->seed;
	const size_t T = (size_t)tot_u, NP = (size_t)n_prob;
	const double t0 = now_ms();
	const RegionsLayout L(T, NP);
	if (B.rg.ensure(L.dev_bytes) != MPA_OK || H.h_R.ensure(L.pinned_bytes) != MPA_OK) {
		tl_alloc_failed = false;
		if (timing_on()) fprintf(stderr, "[mpa-timing]   device regions declined (%s): chains to the host\n", mpa_last_error());
		return MPA_ERR_UNSUPPORTED;
	}
	char *G = B.rg.as<char>(), *P = H.h_R.as<char>();
	rt.R = L.h_rec.in(P), rt.E = L.h_ext.in(P), rt.n_reg = L.h_nreg.in(P);
	if (tot_u == 0) { memset(L.h_nreg.in(P), 0, L.h_nreg.bytes()); rt.done = true; return MPA_OK; }
	RegionsArgs ra;
	ra.first = v.first, ra.a = c.out_a.in(X), ra.u = c.out_u.in(X), ra.nu = c.nu.in(X), ra.offu = c.offu.in(X);
	ra.bo = rt.d_bo, ra.p = rt.p;
	ra.tmp = L.tmp.in(G), ra.out = L.out.in(G), ra.ext = L.ext.in(G), ra.cov = L.cov.in(G), ra.key = L.key.in(G);
	ra.stack = L.stack.in(G), ra.hist = L.hist.in(G), ra.prim = L.prim.in(G), ra.ctl = L.ctl.in(G), ra.n_reg = L.n_reg.in(G);
	hipLaunchKernelGGL(k_regions, dim3((unsigned)((n_prob + REGIONS_WAVES - 1) / REGIONS_WAVES)), dim3(64 * REGIONS_WAVES), 0, s, ra, n_prob);
	hipLaunchKernelGGL(k_region_pack, dim3((unsigned)n_prob), dim3(256), 0, s, ra.offu, (const int32_t*)ra.n_reg, (const RegionRec*)ra.out, (const uint64_t*)ra.ext,
	                   L.h_rec.in(P), L.h_ext.in(P), L.h_nreg.in(P));
	HIP_TRY(hipGetLastError());
	HIP_TRY(wait_stream(ctx, s));
	rt.done = true;
	timing_note("    seed: regions + pack (wait)", now_ms() - t0);
	return MPA_OK;
}

// The plans of every query behind the extraction of its refinement windows' chains (MPA_GPU_PLANS=1): k_plans reads the chains where
// the extraction left them in X, k_plan_pack puts the kept records and the counts into the holder's pinned block.  Everything is
// laid out by the windows and by the prefix of their extracted anchors (h_offa, on the device at c.offa), which the caller has just
// downloaded: a query has at most a region and a plan per window, a gap segment per anchor and four tasks per window on top of
// those.  MPA_ERR_UNSUPPORTED: a pool or the pinned block could not grow -- nothing was launched, the caller packs the chains.
static int plans_tail(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, int32_t n_prob, SeedHold &H, int64_t tot_a, PlansTail &pt)
{
	SeedBufs &B = ctx->seed;
	const size_t T = (size_t)tot_a, NW = (size_t)n_prob, NQ = (size_t)pt.n_query;
	const double t0 = now_ms();
	const PlansLayout L(T, NW, NQ);
	if (B.pl.ensure(L.dev_bytes) != MPA_OK || H.h_P.ensure(L.pinned_bytes) != MPA_OK) {
		tl_alloc_failed = false;
		if (timing_on()) fprintf(stderr, "[mpa-timing]   device plans declined (%s): chains to the host\n", mpa_last_error());
		return MPA_ERR_UNSUPPORTED;
	}
	char *G = B.pl.as<char>(), *P = H.h_P.as<char>();
	pt.R = L.h_reg.in(P), pt.P = L.h_plan.in(P), pt.T = L.h_task.in(P), pt.S = L.h_seg.in(P), pt.N = L.h_cnt.in(P);
	PlansArgs pa{};
	pa.first = v.first, pa.nu = c.nu.in(X), pa.offa = c.offa.in(X), pa.u = c.out_u.in(X), pa.a = c.out_a.in(X);
	pa.win = pt.d_win, pa.win0 = pt.d_win0, pa.q_off = pt.d_qoff, pa.text = pt.d_text, pa.tabs = pt.d_tabs;
	pa.g = PlansGenome{ pt.d_seq, pt.d_ctg_off, pt.d_ctg_len }, pa.p = pt.p;
	pa.tmp = L.tmp.in(G), pa.key = L.key.in(G), pa.stack = L.stack.in(G), pa.hist = L.hist.in(G), pa.prim = L.prim.in(G);
	pa.flag = L.flag.in(G), pa.list = L.list.in(G), pa.ctl = L.ctl.in(G), pa.cov = L.cov.in(G), pa.ext = L.ext.in(G);
	pa.aoff = L.aoff.in(G), pa.reg = L.reg.in(G), pa.plan = L.plan.in(G), pa.task = L.task.in(G), pa.seg = L.seg.in(G);
	pa.cnt = L.cnt.in(G);
	hipLaunchKernelGGL(k_plans, dim3((unsigned)((pt.n_query + PLANS_WAVES - 1) / PLANS_WAVES)), dim3(64 * PLANS_WAVES), 0, s, pa, pt.n_query);
	hipLaunchKernelGGL(k_plan_pack, dim3((unsigned)pt.n_query), dim3(256), 0, s, pa.win0, pa.offa, (const PlansCounts*)pa.cnt, (const RegionRec*)pa.reg, (const PlanRec*)pa.plan,
	                   (const mpa_dp_task_t*)pa.task, (const SegRec*)pa.seg, L.h_reg.in(P), L.h_plan.in(P), L.h_task.in(P), L.h_seg.in(P), L.h_cnt.in(P));
	HIP_TRY(hipGetLastError());
	HIP_TRY(wait_stream(ctx, s));
	pt.done = true;
	timing_note("    refine: plans + pack (wait)", now_ms() - t0);
	return MPA_OK;
}

int chain_extract_pack(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, const ChainParams &p, int32_t n_prob, SeedHold &H,
                       const char *prof_label, const char *status_error, ChainTailOut out, const int32_t **h_status_out, RegionsTail *regions, PlansTail *plans)
{
	SeedBufs &B = ctx->seed;
	const size_t NP = (size_t)n_prob;
	int rc;
	if ((rc = chain_extract_launch(ctx, s, X, c, v, p, n_prob, 0, prof_label))) return rc;
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, c.na.in(X), c.nu.in(X), n_prob, c.offa.in(X), c.offu.in(X));
	HIP_TRY(hipGetLastError());
	// offsets + status down (one pinned block, packed: offa | offu | status), then the chains themselves straight into pinned memory
	Carve hc(1);
	const auto p_offa = hc.take<int64_t>(NP + 1), p_offu = hc.take<int64_t>(NP + 1); const auto p_status = hc.take<int32_t>(NP);
	if ((rc = B.h_xoff.ensure(hc.at + 64))) return rc;
	int64_t *h_offa = p_offa.in(B.h_xoff.p), *h_offu = p_offu.in(B.h_xoff.p); int32_t *h_status = p_status.in(B.h_xoff.p);
	HIP_TRY(hipMemcpyAsync(h_offa, c.offa.in(X), p_offa.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_offu, c.offu.in(X), p_offu.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_status, c.status.in(X), p_status.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	if (status_error)
		for (size_t w = 0; w < NP; ++w) if (h_status[w]) { set_error(status_error); return MPA_ERR_UNSUPPORTED; }
	const int64_t tot_a = h_offa[n_prob], tot_u = h_offu[n_prob];
	bool chains = true;                                      // the regions or the plans instead of the chains; declined: the chains, as without them
	if (regions) {
		regions->done = false;
		rc = regions_tail(ctx, s, X, c, v, n_prob, H, tot_u, *regions);
		if (rc != MPA_OK && rc != MPA_ERR_UNSUPPORTED) return rc;
		chains = rc != MPA_OK;
	}
	if (plans && chains) {
		plans->done = false;
		rc = plans_tail(ctx, s, X, c, v, n_prob, H, tot_a, *plans);
		if (rc != MPA_OK && rc != MPA_ERR_UNSUPPORTED) return rc;
		chains = rc != MPA_OK;
	}
	if (chains) {
		if ((rc = H.h_A.ensure((size_t)tot_a * 8 + 64)) || (rc = H.h_U.ensure((size_t)tot_u * 8 + 64))) return rc;
		if (tot_a > 0 || tot_u > 0) {
			hipLaunchKernelGGL(k_chain_pack, dim3((unsigned)n_prob), dim3(256), 0, s, v.first, c.na.in(X), c.nu.in(X), c.offa.in(X), c.offu.in(X), c.out_a.in(X), c.out_u.in(X),
			                   H.h_A.as<uint64_t>(), H.h_U.as<uint64_t>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(wait_stream(ctx, s));
		}
	}
	out.a_first.assign(h_offa, h_offa + n_prob + 1), out.u_first.assign(h_offu, h_offu + n_prob + 1);
	out.A = chains ? H.h_A.as<uint64_t>() : nullptr, out.U = chains ? H.h_U.as<uint64_t>() : nullptr;
	if (h_status_out) *h_status_out = h_status;
	return MPA_OK;
}

// the queries the host takes over: those an extraction declined (h_status) on top of the sift's hand-backs (h_flag, may be null)
static void seed_mark_on_host(PrechainSparse &out, int32_t n_query, const int32_t *h_status, const int32_t *h_flag)
{
	bool any = !out.on_host.empty();
	for (int32_t q = 0; q < n_query && !any; ++q) any = h_status[q] != 0;
	if (any) {
		if (out.on_host.empty()) out.on_host.assign((size_t)n_query, 0);
		for (int32_t q = 0; q < n_query; ++q) if (h_status[q] || (h_flag && h_flag[q])) out.on_host[(size_t)q] = 1;
	}
}

// what a seeding route hands the chain tail for MPA_GPU_REGIONS=1 (nullptr: the chains), and what it takes from it afterwards
static RegionsTail *regions_tail_begin(mpa_ctx_t *ctx, mpa_idx_s *mi, const RegionsParams *rp, RegionsTail &rt)
{
	if (!rp) return nullptr;
	// bo[] next to kb[] in HBM, on the first device regions call of a device.  No device memory for it: the chains' route
	DeviceIndex *d = mi->dev[ctx->device];
	const hipError_t e = dev_index_table(ctx, d->bo, mi->bo.data(), mi->bo.size() * 4, "index upload: block offsets");
	const uint32_t *d_bo = d->bo;
	if (e != hipSuccess) {
		set_error(e == hipErrorOutOfMemory ? "device regions: no device memory for the block offsets" : "device regions: uploading the block offsets");
		if (timing_on()) fprintf(stderr, "[mpa-timing]   device regions declined (%s): chains to the host\n", mpa_last_error());
		return nullptr;
	}
	rt = RegionsTail{ *rp, d_bo, false, nullptr, nullptr, nullptr };
	return &rt;
}
static void regions_tail_end(const RegionsTail *rt, PrechainSparse &out)
{
	out.has_regions = rt && rt->done;
	if (out.has_regions) out.R = rt->R, out.E = rt->E, out.n_reg = rt->n_reg;
}
} // namespace mpa

namespace mpa {
// dev_prechain_forward() with k_seed_sift (the default).  The caller has uploaded the jobs.  Per-anchor memory: 16 bytes of
// staging; everything behind the sift is sized by the kept anchors.  The result arrays are written by k_seed_compact straight
// into pinned host memory (no copy kernels, no second pass over HBM).
static int dev_chains_on_device(mpa_ctx_t *ctx, int32_t n_query, int64_t m, int64_t n2, int nb, const uint64_t *key, const uint64_t *val, const int64_t *d_qfirst,
                                const int32_t *h_flag, const ChainParams &pre, const ChainParams &mainp, PrechainSparse &out, SeedHold &H, RegionsTail *regions);

// The sift of a batch up to the host's first look at it: segments, k_seed_sift, k_sift_offsets, the per-query first kept anchor
// and the hand-back flags down (one wait).  reach < 0: the pre-chain's keep rule (same or adjacent block, halved staging for large
// queries); reach >= 0: the main chain's reach, full staging (k_seed_sift<4096, true>).  n_seg == 0 / n2 == 0: nothing (kept).
struct SiftFront {
	int32_t n_seg = 0;
	int64_t n2 = 0;                                          // kept anchors of the batch
	const SiftSeg *d_segs = nullptr;
	const int64_t *d_qfirst = nullptr;
	uint64_t *stage0 = nullptr, *stage1 = nullptr;
	int64_t *h_qfirst2 = nullptr, *h_cfirst = nullptr;       // pinned: first kept anchor of every query; room for one more prefix array
	int32_t *h_flag = nullptr;                               // pinned: the sift's hand-back flags
	size_t meta_q = 0;
	double t_sift = 0;
};
static int dev_sift_front(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, int nb, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs, int64_t n_jobs,
                          PrechainSparse &out, double t_begin, const int64_t *jfirst_in, int32_t reach, SiftFront &F)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	if (n_block >= 0x7fffffffu) { set_error("GPU seeding: more than 2^31 blocks"); return MPA_ERR_UNSUPPORTED; }
	// ---- segments: a query's block space in pieces of ~seg_target anchors (evenly, the kernel adapts inside a segment)
	const int64_t seg_target = [] { const char *e = getenv("MPA_SIFT_SEG"); const int64_t v = e ? atoll(e) : 49152; return v < 256 ? (int64_t)256 : v; }();   // (read per call: the tests flip it)
	static thread_local std::vector<SiftSeg> segs;
	static thread_local std::vector<int64_t> jfirst;
	static thread_local std::vector<int32_t> qseg;
	segs.clear();
	int64_t n_cur = 0;                                         // cursors: one per (segment, list of its query)
	static thread_local std::vector<int64_t> sfirst;          // first staging slot of every query (sift_stage_slots)
	jfirst.assign((size_t)n_query + 1, 0), qseg.assign((size_t)n_query + 1, 0), sfirst.assign((size_t)n_query + 1, 0);
	for (int32_t q = 0; q < n_query; ++q) sfirst[(size_t)q + 1] = sfirst[(size_t)q] + (reach >= 0 ? qfirst[q + 1] - qfirst[q] : sift_stage_slots(qfirst[q + 1] - qfirst[q]));
	const int64_t n_stage = sfirst[(size_t)n_query];
	if (jfirst_in) jfirst.assign(jfirst_in, jfirst_in + n_query + 1);      // (the jobs were made on the device: dev_sketch_jobs counted them)
	else {
		for (int64_t j = 0; j < n_jobs; ++j) ++jfirst[(size_t)jobs[j].qid + 1];
		for (int32_t q = 0; q < n_query; ++q) jfirst[(size_t)q + 1] += jfirst[(size_t)q];
	}
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t na = qfirst[q + 1] - qfirst[q];
		qseg[(size_t)q] = (int32_t)segs.size();
		if (na == 0) continue;
		if (na >= (int64_t)1 << 31) { set_error("GPU seeding: a query with more than 2^31 anchors"); return MPA_ERR_UNSUPPORTED; }
		const int64_t nl_q = jfirst[(size_t)q + 1] - jfirst[(size_t)q];
		if (nl_q > (1 << 20)) { set_error("GPU seeding: a query with more than 2^20 seeds"); return MPA_ERR_UNSUPPORTED; }
		const int64_t ns = std::min<int64_t>((na + seg_target - 1) / seg_target, n_block);
		for (int64_t k = 0; k < ns; ++k) {
			const uint32_t lo = (uint32_t)((uint64_t)n_block * (uint64_t)k / (uint64_t)ns), hi = (uint32_t)((uint64_t)n_block * (uint64_t)(k + 1) / (uint64_t)ns);
			if (hi > lo) {
				if (n_cur > INT32_MAX - nl_q) { set_error("GPU seeding: too many (segment, seed) cursors in one batch"); return MPA_ERR_UNSUPPORTED; }
				segs.push_back(SiftSeg{ q, lo, hi, (int32_t)n_cur });
				n_cur += nl_q;
			}
		}
	}
	qseg[(size_t)n_query] = (int32_t)segs.size();
	const int32_t n_seg = (int32_t)segs.size();
	if (n_seg == 0) return MPA_OK;                             // (F.n_seg stays 0)
	// one pinned block up, packed: qfirst | jfirst | sfirst | segments | qseg; one down: qfirst2 | cfirst (room for one more prefix array) | flag
	const size_t NQ1 = (size_t)n_query + 1;
	Carve mc(1), bc(1), xc;
	const auto m_qf = mc.take<int64_t>(NQ1), m_jf = mc.take<int64_t>(NQ1), m_sf = mc.take<int64_t>(NQ1); const auto m_seg = mc.take<SiftSeg>((size_t)n_seg); const auto m_qs = mc.take<int32_t>(NQ1);
	const auto b_qfirst2 = bc.take<int64_t>(NQ1), b_cfirst = bc.take<int64_t>(NQ1); const auto b_flag = bc.take<int32_t>((size_t)n_query);
	const size_t meta_q = m_qf.bytes(), meta_bytes = mc.at;
	int rc;
	// (round 6: the two staging arrays of the sift -- 8 B per staging slot each, dead once k_sift_copy has packed the kept anchors --
	// live at the front of the chaining block, which is carved up only behind that copy: 4.4 GB less per seeder at genome scale)
	const auto x_stage0 = xc.take<uint64_t>((size_t)n_stage, 64), x_stage1 = xc.take<uint64_t>((size_t)n_stage, 64);
	if ((rc = B.h_meta.ensure(meta_bytes))) return rc;
	char *hm = B.h_meta.as<char>();
	memcpy(m_qf.in(hm), qfirst, meta_q), memcpy(m_jf.in(hm), jfirst.data(), meta_q), memcpy(m_sf.in(hm), sfirst.data(), meta_q), memcpy(m_seg.in(hm), segs.data(), m_seg.bytes()), memcpy(m_qs.in(hm), qseg.data(), m_qs.bytes());
	if ((rc = B.s_meta.ensure(meta_bytes)) || (rc = B.s_cur.ensure((size_t)n_cur * 4 + 16)) || (rc = B.s_cur2.ensure((size_t)n_cur * 4 + 16)) ||
	    (rc = B.s_kept.ensure((size_t)n_seg * 4)) || (rc = B.s_base.ensure((size_t)n_seg * 8)) || (rc = B.s_out.ensure(((size_t)n_seg + 1) * 8)) ||
	    (rc = B.s_flag.ensure((size_t)n_query * 4 + 16)) || (rc = B.pf_qfirst2.ensure(meta_q)) || (rc = B.cfirst.ensure(meta_q)) ||
	    (rc = B.x_all.ensure(xc.at)) || (rc = B.h_back.ensure(bc.at + 64))) return rc;
	uint64_t *const stage0 = x_stage0.in(B.x_all.p), *const stage1 = x_stage1.in(B.x_all.p);
	HIP_TRY(hipMemcpyAsync(B.s_meta.p, hm, meta_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.s_flag.p, 0, (size_t)n_query * 4 + 16, s));
	const char *dm = B.s_meta.as<char>();
	const int64_t *d_qfirst = m_qf.in(dm), *d_jfirst = m_jf.in(dm), *d_sfirst = m_sf.in(dm);
	const SiftSeg *d_segs = m_seg.in(dm); const int32_t *d_qseg = m_qs.in(dm);
	// (MPA_SIFT_CAP=2048, measurement: ranges of half the size need 18 KB of LDS instead of 37 KB -- a workgroup then fits next to
	// four DP workgroups on a CU -- and touch the lists twice as often)
	static const int sift_cap = [] { const char *e = getenv("MPA_SIFT_CAP"); return e ? atoi(e) : 4096; }();
	auto sift = [&](auto kernel, auto... reach_arg) {           // the three instantiations differ in the template arguments and the trailing reach alone
		hipLaunchKernelGGL(kernel, dim3((unsigned)n_seg), dim3(SIFT_THREADS), 0, s, d_segs, B.jobs.as<SeedJobDev>(), d_jfirst, d_qfirst, d_sfirst, d->kb, n_block, nb,
		                   B.s_cur.as<int32_t>(), B.s_cur2.as<int32_t>(), stage0, stage1, B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(), B.s_flag.as<int32_t>(), reach_arg...);
	};
	if (reach >= 0) sift(k_seed_sift<4096, true, uint32_t>, (uint32_t)reach);
	else if (sift_cap == 2048) sift(k_seed_sift<2048>);
	else sift(k_seed_sift<4096>);
	hipLaunchKernelGGL(k_sift_offsets, dim3(1), dim3(256), 0, s, d_segs, n_seg, n_query, d_qseg, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_out.as<int64_t>(),
	                   B.pf_qfirst2.as<int64_t>());
	HIP_TRY(hipGetLastError());
	int64_t *h_qfirst2 = b_qfirst2.in(B.h_back.p), *h_cfirst = b_cfirst.in(B.h_back.p); int32_t *h_flag = b_flag.in(B.h_back.p);
	HIP_TRY(hipMemcpyAsync(h_qfirst2, B.pf_qfirst2.p, meta_q, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_flag, B.s_flag.p, b_flag.bytes(), hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const double t_sift = now_ms();
	timing_note("    seed: segments + sift (wait)", t_sift - t_begin);
	int32_t n_declined = 0;
	for (int32_t q = 0; q < n_query; ++q) n_declined += h_flag[q] != 0;
	if (n_declined) {
		out.on_host.assign((size_t)n_query, 0);
		for (int32_t q = 0; q < n_query; ++q) out.on_host[(size_t)q] = h_flag[q] != 0;
	}
	F.n_seg = n_seg, F.n2 = h_qfirst2[n_query], F.d_segs = d_segs, F.d_qfirst = d_qfirst, F.stage0 = stage0, F.stage1 = stage1;
	F.h_qfirst2 = h_qfirst2, F.h_cfirst = h_cfirst, F.h_flag = h_flag, F.meta_q = meta_q, F.t_sift = t_sift;
	return MPA_OK;
}

static int dev_prechain_forward_sift(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, const PreParams &pp, int nb, int32_t n_query, const int64_t *qfirst,
                                     const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, double t_begin, const ChainParams *pre_cp, const ChainParams *main_cp, SeedHold &H,
                                     const int64_t *jfirst_in = nullptr, RegionsTail *regions = nullptr)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	SiftFront F;
	int rc = dev_sift_front(ctx, d, n_block, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, jfirst_in, -1, F);
	if (rc != MPA_OK || F.n_seg == 0 || F.n2 == 0) return rc;
	const int32_t n_seg = F.n_seg;
	const int64_t n2 = F.n2;
	const SiftSeg *d_segs = F.d_segs;
	const int64_t *d_qfirst = F.d_qfirst;
	uint64_t *const stage0 = F.stage0, *const stage1 = F.stage1;
	int64_t *h_cfirst = F.h_cfirst;
	const int32_t *h_flag = F.h_flag;
	const size_t meta_q = F.meta_q;
	const double t_sift = F.t_sift;
	if ((rc = B.dkey.ensure((size_t)n2 * 8)) || (rc = B.val64[0].ensure((size_t)n2 * 8)) || (rc = B.f.ensure((size_t)n2 * 4)) || (rc = B.pred.ensure((size_t)n2 * 4)) ||
	    (rc = B.mark.ensure((size_t)n2 * 4)) || (rc = B.flag.ensure((size_t)n2 * 4)) || (rc = B.idx.ensure((size_t)n2 * 4))) return rc;
	const unsigned nblk = (unsigned)((n2 + 255) / 256);
	const uint64_t *key = B.dkey.as<uint64_t>();
	const uint64_t *val = B.val64[0].as<uint64_t>();
	hipLaunchKernelGGL(k_sift_copy, dim3((unsigned)n_seg), dim3(256), 0, s, d_segs, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(), B.s_out.as<int64_t>(),
	                   stage0, stage1, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>());
	hipLaunchKernelGGL(k_seed_fill, dim3(nblk), dim3(256), 0, s, n2, pp.kmer, B.f.as<int32_t>(), B.pred.as<int32_t>(), B.mark.as<int32_t>(), B.flag.as<uint32_t>());
	hipLaunchKernelGGL(k_prechain_fwd<uint64_t>, dim3(nblk), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), pp, B.f.as<int32_t>(), B.pred.as<int32_t>(),
	                   B.mark.as<int32_t>(), B.flag.as<uint32_t>());
	HIP_TRY(hipGetLastError());
	if ((rc = dev_exclusive_scan(B.tmp, false, B.flag.as<uint32_t>(), B.idx.as<uint32_t>(), 0u, (size_t)n2, s))) return rc;
	hipLaunchKernelGGL(k_seed_bounds, dim3((unsigned)(n_query / 256 + 1)), dim3(256), 0, s, B.pf_qfirst2.as<int64_t>(), n_query, n2, B.idx.as<uint32_t>(), B.flag.as<uint32_t>(),
	                   B.cfirst.as<int64_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h_cfirst, B.cfirst.p, meta_q, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const double t_kernels = now_ms();
	memcpy(out.cfirst.data(), h_cfirst, meta_q);
	const int64_t m = out.cfirst[n_query];
	out.m = m;
	timing_note("    seed: copy + pre-chain + scan (wait)", t_kernels - t_sift);
	if (m == 0) return MPA_OK;
	// both chaining rounds on the device (main_cp == nullptr: the caller wants the pre-chain's linked anchors, as rounds 1-2 did)
	{
		if (main_cp && pre_cp) {
			rc = dev_chains_on_device(ctx, n_query, m, n2, nb, key, val, d_qfirst, h_flag, *pre_cp, *main_cp, out, H, regions);
			if (rc != MPA_ERR_UNSUPPORTED) { timing_note("    seed: chains on the device", now_ms() - t_kernels); return rc; }
		}
	}
	if ((rc = H.h_pos.ensure((size_t)m * 4)) || (rc = H.h_f.ensure((size_t)m * 4)) || (rc = H.h_pred.ensure((size_t)m * 4)) || (rc = H.h_a.ensure((size_t)m * 8))) return rc;
	hipLaunchKernelGGL((k_seed_compact<uint64_t, true>), dim3(nblk), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), B.flag.as<uint32_t>(), B.idx.as<uint32_t>(),
	                   B.f.as<int32_t>(), B.pred.as<int32_t>(), H.h_pos.as<int32_t>(), H.h_f.as<int32_t>(), H.h_pred.as<int32_t>(), H.h_a.as<uint64_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(wait_stream(ctx, s));
	out.pos = H.h_pos.as<int32_t>(), out.f = H.h_f.as<int32_t>(), out.pred = H.h_pred.as<int32_t>(), out.a = H.h_a.as<uint64_t>();
	timing_note("    seed: compact into pinned memory", now_ms() - t_kernels);
	return MPA_OK;
}

// Both chaining rounds of every query on the device, behind the forward pass of the pre-chain (map.c:186-196):
//   k_seed_compact      the linked anchors of every query as a sparse view (position in the full list, f, pred, anchor), in HBM
//   k_chain_extract     pre-chain extraction (set): the survivors of every query, ascending
//   k_chain_fwd         forward pass of the main chain over them (block anchors, max_dist_x = max_intron)
//   k_chain_extract     main-chain extraction: chains (score, count) and their anchors, sorted by first target position
//   k_offsets2 + k_chain_pack   the chains of all queries, densely, into pinned host memory
// What travels back is what mp_reg_gen_from_block() consumes (a few hundred anchors per query) instead of every linked anchor
// (~11 000 per query at 3 Gbp), and the host no longer spends a core-second per mini-batch on chaining.
// key/val: the kept anchors (dense, sorted), with B.f / B.pred / B.flag / B.idx / B.cfirst from the pre-chain's forward pass.
static int dev_chains_on_device(mpa_ctx_t *ctx, int32_t n_query, int64_t m, int64_t n2, int nb, const uint64_t *key, const uint64_t *val, const int64_t *d_qfirst,
                                const int32_t *h_flag, const ChainParams &pre, const ChainParams &mainp, PrechainSparse &out, SeedHold &H, RegionsTail *regions)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	if (mainp.bbit != pre.bbit || mainp.kmer != pre.kmer) { set_error("device chains: pre-chain and main chain disagree on the anchors"); return MPA_ERR_UNSUPPORTED; }
	// ---- one allocation, carved up: everything is indexed like the view (m entries), `ends` and `stack` have extras per problem
	const size_t M = (size_t)m, NQ = (size_t)n_query;
	Carve carve;
	// (the view's positions and scores share one piece: the main chains' u words land there once the pre-chain has been extracted)
	const auto v_posf = carve.take<int32_t>(2 * M), v_pos = v_posf.sub<int32_t>(0, M), v_f = v_posf.sub<int32_t>(M * 4, M), v_pred = carve.take<int32_t>(M); const auto v_a = carve.take<uint64_t>(M);
	ExtractCarve xc = carve_extract_scratch(carve, M, NQ);
	const auto pre_a = carve.take<uint64_t>(M), pre_u = carve.take<uint64_t>(M); const auto pre_na = carve.take<int64_t>(NQ + 1), pre_nu = carve.take<int64_t>(NQ + 1);
	const ChainFwdCarve fw = carve_chain_fwd(carve, M, kChainSerialRun);   // longer runs of the main chain get a wavefront each (k_chain_fwd_wave)
	// (the main chains go where the pre-chain's view was: it is dead once the pre-chain has been extracted)
	xc.out_a = v_a, xc.out_u = v_posf.sub<uint64_t>(0, M);
	carve_extract_counts(carve, NQ, xc);
	int rc;
	if ((rc = B.x_all.ensure(carve.at))) return rc;         // (ensure() adds a third of slack: a re-allocation is a hipFree, which waits for the whole device)
	char *X = B.x_all.as<char>();
	HIP_TRY(hipMemsetAsync(xc.status.in(X), 0, xc.status.bytes() + 16, s));
	const unsigned nblk2 = (unsigned)((n2 + 255) / 256);
	// the sparse view of the pre-chain's forward pass
	hipLaunchKernelGGL((k_seed_compact<uint64_t, true>), dim3(nblk2), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), B.flag.as<uint32_t>(), B.idx.as<uint32_t>(),
	                   B.f.as<int32_t>(), B.pred.as<int32_t>(), v_pos.in(X), v_f.in(X), v_pred.in(X), v_a.in(X));
	// pre-chain extraction (the survivors as a set): into the pre_* arrays, over the scratch the main chain's extraction uses again
	ExtractCarve pc = xc;
	pc.out_a = pre_a, pc.out_u = pre_u, pc.na = pre_na, pc.nu = pre_nu;
	const ChainViewDev pre_view{ B.cfirst.as<int64_t>(), nullptr, d_qfirst, v_pos.in(X), v_f.in(X), v_pred.in(X), v_a.in(X) };
	if ((rc = chain_extract_launch(ctx, s, X, pc, pre_view, pre, n_query, 1, "pre-chain"))) return rc;
	// the main chain over the survivors: forward pass ...
	const PreParams pm = pre_params(mainp);
	HIP_TRY(hipMemsetAsync(fw.n_runs.in(X), 0, fw.n_runs.bytes(), s));
	if ((rc = chain_fwd_launch(s, pre_a.in(X), m, B.cfirst.as<int64_t>(), pre_na.in(X), n_query, pm, kChainSerialRun, fw.in(X, xc)))) return rc;
	// ... and extraction: dense views over the survivors; the chains of all queries into pinned memory
	const ChainViewDev main_view{ B.cfirst.as<int64_t>(), pre_na.in(X), nullptr, nullptr, fw.f.in(X), fw.pred.in(X), pre_a.in(X) };
	const int32_t *h_status = nullptr;
	if ((rc = chain_extract_pack(ctx, s, X, xc, main_view, mainp, n_query, H, "main chain", nullptr, ChainTailOut{ out.a_first, out.u_first, out.A, out.U }, &h_status, regions))) return rc;
	out.has_chains = true;
	seed_mark_on_host(out, n_query, h_status, h_flag);
	return MPA_OK;
}

// Seeding without a pre-chain (map.c:186 skips it with -S and --no-pre-chain), on the seeding stream:
//   k_seed_sift<4096, true>   the anchors of every query in sorted order, those kept that have another one within the main chain's reach
//   k_sift_offsets, k_sift_copy   ... densely; k_sift_anchors: block << 32 | query position, and the rank the sift carried
//   k_chain_fwd + k_chain_fwd_wave   forward pass of the MAIN chain over the kept anchors (the kernels of dev_chains_on_device, unchanged)
//   k_chain_extract     main-chain extraction from a SPARSE view: every kept anchor at its rank in the query's full list (set_only = 0)
//   k_offsets2 + k_chain_pack   the chains of all queries, densely, into pinned host memory
// The view holds ALL kept anchors, not only those the pass linked: a kept anchor without a link is a root like an absent one, the
// extraction steps over both alike, and a second compaction would cost a scan and a pass over the view to save part of one.
// Exact because a dropped anchor has no anchor of its query within max_dist_x: it has no predecessor, is nobody's predecessor and
// lies in no window that a kept anchor's max_skip / max_iter walk visits -- what a sparse view may leave out (chain_core.h).
// pm: the main chain's parameters as the forward pass takes them (pm.max_dblock = the sift's reach).
static int dev_seed_direct_impl(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, const PreParams &pm, int nb, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs,
                                int64_t n_jobs, PrechainSparse &out, double t_begin, const ChainParams &mainp, SeedHold &H, const int64_t *jfirst_in, SiftKept *kept, RegionsTail *regions)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	SiftFront F;
	int rc = dev_sift_front(ctx, d, n_block, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, jfirst_in, pm.max_dblock, F);
	if (rc != MPA_OK || F.n_seg == 0) return rc;
	if (kept) for (int32_t q = 0; q < n_query; ++q) kept->flag[(size_t)q] = F.h_flag[q] != 0;
	if (F.n2 == 0) return MPA_OK;
	const int64_t n2 = F.n2;
	const size_t M = (size_t)n2, NQ = (size_t)n_query;
	if ((rc = B.dkey.ensure(M * 8)) || (rc = B.val64[0].ensure(M * 8))) return rc;
	hipLaunchKernelGGL(k_sift_copy, dim3((unsigned)F.n_seg), dim3(256), 0, s, F.d_segs, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(), B.s_out.as<int64_t>(),
	                   F.stage0, F.stage1, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>());
	HIP_TRY(hipGetLastError());
	if (kept) {                                                // (test hook: the kept anchors of every query, as the chain would take them)
		std::vector<uint64_t> hk(M), hv(M);
		HIP_TRY(hipMemcpyAsync(hk.data(), B.dkey.p, M * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(hv.data(), B.val64[0].p, M * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		kept->first.assign(F.h_qfirst2, F.h_qfirst2 + n_query + 1), kept->a.resize(M);
		for (size_t i = 0; i < M; ++i) kept->a[i] = (hk[i] & ((1ULL << nb) - 1)) << 32 | (uint32_t)hv[i];
		return MPA_OK;
	}
	// ---- one allocation, carved up, as in dev_chains_on_device: the view (= the forward pass's own arrays), the extraction's scratch, the chains
	Carve carve;
	ChainFwdCarve fw{};                                      // (the view's f / pred ARE the forward pass's)
	const auto v_pos = carve.take<int32_t>(M), v_f = fw.f = carve.take<int32_t>(M), v_pred = fw.pred = carve.take<int32_t>(M); const auto v_a = carve.take<uint64_t>(M);
	fw.mark = carve.take<int32_t>(M);
	ExtractCarve xc = carve_extract_scratch(carve, M, NQ);
	carve_chain_runs(carve, M, kChainSerialRun, fw);         // longer runs get a wavefront each (k_chain_fwd_wave)
	xc.out_a = carve.take<uint64_t>(M), xc.out_u = carve.take<uint64_t>(M);
	carve_extract_counts(carve, NQ, xc);
	// (the sift's staging sits at the front of this block: if the block has to move, k_sift_copy must have read it first)
	if (carve.at > B.x_all.cap) HIP_TRY(wait_stream(ctx, s));
	if ((rc = B.x_all.ensure(carve.at))) return rc;
	char *X = B.x_all.as<char>();
	const unsigned nblk = (unsigned)((n2 + 255) / 256);
	const int64_t *d_first = B.pf_qfirst2.as<int64_t>();       // first kept anchor of every query (k_sift_offsets)
	HIP_TRY(hipMemsetAsync(xc.status.in(X), 0, xc.status.bytes() + 16, s));
	HIP_TRY(hipMemsetAsync(fw.n_runs.in(X), 0, fw.n_runs.bytes(), s));
	hipLaunchKernelGGL(k_sift_anchors, dim3(nblk), dim3(256), 0, s, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>(), n2, nb, v_a.in(X), v_pos.in(X));
	if ((rc = chain_fwd_launch(s, v_a.in(X), n2, d_first, nullptr, n_query, pm, kChainSerialRun, fw.in(X, xc)))) return rc;
	const ChainViewDev view{ d_first, nullptr, F.d_qfirst, v_pos.in(X), v_f.in(X), v_pred.in(X), v_a.in(X) };
	const int32_t *h_status = nullptr;
	if ((rc = chain_extract_pack(ctx, s, X, xc, view, mainp, n_query, H, nullptr, nullptr, ChainTailOut{ out.a_first, out.u_first, out.A, out.U }, &h_status, regions))) return rc;
	out.has_chains = true;
	seed_mark_on_host(out, n_query, h_status, F.h_flag);       // (the sift's hand-backs are in out.on_host already: dev_sift_front)
	timing_note("    seed: copy + main chain on the device", now_ms() - F.t_sift);
	return MPA_OK;
}

// GPU seeding for one mini-batch: anchors -> sort -> forward pass of the pre-chain -> the anchors that have a neighbour.
// jobs: the kept seeds of all queries (qid ascending, within a query ascending query position, dst = running anchor
// offset); qfirst[n_query + 1]: first anchor of every query.  out: per query a sparse ChainView's arrays
// (pred = index into the query's part of the view, -1 for none).
// pre_p == nullptr: the direct route (dev_seed_direct) -- no pre-chain, the sift keeps by the reach of the main chain *main
static int dev_seed_entry(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams *pre_p, int32_t n_query, const int64_t *qfirst,
                          const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, const ChainParams *main, SeedHold *hold, const int64_t *jfirst_dev, SiftKept *kept,
                          const RegionsParams *regions)
{
	const int64_t n = qfirst[n_query];
	out.cfirst.assign((size_t)n_query + 1, 0);
	out.pos = out.f = out.pred = nullptr, out.a = nullptr, out.m = 0, out.on_host.clear();
	out.has_chains = false, out.U = out.A = nullptr, out.u_first.clear(), out.a_first.clear();
	out.has_regions = false, out.R = nullptr, out.E = nullptr, out.n_reg = nullptr;
	if (!pre_p) {                                              // (no anchors: no chains -- the planners take that from the device's result like any other)
		out.has_chains = !kept, out.u_first.assign((size_t)n_query + 1, 0), out.a_first.assign((size_t)n_query + 1, 0);
		if (kept) kept->first.assign((size_t)n_query + 1, 0), kept->a.clear(), kept->flag.assign((size_t)n_query, 0);
	}
	if (n == 0 || n_jobs == 0) return MPA_OK;
	const ChainParams &pre = pre_p ? *pre_p : *main;
	if (pre.bbit <= 0) { set_error("GPU seeding needs block anchors (bbit > 0)"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	HIP_TRY(dev_index_table(ctx, d->kb, mi->kb.data(), mi->kb.size() * 4, "index upload: occurrence lists"));
	const PreParams pp = pre_params(pre);                      // (direct route: the main chain's parameters, as dev_chains_on_device derives them)
	int nb = 1, qb = 1;
	while ((1ULL << nb) < (uint64_t)mi->n_block + (uint64_t)pp.max_dblock + 2) ++nb;
	while ((1LL << qb) < n_query) ++qb;
	if (nb + qb > 64) { set_error("GPU pre-chain: too many queries x blocks for a 64-bit key"); return MPA_ERR_UNSUPPORTED; }
	if (pre_p && pp.max_dblock != 1) { set_error("GPU seeding: the sift assumes a pre-chain that reaches one block"); return MPA_ERR_UNSUPPORTED; }
	{	// the working set is ~60 bytes per anchor (sift: 16 of staging, the rest sized by the kept ones); a batch that does not fit
		// stays on the host (the caller falls back).  Direct route: the staging is full -- 16 B per anchor where the halved one takes 8 --
		// and the rule keeps every second anchor or more, 36 B each, before the chaining block is carved: 56 B per anchor
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			const SeedBufs &Bc = ctx->seed;
			const size_t have = Bc.f.cap + Bc.pred.cap + Bc.mark.cap + Bc.flag.cap + Bc.idx.cap + Bc.tmp.cap + Bc.x_all.cap + Bc.dkey.cap + Bc.val64[0].cap;
			if ((size_t)n * (pre_p ? 40 : 56) > have + free_b - (free_b >> 3)) { set_error("GPU seeding: batch too large for device memory"); return MPA_ERR_UNSUPPORTED; }
		}
	}
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const double t_begin = now_ms();
	// ---- upload the seed jobs (jfirst_dev: dev_sketch_jobs of this context has left them in B.jobs)
	if (!jfirst_dev) {
		if (B.h_jobs.ensure((size_t)n_jobs * sizeof(SeedJobDev)) != MPA_OK) return MPA_ERR_HIP;
		SeedJobDev *hj = B.h_jobs.as<SeedJobDev>();
		for (int64_t i = 0; i < n_jobs; ++i) hj[i] = SeedJobDev{ jobs[i].kb_off, jobs[i].dst, jobs[i].cnt, jobs[i].qpos, jobs[i].qid, 0 };
		if (B.jobs.ensure((size_t)n_jobs * sizeof(SeedJobDev)) != MPA_OK) return MPA_ERR_HIP;
		HIP_TRY(hipMemcpyAsync(B.jobs.p, hj, (size_t)n_jobs * sizeof(SeedJobDev), hipMemcpyHostToDevice, s));
	}
	// merge the occurrence lists per query in block order, keep what has a neighbour (k_seed_sift, seed_exec.hip)
	tl_alloc_failed = false;
	RegionsTail rtail;
	RegionsTail *const rt = regions_tail_begin(ctx, mi, main && !kept ? regions : nullptr, rtail);
	const int rc = pre_p ? dev_prechain_forward_sift(ctx, d, mi->n_block, pp, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, &pre, main, hold ? *hold : B.own, jfirst_dev, rt)
	                     : dev_seed_direct_impl(ctx, d, mi->n_block, pp, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, *main, hold ? *hold : B.own, jfirst_dev, kept, rt);
	if (rc == MPA_OK) regions_tail_end(rt, out);
	// a pool that could not grow (the admission check above is an estimate): the batch is seeded on the host, as for any batch
	// that does not fit -- nothing has been handed to the caller yet
	if (rc == MPA_ERR_HIP && tl_alloc_failed) { (void)hipStreamSynchronize(s); return MPA_ERR_UNSUPPORTED; }
	return rc;
}
int dev_prechain_forward(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &pre, int32_t n_query, const int64_t *qfirst,
                         const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, const ChainParams *main, SeedHold *hold, const int64_t *jfirst_dev, const RegionsParams *regions)
{
	return dev_seed_entry(ctx, mi, &pre, n_query, qfirst, jobs, n_jobs, out, main, hold, jfirst_dev, nullptr, regions);
}
// Seeding without a pre-chain (-S, --no-pre-chain; MPA_GPU_SEED_NOPRE): sift by the main chain's reach, then the main chain itself
// (dev_seed_direct_impl).  Same contract as dev_prechain_forward(main != nullptr): out.has_chains, out.on_host.  kept != nullptr
// (test hook): stop behind the sift and hand out the kept anchors instead.
int dev_seed_direct(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &mainp, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs, int64_t n_jobs,
                    PrechainSparse &out, SeedHold *hold, const int64_t *jfirst_dev, SiftKept *kept, const RegionsParams *regions)
{
	return dev_seed_entry(ctx, mi, nullptr, n_query, qfirst, jobs, n_jobs, out, &mainp, hold, jfirst_dev, kept, regions);
}

static int dev_sketch_jobs_impl(mpa_ctx_t *ctx, mpa_idx_s *mi, DeviceIndex *d, int32_t max_occ, const mpa_qbatch_t *q, SketchResult &out)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	const int32_t n_query = q->n_seq;
	const int64_t base = q->q_off[0], L = q->q_off[n_query] - base;
	const size_t NQ = (size_t)n_query;
	// one pinned block up, packed: residue table | q_off (from 0) | protein text
	Carve up(1), cnt(1), res8(1), res(16);
	const auto u_tab = up.take<uint8_t>(256); const auto u_qo = up.take<int64_t>(NQ + 1); const auto u_tx = up.take<uint8_t>((size_t)L);
	const size_t up_bytes = up.at + 16;
	// k_q: anchors and seeds per query | the results, as they come down: qfirst | jfirst | cut-offs | flags (the last two in 16-byte sections)
	const auto q_na = cnt.take<int64_t>(NQ + 1), q_nk = cnt.take<int64_t>(NQ + 1), r_qfirst = res8.take<int64_t>(NQ + 1), r_jfirst = res8.take<int64_t>(NQ + 1);
	res.skip(res8.at);
	const auto r_mo = res.take<int32_t>(NQ), r_flag = res.take<int32_t>(NQ);
	int rc;
	if ((rc = B.h_kin.ensure(up_bytes)) || (rc = B.k_in.ensure(up_bytes)) || (rc = B.k_cnt.ensure((size_t)L * 4 + 16)) || (rc = B.k_bkt.ensure((size_t)L * 4 + 16)) ||
	    (rc = B.k_q.ensure(cnt.at + res.at)) || (rc = B.h_kout.ensure(res.at)) || (rc = B.jobs.ensure(((size_t)L + 1) * sizeof(SeedJobDev)))) return rc;   // (a position ends at most one seed)
	char *hu = B.h_kin.as<char>();
	memcpy(u_tab.in(hu), tab_aa13(), 256);
	{ int64_t *qo = u_qo.in(hu); for (int32_t i = 0; i <= n_query; ++i) qo[i] = q->q_off[i] - base; }
	if (L > 0) memcpy(u_tx.in(hu), q->seqs + base, (size_t)L);
	HIP_TRY(hipMemcpyAsync(B.k_in.p, hu, up.at, hipMemcpyHostToDevice, s));
	const char *din = B.k_in.as<char>();
	char *dq = B.k_q.as<char>(), *dres = dq + cnt.at;
	int64_t *d_na = q_na.in(dq), *d_nk = q_nk.in(dq), *d_qfirst = r_qfirst.in(dres), *d_jfirst = r_jfirst.in(dres);
	int32_t *d_mo = r_mo.in(dres), *d_flag = r_flag.in(dres);
	SketchParams sp;
	sp.n_bucket = (int64_t)mi->ki.size(), sp.n_kb = mi->n_kb, sp.kmer = mi->opt.kmer, sp.mod_bit = mi->opt.mod_bit, sp.max_occ = max_occ, sp.pad = 0;
	const unsigned nwg = (unsigned)((n_query + SKETCH_WAVES - 1) / SKETCH_WAVES);
	hipLaunchKernelGGL(k_sketch_count, dim3(nwg), dim3(64 * SKETCH_WAVES), 0, s, u_tx.in(din), u_qo.in(din), n_query, u_tab.in(din),
	                   (const int64_t*)d->ki, sp, B.k_cnt.as<int32_t>(), B.k_bkt.as<uint32_t>(), d_na, d_nk, d_mo, d_flag);
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, (const int64_t*)d_na, (const int64_t*)d_nk, n_query, d_qfirst, d_jfirst);
	hipLaunchKernelGGL(k_sketch_emit, dim3(nwg), dim3(64 * SKETCH_WAVES), 0, s, u_qo.in(din), n_query, (const int64_t*)d->ki, B.k_cnt.as<int32_t>(),
	                   B.k_bkt.as<uint32_t>(), (const int64_t*)d_qfirst, (const int64_t*)d_jfirst, (const int32_t*)d_mo, (const int32_t*)d_flag, B.jobs.as<SeedJobDev>());
	HIP_TRY(hipGetLastError());
	// the results: contiguous on the device, one copy, one wait
	const char *hd = B.h_kout.as<char>();
	HIP_TRY(hipMemcpyAsync(B.h_kout.p, dres, res.at, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	out.qfirst = r_qfirst.in(hd), out.jfirst = r_jfirst.in(hd), out.max_occ = r_mo.in(hd), out.flag = r_flag.in(hd);
	out.n_anchor = out.qfirst[n_query], out.n_jobs = out.jfirst[n_query];
	for (int32_t i = 0; i < n_query; ++i) out.n_flagged += out.flag[i] != 0;
	return MPA_OK;
}

// The sketch stage of a mini-batch on the device (sketch_exec.hip): protein text up, the seed jobs of every query left in the
// seeder context's B.jobs for dev_prechain_forward(jfirst_dev), the two prefix arrays, cut-offs and flags back.  out points into
// pinned memory of the context, valid until its next sketch.  MPA_ERR_UNSUPPORTED: the caller runs the host stage.
int dev_sketch_jobs(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t max_occ, const mpa_qbatch_t *q, SketchResult &out)
{
	out = SketchResult();
	const mpa_idxopt_t &io = mi->opt;
	if (q->n_seq <= 0) { set_error("GPU sketch: an empty batch"); return MPA_ERR_UNSUPPORTED; }
	if (io.kmer < 1 || io.kmer > 7) { set_error("GPU sketch: k-mers of 1..7 residues only"); return MPA_ERR_UNSUPPORTED; }
	if (io.mod_bit < 0 || io.mod_bit >= 4 * io.kmer || mi->ki.size() != (size_t)1 << (4 * io.kmer - io.mod_bit)) { set_error("GPU sketch: the index has no k-mer table of 2^(4k - M) buckets"); return MPA_ERR_UNSUPPORTED; }
	if (q->q_off[q->n_seq] - q->q_off[0] >= (int64_t)INT32_MAX) { set_error("GPU sketch: too many seeds in a batch for 32-bit job indices"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	// ki[] next to kb[] in HBM, on the first device sketch of a device.  The host array may be a misaligned view into a mapped .mpi:
	// it is only ever copied byte-wise.  No device memory for it: the caller sketches on the host.
	const hipError_t e = dev_index_table(ctx, d->ki, (const void*)mi->ki.data(), mi->ki.size() * 8, "index upload: bucket offsets");
	if (e == hipErrorOutOfMemory) { set_error("GPU sketch: no device memory for the bucket offsets"); return MPA_ERR_UNSUPPORTED; }
	if (e != hipSuccess) { set_error(std::string("GPU sketch: uploading the bucket offsets: ") + hipGetErrorString(e)); return MPA_ERR_HIP; }
	ensure_seed_stream(ctx);
	tl_alloc_failed = false;
	const int rc = dev_sketch_jobs_impl(ctx, mi, d, max_occ, q, out);
	if (rc == MPA_ERR_HIP && tl_alloc_failed) { (void)hipStreamSynchronize(ctx->seed_stream); out = SketchResult(); return MPA_ERR_UNSUPPORTED; }   // (a pool could not grow: host stage)
	return rc;
}

// test hook (mpa_dbg_seed_jobs): the first n_jobs records of B.jobs, and the bucket that rides in their pad field
int dev_sketch_fetch(mpa_ctx_t *ctx, int64_t n_jobs, SeedJob *jobs, int32_t *bucket)
{
	if (n_jobs <= 0) return MPA_OK;
	SeedBufs &B = ctx->seed;
	if ((size_t)n_jobs * sizeof(SeedJobDev) > B.jobs.cap) { set_error("dev_sketch_fetch: more jobs than the context holds"); return MPA_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<SeedJobDev> h((size_t)n_jobs);
	HIP_TRY(hipMemcpyAsync(h.data(), B.jobs.p, (size_t)n_jobs * sizeof(SeedJobDev), hipMemcpyDeviceToHost, ctx->seed_stream));
	HIP_TRY(wait_stream(ctx, ctx->seed_stream));
	for (int64_t i = 0; i < n_jobs; ++i) {
		const SeedJobDev &j = h[(size_t)i];
		jobs[i] = SeedJob{ j.kb_off, j.dst, j.cnt, j.qpos, j.qid }, bucket[i] = j.pad;
	}
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// Forward pass of mp_chain for a batch of chaining problems on the device (k_chain_fwd): the main chain of every query of a
// mini-batch, or the refinement chains of its regions.  The caller writes the sorted anchors of all problems, back to back,
// into io.a (pinned memory of the context) and finds f / pred (index inside the problem) in io.f / io.pred afterwards.
int dev_chain_buffers(mpa_ctx_t *ctx, int64_t n, ChainIO &io)
{
	SeedBufs &B = ctx->seed;
	int rc;
	if ((rc = B.hc_a.ensure((size_t)n * 8 + 64)) || (rc = B.hc_f.ensure((size_t)n * 4 + 64)) || (rc = B.hc_pred.ensure((size_t)n * 4 + 64))) return rc;
	io.a = B.hc_a.as<uint64_t>(), io.f = B.hc_f.as<int32_t>(), io.pred = B.hc_pred.as<int32_t>();
	return MPA_OK;
}

int dev_chain_forward(mpa_ctx_t *ctx, const ChainParams &cp, int32_t n_prob, const int64_t *first, const ChainIO &io)
{
	const int64_t n = first[n_prob];
	if (n == 0 || n_prob == 0) return MPA_OK;
	if (n_prob > (1 << 30) || cp.kmer < 0) { set_error("chain forward pass: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	for (int32_t q = 0; q < n_prob; ++q)
		if (first[q + 1] - first[q] > INT32_MAX - 2) { set_error("chain forward pass: a problem has too many anchors"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const PreParams pp = pre_params(cp);
	int rc;
	if ((rc = B.c_a.ensure((size_t)n * 8)) || (rc = B.c_f.ensure((size_t)n * 4)) || (rc = B.c_pred.ensure((size_t)n * 4)) || (rc = B.c_mark.ensure((size_t)n * 4)) ||
	    (rc = B.c_flag.ensure((size_t)n * 4)) || (rc = B.c_first.ensure(((size_t)n_prob + 1) * 8))) return rc;
	// runs longer than this get a wavefront each (k_chain_fwd_wave); MPA_CHAIN_SERIAL_RUN overrides (tests: 4 = almost every run)
	const int32_t serial_run = [] { const char *e = getenv("MPA_CHAIN_SERIAL_RUN"); return e ? std::max(1, atoi(e)) : kChainSerialRun; }();
	Carve lc(1);                                             // c_long, packed: the counter's 64 bytes | the list
	const auto p_nlong = lc.take<unsigned int>(16); const auto p_long = lc.take<LongRun>((size_t)n / (size_t)(serial_run + 1) + 16);
	const size_t long_cap = p_long.n;
	if ((rc = B.c_long.ensure(lc.at))) return rc;
	unsigned int *d_nlong = p_nlong.in(B.c_long.p); LongRun *d_long = p_long.in(B.c_long.p);
	HIP_TRY(hipMemsetAsync(d_nlong, 0, p_nlong.bytes(), s));
	HIP_TRY(hipMemcpyAsync(B.c_a.p, io.a, (size_t)n * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(B.c_first.p, first, ((size_t)n_prob + 1) * 8, hipMemcpyHostToDevice, s));
	if ((rc = chain_fwd_launch(s, B.c_a.as<uint64_t>(), n, B.c_first.as<int64_t>(), nullptr, n_prob, pp, serial_run,
	                           ChainFwdBufs{ B.c_f.as<int32_t>(), B.c_pred.as<int32_t>(), B.c_mark.as<int32_t>(), B.c_flag.as<uint32_t>(), d_long, d_nlong, long_cap }))) return rc;
	HIP_TRY(hipMemcpyAsync(io.f, B.c_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(io.pred, B.c_pred.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));                       // (first[] may be pageable memory of the caller: it is consumed by now)
	return MPA_OK;
}

// Test hook (mpa_dbg_chain_extract, chain_dbg.cpp): k_chain_extract over views the caller has made on the host -- vfirst[n_prob + 1] their
// offsets; sparse views with v_pos and ntot_first, dense ones with both null -- through what every chaining route goes through: the
// carving of the scratch in the context's chaining pool (which keeps whatever the last call left in it), the status memset, and
// chain_extract_launch (set_only: the kept anchors as a set) or chain_extract_pack (the chains, packed by k_offsets2 + k_chain_pack).
// u / a_out: room for vfirst[n_prob] words; off_u / off_a [n_prob + 1]; status[n_prob].
int dev_chain_extract_dbg(mpa_ctx_t *ctx, const ChainParams &p, int32_t n_prob, const int64_t *vfirst, const int64_t *ntot_first, const int32_t *v_pos, const int32_t *v_f,
                          const int32_t *v_pred, const uint64_t *v_a, int32_t set_only, int64_t *off_u, uint64_t *u, int64_t *off_a, uint64_t *a_out, int32_t *status)
{
	for (int32_t q = 0; q <= n_prob; ++q) off_u[q] = off_a[q] = 0;
	for (int32_t q = 0; q < n_prob; ++q) status[q] = 0;
	const int64_t m = vfirst[n_prob];
	if (n_prob == 0 || m == 0) return MPA_OK;                  // (no view, no launch: as in every route)
	HIP_TRY(hipSetDevice(ctx->device));
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const size_t M = (size_t)m, NP = (size_t)n_prob;
	Carve carve;
	const auto x_first = carve.take<int64_t>(NP + 1), x_ntot = carve.take<int64_t>(NP + 1); const auto x_pos = carve.take<int32_t>(M), x_f = carve.take<int32_t>(M), x_pred = carve.take<int32_t>(M);
	const auto x_a = carve.take<uint64_t>(M);
	ExtractCarve xc = carve_extract_scratch(carve, M, NP);
	xc.out_a = carve.take<uint64_t>(M), xc.out_u = carve.take<uint64_t>(M);
	carve_extract_counts(carve, NP, xc);
	int rc;
	if ((rc = B.x_all.ensure(carve.at))) return rc;
	char *X = B.x_all.as<char>();
	HIP_TRY(hipMemsetAsync(xc.status.in(X), 0, xc.status.bytes() + 16, s));
	HIP_TRY(hipMemcpyAsync(x_first.in(X), vfirst, x_first.bytes(), hipMemcpyHostToDevice, s));
	if (ntot_first) HIP_TRY(hipMemcpyAsync(x_ntot.in(X), ntot_first, x_ntot.bytes(), hipMemcpyHostToDevice, s));
	if (v_pos) HIP_TRY(hipMemcpyAsync(x_pos.in(X), v_pos, x_pos.bytes(), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(x_f.in(X), v_f, x_f.bytes(), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(x_pred.in(X), v_pred, x_pred.bytes(), hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(x_a.in(X), v_a, x_a.bytes(), hipMemcpyHostToDevice, s));
	const ChainViewDev view{ x_first.in(X), nullptr, ntot_first ? x_ntot.in(X) : nullptr, v_pos ? x_pos.in(X) : nullptr, x_f.in(X), x_pred.in(X), x_a.in(X) };
	if (set_only) {
		if ((rc = chain_extract_launch(ctx, s, X, xc, view, p, n_prob, 1, nullptr))) return rc;
		std::vector<int64_t> na(NP);
		std::vector<int32_t> st(NP);
		std::vector<uint64_t> all(M);
		HIP_TRY(hipMemcpyAsync(na.data(), xc.na.in(X), NP * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(st.data(), xc.status.in(X), NP * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(all.data(), xc.out_a.in(X), M * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		for (size_t q = 0; q < NP; ++q) {
			const int64_t room = vfirst[q + 1] - vfirst[q];
			if (na[q] < 0 || na[q] > room) { set_error("dev_chain_extract_dbg: a problem reports more anchors than its view holds"); return MPA_ERR_HIP; }
			if (na[q] > 0) memcpy(a_out + off_a[q], all.data() + vfirst[q], (size_t)na[q] * 8);
			off_a[q + 1] = off_a[q] + na[q], status[q] = st[q];
		}
		return MPA_OK;
	}
	std::vector<int64_t> a_first, u_first;
	const uint64_t *A = nullptr, *U = nullptr;
	const int32_t *h_status = nullptr;
	if ((rc = chain_extract_pack(ctx, s, X, xc, view, p, n_prob, B.own, nullptr, nullptr, ChainTailOut{ a_first, u_first, A, U }, &h_status))) return rc;
	if (a_first[NP] < 0 || a_first[NP] > m || u_first[NP] < 0 || u_first[NP] > m) { set_error("dev_chain_extract_dbg: more chains than the views hold anchors"); return MPA_ERR_HIP; }
	for (size_t q = 0; q <= NP; ++q) off_a[q] = a_first[q], off_u[q] = u_first[q];
	for (size_t q = 0; q < NP; ++q) status[q] = h_status[q];
	if (a_first[NP] > 0) memcpy(a_out, A, (size_t)a_first[NP] * 8);
	if (u_first[NP] > 0) memcpy(u, U, (size_t)u_first[NP] * 8);
	return MPA_OK;
}
} // namespace mpa
