// refine_run.hip -- host drivers of the refinement stage on the device (mp_refine_reg, map.c:32-111): the window scan for the host's
// pairing (dev_refine_scan) and the whole refinement -- scan, pairing, sort, chains -- of a mini-batch (dev_refine_chains).  The unit
// of the refinement kernels (refine_kernels.hip); the chains of the pairs come from the seeding unit's chain tail (dev_ctx.h).
#include "dev_ctx.h"
#include "refine_kernels.hip"

namespace mpa {
// MPA_REFINE_GMAP_MIN: from how many entries (groups in dev_refine_chains, k-mers in dev_refine_scan) a query's k-mer table lives in
// device memory instead of LDS.  Unset = lds_max + 1, the first size the LDS classes do not take; a smaller number sends more
// queries there (1 = every query: the tests); "off" = none, and a batch with a longer query is declined.  Read on every call.
// Returns the threshold, or -1 for "off".
static int64_t refine_gmap_min(int64_t lds_max)
{
	const char *e = getenv("MPA_REFINE_GMAP_MIN");
	if (!e || !*e) return lds_max + 1;
	if (!strcmp(e, "off")) return -1;
	const long long v = atoll(e);
	return v < 1 ? lds_max + 1 : std::min<int64_t>(v, lds_max + 1);
}
// The tables of a call's long queries: slots per query (power of two >= 2 x entries, at least 1 024), their places in the pool.
struct GmapPlan {
	std::vector<int32_t> long_q;          // the queries that get a table
	std::vector<int64_t> desc;            // [n_query] first slot << 8 | log2 slots (0 for the others)
	int64_t n_slots = 0, max_entries = 0;
	void add(int32_t q, int64_t entries) {
		int lg = 10;
		while ((1LL << lg) < 2 * entries) ++lg;
		long_q.push_back(q), desc[(size_t)q] = n_slots << 8 | lg;
		n_slots += 1LL << lg, max_entries = std::max(max_entries, entries);
	}
};
// memset + build of the tables on stream s: d_first / d_words = the entries of every query on the device, d_long / d_desc = the plan
static int gmap_build(SeedBufs &B, hipStream_t s, const GmapPlan &gp, const int64_t *d_first, const uint32_t *d_words, const int32_t *d_long, const int64_t *d_desc)
{
	HIP_TRY(hipMemsetAsync(B.r_gmap.p, 0xff, (size_t)gp.n_slots * 8, s));
	const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (gp.max_entries + 255) / 256));
	for (size_t k = 0; k < gp.long_q.size(); k += 65535)            // (gridDim.y)
		hipLaunchKernelGGL(k_refine_gmap_build, dim3(gx, (unsigned)std::min<size_t>(65535, gp.long_q.size() - k)), dim3(256), 0, s, d_first, d_words, d_long + k, d_desc, B.r_gmap.as<uint32_t>());
	HIP_TRY(hipGetLastError());
	return MPA_OK;
}

// Refinement scan of a mini-batch's region windows on the device (k_refine_scan).  qw_first/qwords: the k-mer words
// of every query.  out.first[w] .. out.first[w+1]: the hits (hash << 32 | window position) of window w, unsorted.
// Windows of a query with more than 4 096 k-mers (MPA_REFINE_GMAP_MIN) go to a second launch that probes the query's table in
// device memory (k_refine_scan_gset).  MPA_ERR_UNSUPPORTED (the caller scans on the host): k too large.
int dev_refine_scan(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t n_query, const int64_t *qw_first, const uint32_t *qwords,
                    int64_t n_win, const RefineWindow *wins, RefineHits &out)
{
	out.first.assign((size_t)n_win + 1, 0);
	out.hits.clear();
	if (n_win == 0) return MPA_OK;
	static_assert(REFINE_HALO == kRefineHaloBases, "dev_refine_in_range() states the halo of the scan kernels");
	if (!dev_refine_in_range(kmer, min_aa_len)) { set_error("refinement scan: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	const int64_t gmin = refine_gmap_min(4096);
	GmapPlan gp;
	gp.desc.assign((size_t)n_query, 0);
	std::vector<uint8_t> q_used((size_t)n_query, 0);
	for (int64_t k = 0; k < n_win; ++k) if (wins[k].len > 0) q_used[(size_t)wins[k].qid] = 1;
	int64_t max_words = 0;                                     // ... of the queries whose set goes to LDS
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t nw = qw_first[q + 1] - qw_first[q];
		if (gmin > 0 && nw >= gmin) { if (q_used[(size_t)q]) gp.add(q, nw); }
		else max_words = std::max(max_words, nw);
	}
	int hs_log2 = 10;
	while ((1LL << hs_log2) < 2 * max_words) ++hs_log2;
	if (hs_log2 > 13) { set_error("refinement scan: query too long for the LDS k-mer set"); return MPA_ERR_UNSUPPORTED; }
	const size_t n_long = gp.long_q.size();
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	// windows, chunks, the queries' k-mer words: laid out in ONE pinned block and uploaded with one copy (pageable copies are
	// staged by the runtime, synchronously and spinning)
	int64_t n_pos = 0, n_chunk = 0;
	for (int64_t k = 0; k < n_win; ++k) n_pos += wins[k].len, n_chunk += (wins[k].len + REFINE_CHUNK - 1) / REFINE_CHUNK;
	if (n_chunk == 0) return MPA_OK;
	const unsigned long long cap = (unsigned long long)(n_pos / 64 + (1 << 20));   // ~0.04 % of the positions hit on random sequence
	const int64_t n_words = qw_first[n_query];
	Carve up(64);
	const auto u_win = up.take<RefineWindowDev>((size_t)n_win); const auto u_chunk = up.take<RefineChunk>((size_t)n_chunk); const auto u_qf = up.take<int64_t>((size_t)n_query + 1);
	const auto u_words = up.take<uint32_t>((size_t)n_words, 16); const auto u_gd = up.take<int64_t>((size_t)n_query + 1); const auto u_lq = up.take<int32_t>(n_long + 1);
	const size_t up_bytes = up.at;
	int rc;
	if ((rc = B.h_meta.ensure(up_bytes + 64)) || (rc = B.r_win.ensure(up_bytes)) || (rc = B.r_hits.ensure((size_t)cap * 16)) || (rc = B.r_count.ensure(16)) ||
	    (rc = B.h_back.ensure(64)) || (n_long && (rc = B.r_gmap.ensure((size_t)gp.n_slots * 8)))) return rc;
	char *hm = B.h_meta.as<char>();
	int64_t c_lds = 0;                                         // the chunks of the LDS launch come first, then those of the long queries' windows
	{
		RefineWindowDev *dw = u_win.in(hm);
		RefineChunk *ch = u_chunk.in(hm);
		int64_t c = 0;
		for (int pass = 0; pass < 2; ++pass) {
			for (int64_t k = 0; k < n_win; ++k) {
				if (pass == 0) dw[k] = RefineWindowDev{ wins[k].as, wins[k].qid, wins[k].vid, wins[k].len, 0 };
				if ((gp.desc[(size_t)wins[k].qid] != 0) != (pass == 1)) continue;
				for (int32_t st = 0; st < wins[k].len; st += REFINE_CHUNK) ch[c++] = RefineChunk{ (int32_t)k, st };
			}
			if (pass == 0) c_lds = c;
		}
		memcpy(u_qf.in(hm), qw_first, u_qf.bytes());
		memcpy(u_words.in(hm), qwords, u_words.bytes());
		memcpy(u_gd.in(hm), gp.desc.data(), (size_t)n_query * 8);
		if (n_long) memcpy(u_lq.in(hm), gp.long_q.data(), n_long * 4);
	}
	HIP_TRY(hipMemcpyAsync(B.r_win.p, hm, up_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.r_count.p, 0, 16, s));
	RefineTab rt;
	for (int c = 0; c < 64; ++c) rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, nullptr, mi->l_seq };
	const size_t lds = ((size_t)4 << hs_log2) + REFINE_CHUNK + 2 * REFINE_HALO;
	const char *dm = B.r_win.as<char>();
	if (c_lds > 0)
		hipLaunchKernelGGL(k_refine_scan, dim3((unsigned)c_lds), dim3(256), lds, s, dg, u_win.in(dm), u_chunk.in(dm), u_qf.in(dm), u_words.in(dm), rt, kmer, min_aa_len, hs_log2, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap);
	if (n_chunk > c_lds) {
		if ((rc = gmap_build(B, s, gp, u_qf.in(dm), u_words.in(dm), u_lq.in(dm), u_gd.in(dm)))) return rc;
		hipLaunchKernelGGL(k_refine_scan_gset, dim3((unsigned)(n_chunk - c_lds)), dim3(256), REFINE_CHUNK + 2 * REFINE_HALO, s, dg, u_win.in(dm),
		                   u_chunk.in(dm) + c_lds, rt, kmer, min_aa_len, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap,
		                   RefineGmap{ B.r_gmap.as<uint2>(), u_gd.in(dm) });
		if (timing_on()) fprintf(stderr, "[mpa-timing]     refine scan: global-set launch (%zu queries, %lld chunks)\n", n_long, (long long)(n_chunk - c_lds));
	}
	HIP_TRY(hipGetLastError());
	unsigned long long *h_n = B.h_back.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(h_n, B.r_count.p, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const unsigned long long n_hits = *h_n;
	if (n_hits > cap) { set_error("refinement scan: more hits than the buffer holds"); return MPA_ERR_UNSUPPORTED; }
	if (n_hits == 0) return MPA_OK;
	if ((rc = B.h_rhits.ensure((size_t)n_hits * 16)) != MPA_OK) return rc;
	HIP_TRY(hipMemcpyAsync(B.h_rhits.p, B.r_hits.p, (size_t)n_hits * 16, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	// group by window (counting sort)
	const uint4 *h = B.h_rhits.as<uint4>();
	for (unsigned long long k = 0; k < n_hits; ++k) ++out.first[(size_t)h[k].x + 1];
	for (int64_t k = 0; k < n_win; ++k) out.first[(size_t)k + 1] += out.first[(size_t)k];
	out.hits.resize((size_t)n_hits);
	std::vector<int64_t> at(out.first.begin(), out.first.end() - 1);
	for (unsigned long long k = 0; k < n_hits; ++k) out.hits[(size_t)at[h[k].x]++] = (uint64_t)h[k].z << 32 | h[k].y;
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// mp_refine_reg (map.c:32-96) for all windows of a mini-batch on the device: see the kernels in refine_kernels.hip ("Refinement
// pairing on the device") and the chain tail of seed_run.hip (k_chain_fwd / k_chain_fwd_wave / k_chain_extract).  MPA_ERR_UNSUPPORTED: outside the kernels' range
// (the caller refines on the host).  out.on_host[w] = 1: this window alone is the host's (2^22 bases or more, or a query with a
// position of 2^22 or more -- the sort key window << 44 | position << 22 | query position holds neither); its chains come back empty.
// A query with more groups than the largest LDS map takes (MPA_REFINE_GMAP_MIN) gets its map in device memory: a fourth launch.
int dev_refine_chains(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t max_ava, const ChainParams &cp, int32_t n_query, const RefineGroupsHost &G,
                      int64_t n_win, const RefineWindow *wins, RefineChains &out, const PlansRequest *plans)
{
	out.has_plans = false;
	out.u_first.assign((size_t)n_win + 1, 0), out.a_first.assign((size_t)n_win + 1, 0);
	out.U = out.A = nullptr;
	out.on_host.assign((size_t)n_win, 0);
	if (n_win == 0) return MPA_OK;
	if (!dev_refine_in_range(kmer, min_aa_len) || cp.bbit != 0) { set_error("device refinement: parameters outside the kernels' range"); return MPA_ERR_UNSUPPORTED; }
	if (n_win >= (1 << 20)) { set_error("device refinement: more than 2^20 windows in a batch"); return MPA_ERR_UNSUPPORTED; }
	const int64_t gmin = refine_gmap_min(2048);
	// which windows the device takes, and the size class of every query that has one: 0..2 = LDS map of 1 024 / 2 048 / 4 096 slots, 3 = map in device memory
	std::vector<uint8_t> q_far((size_t)n_query, 0);
	std::vector<int8_t> q_cls((size_t)n_query, -1);
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t g0 = G.qg_first[(size_t)q], g1 = G.qg_first[(size_t)q + 1];
		const size_t p0 = g0 < g1 ? G.gfirst[(size_t)g0] : 0, p1 = g0 < g1 ? (size_t)G.gfirst[(size_t)g1 - 1] + G.gcount[(size_t)g1 - 1] : 0;
		for (size_t k = p0; k < p1; ++k) if (G.qpos[k] >= (1u << 22)) { q_far[(size_t)q] = 1; break; }
	}
	GmapPlan gp;
	gp.desc.assign((size_t)n_query, 0);
	int64_t n_long_win = 0;
	for (int64_t k = 0; k < n_win; ++k) {
		const size_t q = (size_t)wins[k].qid;
		if (wins[k].len >= (1 << 22) || q_far[q]) { out.on_host[(size_t)k] = 1; continue; }
		if (q_cls[q] < 0) {
			const int64_t ng = G.qg_first[q + 1] - G.qg_first[q];
			if (gmin > 0 && ng >= gmin) q_cls[q] = 3, gp.add((int32_t)q, ng);
			else if (2 * ng > 4096) { set_error("device refinement: query too long for the LDS k-mer map"); return MPA_ERR_UNSUPPORTED; }
			else q_cls[q] = 2 * ng <= 1024 ? 0 : 2 * ng <= 2048 ? 1 : 2;
		}
		n_long_win += q_cls[q] == 3;
	}
	const size_t n_long = gp.long_q.size();
	// MPA_GPU_PLANS=1: the call carries on to the plans unless a window is the host's -- its region would come from another path
	if (plans)
		for (int64_t k = 0; k < n_win; ++k)
			if (out.on_host[(size_t)k]) {
				if (timing_on()) fprintf(stderr, "[mpa-timing]   device plans declined (a refinement window is the host's): chains to the host\n");
				plans = nullptr;
				break;
			}
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const double t0 = now_ms();
	// ---- one pinned block up: windows | chunks | wg_first | qg_first | gword | gfirst | gcount | qpos (| with plans: what k_plans
	// reads of the windows' regions and of the queries: PlansWindow records | first window and first residue of every query | tables | text)
	static const int n_super = [] { const char *e = getenv("MPA_REFINE_SUPER"); const int v = e ? atoi(e) : REFINE_SUPER; return v < 1 ? 1 : v > 16 ? 16 : v; }();
	int64_t n_pos = 0, n_chunk = 0, wg_total = 0;
	for (int64_t k = 0; k < n_win; ++k) {
		if (out.on_host[(size_t)k]) continue;
		n_pos += wins[k].len, n_chunk += (wins[k].len + n_super * REFINE_CHUNK - 1) / (n_super * REFINE_CHUNK);   // (a workgroup sweeps n_super chunks of its window)
	}
	if (n_chunk == 0) return MPA_OK;
	const unsigned long long cap = (unsigned long long)(n_pos / 64 + (1 << 20));
	const size_t n_group = G.gword.size(), n_qpos = G.qpos.size(), NW = (size_t)n_win, NQ = (size_t)n_query;
	const int64_t text0 = plans ? plans->q_off[0] : 0, text_bytes = plans ? plans->q_off[n_query] - text0 : 0;
	Carve up(64);
	const auto u_win = up.take<RefineWindowDev>(NW); const auto u_chunk = up.take<RefineChunk>((size_t)n_chunk); const auto u_wg = up.take<int64_t>(NW + 1), u_qg = up.take<int64_t>(NQ + 1);
	const auto u_gw = up.take<uint32_t>(n_group + 1), u_gf = up.take<uint32_t>(n_group + 1), u_gc = up.take<uint32_t>(n_group + 1), u_qp = up.take<uint32_t>(n_qpos + 1);
	const auto u_gd = up.take<int64_t>(NQ + 1); const auto u_lq = up.take<int32_t>(n_long + 1); const auto u_pw = up.take_if<PlansWindow>(plans, NW);
	const auto u_w0 = up.take_if<int64_t>(plans, NQ + 1), u_qo = up.take_if<int64_t>(plans, NQ + 1); const auto u_tab = up.take_if<uint8_t>(plans, ALN_TAB_BYTES), u_txt = up.take_if<uint8_t>(plans, (size_t)text_bytes, 16);
	const size_t up_bytes = up.at;
	int rc;
	int64_t cls_end[4] = { 0, 0, 0, 0 };                       // chunks of the windows whose query's map has 1 024 / 2 048 / 4 096 LDS slots, or lives in device memory, end here
	if ((rc = B.h_meta.ensure(up_bytes + 64)) || (rc = B.r_win.ensure(up_bytes)) || (rc = B.r_hits.ensure((size_t)cap * 16)) || (rc = B.r_count.ensure(16)) ||
	    (rc = B.h_back.ensure(256)) || (n_long && (rc = B.r_gmap.ensure((size_t)gp.n_slots * 8)))) return rc;
	char *hm = B.h_meta.as<char>();
	{
		RefineWindowDev *dw = u_win.in(hm);
		RefineChunk *ch = u_chunk.in(hm);
		int64_t *wg = u_wg.in(hm);
		for (int64_t k = 0; k < n_win; ++k) {
			dw[k] = RefineWindowDev{ wins[k].as, wins[k].qid, wins[k].vid, wins[k].len, 0 };
			wg[k] = wg_total;
			if (!out.on_host[(size_t)k]) wg_total += G.qg_first[(size_t)wins[k].qid + 1] - G.qg_first[(size_t)wins[k].qid];   // (a window of the host has no workgroup, no hits, no pairs: an empty problem)
		}
		wg[n_win] = wg_total;
		// the workgroups of a window, grouped by the size of its query's k-mer map (1 024 / 2 048 / 4 096 slots, or a table in device
		// memory): one launch per size, so that the windows of ordinary proteins take 13 KB of LDS per workgroup and not the 37 KB the
		// longest protein of the LDS classes needs
		int64_t c = 0;
		for (int cls = 0; cls < 4; ++cls) {
			for (int64_t k = 0; k < n_win; ++k) {
				if (out.on_host[(size_t)k] || q_cls[(size_t)wins[k].qid] != cls) continue;
				for (int32_t st = 0; st < wins[k].len; st += n_super * REFINE_CHUNK) ch[c++] = RefineChunk{ (int32_t)k, st };
			}
			cls_end[cls] = c;
		}
		memcpy(u_qg.in(hm), G.qg_first.data(), u_qg.bytes());
		if (n_group) memcpy(u_gw.in(hm), G.gword.data(), n_group * 4), memcpy(u_gf.in(hm), G.gfirst.data(), n_group * 4), memcpy(u_gc.in(hm), G.gcount.data(), n_group * 4);
		if (n_qpos) memcpy(u_qp.in(hm), G.qpos.data(), n_qpos * 4);
		memcpy(u_gd.in(hm), gp.desc.data(), NQ * 8);
		if (n_long) memcpy(u_lq.in(hm), gp.long_q.data(), n_long * 4);
		if (plans) {
			memcpy(u_pw.in(hm), plans->win, u_pw.bytes());
			memcpy(u_w0.in(hm), plans->win0, u_w0.bytes());
			int64_t *qo = u_qo.in(hm);
			for (size_t q = 0; q <= NQ; ++q) qo[q] = plans->q_off[q] - text0;
			uint8_t *tab = u_tab.in(hm);
			memcpy(tab + ALN_TAB_CODON, tab_codon(), 64), memcpy(tab + ALN_TAB_AA20, tab_aa20(), 256), memcpy(tab + ALN_TAB_MAT, plans->mat, 484);
			if (text_bytes > 0) memcpy(u_txt.in(hm), plans->text + text0, (size_t)text_bytes);
		}
	}
	// device tables: per (window, group) hit counts and per-window pair counts, zeroed
	Carve rc_tab;
	const auto r_wcnt = rc_tab.take<uint32_t>((size_t)wg_total + 1), r_wpairs = rc_tab.take<uint32_t>(NW + 2); const auto r_first = rc_tab.take<int64_t>(NW + 2);
	const size_t zero_bytes = rc_tab.at;
	if ((rc = B.rx_all.ensure(zero_bytes))) return rc;
	HIP_TRY(hipMemcpyAsync(B.r_win.p, hm, up_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.r_count.p, 0, 16, s));
	HIP_TRY(hipMemsetAsync(B.rx_all.p, 0, zero_bytes, s));
	RefineTab rt;
	for (int c = 0; c < 64; ++c) rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, nullptr, mi->l_seq };
	const char *dm = B.r_win.as<char>();
	RefineGroups gr{ u_qg.in(dm), u_gw.in(dm), u_gf.in(dm), u_gc.in(dm), u_qp.in(dm) };
	const int64_t *d_wg = u_wg.in(dm);
	char *R = B.rx_all.as<char>();
	uint32_t *d_wcnt = r_wcnt.in(R), *d_wpairs = r_wpairs.in(R); int64_t *d_first = r_first.in(R);
	HIP_TRY(ensure_dynamic_lds((const void*)k_refine_scan_map, ctx->device, 48 * 1024));
	for (int cls = 0; cls < 3; ++cls) {
		const int64_t c_first = cls ? cls_end[cls - 1] : 0, c_n = cls_end[cls] - c_first;
		if (c_n == 0) continue;
		const int hs = 10 + cls;
		const size_t lds = ((size_t)8 << hs) + 2 * (REFINE_CHUNK + 2 * REFINE_HALO);   // k-mer map, bases, codons
		hipLaunchKernelGGL(k_refine_scan_map, dim3((unsigned)c_n), dim3(256), lds, s, dg, u_win.in(dm), u_chunk.in(dm) + c_first, gr, d_wg, rt,
		                   kmer, min_aa_len, hs, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap, d_wcnt, (int32_t)n_super);
	}
	if (cls_end[3] > cls_end[2]) {                             // the long queries: their tables once per batch, then the scan that probes them (LDS: bases + codons)
		if ((rc = gmap_build(B, s, gp, gr.qg_first, gr.gword, u_lq.in(dm), u_gd.in(dm)))) return rc;
		hipLaunchKernelGGL(k_refine_scan_gmap, dim3((unsigned)(cls_end[3] - cls_end[2])), dim3(256), 2 * (REFINE_CHUNK + 2 * REFINE_HALO), s, dg, u_win.in(dm),
		                   u_chunk.in(dm) + cls_end[2], gr, d_wg, rt, kmer, min_aa_len, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap, d_wcnt, (int32_t)n_super,
		                   RefineGmap{ B.r_gmap.as<uint2>(), u_gd.in(dm) });
		if (timing_on()) fprintf(stderr, "[mpa-timing]     refine: global-map class (%zu queries, %lld windows)\n", n_long, (long long)n_long_win);
	}
	HIP_TRY(hipGetLastError());
	unsigned long long *h_n = B.h_back.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(h_n, B.r_count.p, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t n_hits = (int64_t)*h_n;
	if ((unsigned long long)n_hits > cap) { set_error("device refinement: more hits than the buffer holds"); return MPA_ERR_UNSUPPORTED; }
	timing_note("    refine: scan (wait)", now_ms() - t0);
	if (n_hits == 0) return MPA_OK;
	// ---- pairs: count, offsets, emit, sort, decode
	const double t1 = now_ms();
	if ((rc = B.r_chunk.ensure((size_t)n_hits * 4 + 16)) || (rc = B.r_words.ensure((size_t)n_hits * 8 + 16))) return rc;   // pairs per hit, and where they go
	uint32_t *d_pc = B.r_chunk.as<uint32_t>();
	uint64_t *d_po = B.r_words.as<uint64_t>();
	const unsigned nbh = (unsigned)((n_hits + 255) / 256);
	hipLaunchKernelGGL(k_refine_pair_count, dim3(nbh), dim3(256), 0, s, B.r_hits.as<uint4>(), n_hits, d_wg, d_wcnt, gr.gcount, max_ava, d_pc, d_wpairs);
	HIP_TRY(hipGetLastError());
	{
		auto in = rocprim::make_transform_iterator((const uint32_t*)d_pc, U32ToU64());
		auto inw = rocprim::make_transform_iterator((const uint32_t*)d_wpairs, U32ToU64());
		// (two scans behind one another share one sizing of the scratch, the larger one's: dev_exclusive_scan twice could grow the pool twice)
		size_t tb = 0, tb2 = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, d_po, (uint64_t)0, (size_t)n_hits, rocprim::plus<uint64_t>(), s));
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb2, inw, (uint64_t*)d_first, (uint64_t)0, NW + 1, rocprim::plus<uint64_t>(), s));
		if ((rc = B.tmp.ensure(std::max(tb, tb2) + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(B.tmp.p, tb, in, d_po, (uint64_t)0, (size_t)n_hits, rocprim::plus<uint64_t>(), s));
		HIP_TRY(rocprim::exclusive_scan(B.tmp.p, tb2, inw, (uint64_t*)d_first, (uint64_t)0, NW + 1, rocprim::plus<uint64_t>(), s));
	}
	int64_t *h_np = B.h_back.as<int64_t>() + 1;               // (h_back: the hit count | the pair count)
	HIP_TRY(hipMemcpyAsync(h_np, d_first + n_win, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t np = *h_np;
	if (np == 0) return MPA_OK;
	Carve kc(1);                                             // rx_keys, packed: the pair keys (two buffers of the sort) | the pairs as anchors
	const auto k_keys0 = kc.take<uint64_t>((size_t)np), k_keys1 = kc.take<uint64_t>((size_t)np), k_a = kc.take<uint64_t>((size_t)np);
	if ((rc = B.rx_keys.ensure(kc.at + 64))) return rc;
	uint64_t *keys0 = k_keys0.in(B.rx_keys.p), *keys1 = k_keys1.in(B.rx_keys.p), *d_a = k_a.in(B.rx_keys.p);
	hipLaunchKernelGGL(k_refine_pair_emit, dim3(nbh), dim3(256), 0, s, B.r_hits.as<uint4>(), n_hits, (const uint32_t*)d_pc, (const uint64_t*)d_po, gr, keys0);
	HIP_TRY(hipGetLastError());
	{
		int wbits = 1;
		while ((1LL << wbits) < n_win) ++wbits;
		if ((rc = dev_sort_keys(B.tmp, false, keys0, keys1, (size_t)np, 0u, (unsigned)(44 + wbits), s))) return rc;
	}
	const unsigned nbp = (unsigned)((np + 255) / 256);
	hipLaunchKernelGGL(k_refine_pair_decode, dim3(nbp), dim3(256), 0, s, (const uint64_t*)keys1, np, d_a);
	HIP_TRY(hipGetLastError());
	// ---- the chains of every window: forward pass (base resolution), extraction, pack
	const PreParams pm = pre_params(cp);
	const size_t M = (size_t)np;
	Carve xcarve;
	ExtractCarve xc = carve_extract_scratch(xcarve, M, NW);
	ChainFwdCarve fw{};
	fw.f = xcarve.take<int32_t>(M), fw.pred = xcarve.take<int32_t>(M), fw.mark = xcarve.take<int32_t>(M);
	xc.out_a = xcarve.take<uint64_t>(M), xc.out_u = xcarve.take<uint64_t>(M);
	carve_extract_counts(xcarve, NW, xc);
	carve_chain_runs(xcarve, M, kChainSerialRun, fw);
	if ((rc = B.x_all.ensure(xcarve.at))) return rc;
	char *X = B.x_all.as<char>();
	HIP_TRY(hipMemsetAsync(xc.status.in(X), 0, xc.status.bytes() + 16, s));
	HIP_TRY(hipMemsetAsync(fw.n_runs.in(X), 0, fw.n_runs.bytes(), s));
	if ((rc = chain_fwd_launch(s, (const uint64_t*)d_a, np, (const int64_t*)d_first, nullptr, (int32_t)n_win, pm, kChainSerialRun, fw.in(X, xc)))) return rc;
	const ChainViewDev view{ d_first, nullptr, nullptr, nullptr, fw.f.in(X), fw.pred.in(X), (const uint64_t*)d_a };
	PlansTail ptail;
	if (plans) {
		const DeviceIndex *d = mi->dev[ctx->device];
		ptail = PlansTail{ plans->p, n_query, u_pw.in(dm), u_w0.in(dm), u_qo.in(dm), u_txt.in(dm), u_tab.in(dm), (const uint8_t*)d->seq, (const int64_t*)d->ctg_off, (const int64_t*)d->ctg_len, false, nullptr, nullptr, nullptr, nullptr, nullptr };
	}
	if ((rc = chain_extract_pack(ctx, s, X, xc, view, cp, (int32_t)n_win, B.own, nullptr, "device refinement: a chain extraction needs the host",   // (dense views never do)
	                             ChainTailOut{ out.a_first, out.u_first, out.A, out.U }, nullptr, nullptr, plans ? &ptail : nullptr))) return rc;
	if (plans && ptail.done) out.has_plans = true, out.PR = ptail.R, out.PP = ptail.P, out.PT = ptail.T, out.PS = ptail.S, out.PN = ptail.N;
	timing_note("    refine: pairs + chains (wait)", now_ms() - t1);
	return MPA_OK;
}
} // namespace mpa
