// host_hooks.cpp -- the test hooks of stage A that libmpamd.so exports (mpa_dbg_*, not in include/mpamd.h) and mpa_idx_bucket_counts:
// single steps of host_plan.cpp, on the host or on the device, in a form a test can compare with the reference's own functions.
#include <algorithm>
#include <cstring>
#include <memory>
#include "host_batch.h"

using namespace mpa;

// the rows of a hook's result back to back in one malloc'd block (mpa_free); off[n + 1] receives where each begins
static uint64_t *pack_rows(const std::vector<std::vector<uint64_t>> &per, int64_t *off)
{
	off[0] = 0;
	for (size_t i = 0; i < per.size(); ++i) off[i + 1] = off[i] + (int64_t)per[i].size();
	uint64_t *o = (uint64_t*)malloc((size_t)std::max<int64_t>(off[per.size()], 1) * 8);
	for (size_t i = 0; i < per.size(); ++i) if (!per[i].empty()) memcpy(o + off[i], per[i].data(), per[i].size() * 8);
	return o;
}

extern "C" {

// Test hook (not in include/mpamd.h): the refinement scan of n_win windows [as, as + len) on vid for ONE query, on the host
// (ctx == NULL: refine_seed_pairs' scan) or on the device (k_refine_scan).  first[n_win + 1] / *out (mpa_free): the hits
// (hash << 32 | window position) of every window, sorted.
int64_t mpa_dbg_refine_hits(mpa_ctx_t *ctx, const mpa_idx_t *mi, int32_t kmer, const char *aa, int32_t l_aa, int32_t n_win, const int32_t *vid, const int64_t *as,
                            const int32_t *len, int64_t *first, uint64_t **out)
{
	*out = nullptr;
	std::vector<std::vector<uint64_t>> per((size_t)n_win);
	if (ctx) {
		std::vector<RefineWindow> wins((size_t)n_win);
		for (int32_t k = 0; k < n_win; ++k) wins[k] = RefineWindow{ as[k], 0, vid[k], len[k] };
		std::vector<uint32_t> w;
		query_words(aa, l_aa, kmer, w);
		const int64_t qw_first[2] = { 0, (int64_t)w.size() };
		RefineHits rh;
		const int rc = dev_refine_scan(ctx, const_cast<mpa_idx_s*>(mi), kmer, mi->opt.min_aa_len, 1, qw_first, w.data(), n_win, wins.data(), rh);
		if (rc != MPA_OK) return rc;
		for (int32_t k = 0; k < n_win; ++k) per[k].assign(rh.hits.begin() + rh.first[k], rh.hits.begin() + rh.first[k + 1]);
	} else {
		RefineQuery rq(aa, l_aa, kmer);
		std::vector<uint8_t> nt;
		std::vector<uint64_t> a;
		for (int32_t k = 0; k < n_win; ++k) {
			nt.resize((size_t)std::max(len[k], 1));
			fetch_nt(mi, vid[k], as[k], as[k] + len[k], nt.data());
			if (rq.filter) { refine_seed_pairs(nt.data(), len[k], mi->opt.min_aa_len, kmer, rq.qk, rq.filter->data(), INT32_MAX, per[k], a); continue; }
			// large k (no bitmap of the query's words, as in refine_region_pairs): the reference's own sketch of the window, and of it
			// the k-mers whose hash the query has
			sketch_nt4(nt.data(), len[k], mi->opt.min_aa_len, kmer, 0, 0, 0, a, false);
			for (uint64_t x : a) {
				const auto it = std::lower_bound(rq.qk.begin(), rq.qk.end(), x >> 32 << 32);
				if (it != rq.qk.end() && *it >> 32 == x >> 32) per[k].push_back(x);
			}
		}
	}
	for (int32_t k = 0; k < n_win; ++k) std::sort(per[k].begin(), per[k].end());
	*out = pack_rows(per, first);
	return first[n_win];
}

// Operator-level entry point of the refinement chains: what mp_chain() returns at map.c:88 for n_win windows [as, as + len) on vid,
// each refined for query qid of the batch -- u = score << 32 | anchors per chain and the chains' anchors (window position << 32 |
// query position), off_u / off_a [n_win + 1] -- from dev_refine_chains (ctx != NULL) or from the host's refine_region_pairs +
// chain_anchors (ctx == NULL).  host_flag[n_win]: 1 = the device handed the window back (its chains are then empty here).
int64_t mpa_dbg_refine_chains(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_win, const int32_t *qid, const int32_t *vid,
                              const int64_t *as, const int32_t *len, int64_t *off_u, uint64_t **out_u, int64_t *off_a, uint64_t **out_a, uint8_t *host_flag)
{
	*out_u = *out_a = nullptr;
	for (int32_t k = 0; k < n_win; ++k) {
		if (qid[k] < 0 || qid[k] >= q->n_seq || vid[k] < 0 || vid[k] >= 2 * (int32_t)mi->ctg.size() || len[k] < 0 || as[k] < 0 || as[k] + len[k] > mi->ctg[vid[k] >> 1].len) {
			set_error("mpa_dbg_refine_chains: window " + std::to_string(k) + " is outside its contig or names no query");
			return MPA_ERR_ARG;
		}
		host_flag[k] = 0;
	}
	const ChainParams cp = refine_chain_params(*opt);
	std::vector<std::vector<uint64_t>> us((size_t)n_win), aa((size_t)n_win);
	if (ctx) {
		std::vector<QueryGroups> per((size_t)q->n_seq);
		for (int32_t i = 0; i < q->n_seq; ++i) query_groups(q->seqs + q->q_off[i], (int32_t)(q->q_off[i + 1] - q->q_off[i]), opt->kmer2, per[(size_t)i]);
		RefineGroupsHost G;
		gather_query_groups(per.data(), q->n_seq, G);
		std::vector<RefineWindow> wins((size_t)n_win);
		for (int32_t k = 0; k < n_win; ++k) wins[(size_t)k] = RefineWindow{ as[k], qid[k], vid[k], len[k] };
		RefineChains rc;
		const int r = dev_refine_chains(ctx, const_cast<mpa_idx_s*>(mi), opt->kmer2, mi->opt.min_aa_len, opt->max_ava, cp, q->n_seq, G, n_win, wins.data(), rc);
		if (r != MPA_OK) return r;
		for (int32_t k = 0; k < n_win; ++k) {
			host_flag[k] = rc.on_host[(size_t)k];
			if (rc.U) us[(size_t)k].assign(rc.U + rc.u_first[(size_t)k], rc.U + rc.u_first[(size_t)k + 1]);
			if (rc.A) aa[(size_t)k].assign(rc.A + rc.a_first[(size_t)k], rc.A + rc.a_first[(size_t)k + 1]);
		}
	} else {
		for (int32_t k = 0; k < n_win; ++k) {
			if (len[k] == 0) continue;
			// (one RefineQuery at a time: a thread has ONE bitmap of k-mer words, which the query that owns it clears when it goes)
			RefineQuery one(q->seqs + q->q_off[qid[k]], (int32_t)(q->q_off[qid[k] + 1] - q->q_off[qid[k]]), opt->kmer2);
			Region r;
			r.vid = (uint32_t)vid[k], r.vs = as[k], r.ve = as[k] + len[k];
			refine_region_pairs(mi, *opt, one, r, 0, 0, nullptr, 0, aa[(size_t)k]);
			chain_anchors(cp, aa[(size_t)k], us[(size_t)k]);
		}
	}
	*out_u = pack_rows(us, off_u), *out_a = pack_rows(aa, off_a);
	return off_a[n_win];
}

// Test hook (not in include/mpamd.h): the anchors that survive the pre-chain (map.c:163-192), query by query, computed on the
// host (ctx == NULL) or with the device seeding stage (seed_exec.hip).  off[n_seq + 1] receives the offsets into *out
// (malloc'd, mpa_free).  Returns the total or a negative error code.
// Test hook: the anchors of every query as map.c:163-178 leaves them (block << 32 | query position, sorted) -- the INPUT of the
// reference's pre-chain call (map.c:188), so that a test can hand them to the real mp_chain().  off [n_seq + 1]; *out malloc'd.
int64_t mpa_dbg_anchors(const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, int64_t *off, uint64_t **out)
{
	*out = nullptr;
	mpa_mapopt_t o2 = *opt;
	o2.flag |= MPA_MF_NO_PRE_CHAIN;                       // (stage_anchors_host then stops after the sort)
	mpa_batch_t *b;
	{ SeedModeScope host_only(0); b = batch_seed_phase(nullptr, mi, &o2, q, n_threads, false); }
	if (!b) return MPA_ERR_ARG;
	std::vector<std::vector<uint64_t>> per((size_t)q->n_seq);
	parallel_for(b->n_threads, q->n_seq, [&](int64_t i) { stage_anchors_host(b, b->qs[i], per[i]); });
	*out = pack_rows(per, off);
	delete b;
	return off[q->n_seq];
}

// Test hook: the kept seeds of every query (map.c:152-170) as (query position, bucket, occurrences) triples in job order and the
// occurrence cut-off in force per query, from the host stage (ctx == NULL: stage_seeds) or from the device stage (sketch_exec.hip:
// a download of the jobs it left for k_seed_sift, whose kb_off / dst / qid fields are checked here against ki[] and the prefix
// arrays).  off[n_seq + 1]: triples before every query; max_occ[n_seq]; *out malloc'd (mpa_free).  Returns the number of queries the
// device handed to the host (their triples are the host's), or a negative error code.
int64_t mpa_dbg_seed_jobs(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, int64_t *off, int32_t *max_occ, int32_t **out)
{
	*out = nullptr;
	return mpa::guarded<int64_t>((int64_t)MPA_ERR_HIP, [&]() -> int64_t {
		mpa_batch_s *b = batch_shell(mi, opt, q, n_threads);
		if (!b) return MPA_ERR_ARG;
		std::unique_ptr<mpa_batch_s> own(b);
		const int32_t n = q->n_seq;
		const int64_t n_bucket = (int64_t)mi->ki.size();
		SketchResult sk;
		std::vector<SeedJob> jobs;
		std::vector<int32_t> bucket;
		if (ctx && n > 0) {
			int rc = dev_sketch_jobs(ctx, const_cast<mpa_idx_s*>(mi), opt->max_occ, q, sk);
			if (rc != MPA_OK) return rc;
			jobs.resize((size_t)sk.n_jobs), bucket.resize((size_t)sk.n_jobs);
			if ((rc = dev_sketch_fetch(ctx, sk.n_jobs, jobs.data(), bucket.data())) != MPA_OK) return rc;
		}
		parallel_for(b->n_threads, n, [&](int64_t i) { if (!ctx || sk.flag[i]) stage_seeds(b, b->qs[i]); });
		off[0] = 0;
		for (int32_t i = 0; i < n; ++i) off[i + 1] = off[i] + (b->qs[i].seeds_ready ? (int64_t)b->qs[i].seeds.size() : sk.jfirst[i + 1] - sk.jfirst[i]);
		int32_t *o = (int32_t*)malloc((size_t)std::max<int64_t>(off[n], 1) * 12);
		if (!o) { set_error("out of host memory"); return MPA_ERR_ARG; }
		for (int32_t i = 0; i < n; ++i) {
			int32_t *t = o + 3 * off[i];
			const QueryState &qs = b->qs[i];
			if (qs.seeds_ready) {
				max_occ[i] = qs.max_occ;
				for (uint64_t kq : qs.seeds) {
					const int64_t bkt = (int64_t)(uint32_t)kq, st = mi->ki[bkt], en = bkt + 1 < n_bucket ? mi->ki[bkt + 1] : mi->n_kb;
					*t++ = (int32_t)(kq >> 32), *t++ = (int32_t)bkt, *t++ = (int32_t)(en - st);
				}
				continue;
			}
			max_occ[i] = sk.max_occ[i];
			int64_t dst = sk.qfirst[i];
			for (int64_t j = sk.jfirst[i]; j < sk.jfirst[i + 1]; ++j) {
				const SeedJob &s = jobs[(size_t)j];
				const int64_t bkt = (int64_t)(uint32_t)bucket[(size_t)j];
				if (bkt >= n_bucket || s.kb_off != mi->ki[bkt] || s.dst != dst || s.qid != i) {
					free(o);
					set_error("device seed job " + std::to_string(j) + " of query " + std::to_string(i) + ": kb_off / dst / qid differ from the index and the prefix arrays");
					return MPA_ERR_ARG;
				}
				*t++ = s.qpos, *t++ = (int32_t)bkt, *t++ = s.cnt;
				dst += s.cnt;
			}
			if (dst != sk.qfirst[i + 1]) { free(o); set_error("device seed jobs of query " + std::to_string(i) + ": their counts do not add up to qfirst"); return MPA_ERR_ARG; }
		}
		*out = o;
		return ctx ? (int64_t)sk.n_flagged : 0;
	});
}

// cnt[i] = occurrences of bucket[i] in the index's k-mer table (ki[b + 1] - ki[b]; n_kb closes the last bucket).  Host only.
int mpa_idx_bucket_counts(const mpa_idx_t *mi, int64_t n, const uint32_t *bucket, int64_t *cnt)
{
	const int64_t n_bucket = (int64_t)mi->ki.size();
	for (int64_t i = 0; i < n; ++i) {
		const int64_t b = (int64_t)bucket[i];
		if (b >= n_bucket) { set_error("mpa_idx_bucket_counts: bucket " + std::to_string(b) + " beyond the table"); return MPA_ERR_ARG; }
		cnt[i] = (b + 1 < n_bucket ? mi->ki[b + 1] : mi->n_kb) - mi->ki[b];
	}
	return MPA_OK;
}

int64_t mpa_dbg_prechain_survivors(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, int64_t *off, uint64_t **out)
{
	*out = nullptr;
	mpa_batch_t *b;
	{ SeedModeScope forced(ctx ? 1 : 0); b = batch_seed_phase(ctx, mi, opt, q, n_threads, false); }
	if (!b) return MPA_ERR_ARG;
	if (ctx && !b->seeded_on_device && q->n_seq > 0 && seed_route(*opt, mi->opt) == SEED_PRECHAIN) { delete b; set_error("device seeding was not used"); return MPA_ERR_UNSUPPORTED; }
	std::vector<std::vector<uint64_t>> per((size_t)q->n_seq);
	parallel_for(b->n_threads, q->n_seq, [&](int64_t i) {
		if (b->seeded_on_device) stage_anchors_from_device(b, b->qs[i], b->sparse, per[i]);
		else stage_anchors_host(b, b->qs[i], per[i]);
	});
	*out = pack_rows(per, off);
	delete b;
	return off[q->n_seq];
}

// Test hook (not in include/mpamd.h): the MAIN chains of every query (what mp_chain() returns at map.c:195: u = score << 32 |
// anchors per chain, a = the chains' anchors), from the host stages (ctx == NULL) or from the device, which runs both chaining
// rounds (k_chain_extract, k_chain_fwd).  off_u / off_a [n_seq + 1]; *out_u / *out_a malloc'd (mpa_free).  Returns the number of
// queries the device handed back to the host (>= 0) or a negative error code.
int64_t mpa_dbg_main_chains(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, int64_t *off_u, uint64_t **out_u,
                            int64_t *off_a, uint64_t **out_a)
{
	*out_u = *out_a = nullptr;
	mpa_batch_t *b;
	{ SeedModeScope forced(ctx ? 1 : 0); b = batch_seed_phase(ctx, mi, opt, q, n_threads, true); }
	if (!b) return MPA_ERR_ARG;
	if (ctx && q->n_seq > 0 && seed_route(*opt, mi->opt) != SEED_ON_HOST && !(b->seeded_on_device && b->sparse.has_chains)) { delete b; set_error("the device did not chain"); return MPA_ERR_UNSUPPORTED; }
	std::vector<std::vector<uint64_t>> us((size_t)q->n_seq), as((size_t)q->n_seq);
	const ChainParams cp = main_chain_params(mi, *opt);
	int64_t n_back = 0;
	for (int32_t i = 0; i < q->n_seq; ++i) {
		const PrechainSparse &ps = b->sparse;
		if (b->seeded_on_device && ps.has_chains && !(!ps.on_host.empty() && ps.on_host[(size_t)i])) {
			us[i].assign(ps.U + ps.u_first[(size_t)i], ps.U + ps.u_first[(size_t)i + 1]);
			as[i].assign(ps.A + ps.a_first[(size_t)i], ps.A + ps.a_first[(size_t)i + 1]);
			continue;
		}
		n_back += b->seeded_on_device ? 1 : 0;
		stage_anchors_host(b, b->qs[i], as[i]);
		chain_anchors(cp, as[i], us[i]);
	}
	*out_u = pack_rows(us, off_u), *out_a = pack_rows(as, off_a);
	delete b;
	return n_back;
}

// Test hook: what the sift of the direct route (SEED_DIRECT: k_seed_sift<4096, true>) keeps -- the anchors of every query that have
// another one of the query within reach = max(max_intron, bw) >> bbit blocks before or behind them in sorted order, all of them when
// reach > kSiftReachMax (15) -- in sorted order.  ctx == NULL: a plain host restatement of that rule over mpa_dbg_anchors().  off[n_seq + 1]; *out
// malloc'd (mpa_free); flag[n_seq]: 1 = the device's sift handed the query back (its anchors are not in *out); *reach: the reach in
// force.  Returns the total, or MPA_ERR_UNSUPPORTED where the direct route does not apply (MPA_GPU_SEED_NOPRE unset, a run with a
// pre-chain, options that rule out a sparse view).
int64_t mpa_dbg_sift_kept(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, int64_t *off, uint64_t **out, int32_t *flag, int32_t *reach)
{
	*out = nullptr;
	if (seed_route(*opt, mi->opt) != SEED_DIRECT) { set_error("mpa_dbg_sift_kept: the direct seeding route does not apply to this run"); return MPA_ERR_UNSUPPORTED; }
	const ChainParams cp = main_chain_params(mi, *opt);
	const int64_t D = std::max(cp.max_dist_x, cp.bw) >> cp.bbit;
	*reach = (int32_t)D;
	const int32_t n = q->n_seq;
	for (int32_t i = 0; i < n; ++i) flag[i] = 0;
	if (!ctx) {
		uint64_t *a = nullptr;
		std::vector<int64_t> a_off((size_t)n + 1, 0);
		const int64_t n_a = mpa_dbg_anchors(mi, opt, q, n_threads, a_off.data(), &a);
		if (n_a < 0) return n_a;
		uint64_t *o = (uint64_t*)malloc((size_t)std::max<int64_t>(n_a, 1) * 8);
		if (!o) { free(a); set_error("out of host memory"); return MPA_ERR_ARG; }
		int64_t k = 0;
		for (int32_t i = 0; i < n; ++i) {
			off[i] = k;
			for (int64_t j = a_off[(size_t)i]; j < a_off[(size_t)i + 1]; ++j) {
				const int64_t blk = (int64_t)(a[j] >> 32);
				const bool left = j > a_off[(size_t)i] && blk - (int64_t)(a[j - 1] >> 32) <= D, right = j + 1 < a_off[(size_t)i + 1] && (int64_t)(a[j + 1] >> 32) - blk <= D;
				if (D > kSiftReachMax || left || right) o[k++] = a[j];
			}
		}
		off[n] = k;
		free(a);
		*out = o;
		return k;
	}
	return mpa::guarded<int64_t>((int64_t)MPA_ERR_HIP, [&]() -> int64_t {
		mpa_batch_s *b = batch_shell(mi, opt, q, n_threads);
		if (!b) return MPA_ERR_ARG;
		std::unique_ptr<mpa_batch_s> own(b);
		{ SeedModeScope forced(1); batch_host_seeds(b, true); }
		SiftKept kept;
		kept.first.assign((size_t)n + 1, 0), kept.flag.assign((size_t)n, 0);
		if (!b->seed_jobs.empty()) {
			const int rc = dev_seed_direct(ctx, const_cast<mpa_idx_s*>(mi), cp, n, b->seed_qfirst.data(), b->seed_jobs.data(), (int64_t)b->seed_jobs.size(), b->sparse, nullptr, nullptr, &kept);
			if (rc != MPA_OK) return rc;
		}
		uint64_t *o = (uint64_t*)malloc(std::max<size_t>(kept.a.size(), 1) * 8);
		if (!o) { set_error("out of host memory"); return MPA_ERR_ARG; }
		if (!kept.a.empty()) memcpy(o, kept.a.data(), kept.a.size() * 8);
		for (int32_t i = 0; i <= n; ++i) off[i] = kept.first[(size_t)i];
		for (int32_t i = 0; i < n; ++i) flag[i] = kept.flag[(size_t)i];
		*out = o;
		return (int64_t)kept.a.size();
	});
}

// Test hook: the forward pass of mp_chain (chain.c:181-209) for n_prob chaining problems whose sorted anchors lie back to back
// in a[] (first[n_prob + 1] = boundaries): f / pred (index inside the problem, -1 = none) of every anchor, from the device
// kernel k_chain_fwd (ctx != NULL) or from the host pass that chain_anchors() runs (ctx == NULL).
int mpa_dbg_chain_forward(mpa_ctx_t *ctx, int32_t max_dist_x, int32_t max_dist_y, int32_t bw, int32_t max_skip, int32_t max_iter, float coef_log,
                          int32_t is_spliced, int32_t kmer, int32_t bbit, int32_t n_prob, const int64_t *first, const uint64_t *a, int32_t *f, int32_t *pred)
{
	const ChainParams p{ max_dist_x, max_dist_y, bw, max_skip, max_iter, 1, 0, coef_log, is_spliced, kmer, bbit };
	const int64_t n = first[n_prob];
	if (!ctx) {
		for (int32_t q = 0; q < n_prob; ++q) chain_forward(p, a + first[q], first[q + 1] - first[q], f + first[q], pred + first[q]);
		return MPA_OK;
	}
	ChainIO io;
	int rc = dev_chain_buffers(ctx, n, io);
	if (rc != MPA_OK) return rc;
	if (n > 0) memcpy(io.a, a, (size_t)n * 8);
	if ((rc = dev_chain_forward(ctx, p, n_prob, first, io)) != MPA_OK) return rc;
	if (n > 0) memcpy(f, io.f, (size_t)n * 4), memcpy(pred, io.pred, (size_t)n * 4);
	return MPA_OK;
}

} // extern "C"
