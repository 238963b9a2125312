// chain_dbg.cpp -- mpa_dbg_chain_extract (include/mpamd_dbg.h), the test hook of the chain extraction on raw anchors: the forward pass, the
// views a device chaining route would hand k_chain_extract (dense, or sparse as mpa_dbg_prechain_sparse builds them), and the extraction
// itself -- on the device through the product's own carving and launch helpers (dev_chain_extract_dbg of seed_run.hip) or, without a
// context, through chain_extract_core<CoopSerial> with the work space the kernel gives a problem (ends_cap = m + 64).  Next to the chains
// it says which path of chain_core.h every problem takes (chain_path_record: derived from f / pred and the view, never read back from the
// kernel).  Built into libmpamd_dbg.so: the C ABI of libmpamd.so stays what it was.
#include <algorithm>
#include <cstring>
#include <vector>
#include "mpa_internal.h"
#include "host_core.h"
#include "chain_core.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

namespace mpa {
int dev_chain_extract_dbg(mpa_ctx_t *ctx, const ChainParams &p, int32_t n_prob, const int64_t *vfirst, const int64_t *ntot_first, const int32_t *v_pos, const int32_t *v_f,
                          const int32_t *v_pred, const uint64_t *v_a, int32_t set_only, int64_t *off_u, uint64_t *u, int64_t *off_a, uint64_t *a_out, int32_t *status);
}

namespace {
// Which way a view goes through chain_extract_core (the preconditions of sorted_chain_ends_sparse and the room the kernel gives the
// full list), and the sizes that decide between the branches behind them.  rec[MPA_DBG_CHAIN_REC].
void chain_path_record(const ChainParams &p, const ChainView &v, int64_t ends_cap, int64_t *rec)
{
	int64_t non_roots = 0, max_f = 0, hi = 0, big = 0;
	bool odd = false;
	std::vector<int64_t> cnt8(256, 0);
	for (int64_t i = 0; i < v.m; ++i) {
		if (v.pred[i] < 0) continue;
		++non_roots;
		if (v.f[i] <= p.kmer) odd = true;
		max_f = std::max<int64_t>(max_f, v.f[i]);
		if (v.f[i] >= 256) ++hi, ++cnt8[(size_t)(v.f[i] >> 8 & 0xff)];
	}
	for (int d = 1; d < 256; ++d) big = std::max(big, cnt8[(size_t)d]);
	int64_t why = 0;
	if (p.min_cnt <= 1) why |= MPA_DBG_CHAIN_WHY_MIN_CNT;
	if (p.min_sc > p.kmer) why |= MPA_DBG_CHAIN_WHY_MIN_SC;
	if (v.n_total <= 64) why |= MPA_DBG_CHAIN_WHY_SMALL;
	if (p.kmer < 0 || p.kmer > 255 || odd) why |= MPA_DBG_CHAIN_WHY_OTHER;
	if (!why && max_f >= 65536) why |= MPA_DBG_CHAIN_WHY_MAX_F;          // (only looked at when nothing in front of it sent the problem back)
	int64_t cls = MPA_DBG_CHAIN_ONE_LEVEL;
	if (why) cls = v.n_total > ends_cap ? MPA_DBG_CHAIN_DECLINED : MPA_DBG_CHAIN_FULL_LIST;
	else if (max_f >= 256) cls = MPA_DBG_CHAIN_TWO_LEVEL;
	rec[0] = v.m, rec[1] = v.n_total, rec[2] = non_roots, rec[3] = max_f, rec[4] = cls;
	rec[5] = max_f < 65536 ? v.n_total - hi : 0, rec[6] = max_f < 65536 ? big : 0, rec[7] = why;
}

// one problem through the shared source with a team of one, in work space of the kernel's sizes
int extract_on_host(const ChainParams &p, const ChainView &v, bool set_only, std::vector<uint64_t> &a_out, std::vector<uint64_t> &u)
{
	const size_t m = (size_t)v.m, cap = m + 64;
	std::vector<int32_t> mark(m), order(m);
	std::vector<Pair64> ends(cap), tail8(m), first(m);
	std::vector<SparseItem> items(m), moved(m), merged(m);
	std::vector<uint8_t> kept(m);
	std::vector<uint64_t> packed(m), u_sorted(m);
	std::vector<SortRange> stack(cap / 64 + 4);
	uint32_t hist[1280];
	const ExtractScratch S{ mark.data(), order.data(), ends.data(), (int64_t)cap, items.data(), moved.data(), merged.data(), tail8.data(), first.data(), kept.data(), packed.data(),
	                        u_sorted.data(), stack.data(), hist };
	a_out.assign(m, 0), u.assign(m, 0);
	int64_t n_a = 0, n_u = 0;
	const int rc = chain_extract_core<CoopSerial>(p, v, S, a_out.data(), &n_a, u.data(), &n_u, set_only);
	if (rc != 0) n_a = n_u = 0;
	a_out.resize((size_t)n_a), u.resize((size_t)n_u);
	return rc;
}
}

extern "C" int mpa_dbg_chain_extract(mpa_ctx_t *ctx, int32_t max_dist_x, int32_t max_dist_y, int32_t bw, int32_t max_skip, int32_t max_iter, int32_t min_cnt, int32_t min_sc,
                                     float coef_log, int32_t is_spliced, int32_t kmer, int32_t bbit, int32_t n_prob, const int64_t *first, const uint64_t *a, int32_t mode,
                                     int64_t *off_u, uint64_t *u, int64_t *off_a, uint64_t *a_out, int32_t *status, int64_t *rec)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&]() -> int {
		if (n_prob < 0 || !first || !off_u || !off_a || !status || !rec || mode < MPA_DBG_CHAIN_DENSE || mode > MPA_DBG_CHAIN_SPARSE_CHAINS) { set_error("mpa_dbg_chain_extract: missing arguments"); return MPA_ERR_ARG; }
		const int64_t n = first[n_prob];
		for (int32_t q = 0; q < n_prob; ++q)
			if (first[q + 1] < first[q] || first[q + 1] - first[q] > INT32_MAX - 2) { set_error("mpa_dbg_chain_extract: first[] is not a prefix of problem sizes"); return MPA_ERR_ARG; }
		if (first[0] != 0 || (n > 0 && (!a || !u || !a_out))) { set_error("mpa_dbg_chain_extract: missing arguments"); return MPA_ERR_ARG; }
		const ChainParams p{ max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, coef_log, is_spliced, kmer, bbit };
		const bool sparse = mode != MPA_DBG_CHAIN_DENSE, set_only = mode == MPA_DBG_CHAIN_SPARSE_SET;
		// ---- the forward pass
		std::vector<int32_t> f((size_t)n + 1), pred((size_t)n + 1);
		if (ctx && n > 0) {
			ChainIO io;
			int rc = dev_chain_buffers(ctx, n, io);
			if (rc != MPA_OK) return rc;
			memcpy(io.a, a, (size_t)n * 8);
			if ((rc = dev_chain_forward(ctx, p, n_prob, first, io)) != MPA_OK) return rc;
			memcpy(f.data(), io.f, (size_t)n * 4), memcpy(pred.data(), io.pred, (size_t)n * 4);
		} else
			for (int32_t q = 0; q < n_prob; ++q) chain_forward(p, a + first[q], first[q + 1] - first[q], f.data() + first[q], pred.data() + first[q]);
		// ---- the views: dense = the pass's own arrays; sparse = the anchors of runs of two or more whose consecutive blocks lie within reach
		std::vector<int64_t> vfirst(first, first + n_prob + 1);
		std::vector<int32_t> vpos, vf, vpred;
		std::vector<uint64_t> va;
		if (sparse) {
			const uint64_t max_dblock = (uint64_t)(std::max(p.max_dist_x, p.bw) >> (p.bbit > 0 ? p.bbit : 0));
			for (int32_t q = 0; q < n_prob; ++q) {
				const int64_t q0 = first[q], nq = first[q + 1] - q0, v0 = (int64_t)vpos.size();
				const uint64_t *aq = a + q0;
				vfirst[(size_t)q] = v0;
				for (int64_t s = 0; s < nq;) {
					int64_t e = s + 1;
					while (e < nq && (aq[e] >> 32) - (aq[e - 1] >> 32) <= max_dblock) ++e;
					if (e - s >= 2)
						for (int64_t i = s; i < e; ++i) {
							const int32_t c = (int32_t)((int64_t)vpos.size() - v0), pi = pred[(size_t)(q0 + i)];
							vpos.push_back((int32_t)i), vf.push_back(f[(size_t)(q0 + i)]), va.push_back(aq[i]);
							vpred.push_back(pi < 0 ? -1 : c - (int32_t)(i - pi));
						}
					s = e;
				}
			}
			vfirst[(size_t)n_prob] = (int64_t)vpos.size();
			vpos.push_back(0), vf.push_back(0), vpred.push_back(-1), va.push_back(0);     // (never empty: data() is a pointer)
		}
		const int32_t *P = sparse ? vpos.data() : nullptr, *F = sparse ? vf.data() : f.data(), *PR = sparse ? vpred.data() : pred.data();
		const uint64_t *A = sparse ? va.data() : a;
		auto view_of = [&](int32_t q) {
			const int64_t o = vfirst[(size_t)q];
			return ChainView{ first[q + 1] - first[q], vfirst[(size_t)q + 1] - o, P ? P + o : nullptr, F + o, PR + o, A + o };
		};
		for (int32_t q = 0; q < n_prob; ++q) {
			const ChainView v = view_of(q);
			chain_path_record(p, v, v.m + 64, rec + (size_t)q * MPA_DBG_CHAIN_REC);
			status[q] = 0;
		}
		// ---- the extraction
		if (ctx) return dev_chain_extract_dbg(ctx, p, n_prob, vfirst.data(), sparse ? first : nullptr, P, F, PR, A, set_only ? 1 : 0, off_u, u, off_a, a_out, status);
		std::vector<uint64_t> av, uv;
		off_u[0] = off_a[0] = 0;
		for (int32_t q = 0; q < n_prob; ++q) {
			const ChainView v = view_of(q);
			av.clear(), uv.clear();
			if (v.m > 0) status[q] = extract_on_host(p, v, set_only, av, uv);
			if (!av.empty()) memcpy(a_out + off_a[q], av.data(), av.size() * 8);
			if (!uv.empty()) memcpy(u + off_u[q], uv.data(), uv.size() * 8);
			off_a[q + 1] = off_a[q] + (int64_t)av.size(), off_u[q + 1] = off_u[q] + (int64_t)uv.size();
		}
		return MPA_OK;
	});
}
