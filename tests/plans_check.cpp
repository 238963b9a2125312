// plans_check.cpp -- a stand-alone check of miniprot_amd/csrc/plans_core.h (tests/test_plans_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written and random refinement chains over a small genome go through the shared
// core twice -- with a team of one (PlansSerial, what MPA_GPU_PLANS=model runs) and with a team of 64 host threads that meet at a
// barrier for every sync, sum and ballot (the device's wavefront in slow motion: same lane-strided loops, same lane-0 work) -- and
// are compared, field by field, with plain restatements of the host functions on std::vector, written here after host_plan.cpp
// (refine_region_from_chains, mark_reliable_anchors, plan_alignment, plan_round1, make_segment, ungapped_score) and
// host_regions.cpp (chain_score_ungapped, sort_regions, assign_parents, select_secondary with its renumbering, extension_limits in
// its genome-coordinate form).  The order of equal scores is the reference's unstable radix sort: both sides take it from
// sort_pairs_by_x_core (chain_core.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "plans_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static uint64_t g_slot[64];
static thread_local int tl_lane = 0;
struct PlansThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static void sync() { pthread_barrier_wait(&g_bar); }
	static int32_t sum(int32_t v)
	{
		g_slot[tl_lane] = (uint32_t)v;
		pthread_barrier_wait(&g_bar);
		uint32_t s = 0;
		for (int i = 0; i < 64; ++i) s += (uint32_t)g_slot[i];
		pthread_barrier_wait(&g_bar);
		return (int32_t)s;
	}
	static uint64_t ballot(bool p)
	{
		g_slot[tl_lane] = p ? 1u : 0u;
		pthread_barrier_wait(&g_bar);
		uint64_t m = 0;
		for (int i = 0; i < 64; ++i) m |= g_slot[i] << i;
		pthread_barrier_wait(&g_bar);
		return m;
	}
	static int rank(uint64_t m) { return __builtin_popcountll(m & ((1ull << tl_lane) - 1ull)); }
	static int popc(uint64_t m) { return __builtin_popcountll(m); }
};

static uint64_t g_rng = 88172645463325252ULL;
static uint64_t rnd(uint64_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng % n; }

// ---- the genome, the tables ---------------------------------------------------------------------------
static const int64_t kCtgLen[3] = { 6000, 3000, 9000 };
static int64_t g_ctg_off[3];
static std::vector<uint8_t> g_fwd;                        // nt4 codes of the forward strands, contig after contig
static uint8_t g_tab[ALN_TAB_BYTES];

struct StrandReader {                                     // what the core reads the genome through
	int64_t off, len;
	int rev;
	uint32_t base(int64_t x) const
	{
		if (x < 0 || x >= len) return 4;
		const uint8_t c = rev ? g_fwd[(size_t)(off + len - 1 - x)] : g_fwd[(size_t)(off + x)];
		return rev && c < 4 ? 3u - c : c;
	}
};
struct GenomeReader {
	int64_t off(int32_t c) const { return g_ctg_off[c]; }
	int64_t len(int32_t c) const { return kCtgLen[c]; }
	StrandReader strand(uint32_t vid) const { return StrandReader{ g_ctg_off[vid >> 1], kCtgLen[vid >> 1], (int)(vid & 1) }; }
};
// the plain side's fetch (mp_ntseq_get_by_v, ntseq.c:108-114): the strand written out, then indexed
static std::vector<uint8_t> plain_strand(uint32_t vid)
{
	const int64_t off = g_ctg_off[vid >> 1], len = kCtgLen[vid >> 1];
	std::vector<uint8_t> s(g_fwd.begin() + off, g_fwd.begin() + off + len);
	if (vid & 1) {
		std::reverse(s.begin(), s.end());
		for (uint8_t &c : s) if (c < 4) c = (uint8_t)(3 - c);
	}
	return s;
}

static void make_world()
{
	int64_t o = 0;
	for (int c = 0; c < 3; ++c) g_ctg_off[c] = o, o += kCtgLen[c];
	g_fwd.resize((size_t)o);
	for (uint8_t &b : g_fwd) b = rnd(40) == 0 ? 4 : (uint8_t)rnd(4);
	const char *codon = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF", *aa = "ARNDCQEGHILKMFPSTWYV*X";
	memset(g_tab, 21, sizeof g_tab);
	for (int i = 0; i < 22; ++i) g_tab[ALN_TAB_AA20 + (uint8_t)aa[i]] = (uint8_t)i;
	for (int i = 0; i < 64; ++i) g_tab[ALN_TAB_CODON + i] = g_tab[ALN_TAB_AA20 + (uint8_t)codon[i]];
	for (int i = 0; i < 484; ++i) g_tab[ALN_TAB_MAT + i] = (uint8_t)(int8_t)((int)rnd(14) - 4);
}

// ---- a case -----------------------------------------------------------------------------------------
struct Chain { int32_t sc; std::vector<std::pair<int32_t, int32_t>> an; };   // anchors: (window-relative x, query position)
struct Window { PlansWindow w; std::vector<Chain> chains; };
struct Case {
	int32_t qlen = 0;
	std::string prot;
	std::vector<Window> win;
	Window &add(int64_t as, uint32_t vid, int32_t n_sub = 0, int32_t subsc = 0, int32_t split = 0)
	{
		win.push_back(Window{ PlansWindow{ as, vid, n_sub, subsc, split }, {} });
		return win.back();
	}
};
static void set_protein(Case &c, int32_t qlen)
{
	c.qlen = qlen, c.prot.resize((size_t)qlen);
	for (char &ch : c.prot) ch = "ARNDCQEGHILKMFPSTWYV*X"[rnd(22)];
}
// n anchors from (x, q) in steps of (dx, dq)
static Chain line(int32_t sc, int32_t x, int32_t q, int32_t n, int32_t dx = 3, int32_t dq = 1)
{
	Chain c{ sc, {} };
	for (int32_t i = 0; i < n; ++i) c.an.push_back({ x + i * dx, q + i * dq });
	return c;
}
static void extend(Chain &c, int32_t n, int32_t dx, int32_t dq, int32_t gap_x, int32_t gap_q)
{
	int32_t x = c.an.back().first + gap_x, q = c.an.back().second + gap_q;
	for (int32_t i = 0; i < n; ++i) c.an.push_back({ x + i * dx, q + i * dq });
}

// ---- the plain side ---------------------------------------------------------------------------------
struct Plain {
	int32_t off = 0, cnt = 0, id = 0, parent = 0, n_sub = 0, subsc = 0, chn_sc = 0, chn_sc_ungap = 0;
	uint32_t vid = 0;
	int32_t qs = 0, qe = 0;
	int64_t vs = 0, ve = 0;
	int32_t split = 0;
	std::vector<uint64_t> a;
};
struct PlainOut { std::vector<Plain> reg; std::vector<PlanRec> plan; std::vector<mpa_dp_task_t> task; std::vector<SegRec> seg; };

static int32_t plain_score_ungapped(const std::vector<uint64_t> &a, int32_t kmer)      // hit.c:18-30
{
	int32_t x = kmer;
	for (size_t i = 1; i < a.size(); ++i) {
		const int32_t dq = (int32_t)a[i] - (int32_t)a[i - 1], dr3 = (int32_t)((a[i] >> 32) - (a[i - 1] >> 32)), dr = dr3 / 3;
		if (dq >= dr && dr3 != dr * 3) --x;
		else x += std::min(std::min(dq, dr), kmer);
	}
	return x;
}

static bool plain_refine(const PlansParams &p, const Window &w, Plain &r)                // map.c:89-111
{
	if (w.chains.empty()) return false;
	size_t best = 0;
	for (size_t i = 1; i < w.chains.size(); ++i) if (w.chains[best].sc < w.chains[i].sc) best = i;
	const Chain &c = w.chains[best];
	r = Plain();
	r.vid = w.w.vid, r.n_sub = w.w.n_sub, r.subsc = w.w.subsc, r.split = w.w.split;
	r.chn_sc = c.sc, r.cnt = (int32_t)c.an.size(), r.off = 0;
	r.qs = c.an.front().second - (p.kmer2 - 1), r.qe = c.an.back().second + 1;
	r.vs = w.w.as + c.an.front().first + 1 - 3 * p.kmer2, r.ve = w.w.as + c.an.back().first + 1;
	for (auto &x : c.an) r.a.push_back((uint64_t)((int64_t)x.first + w.w.as - r.vs) << 32 | (uint32_t)x.second);
	r.chn_sc_ungap = plain_score_ungapped(r.a, p.kmer2);
	return true;
}

static void plain_sort(std::vector<Plain> &r)
{
	const int32_t n = (int32_t)r.size();
	if (n <= 1) return;
	std::vector<Pair64> key;
	for (int32_t i = 0; i < n; ++i) key.push_back(Pair64{ (uint64_t)r[(size_t)i].chn_sc << 32, (uint64_t)i });
	std::vector<SortRange> stack(key.size() / 64 + 4);
	std::vector<uint32_t> hist(768);
	sort_pairs_by_x_core(key.data(), key.data() + key.size(), stack.data(), hist.data());
	std::vector<Plain> sorted;
	for (size_t i = key.size(); i-- > 0;) sorted.push_back(r[key[i].y]);
	r.swap(sorted);
}

static void plain_parents(float mask_level, int mask_len, std::vector<Plain> &r)
{
	const int n = (int)r.size();
	if (n <= 0) return;
	for (int i = 0; i < n; ++i) r[(size_t)i].id = i;
	std::vector<int> prim(1, 0);
	r[0].parent = 0;
	for (int i = 1; i < n; ++i) {
		Plain &ri = r[(size_t)i];
		const int si = ri.qs, ei = ri.qe;
		std::vector<uint64_t> cov;
		for (int w : prim) {
			const int sj = r[(size_t)w].qs, ej = r[(size_t)w].qe;
			if (ej <= si || sj >= ei) continue;
			cov.push_back((uint64_t)std::max(sj, si) << 32 | (uint32_t)std::min(ej, ei));
		}
		bool is_primary = true;
		if (!cov.empty()) {
			std::sort(cov.begin(), cov.end());
			int x = si, uncovered = 0;
			for (uint64_t c : cov) {
				if ((int)(c >> 32) > x) uncovered += (int)(c >> 32) - x;
				x = std::max((int)(int32_t)c, x);
			}
			if (ei > x) uncovered += ei - x;
			for (int w : prim) {
				Plain &rp = r[(size_t)w];
				const int sj = rp.qs, ej = rp.qe;
				if (ej <= si || sj >= ei) continue;
				const int lo = std::min(ej - sj, ei - si), hi = std::max(ej - sj, ei - si);
				const int ol = std::max(0, std::min(ei, ej) - std::max(si, sj));
				if ((float)ol / lo - (float)uncovered / hi > mask_level && uncovered <= mask_len) {
					ri.parent = rp.parent;
					rp.subsc = std::max(rp.subsc, ri.chn_sc);
					if (ri.cnt >= rp.cnt) ++rp.n_sub;
					is_primary = false;
					break;
				}
			}
		}
		if (is_primary) prim.push_back(i), ri.parent = i, ri.n_sub = 0;
	}
}

static void plain_select(float pri_ratio, int min_diff, int best_n, std::vector<Plain> &r)
{
	if (!(pri_ratio > 0.0f) || r.empty()) return;
	const int n = (int)r.size();
	int top_ungap = -1, n_2nd = 0;
	for (const Plain &x : r) top_ungap = std::max(top_ungap, x.chn_sc_ungap);
	std::vector<Plain> kept;
	for (int i = 0; i < n; ++i) {
		const int p = r[(size_t)i].parent;
		const Plain &rp = p < (int)kept.size() ? kept[(size_t)p] : r[(size_t)p];   // (the reference reads the array it is compacting)
		const Plain &x = r[(size_t)i];
		const bool same = x.qs == rp.qs && x.qe == rp.qe && x.vid == rp.vid && x.vs == rp.vs && x.ve == rp.ve;
		bool keep = false;
		if (p == i) keep = true;
		else if ((x.chn_sc >= rp.chn_sc * pri_ratio || x.chn_sc + min_diff >= rp.chn_sc) && n_2nd < best_n) { if (!same) keep = true, ++n_2nd; }
		else if (top_ungap > 0 && x.chn_sc_ungap >= top_ungap * pri_ratio && n_2nd < best_n) { if (!same) keep = true, ++n_2nd; }
		if (keep) kept.push_back(x);
	}
	const bool dropped = (int)kept.size() != n;
	r.swap(kept);
	if (!dropped) return;
	int max_id = -1;
	for (const Plain &x : r) max_id = std::max(max_id, x.id);
	std::vector<int> where((size_t)max_id + 1, -1);
	for (size_t i = 0; i < r.size(); ++i) if (r[i].id >= 0) where[(size_t)r[i].id] = (int)i;
	for (size_t i = 0; i < r.size(); ++i) {
		Plain &x = r[i];
		x.id = (int)i;
		if (x.parent == -2) x.parent = (int)i;
		else if (x.parent >= 0 && x.parent <= max_id && where[(size_t)x.parent] >= 0) x.parent = where[(size_t)x.parent];
		else x.parent = -1;
	}
}

static void plain_limits(const std::vector<Plain> &r, int32_t min_ext, int32_t max_ext, std::vector<uint64_t> &ext)   // hit.c:252-287, genome coordinates
{
	const int32_t n = (int32_t)r.size();
	ext.assign((size_t)n, 0);
	if (n <= 0) return;
	std::vector<Pair64> pos((size_t)n);
	for (int32_t i = 0; i < n; ++i) {
		const Plain &x = r[(size_t)i];
		pos[(size_t)i] = Pair64{ (uint64_t)(x.vs + g_ctg_off[x.vid >> 1] + ((x.vid & 1) ? kCtgLen[x.vid >> 1] : 0)), (uint64_t)i };
	}
	std::vector<SortRange> stack((size_t)n / 64 + 4);
	std::vector<uint32_t> hist(768);
	sort_pairs_by_x_core(pos.data(), pos.data() + n, stack.data(), hist.data());
	for (int32_t i = 0; i < n; ++i) {
		const Plain &x = r[pos[(size_t)i].y];
		int64_t left = max_ext, right = max_ext;
		if (i > 0) {
			const Plain &q = r[pos[(size_t)i - 1].y];
			if (q.vid == x.vid && q.qe >= x.qs) left = std::max<int64_t>(std::min<int64_t>(x.vs - q.ve, max_ext), min_ext);
		}
		if (i < n - 1) {
			const Plain &q = r[pos[(size_t)i + 1].y];
			if (q.vid == x.vid && x.qe >= q.qs) right = std::max<int64_t>(std::min<int64_t>(q.vs - x.ve, max_ext), min_ext);
		}
		ext[pos[(size_t)i].y] = (uint64_t)(uint32_t)(int32_t)left << 32 | (uint32_t)(int32_t)right;
	}
}

static void plain_mark(std::vector<uint64_t> &a, int32_t max_aa_dist, int32_t min_cnt, int32_t kmer2, int32_t trim)   // mp_filter_seed, align.c:6-31
{
	const int32_t cnt = (int32_t)a.size();
	for (int32_t i = 0; i < cnt; ++i) {
		int32_t j = i + 1;
		for (; j < cnt; ++j) {
			const int32_t dx = (int32_t)(a[(size_t)j] >> 32) - (int32_t)(a[(size_t)j - 1] >> 32), dy = (int32_t)a[(size_t)j] - (int32_t)a[(size_t)j - 1];
			if (dx % 3 != 0 || dx > max_aa_dist * 3 || dy > max_aa_dist) break;
		}
		if (j - i < min_cnt) continue;
		int32_t k = j - 2, t = (int32_t)a[(size_t)j - 1];
		while (k >= i && t - (int32_t)a[(size_t)k] < trim) --k;
		t = (int32_t)a[(size_t)i] + 1 - kmer2;
		while (i < k && (int32_t)a[(size_t)i] + 1 - t < trim) ++i;
		for (; i <= k; ++i) a[(size_t)i] |= 1ULL << 31;
		i = j - 1;
	}
}

static mpa_dp_task_t plain_task(int32_t qid, const Plain &r, int64_t nt_off, int64_t nl, int32_t aa_off, int32_t al, int32_t flag, int32_t io)
{
	mpa_dp_task_t t;
	t.nt_off = nt_off, t.vid = (int32_t)r.vid, t.nl = (int32_t)nl, t.qid = qid, t.aa_off = aa_off, t.al = al, t.flag = flag, t.io = io, t.tag = 0;
	return t;
}

static int32_t plain_ungapped(const PlansParams &p, const Plain &r, int64_t nt_off, int32_t alen, const char *aa)   // align.c:33-40
{
	const std::vector<uint8_t> s = plain_strand(r.vid);
	std::vector<uint8_t> nt((size_t)alen * 3);
	for (int32_t i = 0; i < alen * 3; ++i) nt[(size_t)i] = nt_off + i >= 0 && nt_off + i < (int64_t)s.size() ? s[(size_t)(nt_off + i)] : 4;
	int32_t sc = 0;
	for (int32_t i = 0, j = 0; i < alen; i += 3, ++j) {
		const uint8_t *c = &nt[(size_t)i];
		const uint8_t codon = c[0] > 3 || c[1] > 3 || c[2] > 3 ? 21 : g_tab[ALN_TAB_CODON + (c[0] << 4 | c[1] << 2 | c[2])];
		sc += (int8_t)g_tab[ALN_TAB_MAT + codon * p.asize + g_tab[ALN_TAB_AA20 + (uint8_t)aa[j]]];
	}
	return sc;
}

static void plain_all(const PlansParams &p, const Case &c, int32_t qid, PlainOut &o)
{
	o = PlainOut();
	for (const Window &w : c.win) { Plain r; if (plain_refine(p, w, r)) o.reg.push_back(r); }
	plain_sort(o.reg);
	plain_parents(p.mask_level, p.mask_len, o.reg);
	plain_select(p.pri_ratio, p.kmer * 2, p.best_n, o.reg);
	if (p.no_align) return;
	std::vector<uint64_t> ext;
	plain_limits(o.reg, 100, p.max_intron / 2, ext);
	std::vector<int32_t> i0s;
	for (size_t ri = 0; ri < o.reg.size(); ++ri) {                            // plan_alignment
		Plain &r = o.reg[ri];
		plain_mark(r.a, 6, 3, p.kmer2, p.kmer2 + 1);
		int32_t i0 = 0;
		while (i0 < r.cnt && !(r.a[(size_t)i0] >> 31 & 1)) ++i0;
		if (i0 == r.cnt) { r.cnt = 0; continue; }
		const int32_t extl0 = (int32_t)(ext[ri] >> 32), extr0 = (int32_t)ext[ri];
		int32_t extl = p.max_ext, extr = p.max_ext;
		if (r.qs >= 10) extl = p.max_intron / 2;
		if (c.qlen - r.qe >= 10) extr = p.max_intron / 2;
		if (extl0 > 0) extl = std::min(extl, extl0);
		if (extr0 > 0) extr = std::min(extr, extr0);
		const int64_t ctg_len = kCtgLen[r.vid >> 1];
		PlanRec pl;
		memset(&pl, 0, sizeof pl);
		pl.reg = (int32_t)ri;
		pl.as = r.vs > extl ? r.vs - extl : 0;
		pl.ae = r.ve + extr < ctg_len ? r.ve + extr : ctg_len;
		pl.vs0 = r.vs;
		pl.vs1 = pl.vs0 + (int64_t)(r.a[(size_t)i0] >> 32) + 1;
		pl.as1 = (int32_t)((uint32_t)r.a[(size_t)i0] << 1 >> 1) + 1;
		int32_t ne = 0, ae = 0;
		for (int32_t i = i0; i < r.cnt; ++i)
			if (r.a[(size_t)i] >> 31 & 1) ne = (int32_t)(r.a[(size_t)i] >> 32) + 1, ae = (int32_t)((uint32_t)r.a[(size_t)i] << 1 >> 1) + 1;
		pl.mid_ve = ne + pl.vs0, pl.mid_qe = ae;
		pl.has_right = pl.mid_qe < c.qlen && pl.mid_ve < pl.ae;
		pl.t_left = pl.t_left2 = pl.t_right = pl.t_right2 = -1;
		o.plan.push_back(pl), i0s.push_back(i0);
	}
	const bool retry = p.io > p.io_end;
	for (size_t pi = 0; pi < o.plan.size(); ++pi) {                           // plan_round1
		PlanRec &pl = o.plan[pi];
		const Plain &r = o.reg[(size_t)pl.reg];
		pl.t_left = (int32_t)o.task.size();
		o.task.push_back(plain_task(qid, r, pl.as, pl.vs1 - pl.as, 0, pl.as1, MPA_F_EXT_LEFT | MPA_F_SS_SKIP0, p.io));
		if (retry) {
			const int64_t as_alt = pl.vs1 - pl.as > p.max_ext ? pl.vs1 - p.max_ext : pl.as;
			pl.t_left2 = (int32_t)o.task.size();
			o.task.push_back(plain_task(qid, r, as_alt, pl.vs1 - as_alt, 0, pl.as1, MPA_F_EXT_LEFT | (as_alt == pl.as ? MPA_F_SS_SKIP0 : 0), p.io_end));
		}
		if (pl.has_right) {
			pl.t_right = (int32_t)o.task.size();
			o.task.push_back(plain_task(qid, r, pl.mid_ve, pl.ae - pl.mid_ve, pl.mid_qe, c.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, p.io));
			if (retry) {
				const int64_t l_ext = std::min<int64_t>(pl.ae - pl.mid_ve, p.max_ext);
				pl.t_right2 = (int32_t)o.task.size();
				o.task.push_back(plain_task(qid, r, pl.mid_ve, l_ext, pl.mid_qe, c.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, p.io_end));
			}
		}
		pl.gap0 = (int32_t)o.seg.size();
		int32_t ne0 = (int32_t)(pl.vs1 - pl.vs0), ae0 = pl.as1;
		for (int32_t i = i0s[pi] + 1; i < r.cnt; ++i) {
			if (!(r.a[(size_t)i] >> 31 & 1)) continue;
			const int32_t ne1 = (int32_t)(r.a[(size_t)i] >> 32) + 1, ae1 = (int32_t)((uint32_t)r.a[(size_t)i] << 1 >> 1) + 1;
			SegRec s{ ne0, ne1, ae0, ae1, -1, 0 };                                   // make_segment
			const int32_t nlen = ne1 - ne0, alen = ae1 - ae0;
			if (nlen == alen * 3 && alen <= p.kmer2) s.score = plain_ungapped(p, r, pl.vs0 + ne0, alen, c.prot.data() + ae0);
			else {
				s.task = (int32_t)o.task.size();
				o.task.push_back(plain_task(qid, r, pl.vs0 + ne0, nlen, ae0, alen, MPA_F_CIGAR, p.io));
			}
			o.seg.push_back(s);
			ne0 = ne1, ae0 = ae1;
		}
		pl.n_gap = (int32_t)o.seg.size() - pl.gap0;
	}
}

// ---- the core ---------------------------------------------------------------------------------------
static int g_cases = 0, g_fail = 0;
struct Got { PlansCounts n; std::vector<RegionRec> reg; std::vector<PlanRec> plan; std::vector<mpa_dp_task_t> task; std::vector<SegRec> seg; };

template<class C> static void run_core(const PlansParams &p, const Case &c, int32_t qid, Got &g, int lanes)
{
	const size_t n = c.win.size();
	std::vector<PlansWindow> win;
	std::vector<int64_t> cu, ca, nu;
	std::vector<uint64_t> U, A;
	size_t longest = 0;
	for (const Window &w : c.win) {
		win.push_back(w.w), cu.push_back((int64_t)U.size()), ca.push_back((int64_t)A.size()), nu.push_back((int64_t)w.chains.size());
		for (const Chain &ch : w.chains) {
			U.push_back((uint64_t)(uint32_t)ch.sc << 32 | (uint32_t)ch.an.size());
			for (auto &x : ch.an) A.push_back((uint64_t)(uint32_t)x.first << 32 | (uint32_t)x.second);
			longest = std::max(longest, ch.an.size());
		}
	}
	const size_t m = A.size();
	RegionRec zr;
	PlanRec zp;
	mpa_dp_task_t zt;
	memset(&zr, 0, sizeof zr), memset(&zp, 0, sizeof zp), memset(&zt, 0, sizeof zt);
	// (every array has exactly the size the header states: AddressSanitizer sees a write one element beyond it)
	std::vector<RegionRec> tmp(n, zr);
	std::vector<Pair64> key(n);
	std::vector<SortRange> stack(n / 64 + 4);
	std::vector<uint32_t> hist(768);
	std::vector<int32_t> prim(n), flag(longest), list(longest), ctl(2);
	std::vector<uint64_t> cov(n), ext(n);
	std::vector<int64_t> aoff(n);
	g.reg.assign(n, zr), g.plan.assign(n, zp), g.task.assign(4 * n + m, zt), g.seg.assign(m, SegRec{ 0, 0, 0, 0, 0, 0 });
	const PlansQuery Q{ (int32_t)n, qid, c.qlen, win.data(), cu.data(), ca.data(), nu.data(), U.data(), A.data(), (const uint8_t*)c.prot.data() };
	const PlansScratch S{ tmp.data(), key.data(), stack.data(), hist.data(), prim.data(), cov.data(), ext.data(), aoff.data(), flag.data(), list.data(), ctl.data() };
	const GenomeReader G;
	if (lanes == 1) { g.n = plans_core<C>(p, Q, G, g_tab, S, g.reg.data(), g.plan.data(), g.task.data(), g.seg.data()); return; }
	std::vector<PlansCounts> ns(64);
	std::vector<std::thread> th;
	for (int l = 0; l < 64; ++l) th.emplace_back([&, l] { tl_lane = l; ns[(size_t)l] = plans_core<C>(p, Q, G, g_tab, S, g.reg.data(), g.plan.data(), g.task.data(), g.seg.data()); });
	for (auto &t : th) t.join();
	g.n = ns[0];
	for (int l = 1; l < 64; ++l) if (memcmp(&ns[(size_t)l], &ns[0], sizeof(PlansCounts))) { fprintf(stderr, "lane %d returns other counts than lane 0\n", l); ++g_fail; }
}

static void compare(const char *name, const char *team, const PlainOut &w, const Got &g)
{
	if (g.n.n_reg != (int32_t)w.reg.size() || g.n.n_plan != (int32_t)w.plan.size() || g.n.n_task != (int32_t)w.task.size() || g.n.n_seg != (int32_t)w.seg.size()) {
		fprintf(stderr, "MISMATCH %s (%s): %d regions, %d plans, %d tasks, %d segments; expected %zu, %zu, %zu, %zu\n", name, team, g.n.n_reg, g.n.n_plan, g.n.n_task, g.n.n_seg,
		        w.reg.size(), w.plan.size(), w.task.size(), w.seg.size());
		++g_fail;
		return;
	}
#define F(what, i, f) if ((int64_t)x.f != (int64_t)y.f) { fprintf(stderr, "MISMATCH %s (%s): %s %zu: " #f " %lld, expected %lld\n", name, team, what, i, (long long)y.f, (long long)x.f); ++g_fail; return; }
	for (size_t i = 0; i < w.reg.size(); ++i) {
		const Plain &x = w.reg[i];
		const RegionRec &y = g.reg[i];
		F("region", i, off) F("region", i, cnt) F("region", i, id) F("region", i, parent) F("region", i, n_sub) F("region", i, subsc) F("region", i, chn_sc)
		F("region", i, chn_sc_ungap) F("region", i, vid) F("region", i, qs) F("region", i, qe) F("region", i, vs) F("region", i, ve) F("region", i, split)
	}
	for (size_t i = 0; i < w.plan.size(); ++i) {
		const PlanRec &x = w.plan[i], &y = g.plan[i];
		F("plan", i, as) F("plan", i, ae) F("plan", i, vs0) F("plan", i, vs1) F("plan", i, mid_ve) F("plan", i, reg) F("plan", i, as1) F("plan", i, mid_qe)
		F("plan", i, has_right) F("plan", i, t_left) F("plan", i, t_left2) F("plan", i, t_right) F("plan", i, t_right2) F("plan", i, gap0) F("plan", i, n_gap)
	}
	for (size_t i = 0; i < w.task.size(); ++i) {
		const mpa_dp_task_t &x = w.task[i], &y = g.task[i];
		F("task", i, nt_off) F("task", i, vid) F("task", i, nl) F("task", i, qid) F("task", i, aa_off) F("task", i, al) F("task", i, flag) F("task", i, io) F("task", i, tag)
	}
	for (size_t i = 0; i < w.seg.size(); ++i) {
		const SegRec &x = w.seg[i], &y = g.seg[i];
		F("segment", i, ne0) F("segment", i, ne1) F("segment", i, ae0) F("segment", i, ae1) F("segment", i, task) F("segment", i, score)
	}
#undef F
}

static PlainOut run_case(const char *name, const PlansParams &p, const Case &c, bool wave = true)
{
	PlainOut w;
	const int32_t qid = 7;
	plain_all(p, c, qid, w);
	Got g;
	run_core<PlansSerial>(p, c, qid, g, 1);
	compare(name, "team of one", w, g);
	if (wave) {
		run_core<PlansThreads>(p, c, qid, g, 64);
		compare(name, "team of 64", w, g);
	}
	++g_cases;
	return w;
}
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "CASE DOES NOT SHOW WHAT IT IS FOR: %s (line %d)\n", #cond, __LINE__); ++g_fail; } } while (0)

static PlansParams params()
{
	PlansParams p;
	p.kmer2 = 5, p.kmer = 6, p.mask_len = 0x7fffffff, p.best_n = 30, p.max_ext = 1000, p.max_intron = 4000, p.io = 29, p.io_end = 19, p.no_align = 0, p.asize = 22;
	p.mask_level = 0.5f, p.pri_ratio = 0.7f * 0.7f;
	return p;
}
static int count_marked_none(const PlainOut &w) { int n = 0; for (const Plain &r : w.reg) n += r.cnt == 0; return n; }
static int count_short(const PlainOut &w) { int n = 0; for (const SegRec &s : w.seg) n += s.task < 0; return n; }

int main()
{
	pthread_barrier_init(&g_bar, nullptr, 64);
	make_world();
	const PlansParams P = params();
	// ---- windows and chains
	{ Case c; set_protein(c, 300); const PlainOut w = run_case("no windows", P, c); EXPECT(w.reg.empty()); }
	{	// a window without chains between two that have one; then all windows without chains
		Case c; set_protein(c, 300);
		c.add(1000, 0).chains.push_back(line(200, 20, 30, 40));
		c.add(2000, 0);
		c.add(3000, 0).chains.push_back(line(150, 20, 150, 30));
		const PlainOut w = run_case("a window without chains", P, c);
		EXPECT(w.reg.size() == 2 && w.plan.size() == 2);
		Case e; set_protein(e, 300);
		e.add(1000, 0), e.add(2000, 2), e.add(100, 4);
		const PlainOut v = run_case("all windows without chains", P, e);
		EXPECT(v.reg.empty() && v.task.empty());
	}
	{	// the best chain not first; two chains sharing the highest score: the first of them
		Case c; set_protein(c, 400);
		Window &a = c.add(1000, 0);
		a.chains.push_back(line(100, 20, 30, 12)), a.chains.push_back(line(300, 200, 60, 40)), a.chains.push_back(line(200, 500, 120, 15));
		Window &b = c.add(500, 2);
		b.chains.push_back(line(90, 20, 230, 12)), b.chains.push_back(line(250, 100, 250, 30)), b.chains.push_back(line(250, 400, 300, 35));
		const PlainOut w = run_case("best chain not first, equal best scores", P, c);
		EXPECT(w.reg.size() == 2 && w.reg[0].cnt == 40 && w.reg[1].cnt == 30 && w.reg[1].qs == 250 - 4);
	}
	{	// more than 64 windows: 70 regions side by side on three strands, of equal score in runs (the radix passes of the order)
		Case c; set_protein(c, 2000);
		PlansParams p = P;
		p.best_n = 1000;
		for (int i = 0; i < 70; ++i) c.add(100 + 80 * (i % 30), (uint32_t)(i % 3) * 2 + (i % 2), i % 4, i % 5 * 10, i % 3).chains.push_back(line(77 + (i % 2), 20, 10 + 25 * i, 12 + i % 7));
		const PlainOut w = run_case("70 windows", p, c);
		EXPECT(w.reg.size() > 64 && w.plan.size() > 64);
	}
	for (int n : { 64, 65, 128, 129, 300, 1000 }) {            // chains of 65 and of more than 128 anchors: every lane-strided loop wraps
		Case c; set_protein(c, 1200);
		c.add(200, 4).chains.push_back(line(5000, 20, 30, n));
		c.add(3000, 5).chains.push_back(line(4000, 20, 40, n + 1, 6, 1));
		char nm[64];
		snprintf(nm, sizeof nm, "long chains (%d)", n);
		const PlainOut w = run_case(nm, P, c);
		EXPECT(w.reg.size() == 2 && w.plan.size() == 2 && w.plan[0].n_gap == n - 8 && w.reg[0].chn_sc_ungap == 5 + (n - 1));
	}
	// ---- runs and trims
	{	// runs of 2 (below min_cnt) and of 3 with wide steps (its middle anchor is marked), separated by breaks of every kind
		Case c; set_protein(c, 600);
		Chain ch = line(300, 20, 20, 2, 18, 6);             // run of 2
		extend(ch, 3, 18, 6, 20, 6);                          // break: dx % 3 != 0; run of 3
		extend(ch, 3, 18, 6, 18, 6);                          // dx 18, dy 6: no break: the run grows to 6
		extend(ch, 3, 18, 6, 19, 6);                          // break: dx 19
		extend(ch, 3, 18, 6, 21, 6);                          // break: dx 21 (in frame, too far)
		extend(ch, 3, 18, 6, 18, 7);                          // break: dy 7
		extend(ch, 2, 18, 6, 18, 7);                          // run of 2 at the end
		c.add(100, 0).chains.push_back(ch);
		const PlainOut w = run_case("runs of 2 and 3, breaks at the thresholds", P, c);
		EXPECT(w.plan.size() == 1 && w.plan[0].n_gap == 4 + 1 + 1 + 1 - 1);   // marks: 4 of the run of 6, 1 of each run of 3
	}
	{	// trims that empty a run (runs of 3 .. 6 with steps of one residue: the last six anchors go at the end, one more at the front),
		// next to a run of 7, which keeps its first anchor, and a run of 12, which keeps five
		Case c; set_protein(c, 600);
		Chain ch = line(300, 20, 20, 5);
		extend(ch, 6, 3, 1, 30, 9), extend(ch, 7, 3, 1, 30, 9), extend(ch, 12, 3, 1, 30, 9), extend(ch, 3, 3, 1, 30, 9);
		c.add(100, 0).chains.push_back(ch);
		const PlainOut w = run_case("trims that empty a run", P, c);
		EXPECT(w.plan.size() == 1 && w.plan[0].n_gap == 1 + 5 - 1 && w.plan[0].as1 == 20 + 4 + 9 + 5 + 9 + 1);
	}
	{	// a region with no marked anchor: cnt becomes 0, no plan; it stays in the list in front of one that has a plan
		Case c; set_protein(c, 600);
		c.add(100, 0).chains.push_back(line(500, 20, 20, 6));
		c.add(2000, 0).chains.push_back(line(300, 20, 300, 20));
		const PlainOut w = run_case("a region without a marked anchor", P, c);
		EXPECT(w.reg.size() == 2 && count_marked_none(w) == 1 && w.reg[0].cnt == 0 && w.plan.size() == 1 && w.plan[0].reg == 1);
	}
	// ---- window clamps and thresholds
	{	// as clamped at 0, ae clamped at the contig's end (contig 1 has 3 000 bases), on a reverse strand
		Case c; set_protein(c, 600);
		c.add(50, 3).chains.push_back(line(300, 20, 100, 20));
		c.add(2800, 3).chains.push_back(line(290, 20, 400, 20));
		const PlainOut w = run_case("window clamped at both ends, reverse strand", P, c);
		EXPECT(w.plan.size() == 2 && w.plan[0].as == 0 && w.plan[1].ae == 3000 && w.plan[0].ae < 3000 && w.plan[1].as > 0);
	}
	for (int d : { 0, 1 }) {                                  // r.qs 9 against 10, qlen - r.qe 9 against 10: max_ext against max_intron / 2
		Case c; set_protein(c, 200 + d);
		c.add(4000, 4).chains.push_back(line(300, 20, 13 + d, 178, 3, 1));         // qs = 9 + d; qe = 13 + d + 177 + 1 = 191 + d: qlen - qe = 9
		PlainOut w = run_case(d ? "qs 10" : "qs 9", P, c);
		EXPECT(w.plan.size() == 1 && w.reg[0].qs == 9 + d && w.reg[0].vs - w.plan[0].as == (d ? 2000 : 1000));
		Case e; set_protein(e, 200 + d);
		e.add(4000, 4).chains.push_back(line(300, 20, 20, 171, 3, 1));              // qe = 191: qlen - qe = 9 + d
		w = run_case(d ? "qlen - qe 10" : "qlen - qe 9", P, e);
		EXPECT(w.plan.size() == 1 && w.plan[0].ae - w.reg[0].ve == (d ? 2000 : 1000));
	}
	{	// neighbours on one strand whose queries overlap: 0 bases apart and 50 (both below 100: 100), 300 (below max_intron / 2: 300)
		Case c; set_protein(c, 900);
		PlansParams p = P;
		p.mask_level = 0.95f;
		c.add(1000, 4).chains.push_back(line(300, 14, 100, 100, 3, 1));            // vs 1000, ve 1000 + 14 + 297 + 1 = 1312
		c.add(1312, 4).chains.push_back(line(290, 14, 190, 100, 3, 1));            // vs 1312: 0 apart; ve 1624
		c.add(1674, 4).chains.push_back(line(280, 14, 280, 100, 3, 1));            // vs 1674: 50 apart; ve 1986
		c.add(2286, 4).chains.push_back(line(270, 14, 370, 100, 3, 1));            // vs 2286: 300 apart
		const PlainOut w = run_case("limits between neighbours", p, c);
		EXPECT(w.plan.size() == 4 && w.plan[0].ae == 1312 + 100 && w.plan[1].as == 1312 - 100 && w.plan[1].ae == 1624 + 100 && w.plan[2].ae == 1986 + 300 && w.plan[3].as == 2286 - 300);
	}
	// ---- right extension and repeats
	{	// has_right false through mid_qe == qlen (the anchors behind the last marked one lie beyond the protein's end) and through
		// mid_ve == ae (the anchor behind the last marked one has its position, at the contig's end)
		Case c; set_protein(c, 120);
		Chain ch = line(300, 20, 20, 17, 18, 6);             // q 20 .. 116
		ch.an.push_back({ 20 + 17 * 18, 119 });               // marked: 119 + 1 == qlen
		ch.an.push_back({ 20 + 18 * 18, 125 });
		c.add(100, 0).chains.push_back(ch);
		const PlainOut w = run_case("no right extension: the protein's end", P, c);
		EXPECT(w.plan.size() == 1 && !w.plan[0].has_right && w.plan[0].mid_qe == 120 && w.plan[0].t_right == -1 && w.plan[0].t_right2 == -1);
		Case e; set_protein(e, 400);
		Chain ce = line(300, 20, 20, 10, 18, 6);
		ce.an.push_back({ ce.an.back().first, ce.an.back().second + 6 });
		e.add(6000 - 1 - ce.an.back().first, 0).chains.push_back(ce);             // ve == the contig's length
		const PlainOut v = run_case("no right extension: the contig's end", P, e);
		EXPECT(v.plan.size() == 1 && !v.plan[0].has_right && v.plan[0].mid_ve == 6000 && v.plan[0].ae == 6000 && v.plan[0].mid_qe < 400);
	}
	for (int same : { 0, 1 }) {                               // io > io_end: two repeats; io == io_end: none.  Left windows shorter and longer than max_ext
		Case c; set_protein(c, 600);
		PlansParams p = P;
		if (same) p.io_end = p.io;
		c.add(300, 0).chains.push_back(line(300, 20, 5, 30));                       // qs < 10: window of max_ext clamped at 0: shorter than max_ext
		c.add(4000, 0).chains.push_back(line(280, 20, 300, 30));                    // qs >= 10: max_intron / 2 = 2 000 > max_ext
		const PlainOut w = run_case(same ? "io == io_end" : "io > io_end", p, c);
		EXPECT(w.plan.size() == 2);
		if (same) EXPECT(w.plan[0].t_left2 == -1 && w.plan[1].t_right2 == -1 && w.task.size() == 4 + w.seg.size() - (size_t)count_short(w));
		else {
			EXPECT(w.plan[0].t_left2 == 1 && w.plan[0].t_right2 == 3 && w.plan[1].t_left2 == w.plan[1].t_left + 1);
			EXPECT((w.task[1].flag & MPA_F_SS_SKIP0) && w.task[1].nt_off == w.plan[0].as);                       // as_alt == as
			EXPECT(!(w.task[(size_t)w.plan[1].t_left2].flag & MPA_F_SS_SKIP0) && w.task[(size_t)w.plan[1].t_left2].nl == 1000);
		}
	}
	// ---- gap segments
	{	// gaps with nlen == 3 alen at alen == kmer2 (the shortcut) and kmer2 + 1 (a DP task), alen 4 and 5 (no multiples of 3: the
		// ceil(alen / 3) codons of the quirk), a codon with an N inside a shortcut gap, and a gap that is not in frame by its lengths
		Case c; set_protein(c, 900);
		Chain ch = line(300, 20, 20, 8, 15, 5);               // alen 5 == kmer2: shortcut
		extend(ch, 8, 18, 6, 18, 6);                          // alen 6: DP
		extend(ch, 8, 12, 4, 12, 4);                          // alen 4
		extend(ch, 6, 6, 5, 6, 5);                            // nlen 6, alen 5: DP
		extend(ch, 12, 3, 1, 3, 1);                           // alen 1
		const int64_t as = 500;
		c.add(as, 2).chains.push_back(ch);
		const int64_t vs = as + 20 + 1 - 15;
		for (int k = 0; k < 3; ++k) g_fwd[(size_t)(g_ctg_off[1] + vs + 15 + 21 + 15 * k)] = 4;                 // Ns in the first codons of three shortcut gaps
		const PlainOut w = run_case("shortcut at kmer2, task at kmer2 + 1, an N", P, c);
		int n5 = 0, n6 = 0, n4 = 0, n1 = 0, odd = 0;
		for (const SegRec &s : w.seg) {
			const int alen = s.ae1 - s.ae0, nlen = s.ne1 - s.ne0;
			n5 += alen == 5 && nlen == 15 && s.task < 0, n6 += alen == 6 && nlen == 18 && s.task >= 0, n4 += alen == 4 && s.task < 0, n1 += alen == 1 && s.task < 0;
			odd += nlen != 3 * alen && s.task >= 0;
		}
		EXPECT(w.plan.size() == 1 && n5 >= 5 && n6 >= 5 && n4 >= 5 && n1 >= 3 && odd >= 3);
	}
	{	// -A: the step stops behind the selection
		Case c; set_protein(c, 600);
		PlansParams p = P;
		p.no_align = 1;
		c.add(100, 0, 2, 40, 1).chains.push_back(line(300, 20, 20, 30)), c.add(3000, 1, 1, 30, 2).chains.push_back(line(200, 20, 25, 30));
		const PlainOut w = run_case("no alignment", p, c);
		EXPECT(w.reg.size() == 2 && w.plan.empty() && w.task.empty() && w.reg[0].cnt == 30);
	}
	{	// what the first region pass left in n_sub and subsc is carried: a secondary adds to them
		Case c; set_protein(c, 600);
		c.add(100, 0, 3, 55, 1).chains.push_back(line(300, 20, 20, 30)), c.add(3000, 2, 2, 44, 2).chains.push_back(line(200, 20, 22, 30));
		const PlainOut w = run_case("carried n_sub and subsc", P, c);
		EXPECT(w.reg.size() == 2 && w.reg[1].parent == 0 && w.reg[0].n_sub == 4 && w.reg[0].subsc == 200 && w.reg[1].n_sub == 2 && w.reg[1].subsc == 44 && w.reg[1].split == 2);
	}
	// ---- random inputs: small parameters so that every branch is taken
	for (int it = 0; it < 400; ++it) {
		Case c;
		set_protein(c, 150 + (int32_t)rnd(600));
		PlansParams p = P;
		p.best_n = 1 + (int32_t)rnd(8), p.mask_len = rnd(3) ? 0x7fffffff : (int32_t)rnd(40), p.max_ext = rnd(2) ? 300 : 1000, p.max_intron = rnd(2) ? 1000 : 4000;
		p.pri_ratio = rnd(4) ? 0.49f : 0.0f, p.mask_level = rnd(2) ? 0.5f : 0.9f, p.io_end = rnd(3) ? 19 : 29, p.kmer2 = 4 + (int32_t)rnd(3), p.no_align = rnd(12) == 0;
		const int n_win = (int)rnd(it % 25 == 0 ? 100 : 10);
		for (int k = 0; k < n_win; ++k) {
			const uint32_t vid = (uint32_t)rnd(6);
			const int64_t len = kCtgLen[vid >> 1];
			const int64_t as = (int64_t)rnd((uint64_t)len - 1200);
			Window &w = c.add(as, vid, (int32_t)rnd(3), (int32_t)rnd(60), (int32_t)rnd(3));
			const int n_ch = (int)rnd(4);
			for (int h = 0; h < n_ch; ++h) {
				Chain ch{ 20 + (int32_t)rnd(rnd(2) ? 6 : 400), {} };
				const int cnt = 1 + (int)rnd(h == 0 && k % 5 == 0 ? 200 : 40);
				int32_t x = 3 * p.kmer2 + (int32_t)rnd(60), q = p.kmer2 - 1 + (int32_t)rnd(40);
				for (int i = 0; i < cnt && x < 1100 && q < c.qlen - 1; ++i) {
					ch.an.push_back({ x, q });
					const int mode = (int)rnd(10);
					if (mode < 5) x += 3, q += 1;                                       // tight, in frame
					else if (mode < 7) { const int s = 1 + (int)rnd(6); x += 3 * s, q += s; }   // in frame, up to the thresholds
					else if (mode == 7) x += 18 + (int32_t)rnd(4), q += 6 + (int32_t)rnd(2);    // at and beyond them
					else if (mode == 8) x += 1 + (int32_t)rnd(30), q += 1 + (int32_t)rnd(9);    // out of frame
					else x += 3 * (int32_t)rnd(3), q += (int32_t)rnd(8);                  // steps that stand still on one side
				}
				if (!ch.an.empty()) w.chains.push_back(ch);
			}
		}
		char nm[64];
		snprintf(nm, sizeof nm, "random %d", it);
		run_case(nm, p, c, it % 8 == 0);
	}
	printf("plans_check: %d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
