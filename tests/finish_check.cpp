// finish_check.cpp -- a stand-alone check of miniprot_amd/csrc/finish_core.h (tests/test_finish_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written and random tables of aligned regions go through the shared core twice -- with
// a team of one (FinishSerial, what MPA_GPU_FINISH=model runs) and with a team of 64 host threads that meet at a barrier for every sync,
// ballot, scan and sum (the device's wavefront in slow motion: same lane-strided loops, same lane-0 work) -- into output arrays of exactly
// the size the result needs (the sanitizer guards their ends), and are compared, byte by byte, with a plain restatement on std::vector
// of stage_finish() (host_align.cpp: sort_regions, prefer_multi_exon, assign_parents, select_secondary of host_regions.cpp, written here
// after hit.c:97-250) and of the flatten loop of mpa_batch_finish() (host_map.cpp).  The order of equal keys is the reference's unstable
// radix sort: both sides take it from sort_pairs_by_x_core (chain_core.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "finish_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static int64_t g_slot[64];
static thread_local int tl_lane = 0;
struct FinishThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static void sync() { pthread_barrier_wait(&g_bar); }
	static void gather(int64_t v, int64_t *all)
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		for (int i = 0; i < 64; ++i) all[i] = g_slot[i];
		pthread_barrier_wait(&g_bar);
	}
	static uint64_t ballot(bool p) { int64_t a[64]; gather(p, a); uint64_t m = 0; for (int i = 0; i < 64; ++i) m |= (uint64_t)(a[i] != 0) << i; return m; }
	static int rank(uint64_t m) { return __builtin_popcountll(m & ((1ull << tl_lane) - 1ull)); }
	static int popc(uint64_t m) { return __builtin_popcountll(m); }
	static int64_t scan_excl(int64_t v, int64_t *total) { int64_t a[64], s = 0, t = 0; gather(v, a); for (int i = 0; i < 64; ++i) { if (i < tl_lane) s += a[i]; t += a[i]; } *total = t; return s; }
	static int64_t sum64(int64_t v) { int64_t t; scan_excl(v, &t); return t; }
};

static uint64_t g_rng = 88172645463325252ULL;
static uint64_t rnd(uint64_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng % n; }

// ---- a table and a flat result ------------------------------------------------------------------------
struct Table {
	FinParams p;
	std::vector<int64_t> first;
	std::vector<FinRec> rec;
	std::vector<uint32_t> words;
	std::vector<mpa_feat_t> feats;
	std::string cs, rows;
};
struct Flat {
	std::vector<FinCounts> off;
	std::vector<mpa_hit_t> hits;
	std::vector<uint32_t> cigars;
	std::vector<mpa_feat_t> feats;
	std::vector<FinCsRef> cs;
	std::vector<FinRowsRef> rows;
	std::string cs_text, rows_text;
};

// ---- the plain side ---------------------------------------------------------------------------------
struct Plain { FinRec x; int32_t id = 0, src = 0; };

static void plain_rank(const FinParams &p, std::vector<Plain> &r)
{
	const int n0 = (int)r.size();
	if (n0 > 1) {                                             // sort_regions
		std::vector<Pair64> key;
		for (int i = 0; i < n0; ++i) if (r[i].x.cnt > 0) key.push_back(Pair64{ (uint64_t)r[i].x.dp_max << 32 | r[i].x.hash, (uint64_t)i });
		std::vector<SortRange> stack(key.size() / 64 + 8);
		std::vector<uint32_t> hist(768);
		sort_pairs_by_x_core(key.data(), key.data() + key.size(), stack.data(), hist.data());
		std::vector<Plain> s;
		for (size_t i = key.size(); i-- > 0;) s.push_back(r[key[i].y]);
		r.swap(s);
	}
	const int n = (int)r.size();
	if (n >= 2 && r[0].x.n_exon == 1) {                       // prefer_multi_exon
		int i = 1;
		while (i < n && r[i].x.n_exon < 2) ++i;
		if (i < n && r[0].x.dp_max < r[i].x.dp_max + p.io) std::swap(r[0], r[i]);
	}
	if (n <= 0) return;
	for (int i = 0; i < n; ++i) r[i].id = i;                  // assign_parents, aligned
	std::vector<int> prim(1, 0);
	r[0].x.parent = 0;
	for (int i = 1; i < n; ++i) {
		FinRec &ri = r[i].x;
		const int si = ri.qs, ei = ri.qe;
		std::vector<uint64_t> cov;
		for (int w : prim) { const int sj = r[w].x.qs, ej = r[w].x.qe; if (ej <= si || sj >= ei) continue; cov.push_back((uint64_t)std::max(sj, si) << 32 | (uint32_t)std::min(ej, ei)); }
		bool is_primary = true;
		if (!cov.empty()) {
			int x = si, uncovered = 0;
			std::sort(cov.begin(), cov.end());
			for (uint64_t c : cov) { if ((int)(c >> 32) > x) uncovered += (int)(c >> 32) - x; x = std::max((int)(int32_t)c, x); }
			if (ei > x) uncovered += ei - x;
			for (int w : prim) {
				FinRec &rp = r[w].x;
				const int sj = rp.qs, ej = rp.qe;
				if (ej <= si || sj >= ei) continue;
				const int lo = std::min(ej - sj, ei - si), hi = std::max(ej - sj, ei - si);
				const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
				if ((float)ol / lo - (float)uncovered / hi > p.mask_level && uncovered <= p.mask_len) {
					int counts = 0;
					ri.parent = rp.parent;
					rp.subsc = std::max(rp.subsc, ri.chn_sc);
					if (ri.cnt >= rp.cnt) counts = 1;
					if (rp.vid != ri.vid || rp.vs != ri.vs || rp.ve != ri.ve || ol != lo) { rp.dp_max2 = std::max(rp.dp_max2, ri.dp_max); if (rp.dp_max - ri.dp_max <= p.kmer) counts = 1; }
					if (counts) ++rp.n_sub;
					is_primary = false;
					break;
				}
			}
		}
		if (is_primary) prim.push_back(i), ri.parent = i, ri.n_sub = 0;
	}
	if (!(p.pri_ratio > 0.0f)) return;                        // select_secondary
	std::vector<Plain> kept;
	int n_2nd = 0;
	for (int i = 0; i < n; ++i) {
		const int pa = r[i].x.parent;
		const FinRec &rp = pa < (int)kept.size() ? kept[pa].x : r[pa].x, &x = r[i].x;
		bool keep = false;
		if (pa == i) keep = true;
		else if ((x.dp_max >= rp.dp_max * p.pri_ratio || x.dp_max + 2 * p.kmer >= rp.dp_max) && n_2nd < p.best_n)
			if (!(x.qs == rp.qs && x.qe == rp.qe && x.vid == rp.vid && x.vs == rp.vs && x.ve == rp.ve)) keep = true, ++n_2nd;
		if (keep) kept.push_back(r[i]);
	}
	const bool dropped = (int)kept.size() != n;
	r.swap(kept);
	if (!dropped) return;
	std::vector<int> where(n, -1);
	for (size_t i = 0; i < r.size(); ++i) where[r[i].id] = (int)i;
	for (size_t i = 0; i < r.size(); ++i) { r[i].id = (int)i; r[i].x.parent = r[i].x.parent >= 0 && where[r[i].x.parent] >= 0 ? where[r[i].x.parent] : -1; }
}

static void plain_flat(const Table &t, Flat &F)
{
	const size_t nq = t.first.size() - 1;
	F = Flat();
	F.off.resize(nq + 1);
	FinCounts a{ 0, 0, 0, 0, 0, 0, 0, 0 };
	for (size_t q = 0; q < nq; ++q) {
		std::vector<Plain> r;
		for (int64_t i = t.first[q]; i < t.first[q + 1]; ++i) { Plain y; y.x = t.rec[i], y.src = (int32_t)(i - t.first[q]); r.push_back(y); }
		plain_rank(t.p, r);
		F.off[q] = a;
		for (const Plain &y : r) {
			const FinRec &x = y.x;
			mpa_hit_t h;
			memset(&h, 0, sizeof h);
			h.qid = (int32_t)q, h.id = y.id, h.parent = x.parent, h.n_sub = x.n_sub, h.subsc = x.subsc, h.cnt = x.cnt, h.n_exon = x.n_exon, h.chn_sc = x.chn_sc, h.chn_sc_ungap = x.chn_sc_ungap;
			h.vid = x.vid, h.qs = x.qs, h.qe = x.qe, h.vs = x.vs, h.ve = x.ve, h.has_aln = 1, h.dp_score = x.dp_score, h.dp_max = x.dp_max, h.dp_max2 = x.dp_max2, h.blen = x.blen;
			h.n_fs = x.n_fs, h.n_stop = x.n_stop, h.dist_stop = x.dist_stop, h.dist_start = x.dist_start, h.n_iden = x.n_iden, h.n_plus = x.n_plus, h.n_cigar = x.n_cigar, h.n_feat = x.n_feat;
			h.cigar_off = (int64_t)F.cigars.size(), h.feat_off = (int64_t)F.feats.size();
			F.hits.push_back(h);
			F.cigars.insert(F.cigars.end(), t.words.begin() + x.cig_off, t.words.begin() + x.cig_off + x.n_cigar);
			for (int k = 0; k < x.n_feat; ++k) { mpa_feat_t f = t.feats[x.feat_off + k]; memset((char*)&f + 52, 0, 4); F.feats.push_back(f); }
			FinCsRef c{ 0, 0, 0 };
			if (x.cs_len >= 0) c = FinCsRef{ (int64_t)F.cs_text.size(), x.cs_len, 1 }, F.cs_text.append(t.cs, (size_t)x.cs_off, (size_t)x.cs_len), ++a.n_cs;
			F.cs.push_back(c);
			FinRowsRef w{ 0, 0, 0, 0, 0 };
			if (x.rows_stride >= 0) {
				w = FinRowsRef{ (int64_t)F.rows_text.size(), x.rows_w, x.rows_sta, 1, 0 }, ++a.n_rows;
				for (int k = 0; k < 4; ++k) F.rows_text.append(t.rows, (size_t)(x.rows_off + (int64_t)k * x.rows_stride), (size_t)x.rows_w);
				F.rows_text.append(t.rows, (size_t)(x.rows_off + 4 * (int64_t)x.rows_stride), (size_t)x.rows_sta);
			}
			F.rows.push_back(w);
		}
		a.hit = (int64_t)F.hits.size(), a.cigar = (int64_t)F.cigars.size(), a.feat = (int64_t)F.feats.size(), a.cs = (int64_t)F.cs_text.size(), a.rows = (int64_t)F.rows_text.size();
	}
	F.off[nq] = a;
}

// ---- the shared core: every lane of a team runs this ---------------------------------------------------
struct Work {
	std::vector<FinOut> out;
	std::vector<FinCounts> cnt;
	std::vector<FinRank> tmp, r;
	std::vector<Pair64> key;
	std::vector<SortRange> stack;
	std::vector<uint32_t> hist;
	std::vector<int32_t> prim;
	std::vector<uint64_t> cov;
	int32_t ctl[2];
	// exact-size heap blocks, so that the sanitizer sees a write one past the end
	mpa_hit_t *hits = nullptr; uint32_t *cigars = nullptr; mpa_feat_t *feats = nullptr; FinCsRef *cs = nullptr; FinRowsRef *rows = nullptr; char *cs_text = nullptr, *rows_text = nullptr;
};

template<class C> static void core_run(const Table &t, Work &W, Flat &F)
{
	const int64_t nq = (int64_t)t.first.size() - 1;
	for (int64_t q = 0; q < nq; ++q) {
		const int64_t f = t.first[q];
		const int32_t n = (int32_t)(t.first[q + 1] - f);
		const FinScratch S{ W.tmp.data(), W.r.data(), W.key.data(), W.stack.data(), W.hist.data(), W.prim.data(), W.cov.data(), W.ctl };
		finish_rank_core<C>(t.p, t.rec.data() + f, n, S, W.out.data() + f, &W.cnt[(size_t)q]);
		C::sync();
	}
	if (C::lane() == 0) {
		F.off.resize((size_t)nq + 1);
		finish_scan_serial(W.cnt.data(), nq, F.off.data());
		const FinCounts &tot = F.off[(size_t)nq];
		W.hits = (mpa_hit_t*)malloc((size_t)tot.hit * sizeof(mpa_hit_t) + 0), W.cigars = (uint32_t*)malloc((size_t)tot.cigar * 4), W.feats = (mpa_feat_t*)malloc((size_t)tot.feat * sizeof(mpa_feat_t));
		W.cs = (FinCsRef*)malloc((size_t)tot.hit * sizeof(FinCsRef)), W.rows = (FinRowsRef*)malloc((size_t)tot.hit * sizeof(FinRowsRef));
		W.cs_text = (char*)malloc((size_t)tot.cs), W.rows_text = (char*)malloc((size_t)tot.rows);
	}
	C::sync();
	const FinDst dst{ W.hits, W.cigars, W.feats, W.cs, W.cs_text, W.rows, W.rows_text };
	for (int64_t q = 0; q < nq; ++q) {
		const int64_t f = t.first[q];
		const FinCounts at = F.off[(size_t)q];
		for (int64_t j = 0; j < W.cnt[(size_t)q].hit; ++j) {
			const FinOut &o = W.out[(size_t)(f + j)];
			finish_gather_core<C>((int32_t)q, t.rec[(size_t)(f + o.src)], o, at.hit + j, at, t.words.data(), t.feats.data(), t.cs.data(), t.rows.data(), dst);
		}
	}
	C::sync();
	if (C::lane() == 0) {
		const FinCounts &tot = F.off[(size_t)nq];
		F.hits.assign(W.hits, W.hits + tot.hit), F.cigars.assign(W.cigars, W.cigars + tot.cigar), F.feats.assign(W.feats, W.feats + tot.feat);
		F.cs.assign(W.cs, W.cs + tot.hit), F.rows.assign(W.rows, W.rows + tot.hit), F.cs_text.assign(W.cs_text, (size_t)tot.cs), F.rows_text.assign(W.rows_text, (size_t)tot.rows);
		free(W.hits), free(W.cigars), free(W.feats), free(W.cs), free(W.rows), free(W.cs_text), free(W.rows_text);
	}
}

static void work_for(const Table &t, Work &W)
{
	int64_t big = 0;
	for (size_t q = 0; q + 1 < t.first.size(); ++q) big = std::max(big, t.first[q + 1] - t.first[q]);
	// (the scratch of the largest query, exactly: FINISH_STACK is the only piece with slack)
	W.out.resize(t.rec.size()), W.cnt.resize(t.first.size() - 1), W.tmp.resize((size_t)big), W.r.resize((size_t)big), W.key.resize((size_t)big), W.stack.resize((size_t)FINISH_STACK(big));
	W.hist.resize(768), W.prim.resize((size_t)big), W.cov.resize((size_t)big);
}

static int g_cases = 0, g_fail = 0;

template<class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T))); }
static bool same_flat(const Flat &a, const Flat &b)
{
	return same(a.off, b.off) && same(a.hits, b.hits) && same(a.cigars, b.cigars) && same(a.feats, b.feats) && same(a.cs, b.cs) && same(a.rows, b.rows) && a.cs_text == b.cs_text &&
	       a.rows_text == b.rows_text;
}

static void check(const char *name, const Table &t)
{
	Flat want, one, team;
	plain_flat(t, want);
	{ Work W; work_for(t, W); core_run<FinishSerial>(t, W, one); }
	{
		Work W;
		work_for(t, W);
		std::vector<std::thread> th;
		for (int l = 0; l < 64; ++l) th.emplace_back([&, l] { tl_lane = l; core_run<FinishThreads>(t, W, team); });
		for (std::thread &x : th) x.join();
	}
	++g_cases;
	if (!same_flat(one, want)) { ++g_fail; printf("MISMATCH %s: team of one against the plain restatement (%zu hits against %zu)\n", name, one.hits.size(), want.hits.size()); }
	if (!same_flat(team, want)) { ++g_fail; printf("MISMATCH %s: team of 64 against the plain restatement (%zu hits against %zu)\n", name, team.hits.size(), want.hits.size()); }
}

// ---- tables -------------------------------------------------------------------------------------------
static FinRec region(int32_t qs, int32_t qe, int32_t dp_max)
{
	FinRec x;
	memset(&x, 0, sizeof x);
	x.qs = qs, x.qe = qe, x.dp_max = dp_max, x.vs = 3 * (int64_t)qs + 1000, x.ve = 3 * (int64_t)qe + 1000, x.vid = (uint32_t)rnd(4), x.hash = (uint32_t)rnd(1u << 31), x.cnt = 1 + (int32_t)rnd(8);
	x.n_exon = 1 + (int32_t)rnd(3), x.chn_sc = (int32_t)rnd(300), x.chn_sc_ungap = (int32_t)rnd(300), x.parent = (int32_t)rnd(4), x.n_sub = (int32_t)rnd(3), x.subsc = (int32_t)rnd(40);
	x.dp_max2 = (int32_t)rnd(30), x.blen = (int32_t)rnd(900), x.n_iden = (int32_t)rnd(900), x.dist_stop = -1, x.cs_len = -1, x.rows_stride = -1;
	return x;
}
static FinRec random_region(int span, int n_scores)
{
	const int32_t qs = (int32_t)rnd((uint64_t)span - 10), qe = qs + 5 + (int32_t)rnd((uint64_t)std::min(115, span - qs - 5) + 1);
	return region(qs, qe, n_scores > 0 ? 40 + 3 * (int32_t)rnd((uint64_t)n_scores) : (int32_t)rnd(500) - 50);
}
// what hangs off the regions, behind a little slack in front of every array
static void payload(Table &t, bool edges, int cs_mode, int rows_mode)
{
	static const int kCig[5] = { 1, 63, 64, 65, 1000 }, kCs[4] = { 1, 255, 256, 5000 }, kW[6] = { 0, 1, 63, 64, 65, 300 };
	t.words.assign(3, 7u), t.feats.assign(1, mpa_feat_t()), t.cs.assign(5, '#'), t.rows.assign(7, '%');
	for (size_t i = 0; i < t.rec.size(); ++i) {
		FinRec &x = t.rec[i];
		x.dp_score = (int32_t)i;
		x.n_cigar = edges ? kCig[i % 5] : 1 + (int32_t)rnd(3), x.cig_off = (int64_t)t.words.size();
		for (int k = 0; k < x.n_cigar; ++k) t.words.push_back((uint32_t)rnd(1ull << 32));
		x.n_feat = edges ? 1 + (int32_t)((7 * i) % 40) : 1 + (int32_t)rnd(2), x.feat_off = (int64_t)t.feats.size();
		for (int k = 0; k < x.n_feat; ++k) { mpa_feat_t f; memset(&f, 0xa5, sizeof f); f.vs = (int64_t)rnd(1000), f.score = (int32_t)rnd(99); t.feats.push_back(f); }   // (padding not zero: the gather zeroes it)
		if (cs_mode == 1 || (cs_mode == 2 && rnd(2))) {
			x.cs_len = edges ? kCs[i % 4] : (int32_t)rnd(12), x.cs_off = (int64_t)t.cs.size();
			for (int k = 0; k < x.cs_len; ++k) t.cs.push_back((char)(33 + rnd(90)));
			t.cs.push_back('!');
		}
		if (rows_mode == 1 || (rows_mode == 2 && rnd(2))) {
			x.rows_w = edges ? kW[i % 6] : (int32_t)rnd(9), x.rows_sta = edges ? (int32_t)(i % 3) * 35 : (int32_t)rnd(4), x.rows_stride = x.rows_w + (int32_t)rnd(4), x.rows_off = (int64_t)t.rows.size();
			for (int k = 0; k < 4 * x.rows_stride + x.rows_sta; ++k) t.rows.push_back((char)(33 + rnd(90)));
		}
	}
}
static void add_query(Table &t, const std::vector<FinRec> &r) { t.rec.insert(t.rec.end(), r.begin(), r.end()), t.first.push_back((int64_t)t.rec.size()); }
static Table table(float mask_level, int32_t mask_len, float pri_ratio, int32_t best_n, int32_t io, int32_t kmer)
{
	Table t;
	t.p = FinParams{ kmer, mask_len, best_n, io, mask_level, pri_ratio };
	t.first.assign(1, 0);
	return t;
}

int main()
{
	pthread_barrier_init(&g_bar, nullptr, 64);
	{	// sizes around the sort's insertion threshold and its digit passes; ties
		Table t = table(0.5f, INT32_MAX, 0.7f, 30, 29, 6);
		for (int n : { 0, 1, 2, 3, 63, 64, 65, 257, 300 }) { std::vector<FinRec> r; for (int i = 0; i < n; ++i) r.push_back(random_region(300, 0)); add_query(t, r); }
		for (int n : { 70, 300 }) { std::vector<FinRec> r; for (int i = 0; i < n; ++i) r.push_back(random_region(300, 1)); add_query(t, r); }                     // all dp_max equal
		for (int n : { 5, 66, 260 }) { std::vector<FinRec> r; for (int i = 0; i < n; ++i) { FinRec x = random_region(300, 1); x.hash = 9; r.push_back(x); } add_query(t, r); }   // equal full keys
		{ std::vector<FinRec> r; for (int v : { -5, 12, -200, 0, 7, -1, -5, 300, -1000000000, 1000000000 }) r.push_back(region(20 * (int)r.size(), 20 * (int)r.size() + 30, v)); add_query(t, r); }
		payload(t, false, 1, 1);
		check("sizes and keys", t);
	}
	{	// the multi-exon swap at dp_max + io equal to, one below and one above the top
		Table t = table(0.5f, INT32_MAX, 0.7f, 30, 29, 6);
		for (int d : { 0, -1, 1 }) {
			std::vector<FinRec> r{ region(0, 50, 100), region(60, 90, 90), region(100, 150, 71 + d), region(160, 200, 72 + d) };
			r[0].n_exon = r[1].n_exon = 1, r[2].n_exon = 2, r[3].n_exon = 3;
			add_query(t, r);
		}
		payload(t, false, 0, 0);
		check("multi-exon", t);
	}
	{	// parents: secondary to the second of two overlapping primaries; uncovered at mask_len and one above; the identical hit after DP
		Table t = table(0.5f, 10, 0.7f, 30, 29, 6);
		add_query(t, { region(0, 100, 500), region(60, 160, 400), region(70, 150, 300), region(65, 155, 299), region(0, 160, 200) });
		add_query(t, { region(300, 500, 500), region(310, 510, 300) });
		add_query(t, { region(300, 500, 500), region(310, 511, 300) });
		{ std::vector<FinRec> r{ region(0, 100, 500), region(0, 100, 400), region(10, 100, 399), region(0, 100, 398) }; for (FinRec &x : r) x.vid = 1, x.vs = 1000, x.ve = 1300; r[3].vid = 2; add_query(t, r); }
		payload(t, false, 2, 2);
		check("parents", t);
	}
	for (int best_n : { 0, 1, 2, 30 }) for (float pr : { 0.0f, 0.3f }) {   // selection: the gaps at sub_diff, min_diff and pri_ratio; best_n; one place; soft-deleted entries
		Table t = table(0.5f, INT32_MAX, pr, best_n, 29, 6);
		add_query(t, { region(0, 100, 1000), region(0, 99, 994), region(1, 100, 993), region(2, 100, 500), region(3, 100, 299), region(4, 100, 300) });
		add_query(t, { region(0, 100, 17), region(0, 99, 5), region(1, 100, 4), region(2, 100, 6) });
		{ std::vector<FinRec> r{ region(0, 100, 100) }; for (int i = 1; i < 6; ++i) r.push_back(region(i, 100, 90 - i)); add_query(t, r); }
		{ std::vector<FinRec> r{ region(0, 100, 100), region(0, 100, 90), region(0, 100, 80) }; r[1].vid = r[0].vid, r[1].vs = r[0].vs, r[1].ve = r[0].ve; add_query(t, r); }
		{ std::vector<FinRec> r{ region(0, 100, 100), region(0, 100, 999), region(5, 100, 90), region(200, 250, 10) }; r[1].cnt = 0, r[3].cnt = -1; add_query(t, r); }
		{ std::vector<FinRec> r{ region(0, 10, 5) }; r[0].cnt = 0; add_query(t, r); }
		payload(t, false, 1, 0);
		check("selection", t);
	}
	{	// gather lengths; rows and cs present, absent and mixed
		for (int mode : { 0, 1, 2 }) {
			Table t = table(0.5f, INT32_MAX, 0.7f, 30, 29, 6);
			{ std::vector<FinRec> r; for (int i = 0; i < 12; ++i) r.push_back(region(40 * i, 40 * i + 30, 100 + i)); add_query(t, r); }
			{ std::vector<FinRec> r; for (int i = 0; i < 20; ++i) r.push_back(random_region(300, 5)); add_query(t, r); }
			add_query(t, {});
			payload(t, true, mode, mode);
			check("gather", t);
		}
	}
	for (int k = 0; k < 400; ++k) {                          // random tables under random options
		static const float kLevel[3] = { 0.1f, 0.5f, 0.9f }, kRatio[4] = { 0.0f, 0.3f, 0.7f, 1.0f };
		static const int32_t kLen[3] = { 0, 20, INT32_MAX }, kBest[4] = { 0, 1, 3, 30 };
		Table t = table(kLevel[rnd(3)], kLen[rnd(3)], kRatio[rnd(4)], kBest[rnd(4)], rnd(2) ? 29 : 0, rnd(2) ? 6 : 5);
		const int nq = 1 + (int)rnd(6), scores = (int)rnd(3) * 4;
		for (int q = 0; q < nq; ++q) {
			const int n = rnd(10) == 0 ? 100 + (int)rnd(120) : (int)rnd(30);
			std::vector<FinRec> r;
			for (int i = 0; i < n; ++i) {
				FinRec x = random_region(300, scores);
				if (rnd(4) == 0) x.hash = 7;
				if (rnd(25) == 0) x.cnt = 0;
				if (!r.empty() && rnd(7) == 0) { const FinRec &o = r[rnd(r.size())]; x.vid = o.vid, x.vs = o.vs, x.ve = o.ve; if (rnd(2)) x.qs = o.qs, x.qe = o.qe; }
				r.push_back(x);
			}
			add_query(t, r);
		}
		payload(t, false, (int)rnd(3), (int)rnd(3));
		check("random", t);
	}
	printf("finish_check: %d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail != 0;
}
