// regions_check.cpp -- a stand-alone check of miniprot_amd/csrc/regions_core.h (tests/test_regions_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written and random main chains over a hand-written bo[] go through the shared core
// twice -- with a team of one (RegionsSerial, what MPA_GPU_REGIONS=model runs) and with a team of 64 host threads that meet at a
// barrier for every sync and sum (the device's wavefront in slow motion: same lane-strided loops, same lane-0 work) -- and are
// compared, field by field, with plain restatements of the five host functions (host_regions.cpp: regions_from_chains, sort_regions,
// assign_parents, select_secondary with its renumbering, extension_limits) on std::vector, written here after hit.c:32-287.  The
// order of equal scores is the reference's unstable radix sort: both sides take it from sort_pairs_by_x_core (chain_core.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <thread>
#include <vector>
#include <pthread.h>
#include "regions_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static uint64_t g_slot[64];
static thread_local int tl_lane = 0;
struct RegionsThreads {
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
};

static uint64_t g_rng = 88172645463325252ULL;
static uint64_t rnd(uint64_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng % n; }

// ---- the plain side ---------------------------------------------------------------------------------
struct Plain { int32_t off = 0, cnt = 0, id = 0, parent = 0, n_sub = 0, subsc = 0, chn_sc = 0, chn_sc_ungap = 0; uint32_t vid = 0; int32_t qs = 0, qe = 0; int64_t vs = 0, ve = 0; int32_t split = 0; };

static int32_t plain_block2vid(const std::vector<uint32_t> &bo, uint32_t blk)
{
	int32_t v = -1;                                            // the largest v with bo[v] <= blk, by a plain scan
	for (int32_t i = 0; i + 1 < (int32_t)bo.size(); ++i) if (bo[i] <= blk) v = i;
	return v;
}

static void plain_from_chains(const RegionsParams &p, const std::vector<uint32_t> &bo, const std::vector<uint64_t> &u, const std::vector<uint64_t> &a, std::vector<Plain> &out)
{
	out.assign(u.size(), Plain());
	int32_t k = 0;
	for (size_t c = 0; c < u.size(); ++c) {
		const int32_t n = (int32_t)(uint32_t)u[c];
		Plain &r = out[c];
		r.off = k, r.cnt = n;
		int32_t first = k, last = k + n - 1;
		const int32_t vf = plain_block2vid(bo, (uint32_t)(a[first] >> 32)), vl = plain_block2vid(bo, (uint32_t)(a[last] >> 32));
		if (vf == vl) r.vid = (uint32_t)vf;
		else {
			int32_t n_head = 0, n_tail = 0;                     // anchors on the first strand, anchors on the last
			for (int32_t j = k; j < k + n && (a[j] >> 32) < bo[vf + 1]; ++j) ++n_head;
			for (int32_t j = k + n - 1; j >= k + n_head && (a[j] >> 32) >= bo[vl]; --j) ++n_tail;
			if (n_head > n_tail) r.vid = (uint32_t)vf, last = k + n_head - 1, r.split = 1;
			else r.vid = (uint32_t)vl, first = k + n - n_tail, r.split = 2;
		}
		r.vs = (int64_t)((a[first] >> 32) - bo[r.vid]) << p.bbit;
		r.ve = (int64_t)((a[last] >> 32) - bo[r.vid] + 1) << p.bbit;
		r.qs = (int32_t)(uint32_t)a[first], r.qe = (int32_t)(uint32_t)a[last];
		const int32_t sc = (int32_t)(u[c] >> 32);
		r.chn_sc = vf == vl ? sc : (int32_t)(uint32_t)((double)sc * (last - first + 1) / n + .499);
		int32_t x = p.kmer;
		for (int32_t i = 1; i < n; ++i) {
			const int32_t dq = (int32_t)a[k + i] - (int32_t)a[k + i - 1];
			x += std::min(dq, p.kmer);
			if (a[k + i] >> 32 == a[k + i - 1] >> 32) x += 2;
		}
		r.chn_sc_ungap = x;
		k += n;
	}
}

static void plain_sort(std::vector<Plain> &r)
{
	const int32_t n = (int32_t)r.size();
	if (n <= 1) return;
	std::vector<Pair64> key;
	for (int32_t i = 0; i < n; ++i) key.push_back(Pair64{ (uint64_t)r[i].chn_sc << 32, (uint64_t)i });
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
	for (int i = 0; i < n; ++i) r[i].id = i;
	std::vector<int> prim(1, 0);
	r[0].parent = 0;
	for (int i = 1; i < n; ++i) {
		Plain &ri = r[i];
		const int si = ri.qs, ei = ri.qe;
		std::vector<uint64_t> cov;
		for (int w : prim) {
			const int sj = r[w].qs, ej = r[w].qe;
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
				Plain &rp = r[w];
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
		const int p = r[i].parent;
		const Plain &rp = p < (int)kept.size() ? kept[p] : r[p];   // (the reference reads the array it is compacting)
		const bool same = r[i].qs == rp.qs && r[i].qe == rp.qe && r[i].vid == rp.vid && r[i].vs == rp.vs && r[i].ve == rp.ve;
		bool keep = false;
		if (p == i) keep = true;
		else if ((r[i].chn_sc >= rp.chn_sc * pri_ratio || r[i].chn_sc + min_diff >= rp.chn_sc) && n_2nd < best_n) { if (!same) keep = true, ++n_2nd; }
		else if (top_ungap > 0 && r[i].chn_sc_ungap >= top_ungap * pri_ratio && n_2nd < best_n) { if (!same) keep = true, ++n_2nd; }
		if (keep) kept.push_back(r[i]);
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

static void plain_limits(const std::vector<Plain> &r, const std::vector<uint64_t> &a, int32_t min_ext, int32_t max_ext, std::vector<uint64_t> &ext)
{
	const int32_t n = (int32_t)r.size();
	ext.assign((size_t)n, 0);
	if (n <= 0) return;
	std::vector<Pair64> pos((size_t)n);
	for (int32_t i = 0; i < n; ++i) pos[(size_t)i] = Pair64{ a[(size_t)r[(size_t)i].off] >> 32, (uint64_t)i };
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

// ---- a case -----------------------------------------------------------------------------------------
struct Chains {
	std::vector<uint64_t> u, a;
	// n anchors from (blk, q) in steps of (db, dq)
	void add(int32_t sc, uint32_t blk, int32_t q, int32_t n, uint32_t db, int32_t dq)
	{
		u.push_back((uint64_t)(uint32_t)sc << 32 | (uint32_t)n);
		for (int32_t i = 0; i < n; ++i) a.push_back((uint64_t)(blk + (uint32_t)i * db) << 32 | (uint32_t)(q + i * dq));
	}
	// explicit anchors
	void add(int32_t sc, const std::vector<std::pair<uint32_t, int32_t>> &an)
	{
		u.push_back((uint64_t)(uint32_t)sc << 32 | (uint32_t)an.size());
		for (auto &x : an) a.push_back((uint64_t)x.first << 32 | (uint32_t)x.second);
	}
};

static int g_cases = 0, g_fail = 0;
static const std::vector<uint32_t> kBo = { 0, 100, 200, 200, 200, 300, 400, 1000, 1600 };   // contig 1 has no blocks (strands 2 and 3); contig 3 is 600 blocks a strand
static RegionsParams params()
{
	RegionsParams p;
	p.n_vid = (int32_t)kBo.size() - 1, p.bbit = 8, p.kmer = 6, p.mask_len = 0x7fffffff, p.best_n = 30, p.max_ext = 10000, p.min_ext = 100, p.min_diff = 12;
	p.mask_level = 0.5f, p.pri_ratio = 0.7f * 0.7f;
	return p;
}

struct Got { int32_t k; std::vector<RegionRec> out; std::vector<uint64_t> ext; };
template<class C> static void run_core(const RegionsParams &p, const Chains &c, Got &g, int lanes)
{
	const int32_t n = (int32_t)c.u.size();
	const size_t N = (size_t)n;
	RegionRec zero;
	memset(&zero, 0, sizeof zero);
	std::vector<RegionRec> tmp(N, zero);
	std::vector<Pair64> key(N);
	std::vector<SortRange> stack(N / 64 + 4);
	std::vector<uint32_t> hist(768);
	std::vector<int32_t> prim(N), ctl(2);
	std::vector<uint64_t> cov(N);
	g.out.assign(N, zero), g.ext.assign(N, 0);
	const RegionsScratch S{ tmp.data(), key.data(), stack.data(), hist.data(), prim.data(), cov.data(), ctl.data() };
	if (lanes == 1) { g.k = regions_core<C>(p, kBo.data(), c.u.data(), n, c.a.data(), S, g.out.data(), g.ext.data()); return; }
	std::vector<int32_t> ks(64, -1);
	std::vector<std::thread> th;
	for (int l = 0; l < 64; ++l) th.emplace_back([&, l] { tl_lane = l; ks[(size_t)l] = regions_core<C>(p, kBo.data(), c.u.data(), n, c.a.data(), S, g.out.data(), g.ext.data()); });
	for (auto &t : th) t.join();
	g.k = ks[0];
	for (int l = 1; l < 64; ++l) if (ks[(size_t)l] != ks[0]) { fprintf(stderr, "lane %d returns %d, lane 0 %d\n", l, ks[(size_t)l], ks[0]); ++g_fail; }
}

static void compare(const char *name, const char *team, const std::vector<Plain> &w, const std::vector<uint64_t> &we, const Got &g)
{
	if (g.k != (int32_t)w.size()) { fprintf(stderr, "MISMATCH %s (%s): %d regions, expected %zu\n", name, team, g.k, w.size()); ++g_fail; return; }
	for (size_t i = 0; i < w.size(); ++i) {
		const Plain &x = w[i];
		const RegionRec &y = g.out[i];
#define F(f) if ((int64_t)x.f != (int64_t)y.f) { fprintf(stderr, "MISMATCH %s (%s): region %zu: " #f " %lld, expected %lld\n", name, team, i, (long long)y.f, (long long)x.f); ++g_fail; return; }
		F(off) F(cnt) F(id) F(parent) F(n_sub) F(subsc) F(chn_sc) F(chn_sc_ungap) F(vid) F(qs) F(qe) F(vs) F(ve) F(split)
#undef F
		if (we[i] != g.ext[i]) { fprintf(stderr, "MISMATCH %s (%s): region %zu: limits %#llx, expected %#llx\n", name, team, i, (unsigned long long)g.ext[i], (unsigned long long)we[i]); ++g_fail; return; }
	}
}

// what the plain side found, for the cases that must show something
struct Seen { int n = 0, n_before = 0, split1 = 0, split2 = 0, secondaries = 0, max_parent = 0, min_left = 1 << 30, min_right = 1 << 30; std::vector<Plain> r; std::vector<uint64_t> ext; };
static Seen run_case(const char *name, const RegionsParams &p, const Chains &c, bool wave = true)
{
	std::vector<Plain> w;
	std::vector<uint64_t> we;
	plain_from_chains(p, kBo, c.u, c.a, w);
	Seen s;
	s.n_before = (int)w.size();
	for (const Plain &x : w) s.split1 += x.split == 1, s.split2 += x.split == 2;
	plain_sort(w);
	plain_parents(p.mask_level, p.mask_len, w);
	plain_select(p.pri_ratio, p.min_diff, p.best_n, w);
	plain_limits(w, c.a, p.min_ext, p.max_ext, we);
	s.n = (int)w.size();
	for (size_t i = 0; i < w.size(); ++i) {
		s.secondaries += w[i].parent != (int)i, s.max_parent = std::max(s.max_parent, w[i].parent);
		s.min_left = std::min(s.min_left, (int)(we[i] >> 32)), s.min_right = std::min(s.min_right, (int)(uint32_t)we[i]);
	}
	s.r = w, s.ext = we;
	Got g;
	run_core<RegionsSerial>(p, c, g, 1);
	compare(name, "team of one", w, we, g);
	if (wave) {
		run_core<RegionsThreads>(p, c, g, 64);
		compare(name, "team of 64", w, we, g);
	}
	++g_cases;
	return s;
}
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "CASE DOES NOT SHOW WHAT IT IS FOR: %s (line %d)\n", #cond, __LINE__); ++g_fail; } } while (0)

int main()
{
	pthread_barrier_init(&g_bar, nullptr, 64);
	const RegionsParams P = params();
	{ Chains c; const Seen s = run_case("zero chains", P, c); EXPECT(s.n == 0); }
	{ Chains c; c.add(50, 10, 5, 8, 1, 7); const Seen s = run_case("one chain", P, c); EXPECT(s.n == 1 && s.r[0].parent == 0); }
	{	// chains spanning two strands: head larger, tail larger, equal (the tail wins); across a contig boundary and the empty strands
		Chains c;
		c.add(90, { { 95, 10 }, { 96, 20 }, { 97, 30 }, { 101, 40 }, { 102, 50 } });
		c.add(80, { { 98, 110 }, { 99, 120 }, { 100, 130 }, { 101, 140 }, { 103, 150 } });
		c.add(70, { { 98, 210 }, { 99, 220 }, { 100, 230 }, { 101, 240 } });
		c.add(60, { { 198, 310 }, { 199, 320 }, { 199, 330 }, { 200, 340 } });       // strand 1 -> strand 4: strands 2 and 3 have no blocks
		c.add(55, { { 199, 410 }, { 200, 420 }, { 201, 430 }, { 299, 440 }, { 300, 450 } });   // ... three strands: head 1, tail 1 of the last: the tail
		const Seen s = run_case("chains across strands", P, c);
		EXPECT(s.split1 == 2 && s.split2 == 3 && s.n_before == 5);
	}
	{	// a strand with no blocks in front of the chain: block 250 lies on strand 4
		Chains c;
		c.add(40, 250, 5, 6, 1, 9), c.add(30, 200, 100, 4, 2, 9);
		const Seen s = run_case("behind the empty strands", P, c);
		EXPECT(s.n == 2 && s.r[0].vid == 4 && s.r[1].vid == 4 && s.r[1].vs == 0);
	}
	// ties in the sort: 65 and 300 regions of one score reach the radix passes, 64 and fewer take the insertion sort
	for (int n : { 2, 63, 64, 65, 130, 300 }) {
		Chains c;
		RegionsParams p = P;
		p.best_n = 1000;
		for (int i = 0; i < n; ++i) c.add(77, 400 + (uint32_t)((i * 37) % 590), 10 + (i % 5) * 3, 4, 1, 6);
		char nm[64];
		snprintf(nm, sizeof nm, "%d regions of one score", n);
		const Seen s = run_case(nm, p, c, n == 65 || n == 300 || n == 63);
		EXPECT(s.n_before == n && s.n > n / 2);
	}
	{	// runs of equal scores of at most 64 among 200 regions, and scores in two bytes
		Chains c;
		RegionsParams p = P;
		p.best_n = 1000, p.pri_ratio = 0.01f;
		for (int i = 0; i < 200; ++i) c.add(40 + (i % 7) * 60 + (i % 3 == 0 ? 256 : 0), 400 + (uint32_t)((i * 53) % 590), (i % 40) * 25, 3 + i % 4, 1, 5);
		const Seen s = run_case("runs of equal scores", p, c);
		EXPECT(s.n_before == 200);
	}
	{	// secondary to the SECOND of two overlapping primaries: [0, 100) and [60, 200) are both primary, [120, 190) overlaps only the second
		Chains c;
		c.add(300, { { 10, 0 }, { 11, 100 } }), c.add(250, { { 30, 60 }, { 32, 200 } }), c.add(200, { { 50, 120 }, { 51, 190 } }), c.add(190, { { 420, 130 }, { 421, 195 } });
		const Seen s = run_case("secondary to the second primary", P, c);
		EXPECT(s.n == 4 && s.r[1].parent == 1 && s.r[2].parent == 1 && s.r[3].parent == 1 && s.r[1].n_sub >= 1 && s.r[1].subsc == 200);
	}
	for (int d : { 0, 1 }) {                                  // uncovered == mask_len, and one above
		Chains c;
		RegionsParams p = P;
		p.mask_len = 10;
		c.add(300, { { 10, 0 }, { 11, 100 } }), c.add(200, { { 50, 20 }, { 51, 110 + d } });
		const Seen s = run_case(d ? "uncovered one above mask_len" : "uncovered at mask_len", p, c);
		EXPECT(s.n == 2 && s.r[1].parent == (d ? 1 : 0));
	}
	{	// best_n reached: twelve secondaries of one primary, four allowed
		Chains c;
		RegionsParams p = P;
		p.best_n = 4;
		c.add(300, { { 10, 0 }, { 11, 100 } });
		for (int i = 0; i < 12; ++i) c.add(290 - i, { { 420 + 10 * (uint32_t)i, 1 }, { 421 + 10 * (uint32_t)i, 99 } });
		const Seen s = run_case("best_n reached", p, c);
		EXPECT(s.n == 5 && s.secondaries == 4);
	}
	{	// two regions at the same place: same_place drops one, renumber runs; a primary behind the dropped one keeps its children
		Chains c;
		c.add(300, { { 10, 0 }, { 10, 20 }, { 10, 40 }, { 10, 60 }, { 11, 80 }, { 11, 100 } }), c.add(299, { { 10, 0 }, { 11, 100 } });
		c.add(250, { { 500, 200 }, { 501, 300 } }), c.add(240, { { 600, 210 }, { 601, 290 } });
		c.add(10, { { 700, 5 }, { 701, 95 } });               // (far below both ratios: dropped too)
		const Seen s = run_case("same place", P, c);
		EXPECT(s.n == 3 && s.r[1].parent == 1 && s.r[2].parent == 1 && s.r[2].id == 2);
	}
	{	// neighbours on one strand closer than max_ext (30 blocks = 7680 bases) and closer than 100 (adjacent blocks: 0 bases), overlapping queries
		Chains c;
		c.add(300, { { 410, 0 }, { 411, 100 } }), c.add(280, { { 412, 90 }, { 413, 200 } }), c.add(260, { { 443, 190 }, { 444, 300 } }), c.add(240, { { 900, 290 }, { 901, 400 } });
		const Seen s = run_case("limits between neighbours", P, c);
		EXPECT(s.n == 4 && s.min_left == 100 && s.min_right == 100);
		bool mid = false;
		for (uint64_t e : s.ext) mid |= (e >> 32) == 29 * 256 || (uint32_t)e == 29 * 256;
		EXPECT(mid);
	}
	for (int n : { 128, 129, 200, 1000 }) {                  // chains longer than REGIONS_TEAM_CHAIN: the binned score as a team sum
		Chains c;
		c.add(5000, 400, 0, n, 0, 3), c.add(4000, 1000, 7, n + 1, 1, 9), c.add(100, 20, 0, 5, 1, 2);
		char nm[64];
		snprintf(nm, sizeof nm, "long chains (%d)", n);
		const Seen s = run_case(nm, P, c);
		EXPECT(s.n >= 2 && s.r[0].chn_sc_ungap == 6 + (n - 1) * 5);
	}
	// random chains over all strands, a fifth of them across a strand boundary, with small parameters so that every branch is taken
	for (int it = 0; it < 400; ++it) {
		Chains c;
		RegionsParams p = P;
		p.best_n = 1 + (int32_t)rnd(8), p.mask_len = rnd(3) ? 0x7fffffff : (int32_t)rnd(40), p.max_ext = rnd(2) ? 1000 : 50000;
		p.pri_ratio = rnd(4) ? 0.49f : 0.0f, p.mask_level = rnd(2) ? 0.5f : 0.9f;
		const int n = (int)rnd(it % 25 == 0 ? 180 : 14);
		for (int k = 0; k < n; ++k) {
			const int cnt = 1 + (int)rnd(k % 9 == 0 ? 160 : 9);
			const uint32_t edge[6] = { 100, 200, 300, 400, 1000, 1600 };
			uint32_t blk = rnd(5) == 0 ? edge[rnd(5)] - (uint32_t)rnd(cnt + 1) : (uint32_t)rnd(1590);
			if (blk > 1599) blk = 0;
			std::vector<std::pair<uint32_t, int32_t>> an;
			int32_t q = (int32_t)rnd(300);
			for (int i = 0; i < cnt && blk < 1600; ++i) { an.push_back({ blk, q }); blk += (uint32_t)rnd(3), q += 1 + (int32_t)rnd(12); }
			c.add(20 + (int32_t)rnd(rnd(2) ? 6 : 400), an);
		}
		char nm[64];
		snprintf(nm, sizeof nm, "random %d", it);
		run_case(nm, p, c, it % 8 == 0);
	}
	printf("regions_check: %d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
