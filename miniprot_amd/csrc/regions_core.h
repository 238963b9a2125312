// regions_core.h -- from the main chains of a query to its refinement windows (row a17 of DESIGN.md section 1; section 4.6):
// regions_from_chains (hit.c:32-76), sort_regions (hit.c:97-126), assign_parents (hit.c:128-187), select_secondary (hit.c:189-236)
// and extension_limits (hit.c:252-287) of host_regions.cpp as ONE source for the host and the device, like chain_core.h and
// aln_stats_core.h.  The regions here are fresh from the chains -- none is aligned, every hash is 0 -- so the branches of the host
// functions that look at alignments do not occur and are left out.
//
// Execution model.  The code is written for a TEAM (policy C: RegionsSerial = one host thread, RegionsWave = the 64 lanes of a
// wavefront, region_kernels.hip).  What is independent per chain is shared out over the lanes: chain c to lane c mod width() for the
// strand, the larger part of a chain that spans two strands, the coordinates and the binned score; the binned score of a chain of more
// than REGIONS_TEAM_CHAIN anchors is a sum over the whole team (integer addition: exact in any order).  Everything after that is
// serial by its nature and runs on lane 0, with a C::sync() on either side: the sort is the reference's unstable radix sort
// (sort_pairs_by_x_core, whose tie order is the result), region i of assign_parents depends on the primaries found before it, the
// selection compacts in place and reads its parent from the array being compacted.  A query has a few hundred chains at the most;
// what the device buys is that thousands of queries run side by side and that no anchor has to travel to the host.
//
// Floating point.  assign_parents' test `(float)ol / lo - (float)uncovered / hi > mask_level` and the selection's `sci >= scp *
// pri_ratio` are written as on the host.  The library is built with -ffp-contract=off (no fused multiply-add replaces a product and
// a sum) and HIP's float and double divisions are correctly rounded by default, so both sides compute the same IEEE values.
//
// Nothing here has a capacity: any number of chains, with scratch sized by their number n (RegionsScratch).
#pragma once
#include <stdint.h>
#include "chain_core.h"

namespace mpa {

#define REGIONS_TEAM_CHAIN 128           /* chains with more anchors: their binned score is summed by the whole team */

struct RegionRec {                       // Region (host_core.h) as far as a region from a chain has fields; 64 bytes
	int64_t vs, ve;
	int32_t off, cnt, id, parent, n_sub, subsc, chn_sc, chn_sc_ungap;
	uint32_t vid;
	int32_t qs, qe;
	int32_t split;                       // the chain spanned two strands / contigs (1: its head was kept, 2: its tail)
};

struct RegionsParams {
	int32_t n_vid;                       // 2 n_ctg: bo[] has n_vid + 1 entries
	int32_t bbit, kmer, mask_len, best_n, max_ext, min_ext, min_diff;
	float mask_level, pri_ratio;         // pri_ratio: what select_secondary takes (the option squared)
};

// work space for n chains
struct RegionsScratch {
	RegionRec *tmp;                      // [n] the regions before the sort
	Pair64 *key;                         // [n] sort keys (the region order, then the positions of extension_limits)
	SortRange *stack;                    // [n / 64 + 4]
	uint32_t *hist;                      // [768] digit tables of the sort
	int32_t *prim;                       // [n] first anchor of every chain; the primaries; renumber's table
	uint64_t *cov;                       // [n] coverage intervals
	int32_t *ctl;                        // [2] what lane 0 tells the team
};

struct RegionsSerial : CoopSerial {      // a team of one: the host
	static MPA_HD int32_t sum(int32_t v) { return v; }                    // over the team, the same on every lane
};

// mp_idx_block2pos (index.c:28-44), block2vid of index.cpp: the largest v with bo[v] <= blk.  A strand without blocks has
// bo[v] == bo[v + 1]: the search may land in front of it, the walk steps over it.  (An anchor's block is below bo[n]; the host
// returns -1 past it, here the last strand stands in so that nothing is read out of bounds.)
MPA_HD inline int32_t regions_block2vid(const uint32_t *bo, int32_t n, uint32_t blk)
{
	if (n <= 0) return 0;
	if (blk >= bo[n]) return n - 1;
	int32_t lo = 0, hi = n - 1;
	while (lo < hi) {
		const int32_t mid = (lo + hi + 1) >> 1;
		if (bo[mid] <= blk) lo = mid; else hi = mid - 1;
	}
	while (lo + 1 < n && bo[lo + 1] <= blk) ++lo;
	return lo;
}

// one term of binned_chain_score (hit.c:6-16): what anchor i adds behind anchor i - 1
MPA_HD inline int32_t regions_binned_term(uint64_t prev, uint64_t cur, int32_t kmer)
{
	const int32_t dq = (int32_t)cur - (int32_t)prev;
	return (dq < kmer ? dq : kmer) + (cur >> 32 == prev >> 32 ? 2 : 0);
}

// regions_from_chains (hit.c:32-76): u[n] (score << 32 | anchors) and the chains' anchors a[], chain by chain -> r[n]
template<class C> MPA_HD inline void regions_from_chains_core(const RegionsParams &p, const uint32_t *bo, const uint64_t *u, int32_t n, const uint64_t *a, const RegionsScratch &S,
                                                              RegionRec *r)
{
	if (C::lane() == 0) {
		int32_t k = 0;
		for (int32_t c = 0; c < n; ++c) S.prim[c] = k, k += (int32_t)(uint32_t)u[c];
	}
	C::sync();
	MPA_COOP_FOR(C, c, n) {
		const int32_t cnt = (int32_t)(uint32_t)u[c], k = S.prim[c];
		RegionRec x;
		x.off = k, x.cnt = cnt, x.id = 0, x.parent = 0, x.n_sub = 0, x.subsc = 0, x.split = 0;
		int32_t first = k, last = k + cnt - 1;
		const int32_t v_first = regions_block2vid(bo, p.n_vid, (uint32_t)(a[first] >> 32)), v_last = regions_block2vid(bo, p.n_vid, (uint32_t)(a[last] >> 32));
		if (v_first == v_last) x.vid = (uint32_t)v_first;
		else {                                            // the chain spans two strands/contigs: keep the larger part, the tail on a tie
			int32_t j, head_end, tail_beg;
			for (j = k; j < k + cnt; ++j) if ((a[j] >> 32) >= bo[v_first + 1]) break;
			head_end = j;
			for (j = k + cnt - 1; j >= head_end; --j) if ((a[j] >> 32) < bo[v_last]) break;
			tail_beg = j + 1;
			if (head_end - k > k + cnt - tail_beg) x.vid = (uint32_t)v_first, last = head_end - 1, x.split = 1;
			else x.vid = (uint32_t)v_last, first = tail_beg, x.split = 2;
		}
		x.vs = (int64_t)((a[first] >> 32) - bo[x.vid]) << p.bbit;
		x.ve = (int64_t)((a[last] >> 32) - bo[x.vid] + 1) << p.bbit;
		x.qs = (int32_t)(uint32_t)a[first];
		x.qe = (int32_t)(uint32_t)a[last];
		const int32_t sc = (int32_t)(u[c] >> 32);
		x.chn_sc = v_first == v_last ? sc : (int32_t)(uint32_t)((double)sc * (last - first + 1) / cnt + .499);   // (through a double, as the reference)
		int32_t s = p.kmer;
		if (cnt <= REGIONS_TEAM_CHAIN) for (int32_t i = 1; i < cnt; ++i) s += regions_binned_term(a[k + i - 1], a[k + i], p.kmer);
		x.chn_sc_ungap = s;
		r[c] = x;
	}
	C::sync();
	for (int32_t c = 0; c < n; ++c) {                     // the long chains, one after the other, each by the whole team
		const int32_t cnt = (int32_t)(uint32_t)u[c];
		if (cnt <= REGIONS_TEAM_CHAIN) continue;
		const uint64_t *ac = a + S.prim[c];
		int32_t s = 0;
		for (int32_t i = 1 + C::lane(); i < cnt; i += C::width()) s += regions_binned_term(ac[i - 1], ac[i], p.kmer);
		s = C::sum(s);
		if (C::lane() == 0) r[c].chn_sc_ungap = p.kmer + s;
	}
	C::sync();
}

// sort_regions (hit.c:97-126): best chain score first; equal scores in the order the reference's radix sort leaves them
template<class C> MPA_HD inline void regions_sort_core(const RegionRec *r, int32_t n, const RegionsScratch &S, RegionRec *out)
{
	if (n <= 1) {
		if (n == 1 && C::lane() == 0) out[0] = r[0];
		C::sync();
		return;
	}
	MPA_COOP_FOR(C, i, n) S.key[i] = Pair64{ (uint64_t)r[i].chn_sc << 32 | 0u, (uint64_t)i };   // (hash is always 0)
	C::sync();
	if (C::lane() == 0) sort_pairs_by_x_core(S.key, S.key + n, S.stack, S.hist);
	C::sync();
	MPA_COOP_FOR(C, j, n) out[j] = r[S.key[n - 1 - j].y];
	C::sync();
}

// assign_parents (hit.c:128-187) for regions that are not aligned.  One lane: region i depends on the primaries found before it
MPA_HD inline void regions_assign_parents(float mask_level, int32_t mask_len, RegionRec *r, int32_t n, int32_t *prim, uint64_t *cov)
{
	if (n <= 0) return;
	for (int32_t i = 0; i < n; ++i) r[i].id = i;
	int32_t n_prim = 0;
	prim[n_prim++] = 0;
	r[0].parent = 0;
	for (int32_t i = 1; i < n; ++i) {
		RegionRec &ri = r[i];
		const int32_t si = ri.qs, ei = ri.qe;
		int32_t uncovered = 0, n_cov = 0;
		bool is_primary = true;
		for (int32_t w = 0; w < n_prim; ++w) {             // parts of [si,ei) covered by primaries
			const int32_t sj = r[prim[w]].qs, ej = r[prim[w]].qe;
			if (ej <= si || sj >= ei) continue;
			cov[n_cov++] = (uint64_t)(sj > si ? sj : si) << 32 | (uint32_t)(ej < ei ? ej : ei);
		}
		if (n_cov > 0) {
			int32_t x = si;
			for (int32_t k = 1; k < n_cov; ++k) {           // (whole values are sorted: any correct sort gives sort_u64's order)
				const uint64_t v = cov[k];
				int32_t j = k;
				for (; j > 0 && cov[j - 1] > v; --j) cov[j] = cov[j - 1];
				cov[j] = v;
			}
			for (int32_t k = 0; k < n_cov; ++k) {
				const uint64_t c = cov[k];
				if ((int32_t)(c >> 32) > x) uncovered += (int32_t)(c >> 32) - x;
				x = (int32_t)c > x ? (int32_t)c : x;
			}
			if (ei > x) uncovered += ei - x;
			for (int32_t w = 0; w < n_prim; ++w) {         // the FIRST primary in list order that passes takes it
				RegionRec &rp = r[prim[w]];
				const int32_t sj = rp.qs, ej = rp.qe;
				if (ej <= si || sj >= ei) continue;
				const int32_t lo = ej - sj < ei - si ? ej - sj : ei - si, hi = ej - sj > ei - si ? ej - sj : ei - si;
				const int32_t ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
				if ((float)ol / lo - (float)uncovered / hi > mask_level && uncovered <= mask_len) {   // secondary to rp
					ri.parent = rp.parent;
					rp.subsc = rp.subsc > ri.chn_sc ? rp.subsc : ri.chn_sc;
					if (ri.cnt >= rp.cnt) ++rp.n_sub;
					is_primary = false;
					break;
				}
			}
		}
		if (is_primary) prim[n_prim++] = i, ri.parent = i, ri.n_sub = 0;
	}
}

// select_secondary (hit.c:189-236) with its renumbering (hit.c:189-210), in place as the reference: position p may already hold
// a moved element; parents precede their children and kept elements only move towards the front, which keeps r[p] the parent.
// where: [n].  Returns how many regions are left.
MPA_HD inline int32_t regions_select_secondary(float pri_ratio, int32_t min_diff, int32_t best_n, RegionRec *r, int32_t n, int32_t *where)
{
	if (!(pri_ratio > 0.0f) || n <= 0) return n;
	int32_t top_ungap = -1, n_2nd = 0, k = 0;
	for (int32_t i = 0; i < n; ++i) top_ungap = top_ungap > r[i].chn_sc_ungap ? top_ungap : r[i].chn_sc_ungap;
	for (int32_t i = 0; i < n; ++i) {
		const int32_t p = r[i].parent;
		const RegionRec &rp = r[p];
		const RegionRec &x = r[i];
		const int32_t sci = x.chn_sc, scp = rp.chn_sc;
		const bool same_place = x.qs == rp.qs && x.qe == rp.qe && x.vid == rp.vid && x.vs == rp.vs && x.ve == rp.ve;
		bool keep = false;
		if (p == i) keep = true;
		else if ((sci >= scp * pri_ratio || sci + min_diff >= scp) && n_2nd < best_n) {
			if (!same_place) keep = true, ++n_2nd;
		} else if (top_ungap > 0 && x.chn_sc_ungap >= top_ungap * pri_ratio && n_2nd < best_n) {
			if (!same_place) keep = true, ++n_2nd;
		}
		if (keep) { const RegionRec v = r[i]; r[k++] = v; }
	}
	if (k == n) return n;
	// renumber: ids and parents after dropping regions (ids before were the positions 0 .. n - 1)
	for (int32_t i = 0; i < n; ++i) where[i] = -1;
	for (int32_t i = 0; i < k; ++i) if (r[i].id >= 0) where[r[i].id] = i;
	int32_t max_id = -1;
	for (int32_t i = 0; i < k; ++i) max_id = max_id > r[i].id ? max_id : r[i].id;
	for (int32_t i = 0; i < k; ++i) {
		RegionRec &x = r[i];
		x.id = i;
		if (x.parent == -2) x.parent = i;
		else if (x.parent >= 0 && x.parent <= max_id && where[x.parent] >= 0) x.parent = where[x.parent];
		else x.parent = -1;
	}
	return k;
}

// extension_limits (hit.c:252-287) with the block of a region's first anchor as its position (the call with anchors != nullptr)
MPA_HD inline void regions_extension_limits(const RegionRec *r, int32_t n, const uint64_t *a, int32_t min_ext, int32_t max_ext, Pair64 *pos, SortRange *stack, uint32_t *hist,
                                            uint64_t *ext)
{
	if (n <= 0) return;
	for (int32_t i = 0; i < n; ++i) pos[i] = Pair64{ a[r[i].off] >> 32, (uint64_t)i };
	sort_pairs_by_x_core(pos, pos + n, stack, hist);
	for (int32_t i = 0; i < n; ++i) {
		const int32_t j = (int32_t)pos[i].y;
		const RegionRec &x = r[j];
		int32_t left = max_ext, right = max_ext;
		if (i > 0) {
			const RegionRec &q = r[pos[i - 1].y];
			if (q.vid == x.vid && q.qe >= x.qs) {
				left = (int32_t)(x.vs - q.ve < max_ext ? x.vs - q.ve : max_ext);
				left = left > min_ext ? left : min_ext;
			}
		}
		if (i < n - 1) {
			const RegionRec &q = r[pos[i + 1].y];
			if (q.vid == x.vid && x.qe >= q.qs) {
				right = (int32_t)(q.vs - x.ve < max_ext ? q.vs - x.ve : max_ext);
				right = right > min_ext ? right : min_ext;
			}
		}
		ext[j] = (uint64_t)(uint32_t)left << 32 | (uint32_t)right;
	}
}

// The whole stage for one query: out[] (room for n) receives the selected regions in the host's order and with its ids, ext[] (room
// for n) their refinement limits.  Every lane returns how many regions are left; n itself is the number of chains before selection.
template<class C> MPA_HD inline int32_t regions_core(const RegionsParams &p, const uint32_t *bo, const uint64_t *u, int32_t n, const uint64_t *a, const RegionsScratch &S,
                                                     RegionRec *out, uint64_t *ext)
{
	if (n <= 0) return 0;
	regions_from_chains_core<C>(p, bo, u, n, a, S, S.tmp);
	regions_sort_core<C>(S.tmp, n, S, out);
	if (C::lane() == 0) {
		regions_assign_parents(p.mask_level, p.mask_len, out, n, S.prim, S.cov);
		const int32_t k = regions_select_secondary(p.pri_ratio, p.min_diff, p.best_n, out, n, S.prim);
		regions_extension_limits(out, k, a, p.min_ext, p.max_ext, S.key, S.stack, S.hist, ext);
		S.ctl[0] = k;
	}
	C::sync();
	return S.ctl[0];
}

} // namespace mpa
