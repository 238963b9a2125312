// plans_core.h -- from the refinement chains of a query to its regions, alignment plans, round-1 DP tasks and gap segments (the part of
// rows a11 / a12 of DESIGN.md section 1 between the refinement and DP round 1; section 4.7): what mp_refine_reg() makes of a window's chains (map.c:89-111,
// refine_region_from_chains of host_plan.cpp), the second sort_regions / assign_parents / select_secondary, extension_limits in its
// genome-coordinate form (hit.c:252-287), mp_filter_seed (align.c:6-31, mark_reliable_anchors), the window and the extension
// calls of mp_align() (align.c:239-301, plan_alignment / plan_round1) and the gaps between its kept anchors with their ungapped
// shortcut (align.c:62-80, make_segment) as ONE source for the host and the device, like regions_core.h, whose pieces it is built
// from.  The regions are not aligned and every hash is 0, as there.
//
// Execution model.  The code is written for a TEAM (policy C: PlansSerial = one host thread, PlansWave = the 64 lanes of a
// wavefront, plan_kernels.hip) and a genome G (G::off / G::len of a contig, G::strand(vid) = the reader aln_stats_core.h takes).
//   parallel   the best chain of every window (window w to lane w mod width()); per window the terms of chain_score_ungapped, a
//              team sum of independent terms (integer addition: exact in any order), and the re-basing of its anchors; per region
//              the reliable-anchor marks -- the breaks between consecutive anchors are independent, so a maximal run is, and the
//              lane that owns a run's first anchor walks, trims and marks it --, the list of marked anchors (ballot + rank, in
//              order), and the gaps between them: gap g to lane g mod width(), its ungapped score or its DP task, the task's number
//              from a ballot over the gaps that need one
//   serial     the region order (the reference's unstable radix sort, whose tie order is the result), assign_parents (region i
//              depends on the primaries before it), select_secondary (compacts in place), extension_limits (a sort, then neighbours)
//              on lane 0 as in regions_core.h; the plan's scalars and its up to four extension tasks are computed by every lane
//              alike and stored by lane 0; regions follow each other, because a plan's task and segment numbers continue the
//              previous plan's
// Marks go to a flag per anchor, not into the anchors: no lane reads a word another lane is changing.
//
// Floating point: as regions_core.h (-ffp-contract=off, correctly rounded divisions).
// Nothing here has a capacity: scratch is sized by the windows and the anchors of the query (PlansScratch).
#pragma once
#include <stdint.h>
#include "regions_core.h"
#include "aln_stats_core.h"
#include "../../include/mpamd.h"

namespace mpa {

// a refinement window of the query and what its region carries over from the first region pass (assign_parents resets neither
// subsc nor the n_sub of the first region and of secondaries)
struct PlansWindow {
	int64_t as;                          // window start, strand-local on vid
	uint32_t vid;
	int32_t n_sub, subsc, split;
};

struct PlansParams {
	int32_t kmer2, kmer, mask_len, best_n, max_ext, max_intron, io, io_end, no_align, asize;
	float mask_level, pri_ratio;         // pri_ratio: what select_secondary takes (the option squared)
};

struct PlanRec {                         // AlignPlan (host_plan.cpp) after plan_round1, as far as it is set there; 80 bytes
	int64_t as, ae, vs0, vs1, mid_ve;
	int32_t reg, as1, mid_qe, has_right, t_left, t_left2, t_right, t_right2;
	int32_t gap0, n_gap;                 // its gap segments: seg[gap0 .. gap0 + n_gap)
};
struct SegRec { int32_t ne0, ne1, ae0, ae1, task, score; };   // Segment; task == -1: the ungapped shortcut, cigar = alen << 4

// one query
struct PlansQuery {
	int32_t n_win, qid, qlen;
	const PlansWindow *win;              // [n_win]
	const int64_t *cu, *ca, *nu;         // [n_win] window w's chains are u[cu[w] .. cu[w] + nu[w]), their anchors start at a[ca[w]]
	const uint64_t *u;                   // score << 32 | anchors, per chain
	uint64_t *a;                         // the chains' anchors; those of every window's best chain are re-based in place
	const uint8_t *seq;                  // the protein
};

// work space for n windows and m anchors (all chains of the query's windows)
struct PlansScratch {
	RegionRec *tmp;                      // [n]
	Pair64 *key;                         // [n]
	SortRange *stack;                    // [n / 64 + 4]
	uint32_t *hist;                      // [768]
	int32_t *prim;                       // [n] best chain of every window; then assign_parents' / select_secondary's table
	uint64_t *cov;                       // [n]
	uint64_t *ext;                       // [n]
	int64_t *aoff;                       // [n] where the best chain's anchors start in a[], -1 for a window without chains
	int32_t *flag, *list;                // [largest chain] marks; the marked anchors in order
	int32_t *ctl;                        // [2]
};

struct PlansCounts { int32_t n_reg, n_plan, n_task, n_seg; };

struct PlansSerial : CoopSerial {        // a team of one: the host
	static MPA_HD int32_t sum(int32_t v) { return v; }
};

// one term of chain_score_ungapped (hit.c:18-30): what anchor i adds behind anchor i - 1
MPA_HD inline int32_t plans_ungapped_term(uint64_t prev, uint64_t cur, int32_t kmer)
{
	const int32_t dq = (int32_t)cur - (int32_t)prev, dr3 = (int32_t)((cur >> 32) - (prev >> 32));
	const int32_t dr = dr3 / 3;
	if (dq >= dr && dr3 != dr * 3) return -1;
	const int32_t m = dq < dr ? dq : dr;
	return m < kmer ? m : kmer;
}

// mp_filter_seed's break between two consecutive anchors (align.c:12-16)
MPA_HD inline bool plans_break(uint64_t prev, uint64_t cur, int32_t max_aa_dist)
{
	const int32_t dx = (int32_t)(cur >> 32) - (int32_t)(prev >> 32), dy = (int32_t)cur - (int32_t)prev;
	return dx % 3 != 0 || dx > max_aa_dist * 3 || dy > max_aa_dist;
}

// extension_limits (hit.c:252-287) with the region's start on the genome as its position (the call with anchors == nullptr)
template<class G> MPA_HD inline void plans_extension_limits(const RegionRec *r, int32_t n, const G &g, int32_t min_ext, int32_t max_ext, Pair64 *pos, SortRange *stack,
                                                            uint32_t *hist, uint64_t *ext)
{
	if (n <= 0) return;
	for (int32_t i = 0; i < n; ++i) {
		const RegionRec &x = r[i];
		pos[i] = Pair64{ (uint64_t)(x.vs + g.off((int32_t)(x.vid >> 1)) + ((x.vid & 1) ? g.len((int32_t)(x.vid >> 1)) : 0)), (uint64_t)i };
	}
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

// ungapped_score (align.c:33-40) exactly as written: the nucleotide index advances by 3 but is bounded by the AMINO-ACID length,
// so only the first ceil(alen / 3) codons count
template<class S> MPA_HD inline int32_t plans_ungapped_score(const S &g, const uint8_t *tab, int32_t asize, int64_t nt_off, int32_t alen, const uint8_t *aa)
{
	int32_t sc = 0;
	for (int32_t i = 0, j = 0; i < alen; i += 3, ++j)
		sc += (int8_t)tab[ALN_TAB_MAT + (int32_t)aln_codon_aa(g, tab, nt_off + i) * asize + tab[ALN_TAB_AA20 + aa[j]]];
	return sc;
}

MPA_HD inline mpa_dp_task_t plans_task(int32_t qid, uint32_t vid, int64_t nt_off, int64_t nl, int32_t aa_off, int32_t al, int32_t flag, int32_t io)
{
	mpa_dp_task_t t;
	t.nt_off = nt_off, t.vid = (int32_t)vid, t.nl = (int32_t)nl, t.qid = qid, t.aa_off = aa_off, t.al = al, t.flag = flag, t.io = io, t.tag = 0;
	return t;
}

// mark_reliable_anchors(a, max_aa_dist, min_cnt, kmer2, trim) into flag[cnt]: 1 for an anchor the host would mark with bit 31
template<class C> MPA_HD inline void plans_mark_core(const uint64_t *a, int32_t cnt, int32_t max_aa_dist, int32_t min_cnt, int32_t kmer2, int32_t trim, int32_t *flag)
{
	MPA_COOP_FOR(C, s, cnt) flag[s] = 0;
	C::sync();
	MPA_COOP_FOR(C, s, cnt) {
		if (s > 0 && !plans_break(a[s - 1], a[s], max_aa_dist)) continue;      // not the first anchor of a maximal run
		int32_t i = (int32_t)s, j = i + 1;
		for (; j < cnt; ++j) if (plans_break(a[j - 1], a[j], max_aa_dist)) break;
		if (j - i < min_cnt) continue;
		int32_t k = j - 2, t = (int32_t)a[j - 1];
		while (k >= i && t - (int32_t)a[k] < trim) --k;
		t = (int32_t)a[i] + 1 - kmer2;
		while (i < k && (int32_t)a[i] + 1 - t < trim) ++i;
		for (; i <= k; ++i) flag[i] = 1;
	}
	C::sync();
}

// The whole step for one query.  reg / plan: room for n_win; task: room for 4 n_win + the query's anchors; seg: room for its anchors.
// Every lane returns the counts.
template<class C, class G> MPA_HD inline PlansCounts plans_core(const PlansParams &p, const PlansQuery &Q, const G &g, const uint8_t *tab, const PlansScratch &S,
                                                                RegionRec *reg, PlanRec *plan, mpa_dp_task_t *task, SegRec *seg)
{
	PlansCounts n_out{ 0, 0, 0, 0 };
	if (Q.n_win <= 0) return n_out;
	// ---- a. the region of every window from its chains (map.c:89-111)
	MPA_COOP_FOR(C, w, Q.n_win) {
		const int64_t nu = Q.nu[w];
		int64_t best = 0, skip = 0;
		const uint64_t *u = Q.u + Q.cu[w];
		for (int64_t i = 1; i < nu; ++i) if ((int32_t)(u[best] >> 32) < (int32_t)(u[i] >> 32)) best = i;   // the first chain with the highest score
		for (int64_t i = 0; i < best; ++i) skip += (uint32_t)u[i];
		S.prim[w] = (int32_t)best, S.aoff[w] = nu > 0 ? Q.ca[w] + skip : -1;
	}
	C::sync();
	int32_t n = 0;
	for (int32_t w = 0; w < Q.n_win; ++w) {
		const int64_t o = S.aoff[w];
		if (o < 0) continue;                                                    // a window without chains: no region
		const uint64_t ub = Q.u[Q.cu[w] + S.prim[w]];
		const int32_t cnt = (int32_t)(uint32_t)ub;
		uint64_t *a = Q.a + o;
		const uint64_t first = a[0], last = a[cnt - 1];
		const PlansWindow W = Q.win[w];
		RegionRec x;
		x.off = w, x.cnt = cnt, x.id = 0, x.parent = 0, x.n_sub = W.n_sub, x.subsc = W.subsc, x.split = W.split, x.vid = W.vid;
		x.chn_sc = (int32_t)(ub >> 32);
		x.qs = (int32_t)(uint32_t)first - (p.kmer2 - 1);
		x.qe = (int32_t)(uint32_t)last + 1;
		x.vs = W.as + (int64_t)(first >> 32) + 1 - 3 * p.kmer2;
		x.ve = W.as + (int64_t)(last >> 32) + 1;
		int32_t s = 0;
		for (int32_t i = 1 + C::lane(); i < cnt; i += C::width()) s += plans_ungapped_term(a[i - 1], a[i], p.kmer2);   // (differences: the same before and after re-basing)
		s = C::sum(s);
		x.chn_sc_ungap = p.kmer2 + s;
		C::sync();
		const int64_t d = W.as - x.vs;
		MPA_COOP_FOR(C, i, cnt) { const uint64_t v = a[i]; a[i] = (uint64_t)((int64_t)(v >> 32) + d) << 32 | (v << 32 >> 32); }
		if (C::lane() == 0) S.tmp[n] = x;
		++n;
	}
	C::sync();
	if (n == 0) return n_out;
	// ---- b. the second region pass
	const RegionsScratch RS{ S.tmp, S.key, S.stack, S.hist, S.prim, S.cov, S.ctl };
	regions_sort_core<C>(S.tmp, n, RS, reg);
	if (C::lane() == 0) {
		regions_assign_parents(p.mask_level, p.mask_len, reg, n, S.prim, S.cov);
		const int32_t k = regions_select_secondary(p.pri_ratio, p.kmer * 2, p.best_n, reg, n, S.prim);
		// ---- c. how far the alignment windows may reach
		if (!p.no_align) plans_extension_limits(reg, k, g, 100, p.max_intron / 2, S.key, S.stack, S.hist, S.ext);
		S.ctl[0] = k;
	}
	C::sync();
	const int32_t k = S.ctl[0];
	n_out.n_reg = k;
	if (!p.no_align) {
		const bool retry = p.io > p.io_end;
		for (int32_t ri = 0; ri < k; ++ri) {
			// ---- d. reliable anchors and the plan (align.c:239-301)
			const RegionRec r = reg[ri];
			const uint64_t *a = Q.a + S.aoff[r.off];
			plans_mark_core<C>(a, r.cnt, 6, 3, p.kmer2, p.kmer2 + 1, S.flag);
			int32_t nm = 0;
			for (int32_t base = 0; base < r.cnt; base += C::width()) {          // the marked anchors, in order
				const int32_t i = base + C::lane();
				const bool m = i < r.cnt && S.flag[i] != 0;
				const uint64_t b = C::ballot(m);
				if (m) S.list[nm + C::rank(b)] = i;
				nm += C::popc(b);
			}
			C::sync();
			if (nm == 0) {                                                      // no reliable anchor: the region stays, without a plan
				if (C::lane() == 0) reg[ri].cnt = 0;
				continue;
			}
			const int32_t extl0 = (int32_t)(S.ext[ri] >> 32), extr0 = (int32_t)S.ext[ri];
			int32_t extl = p.max_ext, extr = p.max_ext;
			if (r.qs >= 10) extl = p.max_intron / 2;
			if (Q.qlen - r.qe >= 10) extr = p.max_intron / 2;
			if (extl0 > 0) extl = extl < extl0 ? extl : extl0;
			if (extr0 > 0) extr = extr < extr0 ? extr : extr0;
			const int64_t ctg_len = g.len((int32_t)(r.vid >> 1));
			const uint64_t a0 = a[S.list[0]], a1 = a[S.list[nm - 1]];
			PlanRec pl;
			pl.reg = ri;
			pl.as = r.vs > extl ? r.vs - extl : 0;
			pl.ae = r.ve + extr < ctg_len ? r.ve + extr : ctg_len;
			pl.vs0 = r.vs;
			pl.vs1 = pl.vs0 + (int64_t)(a0 >> 32) + 1;
			pl.as1 = (int32_t)((uint32_t)a0 << 1 >> 1) + 1;
			pl.mid_ve = (int32_t)(a1 >> 32) + 1 + pl.vs0, pl.mid_qe = (int32_t)((uint32_t)a1 << 1 >> 1) + 1;
			pl.has_right = pl.mid_qe < Q.qlen && pl.mid_ve < pl.ae;
			// ---- e. the extension calls of round 1 (align.c:290-296, 324-331)
			mpa_dp_task_t *t = task + n_out.n_task;
			int32_t nt = 0;
			pl.t_left2 = pl.t_right = pl.t_right2 = -1;
			pl.t_left = n_out.n_task + nt;
			const mpa_dp_task_t tl = plans_task(Q.qid, r.vid, pl.as, pl.vs1 - pl.as, 0, pl.as1, MPA_F_EXT_LEFT | MPA_F_SS_SKIP0, p.io);
			if (C::lane() == 0) t[nt] = tl;
			++nt;
			if (retry) {
				const int64_t as_alt = pl.vs1 - pl.as > p.max_ext ? pl.vs1 - p.max_ext : pl.as;
				pl.t_left2 = n_out.n_task + nt;
				const mpa_dp_task_t x = plans_task(Q.qid, r.vid, as_alt, pl.vs1 - as_alt, 0, pl.as1, MPA_F_EXT_LEFT | (as_alt == pl.as ? MPA_F_SS_SKIP0 : 0), p.io_end);
				if (C::lane() == 0) t[nt] = x;
				++nt;
			}
			if (pl.has_right) {
				pl.t_right = n_out.n_task + nt;
				const mpa_dp_task_t x = plans_task(Q.qid, r.vid, pl.mid_ve, pl.ae - pl.mid_ve, pl.mid_qe, Q.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, p.io);
				if (C::lane() == 0) t[nt] = x;
				++nt;
				if (retry) {
					const int64_t l_ext = pl.ae - pl.mid_ve < p.max_ext ? pl.ae - pl.mid_ve : p.max_ext;
					pl.t_right2 = n_out.n_task + nt;
					const mpa_dp_task_t y = plans_task(Q.qid, r.vid, pl.mid_ve, l_ext, pl.mid_qe, Q.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, p.io_end);
					if (C::lane() == 0) t[nt] = y;
					++nt;
				}
			}
			n_out.n_task += nt;
			// ---- f. the gaps between consecutive kept anchors (align.c:305-313): gap j lies between marked anchors j - 1 and j
			pl.gap0 = n_out.n_seg, pl.n_gap = nm - 1;
			if (C::lane() == 0) plan[n_out.n_plan] = pl;
			++n_out.n_plan;
			const int64_t vs0 = r.vs;
			const int32_t gap0 = n_out.n_seg;
			const auto gs = g.strand(r.vid);
			for (int32_t base = 1; base < nm; base += C::width()) {
				const int32_t j = base + C::lane();
				const bool valid = j < nm;
				SegRec s;
				s.ne0 = s.ne1 = s.ae0 = s.ae1 = 0, s.task = -1, s.score = 0;
				bool dp = false;
				if (valid) {
					const uint64_t x0 = a[S.list[j - 1]], x1 = a[S.list[j]];
					s.ne0 = (int32_t)(x0 >> 32) + 1, s.ae0 = (int32_t)((uint32_t)x0 << 1 >> 1) + 1;
					s.ne1 = (int32_t)(x1 >> 32) + 1, s.ae1 = (int32_t)((uint32_t)x1 << 1 >> 1) + 1;
					const int32_t nlen = s.ne1 - s.ne0, alen = s.ae1 - s.ae0;
					dp = !(nlen == alen * 3 && alen <= p.kmer2);
				}
				const uint64_t b = C::ballot(dp);
				if (valid) {
					if (dp) {
						s.task = n_out.n_task + C::rank(b);
						task[s.task] = plans_task(Q.qid, r.vid, vs0 + s.ne0, s.ne1 - s.ne0, s.ae0, s.ae1 - s.ae0, MPA_F_CIGAR, p.io);
					} else s.score = plans_ungapped_score(gs, tab, p.asize, vs0 + s.ne0, s.ae1 - s.ae0, Q.seq + s.ae0);
					seg[gap0 + j - 1] = s;
				}
				n_out.n_task += C::popc(b);
			}
			n_out.n_seg += nm - 1;
			C::sync();
		}
	}
	C::sync();
	MPA_COOP_FOR(C, i, k) reg[i].off = 0;                                       // (the host's regions own their anchors: off is 0 after the refinement)
	C::sync();
	return n_out;
}

} // namespace mpa
