// spans_core.h -- the two host steps in the middle of the DP stage as ONE source for the host and the device,
// like plans_core.h, whose records and pieces it is built from:
//   spans_accept     between DP round 1 and round 2 (take_round1_emit_round2 of host_align.cpp; align.c:290-300, 324-331): which of an
//                    extension's two calls counts, where the region starts, the two accepted spans as segments -- the ungapped shortcut
//                    or a round-2 DP task
//   spans_assemble   behind DP round 2 (assemble_alignment + count_exons; align.c:302-338): the region's CIGAR joined from its
//                    segments' words with the merge rule of ns_push_cigar (nasw.h:141-152), its score, end and exon count
//
// Execution model.  spans_accept is one lane's work: a handful of integers and at most kmer2 codons per plan; the numbering of the
// round-2 tasks over the batch's plans (query-major, left before right) is the caller's scan (span_kernels.hip; a running count on the
// host).  spans_assemble is written for a TEAM (policy C: SpansSerial = one host thread, SpansWave = the 64 lanes of a wavefront):
//   parallel   what a segment is -- its result record, its number of words, the ops of its first and last word --, segment s to lane
//              s mod width(); whether its first word merges (the last op of the nearest non-empty segment before it: a team scan of
//              (segment number, op) by maximum); where its words go (a team prefix sum of words minus merged first words); the score (a
//              team sum; integer addition is exact in any order); the copy of a segment's words, word j to lane j mod width(); the
//              count of intron words
//   serial     the segments of a group of width() follow each other in one loop that every lane runs alike (their descriptors are
//              broadcast); a merged first word adds its length to the word before it on lane 0, between two team syncs, so a run of
//              single-word segments collapses into one word in segment order
// A merge can only happen at a segment's FIRST word: the words of a DP call come from ns_push_cigar, which has merged what it could.
// Merging never changes an op, so "the op of the last output word" is the op of the last input word: the decision needs no output.
// A segment that breaks the rule (two mergeable neighbours inside it) is reported in AsmRec::bad and the caller keeps the host step.
//
// Nothing here has a capacity: any number of segments, any number of words.
#pragma once
#include <stdint.h>
#include "plans_core.h"

namespace mpa {

struct SpansParams { int32_t kmer2, max_ext, io, asize; };

// a plan of the batch as the two steps read it
struct SpansPlan {
	PlanRec pl;                          // gap0: its first gap segment in the BATCH's segment array
	int64_t q_off;                       // the query's first residue in the batch text
	int32_t qid, qlen;
	uint32_t vid;                        // of the plan's region
	int32_t base1;                       // the query's first record in the round-1 results (gap tasks and t_left .. t_right2 count from it)
};
#define SPANS_LEFT 1                     /* SpanRec::flags: the left span was made (always) */
#define SPANS_RIGHT 2                    /* the right span was made: has_right && r_nt > 0 && r_aa > 0 */
#define SPANS_LREP 4                     /* the left terminal-exon repeat counted */
#define SPANS_RREP 8                     /* the right one */
struct SpanRec {                         // what spans_accept leaves of a plan; 80 bytes
	int64_t vs;                          // the region's start after the left extension
	int32_t qs, l_nt, l_aa, r_nt, r_aa, flags;
	SegRec left, right;                  // task: -1 for the shortcut, else its number among the round-2 tasks
};
struct AsmRec {                          // what spans_assemble leaves of a plan; 40 bytes
	int64_t ve, cig_off;                 // cig_off: the caller's (where the slot starts in its pool)
	int32_t qe, dp_score, n_cigar, n_exon, bad, n_merged;   // n_merged: first words that went into the word before them
};

struct SpansSerial : StatsSerial {};     // a team of one: the host

// make_segment (host_plan.cpp; align.c:62-80): the shortcut's score, or the call that aligns the span.  Returns true for a DP task
template<class S> MPA_HD inline bool spans_segment(const SpansParams &p, const SpansPlan &P, const S &g, const uint8_t *tab, const uint8_t *text, int32_t ne0, int32_t ne1, int32_t ae0,
                                                   int32_t ae1, SegRec &s, mpa_dp_task_t &t)
{
	s.ne0 = ne0, s.ne1 = ne1, s.ae0 = ae0, s.ae1 = ae1, s.task = -1, s.score = 0;
	const int32_t nlen = ne1 - ne0, alen = ae1 - ae0;
	if (nlen == alen * 3 && alen <= p.kmer2) {
		s.score = plans_ungapped_score(g, tab, p.asize, P.pl.vs0 + ne0, alen, text + P.q_off + ae0);
		return false;
	}
	s.task = 0;
	t = plans_task(P.qid, P.vid, P.pl.vs0 + ne0, nlen, ae0, alen, MPA_F_CIGAR, p.io);
	return true;
}

// Residues an extension call consumed, as the accept rules read them.  A call that consumed no row of its window extended nothing,
// whatever its aa_len says: mpa_dp_run() answers an extension call of fewer than three rows with (0, al + 1, INT32_MIN) (include/mpamd.h;
// the reference fails an assertion there), and al + 1 residues must neither move a region's start or end nor pass for "reached the end
// of the protein".  Every swept call that finds no best row returns (0, 0) already.
MPA_HD inline int32_t spans_ext_aa(const mpa_dp_rst_t &r) { return r.nt_len > 0 ? r.aa_len : 0; }

// One plan between the rounds.  rst1: the round-1 results of the batch; g: the strand of P.vid; text: the batch's protein text.
// Returns the number of round-2 tasks (0 .. 2) written to t[]; R.left.task / R.right.task number them from 0 (the caller adds the
// tasks of the plans before this one)
template<class S> MPA_HD inline int32_t spans_accept(const SpansParams &p, const SpansPlan &P, const mpa_dp_rst_t *rst1, const S &g, const uint8_t *tab, const uint8_t *text,
                                                     SpanRec &R, mpa_dp_task_t *t)
{
	const PlanRec &pl = P.pl;
	const mpa_dp_rst_t *mine = rst1 + P.base1;
	// (an extension that consumed no row is no extension: spans_ext_aa() makes the (0, al + 1, INT32_MIN) of a window of fewer than
	// three rows the (0, 0) every swept call that finds no best row returns)
	int32_t l_nt = mine[pl.t_left].nt_len, l_aa = spans_ext_aa(mine[pl.t_left]), r_nt = 0, r_aa = 0, flags = SPANS_LEFT;
	// the terminal-exon repeat counts iff the reference would have made it AND it reaches the end of the protein (align.c:290-296)
	if (pl.t_left2 >= 0 && l_aa != pl.as1 && l_nt < p.max_ext && spans_ext_aa(mine[pl.t_left2]) == pl.as1)
		l_nt = mine[pl.t_left2].nt_len, l_aa = mine[pl.t_left2].aa_len, flags |= SPANS_LREP;
	if (pl.has_right) {
		r_nt = mine[pl.t_right].nt_len, r_aa = spans_ext_aa(mine[pl.t_right]);
		if (pl.t_right2 >= 0 && r_aa < P.qlen - pl.mid_qe && r_nt < p.max_ext && spans_ext_aa(mine[pl.t_right2]) == P.qlen - pl.mid_qe)
			r_nt = mine[pl.t_right2].nt_len, r_aa = mine[pl.t_right2].aa_len, flags |= SPANS_RREP;
	}
	R.l_nt = l_nt, R.l_aa = l_aa, R.r_nt = r_nt, R.r_aa = r_aa;
	R.vs = pl.vs1 - l_nt, R.qs = pl.as1 - l_aa, R.flags = flags;
	int32_t n = 0;
	if (spans_segment(p, P, g, tab, text, (int32_t)(R.vs - pl.vs0), (int32_t)(pl.vs1 - pl.vs0), R.qs, pl.as1, R.left, t[n])) R.left.task = n++;
	R.right = SegRec{ 0, 0, 0, 0, -1, 0 };
	if (pl.has_right && r_nt > 0 && r_aa > 0) {                                 // the accepted right-extension span (align.c:331)
		const int32_t ne0 = (int32_t)(pl.mid_ve - pl.vs0);
		R.flags |= SPANS_RIGHT;
		if (spans_segment(p, P, g, tab, text, ne0, ne0 + r_nt, pl.mid_qe, pl.mid_qe + r_aa, R.right, t[n])) R.right.task = n++;
	}
	return n;
}

// the segments of a plan in order: left span, gaps, right span
MPA_HD inline int32_t spans_n_seg(const SpansPlan &P, const SpanRec &R) { return 1 + P.pl.n_gap + ((R.flags & SPANS_RIGHT) ? 1 : 0); }
// how many words segment s brings (the slot of a plan is the sum over its segments: merges only shorten it)
MPA_HD inline int32_t spans_seg_words(const SpansPlan &P, const SpanRec &R, const SegRec *gap, const mpa_dp_rst_t *rst1, const mpa_dp_rst_t *rst2, int32_t s)
{
	if (s >= 1 && s <= P.pl.n_gap) { const SegRec &x = gap[P.pl.gap0 + s - 1]; return x.task < 0 ? 1 : rst1[P.base1 + x.task].n_cigar; }
	const SegRec &x = s == 0 ? R.left : R.right;
	return x.task < 0 ? 1 : rst2[x.task].n_cigar;
}

// One plan behind round 2.  gap: the batch's gap segments; rst1 / pool1: the round-1 results and their CIGAR pool; rst2 / pool2: those
// of round 2 (both null where round 2 had no tasks: every span took the shortcut); out: the plan's slot.  Every lane returns the
// same record; cig_off is left 0
template<class C> MPA_HD inline AsmRec spans_assemble(const SpansPlan &P, const SpanRec &R, const SegRec *gap, const mpa_dp_rst_t *rst1, const uint32_t *pool1,
                                                      const mpa_dp_rst_t *rst2, const uint32_t *pool2, uint32_t *out)
{
	const int32_t n_seg = spans_n_seg(P, R);
	int32_t out_n = 0, carry_op = -1, score = 0, n_intron = 0, n_merged = 0;                  // the same on every lane (n_intron: this lane's)
	bool bad = false;
	for (int32_t base = 0; base < n_seg; base += C::width()) {
		// ---- what this lane's segment is
		const int32_t s = base + C::lane();
		int32_t n = 0, sc = 0, sel = 0;                                         // sel: 0 = one word of its own, 1 / 2 = words of pool 1 / 2
		int64_t off = 0;
		uint32_t single = 0, first = 0, last = 0;
		if (s < n_seg) {
			const bool is_gap = s >= 1 && s <= P.pl.n_gap;
			const SegRec x = is_gap ? gap[P.pl.gap0 + s - 1] : s == 0 ? R.left : R.right;
			if (x.task < 0) n = 1, sc = x.score, single = (uint32_t)(x.ae1 - x.ae0) << 4, first = last = single & 0xf;
			else {
				const mpa_dp_rst_t o = is_gap ? rst1[P.base1 + x.task] : rst2[x.task];
				const uint32_t *w = (is_gap ? pool1 : pool2) + o.cigar_off;
				n = o.n_cigar, sc = o.score, sel = is_gap ? 1 : 2, off = o.cigar_off;
				if (n > 0) first = w[0] & 0xf, last = w[n - 1] & 0xf;
			}
		}
		// ---- does its first word merge: the last op of the nearest non-empty segment before it
		int64_t top;
		const int64_t below = C::scan_max_excl(n > 0 ? (int64_t)s << 8 | last : -1, &top);
		const int32_t prev_op = below >= 0 ? (int32_t)(below & 0xff) : carry_op;
		if (top >= 0) carry_op = (int32_t)(top & 0xff);
		const int32_t merge = n > 0 && prev_op == (int32_t)first && first != 10 && first != 11 ? 1 : 0;
		// ---- where its words go
		int64_t total;
		const int32_t pos = out_n + (int32_t)C::scan_excl(n - merge, &total);
		out_n += (int32_t)total, n_merged += C::sum(merge);
		score += C::sum(sc);
		// ---- the copy, segment after segment
		const int32_t n_here = n_seg - base < C::width() ? n_seg - base : C::width();
		for (int32_t k = 0; k < n_here; ++k) {
			const int32_t bn = (int32_t)C::bcast((uint32_t)n, k), bmerge = (int32_t)C::bcast((uint32_t)merge, k), bpos = (int32_t)C::bcast((uint32_t)pos, k);
			const int32_t bsel = (int32_t)C::bcast((uint32_t)sel, k);
			const int64_t boff = (int64_t)((uint64_t)C::bcast((uint32_t)((uint64_t)off >> 32), k) << 32 | C::bcast((uint32_t)off, k));
			const uint32_t bsingle = C::bcast(single, k);
			const uint32_t *w = bsel == 1 ? pool1 + boff : bsel == 2 ? pool2 + boff : nullptr;
			for (int32_t j = C::lane(); j < bn; j += C::width()) {
				const uint32_t c = w ? w[j] : bsingle, op = c & 0xf;
				if (j > 0 && (w[j - 1] & 0xf) == op && op != 10 && op != 11) bad = true;   // (a word that would merge inside a segment)
				if (j >= bmerge) out[bpos + j - bmerge] = c, n_intron += op == 3 || op == 12 || op == 13;
			}
			if (bmerge) {                                                       // its first word's length goes to the word before it
				C::sync();
				if (C::lane() == 0) out[bpos - 1] += (w ? w[0] : bsingle) & ~(uint32_t)0xf;
				C::sync();
			}
		}
	}
	C::sync();
	AsmRec A;
	A.ve = P.pl.mid_ve, A.qe = P.pl.mid_qe, A.cig_off = 0;
	if (R.flags & SPANS_RIGHT) A.ve += R.r_nt, A.qe += R.r_aa;
	A.dp_score = score, A.n_cigar = out_n, A.n_exon = 1 + C::sum(n_intron), A.bad = C::sum(bad ? 1 : 0) != 0, A.n_merged = n_merged;
	return A;
}

} // namespace mpa
