// aln_stats_core.h -- the statistics pass over a finished alignment (row a16 of DESIGN.md section 1): mp_extra_stop and
// mp_extra_start (align.c:214-237) and mp_extra_cal (align.c:82-201) as ONE source for the host and the device, like chain_core.h
// and gs32_core.h.
//
// Execution model.  The code is written for a TEAM (policy C: StatsSerial = one host thread, StatsWave = the 64 lanes of a
// wavefront, stats_kernels.hip) and a genome reader G (G::base(x) = the base at strand-local position x of the alignment's strand,
// 4 outside the contig).  Every lane walks the CIGAR with identical scalar state -- nl, al, blen, n_fs, the gap and frameshift
// penalties -- and the codons of an M or D run are shared out, codon l to lane l mod width().  What a codon contributes (stop,
// identity, positive, score) goes into four per-lane partial sums; they are added up over the team only where a value is consumed:
// at an intron, which closes a feature, and at the end.  Integer addition makes any order exact.  The codon split by a U / V intron,
// the donor and acceptor bases and the feature records are lane 0's work.  The two distance scans test width() codons per step.
//
// Nothing here has a capacity: any number of CIGAR words, any run length, any feature count.
#pragma once
#include <stdint.h>
#include "chain_core.h"

namespace mpa {

// one alignment.  Positions are strand-local on vid; [as, ae) is the window mp_align() worked in (ae <= the contig's length)
struct AlnStatsJob {
	int64_t vs, ve, as, ae;
	int64_t q_off;                       // the query's first residue in the batch text
	int64_t cig_off;                     // its assembled CIGAR words
	int64_t feat_off;                    // its feature slots: one per exon and one for a stop-codon feature
	int32_t vid, qs, qe, qlen, n_cigar, pad;
};
struct AlnStatsParams { int32_t go, ge, fs, asize; };
// codon table (tab_codon) | aa20 | substitution matrix: the shared tables as one block (LDS on the device)
#define ALN_TAB_CODON 0
#define ALN_TAB_AA20 64
#define ALN_TAB_MAT 320
#define ALN_TAB_BYTES (320 + 484)
struct AlnStatsOut { int32_t dist_stop, dist_start, dp_max, blen, n_iden, n_plus, n_fs, n_stop, bad, n_feat; };   // bad: the walk did not end at (ve - vs, qe - qs)
struct AlnFeat {                         // Feat (host_core.h), field by field
	int64_t vs, ve;
	int32_t qs, qe;
	int16_t type, phase;
	int32_t n_fs, n_stop, score, n_iden, blen;
	char donor[2], acceptor[2];
};

struct StatsSerial : CoopSerial {        // a team of one: the host
	static MPA_HD int32_t sum(int32_t v) { return v; }                    // over the team, the same on every lane
	static MPA_HD uint32_t bcast(uint32_t v, int) { return v; }           // lane k's value (k the same on every lane)
	static MPA_HD int32_t scan32(int32_t v, int32_t *total) { *total = v; return 0; }   // sum of v over the lanes below this one; the team's total (aln_cs_core.h)
};

// codon at strand-local position j -> aa20 code, 21 for a codon with an ambiguous base (ns_tab_codon through the nt4 codes)
template<class G> MPA_HD inline uint32_t aln_codon_aa(const G &g, const uint8_t *tab, int64_t j)
{
	const uint32_t b0 = g.base(j), b1 = g.base(j + 1), b2 = g.base(j + 2);
	return b0 > 3 || b1 > 3 || b2 > 3 ? 21u : tab[ALN_TAB_CODON + (b0 << 4 | b1 << 2 | b2)];
}
MPA_HD inline char aln_nt_char(uint32_t b) { return b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : b == 3 ? 'T' : 'N'; }

// mp_extra_stop (align.c:214-224): in-frame distance from ve to the first stop codon inside the window, -1 for none
template<class C, class G> MPA_HD inline int32_t aln_dist_stop(const G &g, const uint8_t *tab, int64_t ve, int64_t ae)
{
	for (int64_t base = ve; base + 2 < ae; base += 3 * C::width()) {
		const int64_t j = base + 3 * C::lane();
		const uint64_t m = C::ballot(j + 2 < ae && aln_codon_aa(g, tab, j) == 20);
		if (m) return (int32_t)(base + 3 * C::lowest(m) - ve);
	}
	return -1;
}

// mp_extra_start (align.c:226-237): backwards from vs, in frame: -1 at a stop codon or the window's start, the distance at an M
// codon -- whichever comes first, i.e. is nearer to vs
template<class C, class G> MPA_HD inline int32_t aln_dist_start(const G &g, const uint8_t *tab, int64_t vs, int64_t as, int64_t ae)
{
	if (vs + 2 >= ae) return -1;
	for (int64_t base = vs; base >= as; base -= 3 * C::width()) {
		const int64_t j = base - 3 * C::lane();
		const uint32_t aa = j >= as ? aln_codon_aa(g, tab, j) : 21u;
		const uint64_t m_stop = C::ballot(aa == 20), m_met = C::ballot(aa == 12);
		if (m_stop | m_met) {
			const int k = C::lowest(m_stop | m_met);
			return m_stop >> k & 1 ? -1 : (int32_t)(3 * k + (vs - base));
		}
	}
	return -1;
}

// mp_extra_cal (align.c:82-201) behind the two scans.  text: the batch's protein text; cig: the CIGAR pool; feat: the feature pool.
// Every lane returns the same record; lane 0 writes the features.
template<class C, class G>
MPA_HD inline AlnStatsOut aln_stats_core(const AlnStatsJob &J, const AlnStatsParams p, const uint8_t *tab, const uint8_t *text, const uint32_t *cig_pool, const G &g,
                                         AlnFeat *feat_pool)
{
	AlnStatsOut o;
	o.dist_stop = aln_dist_stop<C>(g, tab, J.ve, J.ae);
	o.dist_start = aln_dist_start<C>(g, tab, J.vs, J.as, J.ae);
	const uint32_t *cig = cig_pool + J.cig_off;
	const uint8_t *aa = text + J.q_off;                          // (whole query: residue i of the alignment is aa[qs + i])
	AlnFeat *feat = feat_pool + J.feat_off;
	const bool has_stop = J.qe == J.qlen && o.dist_stop == 0;
	const int64_t vs = J.vs;
	int32_t s_stop = 0, s_iden = 0, s_plus = 0, s_score = 0;     // this lane's partial sums
	int32_t nl = 0, al = 0, blen = 0, n_fs = 0, pen = 0, ft = 0; // the same on every lane
	int32_t blen0 = 0, iden0 = 0, score0 = 0, fs0 = 0, stop0 = 0, phase0 = 0, qs0 = J.qs;
	int64_t vs0 = vs;
	char acc0[2] = { 0, 0 };
	auto score_codon = [&](uint32_t nt_aa, int32_t aa_idx) {
		const int32_t qi = J.qs + aa_idx;
		const uint32_t q = tab[ALN_TAB_AA20 + (qi >= 0 && qi < J.qlen ? aa[qi] : (uint8_t)'X')];
		const int32_t s = (int8_t)tab[ALN_TAB_MAT + nt_aa * p.asize + q];
		s_stop += nt_aa == 20, s_iden += nt_aa == q, s_plus += s > 0, s_score += s;
	};
	// a feature closes: the three sums it quotes, over the team
	auto close_exon = [&](int64_t ve, AlnFeat &f) {
		const int32_t t_stop = C::sum(s_stop), t_iden = C::sum(s_iden), t_score = C::sum(s_score) - pen;
		f.type = 0, f.vs = vs0, f.ve = ve, f.qs = qs0, f.qe = J.qs + al, f.phase = (int16_t)phase0;
		f.blen = blen - blen0, f.n_iden = t_iden - iden0, f.n_fs = n_fs - fs0, f.n_stop = t_stop - stop0, f.score = t_score - score0;
		f.donor[0] = f.donor[1] = 0;
		f.acceptor[0] = ft > 0 ? acc0[0] : 0, f.acceptor[1] = ft > 0 ? acc0[1] : 0;
		fs0 = n_fs, stop0 = t_stop, score0 = t_score, blen0 = blen, iden0 = t_iden;
	};
	for (int32_t base = 0; base < J.n_cigar; base += C::width()) {   // the words, width() at a time: one per lane
		const uint32_t mine = base + C::lane() < J.n_cigar ? cig[base + C::lane()] : 0u;
		const int32_t n_here = J.n_cigar - base < C::width() ? J.n_cigar - base : C::width();
		for (int32_t k = 0; k < n_here; ++k) {
			const uint32_t c = C::bcast(mine, k);
			const int32_t op = (int32_t)(c & 0xf), len = (int32_t)(c >> 4);
			if (op == 0) {                                             // M
				for (int32_t l = C::lane(); l < len; l += C::width()) score_codon(aln_codon_aa(g, tab, vs + nl + 3 * (int64_t)l), al + l);
				nl += len * 3, al += len, blen += len * 3;
			} else if (op == 1) {                                      // I
				pen += p.go + p.ge * len;
				al += len, blen += len * 3;
			} else if (op == 2) {                                      // D: in-frame stop codons inside deletions count
				for (int32_t l = C::lane(); l < len; l += C::width()) s_stop += aln_codon_aa(g, tab, vs + nl + 3 * (int64_t)l) == 20;
				pen += p.go + p.ge * len;
				nl += len * 3, blen += len * 3;
			} else if (op == 10) {                                     // F
				pen += p.fs;
				nl += len, blen += len, n_fs++;
			} else if (op == 11) {                                     // G
				pen += p.fs;
				nl += len, ++al, blen += 3, n_fs++;
			} else if (op == 3 || op == 12 || op == 13) {              // N / U / V introns
				if (op != 3) {                                         // the codon split by a phase-1/2 intron
					if (C::lane() == 0) {
						const int64_t x = vs + nl;
						const uint32_t b0 = g.base(x), b1 = g.base(op == 12 ? x + len - 2 : x + 1), b2 = g.base(x + len - 1);
						score_codon(b0 > 3 || b1 > 3 || b2 > 3 ? 21u : tab[ALN_TAB_CODON + (b0 << 4 | b1 << 2 | b2)], al);
					}
					blen += 3;
				}
				AlnFeat f;
				const int64_t ve = op == 3 ? vs + nl : op == 12 ? vs + nl + 1 : vs + nl + 2;
				close_exon(ve, f);
				if (op == 3) vs0 = vs + nl + len, phase0 = 0;
				else if (op == 12) vs0 = vs + nl + len - 2, phase0 = 2;
				else vs0 = vs + nl + len - 1, phase0 = 1;
				qs0 = f.qe;
				if (C::lane() == 0) {
					f.donor[0] = ve < J.ae ? aln_nt_char(g.base(ve)) : '.';
					f.donor[1] = ve + 1 < J.ae ? aln_nt_char(g.base(ve + 1)) : '.';
					feat[ft] = f;
					acc0[0] = vs0 - vs >= 2 ? aln_nt_char(g.base(vs0 - 2)) : '.';
					acc0[1] = vs0 - vs >= 1 ? aln_nt_char(g.base(vs0 - 1)) : '.';
				}
				++ft;
				nl += len, al += op != 3;
			}
		}
	}
	AlnFeat f;
	close_exon(vs + nl, f);
	if (C::lane() == 0) feat[ft] = f;
	++ft;
	if (has_stop) {
		if (C::lane() == 0) {
			AlnFeat s;
			s.type = 1, s.vs = J.ve, s.ve = J.ve + 3, s.qs = s.qe = J.qe + al, s.phase = 0, s.n_fs = 0, s.n_stop = 0, s.score = 0, s.n_iden = 0, s.blen = 3;
			s.donor[0] = s.donor[1] = s.acceptor[0] = s.acceptor[1] = 0;
			feat[ft] = s;
		}
		++ft;
	}
	o.dp_max = score0, o.blen = blen, o.n_iden = iden0, o.n_plus = C::sum(s_plus), o.n_fs = n_fs, o.n_stop = stop0;   // (the last close_exon left the totals)
	o.bad = !(nl == J.ve - J.vs && al == J.qe - J.qs);
	o.n_feat = ft;
	return o;
}

} // namespace mpa
