// aln_rows_core.h -- the residue rows of --aln / --trans for a finished alignment (put_residues of host_format.cpp; format.c:189-331)
// as ONE source for the host and the device, in the manner of aln_cs_core.h: the same job record, the same table block, the same
// CIGAR pool and protein text, plus a small parameter struct and a destination.  What is stored is the four rows of equal width
// (##ATN, ##ATA, ##AAS, ##AQA) and the translated target (##STA), each without its prefix and newline.
//
// Execution model.  The code is written for a TEAM (policy C: StatsSerial = one host thread, StatsWave = a wavefront) and a genome
// reader G (G::base(x) = the base at strand-local position x, 4 outside the contig; G::len = the strand's length).  Every lane walks
// the CIGAR with identical scalar state -- nl, al, the column cp, the STA position sp, the last STA byte -- and the words are read
// width() at a time and broadcast.  The columns of an operation are shared out one lane per COLUMN: lane i of a step reads the base
// of column i, the lane of a codon's first column also reads the other two, translates, and stores the STA byte; every lane stores
// its four bytes.  So a store instruction of a step covers width() consecutive bytes of one row.  Where an operation starts follows
// from the CIGAR and the flank alone (aln_rows_cols / aln_rows_codons), so nothing is scanned, nothing has a capacity, and the
// output does not depend on width().
//
// The slot.  stride = aln_rows_cols() + 3 (the trailing codon's columns); with the rows on, row r of the four is at dst + r * stride
// and the STA bytes follow at dst + 4 * stride (aln_rows_codons() + 1 of them with --trans); with --trans alone the slot is the STA
// bytes.  aln_rows_slot() is the size.
#pragma once
#include <stdint.h>
#include "aln_cs_core.h"

namespace mpa {

struct AlnRowsParams { int32_t asize, flank, show_aln, show_trans; };   // opt.asize, opt.max_intron_flank, MPA_MF_SHOW_RESIDUE, MPA_MF_SHOW_TRANS
struct AlnRowsOut { int32_t width, n_sta, bad, pad; };    // columns written (0 without the rows), STA bytes counted; bad: the walk did not end at (ve - vs, qe - qs)

// the columns an intron of `intron` bases takes: whole when it is at most twice the flank, else flank + '~' + its length + '~' + flank
MPA_HD inline int64_t aln_rows_intron_cols(int32_t intron, int32_t flank)
{
	if ((int64_t)intron <= 2 * (int64_t)flank) return intron > 0 ? intron : 0;
	return 2 * (int64_t)(flank > 0 ? flank : 0) + 2 + (intron < 0) + aln_cs_digits(intron < 0 ? 0u - (uint32_t)intron : (uint32_t)intron);
}
// columns of one CIGAR word
MPA_HD inline int64_t aln_rows_op_cols(uint32_t c, int32_t flank)
{
	const uint32_t op = c & 0xf;
	const int32_t len = (int32_t)(c >> 4);
	if (op == 0 || op == 1 || op == 2) return 3 * (int64_t)len;
	if (op == 10 || op == 11) return len;
	if (op == 3) return aln_rows_intron_cols(len, flank);
	if (op == 12 || op == 13) return 3 + aln_rows_intron_cols(len - 3, flank);
	return 0;
}
// the exact width of the four rows, and the exact length of the STA row, both without the trailing codon
MPA_HD inline int64_t aln_rows_cols(const uint32_t *cig, int32_t n_cigar, int32_t flank)
{
	int64_t n = 0;
	for (int32_t k = 0; k < n_cigar; ++k) n += aln_rows_op_cols(cig[k], flank);
	return n;
}
MPA_HD inline int64_t aln_rows_codons(const uint32_t *cig, int32_t n_cigar)
{
	int64_t n = 0;
	for (int32_t k = 0; k < n_cigar; ++k) {
		const uint32_t op = cig[k] & 0xf;
		n += op == 0 || op == 2 ? (int64_t)(cig[k] >> 4) : op == 12 || op == 13 ? 1 : 0;
	}
	return n;
}
MPA_HD inline int64_t aln_rows_slot(const uint32_t *cig, int32_t n_cigar, const AlnRowsParams &p)
{
	return (p.show_aln ? 4 * (aln_rows_cols(cig, n_cigar, p.flank) + 3) : 0) + (p.show_trans ? aln_rows_codons(cig, n_cigar) + 1 : 0);
}

MPA_HD inline char aln_rows_i2c(uint32_t t) { return "ARNDCQEGHILKMFPSTWYV*X"[t < 21 ? t : 21]; }

// Every lane returns the same record.  dst: the alignment's slot, aln_rows_slot() bytes.
template<class C, class G>
MPA_HD inline AlnRowsOut aln_rows_core(const AlnStatsJob &J, const AlnRowsParams p, const uint8_t *tab, const uint8_t *text, const uint32_t *cig_pool, const G &g, char *dst)
{
	const uint32_t *cig = cig_pool + J.cig_off;
	const uint8_t *aa = text + J.q_off;                          // (whole query: residue i of the alignment is aa[qs + i])
	const int64_t vs = J.vs;
	const bool rows = p.show_aln != 0, trans = p.show_trans != 0;
	int64_t stride = 0;
	if (rows) {                                                  // the width from the CIGAR: a word per lane, summed over the team
		int32_t part = 0;
		for (int32_t k = C::lane(); k < J.n_cigar; k += C::width()) part += (int32_t)aln_rows_op_cols(cig[k], p.flank);
		stride = (int64_t)C::sum(part) + 3;
	}
	char *const atn = dst, *const ata = dst + stride, *const aas = dst + 2 * stride, *const aqa = dst + 3 * stride, *const sta = dst + 4 * stride;
	int32_t nl = 0, al = 0;                                      // the same on every lane
	int64_t cp = 0, sp = 0;
	char last = '\t';                                            // the last STA byte; none yet: the tab of "##STA\t"
	auto residue = [&](int32_t aa_idx) -> uint8_t { const int32_t qi = J.qs + aa_idx; return qi >= 0 && qi < J.qlen ? aa[qi] : (uint8_t)'X'; };
	auto uc = [&](int64_t x) { return aln_nt_char(g.base(vs + x)); };
	auto lc = [&](int64_t x) { return aln_cs_lc(g.base(vs + x)); };
	auto match_char = [&](uint32_t t, uint8_t r) {
		const uint32_t q = tab[ALN_TAB_AA20 + r];
		return t == q ? '|' : (int8_t)tab[ALN_TAB_MAT + t * p.asize + q] > 0 ? '+' : ' ';
	};
	auto col = [&](int64_t c, char a, char b, char m, char q) { if (rows) atn[c] = a, ata[c] = b, aas[c] = m, aqa[c] = q; };
	for (int32_t base = 0; base < J.n_cigar; base += C::width()) {   // the words, width() at a time: one per lane
		const uint32_t mine = base + C::lane() < J.n_cigar ? cig[base + C::lane()] : 0u;
		const int32_t n_here = J.n_cigar - base < C::width() ? J.n_cigar - base : C::width();
		for (int32_t k = 0; k < n_here; ++k) {
			const uint32_t c = C::bcast(mine, k);
			const int32_t op = (int32_t)(c & 0xf), len = (int32_t)(c >> 4);
			if (op == 0 || op == 2) {                                  // M / D: three columns and one STA byte per codon
				const int32_t n = 3 * len;
				for (int32_t i = C::lane(); i < n; i += C::width()) {
					const int32_t l = i / 3;
					const int64_t x = (int64_t)nl + i;
					char b = '.', m = ' ', q = ' ';
					if (i == 3 * l) {                                      // the codon's first column
						const uint32_t t = aln_codon_aa(g, tab, vs + x);
						b = aln_rows_i2c(t);
						if (op == 0) { const uint8_t r = residue(al + l); m = match_char(t, r), q = aln_cs_upper(r); }
						else q = '-';
						if (trans) sta[sp + l] = b;
					}
					col(cp + i, uc(x), b, m, q);
				}
				if (len > 0) last = aln_rows_i2c(aln_codon_aa(g, tab, vs + nl + 3 * (int64_t)(len - 1)));   // (the same on every lane)
				cp += n, sp += len, nl += n;
				if (op == 0) al += len;
			} else if (op == 1) {                                      // I: three columns per residue, no target
				const int32_t n = 3 * len;
				for (int32_t i = C::lane(); i < n; i += C::width()) {
					const int32_t l = i / 3;
					if (i == 3 * l) col(cp + i, '-', '-', ' ', aln_cs_upper(residue(al + l)));
					else col(cp + i, '-', '.', ' ', ' ');
				}
				cp += n, al += len;
			} else if (op == 10) {                                     // F: one column per base
				for (int32_t i = C::lane(); i < len; i += C::width()) col(cp + i, uc((int64_t)nl + i), '!', ' ', ' ');
				cp += len, nl += len;
			} else if (op == 11) {                                     // G: one column per base, one residue
				for (int32_t i = C::lane(); i < len; i += C::width()) col(cp + i, uc((int64_t)nl + i), '$', ' ', i == 0 ? aln_cs_upper(residue(al)) : ' ');
				cp += len, nl += len, ++al;
			} else if (op == 3 || op == 12 || op == 13) {              // N / U / V introns
				const int32_t head = op == 3 ? 0 : op == 12 ? 1 : 2, tail = head ? 3 - head : 0;
				const int32_t intron = len - (head + tail);
				if (head) {                                            // the split codon: its bases on either side of the intron
					const int64_t x = vs + nl;
					const uint32_t b0 = g.base(x), b1 = g.base(op == 12 ? x + len - 2 : x + 1), b2 = g.base(x + len - 1);
					const uint32_t t = b0 > 3 || b1 > 3 || b2 > 3 ? 21u : tab[ALN_TAB_CODON + (b0 << 4 | b1 << 2 | b2)];
					const uint8_t r = residue(al);
					last = aln_rows_i2c(t);
					if (C::lane() == 0) {
						col(cp, aln_nt_char(b0), last, match_char(t, r), aln_cs_upper(r));
						if (head == 2) col(cp + 1, aln_nt_char(b1), '.', ' ', ' ');
						if (trans) sta[sp] = last;
					}
					cp += head, nl += head, ++sp, ++al;
				}
				const int64_t n_col = aln_rows_intron_cols(intron, p.flank);
				if (rows) {
					for (int64_t i = C::lane(); i < n_col; i += C::width()) ata[cp + i] = ' ', aas[cp + i] = ' ', aqa[cp + i] = ' ';
					if ((int64_t)intron <= 2 * (int64_t)p.flank) {
						for (int32_t i = C::lane(); i < intron; i += C::width()) atn[cp + i] = lc((int64_t)nl + i);
					} else {                                               // flank bases, '~', the length, '~', flank bases
						const int32_t f = p.flank > 0 ? p.flank : 0;
						const int64_t right = n_col - f;
						for (int32_t i = C::lane(); i < f; i += C::width()) atn[cp + i] = lc((int64_t)nl + i), atn[cp + right + i] = lc((int64_t)nl + intron - f + i);
						if (C::lane() == 0) atn[cp + f] = '~', aln_cs_put_int(atn + cp + f + 1, intron), atn[cp + right - 1] = '~';
					}
				}
				cp += n_col, nl += intron;
				if (C::lane() == 0)
					for (int32_t i = 0; i < tail; ++i) col(cp + i, uc((int64_t)nl + i), '.', ' ', ' ');
				cp += tail, nl += tail;
			}
		}
	}
	// one more codon -- the stop, if the alignment ends right before it -- when the contig has it and the last STA byte is no '*'
	if (J.ve + 3 <= g.len && last != '*') {
		if (C::lane() == 0) {
			const char b = aln_rows_i2c(aln_codon_aa(g, tab, vs + nl));
			col(cp, uc(nl), b, ' ', ' '), col(cp + 1, uc((int64_t)nl + 1), '.', ' ', ' '), col(cp + 2, uc((int64_t)nl + 2), '.', ' ', ' ');
			if (trans) sta[sp] = b;
		}
		cp += 3, ++sp;
	}
	AlnRowsOut o;
	o.width = rows ? (int32_t)cp : 0, o.n_sta = (int32_t)sp, o.pad = 0;
	o.bad = !(nl == J.ve - J.vs && al == J.qe - J.qs);
	return o;
}

} // namespace mpa
