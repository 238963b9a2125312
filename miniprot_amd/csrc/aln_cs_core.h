// aln_cs_core.h -- the cs:Z: difference string of a finished alignment (mp_write_cs, format.c:102-187) as ONE source for the host and
// the device, in the manner of aln_stats_core.h: the same job record, the same table block, the same CIGAR pool and protein text,
// plus a destination.  What is stored is the body, i.e. what follows "cs:Z:".
//
// Execution model.  The code is written for a TEAM (policy C: StatsSerial = one host thread, StatsWave = a wavefront) and a genome
// reader G (G::base(x) = the base at strand-local position x, 4 outside the contig).  Every lane walks the CIGAR with identical
// scalar state -- nl, al, the write position wp, the match run carried through an M operation -- and the words are read width() at
// a time and broadcast.  An M operation is shared out width() codons per step: every lane translates its codon, a ballot gives the
// mismatch mask, a mismatching lane derives the match run in front of it from the mask (or from the run carried in from the steps
// before when no lower bit is set), sizes its piece ((run ? 1 + digits(run) : 0) + 5 bytes), an exclusive scan places it, and the
// run that is still open behind the operation's last step is written by lane 0.  So a run of n matches is one ":n" however many
// steps it spans, and the string does not depend on width().  I, D, F and G are strided copies; an intron is lane 0's work.
//
// Nothing here has a capacity: any number of CIGAR words, any run length.  The destination is a slot of aln_cs_bound() bytes.
#pragma once
#include <stdint.h>
#include "aln_stats_core.h"

namespace mpa {

struct AlnCsOut { int32_t len, bad; };                    // bytes written; bad: the walk did not end at (ve - vs, qe - qs)

// An upper bound on the body's length from the CIGAR alone.  Per operation of length len:
//   M   5 len   the codons of the run split into mismatches (5 bytes each: '*', three bases, the residue) and maximal match runs; a
//               run of r >= 1 codons is ':' and the digits of r, 1 + digits(r) <= 1 + r <= 5 r bytes.  Exact when every codon mismatches
//   I   1 + len         '+' and one residue per inserted residue
//   D   1 + 3 len       '-' and three bases per deleted codon
//   F   1 + len         '-' and len bases
//   G   2 + len         '*', len bases and the residue
//   N / U / V   22      "*xxA" (at most: the split codon's head and the residue), '~', two donor bases, the decimal length (a
//               CIGAR length has 28 bits: 9 digits, 10 bytes with a sign), two acceptor bases, "-xx" (at most): 4 + 3 + 10 + 2 + 3
// Any other operation writes nothing.
#define ALN_CS_INTRON_BYTES 22
MPA_HD inline int64_t aln_cs_bound(const uint32_t *cig, int32_t n_cigar)
{
	int64_t b = 0;
	for (int32_t k = 0; k < n_cigar; ++k) {
		const uint32_t op = cig[k] & 0xf;
		const int64_t len = (int64_t)(cig[k] >> 4);
		if (op == 0) b += 5 * len;
		else if (op == 1 || op == 10) b += 1 + len;
		else if (op == 2) b += 1 + 3 * len;
		else if (op == 11) b += 2 + len;
		else if (op == 3 || op == 12 || op == 13) b += ALN_CS_INTRON_BYTES;
	}
	return b;
}

MPA_HD inline char aln_cs_lc(uint32_t b) { return b == 0 ? 'a' : b == 1 ? 'c' : b == 2 ? 'g' : b == 3 ? 't' : 'n'; }   // (a code of 4 or more prints n)
MPA_HD inline char aln_cs_upper(uint8_t c) { return (char)(c >= 'a' && c <= 'z' ? c - 32 : c); }                      // toupper in the C locale
MPA_HD inline int32_t aln_cs_digits(uint32_t v) { int32_t n = 1; while (v >= 10) v /= 10, ++n; return n; }
// v in decimal at d (a '-' first when negative); returns the bytes written
MPA_HD inline int32_t aln_cs_put_int(char *d, int32_t v)
{
	int32_t neg = v < 0;
	const uint32_t x = neg ? 0u - (uint32_t)v : (uint32_t)v;
	const int32_t nd = aln_cs_digits(x);
	if (neg) d[0] = '-';
	uint32_t y = x;
	for (int32_t i = nd - 1; i >= 0; --i) d[neg + i] = (char)('0' + y % 10), y /= 10;
	return neg + nd;
}
MPA_HD inline int32_t aln_cs_top_bit(uint64_t m) { return 63 - (int32_t)__builtin_clzll(m); }   // (m != 0)

// Every lane returns the same record.  dst: the alignment's slot, at least aln_cs_bound() bytes.
template<class C, class G>
MPA_HD inline AlnCsOut aln_cs_core(const AlnStatsJob &J, const uint8_t *tab, const uint8_t *text, const uint32_t *cig_pool, const G &g, char *dst)
{
	const uint32_t *cig = cig_pool + J.cig_off;
	const uint8_t *aa = text + J.q_off;                          // (whole query: residue i of the alignment is aa[qs + i])
	const int64_t vs = J.vs;
	int32_t nl = 0, al = 0;                                      // the same on every lane
	int64_t wp = 0;
	auto residue = [&](int32_t aa_idx) -> uint8_t { const int32_t qi = J.qs + aa_idx; return qi >= 0 && qi < J.qlen ? aa[qi] : (uint8_t)'X'; };
	auto base_char = [&](int64_t x) { return aln_cs_lc(g.base(vs + x)); };
	for (int32_t base = 0; base < J.n_cigar; base += C::width()) {   // the words, width() at a time: one per lane
		const uint32_t mine = base + C::lane() < J.n_cigar ? cig[base + C::lane()] : 0u;
		const int32_t n_here = J.n_cigar - base < C::width() ? J.n_cigar - base : C::width();
		for (int32_t k = 0; k < n_here; ++k) {
			const uint32_t c = C::bcast(mine, k);
			const int32_t op = (int32_t)(c & 0xf), len = (int32_t)(c >> 4);
			if (op == 0) {                                             // M: ":n" for maximal match runs, "*xxxA" for a mismatch
				int32_t carry = 0;                                     // matches since the last mismatch of this operation (never of the one before)
				for (int32_t l0 = 0; l0 < len; l0 += C::width()) {
					const int32_t l = l0 + C::lane(), n_step = len - l0 < C::width() ? len - l0 : C::width();
					const int64_t x = nl + 3 * (int64_t)l;
					uint8_t r = 0;
					bool mism = false;
					if (l < len) r = residue(al + l), mism = aln_codon_aa(g, tab, vs + x) != tab[ALN_TAB_AA20 + r];
					const uint64_t mask = C::ballot(mism);
					int32_t run = 0, bytes = 0;
					if (mism) {
						const uint64_t lower = mask & (((uint64_t)1 << C::lane()) - 1);
						run = lower ? C::lane() - aln_cs_top_bit(lower) - 1 : carry + C::lane();
						bytes = (run ? 1 + aln_cs_digits((uint32_t)run) : 0) + 5;
					}
					int32_t total;
					const int32_t off = C::scan32(bytes, &total);
					if (mism) {
						char *d = dst + wp + off;
						if (run) *d++ = ':', d += aln_cs_put_int(d, run);
						d[0] = '*', d[1] = base_char(x), d[2] = base_char(x + 1), d[3] = base_char(x + 2), d[4] = aln_cs_upper(r);
					}
					wp += total;
					carry = mask ? n_step - 1 - aln_cs_top_bit(mask) : carry + n_step;
				}
				if (carry > 0) {                                       // the run still open behind the last step
					if (C::lane() == 0) dst[wp] = ':', aln_cs_put_int(dst + wp + 1, carry);
					wp += 1 + aln_cs_digits((uint32_t)carry);
				}
				nl += len * 3, al += len;
			} else if (op == 1) {                                      // I: '+' and the residues
				if (C::lane() == 0) dst[wp] = '+';
				for (int32_t l = C::lane(); l < len; l += C::width()) dst[wp + 1 + l] = aln_cs_upper(residue(al + l));
				wp += 1 + len, al += len;
			} else if (op == 2 || op == 10) {                          // D / F: '-' and the bases
				const int32_t n = op == 2 ? len * 3 : len;
				if (C::lane() == 0) dst[wp] = '-';
				for (int32_t i = C::lane(); i < n; i += C::width()) dst[wp + 1 + i] = base_char(nl + i);
				wp += 1 + n, nl += n;
			} else if (op == 11) {                                     // G: '*', the bases, the residue
				if (C::lane() == 0) dst[wp] = '*', dst[wp + 1 + len] = aln_cs_upper(residue(al));
				for (int32_t i = C::lane(); i < len; i += C::width()) dst[wp + 1 + i] = base_char(nl + i);
				wp += 2 + len, nl += len, ++al;
			} else if (op == 3 || op == 12 || op == 13) {              // N / U / V introns: lane 0's work; the length's digits are known to all
				const int32_t lshift = op == 3 ? 0 : op == 12 ? 1 : 2, rshift = lshift == 0 ? 0 : 3 - lshift;
				const int32_t ilen = len - (lshift + rshift);
				const int32_t n_int = (ilen < 0) + aln_cs_digits(ilen < 0 ? 0u - (uint32_t)ilen : (uint32_t)ilen);
				if (C::lane() == 0) {
					char *d = dst + wp;
					if (lshift > 0) {
						*d++ = '*';
						for (int32_t i = 0; i < lshift; ++i) *d++ = base_char(nl + i);
						*d++ = aln_cs_upper(residue(al));
					}
					*d++ = '~', *d++ = base_char(nl + lshift), *d++ = base_char(nl + lshift + 1);
					d += aln_cs_put_int(d, ilen);
					*d++ = base_char((int64_t)nl + len - rshift - 2), *d++ = base_char((int64_t)nl + len - rshift - 1);
					if (rshift > 0) {
						*d++ = '-';
						for (int32_t i = 0; i < rshift; ++i) *d++ = base_char((int64_t)nl + len - rshift + i);
					}
				}
				wp += (lshift > 0 ? 2 + lshift : 0) + 3 + n_int + 2 + (rshift > 0 ? 1 + rshift : 0);
				if (lshift) ++al;
				nl += len;
			}
		}
	}
	AlnCsOut o;
	o.len = (int32_t)wp;
	o.bad = !(nl == J.ve - J.vs && al == J.qe - J.qs);
	return o;
}

} // namespace mpa
