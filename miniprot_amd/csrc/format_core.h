// format_core.h -- the output text of a batch from its flat result (MPA_GPU_FORMAT): mp_write_output
// (format.c:453-473) with mp_write_paf (format.c:333-358), mp_write_gff (format.c:360-412), mp_write_gtf (format.c:414-451), the carried
// form of the --aln / --trans rows, and the output filters and running hit id of worker_pipeline step 2 (map.c:298-311) -- what
// put_paf, put_gff, put_gtf, the carried branch of put_residues and format_batch of host_format.cpp do, restated as three stages.  ONE
// source for the host (MPA_GPU_FORMAT=model, the hook without a context) and the device (format_kernels.hip), like finish_core.h.
//
//   select and size   a TEAM per query (FormatSerial = one host thread, FormatWave = a wavefront): which hits passes() prints, the
//                     exact byte count of every printed hit's text, the number of running-id fields in it, and the query's sums
//   scan              the exclusive prefix of the queries' sums over the batch
//   write             a team per printed hit: its text at its offset
//
// Sizing and writing are the SAME code: every emitter below runs on a sink (FmtPut) that counts when it has no text to write into, so
// that a size can never disagree with what is written.  The uniform parts of a line are lane 0's; names, cs bodies and rows are
// lane-strided copies; the words of cg:Z: and the GFF3 / GTF feature lines take a lane each, placed by a scan of their lengths.
//
// Floating point: the filters stay in fp64 in the host's expression shapes and `(double)n * 3 / blen` is one IEEE division
// (-ffp-contract=off, no fast-math); its "%.4f" is made from the double's bits in integer arithmetic (fmt_ratio).
// The running id: the text carries ids relative to the batch (1 .. n_out in print order) as six digits, and id_at[] says where each
// such field lies; format_patch_ids() adds the batch's id0 on the host, where the batches are back in input order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "chain_core.h"
#include "finish_core.h"
#include "../../include/mpamd.h"

namespace mpa {

#define FORMAT_PREFIX_MAX 64             /* bytes of a gff_prefix the step takes; a longer one: declined */
#define FORMAT_ID_LIMIT 999999           /* the largest id "%.6ld" prints in six digits */
#define FORMAT_BAD_RATIO 1               /* a blen of 0: the host would print nan / inf */
#define FORMAT_BAD_CARRIED 2             /* the options print a cs string or rows that the hit does not carry */

struct FmtOpt { uint32_t flag; int32_t out_n; float out_sim, out_cov; int32_t gff_delim, prefix_len; char prefix[FORMAT_PREFIX_MAX]; };
// what the text is made of: the flat result (cs / rows: null when no hit carries one), the queries' lengths and names, the contigs'
// names and lengths.  Names lie back to back in a byte pool, name i = pool[off[i] .. off[i + 1])
struct FmtSrc {
	const mpa_hit_t *hits; const int64_t *hit_off; const uint32_t *cigars; const mpa_feat_t *feats;
	const FinCsRef *cs; const char *cs_text; const FinRowsRef *rows; const char *rows_text;
	const int64_t *q_off; const char *qname; const int64_t *qname_off;
	const char *cname; const int64_t *cname_off, *clen;
	// rec != nullptr: the hits are read where the finish step left them on the device (finish_core.h) instead of from hits / hit_off / cs /
	// rows -- query q's kept hits are out[first[q] ..] by rank, hit j is record rec[first[q] + out[first[q] + j].src], their number is the
	// difference of fin_off[].hit; cigars, feats, cs_text and rows_text are then what the records' offsets point into (the walks' slots)
	const FinRec *rec = nullptr; const FinOut *out = nullptr; const int64_t *first = nullptr; const FinCounts *fin_off = nullptr;
};
// a hit as the emitters read it.  rows: four rows of rows_w bytes rows_stride apart, rows_sta STA bytes behind 4 rows_stride
// (rows_stride < 0: none carried); cs_len < 0: no cs body carried
struct FmtHit { mpa_hit_t h; const uint32_t *cig; const mpa_feat_t *feat; const char *cs, *rows; int64_t rows_stride; int32_t cs_len, rows_w, rows_sta, pad; };
struct FmtAt { int64_t byte; int32_t id, rank; };                // a hit inside its query: first byte, first id field, number among the printed (< 0: not printed)
struct FmtCounts { int64_t bytes, ids, n_out, bad; };            // of a query; their exclusive prefix: where the query's text goes
static_assert(sizeof(FmtAt) == 16 && sizeof(FmtCounts) == 32 && sizeof(FmtHit) % 8 == 0, "record sizes");

struct FormatSerial : CoopSerial {       // a team of one: the host
	static MPA_HD int64_t sum64(int64_t v) { return v; }
};

MPA_HD inline int fmt_digits(uint64_t x) { int n = 1; while (x >= 10) x /= 10, ++n; return n; }

// The sink.  base == nullptr: count only.  `mine`: this lane writes the single bytes (lane 0 of a team-level sink; always for a lane's own
// line).  p: the next byte's offset in the text; n_id: the next id field's number; id: the hit's id relative to the batch
struct FmtPut {
	char *base; int64_t p; int64_t *id_at; int64_t n_id, id; int32_t bad; bool mine;
	MPA_HD void ch(char c) { if (base && mine) base[p] = c; ++p; }
	MPA_HD void lit(const char *s) { for (; *s; ++s) ch(*s); }
	MPA_HD void str(const char *s, int64_t n) { for (int64_t i = 0; i < n; ++i) ch(s[i]); }
	MPA_HD void num(int64_t v)
	{
		char buf[24];
		int n = 0;
		uint64_t x = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
		do buf[n++] = (char)('0' + x % 10), x /= 10; while (x);
		if (v < 0) buf[n++] = '-';
		while (n) ch(buf[--n]);
	}
	MPA_HD void id6()                                            // "%.6ld" of the relative id, and where it lies
	{
		if (base && mine) {
			id_at[n_id] = p;
			int64_t x = id % 1000000;
			for (int k = 5; k >= 0; --k) base[p + k] = (char)('0' + x % 10), x /= 10;
		}
		++n_id, p += 6;
	}
};

// "%.4f" of (double)n * 3 / blen as glibc prints it: x = m 2^e exactly, so x 10^4 = m 625 2^(e + 4) with m 625 < 2^63; the shift
// leaves the integer of the four-decimal figure and an exact remainder, rounded half to even
MPA_HD inline void fmt_ratio(FmtPut &w, int32_t n, int32_t blen)
{
	const double x = (double)n * 3 / blen;
	uint64_t b;
	__builtin_memcpy(&b, &x, 8);
	const int32_t ex = (int32_t)(b >> 52 & 0x7ff);
	uint64_t m = b & (((uint64_t)1 << 52) - 1);
	if (ex == 0x7ff) { w.bad |= FORMAT_BAD_RATIO; return; }    // nan / inf: a blen of 0
	if (b >> 63) w.ch('-');
	const int32_t sh = 1071 - (ex ? ex : 1);                   // x 10^4 = P / 2^sh; |x| < 2^34 keeps sh > 0
	if (ex) m |= (uint64_t)1 << 52;
	const uint64_t P = m * 625;
	uint64_t q = 0;
	if (sh <= 0) { w.bad |= FORMAT_BAD_RATIO; return; }
	if (sh < 64) {
		q = P >> sh;
		const uint64_t rem = P & (((uint64_t)1 << sh) - 1), half = (uint64_t)1 << (sh - 1);
		if (rem > half || (rem == half && (q & 1))) ++q;
	}
	char buf[24];
	int k = 0;
	do buf[k++] = (char)('0' + q % 10), q /= 10; while (q);
	while (k < 5) buf[k++] = '0';
	while (k > 4) w.ch(buf[--k]);
	w.ch('.');
	while (k) w.ch(buf[--k]);
}

// a lane-strided copy into a team-level sink
template<class C> MPA_HD inline void fmt_copy(FmtPut &w, const char *s, int64_t n)
{
	if (w.base) MPA_COOP_FOR(C, i, n) w.base[w.p + i] = s[i];
	w.p += n;
}

MPA_HD inline FmtHit fmt_hit_flat(const FmtSrc &S, int64_t hidx)    // hit hidx of the flat result
{
	FmtHit X;
	X.h = S.hits[hidx];
	X.cig = S.cigars + X.h.cigar_off, X.feat = S.feats + X.h.feat_off;
	X.cs = nullptr, X.cs_len = -1, X.rows = nullptr, X.rows_stride = -1, X.rows_w = X.rows_sta = 0, X.pad = 0;
	if (S.cs && S.cs[hidx].present) X.cs = S.cs_text + S.cs[hidx].off, X.cs_len = S.cs[hidx].len;
	if (S.rows && S.rows[hidx].present) X.rows = S.rows_text + S.rows[hidx].off, X.rows_w = S.rows[hidx].width, X.rows_sta = S.rows[hidx].n_sta, X.rows_stride = X.rows_w;
	return X;
}

MPA_HD inline FmtHit fmt_hit_fin(const FmtSrc &S, int32_t q, int64_t j)   // kept hit j of query q, where the finish step left it
{
	const int64_t f = S.first[q];
	const FinOut o = S.out[f + j];
	const FinRec &x = S.rec[f + o.src];
	FmtHit X;
	mpa_hit_t &h = X.h;
	h.qid = q, h.id = o.id, h.parent = o.parent, h.n_sub = o.n_sub, h.subsc = o.subsc, h.cnt = x.cnt, h.n_exon = x.n_exon, h.chn_sc = x.chn_sc, h.chn_sc_ungap = x.chn_sc_ungap;
	h.vid = x.vid, h.qs = x.qs, h.qe = x.qe, h.vs = x.vs, h.ve = x.ve, h.has_aln = 1, h.dp_score = x.dp_score, h.dp_max = x.dp_max, h.dp_max2 = o.dp_max2, h.blen = x.blen;
	h.n_fs = x.n_fs, h.n_stop = x.n_stop, h.dist_stop = x.dist_stop, h.dist_start = x.dist_start, h.n_iden = x.n_iden, h.n_plus = x.n_plus, h.n_cigar = x.n_cigar, h.n_feat = x.n_feat;
	h.cigar_off = x.cig_off, h.feat_off = x.feat_off;
	X.cig = S.cigars + x.cig_off, X.feat = S.feats + x.feat_off;
	X.cs = x.cs_len >= 0 ? S.cs_text + x.cs_off : nullptr, X.cs_len = x.cs_len;
	X.rows = x.rows_stride >= 0 ? S.rows_text + x.rows_off : nullptr, X.rows_stride = x.rows_stride, X.rows_w = x.rows_w, X.rows_sta = x.rows_sta, X.pad = 0;
	return X;
}
// the hits of query q: where its entries of at[] begin, how many there are, hit j
MPA_HD inline int64_t fmt_base(const FmtSrc &S, int32_t q) { return S.rec ? S.first[q] : S.hit_off[q]; }
MPA_HD inline int64_t fmt_n_reg(const FmtSrc &S, int32_t q) { return S.rec ? S.fin_off[q + 1].hit - S.fin_off[q].hit : S.hit_off[q + 1] - S.hit_off[q]; }
MPA_HD inline FmtHit fmt_hit(const FmtSrc &S, int32_t q, int64_t j) { return S.rec ? fmt_hit_fin(S, q, j) : fmt_hit_flat(S, S.hit_off[q] + j); }

// passes() of format_batch (map.c:298-306), in its expressions
MPA_HD inline bool fmt_passes(const FmtOpt &o, const mpa_hit_t &h, int32_t best_sc, int32_t qlen)
{
	const int32_t sc = h.has_aln ? h.dp_max : h.chn_sc;
	if (sc <= 0 || sc < (double)best_sc * o.out_sim) return false;
	if (h.qe - h.qs < (double)qlen * o.out_cov) return false;
	return true;
}

// put_paf.  X == nullptr: the -u line of a query without a printed hit
template<class C> MPA_HD inline void fmt_paf(FmtPut &w, const FmtOpt &o, const FmtSrc &S, int32_t q, const FmtHit *X)
{
	const int32_t qlen = (int32_t)(S.q_off[q + 1] - S.q_off[q]);
	if (o.flag & (MPA_MF_GFF | MPA_MF_GTF)) w.lit("##PAF\t");
	fmt_copy<C>(w, S.qname + S.qname_off[q], S.qname_off[q + 1] - S.qname_off[q]);
	w.ch('\t'), w.num(qlen);
	if (!X) { w.lit("\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n"); return; }
	const mpa_hit_t &h = X->h;
	const int64_t c = h.vid >> 1, clen = S.clen[c];
	w.ch('\t'), w.num(h.qs), w.ch('\t'), w.num(h.qe), w.ch('\t'), w.ch(h.vid & 1 ? '-' : '+'), w.ch('\t');
	fmt_copy<C>(w, S.cname + S.cname_off[c], S.cname_off[c + 1] - S.cname_off[c]);
	w.ch('\t'), w.num(clen), w.ch('\t');
	if (h.vid & 1) w.num(clen - h.ve), w.ch('\t'), w.num(clen - h.vs);
	else w.num(h.vs), w.ch('\t'), w.num(h.ve);
	w.ch('\t');
	if (h.has_aln) {
		w.num(h.n_iden * 3), w.ch('\t'), w.num(h.blen), w.lit("\t0\tAS:i:"), w.num(h.dp_score);
		w.lit("\tms:i:"), w.num(h.dp_max), w.lit("\tnp:i:"), w.num(h.n_plus), w.lit("\tfs:i:"), w.num(h.n_fs);
		w.lit("\tst:i:"), w.num(h.n_stop), w.lit("\tda:i:"), w.num(h.dist_start), w.lit("\tdo:i:"), w.num(h.dist_stop);
		w.lit("\tcg:Z:");
		if (!w.base) {                                           // sizing: the digit counts, reduced over the lanes
			int64_t s = 0;
			MPA_COOP_FOR(C, k, h.n_cigar) s += fmt_digits(X->cig[k] >> 4) + 1;
			w.p += C::sum64(s);
		} else {                                                 // writing: a word per lane, placed by a scan of the lengths
			const char *ops = "MIDNSHP=XBFGUVE";
			for (int32_t b = 0; b < h.n_cigar; b += C::width()) {
				const int32_t k = b + C::lane();
				const bool have = k < h.n_cigar;
				const uint32_t wd = have ? X->cig[k] : 0;
				const int len = have ? fmt_digits(wd >> 4) + 1 : 0;
				int64_t tot;
				const int64_t e = C::scan_excl(len, &tot);
				if (have) {
					char *d = w.base + w.p + e;
					uint32_t x = wd >> 4;
					for (int i = len - 2; i >= 0; --i) d[i] = (char)('0' + x % 10), x /= 10;
					d[len - 1] = ops[wd & 0xf];
				}
				w.p += tot;
			}
		}
		if (!(o.flag & MPA_MF_NO_CS)) {
			w.lit("\tcs:Z:");
			if (X->cs_len < 0) w.bad |= FORMAT_BAD_CARRIED;
			else fmt_copy<C>(w, X->cs, X->cs_len);
		}
	} else {
		w.num(h.chn_sc), w.ch('\t'), w.num(h.chn_sc_ungap), w.ch('\t'), w.num(h.cnt);
		if (!(o.flag & MPA_MF_NO_CS)) w.ch('\t');
	}
	w.ch('\n');
}

// the carried branch of put_residues
template<class C> MPA_HD inline void fmt_rows(FmtPut &w, const FmtOpt &o, const FmtHit &X)
{
	if (!X.h.has_aln) return;
	if (X.rows_stride < 0) { w.bad |= FORMAT_BAD_CARRIED; return; }
	if (o.flag & MPA_MF_SHOW_RESIDUE)
		for (int k = 0; k < 4; ++k) {
			w.lit(k == 0 ? "##ATN\t" : k == 1 ? "##ATA\t" : k == 2 ? "##AAS\t" : "##AQA\t");
			fmt_copy<C>(w, X.rows + k * X.rows_stride, X.rows_w), w.ch('\n');
		}
	if (o.flag & MPA_MF_SHOW_TRANS) w.lit("##STA\t"), fmt_copy<C>(w, X.rows + 4 * X.rows_stride, X.rows_sta), w.ch('\n');
}

MPA_HD inline void fmt_prefix_id(FmtPut &w, const FmtOpt &o, char mid)   // put_id: "%s<mid>%.6ld"
{
	w.str(o.prefix, o.prefix_len);
	if (mid) w.ch(mid);
	w.id6();
}

struct FmtGffCtx { const char *qname, *cname; int64_t qname_len, cname_len, clen; int32_t hit_idx, n_feat; bool rev, has_stop, delim; };

MPA_HD inline void fmt_gff_ids(FmtPut &w, const FmtOpt &o, const FmtGffCtx &g)
{
	if (g.delim) w.str(g.qname, g.qname_len), w.ch((char)o.gff_delim), w.num(g.hit_idx);
	else fmt_prefix_id(w, o, 0);
}

// feature line j of mp_write_gff, on one lane
MPA_HD inline void fmt_gff_feat(FmtPut &w, const FmtOpt &o, const FmtGffCtx &g, const mpa_feat_t *feat, int32_t j)
{
	const mpa_feat_t f = feat[j];
	int64_t fe = f.ve;
	if (g.has_stop && f.type == 0 && j + 1 < g.n_feat && feat[j + 1].type == 1) fe += 3;   // in GFF3 the last CDS includes the stop codon
	const int64_t vs = g.rev ? g.clen - fe : f.vs, ve = g.rev ? g.clen - f.vs : fe;
	w.str(g.cname, g.cname_len), w.lit("\tminiprot\t"), w.lit(f.type == 1 ? "stop_codon" : "CDS");
	w.ch('\t'), w.num(vs + 1), w.ch('\t'), w.num(ve), w.ch('\t'), w.num(f.score), w.ch('\t'), w.ch(g.rev ? '-' : '+');
	w.ch('\t'), w.num(f.phase), w.lit("\tParent="), fmt_gff_ids(w, o, g), w.lit(";Rank="), w.num(g.hit_idx);
	if (f.type == 0) {
		w.lit(";Identity="), fmt_ratio(w, f.n_iden, f.blen);
		if (f.acceptor[0] && !(f.acceptor[0] == 'A' && f.acceptor[1] == 'G')) w.lit(";Acceptor="), w.ch(f.acceptor[0]), w.ch(f.acceptor[1]);
		if (f.donor[0] && !(f.donor[0] == 'G' && f.donor[1] == 'T')) w.lit(";Donor="), w.ch(f.donor[0]), w.ch(f.donor[1]);
		if (f.n_fs > 0) w.lit(";Frameshift="), w.num(f.n_fs);
		if (f.n_stop > 0) w.lit(";StopCodon="), w.num(f.n_stop);
		w.lit(";Target="), w.str(g.qname, g.qname_len), w.ch(' '), w.num(f.qs + 1), w.ch(' '), w.num(f.qe);
	}
	w.ch('\n');
}

MPA_HD inline void fmt_gtf_head(FmtPut &w, const FmtGffCtx &g, const char *type, int64_t a, int64_t b, int32_t score)
{
	w.str(g.cname, g.cname_len), w.lit("\tminiprot\t"), w.lit(type), w.ch('\t'), w.num(a + 1), w.ch('\t'), w.num(b), w.ch('\t');
	w.num(score), w.ch('\t'), w.ch(g.rev ? '-' : '+'), w.ch('\t');
}
MPA_HD inline void fmt_gtf_tail(FmtPut &w, const FmtOpt &o)       // transcript_id "<tid>"; gene_id "<gid>";
{
	w.lit("\ttranscript_id \""), fmt_prefix_id(w, o, 'T'), w.lit("\"; gene_id \""), fmt_prefix_id(w, o, 'G'), w.lit("\";\n");
}

// the exon and CDS lines of feature j of mp_write_gtf, on one lane (nothing for a stop codon)
MPA_HD inline void fmt_gtf_feat(FmtPut &w, const FmtOpt &o, const FmtGffCtx &g, const mpa_hit_t &h, int64_t ve_mrna, const mpa_feat_t *feat, int32_t j)
{
	const mpa_feat_t f = feat[j];
	if (f.type != 0) return;
	const int64_t a = g.rev ? g.clen - f.ve : f.vs, b = g.rev ? g.clen - f.vs : f.ve;
	int64_t a2 = a, b2 = b;
	if (f.ve == h.ve) { if (g.rev) a2 = g.clen - ve_mrna; else b2 = ve_mrna; }   // the last exon also covers the stop codon
	fmt_gtf_head(w, g, "exon", a2, b2, f.score), w.ch('.'), fmt_gtf_tail(w, o);
	fmt_gtf_head(w, g, "CDS", a, b, f.score), w.num(f.phase), fmt_gtf_tail(w, o);
}

// put_gff (gtf == false) / put_gtf: the hit's lines through the team-level sink, the feature lines a lane each
template<class C> MPA_HD inline void fmt_annot(FmtPut &w, const FmtOpt &o, const FmtSrc &S, int32_t q, const FmtHit &X, int32_t hit_idx, bool gtf)
{
	const mpa_hit_t &h = X.h;
	if (!h.has_aln) return;
	const int32_t qlen = (int32_t)(S.q_off[q + 1] - S.q_off[q]);
	const int64_t c = h.vid >> 1;
	FmtGffCtx g;
	g.qname = S.qname + S.qname_off[q], g.qname_len = S.qname_off[q + 1] - S.qname_off[q];
	g.cname = S.cname + S.cname_off[c], g.cname_len = S.cname_off[c + 1] - S.cname_off[c], g.clen = S.clen[c];
	g.hit_idx = hit_idx, g.n_feat = h.n_feat, g.rev = h.vid & 1, g.has_stop = h.qe == qlen && h.dist_stop == 0;
	g.delim = !gtf && o.gff_delim >= 33 && o.gff_delim <= 126 && hit_idx >= 0;
	const int64_t ve_mrna = g.has_stop ? h.ve + 3 : h.ve;
	const int64_t vs = g.rev ? g.clen - ve_mrna : h.vs, ve = g.rev ? g.clen - h.vs : ve_mrna;
	if (gtf) {
		fmt_gtf_head(w, g, "gene", vs, ve, h.dp_max), w.lit(".\tgene_id \""), fmt_prefix_id(w, o, 'G'), w.lit("\";\n");
		fmt_gtf_head(w, g, "transcript", vs, ve, h.dp_max), w.ch('.'), fmt_gtf_tail(w, o);
	} else {
		fmt_copy<C>(w, g.cname, g.cname_len);
		w.lit("\tminiprot\tmRNA\t"), w.num(vs + 1), w.ch('\t'), w.num(ve), w.ch('\t'), w.num(h.dp_max);
		w.ch('\t'), w.ch(g.rev ? '-' : '+'), w.lit("\t.\tID="), fmt_gff_ids(w, o, g), w.lit(";Rank="), w.num(hit_idx);
		w.lit(";Identity="), fmt_ratio(w, h.n_iden, h.blen);
		w.lit(";Positive="), fmt_ratio(w, h.n_plus, h.blen);
		if (h.n_fs > 0) w.lit(";Frameshift="), w.num(h.n_fs);
		if (h.n_stop > 0) w.lit(";StopCodon="), w.num(h.n_stop);
		w.lit(";Target="), fmt_copy<C>(w, g.qname, g.qname_len), w.ch(' '), w.num(h.qs + 1), w.ch(' '), w.num(h.qe), w.ch('\n');
	}
	for (int32_t b = 0; b < h.n_feat; b += C::width()) {         // a lane per feature: its line's length, a scan places it, the lane writes it
		const int32_t j = b + C::lane();
		const bool have = j < h.n_feat;
		FmtPut cnt{ nullptr, 0, nullptr, 0, 0, 0, true };
		if (have) { if (gtf) fmt_gtf_feat(cnt, o, g, h, ve_mrna, X.feat, j); else fmt_gff_feat(cnt, o, g, X.feat, j); }
		int64_t tot, tot_id;
		const int64_t e = C::scan_excl(cnt.p, &tot), ei = C::scan_excl(cnt.n_id, &tot_id);
		if (C::any(cnt.bad != 0)) w.bad |= FORMAT_BAD_RATIO;
		if (w.base && have && !w.bad) {
			FmtPut l{ w.base, w.p + e, w.id_at, w.n_id + ei, w.id, 0, true };
			if (gtf) fmt_gtf_feat(l, o, g, h, ve_mrna, X.feat, j); else fmt_gff_feat(l, o, g, X.feat, j);
		}
		w.p += tot, w.n_id += tot_id;
	}
}

// everything a printed hit contributes, in format_batch's order; j = its number among the query's hits
template<class C> MPA_HD inline void format_hit_core(FmtPut &w, const FmtOpt &o, const FmtSrc &S, int32_t q, const FmtHit &X, int32_t j)
{
	const bool residues = (o.flag & (MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS)) != 0;
	if (o.flag & MPA_MF_GTF) {
		if (residues) fmt_paf<C>(w, o, S, q, &X), fmt_rows<C>(w, o, X);
		fmt_annot<C>(w, o, S, q, X, j + 1, true);
	} else {
		if (!(o.flag & MPA_MF_NO_PAF)) fmt_paf<C>(w, o, S, q, &X);
		if (residues) fmt_rows<C>(w, o, X);
		if (o.flag & MPA_MF_GFF) fmt_annot<C>(w, o, S, q, X, j + 1, false);
	}
}

// Select and size: query q.  at[]: an entry for every hit of the batch (the query's at fmt_base(S, q)); cnt: the query's sums
template<class C> MPA_HD inline void format_size_core(const FmtOpt &o, const FmtSrc &S, int32_t q, FmtAt *at, FmtCounts *cnt)
{
	const int64_t h0 = fmt_base(S, q), n_reg = fmt_n_reg(S, q);
	const int32_t qlen = (int32_t)(S.q_off[q + 1] - S.q_off[q]);
	int32_t best_sc = -1;
	if (n_reg > 0) { const FmtHit B = fmt_hit(S, q, 0); best_sc = B.h.has_aln ? B.h.dp_max : B.h.chn_sc; }
	FmtCounts c{ 0, 0, 0, 0 };
	for (int64_t j = 0; j < n_reg; ++j) {
		const FmtHit X = fmt_hit(S, q, j);
		if (!(j < o.out_n && fmt_passes(o, X.h, best_sc, qlen))) {
			if (C::lane() == 0) at[h0 + j] = FmtAt{ 0, 0, -1 };
			continue;
		}
		FmtPut w{ nullptr, 0, nullptr, 0, 0, 0, C::lane() == 0 };
		format_hit_core<C>(w, o, S, q, X, (int32_t)j);
		if (C::lane() == 0) at[h0 + j] = FmtAt{ c.bytes, (int32_t)c.ids, (int32_t)c.n_out };
		c.bytes += w.p, c.ids += w.n_id, ++c.n_out, c.bad += w.bad != 0;
	}
	if (c.n_out == 0 && (o.flag & MPA_MF_SHOW_UNMAP)) {
		FmtPut w{ nullptr, 0, nullptr, 0, 0, 0, C::lane() == 0 };
		fmt_paf<C>(w, o, S, q, nullptr);
		c.bytes += w.p;
	}
	if (C::lane() == 0) *cnt = c;
}

// the exclusive prefix of the queries' sums, off[n_query + 1], on one thread (the device scans: k_format_scan)
inline void format_scan_serial(const FmtCounts *cnt, int64_t n_query, FmtCounts *off)
{
	FmtCounts a{ 0, 0, 0, 0 };
	for (int64_t q = 0; q < n_query; ++q) {
		off[q] = a;
		a.bytes += cnt[q].bytes, a.ids += cnt[q].ids, a.n_out += cnt[q].n_out, a.bad += cnt[q].bad;
	}
	off[n_query] = a;
}

// Write: hit j of query q (printed: a.rank >= 0) at its place.  at = the prefix of its query
template<class C> MPA_HD inline void format_write_core(const FmtOpt &o, const FmtSrc &S, int32_t q, int64_t j, const FmtAt &a, const FmtCounts &at, char *text, int64_t *id_at)
{
	const FmtHit X = fmt_hit(S, q, j);
	FmtPut w{ text, at.bytes + a.byte, id_at, at.ids + a.id, at.n_out + a.rank + 1, 0, C::lane() == 0 };
	format_hit_core<C>(w, o, S, q, X, (int32_t)j);
}
// ... and the -u line of a query that prints no hit (the caller has looked at the flag and at the query's n_out)
template<class C> MPA_HD inline void format_unmap_core(const FmtOpt &o, const FmtSrc &S, int32_t q, const FmtCounts &at, char *text)
{
	FmtPut w{ text, at.bytes, nullptr, 0, 0, 0, C::lane() == 0 };
	fmt_paf<C>(w, o, S, q, nullptr);
}

// The batch's first printed hit gets id0 + 1: every six-digit field becomes field + id0, in place.  false: a field would need seven
// digits -- the widths the text was sized by no longer hold, and the caller formats the batch on the host
inline bool format_patch_ids(char *text, const int64_t *id_at, int64_t n_ids, int64_t n_out, int64_t id0)
{
	if (n_ids == 0) return true;
	if (id0 < 0 || id0 + n_out > FORMAT_ID_LIMIT) return false;
	if (id0 == 0) return true;
	for (int64_t k = 0; k < n_ids; ++k) {
		char *d = text + id_at[k];
		int64_t x = 0;
		for (int i = 0; i < 6; ++i) x = x * 10 + (d[i] - '0');
		x += id0;
		for (int i = 5; i >= 0; --i) d[i] = (char)('0' + x % 10), x /= 10;
	}
	return true;
}

} // namespace mpa
