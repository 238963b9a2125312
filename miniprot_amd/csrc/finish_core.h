// finish_core.h -- from the aligned regions of a batch to its flat result (MPA_GPU_FINISH): the tail of mp_map()
// behind mp_align() (map.c:229-236) for one query -- mp_sort_reg (hit.c:97-126), mp_select_multi_exon (hit.c:238-250), mp_set_parent
// with its ALIGNED branch (hit.c:128-187) and mp_select_sub with mp_sync_regs (hit.c:189-236) -- and the layout of what is left as
// mpa_batch_finish() lays it out (host_map.cpp): per-query counts, their prefix over the batch, the mpa_hit_t of every kept hit and the
// gathers of its CIGAR words, features, cs body and residue rows.  ONE source for the host (stage_finish / mpa_batch_finish_impl are its
// restatement on Region objects) and the device (finish_kernels.hip), like regions_core.h, whose note on floating point holds here too:
// `(float)ol / lo - (float)uncovered / hi > mask_level` and `sci >= scp * pri_ratio` in the host's expression shapes, -ffp-contract=off.
//
// Execution model.  A TEAM (FinishSerial = one host thread, FinishWave = a wavefront) per query for the ranking: the records are loaded,
// the cnt > 0 ones compacted into sort keys and moved into rank order across the team; the sort (the reference's unstable radix sort,
// whose tie order is the result), the multi-exon swap, the parents (region i depends on the primaries before it) and the selection
// (compacts in place) run on lane 0 over the team's scratch, which the device keeps in LDS up to FINISH_LDS_REGS regions (beyond, the serial part works in HBM scratch: rare, and slow there).  The gather
// is a team per kept hit.  Every region here is aligned: the branches of the reference that look at chains do not occur.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "chain_core.h"
#include "../../include/mpamd.h"

namespace mpa {

#define FINISH_LDS_REGS 64               /* regions of a query the device ranks in LDS (the sort is then its insertion sort: no digit tables); more: its scratch lies in HBM */

struct FinRec {                          // an aligned region as the step reads it (Region of host_core.h, flattened); 160 bytes
	int64_t vs, ve;
	int64_t cig_off, feat_off;           // its CIGAR words / features in the arrays that come with the records
	int64_t cs_off, rows_off;            // its cs body / rows slot in their texts
	uint32_t vid, hash;
	int32_t qs, qe, cnt, n_exon, chn_sc, chn_sc_ungap;
	int32_t parent, n_sub, subsc, dp_max2;                                                  // carried in (hit.c never resets subsc, n_sub only for primaries)
	int32_t dp_score, dp_max, blen, n_fs, n_stop, dist_stop, dist_start, n_iden, n_plus;
	int32_t n_cigar, n_feat;
	int32_t cs_len;                      // < 0: the region carries no cs body
	int32_t rows_w, rows_sta, rows_stride;   // the slot: four rows of rows_w bytes rows_stride apart, rows_sta STA bytes behind them; stride < 0: none carried
	int32_t job;                         // behind the walks on the device: the alignment's number there (finish_fill_core reads its records); else unused
};
struct FinParams { int32_t kmer, mask_len, best_n, io; float mask_level, pri_ratio; };      // kmer: the index's (sub_diff; min_diff = 2 kmer)
struct FinOut {                          // a kept hit, by rank: which record it is, what the ranking gave it, where its parts go inside the query
	int32_t src, id, parent, n_sub, subsc, dp_max2;
	int32_t pad[2];
	int64_t cig, feat, cs, rows;
};
struct FinCounts { int64_t hit, cigar, feat, cs, rows, n_cs, n_rows, pad; };                // of a query; their exclusive prefix: where the query's parts go
struct FinCsRef { int64_t off; int32_t len, present; };                                     // mpa_result_s::CsRef
struct FinRowsRef { int64_t off; int32_t width, n_sta, present, pad; };                     // mpa_result_s::RowsRef with its padding named
struct FinDst { mpa_hit_t *hits; uint32_t *cigars; mpa_feat_t *feats; FinCsRef *cs; char *cs_text; FinRowsRef *rows; char *rows_text; };

struct FinRank {                         // what the ranking reads and writes of a region; 88 bytes
	int64_t vs, ve;
	uint32_t vid;
	int32_t qs, qe, cnt, n_exon, chn_sc, dp_max, dp_max2, parent, n_sub, subsc, id, src;
	int32_t n_cigar, n_feat, cs_bytes, rows_bytes, pad;
};
struct FinScratch {                      // work space for a query of n regions
	FinRank *tmp, *r;                    // [n] before the sort; in rank order
	Pair64 *key;                         // [n]
	SortRange *stack;                    // [n / 64 + 8]
	uint32_t *hist;                      // [768]
	int32_t *prim;                       // [n] the primaries; mp_sync_regs' table
	uint64_t *cov;                       // [n]
	int32_t *ctl;                        // [2]
};
#define FINISH_STACK(n) ((n) / 64 + 8)

static_assert(sizeof(mpa_hit_t) == 136 && offsetof(mpa_hit_t, n_feat) == 112 && offsetof(mpa_hit_t, cigar_off) == 120, "finish_hit_words writes mpa_hit_t word by word");
static_assert(sizeof(mpa_feat_t) == 56 && sizeof(FinCsRef) == 16 && sizeof(FinRowsRef) == 24 && sizeof(FinRec) == 160 && sizeof(FinOut) == 64 && sizeof(FinRank) == 88, "record sizes");

struct FinishSerial : CoopSerial {       // a team of one: the host
	static MPA_HD int64_t sum64(int64_t v) { return v; }
};

// Behind the walks on the device the record's statistics, its cs length and its rows' width are not the host's: they lie in the walks'
// out records of alignment x.job, where this puts them into the record (cs / rows: null when that walk did not run in the call)
template<class StatsOut, class CsOut, class RowsOut> MPA_HD inline void finish_fill_core(FinRec &x, const StatsOut *st, const CsOut *cs, const RowsOut *rows, int32_t show_trans)
{
	const StatsOut o = st[x.job];
	x.dist_stop = o.dist_stop, x.dist_start = o.dist_start, x.dp_max = o.dp_max, x.blen = o.blen, x.n_iden = o.n_iden, x.n_plus = o.n_plus, x.n_fs = o.n_fs, x.n_stop = o.n_stop, x.n_feat = o.n_feat;
	x.cs_len = cs ? cs[x.job].len : -1;
	if (rows) x.rows_w = rows[x.job].width, x.rows_sta = show_trans ? rows[x.job].n_sta : 0;
	else x.rows_w = x.rows_sta = 0, x.rows_stride = -1;
}

MPA_HD inline int32_t finish_rows_bytes(const FinRec &x) { return x.rows_stride < 0 ? 0 : 4 * x.rows_w + x.rows_sta; }

// mp_select_multi_exon (hit.c:238-250)
MPA_HD inline void finish_multi_exon(FinRank *r, int32_t n, int32_t single_penalty)
{
	if (n < 2 || r[0].n_exon != 1) return;
	int32_t i = 1;
	while (i < n && r[i].n_exon < 2) ++i;
	if (i == n) return;
	if (r[0].dp_max < r[i].dp_max + single_penalty) { const FinRank t = r[0]; r[0] = r[i], r[i] = t; }
}

// mp_set_parent (hit.c:128-187) for aligned regions, hard_mask_level 0.  One lane: region i depends on the primaries found before it
MPA_HD inline void finish_assign_parents(float mask_level, int32_t mask_len, int32_t sub_diff, FinRank *r, int32_t n, int32_t *prim, uint64_t *cov)
{
	if (n <= 0) return;
	for (int32_t i = 0; i < n; ++i) r[i].id = i;
	int32_t n_prim = 0;
	prim[n_prim++] = 0;
	r[0].parent = 0;
	for (int32_t i = 1; i < n; ++i) {
		FinRank &ri = r[i];
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
			for (int32_t k = 1; k < n_cov; ++k) {           // (whole values are sorted: any correct sort gives radix_sort_mp64's order)
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
				FinRank &rp = r[prim[w]];
				const int32_t sj = rp.qs, ej = rp.qe;
				if (ej <= si || sj >= ei) continue;
				const int32_t lo = ej - sj < ei - si ? ej - sj : ei - si, hi = ej - sj > ei - si ? ej - sj : ei - si;
				const int32_t ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
				if ((float)ol / lo - (float)uncovered / hi > mask_level && uncovered <= mask_len) {   // secondary to rp
					int32_t counts = 0;
					ri.parent = rp.parent;
					rp.subsc = rp.subsc > ri.chn_sc ? rp.subsc : ri.chn_sc;
					if (ri.cnt >= rp.cnt) counts = 1;
					if (rp.vid != ri.vid || rp.vs != ri.vs || rp.ve != ri.ve || ol != lo) {           // not the identical hit after DP
						rp.dp_max2 = rp.dp_max2 > ri.dp_max ? rp.dp_max2 : ri.dp_max;
						if (rp.dp_max - ri.dp_max <= sub_diff) counts = 1;
					}
					if (counts) ++rp.n_sub;
					is_primary = false;
					break;
				}
			}
		}
		if (is_primary) prim[n_prim++] = i, ri.parent = i, ri.n_sub = 0;
	}
}

// mp_select_sub (hit.c:212-236) with mp_sync_regs (hit.c:189-210), in place as the reference: position p may already hold a moved
// element; parents precede their children and kept elements only move towards the front, which keeps r[p] the parent.  where: [n]
MPA_HD inline int32_t finish_select(float pri_ratio, int32_t min_diff, int32_t best_n, FinRank *r, int32_t n, int32_t *where)
{
	if (!(pri_ratio > 0.0f) || n <= 0) return n;
	int32_t n_2nd = 0, k = 0;
	for (int32_t i = 0; i < n; ++i) {
		const int32_t p = r[i].parent;
		const FinRank &rp = r[p];
		const FinRank &x = r[i];
		const int32_t sci = x.dp_max, scp = rp.dp_max;
		bool keep = false;
		if (p == i) keep = true;
		else if ((sci >= scp * pri_ratio || sci + min_diff >= scp) && n_2nd < best_n) {
			if (!(x.qs == rp.qs && x.qe == rp.qe && x.vid == rp.vid && x.vs == rp.vs && x.ve == rp.ve)) keep = true, ++n_2nd;
		}
		if (keep) { const FinRank v = r[i]; r[k++] = v; }
	}
	if (k == n) return n;
	for (int32_t i = 0; i < n; ++i) where[i] = -1;           // (ids before were the positions 0 .. n - 1)
	for (int32_t i = 0; i < k; ++i) if (r[i].id >= 0) where[r[i].id] = i;
	int32_t max_id = -1;
	for (int32_t i = 0; i < k; ++i) max_id = max_id > r[i].id ? max_id : r[i].id;
	for (int32_t i = 0; i < k; ++i) {
		FinRank &x = r[i];
		x.id = i;
		if (x.parent == -2) x.parent = i;
		else if (x.parent >= 0 && x.parent <= max_id && where[x.parent] >= 0) x.parent = where[x.parent];
		else x.parent = -1;
	}
	return k;
}

// The ranking of one query: rec[n] -> out[k] (room for n) in rank order and the query's counts.  Every lane returns k
template<class C> MPA_HD inline int32_t finish_rank_core(const FinParams &p, const FinRec *rec, int32_t n, const FinScratch &S, FinOut *out, FinCounts *cnt)
{
	if (n <= 0) {
		if (C::lane() == 0) *cnt = FinCounts{ 0, 0, 0, 0, 0, 0, 0, 0 };
		return 0;
	}
	MPA_COOP_FOR(C, i, n) {
		const FinRec &x = rec[i];
		FinRank y;
		y.vs = x.vs, y.ve = x.ve, y.vid = x.vid, y.qs = x.qs, y.qe = x.qe, y.cnt = x.cnt, y.n_exon = x.n_exon, y.chn_sc = x.chn_sc, y.dp_max = x.dp_max, y.dp_max2 = x.dp_max2;
		y.parent = x.parent, y.n_sub = x.n_sub, y.subsc = x.subsc, y.id = 0, y.src = (int32_t)i;
		y.n_cigar = x.n_cigar, y.n_feat = x.n_feat, y.cs_bytes = x.cs_len > 0 ? x.cs_len : 0, y.rows_bytes = finish_rows_bytes(x), y.pad = 0;
		S.tmp[i] = y;
	}
	C::sync();
	int32_t m = n;
	if (n <= 1) {                                            // (mp_sort_reg returns before it squeezes anything out)
		if (C::lane() == 0) S.r[0] = S.tmp[0];
	} else {
		m = (int32_t)coop_compact<C>(n, [&](int64_t i) { return S.tmp[i].cnt > 0; },
		                             [&](int64_t i, int64_t k) { S.key[k] = Pair64{ (uint64_t)S.tmp[i].dp_max << 32 | rec[i].hash, (uint64_t)i }; });
		C::sync();
		if (C::lane() == 0) sort_pairs_by_x_core(S.key, S.key + m, S.stack, S.hist);
		C::sync();
		MPA_COOP_FOR(C, j, m) S.r[j] = S.tmp[S.key[m - 1 - j].y];
	}
	C::sync();
	if (C::lane() == 0) {
		finish_multi_exon(S.r, m, p.io);
		finish_assign_parents(p.mask_level, p.mask_len, p.kmer, S.r, m, S.prim, S.cov);
		const int32_t k = finish_select(p.pri_ratio, p.kmer * 2, p.best_n, S.r, m, S.prim);
		FinCounts c{ k, 0, 0, 0, 0, 0, 0, 0 };
		for (int32_t j = 0; j < k; ++j) {                      // (the scratch, not the records: no walk through HBM here on the device)
			const FinRank &x = S.r[j];
			S.cov[j] = (uint64_t)c.cigar;                      // (cov is free by now: the hit's first word inside the query)
			c.cigar += x.n_cigar;
		}
		S.ctl[0] = k;
		*cnt = c;                                            // (the rest of the counts: below, across the team)
	}
	C::sync();
	const int32_t k = S.ctl[0];
	// where every kept hit's parts go inside the query: exclusive sums in rank order.  The team takes C::width() hits at a time
	int64_t feat0 = 0, cs0 = 0, rows0 = 0, n_cs = 0, n_rows = 0;
	for (int32_t base = 0; base < k; base += C::width()) {
		const int32_t j = base + C::lane();
		const bool have = j < k;
		const FinRank x = S.r[have ? j : 0];
		const FinRec &y = rec[x.src];
		int64_t tf, tc, tr;
		const int64_t ef = C::scan_excl(have ? x.n_feat : 0, &tf), ec = C::scan_excl(have ? x.cs_bytes : 0, &tc), er = C::scan_excl(have ? x.rows_bytes : 0, &tr);
		if (have) {
			FinOut o;
			o.src = x.src, o.id = x.id, o.parent = x.parent, o.n_sub = x.n_sub, o.subsc = x.subsc, o.dp_max2 = x.dp_max2, o.pad[0] = o.pad[1] = 0;
			o.cig = (int64_t)S.cov[j], o.feat = feat0 + ef, o.cs = cs0 + ec, o.rows = rows0 + er;
			out[j] = o;
			n_cs += y.cs_len >= 0, n_rows += y.rows_stride >= 0;
		}
		feat0 += tf, cs0 += tc, rows0 += tr;
	}
	n_cs = C::sum64(n_cs), n_rows = C::sum64(n_rows);
	C::sync();
	if (C::lane() == 0) cnt->feat = feat0, cnt->cs = cs0, cnt->rows = rows0, cnt->n_cs = n_cs, cnt->n_rows = n_rows;
	return k;
}

// the exclusive prefix of the queries' counts over the batch, off[n_query + 1], on one thread (the device scans: k_finish_scan)
inline void finish_scan_serial(const FinCounts *cnt, int64_t n_query, FinCounts *off)
{
	FinCounts a{ 0, 0, 0, 0, 0, 0, 0, 0 };
	for (int64_t q = 0; q < n_query; ++q) {
		off[q] = a;
		a.hit += cnt[q].hit, a.cigar += cnt[q].cigar, a.feat += cnt[q].feat, a.cs += cnt[q].cs, a.rows += cnt[q].rows, a.n_cs += cnt[q].n_cs, a.n_rows += cnt[q].n_rows;
	}
	off[n_query] = a;
}

// mpa_hit_t as 34 words, field for field as mpa_batch_finish_impl fills it; the padding word is zero
MPA_HD inline void finish_hit_words(int32_t qid, const FinRec &x, const FinOut &o, int64_t cigar_off, int64_t feat_off, uint32_t *w)
{
	w[0] = (uint32_t)qid, w[1] = (uint32_t)o.id, w[2] = (uint32_t)o.parent, w[3] = (uint32_t)o.n_sub, w[4] = (uint32_t)o.subsc, w[5] = (uint32_t)x.cnt;
	w[6] = (uint32_t)x.n_exon, w[7] = (uint32_t)x.chn_sc, w[8] = (uint32_t)x.chn_sc_ungap, w[9] = x.vid, w[10] = (uint32_t)x.qs, w[11] = (uint32_t)x.qe;
	w[12] = (uint32_t)(uint64_t)x.vs, w[13] = (uint32_t)((uint64_t)x.vs >> 32), w[14] = (uint32_t)(uint64_t)x.ve, w[15] = (uint32_t)((uint64_t)x.ve >> 32);
	w[16] = 1;                                               // has_aln
	w[17] = (uint32_t)x.dp_score, w[18] = (uint32_t)x.dp_max, w[19] = (uint32_t)o.dp_max2, w[20] = (uint32_t)x.blen, w[21] = (uint32_t)x.n_fs, w[22] = (uint32_t)x.n_stop;
	w[23] = (uint32_t)x.dist_stop, w[24] = (uint32_t)x.dist_start, w[25] = (uint32_t)x.n_iden, w[26] = (uint32_t)x.n_plus, w[27] = (uint32_t)x.n_cigar, w[28] = (uint32_t)x.n_feat;
	w[29] = 0;
	w[30] = (uint32_t)(uint64_t)cigar_off, w[31] = (uint32_t)((uint64_t)cigar_off >> 32), w[32] = (uint32_t)(uint64_t)feat_off, w[33] = (uint32_t)((uint64_t)feat_off >> 32);
}

// One kept hit into the flat arrays: o = the hit by rank, x = its record, h = its number in the batch, at = the prefix of its query.
// words / feats / cs_text / rows_text: what the records' offsets point into.  dst.cs / dst.rows get an entry for every hit (a caller
// whose batch carries none of a kind drops the array).  The copies run across the team; the small records are lane 0's
template<class C> MPA_HD inline void finish_gather_core(int32_t qid, const FinRec &x, const FinOut &o, int64_t h, const FinCounts &at, const uint32_t *words, const void *feats,
                                                        const char *cs_text, const char *rows_text, const FinDst &dst)
{
	const int64_t cig = at.cigar + o.cig, ft = at.feat + o.feat, cs = at.cs + o.cs, rw = at.rows + o.rows;
	if (C::lane() == 0) {
		uint32_t w[34];
		finish_hit_words(qid, x, o, cig, ft, w);
		uint32_t *d = (uint32_t*)(dst.hits + h);
		for (int i = 0; i < 34; ++i) d[i] = w[i];
		const bool has_cs = x.cs_len >= 0, has_rows = x.rows_stride >= 0;
		dst.cs[h] = FinCsRef{ has_cs ? cs : 0, has_cs ? x.cs_len : 0, has_cs ? 1 : 0 };
		dst.rows[h] = FinRowsRef{ has_rows ? rw : 0, has_rows ? x.rows_w : 0, has_rows ? x.rows_sta : 0, has_rows ? 1 : 0, 0 };
	}
	MPA_COOP_FOR(C, i, x.n_cigar) dst.cigars[cig + i] = words[x.cig_off + i];
	{	// a feature is 14 words, the last of them padding
		const uint32_t *s = (const uint32_t*)feats + 14 * x.feat_off;
		uint32_t *d = (uint32_t*)(dst.feats + ft);
		MPA_COOP_FOR(C, i, 14 * (int64_t)x.n_feat) d[i] = i % 14 == 13 ? 0u : s[i];
	}
	if (x.cs_len > 0) MPA_COOP_FOR(C, i, x.cs_len) dst.cs_text[cs + i] = cs_text[x.cs_off + i];
	if (x.rows_stride >= 0) {                                // the four rows closed up to their width, the STA bytes behind them (rows_apply)
		const int64_t w4 = 4 * (int64_t)x.rows_w;
		for (int k = 0; k < 4; ++k) MPA_COOP_FOR(C, i, x.rows_w) dst.rows_text[rw + k * (int64_t)x.rows_w + i] = rows_text[x.rows_off + k * (int64_t)x.rows_stride + i];
		MPA_COOP_FOR(C, i, x.rows_sta) dst.rows_text[rw + w4 + i] = rows_text[x.rows_off + 4 * (int64_t)x.rows_stride + i];
	}
}

} // namespace mpa
