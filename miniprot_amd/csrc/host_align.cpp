// host_align.cpp -- the host steps of the stage machine (host_map.cpp) between "DP results arrive" and "regions ranked": the second half
// of mp_align() (align.c:290-342) and the tail of mp_map() (map.c:228-237) for a whole batch.
//   spans_take_round1()   round 1 in, round 2 out: which spans the two extensions accepted (take_round1_emit_round2, or through
//                         spans_core.h with MPA_GPU_SPANS)
//   take_round3()         the last round in: (a) the CIGAR of every region (assemble_alignment), (b) the walks over it -- the mp_extra_*
//                         statistics, and with their knobs the cs strings and residue rows the formatter would otherwise build -- and
//                         (c) the final ranking (stage_finish)
// Steps (a) and (b) have a device twin and a model of it behind a knob each (MPA_GPU_SPANS, _STATS, _CS, _ROWS: StepMode of host_batch.h);
// the walks that run on the device share one call (walks_on_device).  Step (c) and the flatten loop of mpa_batch_finish() have one behind
// MPA_GPU_FINISH (host_finish.cpp, finish_core.h).  Everything but the two entry points is local to this file.
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstring>
#include <mutex>
#include <string>
#include "host_batch.h"

using namespace mpa;

namespace mpa {

// mp_extra_stop / mp_extra_start (align.c:214-237)
static int32_t dist_to_stop(const mpa_idx_s *mi, const Region &r, int64_t ae)
{
	uint8_t c[3];
	for (int64_t j = r.ve; j + 2 < ae; j += 3) {
		fetch_nt(mi, (int32_t)r.vid, j, j + 3, c);
		if (codon_aa(c) == 20) return (int32_t)(j - r.ve);
	}
	return -1;
}

static int32_t dist_to_start(const mpa_idx_s *mi, const Region &r, int64_t as, int64_t ae)
{
	uint8_t c[3];
	for (int64_t j = r.vs; j >= as && j + 2 < ae; j -= 3) {
		fetch_nt(mi, (int32_t)r.vid, j, j + 3, c);
		const uint8_t aa = codon_aa(c);
		if (aa == 20) break;
		if (aa == 12) return (int32_t)(r.vs - j);
	}
	return -1;
}

// mp_extra_cal (align.c:82-201): walk the CIGAR once, accumulate identity/score statistics and exon features
static void summarize_alignment(const mpa_idx_s *mi, const mpa_mapopt_t &opt, Region &r, const char *aa_full, int32_t qlen, int64_t win_end)
{
	const int64_t l_nt = win_end - r.vs;
	std::vector<uint8_t> ntv((size_t)std::max<int64_t>(l_nt, 1));
	fetch_nt(mi, (int32_t)r.vid, r.vs, win_end, ntv.data());
	const uint8_t *nt = ntv.data(), *aa20 = tab_aa20();
	const char *aa = aa_full + r.qs;
	const char *nt_char = "ACGTN";
	const bool has_stop = r.qe == qlen && r.dist_stop == 0;
	int32_t n_intron = 0;
	for (uint32_t c : r.cigar) { uint32_t op = c & 0xf; n_intron += (op == 3 || op == 12 || op == 13); }
	r.n_exon = n_intron + 1;
	r.feat.assign((size_t)r.n_exon + (has_stop ? 1 : 0), Feat());
	r.blen = r.n_iden = r.n_plus = r.n_fs = r.n_stop = r.dp_max = 0;
	int32_t nl = 0, al = 0, ft = 0;
	int32_t blen0 = 0, iden0 = 0, score0 = 0, fs0 = 0, stop0 = 0, phase0 = 0, qs0 = r.qs;
	int64_t vs0 = r.vs;
	char acc0[2] = { 0, 0 };
	auto score_codon = [&](uint8_t nt_aa, int32_t aa_idx) {
		const uint8_t q = aa20[(uint8_t)aa[aa_idx]];
		const int32_t s = opt.mat[nt_aa * opt.asize + q];
		r.n_stop += nt_aa == 20, r.n_iden += nt_aa == q, r.n_plus += s > 0, r.dp_max += s;
	};
	auto close_exon = [&](Feat &f, int64_t ve) {
		f.type = 0, f.vs = vs0, f.ve = ve, f.qs = qs0, f.qe = r.qs + al, f.phase = (int16_t)phase0;
		f.blen = r.blen - blen0, f.n_iden = r.n_iden - iden0, f.n_fs = r.n_fs - fs0, f.n_stop = r.n_stop - stop0, f.score = r.dp_max - score0;
		if (ft > 0) f.acceptor[0] = acc0[0], f.acceptor[1] = acc0[1];
	};
	for (uint32_t c : r.cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) {                                             // M
			for (int32_t l = 0; l < len; ++l) score_codon(codon_aa(nt + nl + 3 * l), al + l);
			nl += len * 3, al += len, r.blen += len * 3;
		} else if (op == 1) {                                      // I
			r.dp_max -= opt.go + opt.ge * len;
			al += len, r.blen += len * 3;
		} else if (op == 2) {                                      // D: in-frame stop codons inside deletions count
			for (int32_t l = 0; l < len; ++l) r.n_stop += codon_aa(nt + nl + 3 * l) == 20;
			r.dp_max -= opt.go + opt.ge * len;
			nl += len * 3, r.blen += len * 3;
		} else if (op == 10) {                                     // F
			r.dp_max -= opt.fs;
			nl += len, r.blen += len, r.n_fs++;
		} else if (op == 11) {                                     // G
			r.dp_max -= opt.fs;
			nl += len, ++al, r.blen += 3, r.n_fs++;
		} else if (op == 3 || op == 12 || op == 13) {              // N / U / V introns
			if (op != 3) {                                         // the codon split by a phase-1/2 intron
				uint8_t cod[3];
				if (op == 12) cod[0] = nt[nl], cod[1] = nt[nl + len - 2], cod[2] = nt[nl + len - 1];
				else cod[0] = nt[nl], cod[1] = nt[nl + 1], cod[2] = nt[nl + len - 1];
				score_codon(codon_aa(cod), al);
				r.blen += 3;
			}
			Feat &f = r.feat[ft];
			int64_t ve;
			if (op == 3) ve = r.vs + nl;
			else if (op == 12) ve = r.vs + nl + 1;
			else ve = r.vs + nl + 2;
			close_exon(f, ve);
			++ft;
			if (op == 3) vs0 = r.vs + nl + len, phase0 = 0;
			else if (op == 12) vs0 = r.vs + nl + len - 2, phase0 = 2;
			else vs0 = r.vs + nl + len - 1, phase0 = 1;
			f.donor[0] = f.ve - r.vs < l_nt ? nt_char[nt[f.ve - r.vs]] : '.';
			f.donor[1] = f.ve - r.vs + 1 < l_nt ? nt_char[nt[f.ve - r.vs + 1]] : '.';
			qs0 = f.qe, fs0 = r.n_fs, stop0 = r.n_stop, score0 = r.dp_max, blen0 = r.blen, iden0 = r.n_iden;
			acc0[0] = vs0 - r.vs >= 2 ? nt_char[nt[vs0 - r.vs - 2]] : '.';
			acc0[1] = vs0 - r.vs >= 1 ? nt_char[nt[vs0 - r.vs - 1]] : '.';
			nl += len, al += op != 3;
		}
	}
	close_exon(r.feat[ft], r.vs + nl);
	++ft;
	if (has_stop) {
		Feat &f = r.feat[ft++];
		f.type = 1, f.vs = r.ve, f.ve = r.ve + 3, f.qs = f.qe = r.qe + al, f.phase = 0, f.n_fs = 0, f.blen = 3, f.n_iden = 0;
	}
	assert(nl == r.ve - r.vs && al == r.qe - r.qs);
}

static void append_cigar(std::vector<uint32_t> &cig, uint32_t op, int32_t len)   // ns_push_cigar, nasw.h:141-152
{
	if (!cig.empty() && (cig.back() & 0xf) == op && op != 10 && op != 11) cig.back() += (uint32_t)len << 4;
	else cig.push_back((uint32_t)len << 4 | op);
}

// the tail of mp_map() after mp_align() (map.c:228-237)
static void stage_finish(mpa_batch_s *b, QueryState &qs)
{
	const mpa_mapopt_t &opt = b->opt;
	if (opt.flag & MPA_MF_NO_ALIGN) return;
	std::vector<Region> kept;
	for (Region &r : qs.regs) if (r.aligned) kept.push_back(std::move(r));
	qs.regs.swap(kept);
	sort_regions(qs.regs);
	prefer_multi_exon(qs.regs, opt.io);
	assign_parents(opt.mask_level, opt.mask_len, qs.regs, b->mi->opt.kmer);
	select_secondary(opt.pri_ratio, b->mi->opt.kmer * 2, opt.best_n, qs.regs);
}

static void store_result(Segment &s, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	if (s.task < 0) return;
	const mpa_dp_rst_t &o = rst[s.task];
	s.score = o.score;
	s.cigar.assign(pool + o.cigar_off, pool + o.cigar_off + o.n_cigar);
}

// round 1 in (rst == nullptr: there was nothing to compute), round 2 out: the spans the two extensions accepted, re-aligned with
// traceback (the first and the last mp_align_seq() call of align.c:297-300, 331)
static void take_round1_emit_round2(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	const mpa_mapopt_t &opt = b->opt;
	if (rst) parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		for (size_t pi = 0; pi < qs.plans.size(); ++pi) {
			AlignPlan &pl = qs.plans[pi];
			const mpa_dp_rst_t *mine = rst + qs.base1;                 // this query's slice of the round-1 results
			for (Segment &g : pl.gaps) store_result(g, mine, pool);
			// (spans_ext_aa, spans_core.h: a call that consumed no row extended nothing -- the (0, al + 1, INT32_MIN) of a window of fewer than three rows)
			pl.l_nt = mine[pl.t_left].nt_len, pl.l_aa = spans_ext_aa(mine[pl.t_left]);
			// the terminal-exon repeat counts iff the reference would have made it AND it reaches the end of the protein (align.c:290-296)
			if (pl.t_left2 >= 0 && pl.l_aa != pl.as1 && pl.l_nt < opt.max_ext && spans_ext_aa(mine[pl.t_left2]) == pl.as1)
				pl.l_nt = mine[pl.t_left2].nt_len, pl.l_aa = mine[pl.t_left2].aa_len, pl.l_rep = true;
			if (pl.has_right) {
				pl.r_nt = mine[pl.t_right].nt_len, pl.r_aa = spans_ext_aa(mine[pl.t_right]);
				if (pl.t_right2 >= 0 && pl.r_aa < qs.qlen - pl.mid_qe && pl.r_nt < opt.max_ext && spans_ext_aa(mine[pl.t_right2]) == qs.qlen - pl.mid_qe)
					pl.r_nt = mine[pl.t_right2].nt_len, pl.r_aa = mine[pl.t_right2].aa_len, pl.r_rep = true;
			}
		}
	});
	std::vector<mpa_dp_task_t> next;
	for (size_t qi = 0; qi < b->qs.size(); ++qi) {
		QueryState &qs = b->qs[qi];
		for (size_t pi = 0; pi < qs.plans.size(); ++pi) {
			AlignPlan &pl = qs.plans[pi];
			Region &r = qs.regs[pl.reg];
			// region start after the left extension (align.c:297-300); its span is the first mp_align_seq() call
			r.vs = pl.vs1 - pl.l_nt;
			r.qs = pl.as1 - pl.l_aa;
			pl.has_left_span = true;
			make_segment(b, qs, r, pl, (int32_t)(r.vs - pl.vs0), (int32_t)(pl.vs1 - pl.vs0), r.qs, pl.as1, (int32_t)qi, (int32_t)pi, next, pl.left_span);
			if (pl.has_right && pl.r_nt > 0 && pl.r_aa > 0) {             // the accepted right-extension span (align.c:331)
				const int32_t ne0 = (int32_t)(pl.mid_ve - pl.vs0);
				pl.has_right_span = true;
				make_segment(b, qs, r, pl, ne0, ne0 + pl.r_nt, pl.mid_qe, pl.mid_qe + pl.r_aa, (int32_t)qi, (int32_t)pi, next, pl.right_span);
			}
		}
	}
	b->tasks.swap(next);
}

// ---- take_round3: (a) results in, CIGAR and n_exon of every region; (b) the statistics pass; (c) stage_finish ----
// (a) the accepted spans' results and the region's CIGAR, end coordinates and DP score (align.c:302-338)
static void assemble_alignment(AlignPlan &pl, Region &r, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	int32_t score = 0;
	r.cigar.clear();
	if (pl.has_left_span) store_result(pl.left_span, rst, pool);
	if (pl.has_right_span) store_result(pl.right_span, rst, pool);
	int32_t words = 0;
	auto add = [&](const Segment &s) {
		for (uint32_t c : s.cigar) append_cigar(r.cigar, c & 0xf, (int32_t)(c >> 4));
		score += s.score, words += (int32_t)s.cigar.size();
	};
	if (pl.has_left_span) add(pl.left_span);
	for (const Segment &g : pl.gaps) add(g);
	if (pl.has_right_span) add(pl.right_span);
	r.ve = pl.mid_ve, r.qe = pl.mid_qe;
	if (pl.has_right && pl.r_nt > 0 && pl.r_aa > 0) r.ve += pl.r_nt, r.qe += pl.r_aa;
	r.aligned = true;
	r.dp_score = score, r.dp_max2 = 0;
	pl.n_merged = words - (int32_t)r.cigar.size();
}

// ---- (b) MPA_GPU_STATS: 0 / unset = the statistics pass on the host, as the reference walks it; 1 = on the device, on the context that
// ran the batch's DP rounds (stats_run.hip); model = the host instance of the device's code with a team of one (aln_stats_core.h) ----
static void stats_on_host(const mpa_batch_s *b, const QueryState &qs, const AlignPlan &pl, Region &r)
{
	r.dist_stop = dist_to_stop(b->mi, r, pl.ae);
	r.dist_start = dist_to_start(b->mi, r, pl.as, pl.ae);
	summarize_alignment(b->mi, b->opt, r, qs.seq, qs.qlen, pl.ae);
}

static int32_t count_exons(const Region &r)
{
	int32_t n_intron = 0;
	for (uint32_t c : r.cigar) { const uint32_t op = c & 0xf; n_intron += (op == 3 || op == 12 || op == 13); }
	return n_intron + 1;
}

static AlnStatsJob stats_job(const QueryState &qs, const AlignPlan &pl, const Region &r, int64_t q_off, int64_t cig_off, int64_t feat_off)
{
	AlnStatsJob J;
	J.vs = r.vs, J.ve = r.ve, J.as = pl.as, J.ae = pl.ae, J.q_off = q_off, J.cig_off = cig_off, J.feat_off = feat_off;
	J.vid = (int32_t)r.vid, J.qs = r.qs, J.qe = r.qe, J.qlen = qs.qlen, J.n_cigar = (int32_t)r.cigar.size(), J.pad = 0;
	return J;
}

// what the shared core computed for a region, into the region (n_exon is the host's: count_exons)
static void stats_apply(Region &r, const AlnStatsOut &o, const AlnFeat *f)
{
	assert(!o.bad);                                      // (the walk ends at (ve - vs, qe - qs): summarize_alignment's own check)
	r.dist_stop = o.dist_stop, r.dist_start = o.dist_start;
	r.dp_max = o.dp_max, r.blen = o.blen, r.n_iden = o.n_iden, r.n_plus = o.n_plus, r.n_fs = o.n_fs, r.n_stop = o.n_stop;
	r.feat.assign((size_t)o.n_feat, Feat());
	for (int32_t k = 0; k < o.n_feat; ++k) {
		Feat &d = r.feat[(size_t)k];
		const AlnFeat &s = f[k];
		d.vs = s.vs, d.ve = s.ve, d.qs = s.qs, d.qe = s.qe, d.type = s.type, d.phase = s.phase;
		d.n_fs = s.n_fs, d.n_stop = s.n_stop, d.score = s.score, d.n_iden = s.n_iden, d.blen = s.blen;
		memcpy(d.donor, s.donor, 2), memcpy(d.acceptor, s.acceptor, 2);
	}
}

static AlnStatsParams stats_params(const mpa_mapopt_t &opt) { return AlnStatsParams{ opt.go, opt.ge, opt.fs, opt.asize }; }

// (b) through the shared core on the host: a team of one per region
static void stats_model(mpa_batch_s *b)
{
	uint8_t tab[ALN_TAB_BYTES];
	aln_tables_fill(tab, b->opt.mat, 484);
	const AlnStatsParams p = stats_params(b->opt);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		std::vector<AlnFeat> feat;
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			const StatsGenomeHost g = genome_strand(b->mi, r.vid);
			feat.assign((size_t)r.n_exon + 1, AlnFeat());
			const AlnStatsOut o = aln_stats_core<StatsSerial>(stats_job(qs, pl, r, 0, 0, 0), p, tab, (const uint8_t*)qs.seq, r.cigar.data(), g, feat.data());
			stats_apply(r, o, feat.data());
		}
	});
}

// ---- (b') MPA_GPU_CS: the cs:Z: body of every aligned region, carried in the region to the result ----
// 0 / unset = the formatter builds it (put_cs_body, host_format.cpp); 1 = on the device behind the last DP round (k_aln_cs), on the
// batch's DP context; model = the host instance of the device's code with a team of one (aln_cs_core.h: the CPU tests)
// does the formatter print a cs string for these options at all?  (format_batch: the PAF line is printed unless MPA_MF_NO_PAF is set,
// and with --gtf only next to the residue rows of --aln / --trans)
static bool cs_printed(const mpa_mapopt_t &opt)
{
	if (opt.flag & (MPA_MF_NO_CS | MPA_MF_NO_ALIGN)) return false;
	if (opt.flag & MPA_MF_GTF) return (opt.flag & (MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS)) != 0;
	return !(opt.flag & MPA_MF_NO_PAF);
}

static void cs_apply(Region &r, const AlnCsOut &o, const char *body, int64_t bound, int8_t src)
{
	assert(!o.bad && o.len <= bound);                    // (the walk ends at (ve - vs, qe - qs), inside its slot)
	(void)bound;
	r.cs.assign(body, (size_t)o.len), r.cs_src = src;
}

// through the shared core on the host: a team of one per region
static void cs_model(mpa_batch_s *b)
{
	uint8_t tab[ALN_TAB_BYTES];
	aln_tables_fill(tab, b->opt.mat, 484);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		std::vector<char> slot;
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			const StatsGenomeHost g = genome_strand(b->mi, r.vid);
			const int64_t bound = aln_cs_bound(r.cigar.data(), (int32_t)r.cigar.size());
			slot.resize((size_t)bound + 1);
			const AlnCsOut o = aln_cs_core<StatsSerial>(stats_job(qs, pl, r, 0, 0, 0), tab, (const uint8_t*)qs.seq, r.cigar.data(), g, slot.data());
			cs_apply(r, o, slot.data(), bound, 1);
		}
	});
}

// ---- (b'') MPA_GPU_ROWS: the residue rows of --aln / --trans of every aligned region, carried in the region to the result (DESIGN.md
// section 4.9) ----  0 / unset = put_residues() of the formatter walks; 1 = on the device (k_aln_rows); model = the shared core on the
// host with a team of one
// does the formatter print residue rows for these options at all?
static bool rows_printed(const mpa_mapopt_t &opt)
{
	return !(opt.flag & MPA_MF_NO_ALIGN) && (opt.flag & (MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS)) != 0;
}

static AlnRowsParams rows_params(const mpa_mapopt_t &opt)
{
	return AlnRowsParams{ opt.asize, opt.max_intron_flank, (opt.flag & MPA_MF_SHOW_RESIDUE) != 0, (opt.flag & MPA_MF_SHOW_TRANS) != 0 };
}

// a slot as the shared core left it, into the region: the four rows closed up to their width, the STA bytes behind them
static void rows_apply(Region &r, const AlnRowsParams &p, const AlnRowsOut &o, const char *slot, int64_t slot_bytes, int8_t src)
{
	const int64_t stride = p.show_aln ? aln_rows_cols(r.cigar.data(), (int32_t)r.cigar.size(), p.flank) + 3 : 0;
	const int32_t n_sta = p.show_trans ? o.n_sta : 0;
	assert(!o.bad && o.width <= stride && 4 * stride + n_sta <= slot_bytes);   // (the walk ends at (ve - vs, qe - qs), inside its slot)
	(void)slot_bytes;
	r.rows.clear(), r.rows.reserve((size_t)(4 * (int64_t)o.width + n_sta));
	for (int k = 0; k < 4 && p.show_aln; ++k) r.rows.append(slot + k * stride, (size_t)o.width);
	r.rows.append(slot + 4 * stride, (size_t)n_sta);
	r.rows_w = o.width, r.rows_sta = n_sta, r.rows_src = src;
}

// through the shared core on the host: a team of one per region
static void rows_model(mpa_batch_s *b)
{
	uint8_t tab[ALN_TAB_BYTES];
	aln_tables_fill(tab, b->opt.mat, 484);
	const AlnRowsParams p = rows_params(b->opt);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		std::vector<char> slot;
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			const StatsGenomeHost g = genome_strand(b->mi, r.vid);
			const int64_t bytes = aln_rows_slot(r.cigar.data(), (int32_t)r.cigar.size(), p);
			slot.resize((size_t)bytes + 1);
			const AlnRowsOut o = aln_rows_core<StatsSerial>(stats_job(qs, pl, r, 0, 0, 0), p, tab, (const uint8_t*)qs.seq, r.cigar.data(), g, slot.data());
			rows_apply(r, p, o, slot.data(), bytes, 1);
		}
	});
}

// The walks over the finished alignments on the device in one call, for any of the statistics (`stats`), the cs strings (`cs_on`) and
// the residue rows (`rows_on`): one upload, a launch each, one wait.  MPA_OK: done (*ran: there was something to do);
// MPA_ERR_UNSUPPORTED: the device declined (the last error says why) and nothing was changed; anything else is an error of the call
// want_fin (MPA_GPU_FINISH=1, with stats): the ranking and the flat result run in the same call behind the walks' kernels (DESIGN.md section
// 4.13): only the records' host-side fields go up next to the jobs, the walks' output is neither downloaded nor applied to the regions, and
// b->flat is the batch's result.  *fin_why: why that part declined (the walks then ran as without it)
// want_fmt (MPA_GPU_FORMAT=1, with want_fin and the batch's names): the batch's output text is written behind the
// gather of the same call and stays with b->flat.  *fmt_why: why that part declined (the rest ran as without it)
static int walks_on_device(mpa_batch_s *b, mpa_ctx_t *ctx, bool stats, bool cs_on, bool rows_on, bool *ran, bool want_fin = false, std::string *fin_why = nullptr, bool want_fmt = false,
                           std::string *fmt_why = nullptr)
{
	const double t_call = now_ms();
	const size_t nq = b->qs.size();
	const AlnRowsParams rp = rows_params(b->opt);
	std::vector<int64_t> job0(nq + 1, 0), cig0(nq + 1, 0), feat0(nq + 1, 0), slot0(nq + 1, 0), rslot0(nq + 1, 0);
	std::atomic<bool> too_wide(false);
	parallel_for(b->n_threads, (int64_t)nq, [&](int64_t qi) {                // (the bounds walk every CIGAR: per query, then the prefix)
		const QueryState &qs = b->qs[qi];
		int64_t nc = 0, nf = 0, nb = 0, nr = 0;
		for (const AlignPlan &pl : qs.plans) {
			const Region &r = qs.regs[pl.reg];
			nc += (int64_t)r.cigar.size(), nf += (int64_t)r.n_exon + 1;
			if (cs_on) nb += aln_cs_bound(r.cigar.data(), (int32_t)r.cigar.size());
			if (rows_on) {
				const int64_t bytes = aln_rows_slot(r.cigar.data(), (int32_t)r.cigar.size(), rp);
				if (bytes > (int64_t)1 << 30) too_wide = true;           // (the core counts columns in 32 bits)
				nr += bytes;
			}
		}
		job0[qi + 1] = (int64_t)qs.plans.size(), cig0[qi + 1] = nc, feat0[qi + 1] = nf, slot0[qi + 1] = nb, rslot0[qi + 1] = nr;
	});
	for (size_t qi = 0; qi < nq; ++qi)
		job0[qi + 1] += job0[qi], cig0[qi + 1] += cig0[qi], feat0[qi + 1] += feat0[qi], slot0[qi + 1] += slot0[qi], rslot0[qi + 1] += rslot0[qi];
	const int64_t n_jobs = job0[nq], n_cigar = cig0[nq], n_feat = stats ? feat0[nq] : -1, slot_bytes = cs_on ? slot0[nq] : -1, rows_bytes = rows_on ? rslot0[nq] : -1;
	*ran = n_jobs > 0;
	if (n_jobs == 0) return MPA_OK;
	if (too_wide) { set_error("GPU residue rows: an alignment of more than 2^30 bytes of rows"); return MPA_ERR_UNSUPPORTED; }
	const int64_t t0 = b->q.q_off[0], text_bytes = b->q.q_off[b->q.n_seq] - t0;
	AlnStatsIO io;
	AlnCsIO cs;
	AlnRowsIO rows;
	// MPA_GPU_SPANS=1: k_assemble left the words on this context; they are neither staged nor uploaded
	const bool dev_cig = (int64_t)b->sp_cig_off.size() == n_jobs;
	const int64_t n_up = dev_cig ? 0 : n_cigar;
	const AlnWalkSizes z{ n_jobs, n_up, text_bytes, n_feat, slot_bytes, rows_bytes };
	int rc = dev_aln_walks_stage(ctx, z, io, cs, rows);
	if (rc != MPA_OK) return rc;
	if (text_bytes > 0) memcpy(io.text, b->q.seqs + t0, (size_t)text_bytes);
	if (cs_on) cs.slot_off[n_jobs] = slot_bytes;
	if (rows_on) rows.slot_off[n_jobs] = rows_bytes;
	FinishResident fr;
	FinishTables ft;
	if (want_fin) {
		// (a record per aligned region in the order of the query's regions, as stage_finish meets them; every one of them has a plan)
		for (size_t qi = 0; qi < nq && want_fin; ++qi) {
			int64_t n_aln = 0;
			for (const Region &r : b->qs[qi].regs) n_aln += r.aligned;
			if (n_aln != (int64_t)b->qs[qi].plans.size()) want_fin = false, *fin_why = "an aligned region without a plan";
		}
		fr.p = FinParams{ b->mi->opt.kmer, b->opt.mask_len, b->opt.best_n, b->opt.io, b->opt.mask_level, b->opt.pri_ratio };
		fr.z = FinishSizes{ (int64_t)nq, n_jobs, finish_count_big(job0.data(), (int64_t)nq), 0, 0, 0, 0, n_cigar, feat0[nq], cs_on ? slot_bytes : 0, rows_on ? rows_bytes : 0 };
		if (want_fin) {
			rc = dev_finish_stage(ctx, fr.z, ft);
			if (rc == MPA_ERR_UNSUPPORTED) want_fin = false, *fin_why = mpa_last_error();
			else if (rc != MPA_OK) return rc;
		}
		if (want_fin) memcpy(ft.first, job0.data(), (nq + 1) * 8);
	}
	// (MPA_GPU_FORMAT=1) the names and lengths the text needs, and room for it from bounds: a fixed allowance for a line's fields, 11 bytes
	// per CIGAR word, the cs and rows slots, a line per feature slot, the names wherever a line repeats them (format_bounds' figures)
	FormatResident fmr;
	want_fmt = want_fmt && want_fin;
	if (want_fmt && !format_opt_from(b->opt, fmr.o)) want_fmt = false, *fmt_why = "a gff_prefix longer than 64 bytes";
	if (want_fmt) {
		const std::vector<Contig> &ctg = b->mi->ctg;
		FormatSizes &fz = fmr.z;
		fz = FormatSizes{};
		fz.n_query = (int64_t)nq, fz.n_place = n_jobs, fz.n_ctg = (int64_t)ctg.size();
		for (const Contig &c : ctg) fz.cname_bytes += (int64_t)c.name.size();
		const bool annot = (b->opt.flag & (MPA_MF_GFF | MPA_MF_GTF)) != 0;
		int64_t text = 11 * n_cigar + (cs_on ? slot_bytes : 0) + (rows_on ? rows_bytes + 35 * n_jobs : 0), ids = 0;
		for (size_t qi = 0; qi < nq; ++qi) {
			const QueryState &qs = b->qs[qi];
			const int64_t qn = (int64_t)strlen(b->fmt_names[qi]);
			fz.qname_bytes += qn, text += qn + 128;
			for (const AlignPlan &pl : qs.plans) {
				const Region &r = qs.regs[pl.reg];
				const int64_t cn = (int64_t)ctg[r.vid >> 1].name.size(), nf = (int64_t)r.n_exon + 1;
				text += 640 + qn + cn;
				if (annot) text += (2 + 2 * nf) * (400 + cn + 2 * qn + 2 * fmr.o.prefix_len), ids += 3 + 4 * nf;
			}
		}
		fz.text_cap = text, fz.id_cap = ids;
		FormatTables up;
		rc = dev_format_stage(ctx, fz, up);
		if (rc == MPA_ERR_UNSUPPORTED) want_fmt = false, *fmt_why = mpa_last_error();
		else if (rc != MPA_OK) return rc;
		if (want_fmt) {
			up.qname_off[0] = 0, up.cname_off[0] = 0, up.hit_off[0] = 0;
			for (size_t qi = 0; qi < nq; ++qi) {
				const size_t n = strlen(b->fmt_names[qi]);
				memcpy(up.qname + up.qname_off[qi], b->fmt_names[qi], n);
				up.qname_off[qi + 1] = up.qname_off[qi] + (int64_t)n, up.hit_off[qi + 1] = 0;
				up.q_off[qi] = b->q.q_off[qi];
			}
			up.q_off[nq] = b->q.q_off[nq];
			for (size_t c = 0; c < ctg.size(); ++c) {
				memcpy(up.cname + up.cname_off[c], ctg[c].name.data(), ctg[c].name.size());
				up.cname_off[c + 1] = up.cname_off[c] + (int64_t)ctg[c].name.size(), up.clen[c] = ctg[c].len;
			}
		}
	}
	parallel_for(b->n_threads, (int64_t)nq, [&](int64_t qi) {
		const QueryState &qs = b->qs[qi];
		int64_t j = job0[qi], c = cig0[qi], f = feat0[qi], s = slot0[qi], rs = rslot0[qi];
		for (const AlignPlan &pl : qs.plans) {
			const Region &r = qs.regs[pl.reg];
			if (cs_on) cs.slot_off[j] = s, s += aln_cs_bound(r.cigar.data(), (int32_t)r.cigar.size());
			if (rows_on) rows.slot_off[j] = rs, rs += aln_rows_slot(r.cigar.data(), (int32_t)r.cigar.size(), rp);
			io.jobs[j] = stats_job(qs, pl, r, (qs.seq - b->q.seqs) - t0, dev_cig ? b->sp_cig_off[(size_t)j] : c, f);
			if (want_fin) {
				int64_t at = job0[qi];                                  // (its place among the query's records: plans with a smaller region number)
				for (const AlignPlan &o : qs.plans) at += o.reg < pl.reg;
				FinRec &x = ft.rec[at];
				memset(&x, 0, sizeof x);
				x.vs = r.vs, x.ve = r.ve, x.cig_off = io.jobs[j].cig_off, x.feat_off = f, x.vid = r.vid, x.hash = r.hash, x.qs = r.qs, x.qe = r.qe, x.cnt = r.cnt, x.n_exon = r.n_exon;
				x.chn_sc = r.chn_sc, x.chn_sc_ungap = r.chn_sc_ungap, x.parent = r.parent, x.n_sub = r.n_sub, x.subsc = r.subsc, x.dp_max2 = r.dp_max2, x.dp_score = r.dp_score;
				x.n_cigar = (int32_t)r.cigar.size(), x.job = (int32_t)j, x.cs_len = -1, x.rows_stride = -1;      // (k_finish_fill: the statistics, cs_len, the rows' width)
				if (cs_on) x.cs_off = cs.slot_off[j];
				if (rows_on) x.rows_off = rows.slot_off[j], x.rows_stride = rp.show_aln ? (int32_t)(aln_rows_cols(r.cigar.data(), (int32_t)r.cigar.size(), rp.flank) + 3) : 0;
			}
			++j;
			if (!dev_cig && !r.cigar.empty()) memcpy(io.cigar + c, r.cigar.data(), r.cigar.size() * 4);
			c += (int64_t)r.cigar.size(), f += (int64_t)r.n_exon + 1;
		}
	});
	rc = dev_aln_walks(ctx, const_cast<mpa_idx_s*>(b->mi), stats_params(b->opt), rp, b->opt.mat, z, io, cs, rows, dev_cig, want_fin ? &fr : nullptr, want_fmt ? &fmr : nullptr);
	if (rc != MPA_OK) return rc;
	if (timing_on() && dev_cig) fprintf(stderr, "[mpa-timing]   walks upload: %lld alignments, %lld CIGAR words (the assembled pool is on the device)\n", (long long)n_jobs, (long long)n_up);
	if (want_fin) {                                      // the result is laid out: nothing to apply to the regions
		std::unique_ptr<mpa_result_s> res(new mpa_result_s());
		finish_flat_to_result(fr.flat, (int64_t)nq, res.get());
		if (timing_on()) fprintf(stderr, "[mpa-timing]   finish on the GPU: %lld queries, %lld hits in, %lld kept, %lld bytes down, %.3f ms\n", (long long)nq, (long long)n_jobs,
		                         (long long)res->hits.size(), (long long)fr.flat.bytes_down, now_ms() - t_call);
		if (want_fmt && fmr.out.declined) *fmt_why = format_decline_reason(fmr.out.tot, fmr.z.text_cap, fmr.z.id_cap);
		else if (want_fmt) {                                 // (out of the pinned block: the context's next call reuses it)
			res->fmt_text.assign(fmr.out.text, (size_t)fmr.out.tot.bytes), res->fmt_id_at.assign(fmr.out.id_at, fmr.out.id_at + fmr.out.tot.ids), res->fmt_n_out = fmr.out.tot.n_out;
		}
		b->flat = std::move(res), b->flat_cs_src = cs_on ? 2 : 0;
		return MPA_OK;
	}
	if (timing_on() && cs_on) {                          // what came down against what it held (the bounded slots: DESIGN.md section 4.8)
		int64_t used = 0;
		for (int64_t j = 0; j < n_jobs; ++j) used += cs.out[j].len;
		fprintf(stderr, "[mpa-timing]   cs slots: %lld alignments, %lld bytes down, %lld bytes of strings\n", (long long)n_jobs, (long long)slot_bytes, (long long)used);
	}
	if (timing_on() && rows_on) {                        // (exact slots but for the trailing codon: DESIGN.md section 4.9)
		int64_t used = 0;
		for (int64_t j = 0; j < n_jobs; ++j) used += 4 * (int64_t)rows.out[j].width + (rp.show_trans ? rows.out[j].n_sta : 0);
		fprintf(stderr, "[mpa-timing]   rows slots: %lld alignments, %lld bytes down, %lld bytes of rows\n", (long long)n_jobs, (long long)rows_bytes, (long long)used);
	}
	parallel_for(b->n_threads, (int64_t)nq, [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		int64_t j = job0[qi];
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			if (stats) stats_apply(r, io.out[j], io.feat + io.jobs[j].feat_off);
			if (cs_on) cs_apply(r, cs.out[j], cs.body + cs.slot_off[j], cs.slot_off[j + 1] - cs.slot_off[j], 2);
			if (rows_on) rows_apply(r, rp, rows.out[j], rows.body + rows.slot_off[j], rows.slot_off[j + 1] - rows.slot_off[j], 2);
			++j;
		}
	});
	return MPA_OK;
}

// MPA_CS_DUMP=<file> (diagnostics; the tests' view of the step): behind stage_finish, one record per aligned region in query and region
// order, whichever path produced the body (a region that carries none gets the formatter's, put_cs_body).  Per record: int32 query
// number, vid; int64 vs, ve; int32 qs, qe, source (0 host, 1 shared core, 2 device), length; the body.  Layout and parser: tests/csdump.py
static void cs_dump(const mpa_batch_s *b)
{
	const char *fn = getenv("MPA_CS_DUMP");
	if (!fn || !*fn) return;
	static std::mutex mu;                                // (batches of a stream finish side by side: one writer at a time)
	std::lock_guard<std::mutex> g(mu);
	FILE *fp = fopen(fn, "ab");
	if (!fp) return;
	std::string body;
	if (b->flat) {                                       // (MPA_GPU_FINISH ran: the ranked hits are the flat result's, the regions were left unranked)
		const mpa_result_s &R = *b->flat;
		for (size_t h = 0; h < R.hits.size(); ++h) {
			const mpa_hit_t &x = R.hits[h];
			const bool carried = !R.cs.empty() && R.cs[h].present;
			const char *s = carried ? R.cs_text.data() + R.cs[h].off : nullptr;
			int32_t len = carried ? R.cs[h].len : 0;
			if (!carried) body.clear(), put_cs_body(body, b->mi, b->qs[(size_t)x.qid].seq + x.qs, (int32_t)x.vid, x.vs, x.ve, R.cigars.data() + x.cigar_off, x.n_cigar), s = body.data(), len = (int32_t)body.size();
			const int32_t a[2] = { x.qid, (int32_t)x.vid };
			const int64_t v[2] = { x.vs, x.ve };
			const int32_t w[4] = { x.qs, x.qe, carried ? b->flat_cs_src : 0, len };
			fwrite(a, 4, 2, fp), fwrite(v, 8, 2, fp), fwrite(w, 4, 4, fp);
			if (len > 0) fwrite(s, 1, (size_t)len, fp);
		}
		fclose(fp);
		return;
	}
	for (const QueryState &qs : b->qs)
		for (const Region &r : qs.regs) {
			if (!r.aligned) continue;
			const std::string *s = &r.cs;
			if (!r.cs_src) body.clear(), put_cs_body(body, b->mi, qs.seq + r.qs, (int32_t)r.vid, r.vs, r.ve, r.cigar.data(), (int32_t)r.cigar.size()), s = &body;
			const int32_t a[2] = { qs.qid, (int32_t)r.vid };
			const int64_t v[2] = { r.vs, r.ve };
			const int32_t w[4] = { r.qs, r.qe, r.cs_src, (int32_t)s->size() };
			fwrite(a, 4, 2, fp), fwrite(v, 8, 2, fp), fwrite(w, 4, 4, fp);
			if (!s->empty()) fwrite(s->data(), 1, s->size(), fp);
		}
	fclose(fp);
}

// ---- MPA_GPU_SPANS: the step between the DP rounds (take_round1_emit_round2) and step (a) behind them (assemble_alignment,
// count_exons) through spans_core.h ----  0 / unset = the host functions above; 1 = on the device, on the
// batch's DP context (k_spans, k_spans_emit, k_assemble: span_kernels.hip); model = the shared core on the host with a team of one
static bool spans_dump_on() { const char *fn = getenv("MPA_SPANS_DUMP"); return fn && *fn; }
static SpansParams spans_params(const mpa_mapopt_t &opt) { return SpansParams{ opt.kmer2, opt.max_ext, opt.io, opt.asize }; }

// the batch's plans and gap segments as the shared core reads them: query-major, plans in order (plan0[q]: the first plan of query q)
static void spans_counts(const mpa_batch_s *b, std::vector<int64_t> &plan0, std::vector<int64_t> &seg0)
{
	const size_t nq = b->qs.size();
	plan0.assign(nq + 1, 0), seg0.assign(nq + 1, 0);
	for (size_t qi = 0; qi < nq; ++qi) {
		int64_t ns = 0;
		for (const AlignPlan &pl : b->qs[qi].plans) ns += (int64_t)pl.gaps.size();
		plan0[qi + 1] = plan0[qi] + (int64_t)b->qs[qi].plans.size(), seg0[qi + 1] = seg0[qi] + ns;
	}
}
static void spans_flatten(mpa_batch_s *b, const std::vector<int64_t> &plan0, const std::vector<int64_t> &seg0, SpansPlan *plan, SegRec *seg)
{
	const int64_t t0 = b->q.q_off[0];
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		const QueryState &qs = b->qs[qi];
		int64_t j = plan0[qi], g = seg0[qi];
		for (const AlignPlan &pl : qs.plans) {
			SpansPlan &P = plan[j++];
			PlanRec &y = P.pl;
			y.as = pl.as, y.ae = pl.ae, y.vs0 = pl.vs0, y.vs1 = pl.vs1, y.mid_ve = pl.mid_ve, y.reg = pl.reg, y.as1 = pl.as1, y.mid_qe = pl.mid_qe, y.has_right = pl.has_right ? 1 : 0;
			y.t_left = pl.t_left, y.t_left2 = pl.t_left2, y.t_right = pl.t_right, y.t_right2 = pl.t_right2, y.gap0 = (int32_t)g, y.n_gap = (int32_t)pl.gaps.size();
			P.q_off = (qs.seq - b->q.seqs) - t0, P.qid = qs.qid, P.qlen = qs.qlen, P.vid = qs.regs[pl.reg].vid, P.base1 = (int32_t)qs.base1;
			for (const Segment &s : pl.gaps) seg[g++] = rec_of_segment(s);
		}
	});
}
static void span_segment_apply(Segment &s, const SegRec &z)
{
	s.cigar.clear();                                     // (a DP segment's words of an earlier take; they arrive behind round 2)
	segment_from_rec(s, z);
}
// what spans_accept left (on the host or on the device), into the plans, the regions and the batch's task list
static void spans_apply_round1(mpa_batch_s *b, const std::vector<int64_t> &plan0, const SpanRec *rec, const mpa_dp_task_t *task, int64_t n_task)
{
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		int64_t j = plan0[qi];
		for (AlignPlan &pl : qs.plans) {
			const SpanRec &R = rec[j++];
			Region &r = qs.regs[pl.reg];
			pl.l_nt = R.l_nt, pl.l_aa = R.l_aa, pl.r_nt = R.r_nt, pl.r_aa = R.r_aa;
			r.vs = R.vs, r.qs = R.qs;
			pl.has_left_span = true, span_segment_apply(pl.left_span, R.left);
			pl.has_right_span = (R.flags & SPANS_RIGHT) != 0, pl.l_rep = (R.flags & SPANS_LREP) != 0, pl.r_rep = (R.flags & SPANS_RREP) != 0;
			if (pl.has_right_span) span_segment_apply(pl.right_span, R.right);
		}
	});
	b->tasks.assign(task, task + n_task);
}
// the record of a plan back from its state (behind round 2 the shared core reads what round 1 left)
static SpanRec span_rec_of(const AlignPlan &pl, const Region &r)
{
	SpanRec R;
	R.vs = r.vs, R.qs = r.qs, R.l_nt = pl.l_nt, R.l_aa = pl.l_aa, R.r_nt = pl.r_nt, R.r_aa = pl.r_aa, R.flags = SPANS_LEFT | (pl.has_right_span ? SPANS_RIGHT : 0) | (pl.l_rep ? SPANS_LREP : 0) | (pl.r_rep ? SPANS_RREP : 0);
	R.left = rec_of_segment(pl.left_span);
	R.right = pl.has_right_span ? rec_of_segment(pl.right_span) : SegRec{ 0, 0, 0, 0, -1, 0 };
	return R;
}
static void spans_keep_round1(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool, bool copy_pool)
{
	b->sp_rst1.assign(rst, rst + b->tasks.size());
	free(b->sp_pool1), b->sp_pool1 = nullptr;
	b->spans_want_pool = !copy_pool;                     // (the device path: run_dp_rounds hands the executor's block over)
	if (copy_pool) {
		int64_t n = 0;
		for (const mpa_dp_rst_t &o : b->sp_rst1) n = std::max<int64_t>(n, o.cigar_off + o.n_cigar);
		b->sp_pool1 = (uint32_t*)malloc((size_t)(n > 0 ? n : 1) * 4);
		if (n > 0) memcpy(b->sp_pool1, pool, (size_t)n * 4);
	}
}

// between the rounds through the shared core on the host: one lane per plan, the task numbers from a running count
static void spans_round1_model(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	std::vector<int64_t> plan0, seg0;
	spans_counts(b, plan0, seg0);
	const int64_t n_plan = plan0.back();
	std::vector<SpansPlan> plan((size_t)n_plan);
	std::vector<SegRec> seg((size_t)seg0.back() + 1);
	spans_flatten(b, plan0, seg0, plan.data(), seg.data());
	uint8_t tab[ALN_TAB_BYTES];
	aln_tables_fill(tab, b->opt.mat, 484);
	const SpansParams p = spans_params(b->opt);
	std::vector<SpanRec> rec((size_t)n_plan);
	std::vector<mpa_dp_task_t> task;
	const uint8_t *text = (const uint8_t*)b->q.seqs + b->q.q_off[0];
	for (int64_t j = 0; j < n_plan; ++j) {
		const StatsGenomeHost g = genome_strand(b->mi, plan[j].vid);
		mpa_dp_task_t t[2];
		const int32_t n = spans_accept(p, plan[j], rst, g, tab, text, rec[j], t), t0 = (int32_t)task.size();
		if (rec[j].left.task >= 0) rec[j].left.task += t0;
		if (rec[j].right.task >= 0) rec[j].right.task += t0;
		task.insert(task.end(), t, t + n);
	}
	spans_keep_round1(b, rst, pool, true);
	spans_apply_round1(b, plan0, rec.data(), task.data(), (int64_t)task.size());
}

// between the rounds on the device.  MPA_OK: done; MPA_ERR_UNSUPPORTED: the device declined and nothing was changed
static int spans_round1_device(mpa_batch_s *b, mpa_ctx_t *ctx, const mpa_dp_rst_t *rst)
{
	std::vector<int64_t> plan0, seg0;
	spans_counts(b, plan0, seg0);
	const int64_t n_plan = plan0.back(), n_seg = seg0.back(), n_rst1 = (int64_t)b->tasks.size();
	const int64_t t0 = b->q.q_off[0], text_bytes = b->q.q_off[b->q.n_seq] - t0;
	SpansIO io;
	int rc = dev_spans_stage(ctx, n_plan, n_seg, n_rst1, text_bytes, io);
	if (rc != MPA_OK) return rc;
	spans_flatten(b, plan0, seg0, io.plan, io.seg);
	memcpy(io.rst1, rst, (size_t)n_rst1 * sizeof(mpa_dp_rst_t));
	if (text_bytes > 0) memcpy(io.text, b->q.seqs + t0, (size_t)text_bytes);
	rc = dev_spans_round1(ctx, const_cast<mpa_idx_s*>(b->mi), spans_params(b->opt), b->opt.mat, n_plan, n_seg, n_rst1, text_bytes, nullptr, b->dp_n_pool, io);
	if (rc != MPA_OK) return rc;
	spans_keep_round1(b, rst, nullptr, false);
	spans_apply_round1(b, plan0, io.rec, io.task, io.n_task);
	b->r2_in = io.r2;                                    // (MPA_GPU_ROUND2=1: the tasks in place and their bounds, for run_dp_rounds)
	return MPA_OK;
}

// a step's mode for this batch: the device only where the batch has a context (the stage machine without one: mpa_batch_begin)
static StepMode batch_step_mode(const mpa_batch_s *b, const char *env_name)
{
	const StepMode m = step_mode(env_name);
	return m == STEP_DEVICE && !b->dp_ctx ? STEP_HOST : m;
}

// MPA_GPU_ROUND1=1: round 1 of the batch with the step between the rounds chained into its submission.  The step's
// block is staged here -- counts, plans, gap segments, text; no result record -- and dp_run_round1_chained sends it up before the round is
// launched, runs the round from `tasks`, the step's kernels behind its results kernels, and waits once.  MPA_OK: rst[n] and *n_pool as
// from a resident round, and the step's outputs wait in b->r1_io for spans_take_round1.  MPA_ERR_UNSUPPORTED: declined, *why says what
// held it back before the device was asked (null: the last error says it) -- the batch is untouched and takes mpa_dp_run
int spans_round1_resident(mpa_batch_s *b, mpa_ctx_t *ctx, const mpa_dpopt_t *dpopt, int64_t n, const mpa_dp_task_t *tasks, mpa_dp_rst_t *rst, int64_t *n_pool, const char **why)
{
	*why = nullptr;
	b->r1_prefetched = false, b->r1_resident = false, b->r1_io = SpansIO(), b->r1_n_pool = 0;
	if (!ctx || !b->dp_ctx) { *why = "the batch has no DP context"; return MPA_ERR_UNSUPPORTED; }
	if (batch_step_mode(b, "MPA_GPU_SPANS") != STEP_DEVICE) { *why = "MPA_GPU_SPANS is not 1"; return MPA_ERR_UNSUPPORTED; }
	std::vector<int64_t> plan0, seg0;
	spans_counts(b, plan0, seg0);
	const int64_t n_plan = plan0.back(), n_seg = seg0.back();
	if (n_plan <= 0) { *why = "no plan in the batch"; return MPA_ERR_UNSUPPORTED; }
	const int64_t t0 = b->q.q_off[0], text_bytes = b->q.q_off[b->q.n_seq] - t0;
	SpansIO io;
	int rc = dev_spans_stage(ctx, n_plan, n_seg, n, text_bytes, io);
	if (rc != MPA_OK) return rc;
	spans_flatten(b, plan0, seg0, io.plan, io.seg);
	if (text_bytes > 0) memcpy(io.text, b->q.seqs + t0, (size_t)text_bytes);
	const SpansChain c{ spans_params(b->opt), b->opt.mat, n_plan, n_seg, n, text_bytes, round2_knob() };
	if ((rc = dp_run_round1_chained(ctx, b->mi, dpopt, &b->q, n, tasks, c, rst, n_pool, io, nullptr)) != MPA_OK) return rc;
	b->r1_io = io, b->r1_prefetched = true, b->r1_n_pool = *n_pool;
	return MPA_OK;
}

// MPA_OK, or the error of a device call that failed (a call that merely declines leaves the batch to the host step)
int spans_take_round1(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	const StepMode mode = batch_step_mode(b, "MPA_GPU_SPANS");
	b->spans_src = 0;
	b->r2_in = DpResidentIn(), b->r2_resident = false, b->r2_rst_dev = nullptr;
	const bool prefetched = b->r1_prefetched;
	b->r1_prefetched = false, b->r1_resident = false;
	if (prefetched && rst) {                             // (MPA_GPU_ROUND1=1) the step ran inside round 1's wait: its outputs are here already
		std::vector<int64_t> plan0, seg0;
		spans_counts(b, plan0, seg0);
		spans_keep_round1(b, rst, nullptr, false);
		spans_apply_round1(b, plan0, b->r1_io.rec, b->r1_io.task, b->r1_io.n_task);
		b->r2_in = b->r1_io.r2, b->r1_io = SpansIO();
		b->spans_src = 2, b->r1_resident = true;
		return MPA_OK;
	}
	bool any_plan = false;
	for (const QueryState &qs : b->qs) any_plan = any_plan || !qs.plans.empty();
	if (mode != STEP_HOST && rst && any_plan) {
		const double t0 = now_ms();
		if (mode == STEP_MODEL) {
			spans_round1_model(b, rst, pool);
			b->spans_src = 1;
			timing_note("spans: shared core", now_ms() - t0);
			return MPA_OK;
		}
		const int rc = spans_round1_device(b, b->dp_ctx, rst);
		if (rc == MPA_OK) {
			b->spans_src = 2;
			timing_note("spans on the GPU", now_ms() - t0);
			return MPA_OK;
		}
		if (rc != MPA_ERR_UNSUPPORTED) return rc;
		if (timing_on()) fprintf(stderr, "[mpa-timing]   device spans declined (%s): accepted spans on the host\n", mpa_last_error());
	}
	take_round1_emit_round2(b, rst, pool);
	return MPA_OK;
}

// step (a) behind round 2 on the host for a batch whose round 1 went through the shared core: the gap segments' words come from the
// kept round-1 results
static void spans_assemble_host(mpa_batch_s *b, const mpa_dp_rst_t *rst2, const uint32_t *pool2)
{
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			for (Segment &g : pl.gaps) store_result(g, b->sp_rst1.data() + qs.base1, b->sp_pool1);
			assemble_alignment(pl, r, rst2, pool2);
			r.n_exon = count_exons(r);
		}
	});
}
static void asm_apply(AlignPlan &pl, Region &r, const AsmRec &A, const uint32_t *words, const mpa_dp_rst_t *rst2)
{
	pl.n_merged = A.n_merged;
	if (pl.left_span.task >= 0) pl.left_span.score = rst2[pl.left_span.task].score;       // (as store_result leaves the spans; their words stay in the pool)
	if (pl.has_right_span && pl.right_span.task >= 0) pl.right_span.score = rst2[pl.right_span.task].score;
	r.cigar.assign(words, words + A.n_cigar);
	r.ve = A.ve, r.qe = A.qe, r.aligned = true, r.dp_score = A.dp_score, r.dp_max2 = 0, r.n_exon = A.n_exon;
}
// every plan's slot in words: the sum of its segments' words (merges only shorten it)
static void spans_slots(mpa_batch_s *b, const std::vector<int64_t> &plan0, const mpa_dp_rst_t *rst2, int64_t *slot_off)
{
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		const QueryState &qs = b->qs[qi];
		int64_t j = plan0[qi];
		const mpa_dp_rst_t *mine = b->sp_rst1.data() + qs.base1;
		for (const AlignPlan &pl : qs.plans) {
			int64_t n = pl.left_span.task < 0 ? 1 : rst2[pl.left_span.task].n_cigar;
			for (const Segment &g : pl.gaps) n += g.task < 0 ? 1 : mine[g.task].n_cigar;
			if (pl.has_right_span) n += pl.right_span.task < 0 ? 1 : rst2[pl.right_span.task].n_cigar;
			slot_off[j++ + 1] = n;
		}
	});
	slot_off[0] = 0;
	for (int64_t j = 0; j < plan0.back(); ++j) slot_off[j + 1] += slot_off[j];
}

// step (a) through the shared core on the host: a team of one per plan
static void spans_assemble_model(mpa_batch_s *b, const mpa_dp_rst_t *rst2, const uint32_t *pool2)
{
	std::vector<int64_t> plan0, seg0;
	spans_counts(b, plan0, seg0);
	std::vector<SpansPlan> plan((size_t)plan0.back());
	std::vector<SegRec> seg((size_t)seg0.back() + 1);
	spans_flatten(b, plan0, seg0, plan.data(), seg.data());
	std::vector<int64_t> slot((size_t)plan0.back() + 1);
	spans_slots(b, plan0, rst2, slot.data());
	std::atomic<bool> bad(false);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		std::vector<uint32_t> out;
		int64_t j = plan0[qi];
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			out.assign((size_t)(slot[j + 1] - slot[j]) + 1, 0);
			const AsmRec A = spans_assemble<SpansSerial>(plan[j], span_rec_of(pl, r), seg.data(), b->sp_rst1.data(), b->sp_pool1, rst2, pool2, out.data());
			if (A.bad) bad = true;
			asm_apply(pl, r, A, out.data(), rst2);
			++j;
		}
	});
	if (bad) spans_assemble_host(b, rst2, pool2);        // (a DP call whose own words would merge: the host's word-by-word join)
}

// step (a) on the device.  MPA_OK: done; MPA_ERR_UNSUPPORTED: the device declined and nothing was changed
static int spans_assemble_device(mpa_batch_s *b, mpa_ctx_t *ctx, const mpa_dp_rst_t *rst2)
{
	std::vector<int64_t> plan0, seg0;
	spans_counts(b, plan0, seg0);
	const int64_t n_plan = plan0.back(), n_rst2 = (int64_t)b->tasks.size();
	SpansAsmIO io;
	// (tests) MPA_TEST_ROUND2_DECLINE=1: the step declines behind a resident round 2, so that the late fetch of its pool is taken
	if (b->r2_resident) { const char *e = getenv("MPA_TEST_ROUND2_DECLINE"); if (e && atoi(e) != 0) { set_error("MPA_TEST_ROUND2_DECLINE"); return MPA_ERR_UNSUPPORTED; } }
	int rc = dev_spans_asm_stage(ctx, n_plan, n_rst2, io);
	if (rc != MPA_OK) return rc;
	const mpa_dp_rst_t *d_rst2 = b->r2_resident ? b->r2_rst_dev : nullptr;   // (a resident round 2: the records are read where its kernels wrote them)
	if (n_rst2 > 0 && !d_rst2) memcpy(io.rst2, rst2, (size_t)n_rst2 * sizeof(mpa_dp_rst_t));
	spans_slots(b, plan0, rst2, io.slot_off);
	rc = dev_spans_assemble(ctx, n_plan, n_rst2, nullptr, rst2 ? b->dp_n_pool : 0, io, d_rst2);
	if (rc != MPA_OK) return rc;
	for (int64_t j = 0; j < n_plan; ++j)
		if (io.rec[j].bad) { set_error("GPU spans: a DP call whose own CIGAR words would merge"); return MPA_ERR_UNSUPPORTED; }
	b->sp_cig_off.resize((size_t)n_plan);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		int64_t j = plan0[qi];
		for (AlignPlan &pl : qs.plans) {
			asm_apply(pl, qs.regs[pl.reg], io.rec[j], io.cigar + io.rec[j].cig_off, rst2);
			b->sp_cig_off[(size_t)j] = io.rec[j].cig_off;
			++j;
		}
	});
	return MPA_OK;
}

// MPA_SPANS_DUMP=<file> (diagnostics; the tests' view of the two steps): what they left in every query's state, appended batch after
// batch in query and plan order before stage_finish reorders the regions, whichever path produced it.  Per query: int32 qid, plans.
// Per plan 184 bytes -- int32 l_nt, l_aa, r_nt, r_aa, flags (1 left span, 2 right span, 4 / 8 the left / right
// terminal-exon repeat counted, 16 a segment boundary merged), qs, qe, dp_score, n_exon, n_cigar; int64 vs,
// ve; the left and the right span segment (24 bytes each: int32 ne0, ne1, ae0, ae1, task, score; zeros with task -1 for a right span
// that was not made); their round-2 task records (mpa_dp_task_t, 40 bytes each; zeros for a shortcut) -- then the n_cigar words.
// Layout and parser: tests/spansdump.py
static void spans_dump(const mpa_batch_s *b)
{
	if (!spans_dump_on()) return;
	static std::mutex mu;                                // (batches of a stream finish side by side: one writer at a time)
	std::lock_guard<std::mutex> g(mu);
	FILE *fp = fopen(getenv("MPA_SPANS_DUMP"), "ab");
	if (!fp) return;
	for (const QueryState &qs : b->qs) {
		const int32_t head[2] = { qs.qid, (int32_t)qs.plans.size() };
		fwrite(head, 4, 2, fp);
		for (const AlignPlan &pl : qs.plans) {
			const Region &r = qs.regs[pl.reg];
			const SpanRec R = span_rec_of(pl, r);
			const int32_t w[10] = { R.l_nt, R.l_aa, R.r_nt, R.r_aa, R.flags | (pl.n_merged > 0 ? 16 : 0), r.qs, r.qe, r.dp_score, r.n_exon, (int32_t)r.cigar.size() };
			const int64_t v[2] = { r.vs, r.ve };
			mpa_dp_task_t t[2];
			memset(t, 0, sizeof t);
			if (R.left.task >= 0 && (size_t)R.left.task < b->tasks.size()) t[0] = b->tasks[(size_t)R.left.task];
			if (R.right.task >= 0 && (size_t)R.right.task < b->tasks.size()) t[1] = b->tasks[(size_t)R.right.task];
			fwrite(w, 4, 10, fp), fwrite(v, 8, 2, fp), fwrite(&R.left, sizeof(SegRec), 1, fp), fwrite(&R.right, sizeof(SegRec), 1, fp), fwrite(t, sizeof(mpa_dp_task_t), 2, fp);
			if (!r.cigar.empty()) fwrite(r.cigar.data(), 4, r.cigar.size(), fp);
		}
	}
	fclose(fp);
}

static int take_round3_steps(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	struct Fetched { uint32_t *p = nullptr; ~Fetched() { free(p); } } fetched;   // (a resident round 2's pool, when a fallback needs its words)
	const StepMode mode = batch_step_mode(b, "MPA_GPU_STATS");
	const StepMode cs = cs_printed(b->opt) ? batch_step_mode(b, "MPA_GPU_CS") : STEP_HOST;
	const StepMode rows = rows_printed(b->opt) ? batch_step_mode(b, "MPA_GPU_ROWS") : STEP_HOST;
	const StepMode fin = (b->opt.flag & MPA_MF_NO_ALIGN) ? STEP_HOST : batch_step_mode(b, "MPA_GPU_FINISH");
	b->flat.reset(), b->flat_cs_src = 0;
	// MPA_GPU_FORMAT=1: the text behind the finish step of the same device call, for a batch whose names the stream
	// pipeline handed over.  It needs the finish step on the device, and the cs strings and rows the options print from their device walks
	const bool fmt_asked = b->fmt_names && !(b->opt.flag & MPA_MF_NO_ALIGN) && format_knob() == 1;
	if (mode == STEP_HOST && cs == STEP_HOST && rows == STEP_HOST && fin == STEP_HOST && b->spans_src == 0 && !spans_dump_on()) {   // the three steps in one pass over the queries
		if (fmt_asked && timing_on()) fprintf(stderr, "[mpa-timing] format declined (the finish step does not run on the device)\n");
		parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
			QueryState &qs = b->qs[qi];
			for (AlignPlan &pl : qs.plans) {
				Region &r = qs.regs[pl.reg];
				assemble_alignment(pl, r, rst, pool);
				stats_on_host(b, qs, pl, r);
			}
			stage_finish(b, qs);
		});
		return MPA_OK;
	}
	b->sp_cig_off.clear();
	bool any_plan = false;
	for (const QueryState &qs : b->qs) any_plan = any_plan || !qs.plans.empty();
	if (b->spans_src == 0 || !any_plan) parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {      // (a)
		QueryState &qs = b->qs[qi];
		for (AlignPlan &pl : qs.plans) {
			Region &r = qs.regs[pl.reg];
			assemble_alignment(pl, r, rst, pool);
			r.n_exon = count_exons(r);
		}
	});
	else if (b->spans_src == 1) {                                          // (a) through the shared core: round 1 left no gap words in the plans
		const double t1 = now_ms();
		spans_assemble_model(b, rst, pool);
		timing_note("spans: shared core", now_ms() - t1);
	} else {                                                               // (a) on the device
		const double t1 = now_ms();
		const int rc = b->dp_ctx ? spans_assemble_device(b, b->dp_ctx, rst) : MPA_ERR_UNSUPPORTED;
		if (rc == MPA_OK) timing_note("spans on the GPU", now_ms() - t1);
		else if (rc != MPA_ERR_UNSUPPORTED) return rc;
		else {
			if (timing_on()) fprintf(stderr, "[mpa-timing]   device spans declined (%s): region CIGARs on the host\n", mpa_last_error());
			b->sp_cig_off.clear();
			if (b->r1_resident && !b->sp_pool1) {                              // (MPA_GPU_ROUND1=1) round 1's words never came down: they are in the spans step's pool, a wait of its own
				const double t2 = now_ms();
				const int rc1 = dp_fetch_pool1(b->dp_ctx, b->r1_n_pool, &b->sp_pool1);
				if (rc1 != MPA_OK) return rc1;
				if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: round 1 resident: pool fetched late, %lld bytes down, %.3f ms\n", (long long)(4 * b->r1_n_pool), now_ms() - t2);
			}
			if (b->r2_resident && !pool) {                                     // the words of round 2 are still on the device: a second wait, their size is known by now
				const double t2 = now_ms();
				const int rc2 = dp_fetch_pool(b->dp_ctx, b->dp_n_pool, &fetched.p);
				if (rc2 != MPA_OK) return rc2;
				pool = fetched.p;
				if (timing_on()) fprintf(stderr, "[mpa-timing]   dp: round 2 resident: pool fetched late, %lld bytes down, %.3f ms\n", (long long)(4 * b->dp_n_pool), now_ms() - t2);
			}
			spans_assemble_host(b, rst, pool);
		}
	}
	// (b) the walks over the finished alignments.  They do not read each other's output (the statistics write scalars and features; cs
	// strings and rows read the CIGAR and the job record), so those whose knob is 1 share ONE device call -- one upload of jobs, CIGAR
	// words and text, one wait -- and every other one runs on its own: the statistics on the host or through their model, cs strings
	// and rows through their model or not at all (the formatter builds them).  A call the device declines leaves its walks to the host.
	static const struct { const char *name, *note, *left; } kWalk[3] = {
		{ "alignment statistics", "alignment statistics on the GPU", "statistics on the host" },
		{ "cs strings", "cs strings on the GPU", "the formatter builds them" },
		{ "residue rows", "residue rows on the GPU", "the formatter builds them" } };
	const bool on_dev[3] = { mode == STEP_DEVICE, cs == STEP_DEVICE, rows == STEP_DEVICE };
	bool stats_host = mode == STEP_HOST, stats_dev_ok = on_dev[0];
	std::string fin_why, fmt_why;
	const bool fin_possible = fin == STEP_DEVICE && on_dev[0] && cs != STEP_MODEL && rows != STEP_MODEL;
	const char *fmt_pre = !fmt_asked ? nullptr : !fin_possible ? "the finish step does not run on the device" : cs_printed(b->opt) && cs != STEP_DEVICE ? "cs strings are printed and MPA_GPU_CS is not 1" :
	                      rows_printed(b->opt) && rows != STEP_DEVICE ? "residue rows are printed and MPA_GPU_ROWS is not 1" : nullptr;
	if (on_dev[0] || on_dev[1] || on_dev[2]) {
		const double t0 = now_ms();
		bool ran = false;
		const int rc = walks_on_device(b, b->dp_ctx, on_dev[0], on_dev[1], on_dev[2], &ran, fin_possible, &fin_why, fmt_asked && !fmt_pre, &fmt_why);
		if (rc != MPA_OK && rc != MPA_ERR_UNSUPPORTED) return rc;
		for (int k = 0; k < 3; ++k) {
			if (!on_dev[k]) continue;
			if (rc == MPA_OK && ran) timing_note(kWalk[k].note, now_ms() - t0);      // (one call: the same span)
			if (rc != MPA_OK && timing_on()) fprintf(stderr, "[mpa-timing]   device %s declined (%s): %s\n", kWalk[k].name, mpa_last_error(), kWalk[k].left);
		}
		if (rc != MPA_OK && on_dev[0]) stats_host = true, stats_dev_ok = false;
	}
	if (stats_host) parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		for (AlignPlan &pl : qs.plans) stats_on_host(b, qs, pl, qs.regs[pl.reg]);
	});
	auto through_model = [&](StepMode m, void (*walk)(mpa_batch_s*), const char *note) {
		if (m != STEP_MODEL) return;
		const double t1 = now_ms();
		walk(b);
		timing_note(note, now_ms() - t1);
	};
	through_model(mode, stats_model, "alignment statistics: shared core");
	through_model(cs, cs_model, "cs strings: shared core");                // (b')
	through_model(rows, rows_model, "residue rows: shared core");          // (b'')
	spans_dump(b);
	// (c) MPA_GPU_FINISH.  1: the step ran inside walks_on_device, behind the walks' kernels and in front of their
	// one wait, and left b->flat -- it needs the statistics on the device in that call (dp_max is theirs, and so are the records it
	// reads); declined, the ranking is stage_finish's, with the same result.  model: the shared core on the host (host_finish.cpp).
	// (flat_cs_src is one value per batch: a batch's walks all take one path, so its carried cs bodies have one source)
	if (fmt_asked && !(b->flat && b->flat->fmt_n_out >= 0) && timing_on()) {
		bool any = false;
		for (const QueryState &qs : b->qs) any = any || !qs.plans.empty();
		const char *why = fmt_pre ? fmt_pre : !fmt_why.empty() ? fmt_why.c_str() : !b->flat ? (any ? "the finish step did not run on the device" : "no aligned region in the batch") : "the device call declined";
		fprintf(stderr, "[mpa-timing] format declined (%s)\n", why);
	}
	if (b->flat) return MPA_OK;
	if (fin == STEP_DEVICE) {
		bool any = false;
		for (const QueryState &qs : b->qs) any = any || !qs.plans.empty();
		const char *why = mode != STEP_DEVICE ? "MPA_GPU_STATS is not 1" : !stats_dev_ok ? "the device statistics declined" : cs == STEP_MODEL || rows == STEP_MODEL ? "a walk runs through its model" : !fin_why.empty() ? fin_why.c_str() : nullptr;
		if (any && why && timing_on()) fprintf(stderr, "[mpa-timing]   finish declined (%s): ranking and flatten on the host\n", why);
	} else if (fin == STEP_MODEL && batch_finish_model(b)) {
		for (const QueryState &qs : b->qs) for (const Region &r : qs.regs) if (r.aligned && r.cs_src) b->flat_cs_src = r.cs_src;
		return MPA_OK;
	}
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) { stage_finish(b, b->qs[qi]); });   // (c)
	return MPA_OK;
}

// MPA_OK, or the error of a device call that failed (a call that merely declines leaves the batch to the host walk)
int take_round3(mpa_batch_s *b, const mpa_dp_rst_t *rst, const uint32_t *pool)
{
	const int rc = take_round3_steps(b, rst, pool);
	if (rc == MPA_OK) cs_dump(b);
	return rc;
}

} // namespace mpa
