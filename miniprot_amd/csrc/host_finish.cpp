// host_finish.cpp -- MPA_GPU_FINISH: the final ranking of a batch's aligned regions and the layout of its flat
// result through finish_core.h, in place of stage_finish() (host_align.cpp) and the flatten loop of mpa_batch_finish() (host_map.cpp).
//   batch_finish_model()     MPA_GPU_FINISH=model: the batch's regions as the step's tables, the shared core with a team of one, and the
//                            flat result left with the batch (mpa_batch_s::flat)
//   finish_model()           the shared core on the host: rank per query, the counts' prefix, gather per kept hit
//   finish_flat_to_result()  a device call's arrays into a result, one copy each
//   finish_tables_ok()       every index the step follows (the test hook's tables)
#include <algorithm>
#include <cstring>
#include "host_batch.h"

namespace mpa {

bool finish_tables_ok(const FinishSizes &z, const FinishTables &t)
{
	if (z.n_query < 0 || z.n_rec < 0 || !t.first || t.first[0] != 0 || t.first[z.n_query] != z.n_rec) return false;
	for (int64_t q = 0; q < z.n_query; ++q) if (t.first[q + 1] < t.first[q] || t.first[q + 1] - t.first[q] > INT32_MAX) return false;
	if (finish_count_big(t.first, z.n_query) != z.n_big) return false;
	int64_t w = 0, f = 0, c = 0, r = 0;
	for (int64_t i = 0; i < z.n_rec; ++i) {
		const FinRec &x = t.rec[i];
		if (x.n_cigar < 0 || x.cig_off < 0 || x.cig_off + x.n_cigar > z.in_words || x.n_feat < 0 || x.feat_off < 0 || x.feat_off + x.n_feat > z.in_feat) return false;
		if (x.cs_len > 0 && (x.cs_off < 0 || x.cs_off + x.cs_len > z.in_cs)) return false;
		if (x.rows_stride >= 0 && (x.rows_w < 0 || x.rows_w > x.rows_stride || x.rows_sta < 0 || x.rows_w > (1 << 28) || x.rows_sta > (1 << 28) || x.rows_off < 0 ||
		                           x.rows_off + 4 * (int64_t)x.rows_stride + x.rows_sta > z.in_rows)) return false;
		w += x.n_cigar, f += x.n_feat, c += x.cs_len > 0 ? x.cs_len : 0, r += finish_rows_bytes(x);
	}
	return w == z.out_words && f == z.out_feat && c == z.out_cs && r == z.out_rows;
}

static void result_sized(mpa_result_s *res, int64_t n_query, const FinCounts &tot)
{
	res->n_seq = (int32_t)n_query;
	res->hit_off.resize((size_t)n_query + 1);
	res->hits.resize((size_t)tot.hit), res->cigars.resize((size_t)tot.cigar), res->feats.resize((size_t)tot.feat);
	res->cs.clear(), res->rows.clear(), res->cs_text.clear(), res->rows_text.clear();
	// (one entry per hit when any hit carries one, none at all otherwise: mpa_result_s)
	if (tot.n_cs > 0) res->cs.resize((size_t)tot.hit), res->cs_text.resize((size_t)tot.cs);
	if (tot.n_rows > 0) res->rows.resize((size_t)tot.hit), res->rows_text.resize((size_t)tot.rows);
}

static void refs_into(mpa_result_s *res, const FinCsRef *cs, const FinRowsRef *rows)
{
	for (size_t h = 0; h < res->cs.size(); ++h) res->cs[h] = mpa_result_s::CsRef{ cs[h].off, cs[h].len, cs[h].present };
	for (size_t h = 0; h < res->rows.size(); ++h) res->rows[h] = mpa_result_s::RowsRef{ rows[h].off, rows[h].width, rows[h].n_sta, rows[h].present };
}

void finish_flat_to_result(const FinishFlat &f, int64_t n_query, mpa_result_s *res)
{
	const FinCounts &tot = f.off[n_query];
	result_sized(res, n_query, tot);
	for (int64_t q = 0; q <= n_query; ++q) res->hit_off[(size_t)q] = f.off[q].hit;
	if (tot.hit > 0) memcpy(res->hits.data(), f.hits, (size_t)tot.hit * sizeof(mpa_hit_t));
	if (tot.cigar > 0) memcpy(res->cigars.data(), f.cigars, (size_t)tot.cigar * 4);
	if (tot.feat > 0) memcpy(res->feats.data(), f.feats, (size_t)tot.feat * sizeof(mpa_feat_t));
	if (!res->cs_text.empty()) memcpy(&res->cs_text[0], f.cs_text, res->cs_text.size());
	if (!res->rows_text.empty()) memcpy(&res->rows_text[0], f.rows_text, res->rows_text.size());
	refs_into(res, f.cs, f.rows);
}

void finish_model(const FinParams &p, const FinishSizes &z, const FinishTables &t, mpa_result_s *res)
{
	const int64_t nq = z.n_query;
	std::vector<FinOut> out((size_t)z.n_rec + 1);
	std::vector<FinCounts> cnt((size_t)nq + 1), off((size_t)nq + 1);
	{
		std::vector<FinRank> tmp, r;
		std::vector<Pair64> key;
		std::vector<SortRange> stack;
		std::vector<uint32_t> hist(768);
		std::vector<int32_t> prim;
		std::vector<uint64_t> cov;
		int32_t ctl[2];
		for (int64_t q = 0; q < nq; ++q) {
			const int64_t f = t.first[q];
			const int32_t n = (int32_t)(t.first[q + 1] - f);
			const size_t m = (size_t)n + 1;
			tmp.resize(m), r.resize(m), key.resize(m), stack.resize((size_t)FINISH_STACK(n)), prim.resize(m), cov.resize(m);
			const FinScratch S{ tmp.data(), r.data(), key.data(), stack.data(), hist.data(), prim.data(), cov.data(), ctl };
			finish_rank_core<FinishSerial>(p, t.rec + f, n, S, out.data() + f, &cnt[(size_t)q]);
		}
	}
	finish_scan_serial(cnt.data(), nq, off.data());
	const FinCounts tot = off[(size_t)nq];
	result_sized(res, nq, tot);
	std::vector<FinCsRef> cs((size_t)tot.hit + 1);
	std::vector<FinRowsRef> rows((size_t)tot.hit + 1);
	std::string cs_text((size_t)tot.cs, '\0'), rows_text((size_t)tot.rows, '\0');
	const FinDst dst{ res->hits.data(), res->cigars.data(), res->feats.data(), cs.data(), &cs_text[0], rows.data(), &rows_text[0] };
	for (int64_t q = 0; q < nq; ++q) {
		const int64_t f = t.first[q];
		const FinCounts &at = off[(size_t)q];
		res->hit_off[(size_t)q] = at.hit;
		for (int64_t j = 0; j < cnt[(size_t)q].hit; ++j) {
			const FinOut &o = out[(size_t)(f + j)];
			finish_gather_core<FinishSerial>((int32_t)q, t.rec[f + o.src], o, at.hit + j, at, t.words, t.feats, t.cs_text, t.rows_text, dst);
		}
	}
	res->hit_off[(size_t)nq] = tot.hit;
	if (!res->cs_text.empty()) res->cs_text.swap(cs_text);
	if (!res->rows_text.empty()) res->rows_text.swap(rows_text);
	refs_into(res, cs.data(), rows.data());
}

// MPA_GPU_FINISH=model for a batch behind its walks: the regions flattened into the step's tables, the shared core with a team of one.
// true: b->flat holds the batch's result and the regions were left as they were; false: there was nothing to rank -- the caller runs
// stage_finish.  (On the device the step runs inside the walks' call, walks_on_device of host_align.cpp, and reads no Region.)
bool batch_finish_model(mpa_batch_s *b)
{
	const size_t nq = b->qs.size();
	if (nq == 0) return false;
	const double t0 = now_ms();
	std::vector<FinishSizes> per(nq + 1);                    // (per query, then their prefix: n_rec, in_* as running offsets)
	parallel_for(b->n_threads, (int64_t)nq, [&](int64_t qi) {
		FinishSizes s{};
		for (const Region &r : b->qs[qi].regs) {
			if (!r.aligned) continue;
			++s.n_rec, s.in_words += (int64_t)r.cigar.size(), s.in_feat += (int64_t)r.feat.size();
			if (r.cs_src) s.in_cs += (int64_t)r.cs.size();
			if (r.rows_src) s.in_rows += (int64_t)r.rows.size();
		}
		per[(size_t)qi + 1] = s;
	});
	per[0] = FinishSizes{};
	FinishSizes z{};
	for (size_t q = 0; q < nq; ++q) {
		FinishSizes &a = per[q + 1];
		z.n_big += a.n_rec > FINISH_LDS_REGS;
		a.n_rec += per[q].n_rec, a.in_words += per[q].in_words, a.in_feat += per[q].in_feat, a.in_cs += per[q].in_cs, a.in_rows += per[q].in_rows;
	}
	z.n_query = (int64_t)nq, z.n_rec = per[nq].n_rec, z.in_words = z.out_words = per[nq].in_words, z.in_feat = z.out_feat = per[nq].in_feat;
	z.in_cs = z.out_cs = per[nq].in_cs, z.in_rows = z.out_rows = per[nq].in_rows;
	if (z.n_rec == 0) return false;
	FinishTables t;
	std::vector<int64_t> v_first;
	std::vector<FinRec> v_rec;
	std::vector<uint32_t> v_words;
	std::vector<mpa_feat_t> v_feats;
	std::string v_cs, v_rows;
	v_first.resize(nq + 1), v_rec.resize((size_t)z.n_rec), v_words.resize((size_t)z.in_words + 1), v_feats.resize((size_t)z.in_feat + 1), v_cs.resize((size_t)z.in_cs + 1), v_rows.resize((size_t)z.in_rows + 1);
	t.first = v_first.data(), t.rec = v_rec.data(), t.words = v_words.data(), t.feats = v_feats.data(), t.cs_text = &v_cs[0], t.rows_text = &v_rows[0];
	t.first[nq] = z.n_rec;
	parallel_for(b->n_threads, (int64_t)nq, [&](int64_t qi) {
		const FinishSizes &at = per[(size_t)qi];
		int64_t i = at.n_rec, w = at.in_words, f = at.in_feat, c = at.in_cs, rw = at.in_rows;
		t.first[qi] = i;
		for (const Region &r : b->qs[qi].regs) {
			if (!r.aligned) continue;
			FinRec &x = t.rec[i++];
			memset(&x, 0, sizeof x);
			x.vs = r.vs, x.ve = r.ve, x.cig_off = w, x.feat_off = f, x.vid = r.vid, x.hash = r.hash, x.qs = r.qs, x.qe = r.qe, x.cnt = r.cnt, x.n_exon = r.n_exon;
			x.chn_sc = r.chn_sc, x.chn_sc_ungap = r.chn_sc_ungap, x.parent = r.parent, x.n_sub = r.n_sub, x.subsc = r.subsc, x.dp_max2 = r.dp_max2;
			x.dp_score = r.dp_score, x.dp_max = r.dp_max, x.blen = r.blen, x.n_fs = r.n_fs, x.n_stop = r.n_stop, x.dist_stop = r.dist_stop, x.dist_start = r.dist_start;
			x.n_iden = r.n_iden, x.n_plus = r.n_plus, x.n_cigar = (int32_t)r.cigar.size(), x.n_feat = (int32_t)r.feat.size();
			if (!r.cigar.empty()) memcpy(t.words + w, r.cigar.data(), r.cigar.size() * 4);
			w += (int64_t)r.cigar.size();
			for (const Feat &s : r.feat) {
				mpa_feat_t &o = t.feats[f++];
				memset(&o, 0, sizeof o);
				o.vs = s.vs, o.ve = s.ve, o.qs = s.qs, o.qe = s.qe, o.type = s.type, o.phase = s.phase, o.n_fs = s.n_fs, o.n_stop = s.n_stop, o.score = s.score, o.n_iden = s.n_iden, o.blen = s.blen;
				memcpy(o.donor, s.donor, 2), memcpy(o.acceptor, s.acceptor, 2);
			}
			x.cs_len = -1, x.rows_stride = -1;
			if (r.cs_src) {
				x.cs_off = c, x.cs_len = (int32_t)r.cs.size();
				if (!r.cs.empty()) memcpy(t.cs_text + c, r.cs.data(), r.cs.size());
				c += (int64_t)r.cs.size();
			}
			if (r.rows_src) {                                  // (closed up already: rows_apply)
				x.rows_off = rw, x.rows_w = x.rows_stride = r.rows_w, x.rows_sta = r.rows_sta;
				if (!r.rows.empty()) memcpy(t.rows_text + rw, r.rows.data(), r.rows.size());
				rw += (int64_t)r.rows.size();
			}
		}
	});
	const FinParams p{ b->mi->opt.kmer, b->opt.mask_len, b->opt.best_n, b->opt.io, b->opt.mask_level, b->opt.pri_ratio };
	std::unique_ptr<mpa_result_s> res(new mpa_result_s());
	finish_model(p, z, t, res.get());
	timing_note("finish: shared core", now_ms() - t0);
	b->flat = std::move(res);
	return true;
}

} // namespace mpa
