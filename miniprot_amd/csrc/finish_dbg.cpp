// finish_dbg.cpp -- mpa_dbg_finish, mpa_dbg_finish_last and mpa_dbg_result_flat (include/mpamd_dbg.h), the test hooks of MPA_GPU_FINISH:
// hand-made tables of aligned regions through the ranking and the layout of DESIGN.md section 4.13, on the device (dev_finish of
// stats_run.hip) or through the shared core on the host (finish_core.h), and a result's flat arrays as bytes.  Part of libmpamd_dbg.so.
#include <cstring>
#include <memory>
#include "mpa_internal.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

extern "C" {

static int mpa_dbg_finish_impl(mpa_ctx_t *ctx, const mpa_mapopt_t *opt, int32_t kmer, int32_t n_query, const int64_t *first, const void *recs, const uint32_t *words, int64_t n_words,
                               const mpa_feat_t *feats, int64_t n_feat, const char *cs_text, int64_t cs_bytes, const char *rows_text, int64_t rows_bytes, mpa_result_t **out)
{
	if (out) *out = nullptr;
	if (!opt || n_query <= 0 || !first || !out || n_words < 0 || n_feat < 0 || cs_bytes < 0 || rows_bytes < 0 || first[0] != 0 || first[n_query] < 0 || (first[n_query] > 0 && !recs) ||
	    (n_words > 0 && !words) || (n_feat > 0 && !feats) || (cs_bytes > 0 && !cs_text) || (rows_bytes > 0 && !rows_text)) { set_error("mpa_dbg_finish: missing arguments"); return MPA_ERR_ARG; }
	const FinRec *rec = (const FinRec*)recs;
	FinishSizes z{};
	z.n_query = n_query, z.n_rec = first[n_query], z.in_words = n_words, z.in_feat = n_feat, z.in_cs = cs_bytes, z.in_rows = rows_bytes;
	for (int32_t q = 0; q < n_query; ++q) if (first[q + 1] < first[q] || first[q + 1] > z.n_rec) { set_error("mpa_dbg_finish: first[] is not ascending"); return MPA_ERR_ARG; }
	z.n_big = finish_count_big(first, n_query);
	for (int64_t i = 0; i < z.n_rec; ++i) z.out_words += rec[i].n_cigar, z.out_feat += rec[i].n_feat, z.out_cs += rec[i].cs_len > 0 ? rec[i].cs_len : 0, z.out_rows += finish_rows_bytes(rec[i]);
	FinishTables t;
	t.first = const_cast<int64_t*>(first), t.rec = const_cast<FinRec*>(rec), t.words = const_cast<uint32_t*>(words), t.feats = const_cast<mpa_feat_t*>(feats);
	t.cs_text = const_cast<char*>(cs_text), t.rows_text = const_cast<char*>(rows_text);
	if (!finish_tables_ok(z, t)) { set_error("mpa_dbg_finish: a record that points outside its arrays"); return MPA_ERR_ARG; }
	const FinParams p{ kmer, opt->mask_len, opt->best_n, opt->io, opt->mask_level, opt->pri_ratio };
	std::unique_ptr<mpa_result_s> res(new mpa_result_s());
	if (!ctx || z.n_rec == 0) finish_model(p, z, t, res.get());      // (a table without regions launches nothing)
	else {
		FinishTables up;
		int rc = dev_finish_stage(ctx, z, up);
		if (rc != MPA_OK) return rc;
		memcpy(up.first, first, ((size_t)n_query + 1) * 8), memcpy(up.rec, rec, (size_t)z.n_rec * sizeof(FinRec));
		if (n_words > 0) memcpy(up.words, words, (size_t)n_words * 4);
		if (n_feat > 0) memcpy(up.feats, feats, (size_t)n_feat * sizeof(mpa_feat_t));
		if (cs_bytes > 0) memcpy(up.cs_text, cs_text, (size_t)cs_bytes);
		if (rows_bytes > 0) memcpy(up.rows_text, rows_text, (size_t)rows_bytes);
		FinishFlat flat;
		if ((rc = dev_finish(ctx, p, z, flat)) != MPA_OK) return rc;
		finish_flat_to_result(flat, n_query, res.get());
	}
	*out = res.release();
	return MPA_OK;
}

int mpa_dbg_finish(mpa_ctx_t *ctx, const mpa_mapopt_t *opt, int32_t kmer, int32_t n_query, const int64_t *first, const void *recs, const uint32_t *words, int64_t n_words,
                   const mpa_feat_t *feats, int64_t n_feat, const char *cs_text, int64_t cs_bytes, const char *rows_text, int64_t rows_bytes, mpa_result_t **out)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_dbg_finish_impl(ctx, opt, kmer, n_query, first, recs, words, n_words, feats, n_feat, cs_text, cs_bytes, rows_text, rows_bytes, out); });
}

int mpa_dbg_finish_last(const mpa_ctx_t *ctx, int64_t out[MPA_DBG_FINISH_REC]) { return dev_finish_last(ctx, out); }

int64_t mpa_dbg_result_flat(const mpa_result_t *r, int32_t which, void *buf, int64_t cap)
{
	if (!r) { set_error("mpa_dbg_result_flat: no result"); return MPA_ERR_ARG; }
	const void *src = nullptr;
	int64_t bytes = 0;
	switch (which) {
	case MPA_DBG_FLAT_HITS: src = r->hits.data(), bytes = (int64_t)(r->hits.size() * sizeof(mpa_hit_t)); break;
	case MPA_DBG_FLAT_HIT_OFF: src = r->hit_off.data(), bytes = (int64_t)(r->hit_off.size() * 8); break;
	case MPA_DBG_FLAT_CIGARS: src = r->cigars.data(), bytes = (int64_t)(r->cigars.size() * 4); break;
	case MPA_DBG_FLAT_FEATS: src = r->feats.data(), bytes = (int64_t)(r->feats.size() * sizeof(mpa_feat_t)); break;
	case MPA_DBG_FLAT_CS_TEXT: src = r->cs_text.data(), bytes = (int64_t)r->cs_text.size(); break;
	case MPA_DBG_FLAT_ROWS_TEXT: src = r->rows_text.data(), bytes = (int64_t)r->rows_text.size(); break;
	case MPA_DBG_FLAT_CS: bytes = (int64_t)(r->cs.size() * sizeof(FinCsRef)); break;
	case MPA_DBG_FLAT_ROWS: bytes = (int64_t)(r->rows.size() * sizeof(FinRowsRef)); break;
	default: set_error("mpa_dbg_result_flat: no such array"); return MPA_ERR_ARG;
	}
	if (!buf || bytes > cap) return bytes;
	if (which == MPA_DBG_FLAT_CS) {                          // (field by field: the padding of the result's own records is not defined)
		FinCsRef *d = (FinCsRef*)buf;
		for (size_t h = 0; h < r->cs.size(); ++h) d[h] = FinCsRef{ r->cs[h].off, r->cs[h].len, r->cs[h].present };
	} else if (which == MPA_DBG_FLAT_ROWS) {
		memset(buf, 0, (size_t)bytes);
		FinRowsRef *d = (FinRowsRef*)buf;
		for (size_t h = 0; h < r->rows.size(); ++h) d[h].off = r->rows[h].off, d[h].width = r->rows[h].width, d[h].n_sta = r->rows[h].n_sta, d[h].present = r->rows[h].present;
	} else if (bytes > 0) memcpy(buf, src, (size_t)bytes);
	return bytes;
}

} // extern "C"
