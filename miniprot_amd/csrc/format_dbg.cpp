// format_dbg.cpp -- mpa_dbg_format, mpa_dbg_format_last, mpa_dbg_result_make and mpa_dbg_idx_names (include/mpamd_dbg.h), the test hooks
// of MPA_GPU_FORMAT: a result's output text through the three stages of DESIGN.md section 4.14, on the device (dev_format of
// stats_run.hip) or through the shared core on the host (format_core.h), and hand-made results and name-only indexes to run them on.
// Part of libmpamd_dbg.so.
#include <cstring>
#include <memory>
#include "mpa_internal.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

extern "C" {

static int mpa_dbg_format_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, const char *const *names, const mpa_result_t *r, int64_t id0,
                               char **text, int64_t *len, int64_t *n_out)
{
	if (text) *text = nullptr;
	if (!mi || !opt || !q || !names || !r || !text || !len || !n_out || q->n_seq <= 0 || (int64_t)r->hit_off.size() != (int64_t)q->n_seq + 1 || mi->ctg.empty()) {
		set_error("mpa_dbg_format: missing arguments");
		return MPA_ERR_ARG;
	}
	FmtOpt o;
	FormatInput in;
	const char *why = nullptr;
	std::string body;
	FmtCounts tot{ 0, 0, 0, 0 };
	if (!format_opt_from(*opt, o)) why = "a gff_prefix longer than 64 bytes";
	else {
		format_input(mi, *opt, q, names, r, ctx == nullptr, in);
		if (!format_tables_ok(in)) { set_error("mpa_dbg_format: a hit that points outside its arrays"); return MPA_ERR_ARG; }
		std::vector<int64_t> id_at;
		if (!ctx) {
			FormatText t;
			if (!(why = format_host(o, in, t))) body.swap(t.text), id_at.swap(t.id_at), tot = t.tot;
		} else {
			format_bounds(o, in);
			const FormatSizes &z = in.z;
			FormatTables up;
			int rc = dev_format_stage(ctx, z, up);
			if (rc != MPA_OK) return rc;
			const size_t nq = (size_t)z.n_query, nh = (size_t)z.n_hit, nc = (size_t)z.n_ctg;
			memcpy(up.hit_off, in.S.hit_off, (nq + 1) * 8), memcpy(up.q_off, in.S.q_off, (nq + 1) * 8), memcpy(up.qname_off, in.S.qname_off, (nq + 1) * 8);
			memcpy(up.cname_off, in.S.cname_off, (nc + 1) * 8), memcpy(up.clen, in.S.clen, nc * 8);
			if (nh) memcpy(up.hits, in.S.hits, nh * sizeof(mpa_hit_t));
			if (z.has_cs) memcpy(up.cs, in.S.cs, nh * sizeof(FinCsRef));
			if (z.has_rows) memcpy(up.rows, in.S.rows, nh * sizeof(FinRowsRef));
			if (z.n_feat) memcpy(up.feats, in.S.feats, (size_t)z.n_feat * sizeof(mpa_feat_t));
			if (z.n_words) memcpy(up.cigars, in.S.cigars, (size_t)z.n_words * 4);
			if (z.cs_bytes) memcpy(up.cs_text, in.S.cs_text, (size_t)z.cs_bytes);
			if (z.rows_bytes) memcpy(up.rows_text, in.S.rows_text, (size_t)z.rows_bytes);
			if (z.qname_bytes) memcpy(up.qname, in.S.qname, (size_t)z.qname_bytes);
			if (z.cname_bytes) memcpy(up.cname, in.S.cname, (size_t)z.cname_bytes);
			FormatOut out;
			if ((rc = dev_format(ctx, o, z, out)) != MPA_OK) return rc;
			tot = out.tot;
			if (out.declined) why = format_decline_reason(out.tot, z.text_cap, z.id_cap);
			else body.assign(out.text, (size_t)tot.bytes), id_at.assign(out.id_at, out.id_at + tot.ids);
		}
		if (!why && !format_patch_ids(&body[0], id_at.data(), tot.ids, tot.n_out, id0)) why = "ids reach seven digits";
	}
	if (why) {                                                   // declined: the host formatter's bytes, as the pipeline would give them
		if (timing_on()) fprintf(stderr, "[mpa-timing] format declined (%s)\n", why);
		int64_t id = id0;
		const int64_t n = mpa_format_output(mi, opt, q, names, r, &id, text);
		if (n < 0) return (int)n;
		*len = n, *n_out = id - id0;
		return MPA_DBG_FORMAT_DECLINED;
	}
	char *buf = (char*)malloc(body.size() + 1);
	if (!buf) { set_error("out of host memory"); return MPA_ERR_HIP; }
	memcpy(buf, body.data(), body.size());
	buf[body.size()] = 0;
	*text = buf, *len = (int64_t)body.size(), *n_out = tot.n_out;
	return MPA_OK;
}

int mpa_dbg_format(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, const char *const *names, const mpa_result_t *r, int64_t id0, char **text,
                   int64_t *len, int64_t *n_out)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return mpa_dbg_format_impl(ctx, mi, opt, q, names, r, id0, text, len, n_out); });
}

int mpa_dbg_format_last(const mpa_ctx_t *ctx, int64_t out[MPA_DBG_FORMAT_REC]) { return dev_format_last(ctx, out); }

int mpa_dbg_result_make(int32_t n_seq, const int64_t *hit_off, const mpa_hit_t *hits, const uint32_t *cigars, int64_t n_words, const mpa_feat_t *feats, int64_t n_feat, const void *cs,
                        const char *cs_text, int64_t cs_bytes, const void *rows, const char *rows_text, int64_t rows_bytes, mpa_result_t **out)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] {
		if (out) *out = nullptr;
		if (n_seq <= 0 || !hit_off || !out || hit_off[0] != 0 || hit_off[n_seq] < 0 || (hit_off[n_seq] > 0 && !hits) || n_words < 0 || n_feat < 0 || cs_bytes < 0 || rows_bytes < 0) {
			set_error("mpa_dbg_result_make: missing arguments");
			return MPA_ERR_ARG;
		}
		const size_t nh = (size_t)hit_off[n_seq];
		std::unique_ptr<mpa_result_s> res(new mpa_result_s());
		res->n_seq = n_seq;
		res->hit_off.assign(hit_off, hit_off + n_seq + 1);
		if (nh) res->hits.assign(hits, hits + nh);
		if (n_words) res->cigars.assign(cigars, cigars + n_words);
		if (n_feat) res->feats.assign(feats, feats + n_feat);
		if (cs) {
			const FinCsRef *c = (const FinCsRef*)cs;
			for (size_t h = 0; h < nh; ++h) res->cs.push_back(mpa_result_s::CsRef{ c[h].off, c[h].len, c[h].present });
			res->cs_text.assign(cs_text ? cs_text : "", (size_t)cs_bytes);
		}
		if (rows) {
			const FinRowsRef *w = (const FinRowsRef*)rows;
			for (size_t h = 0; h < nh; ++h) res->rows.push_back(mpa_result_s::RowsRef{ w[h].off, w[h].width, w[h].n_sta, w[h].present });
			res->rows_text.assign(rows_text ? rows_text : "", (size_t)rows_bytes);
		}
		*out = res.release();
		return MPA_OK;
	});
}

mpa_idx_t *mpa_dbg_idx_names(int32_t n_ctg, const char *const *names, const int64_t *lens)
{
	return mpa::guarded<mpa_idx_t*>(nullptr, [&]() -> mpa_idx_t* {
		if (n_ctg <= 0 || !names || !lens) { set_error("mpa_dbg_idx_names: missing arguments"); return nullptr; }
		std::unique_ptr<mpa_idx_s> mi(new mpa_idx_s());
		memset(&mi->opt, 0, sizeof mi->opt);
		int64_t off = 0;
		for (int32_t c = 0; c < n_ctg; ++c) mi->ctg.push_back(Contig{ off, lens[c], names[c] }), off += lens[c];
		mi->l_seq = off;
		return mi.release();
	});
}

} // extern "C"
