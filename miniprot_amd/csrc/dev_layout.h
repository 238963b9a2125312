// dev_layout.h -- the layouts of the device pools and pinned blocks whose element types a host compile sees (chain_core.h,
// regions_core.h, plans_core.h, aln_*_core.h, spans_core.h, mpamd.h): which pieces a block has, in which order, with which slack.
// Host-only like carve.h, so that tests/carve_check.cpp can hold every offset against plain arithmetic; the drivers build one per
// call and read the block through its pieces.  Layouts made of kernel-file types (the sift's segments, the refinement's windows and
// chunks, the device planner's scratch) stay in their unit.  A new piece: a member here, a take() at its place in the block, a line
// in carve_check.cpp.
#pragma once
#include "carve.h"
#include "mpa_internal.h"

namespace mpa {

// ---- the chain tail (seed_run.hip; x_all, 256-byte pieces)
// What one extraction works in and leaves: scratch indexed like the views (m entries; `ends` and `stack` have extras per problem),
// the per-problem status, the chains (out_a, out_u: m words each, placed by the route), their counts and the counts' prefixes.
struct ExtractCarve {
	Piece<int32_t> mark, order; Piece<Pair64> ends, tail8; Piece<SparseItem> items, moved, merged; Piece<uint8_t> kept; Piece<SortRange> stack; Piece<int32_t> status;
	Piece<uint64_t> out_a, out_u; Piece<int64_t> na, nu, offa, offu;
};
inline ExtractCarve carve_extract_scratch(Carve &cv, size_t m, size_t n_prob)   // mark .. status; the caller zeroes status and its 16 bytes of slack
{
	ExtractCarve c{};
	c.mark = cv.take<int32_t>(m), c.order = cv.take<int32_t>(m), c.ends = cv.take<Pair64>(m + 64 * n_prob + 64), c.tail8 = cv.take<Pair64>(m);
	// (the chain layout's scratch -- packed anchors, sorted u, first positions -- is only live after the sort replay and the
	// extraction: k_chain_extract puts it into the problem's own `moved` and `merged` lists)
	c.items = cv.take<SparseItem>(m), c.moved = cv.take<SparseItem>(m), c.merged = cv.take<SparseItem>(m);
	c.kept = cv.take<uint8_t>(m), c.stack = cv.take<SortRange>(m / 64 + 6 * n_prob + 16), c.status = cv.take<int32_t>(n_prob, 16);
	return c;
}
inline void carve_extract_counts(Carve &cv, size_t n_prob, ExtractCarve &c)    // na, nu, offa, offu
{
	c.na = cv.take<int64_t>(n_prob + 1), c.nu = cv.take<int64_t>(n_prob + 1), c.offa = cv.take<int64_t>(n_prob + 1, 8), c.offu = cv.take<int64_t>(n_prob + 1, 8);
}
// The forward pass (chain_fwd_launch, dev_ctx.h) over m anchors.  Its pieces: f, pred, mark, then the list of runs longer than
// serial_run and its counter (64 bytes, zeroed by the caller).  The routes that keep f / pred elsewhere (the direct route's view IS
// the forward pass's arrays; the refinement's run list lies behind its chains) take the run list alone, carve_chain_runs, and put
// the rest into the struct.  In block X it works on ChainFwdBufs; flag is the extraction's `mark`, which it only initialises.
struct ChainFwdBufs { int32_t *f, *pred, *mark; uint32_t *flag; LongRun *runs; unsigned int *n_runs; size_t long_cap; };
struct ChainFwdCarve {
	Piece<int32_t> f, pred, mark; Piece<LongRun> runs; Piece<unsigned int> n_runs;
	ChainFwdBufs in(void *X, const ExtractCarve &xc) const { return ChainFwdBufs{ f.in(X), pred.in(X), mark.in(X), xc.mark.sub<uint32_t>(0, xc.mark.n).in(X), runs.in(X), n_runs.in(X), runs.n }; }
};
inline void carve_chain_runs(Carve &cv, size_t m, int32_t serial_run, ChainFwdCarve &c) { c.runs = cv.take<LongRun>(m / (size_t)(serial_run + 1) + 16), c.n_runs = cv.take<unsigned int>(16); }
inline ChainFwdCarve carve_chain_fwd(Carve &cv, size_t m, int32_t serial_run)
{
	ChainFwdCarve c{};
	c.f = cv.take<int32_t>(m), c.pred = cv.take<int32_t>(m), c.mark = cv.take<int32_t>(m), carve_chain_runs(cv, m, serial_run, c);
	return c;
}

// k_regions' scratch and results in rg (T chains of NP problems), and what k_region_pack leaves in the holder's pinned block, packed
struct RegionsLayout {
	Piece<RegionRec> tmp, out, h_rec; Piece<uint64_t> ext, cov, h_ext; Piece<Pair64> key; Piece<SortRange> stack; Piece<uint32_t> hist; Piece<int32_t> prim, ctl, n_reg, h_nreg;
	size_t dev_bytes, pinned_bytes;
	RegionsLayout(size_t T, size_t NP) {
		Carve cv, h(1);
		tmp = cv.take<RegionRec>(T), out = cv.take<RegionRec>(T), ext = cv.take<uint64_t>(T), cov = cv.take<uint64_t>(T), key = cv.take<Pair64>(T);
		stack = cv.take<SortRange>(T / 64 + 5 * NP + 8), hist = cv.take<uint32_t>(NP * 768), prim = cv.take<int32_t>(T), ctl = cv.take<int32_t>(NP * 2), n_reg = cv.take<int32_t>(NP);
		h_rec = h.take<RegionRec>(T), h_ext = h.take<uint64_t>(T), h_nreg = h.take<int32_t>(NP);
		dev_bytes = cv.at + 256, pinned_bytes = h.at + 64;
	}
};
// k_plans' scratch and results in pl (T extracted anchors, NW windows, NQ queries), and k_plan_pack's pinned block, packed
struct PlansLayout {
	Piece<RegionRec> tmp, reg, h_reg; Piece<Pair64> key; Piece<SortRange> stack; Piece<uint32_t> hist; Piece<int32_t> prim, flag, list, ctl; Piece<uint64_t> cov, ext; Piece<int64_t> aoff;
	Piece<PlanRec> plan, h_plan; Piece<mpa_dp_task_t> task, h_task; Piece<SegRec> seg, h_seg; Piece<PlansCounts> cnt, h_cnt;
	size_t dev_bytes, pinned_bytes;
	PlansLayout(size_t T, size_t NW, size_t NQ) {
		Carve cv, h(1);
		tmp = cv.take<RegionRec>(NW), key = cv.take<Pair64>(NW), stack = cv.take<SortRange>(NW / 64 + 5 * NQ + 8), hist = cv.take<uint32_t>(NQ * 768);
		prim = cv.take<int32_t>(NW), cov = cv.take<uint64_t>(NW), ext = cv.take<uint64_t>(NW), aoff = cv.take<int64_t>(NW);
		flag = cv.take<int32_t>(T + 1), list = cv.take<int32_t>(T + 1), ctl = cv.take<int32_t>(NQ * 2);
		reg = cv.take<RegionRec>(NW), plan = cv.take<PlanRec>(NW), task = cv.take<mpa_dp_task_t>(4 * NW + T), seg = cv.take<SegRec>(T, 8), cnt = cv.take<PlansCounts>(NQ);
		h_reg = h.take<RegionRec>(NW), h_plan = h.take<PlanRec>(NW), h_task = h.take<mpa_dp_task_t>(4 * NW + T), h_seg = h.take<SegRec>(T), h_cnt = h.take<PlansCounts>(NQ);
		dev_bytes = cv.at + 256, pinned_bytes = h.at + 64;
	}
};

// ---- the walks over finished alignments (stats_run.hip; 16-byte sections).  The block that goes up: tables (the first KB) | jobs |
// cs slot offsets | rows slot offsets | CIGAR words | text; one block down per walk: records | what hangs off them.
// slot_bytes < 0: no cs strings; rows_bytes < 0: no residue rows (the block that goes up is then what it was without them)
struct StatsLayout {
	Piece<uint8_t> tabs; Piece<AlnStatsJob> jobs; Piece<int64_t> slot, rslot; Piece<uint32_t> cig; Piece<char> text, body, rbody;
	Piece<AlnStatsOut> out; Piece<AlnFeat> feat; Piece<AlnCsOut> cs_out; Piece<AlnRowsOut> rows_out;
	size_t up_bytes, down_bytes, cs_down_bytes, rows_down_bytes;
	explicit StatsLayout(const AlnWalkSizes &z) {
		const size_t nj = (size_t)z.n_jobs;
		Carve up(16), dn(16), cs(16), rows(16);
		tabs = Piece<uint8_t>{ 0, ALN_TAB_BYTES }, up.skip(1024);
		jobs = up.take<AlnStatsJob>(nj), slot = up.take_if<int64_t>(z.slot_bytes >= 0, nj + 1), rslot = up.take_if<int64_t>(z.rows_bytes >= 0, nj + 1);
		cig = up.take<uint32_t>((size_t)z.n_cigar), text = up.take<char>((size_t)z.text_bytes), up_bytes = up.at + 16;
		out = dn.take<AlnStatsOut>(nj), feat = dn.take<AlnFeat>((size_t)(z.n_feat > 0 ? z.n_feat : 0)), down_bytes = feat.end() + 16;
		cs_out = cs.take<AlnCsOut>(nj), body = cs.take<char>((size_t)(z.slot_bytes > 0 ? z.slot_bytes : 0)), cs_down_bytes = body.end() + 16;
		rows_out = rows.take<AlnRowsOut>(nj), rbody = rows.take<char>((size_t)(z.rows_bytes > 0 ? z.rows_bytes : 0)), rows_down_bytes = rbody.end() + 16;
	}
};
static_assert(ALN_TAB_BYTES <= 1024, "the tables share the first KB of the staging block");

// ---- accepted spans and region CIGARs (stats_run.hip; 16-byte sections)
// sp_in / h_sp_up: tables (the first KB) | plans | gap segments | round-1 results | text; sp_mid: k_spans' records with local
// numbers | tasks | exclusive counts | block sums (`blocks` workgroups); sp_out / h_sp_down: the task count and the tasks' three
// bounds as int64 (the first 32 bytes) | records | round-2 tasks
struct SpansLayout {
	Piece<uint8_t> tabs; Piece<SpansPlan> plan; Piece<SegRec> seg; Piece<mpa_dp_rst_t> rst1; Piece<char> text;
	Piece<SpanRec> mid_rec, rec; Piece<mpa_dp_task_t> tmp, task; Piece<int32_t> excl, bsum, n_task; Piece<int64_t> bounds;
	size_t up_bytes, mid_bytes, down_bytes;
	SpansLayout(int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes, size_t blocks) {
		const size_t np = (size_t)n_plan;
		Carve up(16), mid(16), head(8), dn(16);
		tabs = Piece<uint8_t>{ 0, ALN_TAB_BYTES }, up.skip(1024);
		plan = up.take<SpansPlan>(np), seg = up.take<SegRec>((size_t)n_seg), rst1 = up.take<mpa_dp_rst_t>((size_t)n_rst1), text = up.take<char>((size_t)text_bytes), up_bytes = up.at + 16;
		mid_rec = mid.take<SpanRec>(np), tmp = mid.take<mpa_dp_task_t>(np * 2), excl = mid.take<int32_t>(np), bsum = mid.take<int32_t>(blocks), mid_bytes = mid.at + 16;
		n_task = head.take<int32_t>(1), bounds = head.take<int64_t>(3), dn.skip(head.at);
		rec = dn.take<SpanRec>(np), task = dn.take<mpa_dp_task_t>(np * 2), down_bytes = task.end() + 16;
	}
};
// sp_in2 / h_sp_up2: round-2 results | slot offsets | a caller's round-2 pool; h_sp_down2: per-plan records | the assembled words
struct AsmLayout {
	Piece<mpa_dp_rst_t> rst2; Piece<int64_t> slot; Piece<uint32_t> pool2; Piece<AsmRec> rec; size_t up_bytes, rec_bytes;
	AsmLayout(int64_t n_plan, int64_t n_rst2, int64_t n_pool2) {
		Carve up(16), dn(16);
		rst2 = up.take<mpa_dp_rst_t>((size_t)n_rst2), slot = up.take<int64_t>((size_t)n_plan + 1), pool2 = up.take<uint32_t>((size_t)n_pool2), up_bytes = up.at + 16;
		rec = dn.take<AsmRec>((size_t)n_plan), rec_bytes = dn.at;
	}
	Piece<uint32_t> cigar(size_t n_words) const { return Piece<uint32_t>{ rec_bytes, n_words }; }
};
static_assert(sizeof(SpansPlan) % 8 == 0 && sizeof(SpanRec) % 8 == 0 && sizeof(AsmRec) % 8 == 0, "records in 16-byte aligned sections");

// ---- ranking and flat result of a batch (stats_run.hip, MPA_GPU_FINISH; 16-byte sections)
// fin_in / h_fin_up: the queries' first records | the large queries' numbers | records | CIGAR words | features | cs text | rows text;
// (behind the walks only the first three go up: the rest is read where the walks left it);
// fin_mid: kept hits by rank | counts | their prefix | the scratch of the queries of more than FINISH_LDS_REGS regions (none: empty
// pieces); h_fin_down: the prefix | hits | cs refs | rows refs | CIGAR words | features | cs text | rows text, every array dense from
// its piece's start and with room for a batch that keeps every hit -- the kernels write it directly, so only what is kept travels
struct FinishLayout {
	Piece<int64_t> first; Piece<int32_t> big; Piece<FinRec> rec; Piece<uint32_t> words, cigars; Piece<mpa_feat_t> in_feat, feats; Piece<char> in_cs, in_rows, cs_text, rows_text;
	Piece<FinOut> out; Piece<FinCounts> cnt, off, h_off; Piece<FinRank> tmp, r; Piece<Pair64> key; Piece<SortRange> stack; Piece<uint32_t> hist; Piece<int32_t> prim, ctl; Piece<uint64_t> cov;
	Piece<mpa_hit_t> hits; Piece<FinCsRef> cs; Piece<FinRowsRef> rows;
	size_t up_bytes, mid_bytes, down_bytes;
	explicit FinishLayout(const FinishSizes &z) {
		const size_t nq = (size_t)z.n_query, nr = (size_t)z.n_rec, nb = (size_t)z.n_big, sr = nb ? nr : 0;
		Carve up(16), mid(16), dn(16);
		first = up.take<int64_t>(nq + 1), big = up.take<int32_t>(nq), rec = up.take<FinRec>(nr), words = up.take<uint32_t>((size_t)z.in_words), in_feat = up.take<mpa_feat_t>((size_t)z.in_feat);
		in_cs = up.take<char>((size_t)z.in_cs), in_rows = up.take<char>((size_t)z.in_rows), up_bytes = up.at + 16;
		out = mid.take<FinOut>(nr), cnt = mid.take<FinCounts>(nq), off = mid.take<FinCounts>(nq + 1);
		tmp = mid.take<FinRank>(sr), r = mid.take<FinRank>(sr), key = mid.take<Pair64>(sr), stack = mid.take<SortRange>(nb ? sr / 64 + 8 * nb + 8 : 0), hist = mid.take<uint32_t>(768 * nb);
		prim = mid.take<int32_t>(sr), ctl = mid.take<int32_t>(2 * nb), cov = mid.take<uint64_t>(sr), mid_bytes = mid.at + 16;
		h_off = dn.take<FinCounts>(nq + 1), hits = dn.take<mpa_hit_t>(nr), cs = dn.take<FinCsRef>(nr), rows = dn.take<FinRowsRef>(nr), cigars = dn.take<uint32_t>((size_t)z.out_words);
		feats = dn.take<mpa_feat_t>((size_t)z.out_feat), cs_text = dn.take<char>((size_t)z.out_cs), rows_text = dn.take<char>((size_t)z.out_rows), down_bytes = dn.at + 16;
	}
};

// ---- the output text of a batch (stats_run.hip, MPA_GPU_FORMAT; 16-byte sections)
// fmt_in / h_fmt_up: the hits' prefix | query offsets | query name offsets | contig name offsets | contig lengths | hits | cs refs | rows
// refs | features | CIGAR words | cs text | rows text | query names | contig names (refs and texts only when the result carries them);
// fmt_mid: a place per hit | the queries' sums | their prefix; h_fmt_down: the totals (the head) | where the id fields lie | the text --
// sized from bounds, written by the kernels at their real size
struct FormatLayout {
	Piece<int64_t> hit_off, q_off, qname_off, cname_off, clen, id_at; Piece<mpa_hit_t> hits; Piece<FinCsRef> cs; Piece<FinRowsRef> rows; Piece<mpa_feat_t> feats; Piece<uint32_t> cigars;
	Piece<char> cs_text, rows_text, qname, cname, text; Piece<FmtAt> at; Piece<FmtCounts> cnt, off, head;
	size_t up_bytes, mid_bytes, down_bytes;
	explicit FormatLayout(const FormatSizes &z) {
		const size_t nq = (size_t)z.n_query, nh = (size_t)z.n_hit, nc = (size_t)z.n_ctg;
		Carve up(16), mid(16), dn(16);
		hit_off = up.take<int64_t>(nq + 1), q_off = up.take<int64_t>(nq + 1), qname_off = up.take<int64_t>(nq + 1), cname_off = up.take<int64_t>(nc + 1), clen = up.take<int64_t>(nc);
		hits = up.take<mpa_hit_t>(nh), cs = up.take_if<FinCsRef>(z.has_cs != 0, nh), rows = up.take_if<FinRowsRef>(z.has_rows != 0, nh);
		feats = up.take<mpa_feat_t>((size_t)z.n_feat), cigars = up.take<uint32_t>((size_t)z.n_words), cs_text = up.take<char>((size_t)z.cs_bytes), rows_text = up.take<char>((size_t)z.rows_bytes);
		qname = up.take<char>((size_t)z.qname_bytes), cname = up.take<char>((size_t)z.cname_bytes), up_bytes = up.at + 16;
		at = mid.take<FmtAt>((size_t)z.n_place), cnt = mid.take<FmtCounts>(nq), off = mid.take<FmtCounts>(nq + 1), mid_bytes = mid.at + 16;
		head = dn.take<FmtCounts>(1), id_at = dn.take<int64_t>((size_t)z.id_cap), text = dn.take<char>((size_t)z.text_cap), down_bytes = dn.at + 16;
	}
};

// ---- a resident round's results pool (dp_exec.hip; round.cigoff, 64-byte sections): off[n_glob] | call_off[n] | bsum[blocks + 1] |
// head (64 bytes) | rst[n]; header and records come down in one copy
struct ResLayout {
	Piece<int64_t> off, call_off, bsum, head; Piece<mpa_dp_rst_t> rst; size_t end;
	ResLayout(size_t n, size_t n_glob, size_t blocks) {
		Carve cv(64);
		off = cv.take<int64_t>(n_glob), call_off = cv.take<int64_t>(n), bsum = cv.take<int64_t>(blocks + 1), head = cv.take<int64_t>(8), rst = cv.take<mpa_dp_rst_t>(n);
		end = cv.at + 64;
	}
	size_t down_bytes() const { return rst.end() - head.off; }
};

} // namespace mpa
