// carve_check.cpp -- Carve / Piece (miniprot_amd/csrc/carve.h) against plain arithmetic, and every layout of dev_layout.h against a
// plain restatement of the offset arithmetic the drivers spelled out by hand before the layouts were typed: every offset and every
// total must be equal, every piece must start on a multiple of its element's alignment, end within the block, and be disjoint from
// every other piece of the block.  Stand-alone, compiled by tests/test_carve_cpu.py with AddressSanitizer and UBSan; prints
// "<cases> cases, <n> mismatches".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "dev_layout.h"

using namespace mpa;

static long g_cases = 0, g_fail = 0;
static void fail(const char *what, const char *name, size_t got, size_t want)
{
	if (++g_fail <= 20) fprintf(stderr, "MISMATCH %s %s: %zu, expected %zu\n", what, name, got, want);
}
static void eq(const char *what, const char *name, size_t got, size_t want) { if (got != want) fail(what, name, got, want); }
#define EQ(what, got, want) eq(what, #got, (size_t)(got), (size_t)(want))

// ---- a block's pieces, for the per-layout properties
struct Span { const char *name; size_t off, end, align; };
template<typename T> static Span span(const char *name, const Piece<T> &p) { return Span{ name, p.off, p.end(), alignof(T) }; }
#define SP(L, f) span(#f, (L).f)
static void check_block(const char *what, const std::vector<Span> &v, size_t total)
{
	for (size_t i = 0; i < v.size(); ++i) {
		if (v[i].off % v[i].align) fail(what, v[i].name, v[i].off % v[i].align, 0);
		if (v[i].end > total) fail(what, v[i].name, v[i].end, total);
		for (size_t j = 0; j < i; ++j)
			if (v[i].off < v[i].end && v[j].off < v[j].end && v[i].off < v[j].end && v[j].off < v[i].end) fail(what, v[i].name, v[i].off, v[j].end);
	}
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng; }

// the rounding the drivers wrote out, in one place for the restatements below
static size_t up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
struct Plain256 { size_t at = 0; size_t operator()(size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; } };

static void check_carve()
{
	const size_t aligns[4] = { 1, 16, 64, 256 };
	for (size_t a : aligns) {
		std::vector<size_t> sizes = { 0, 1, a - 1, a, a + 1 };
		for (int k = 0; k < 1000; ++k) sizes.push_back((size_t)(rnd() & (((uint64_t)1 << 33) - 1)));
		Carve c(a);
		size_t at = 0;
		for (size_t k = 0; k < sizes.size(); ++k, ++g_cases) {
			const size_t n = sizes[k], extra = k % 3 == 0 ? 0 : k % 3 == 1 ? 16 : 64;
			// bytes
			const Piece<uint8_t> b = c.take<uint8_t>(n);
			EQ("take<uint8_t>", b.off, at), EQ("take<uint8_t>", b.n, n), EQ("take<uint8_t>", b.bytes(), n), at += up(n, a), EQ("take<uint8_t>", c.at, at);
			// typed elements with slack
			const Piece<uint64_t> w = c.take<uint64_t>(n, extra);
			EQ("take<uint64_t>", w.off, at), EQ("take<uint64_t>", w.bytes(), n * 8), EQ("take<uint64_t>", w.end(), at + n * 8), at += up(n * 8 + extra, a), EQ("take<uint64_t>", c.at, at);
			// an optional part that is absent: an empty piece where it would have been
			const Piece<uint32_t> none = c.take_if<uint32_t>(false, n, extra);
			EQ("take_if(false)", none.off, at), EQ("take_if(false)", none.n, 0), EQ("take_if(false)", c.at, at);
			const Piece<uint32_t> some = c.take_if<uint32_t>(true, n, extra);
			EQ("take_if(true)", some.off, at), at += up(n * 4 + extra, a), EQ("take_if(true)", c.at, at);
			// a piece inside another: the two halves of a pair of 32-bit arrays, and the whole as 64-bit words
			if (n >= 1 && n < ((size_t)1 << 30)) {
				const Piece<int32_t> pair = c.take<int32_t>(2 * n);
				const Piece<int32_t> lo = pair.sub<int32_t>(0, n), hi = pair.sub<int32_t>(n * 4, n);
				const Piece<uint64_t> whole = pair.sub<uint64_t>(0, n);
				EQ("sub", lo.off, at), EQ("sub", hi.off, at + n * 4), EQ("sub", hi.end(), pair.end()), EQ("sub", whole.off, pair.off), EQ("sub", whole.end(), pair.end());
				if (lo.end() > hi.off || hi.end() > pair.end() || lo.off < pair.off) fail("sub", "inside its parent", hi.end(), pair.end());
				at += up(n * 8, a), EQ("sub", c.at, at);
			}
			c.skip(1024), at += 1024, EQ("skip", c.at, at);
		}
		// in(): base plus offset, with the element type
		alignas(16) char block[64];
		const Piece<int32_t> p{ 16, 4 };
		if ((char*)p.in(block) != block + 16 || (const char*)p.in((const char*)block) != block + 16) fail("in", "base + off", 0, 16);
	}
}

// ---- the chain tail: extraction scratch, counts, forward pass
static void check_extract(size_t m, size_t n_prob, size_t before)
{
	++g_cases;
	Plain256 carve;
	Carve cv;
	if (before) carve(before), cv.take<uint8_t>(before);
	// (the drivers' arithmetic)
	const size_t mark = carve(m * 4), order = carve(m * 4), ends = carve((m + 64 * n_prob + 64) * sizeof(Pair64)), tail8 = carve(m * sizeof(Pair64));
	const size_t items = carve(m * sizeof(SparseItem)), moved = carve(m * sizeof(SparseItem)), merged = carve(m * sizeof(SparseItem));
	const size_t kept = carve(m), stack = carve((m / 64 + 6 * n_prob + 16) * sizeof(SortRange)), status = carve(n_prob * 4 + 16);
	const size_t mf = carve(m * 4), mpred = carve(m * 4), mmark = carve(m * 4);
	const size_t long_cap = m / (size_t)(48 + 1) + 16, o_long = carve(long_cap * sizeof(LongRun)), o_nlong = carve(64);
	const size_t na = carve(n_prob * 8 + 8), nu = carve(n_prob * 8 + 8), offa = carve(n_prob * 8 + 16), offu = carve(n_prob * 8 + 16);
	const size_t long2 = carve(long_cap * sizeof(LongRun)), nlong2 = carve(64);

	ExtractCarve c = carve_extract_scratch(cv, m, n_prob);
	const ChainFwdCarve fw = carve_chain_fwd(cv, m, kChainSerialRun);
	carve_extract_counts(cv, n_prob, c);
	ChainFwdCarve runs{};
	carve_chain_runs(cv, m, kChainSerialRun, runs);
	EQ("extract", c.mark.off, mark), EQ("extract", c.order.off, order), EQ("extract", c.ends.off, ends), EQ("extract", c.tail8.off, tail8);
	EQ("extract", c.items.off, items), EQ("extract", c.moved.off, moved), EQ("extract", c.merged.off, merged);
	EQ("extract", c.kept.off, kept), EQ("extract", c.stack.off, stack), EQ("extract", c.status.off, status), EQ("extract", c.status.bytes() + 16, n_prob * 4 + 16);
	EQ("chain fwd", fw.f.off, mf), EQ("chain fwd", fw.pred.off, mpred), EQ("chain fwd", fw.mark.off, mmark), EQ("chain fwd", fw.runs.off, o_long), EQ("chain fwd", fw.runs.n, long_cap);
	EQ("chain fwd", fw.n_runs.off, o_nlong), EQ("chain fwd", fw.n_runs.bytes(), 64);
	EQ("counts", c.na.off, na), EQ("counts", c.nu.off, nu), EQ("counts", c.offa.off, offa), EQ("counts", c.offu.off, offu);
	EQ("counts", c.offa.bytes(), (n_prob + 1) * 8);          // (what comes down: n_prob + 1 prefixes)
	EQ("chain runs", runs.runs.off, long2), EQ("chain runs", runs.n_runs.off, nlong2), EQ("total", cv.at, carve.at);
	check_block("chain tail", { SP(c, mark), SP(c, order), SP(c, ends), SP(c, tail8), SP(c, items), SP(c, moved), SP(c, merged), SP(c, kept), SP(c, stack), SP(c, status),
	                            SP(fw, f), SP(fw, pred), SP(fw, mark), SP(fw, runs), SP(fw, n_runs), SP(c, na), SP(c, nu), SP(c, offa), SP(c, offu), SP(runs, runs), SP(runs, n_runs) }, cv.at);
}

static void check_regions(size_t T, size_t NP)
{
	++g_cases;
	Plain256 cv;
	const size_t o_tmp = cv(T * sizeof(RegionRec)), o_out = cv(T * sizeof(RegionRec)), o_ext = cv(T * 8), o_cov = cv(T * 8), o_key = cv(T * sizeof(Pair64));
	const size_t o_stack = cv((T / 64 + 5 * NP + 8) * sizeof(SortRange)), o_hist = cv(NP * 768 * 4), o_prim = cv(T * 4), o_ctl = cv(NP * 8), o_nreg = cv(NP * 4);
	const size_t h_ext = T * sizeof(RegionRec), h_nreg = h_ext + T * 8;
	const RegionsLayout L(T, NP);
	EQ("regions", L.tmp.off, o_tmp), EQ("regions", L.out.off, o_out), EQ("regions", L.ext.off, o_ext), EQ("regions", L.cov.off, o_cov), EQ("regions", L.key.off, o_key);
	EQ("regions", L.stack.off, o_stack), EQ("regions", L.hist.off, o_hist), EQ("regions", L.prim.off, o_prim), EQ("regions", L.ctl.off, o_ctl), EQ("regions", L.n_reg.off, o_nreg);
	EQ("regions", L.dev_bytes, cv.at + 256);
	EQ("regions pinned", L.h_rec.off, 0), EQ("regions pinned", L.h_ext.off, h_ext), EQ("regions pinned", L.h_nreg.off, h_nreg), EQ("regions pinned", L.h_nreg.bytes(), NP * 4);
	EQ("regions pinned", L.pinned_bytes, h_nreg + NP * 4 + 64);
	check_block("regions", { SP(L, tmp), SP(L, out), SP(L, ext), SP(L, cov), SP(L, key), SP(L, stack), SP(L, hist), SP(L, prim), SP(L, ctl), SP(L, n_reg) }, L.dev_bytes);
	check_block("regions pinned", { SP(L, h_rec), SP(L, h_ext), SP(L, h_nreg) }, L.pinned_bytes);
}

static void check_plans(size_t T, size_t NW, size_t NQ)
{
	++g_cases;
	Plain256 cv;
	const size_t o_tmp = cv(NW * sizeof(RegionRec)), o_key = cv(NW * sizeof(Pair64)), o_stack = cv((NW / 64 + 5 * NQ + 8) * sizeof(SortRange)), o_hist = cv(NQ * 768 * 4);
	const size_t o_prim = cv(NW * 4), o_cov = cv(NW * 8), o_ext = cv(NW * 8), o_aoff = cv(NW * 8), o_flag = cv(T * 4 + 4), o_list = cv(T * 4 + 4), o_ctl = cv(NQ * 8);
	const size_t o_reg = cv(NW * sizeof(RegionRec)), o_plan = cv(NW * sizeof(PlanRec)), o_task = cv((4 * NW + T) * sizeof(mpa_dp_task_t)), o_seg = cv(T * sizeof(SegRec) + 8);
	const size_t o_cnt = cv(NQ * sizeof(PlansCounts));
	const size_t h_plan = NW * sizeof(RegionRec), h_task = h_plan + NW * sizeof(PlanRec), h_seg = h_task + (4 * NW + T) * sizeof(mpa_dp_task_t), h_cnt = h_seg + T * sizeof(SegRec);
	const PlansLayout L(T, NW, NQ);
	EQ("plans", L.tmp.off, o_tmp), EQ("plans", L.key.off, o_key), EQ("plans", L.stack.off, o_stack), EQ("plans", L.hist.off, o_hist), EQ("plans", L.prim.off, o_prim);
	EQ("plans", L.cov.off, o_cov), EQ("plans", L.ext.off, o_ext), EQ("plans", L.aoff.off, o_aoff), EQ("plans", L.flag.off, o_flag), EQ("plans", L.list.off, o_list), EQ("plans", L.ctl.off, o_ctl);
	EQ("plans", L.reg.off, o_reg), EQ("plans", L.plan.off, o_plan), EQ("plans", L.task.off, o_task), EQ("plans", L.seg.off, o_seg), EQ("plans", L.cnt.off, o_cnt);
	EQ("plans", L.dev_bytes, cv.at + 256);
	EQ("plans pinned", L.h_reg.off, 0), EQ("plans pinned", L.h_plan.off, h_plan), EQ("plans pinned", L.h_task.off, h_task), EQ("plans pinned", L.h_seg.off, h_seg), EQ("plans pinned", L.h_cnt.off, h_cnt);
	EQ("plans pinned", L.pinned_bytes, h_cnt + NQ * sizeof(PlansCounts) + 64);
	check_block("plans", { SP(L, tmp), SP(L, key), SP(L, stack), SP(L, hist), SP(L, prim), SP(L, cov), SP(L, ext), SP(L, aoff), SP(L, flag), SP(L, list), SP(L, ctl), SP(L, reg), SP(L, plan),
	                       SP(L, task), SP(L, seg), SP(L, cnt) }, L.dev_bytes);
	check_block("plans pinned", { SP(L, h_reg), SP(L, h_plan), SP(L, h_task), SP(L, h_seg), SP(L, h_cnt) }, L.pinned_bytes);
}

static void check_stats(const AlnWalkSizes &z)
{
	++g_cases;
	auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
	const size_t off_jobs = 1024;
	const size_t off_slot = off_jobs + up16((size_t)z.n_jobs * sizeof(AlnStatsJob));
	const size_t off_rslot = off_slot + (z.slot_bytes >= 0 ? up16((size_t)(z.n_jobs + 1) * 8) : 0);
	const size_t off_cig = off_rslot + (z.rows_bytes >= 0 ? up16((size_t)(z.n_jobs + 1) * 8) : 0);
	const size_t off_text = off_cig + up16((size_t)z.n_cigar * 4);
	const size_t up_bytes = off_text + up16((size_t)z.text_bytes) + 16;
	const size_t off_feat = up16((size_t)z.n_jobs * sizeof(AlnStatsOut));
	const size_t down_bytes = off_feat + (size_t)(z.n_feat > 0 ? z.n_feat : 0) * sizeof(AlnFeat) + 16;
	const size_t off_body = up16((size_t)z.n_jobs * sizeof(AlnCsOut));
	const size_t cs_down_bytes = off_body + (size_t)(z.slot_bytes > 0 ? z.slot_bytes : 0) + 16;
	const size_t off_rbody = up16((size_t)z.n_jobs * sizeof(AlnRowsOut));
	const size_t rows_down_bytes = off_rbody + (size_t)(z.rows_bytes > 0 ? z.rows_bytes : 0) + 16;
	const StatsLayout L(z);
	EQ("walks up", L.tabs.off, 0), EQ("walks up", L.jobs.off, off_jobs), EQ("walks up", L.slot.off, off_slot), EQ("walks up", L.rslot.off, off_rslot), EQ("walks up", L.cig.off, off_cig);
	EQ("walks up", L.text.off, off_text), EQ("walks up", L.up_bytes, up_bytes);
	EQ("walks up", L.slot.n, z.slot_bytes >= 0 ? z.n_jobs + 1 : 0), EQ("walks up", L.rslot.n, z.rows_bytes >= 0 ? z.n_jobs + 1 : 0);
	EQ("walks down", L.out.off, 0), EQ("walks down", L.feat.off, off_feat), EQ("walks down", L.down_bytes, down_bytes);
	EQ("walks cs", L.cs_out.off, 0), EQ("walks cs", L.body.off, off_body), EQ("walks cs", L.cs_down_bytes, cs_down_bytes);
	EQ("walks rows", L.rows_out.off, 0), EQ("walks rows", L.rbody.off, off_rbody), EQ("walks rows", L.rows_down_bytes, rows_down_bytes);
	check_block("walks up", { SP(L, tabs), SP(L, jobs), SP(L, slot), SP(L, rslot), SP(L, cig), SP(L, text) }, L.up_bytes);
	check_block("walks down", { SP(L, out), SP(L, feat) }, L.down_bytes);
	check_block("walks cs", { SP(L, cs_out), SP(L, body) }, L.cs_down_bytes);
	check_block("walks rows", { SP(L, rows_out), SP(L, rbody) }, L.rows_down_bytes);
}

static void check_spans(int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes)
{
	++g_cases;
	auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
	const unsigned blocks = (unsigned)((n_plan + 256 - 1) / 256);
	const size_t off_plan = 1024;
	const size_t off_seg = off_plan + up16((size_t)n_plan * sizeof(SpansPlan));
	const size_t off_rst1 = off_seg + up16((size_t)n_seg * sizeof(SegRec));
	const size_t off_text = off_rst1 + up16((size_t)n_rst1 * sizeof(mpa_dp_rst_t));
	const size_t up_bytes = off_text + up16((size_t)text_bytes) + 16;
	const size_t off_tmp = up16((size_t)n_plan * sizeof(SpanRec));
	const size_t off_excl = off_tmp + up16((size_t)n_plan * 2 * sizeof(mpa_dp_task_t));
	const size_t off_bsum = off_excl + up16((size_t)n_plan * 4);
	const size_t mid_bytes = off_bsum + up16((size_t)blocks * 4) + 16;
	const size_t off_rec = 32;
	const size_t off_task = off_rec + up16((size_t)n_plan * sizeof(SpanRec));
	const size_t down_bytes = off_task + (size_t)n_plan * 2 * sizeof(mpa_dp_task_t) + 16;
	const SpansLayout L(n_plan, n_seg, n_rst1, text_bytes, blocks);
	EQ("spans up", L.tabs.off, 0), EQ("spans up", L.plan.off, off_plan), EQ("spans up", L.seg.off, off_seg), EQ("spans up", L.rst1.off, off_rst1), EQ("spans up", L.text.off, off_text);
	EQ("spans up", L.up_bytes, up_bytes);
	EQ("spans mid", L.mid_rec.off, 0), EQ("spans mid", L.tmp.off, off_tmp), EQ("spans mid", L.excl.off, off_excl), EQ("spans mid", L.bsum.off, off_bsum), EQ("spans mid", L.bsum.n, blocks);
	EQ("spans mid", L.mid_bytes, mid_bytes);
	EQ("spans down", L.n_task.off, 0), EQ("spans down", L.bounds.off, 8), EQ("spans down", L.bounds.bytes(), 24), EQ("spans down", L.rec.off, off_rec), EQ("spans down", L.task.off, off_task);
	EQ("spans down", L.down_bytes, down_bytes);
	check_block("spans up", { SP(L, tabs), SP(L, plan), SP(L, seg), SP(L, rst1), SP(L, text) }, L.up_bytes);
	check_block("spans mid", { SP(L, mid_rec), SP(L, tmp), SP(L, excl), SP(L, bsum) }, L.mid_bytes);
	check_block("spans down", { SP(L, n_task), SP(L, bounds), SP(L, rec), SP(L, task) }, L.down_bytes);
}

static void check_asm(int64_t n_plan, int64_t n_rst2, int64_t n_pool2, size_t n_words)
{
	++g_cases;
	auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
	const size_t off_slot = up16((size_t)n_rst2 * sizeof(mpa_dp_rst_t));
	const size_t off_pool2 = off_slot + up16((size_t)(n_plan + 1) * 8);
	const size_t up_bytes = off_pool2 + up16((size_t)n_pool2 * 4) + 16;
	const size_t rec_bytes = up16((size_t)n_plan * sizeof(AsmRec));
	const size_t down_bytes = rec_bytes + n_words * 4 + 16;
	const AsmLayout L(n_plan, n_rst2, n_pool2);
	const Piece<uint32_t> cig = L.cigar(n_words);
	EQ("assemble up", L.rst2.off, 0), EQ("assemble up", L.slot.off, off_slot), EQ("assemble up", L.pool2.off, off_pool2), EQ("assemble up", L.up_bytes, up_bytes);
	EQ("assemble down", L.rec.off, 0), EQ("assemble down", L.rec.bytes(), (size_t)n_plan * sizeof(AsmRec)), EQ("assemble down", L.rec_bytes, rec_bytes), EQ("assemble down", cig.off, rec_bytes);
	EQ("assemble down", cig.end() + 16, down_bytes);
	check_block("assemble up", { SP(L, rst2), SP(L, slot), SP(L, pool2) }, L.up_bytes);
	check_block("assemble down", { SP(L, rec), span("cigar", cig) }, down_bytes);
}

static void check_res(size_t n, size_t n_glob, size_t blocks)
{
	++g_cases;
	auto up64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t off = 0, call_off = up64(8 * n_glob), bsum = call_off + up64(8 * n), head = bsum + up64(8 * (blocks + 1));
	const size_t rst = head + 64, end = rst + up64(sizeof(mpa_dp_rst_t) * n) + 64;
	const ResLayout L(n, n_glob, blocks);
	EQ("results", L.off.off, off), EQ("results", L.call_off.off, call_off), EQ("results", L.bsum.off, bsum), EQ("results", L.head.off, head), EQ("results", L.head.bytes(), 64);
	EQ("results", L.rst.off, rst), EQ("results", L.end, end), EQ("results", L.down_bytes(), 64 + sizeof(mpa_dp_rst_t) * n);
	check_block("results", { SP(L, off), SP(L, call_off), SP(L, bsum), SP(L, head), SP(L, rst) }, L.end);
}

int main()
{
	check_carve();
	const size_t big[5] = { 1, 63, 64, 65, 4097 }, few[3] = { 1, 2, 65 };
	for (size_t m : big) for (size_t np : few) for (size_t before : { (size_t)0, (size_t)24 }) check_extract(m, np, before);
	for (size_t T : { (size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4097 }) {
		for (size_t np : few) check_regions(T, np);
		for (size_t nw : few) for (size_t nq : few) check_plans(T, nw, nq);
	}
	const int64_t opt[3] = { -1, 0, 4097 };                   // a walk that is off, on with nothing to write, on
	for (size_t nj : big) for (size_t nc : big) for (size_t tb : big) for (int64_t feat : opt) for (int64_t cs : opt) for (int64_t rows : opt)
		check_stats(AlnWalkSizes{ (int64_t)nj, (int64_t)nc, (int64_t)tb, feat, cs, rows });
	for (size_t np : big) for (int64_t ns : { (int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4097 }) for (size_t nr : big) for (size_t tb : big)
		check_spans((int64_t)np, ns, (int64_t)nr, (int64_t)tb);
	for (size_t np : big) for (int64_t nr : { (int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4097 }) for (int64_t p2 : { (int64_t)0, (int64_t)1, (int64_t)63, (int64_t)4097 })
		for (size_t nw : { (size_t)0, (size_t)1, (size_t)4097 }) check_asm((int64_t)np, nr, p2, nw);
	for (size_t n : big) for (size_t ng : { (size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4097 }) for (size_t nb : { (size_t)0, (size_t)1, (size_t)2, (size_t)17 })
		check_res(n, ng, nb);
	printf("%ld cases, %ld mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
