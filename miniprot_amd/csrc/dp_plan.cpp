// dp_plan.cpp -- the planner of a DP round (dp_plan.h): classify the calls, sort them, lay out every pool, pack waves, chunk the
// tracebacks, list the round's units.  Host only; tests/test_dp_plan_cpu.py pins what it produces.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "dp_plan.h"

namespace mpa {

// ns_log2 (nasw-sse.c:330-338) and the extension-length penalty of nasw-sse.c:426 tabulated as a step
// function.  Evaluated on the host with the same float operations as the reference (no FMA contraction),
// so the kernel needs no floating point at all.
static float log2_poly(float x)
{
	union { float f; uint32_t i; } z = { x };
	float r = (float)((int32_t)((z.i >> 23) & 255) - 128);
	z.i &= ~(255u << 23);
	z.i += 127u << 23;
	r += (-0.34484843f * z.f + 2.02466578f) * z.f - 0.67487759f;
	return r;
}

static int build_pen_table(float coef, int32_t max_x, PenTable *pt)
{
	int32_t n = 0, cur = 0;
	pt->x[n] = INT32_MIN, pt->val[n] = 0, ++n;
	for (int32_t x = 2; x <= max_x; ++x) {
		int32_t v = (int32_t)(coef * log2_poly((float)x) + .5f);
		if (v != cur) {
			if (n >= MPA_PEN_MAX - 1) return -1;
			pt->x[n] = x, pt->val[n] = v, ++n, cur = v;
		}
	}
	pt->n = n;
	for (int32_t k = n; k < MPA_PEN_MAX; ++k) pt->x[k] = INT32_MAX, pt->val[k] = cur;
	return 0;
}

static int refuse(DpPlan &P, int rc, const std::string &msg) { P.rc = rc, P.err = msg; return rc; }

// ---- classify: one DTask per call, its class and profile width; ext_ids / glob_ids unsorted
static int classify(DpPlan &P, const mpa_dp_task_t *in, int64_t n, const int64_t *ctg_len, size_t ctg_stride, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn)
{
	// parameter guards: outside these the packed-int16 kernels would not be bit-exact
	int32_t max_mat = 0;
	for (int k = 0; k < 484; ++k) max_mat = std::max<int32_t>(max_mat, opt->mat[k]);
	if (opt->go < 0 || opt->go > 32000 || opt->ge < 0 || opt->ge > 16000 || opt->fs < 0 || opt->fs > 16000 || opt->xdrop < 0 || opt->xdrop > 32000 ||
	    opt->end_bonus < 0 || opt->end_bonus > 1000 || (opt->ge > 255 && opt->go + opt->ge > 32000))
		return refuse(P, MPA_ERR_UNSUPPORTED, "DP parameters outside the supported range (go <= 32000, ge, fs <= 16000, 0 <= xdrop <= 32000, 0 <= end_bonus <= 1000)");
	// Gap-extension / frameshift penalties above 255 (-E / -F of the reference's command line, main.c:133,136) do not fit the byte
	// the row records give them.  Such a run keeps the records' layout -- the byte then flags a stop codon -- and sweeps every call
	// with the kernels that read it that way (glob_cands<K, true>): the stand-alone traceback kernels and, for extension calls,
	// the block-major one-wave sweep (k_ext_huge); the packed round kernel is not used.  Slow, exact, and nobody's default.
	P.wide_ge = opt->ge > 255 || opt->fs > 255;
	const char *too_wide = ": too wide for this gap-extension penalty (columns x ge must stay below 2^19 in the int32 sweeps)";
	P.tasks.assign((size_t)n, DTask{});
	for (int64_t k = 0; k < n; ++k) {
		const mpa_dp_task_t &x = in[k];
		DTask &t = P.tasks[(size_t)k];
		if (x.nl < 0 || x.al <= 0 || x.qid < 0 || x.qid >= q->n_seq || x.io < 0 || x.io > 32000) return refuse(P, MPA_ERR_ARG, "malformed DP task");
		// the kernels address the resident genome and the query buffer with these: a window or a protein slice that leaves its
		// contig / its query would read foreign memory (or fault the context), so it is refused here
		if (x.vid < 0 || x.vid >= 2 * n_ctg || x.nt_off < 0 || x.nt_off + (int64_t)x.nl > *(const int64_t*)((const char*)ctg_len + (size_t)(x.vid >> 1) * ctg_stride) ||
		    x.aa_off < 0 || (int64_t)x.aa_off + x.al > q->q_off[x.qid + 1] - q->q_off[x.qid])
			return refuse(P, MPA_ERR_ARG, "DP task " + std::to_string(k) + " reaches outside its contig or its query");
		t.nt_off = x.nt_off, t.vid = x.vid, t.nl = x.nl, t.al = x.al, t.flag = x.flag, t.io = x.io;
		t.q_off = q->q_off[x.qid] + x.aa_off - q->q_off[0];     // relative to the slice the executor uploads
		t.ncol = (x.al + 7) / 8 * 8;
		t.out_idx = (int32_t)k;
		// (the int32 sweeps keep the striped reference's lane segments apart by offsets of 2^20 in their scans: column * ge must stay
		// below; checked where it matters: the traceback sweeps and the block-major extension sweep)
		const bool seg_overflow = (int64_t)t.ncol * opt->ge >= (1 << 19);
		// The packed int16 kernels run their gap scan on h + j*ge with saturating adds and hold go + j*ge in int16, which is only the
		// reference's value while nothing can reach the int16 limits.  Calls that could -- with BLOSUM62 and ge = 1 more than ~2900
		// columns, always of the huge class; with a large -E or -O already at a few dozen columns -- go to the int32 sweeps, which
		// clamp every operation like the reference does: k_ext_huge for extension calls, the plain traceback sweep for the others.
		const bool may_saturate = (int64_t)x.al * max_mat + (int64_t)t.ncol * opt->ge + std::max(0, opt->end_bonus) > 32000 || opt->go + (int64_t)t.ncol * opt->ge > 32000;
		const bool packed_ok = !P.wide_ge && !may_saturate;
		if (x.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) {
			int cls = ext_class_of(t.ncol);
			if (kn.no_split && cls >= X_SPLIT2) cls = X_HUGE;         // repeated round: no inter-workgroup hand-off (see mpa_dp_run)
			if (!packed_ok) cls = X_HUGE;
			if (cls == X_HUGE && seg_overflow) return refuse(P, MPA_ERR_UNSUPPORTED, "DP call " + std::to_string(k) + too_wide);
			t.pw = cls == X_HUGE ? t.ncol : ext_columns(cls);
			// 65..128 columns: one wave per call instead of a two-wave group per pair of calls (MPA_DP_EXT_DUAL=0: the two-wave groups)
			if (cls == X_W2 && kn.ext_dual && !kn.antidiag) cls = X_128;
			t.cls = cls;
			P.ext_ids.push_back((int32_t)k);
			P.max_nl_ext = std::max(P.max_nl_ext, x.nl);
		} else {
			if (!(x.flag & MPA_F_CIGAR)) return refuse(P, MPA_ERR_UNSUPPORTED, "global DP without CIGAR is not part of miniprot's path");
			if (seg_overflow) return refuse(P, MPA_ERR_UNSUPPORTED, "DP call " + std::to_string(k) + too_wide);
			t.pw = t.ncol;
			t.cls = tb_class_of(t.ncol);
			// Checkpointed traceback (dp_device.h): a call of up to 128 columns and many rows -- the gap fills across introns and the spans
			// of accepted extensions, where nearly every row lies inside an intron -- is swept by the packed sweep and walked by k_walk.
			// Short calls stay on the plain traceback sweep: the walk would recompute all of their rows anyway.  The packed sweep is an
			// int16 one: calls that may saturate stay on the plain sweep too.  129..256 columns under the same predicate with lite_wide
			// (MPA_DP_LITE_WIDE=1; the default keeps them on the plain sweep, and so does the worker pool, whose workers do not know the class).
			const bool many_rows = kn.lite_min > 0 && packed_ok && x.nl >= kn.lite_min && x.nl >= 3;
			if (many_rows && t.cls <= T_W2) t.cls += T_LITE16, t.pw = lite_columns(t.cls);
			else if (many_rows && t.cls == T_W4 && kn.lite_wide && !kn.pool) t.cls = T_LITE_W4, t.pw = lite_columns(T_LITE_W4);
			P.glob_ids.push_back((int32_t)k);
		}
	}
	return MPA_OK;
}

// ---- record, profile, CIGAR, boundary and key ranges of every call, in sorted order; the prep chunks
static void lay_out_pools(DpPlan &P, const DpPlanKnobs &kn)
{
	auto common = [&P](int32_t id) {
		DTask &t = P.tasks[id];
		t.rec_off = P.rec_total, P.rec_total += t.nl;
		t.prof_off = P.prof_total, P.prof_total += (int64_t)22 * t.pw;
		P.max_nl = std::max(P.max_nl, t.nl);
		for (int32_t r = 0; r < t.nl; r += MPA_PREP_CHUNK_ROWS) P.prep.push_back(PrepChunk{ id, r });
	};
	for (int32_t id : P.ext_ids) {
		common(id);
		DTask &t = P.tasks[id];
		if (t.cls == X_HUGE) t.bnd_off = P.bnd_total, P.bnd_total += t.nl, t.tb_off = P.hkey_total, P.hkey_total += t.nl, P.huge_ids.push_back(id);   // (tb_off: per-row keys, 8 B)
	}
	for (int32_t id : P.glob_ids) {
		common(id);
		DTask &t = P.tasks[id];
		t.cig_cap = t.nl + t.al + 4;
		t.cig_off = P.cig_total, P.cig_total += t.cig_cap;
		if (t.cls == T_MB) t.bnd_off = P.bnd_total, P.bnd_total += t.nl;
	}
	P.rec_pad = P.max_nl + 96 + (kn.antidiag ? 64 : 0);        // kernels prefetch records up to 48 rows past a call's end (the anti-diagonal prototype: 128)
	P.rec_total += P.rec_pad;
}

// the next descriptor: up to `per` consecutive calls of ids[p, end) that share the class of ids[p]
template<typename W> static W pack_wave(const std::vector<DTask> &T, const std::vector<int32_t> &ids, size_t &p, size_t end, int per)
{
	W w;
	memset(&w, 0, sizeof(w));
	for (int32_t &t : w.task) t = -1;
	const int32_t cls = T[ids[p]].cls;
	for (int k = 0; k < per && p < end && T[ids[p]].cls == cls; ++k, ++p)
		w.task[k] = ids[p], w.max_nl = std::max(w.max_nl, T[ids[p]].nl);
	return w;
}

// ExtWave descriptors of the calls of class `cls` at ids[p ...]; checkpointed classes get their slot numbers, bit words and checkpoints
static WaveRange pack_ext_class(DpPlan &P, const std::vector<int32_t> &ids, size_t &p, int cls, int per, bool checkpointed)
{
	WaveRange r{ (int)P.ewaves.size(), 0 };
	while (p < ids.size() && P.tasks[ids[p]].cls == cls) {
		ExtWave w = pack_wave<ExtWave>(P.tasks, ids, p, ids.size(), per);
		w.rec_base = P.tasks[w.task[0]].rec_off;                 // (sorted: the first call of a wave has the smallest offset)
		if (checkpointed) {
			w.lite_off = P.lite_total, P.lite_total += lite_bits_dwords(cls, w.max_nl);
			w.ck_off = P.ck_total, P.ck_total += lite_ckpt_dwords(cls, w.max_nl);
			for (int k = 0; k < per && w.task[k] >= 0; ++k) {
				DTask &t = P.tasks[w.task[k]];
				t.flag |= k << MPA_LITE_SLOT_SHIFT, t.tb_off = w.lite_off, t.bnd_off = w.ck_off;
			}
		}
		P.ewaves.push_back(w);
	}
	r.cnt = (int)P.ewaves.size() - r.first;
	return r;
}

static void pack_waves(DpPlan &P)
{
	const std::vector<DTask> &T = P.tasks;
	size_t p = 0;
	for (int cls = X_16; cls <= X_SPLIT4; ++cls) P.ext[cls] = pack_ext_class(P, P.ext_ids, p, cls, ext_calls_per_wave(cls), false);
	for (size_t h = 0; h < P.huge_ids.size();) P.huge_waves.push_back(pack_wave<GlobWave>(T, P.huge_ids, h, P.huge_ids.size(), 1));
	p += P.huge_ids.size();                                     // (X_HUGE sorts between X_SPLIT4 and X_128)
	P.ext128 = pack_ext_class(P, P.ext_ids, p, X_128, ext_calls_per_wave(X_128), false);
	while (P.n_reg_glob < P.glob_ids.size() && !is_checkpointed(T[P.glob_ids[P.n_reg_glob]].cls)) ++P.n_reg_glob;
	P.n_lite = P.glob_ids.size() - P.n_reg_glob;
	p = P.n_reg_glob;
	for (int cls = T_LITE16; cls <= T_LITE128; ++cls) P.lite[cls - T_LITE16] = pack_ext_class(P, P.glob_ids, p, cls, lite_calls_per_wave(cls), true);
	P.lite_w4 = pack_ext_class(P, P.glob_ids, p, T_LITE_W4, lite_calls_per_wave(T_LITE_W4), true);   // pools sized by the group's longest call
	for (int c = 0; c < 5; ++c) P.walk_cnt[c] = 0;
	for (size_t k = P.n_reg_glob; k < P.glob_ids.size(); ++k) ++P.walk_cnt[T[P.glob_ids[k]].cls - T_LITE16];
	// per-row keys of the wide extension kernels: [group][2 halves][key_stride]
	for (int cls = X_W2; cls <= X_SPLIT4; ++cls)
		for (int k = 0; k < P.ext[cls].cnt; ++k) P.key_stride = std::max<int64_t>(P.key_stride, P.ewaves[P.ext[cls].first + k].max_nl), ++P.n_wide_groups;
	P.key_stride = (P.key_stride + 64) & ~(int64_t)63;
	// split classes: boundary granules (16 B per row and boundary: 3 boundaries per 1024-column group, 1 per 512-column group),
	// then the per-group completion counters and the error flag
	P.n_split = P.ext[X_SPLIT2].cnt + P.ext[X_SPLIT4].cnt, P.n_bound = 3 * (int64_t)P.ext[X_SPLIT4].cnt + P.ext[X_SPLIT2].cnt;
	P.xg_bytes = (size_t)P.n_bound * P.key_stride * 16, P.xg_tail = (2 * (size_t)P.n_split + 1) * 4;   // + done[n_split], ticket[n_split], err
}

// ---- chunks of the plain traceback sweep, bounded by traceback memory (their call lists and waves: dp_plan_chunk_waves)
static void plan_tb_chunks(DpPlan &P, const DpPlanKnobs &kn)
{
	for (size_t p = 0; p < P.n_reg_glob;) {
		DpTbChunk r;
		r.first = r.last = p;
		while (r.last < P.n_reg_glob) {
			DTask &t = P.tasks[P.glob_ids[r.last]];
			const int64_t wds = (int64_t)t.nl * t.ncol;
			if (r.last > r.first && (size_t)(r.tb_words + wds) * 2 > (size_t)kn.tb_budget) break;
			t.tb_off = r.tb_words, r.tb_words += wds, ++r.last;
		}
		p = r.last;
		P.tb_max = std::max(P.tb_max, r.tb_words);
		P.chunks.push_back(r);
	}
}

void dp_plan_chunk_waves(DpPlan &P, size_t ri)
{
	DpTbChunk &r = P.chunks[ri];
	r.waves.clear(), r.list.clear();
	size_t p = r.first;
	for (int cls = T_16; cls <= T_MB; ++cls) {
		r.cls[cls].first = (int)r.waves.size();
		while (p < r.last && P.tasks[P.glob_ids[p]].cls == cls) {
			r.waves.push_back(pack_wave<GlobWave>(P.tasks, P.glob_ids, p, r.last, tb_calls_per_wave(cls)));
			for (int32_t id : r.waves.back().task) if (id >= 0) r.list.push_back(id);
		}
		r.cls[cls].cnt = (int)r.waves.size() - r.cls[cls].first;
	}
}

// ---- the units of the round: the extension waves/groups of every class, the packed sweeps of the checkpointed calls and
// (round_has_glob) the plain traceback waves of the first chunk; longest first
// cost model: nanoseconds per row of a unit's longest call, by kind (measured: profiles/r06_dp_ns_per_row.txt, r06_wide_ns_per_row.txt)
enum : int64_t { NS_EXT_NARROW = 160, NS_EXT_WIDE = 270, NS_EXT_SPLIT = 310, NS_EXT128 = 200, NS_LITE = 170, NS_LITE128 = 200, NS_LITE_W4 = 280, NS_GLOB = 430, NS_GLOB_WIDE = 510 };

struct Cost { int64_t cost; DpUnit u; };
static bool costlier(const Cost &x, const Cost &y) { return x.cost > y.cost; }

// every unit of the round with its cost, costliest first
static std::vector<Cost> unit_costs(const DpPlan &P, const DpPlanKnobs &kn)
{
	std::vector<Cost> cu;
	auto add = [&](int kind, int first, int count, int64_t cost, int blk = 0, int n_blk = 1, int sgroup = 0, int xg_first = 0) {
		cu.push_back(Cost{ cost, DpUnit{ kind, first, count, blk, n_blk, sgroup, xg_first, 0 } });
	};
	// `per` neighbours of the sorted descriptors r share a unit (the first is the longest)
	auto add_range = [&](int kind, const WaveRange &r, int per, int64_t ns_per_row) {
		for (int k = 0; k < r.cnt; k += per) add(kind, r.first + k, std::min(per, r.cnt - k), (int64_t)P.ewaves[r.first + k].max_nl * ns_per_row);
	};
	// (worker pool: the one-wave kinds are units of ONE wave descriptor each, taken by single waves; without the pool a
	// workgroup's four waves take four neighbours of the sorted list)
	const int per_narrow = kn.pool ? 1 : 4;
	for (int cls = X_16; cls <= X_64; ++cls)
		if (!(cls == X_32 && kn.antidiag)) add_range(U_EXT16 + cls, P.ext[cls], per_narrow, NS_EXT_NARROW);
	// (worker pool: a workgroup goes on to its next unit, so all four waves must leave a unit through the same barriers -- a
	// 65..128-column group then takes a whole workgroup on the four-wave body, its waves 2 and 3 on dead columns)
	if (kn.pool) add_range(U_EXT_W4, P.ext[X_W2], 1, NS_EXT_WIDE);
	else add_range(U_EXT_W2, P.ext[X_W2], 2, NS_EXT_WIDE);
	add_range(U_EXT_W4, P.ext[X_W4], 1, NS_EXT_WIDE);
	const int n4 = P.ext[X_SPLIT4].cnt;                           // split groups and their boundaries are numbered 1024-column groups first
	for (int k = 0; k < n4; ++k)
		for (int b = 0; b < 4; ++b) add(U_EXT_SPLIT, P.ext[X_SPLIT4].first + k, 1, (int64_t)P.ewaves[P.ext[X_SPLIT4].first + k].max_nl * NS_EXT_SPLIT, b, 4, k, 3 * k);
	for (int k = 0; k < P.ext[X_SPLIT2].cnt; ++k)
		for (int b = 0; b < 2; ++b) add(U_EXT_SPLIT, P.ext[X_SPLIT2].first + k, 1, (int64_t)P.ewaves[P.ext[X_SPLIT2].first + k].max_nl * NS_EXT_SPLIT, b, 2, n4 + k, 3 * n4 + k);
	add_range(U_EXT128, P.ext128, per_narrow, NS_EXT128);
	for (int c = 0; c < 4; ++c) add_range(U_LITE16 + c, P.lite[c], per_narrow, T_LITE16 + c == T_LITE128 ? NS_LITE128 : NS_LITE);
	if (P.round_has_glob) {
		const DpTbChunk &r = P.chunks[0];
		for (int cls = T_16; cls <= T_MB; ++cls) {
			if (cls == T_W8 || cls == T_W16) continue;             // (the 512/1024-thread classes keep their own launch)
			const int kind = cls <= T_64 ? U_GLOB16 + cls : cls == T_MB ? (int)U_GLOB_MB : cls == T_W4 || kn.pool ? (int)U_GLOB_W4 : (int)U_GLOB_W2;
			const int per = cls == T_W2 ? (kn.pool ? 1 : 2) : cls == T_W4 ? 1 : per_narrow;
			for (int k = 0; k < r.cls[cls].cnt; k += per) {
				const GlobWave &g = r.waves[r.cls[cls].first + k];
				int64_t cost = (int64_t)g.max_nl * (cls == T_W2 || cls == T_W4 ? NS_GLOB_WIDE : NS_GLOB);
				if (cls == T_MB) cost *= (P.tasks[g.task[0]].ncol + 63) / 64;
				add(kind, r.cls[cls].first + k, std::min(per, r.cls[cls].cnt - k), cost);
			}
		}
	}
	std::stable_sort(cu.begin(), cu.end(), costlier);           // (stable: the workgroups of a split group stay adjacent, in column order)
	return cu;
}

int dp_plan_units(DpPlan &P, const DpPlanKnobs &kn, DpUnit *out)
{
	std::vector<Cost> cu = unit_costs(P, kn);
	P.n_units = P.n_group = 0, P.sz.units = 0;
	if (cu.empty()) return MPA_OK;
	// worker pool: the units that take a whole workgroup first (queue 0), then the one-wave units (queue 1), each longest first;
	// priorities stay relative to the round's longest unit of either kind
	const int64_t cost_max = cu[0].cost;
	if (kn.pool) {
		auto is_group = [](const Cost &c) { return c.u.kind == U_EXT_W4 || c.u.kind == U_EXT_SPLIT || c.u.kind == U_GLOB_W4; };
		P.n_group = (size_t)(std::stable_partition(cu.begin(), cu.end(), is_group) - cu.begin());
	}
	if (sizeof(DpUnit) * cu.size() > P.up.off - P.up.units) return refuse(P, MPA_ERR_HIP, "internal: more DP units than the staging buffer holds");
	// the units that bound the round's duration issue ahead of the short ones they share a SIMD with (s_setprio in k_dp_round)
	for (size_t k = 0; k < cu.size(); ++k) {
		out[k] = cu[k].u;
		if (kn.unit_prio) out[k].prio = cu[k].cost * 2 >= cost_max ? 3 : cu[k].cost * 4 >= cost_max ? 2 : cu[k].cost * 10 >= cost_max ? 1 : 0;   // (MPA_DP_PRIO=0: measurement)
	}
	P.n_units = cu.size(), P.sz.units = cu.size() * sizeof(DpUnit);
	return MPA_OK;
}

// (MPA_DP_TOP) what bounds the round: the costliest units by kind.  The four-wave groups of the 129..256-column checkpointed class run
// next to the round, in k_lite_wide: listed by the same cost model, as kind U_LITE_W4, so that the longest unit of the traceback round
// is seen whichever kernel sweeps it.  Empty when the round has no unit.
std::string dp_plan_top(const DpPlan &P, const DpPlanKnobs &kn)
{
	std::vector<Cost> shown = unit_costs(P, kn);
	if (shown.empty()) return "";
	for (int k = 0; k < P.lite_w4.cnt; ++k) shown.push_back(Cost{ (int64_t)P.ewaves[P.lite_w4.first + k].max_nl * NS_LITE_W4, DpUnit{ U_LITE_W4, P.lite_w4.first + k, 1, 0, 1, 0, 0, 0 } });
	std::stable_sort(shown.begin(), shown.end(), costlier);
	int64_t by_kind[U_KIND_COUNT] = { 0 }, n_kind[U_KIND_COUNT] = { 0 };
	for (const Cost &c : shown) by_kind[c.u.kind] += c.cost, ++n_kind[c.u.kind];
	char b[128];
	snprintf(b, sizeof(b), "[mpa-dp-top] units %zu; longest:", shown.size());
	std::string t = b;
	for (size_t k = 0; k < shown.size() && k < 6; ++k) snprintf(b, sizeof(b), " kind %d %.1f ms;", shown[k].u.kind, shown[k].cost * 1e-6), t += b;
	t += " | wave-ms by kind:";
	for (int k = 0; k < U_KIND_COUNT; ++k) if (n_kind[k]) snprintf(b, sizeof(b), " %d: %ld units %.0f ms;", k, (long)n_kind[k], by_kind[k] * 1e-6), t += b;
	return t + "\n";
}

// ---- bytes of every device pool; sections of the pinned staging block and of the download block
static void size_buffers(DpPlan &P, int64_t n, size_t round_args_bytes)
{
	const size_t N = (size_t)n, n_glob = P.glob_ids.size(), n_ew = P.ewaves.size();
	DpPlan::Pools &z = P.sz;
	z.tasks = sizeof(DTask) * N, z.chunks = sizeof(PrepChunk) * (P.prep.size() + 1), z.qseq = (size_t)P.q_bytes + 16, z.rec = (size_t)P.rec_total * 4, z.prof = (size_t)P.prof_total * 2 + 16;
	z.waves = sizeof(ExtWave) * (n_ew + 1), z.extout = sizeof(ExtOut) * N, z.tb = (size_t)P.tb_max * 2 + 16, z.cig = (size_t)P.cig_total * 4 + 16, z.ncig = N * 4;
	z.lite = (size_t)P.lite_total * 4 + 256, z.ckpt = (size_t)P.ck_total * 4 + 256, z.wlist = P.n_lite * 4 + 128, z.score = N * 4;
	z.rowkey = (size_t)(P.n_wide_groups * 2 * P.key_stride * 4 + 64), z.bnd = (size_t)P.bnd_total * 16 + 16;
	z.hkey = (size_t)P.hkey_total * 8 + 16 + (sizeof(GlobWave) + 4) * (P.huge_ids.size() + 1);         // keys, then one GlobWave and one list entry per call
	z.list = N * 4 + 128 + sizeof(GlobWave) * (n_glob + 1);                                            // a chunk's call list, then its waves
	z.xg = P.n_split ? P.xg_bytes + P.xg_tail + 64 : 0;
	auto al256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
	DpPlan::Up &u = P.up;
	u.tasks = 0, u.chunks = u.tasks + al256(sizeof(DTask) * N), u.q = u.chunks + al256(sizeof(PrepChunk) * P.prep.size());
	u.waves = u.q + al256((size_t)P.q_bytes), u.list = u.waves + al256(sizeof(ExtWave) * n_ew);
	u.gw = u.list + al256(4 * n_glob), u.units = u.gw + al256(sizeof(GlobWave) * (n_glob + 8));
	u.off = u.units + al256(sizeof(DpUnit) * (4 * n_ew + n_glob + 64));
	u.ids = u.off + al256(8 * n_glob), u.args = u.ids + al256(4 * n_glob), u.wl = u.args + al256(round_args_bytes);
	u.end = u.wl + al256(4 * P.n_lite);
	DpPlan::Down &d = P.dn;
	d.eo = 0, d.sc = d.eo + al256(sizeof(ExtOut) * N), d.nc = d.sc + al256(4 * N), d.err = d.nc + al256(4 * N), d.wb = d.err + 256, d.end = d.wb + 256;
}

// ---- the statistics that follow from the plan (cells = (nl-2) * 8*ceil(al/8); algorithmic bytes per call)
void dp_plan_stats(DpPlan &P)
{
	mpa_dp_stats_t &st = P.stats = mpa_dp_stats_t();
	const bool round = P.n_units > 0;
	for (int32_t id : P.ext_ids) {
		const DTask &t = P.tasks[id];
		const int64_t cells = (int64_t)std::max(0, t.nl - 2) * t.ncol;
		if (round && t.cls != X_HUGE) st.cells_ext_round += cells;
		st.n_ext++, st.cells_ext += cells;
		st.alg_bytes_ext += (t.nl + 1) / 2 + t.al + 12;
	}
	for (size_t gi = 0; gi < P.glob_ids.size(); ++gi) {
		const DTask &t = P.tasks[P.glob_ids[gi]];
		const int64_t cells = (int64_t)std::max(0, t.nl - 2) * t.ncol;
		// (the first traceback chunk rides in the round's launch, except the 512/1024-thread classes)
		if (round && ((!P.chunks.empty() && gi < P.chunks[0].last && t.cls != T_W8 && t.cls != T_W16) || gi >= P.n_reg_glob)) st.cells_glob_round += cells;
		st.n_glob++, st.cells_glob += cells;
		if (t.cls == T_LITE_W4) st.n_ckpt_wide++, st.cells_ckpt_wide += cells;
		else if (is_checkpointed(t.cls)) st.n_ckpt++, st.cells_ckpt += cells;
		st.alg_bytes_glob += (t.nl + 1) / 2 + t.al + 12 + 2 * cells + 2 * ((int64_t)t.nl + t.al);   // (+ 4 B per CIGAR word: the executor adds them)
	}
	st.rows_prep = P.rec_total;
}

int dp_plan(const mpa_dp_task_t *in, int64_t n, const int64_t *ctg_len, size_t ctg_stride, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn,
            size_t round_args_bytes, DpPlan &P)
{
	P = DpPlan();
	memset(&P.pen, 0, sizeof(P.pen));
	if (n < 0) n = 0;
	if (classify(P, in, n, ctg_len, ctg_stride, n_ctg, q, opt, kn)) return P.rc;
	auto by_class_then_len = [&P](int32_t a, int32_t b) {
		const DTask &x = P.tasks[a], &y = P.tasks[b];
		return x.cls != y.cls ? x.cls < y.cls : x.nl != y.nl ? x.nl > y.nl : a < b;
	};
	std::sort(P.ext_ids.begin(), P.ext_ids.end(), by_class_then_len);
	std::sort(P.glob_ids.begin(), P.glob_ids.end(), by_class_then_len);
	lay_out_pools(P, kn);
	pack_waves(P);
	if (build_pen_table(opt->ie_coef, std::max(P.max_nl_ext, 2), &P.pen) < 0) return refuse(P, MPA_ERR_UNSUPPORTED, "ie_coef produces too many penalty steps");
	plan_tb_chunks(P, kn);
	P.q_bytes = q->q_off[q->n_seq] - q->q_off[0];
	size_buffers(P, n, round_args_bytes);
	P.round_has_glob = !P.chunks.empty() && !P.wide_ge;        // the first chunk's calls ride in the round's one launch
	return MPA_OK;
}

int64_t dp_plan_serialize(DpPlan &P, const DpPlanKnobs &kn, void *buf, int64_t cap)
{
	// the stages the executor runs behind its uploads
	for (size_t ri = 0; ri < P.chunks.size(); ++ri) dp_plan_chunk_waves(P, ri);
	std::vector<DpUnit> units((P.up.off - P.up.units) / sizeof(DpUnit));
	if (dp_plan_units(P, kn, units.data())) return P.rc;
	units.resize(P.n_units);
	dp_plan_stats(P);
	std::vector<int64_t> h;
	auto H = [&h](int64_t v) { h.push_back(v); };
	H((int64_t)P.tasks.size()), H((int64_t)P.ext_ids.size()), H((int64_t)P.glob_ids.size()), H((int64_t)P.n_reg_glob), H((int64_t)P.n_lite), H((int64_t)P.prep.size()), H((int64_t)P.ewaves.size());
	H((int64_t)P.chunks.size()), H((int64_t)P.n_units), H((int64_t)P.n_group), H((int64_t)P.huge_ids.size()), H(P.wide_ge), H(P.round_has_glob);
	H(P.max_nl), H(P.max_nl_ext), H(P.rec_total), H(P.rec_pad), H(P.prof_total), H(P.cig_total), H(P.bnd_total), H(P.hkey_total), H(P.lite_total), H(P.ck_total), H(P.tb_max);
	H(P.key_stride), H(P.n_wide_groups), H(P.n_split), H(P.n_bound), H((int64_t)P.xg_bytes), H((int64_t)P.xg_tail), H(P.q_bytes);
	for (const WaveRange &r : P.ext) H(r.first);
	for (const WaveRange &r : P.ext) H(r.cnt);
	H(P.ext128.first), H(P.ext128.cnt);
	for (const WaveRange &r : P.lite) H(r.first);
	for (const WaveRange &r : P.lite) H(r.cnt);
	H(P.lite_w4.first), H(P.lite_w4.cnt);
	const DpPlan::Pools &z = P.sz;
	for (size_t v : { z.tasks, z.chunks, z.qseq, z.rec, z.prof, z.waves, z.extout, z.tb, z.cig, z.ncig, z.lite, z.ckpt, z.wlist, z.score, z.rowkey, z.bnd, z.hkey, z.list, z.xg, z.units }) H((int64_t)v);
	const DpPlan::Up &u = P.up;
	for (size_t v : { u.tasks, u.chunks, u.q, u.waves, u.list, u.gw, u.units, u.off, u.ids, u.args, u.wl, u.end }) H((int64_t)v);
	const DpPlan::Down &d = P.dn;
	for (size_t v : { d.eo, d.sc, d.nc, d.err, d.wb, d.end }) H((int64_t)v);
	const mpa_dp_stats_t &st = P.stats;
	for (int64_t v : { st.n_ext, st.n_glob, st.cells_ext, st.cells_glob, st.alg_bytes_ext, st.alg_bytes_glob, st.rows_prep, st.n_ckpt, st.cells_ckpt, st.n_ckpt_wide, st.cells_ckpt_wide,
	                   st.cells_ext_round, st.cells_glob_round }) H(v);
	// the sections, in upload order
	std::vector<int64_t> chunk_tab;
	std::vector<int32_t> glist;
	std::vector<GlobWave> gwaves;
	for (const DpTbChunk &r : P.chunks) {
		for (int64_t v : { (int64_t)r.first, (int64_t)r.last, r.tb_words, (int64_t)r.waves.size() }) chunk_tab.push_back(v);
		for (const WaveRange &c : r.cls) chunk_tab.push_back(c.first);
		for (const WaveRange &c : r.cls) chunk_tab.push_back(c.cnt);
		glist.insert(glist.end(), r.list.begin(), r.list.end());
		gwaves.insert(gwaves.end(), r.waves.begin(), r.waves.end());
	}
	struct Sec { const void *p; size_t bytes; };
	const Sec secs[] = {
		{ P.tasks.data(), P.tasks.size() * sizeof(DTask) }, { P.prep.data(), P.prep.size() * sizeof(PrepChunk) }, { P.ewaves.data(), P.ewaves.size() * sizeof(ExtWave) },
		{ &P.pen, sizeof(PenTable) }, { chunk_tab.data(), chunk_tab.size() * 8 }, { glist.data(), glist.size() * 4 }, { gwaves.data(), gwaves.size() * sizeof(GlobWave) },
		{ units.data(), units.size() * sizeof(DpUnit) }, { P.glob_ids.data() + P.n_reg_glob, P.n_lite * 4 }, { P.n_lite ? P.walk_cnt : nullptr, P.n_lite ? sizeof(P.walk_cnt) : 0 },
		{ P.huge_waves.data(), P.huge_waves.size() * sizeof(GlobWave) }, { P.huge_ids.data(), P.huge_ids.size() * 4 } };
	size_t at = (h.size() + 2 * (sizeof(secs) / sizeof(secs[0]))) * 8;
	for (const Sec &s : secs) H((int64_t)at), H((int64_t)s.bytes), at += (s.bytes + 7) & ~(size_t)7;
	if (buf && (int64_t)at <= cap) {
		memset(buf, 0, at);
		memcpy(buf, h.data(), h.size() * 8);
		size_t k = h.size() - 2 * (sizeof(secs) / sizeof(secs[0]));
		for (const Sec &s : secs) { if (s.bytes) memcpy((char*)buf + h[k], s.p, s.bytes); k += 2; }
	}
	return (int64_t)at;
}

} // namespace mpa
