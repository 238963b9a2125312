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
	const DpPlanOpt o = dp_plan_opt(opt);
	if (!dp_opt_supported(o))
		return refuse(P, MPA_ERR_UNSUPPORTED, "DP parameters outside the supported range (go <= 32000, ge, fs <= 16000, 0 <= xdrop <= 32000, 0 <= end_bonus <= 1000)");
	P.wide_ge = dp_wide_ge(o);
	const char *too_wide = ": too wide for this gap-extension penalty (columns x ge must stay below 2^19 in the int32 sweeps)";
	P.tasks.assign((size_t)n, DTask{});
	auto len_of = [ctg_len, ctg_stride](int32_t c) { return *(const int64_t*)((const char*)ctg_len + (size_t)c * ctg_stride); };
	for (int64_t k = 0; k < n; ++k) {
		bool is_ext = false;
		switch (dp_classify_call(in[k], (int32_t)k, n_ctg, len_of, q->n_seq, q->q_off, o, kn, P.tasks[(size_t)k], &is_ext)) {      // (the rules: dp_plan_core.h)
		case DP_CALL_MALFORMED: return refuse(P, MPA_ERR_ARG, "malformed DP task");
		case DP_CALL_OUTSIDE: return refuse(P, MPA_ERR_ARG, "DP task " + std::to_string(k) + " reaches outside its contig or its query");
		case DP_CALL_EXT_TOO_WIDE: case DP_CALL_GLOB_TOO_WIDE: return refuse(P, MPA_ERR_UNSUPPORTED, "DP call " + std::to_string(k) + too_wide);
		case DP_CALL_NO_CIGAR: return refuse(P, MPA_ERR_UNSUPPORTED, "global DP without CIGAR is not part of miniprot's path");
		default: break;
		}
		if (is_ext) P.ext_ids.push_back((int32_t)k), P.max_nl_ext = std::max(P.max_nl_ext, in[k].nl), ++P.ext_calls[P.tasks[(size_t)k].cls];
		else P.glob_ids.push_back((int32_t)k);
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

// the descriptors of an extension class
static const WaveRange &ext_range(const DpPlan &P, int cls) { return cls == X_128 ? P.ext128 : cls >= X_SPLIT8 ? P.ext_wide[cls - X_SPLIT8] : P.ext[cls]; }

static void pack_waves(DpPlan &P)
{
	const std::vector<DTask> &T = P.tasks;
	size_t p = 0;
	for (int cls = X_16; cls <= X_SPLIT4; ++cls) P.ext[cls] = pack_ext_class(P, P.ext_ids, p, cls, ext_calls_per_wave(cls), false);
	// X_SPLIT8 / X_SPLIT12 sort behind X_HUGE and X_128; their descriptors follow X_SPLIT4's, so that the wide groups stay neighbours (row keys)
	size_t pw = p + P.huge_ids.size();
	while (pw < P.ext_ids.size() && T[P.ext_ids[pw]].cls == X_128) ++pw;
	for (int cls = X_SPLIT8; cls <= X_SPLIT12; ++cls) P.ext_wide[cls - X_SPLIT8] = pack_ext_class(P, P.ext_ids, pw, cls, ext_calls_per_wave(cls), false);
	for (size_t h = 0; h < P.huge_ids.size();) P.huge_waves.push_back(pack_wave<GlobWave>(T, P.huge_ids, h, P.huge_ids.size(), 1));
	p += P.huge_ids.size();                                     // (X_HUGE sorts between X_SPLIT4 and X_128)
	P.ext128 = pack_ext_class(P, P.ext_ids, p, X_128, ext_calls_per_wave(X_128), false);
	while (P.n_reg_glob < P.glob_ids.size() && !is_checkpointed(T[P.glob_ids[P.n_reg_glob]].cls)) ++P.n_reg_glob;
	P.n_lite = P.glob_ids.size() - P.n_reg_glob;
	p = P.n_reg_glob;
	for (int cls = T_LITE16; cls <= T_LITE128; ++cls) P.lite[cls - T_LITE16] = pack_ext_class(P, P.glob_ids, p, cls, lite_calls_per_wave(cls), true);
	P.lite_w4 = pack_ext_class(P, P.glob_ids, p, T_LITE_W4, lite_calls_per_wave(T_LITE_W4), true);   // pools sized by the group's longest call
	P.lite_w8 = pack_ext_class(P, P.glob_ids, p, T_LITE_W8, lite_calls_per_wave(T_LITE_W8), true);
	for (int c = 0; c < 5; ++c) P.walk_cnt[c] = 0;
	P.walk_cnt_w8 = 0;
	for (size_t k = P.n_reg_glob; k < P.glob_ids.size(); ++k) {
		const int cls = T[P.glob_ids[k]].cls;
		if (cls == T_LITE_W8) ++P.walk_cnt_w8;
		else ++P.walk_cnt[cls - T_LITE16];
	}
	// per-row keys of the wide extension kernels: [group][2 halves][key_stride]
	for (int k = X_W2; k < kNumExtPacked + kNumExtWide; ++k) {
		const WaveRange &r = ext_range(P, ext_class_at(k));
		for (int j = 0; j < r.cnt; ++j) P.key_stride = std::max<int64_t>(P.key_stride, P.ewaves[r.first + j].max_nl), ++P.n_wide_groups;
	}
	P.key_stride = (P.key_stride + 64) & ~(int64_t)63;
	// split classes: boundary granules (16 B per row and boundary: n_blk - 1 boundaries per group -- 11, 7, 3, 1 for 3072, 2048, 1024, 512 columns),
	// then the per-group completion counters and the error flag
	for (int k = 0; k < kNumExtSplit; ++k) {
		const int cls = ext_split_at(k);
		P.n_split += ext_range(P, cls).cnt, P.n_bound += (int64_t)ext_range(P, cls).cnt * (dp_ext_unit_blocks(cls) - 1);
	}
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
	r.n_list = r.list.size(), r.n_waves = r.waves.size();
}

// ---- the units of the round: the extension waves/groups of every class, the packed sweeps of the checkpointed calls and
// (round_has_glob) the plain traceback waves of the first chunk; longest first
// cost model, kinds and how many neighbours share a unit: dp_plan_core.h
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
	const bool pool = kn.pool != 0;
	auto add_ext = [&](int cls, const WaveRange &r) { add_range(dp_ext_unit_kind(cls, pool), r, dp_ext_unit_per(cls, pool), dp_ext_unit_ns(cls)); };
	for (int cls = X_16; cls <= X_64; ++cls)
		if (!(cls == X_32 && kn.antidiag)) add_ext(cls, P.ext[cls]);
	add_ext(X_W2, P.ext[X_W2]);
	add_ext(X_W4, P.ext[X_W4]);
	int sgroup = 0, xg = 0;                                       // split groups and their boundaries are numbered widest class first
	for (int c = 0; c < kNumExtSplit; ++c) {
		const int cls = ext_split_at(c), n_blk = dp_ext_unit_blocks(cls);
		const WaveRange &r = ext_range(P, cls);
		for (int k = 0; k < r.cnt; ++k, ++sgroup, xg += n_blk - 1)
			for (int b = 0; b < n_blk; ++b) add(dp_ext_unit_kind(cls, pool), r.first + k, 1, (int64_t)P.ewaves[r.first + k].max_nl * dp_ext_unit_ns(cls), b, n_blk, sgroup, xg);
	}
	add_ext(X_128, P.ext128);
	for (int c = 0; c < 4; ++c) add_range(dp_lite_unit_kind(T_LITE16 + c), P.lite[c], dp_per_narrow(pool), dp_lite_unit_ns(T_LITE16 + c));
	if (P.round_has_glob) {
		const DpTbChunk &r = P.chunks[0];
		for (int cls = T_16; cls <= T_MB; ++cls) {
			if (!dp_glob_in_round(cls)) continue;                    // (the 512/1024-thread classes keep their own launch)
			const int kind = dp_glob_unit_kind(cls, pool), per = dp_glob_unit_per(cls, pool);
			for (int k = 0; k < r.cls[cls].cnt; k += per) {
				const GlobWave &g = r.waves[r.cls[cls].first + k];
				add(kind, r.cls[cls].first + k, std::min(per, r.cls[cls].cnt - k), dp_glob_unit_cost(cls, g.max_nl, P.tasks[g.task[0]].ncol));
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
	for (size_t k = 0; k < cu.size(); ++k) {
		out[k] = cu[k].u;
		if (kn.unit_prio) out[k].prio = dp_unit_prio(cu[k].cost, cost_max);   // (MPA_DP_PRIO=0: measurement)
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
	// (k_lite_w8's groups likewise; their rows have not been measured: the four-wave groups' constant stands in)
	for (int k = 0; k < P.lite_w8.cnt; ++k) shown.push_back(Cost{ (int64_t)P.ewaves[P.lite_w8.first + k].max_nl * NS_LITE_W4, DpUnit{ U_LITE_W8, P.lite_w8.first + k, 1, 0, 1, 0, 0, 0 } });
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
	const size_t N = (size_t)n, n_glob = P.cnt.n_glob, n_ew = P.cnt.n_ewaves, n_prep = P.cnt.n_prep, n_huge = P.cnt.n_huge;
	DpPlan::Pools &z = P.sz;
	z.tasks = sizeof(DTask) * N, z.chunks = sizeof(PrepChunk) * (n_prep + 1), z.qseq = (size_t)P.q_bytes + 16, z.rec = (size_t)P.rec_total * 4, z.prof = (size_t)P.prof_total * 2 + 16;
	z.waves = sizeof(ExtWave) * (n_ew + 1), z.extout = sizeof(ExtOut) * N, z.tb = (size_t)P.tb_max * 2 + 16, z.cig = (size_t)P.cig_total * 4 + 16, z.ncig = N * 4;
	z.lite = (size_t)P.lite_total * 4 + 256, z.ckpt = (size_t)P.ck_total * 4 + 256, z.wlist = P.n_lite * 4 + 128, z.score = N * 4;
	z.rowkey = (size_t)(P.n_wide_groups * 2 * P.key_stride * 4 + 64), z.bnd = (size_t)P.bnd_total * 16 + 16;
	z.hkey = (size_t)P.hkey_total * 8 + 16 + (sizeof(GlobWave) + 4) * (n_huge + 1);         // keys, then one GlobWave and one list entry per call
	z.list = N * 4 + 128 + sizeof(GlobWave) * (n_glob + 1);                                            // a chunk's call list, then its waves
	z.xg = P.n_split ? P.xg_bytes + P.xg_tail + 64 : 0;
	auto al256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
	DpPlan::Up &u = P.up;
	u.tasks = 0, u.chunks = u.tasks + al256(sizeof(DTask) * N), u.q = u.chunks + al256(sizeof(PrepChunk) * n_prep);
	u.waves = u.q + al256((size_t)P.q_bytes), u.list = u.waves + al256(sizeof(ExtWave) * n_ew);
	u.gw = u.list + al256(4 * n_glob), u.units = u.gw + al256(sizeof(GlobWave) * (n_glob + 8));
	u.off = u.units + al256(sizeof(DpUnit) * (4 * n_ew + n_glob + 64 + 4 * (size_t)P.ext_wide[0].cnt + 8 * (size_t)P.ext_wide[1].cnt));   // (8 / 12 units per X_SPLIT8 / X_SPLIT12 group)
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
		if (t.cls == T_LITE_W4 || t.cls == T_LITE_W8) st.n_ckpt_wide++, st.cells_ckpt_wide += cells;   // (the classes of a group of waves per pair of calls)
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
		return dp_call_before(x.cls, x.nl, a, y.cls, y.nl, b);
	};
	std::sort(P.ext_ids.begin(), P.ext_ids.end(), by_class_then_len);
	std::sort(P.glob_ids.begin(), P.glob_ids.end(), by_class_then_len);
	lay_out_pools(P, kn);
	pack_waves(P);
	if (build_pen_table(opt->ie_coef, std::max(P.max_nl_ext, 2), &P.pen) < 0) return refuse(P, MPA_ERR_UNSUPPORTED, "ie_coef produces too many penalty steps");
	plan_tb_chunks(P, kn);
	P.q_bytes = q->q_off[q->n_seq] - q->q_off[0];
	P.cnt = DpPlan::Counts{ (size_t)n, P.ext_ids.size(), P.glob_ids.size(), P.prep.size(), P.ewaves.size(), P.huge_ids.size() };
	size_buffers(P, n, round_args_bytes);
	P.round_has_glob = !P.chunks.empty() && !P.wide_ge;        // the first chunk's calls ride in the round's one launch
	return MPA_OK;
}

int64_t dp_plan_serialize(DpPlan &P, const DpPlanKnobs &kn, void *buf, int64_t cap, bool wide, bool w8)
{
	// the stages the executor runs behind its uploads
	for (size_t ri = 0; ri < P.chunks.size(); ++ri) dp_plan_chunk_waves(P, ri);
	std::vector<DpUnit> units((P.up.off - P.up.units) / sizeof(DpUnit));
	if (dp_plan_units(P, kn, units.data())) return P.rc;
	units.resize(P.n_units);
	dp_plan_stats(P);
	return dp_plan_write(P, units, buf, cap, wide, w8);
}

int64_t dp_plan_write(const DpPlan &P, const std::vector<DpUnit> &units, void *buf, int64_t cap, bool wide, bool w8)
{
	std::vector<int64_t> h;
	auto H = [&h](int64_t v) { h.push_back(v); };
	H((int64_t)P.tasks.size()), H((int64_t)P.cnt.n_ext), H((int64_t)P.glob_ids.size()), H((int64_t)P.n_reg_glob), H((int64_t)P.n_lite), H((int64_t)P.prep.size()), H((int64_t)P.ewaves.size());
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
	// (mpa_dbg_dp_plan_wide) behind everything else: first and count of X_SPLIT8 and of X_SPLIT12, the boundary count
	const int64_t tail[5] = { P.ext_wide[0].first, P.ext_wide[0].cnt, P.ext_wide[1].first, P.ext_wide[1].cnt, P.n_bound };
	// (mpa_dbg_dp_plan_w8) behind those: first and count of T_LITE_W8's descriptors, the calls of its walk list
	const int64_t tail_w8[3] = { P.lite_w8.first, P.lite_w8.cnt, P.walk_cnt_w8 };
	const size_t total = at + (wide ? sizeof(tail) : 0) + (w8 ? sizeof(tail_w8) : 0);
	if (buf && (int64_t)total <= cap) {
		memset(buf, 0, total);
		memcpy(buf, h.data(), h.size() * 8);
		size_t k = h.size() - 2 * (sizeof(secs) / sizeof(secs[0]));
		for (const Sec &s : secs) { if (s.bytes) memcpy((char*)buf + h[k], s.p, s.bytes); k += 2; }
		if (wide) memcpy((char*)buf + at, tail, sizeof(tail));
		if (w8) memcpy((char*)buf + at + (wide ? sizeof(tail) : 0), tail_w8, sizeof(tail_w8));
	}
	return (int64_t)total;
}

// ---- the device planner's host side: what it declines, the plan from its header, the model
const char *dp_plan_device_declines(const mpa_dpopt_t *opt, const DpPlanKnobs &kn, int64_t n)
{
	const DpPlanOpt o = dp_plan_opt(opt);
	if (!dp_opt_supported(o)) return "options the planner refuses";
	if (dp_wide_ge(o)) return "gap extension or frameshift above 255";
	if (kn.pool) return "the worker pool";
	if (kn.antidiag) return "the anti-diagonal measurement switch";
	if (kn.no_split) return "a repeated round";
	if (n <= 0 || n > MPA_DPPLAN_MAX_N) return "no calls, or more than 2^20";
	return nullptr;
}

int64_t dp_plan_prep_bound(const mpa_dp_task_t *in, int64_t n, int64_t *max_nl, int64_t *max_al)
{
	int64_t chunks = 0, mnl = 0, mal = 0;
	for (int64_t k = 0; k < n; ++k) {
		const int64_t nl = in[k].nl > 0 ? in[k].nl : 0;
		chunks += (nl + MPA_PREP_CHUNK_ROWS - 1) / MPA_PREP_CHUNK_ROWS, mnl = std::max(mnl, nl), mal = std::max<int64_t>(mal, in[k].al);
	}
	*max_nl = mnl, *max_al = mal;
	return chunks;
}

int dp_plan_from_head(const DpDevHead &H, const int32_t *glob_ids, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn, size_t round_args_bytes, DpPlan &P)
{
	P = DpPlan();
	memset(&P.pen, 0, sizeof(P.pen));
	P.on_device = true;
	if (H.status & DPP_REFUSED) return refuse(P, MPA_ERR_UNSUPPORTED, "a call the planner refuses");
	if (H.status & DPP_HUGE) return refuse(P, MPA_ERR_UNSUPPORTED, "a call of the one-wave int32 extension class");
	if (H.status & DPP_LITE_W8) return refuse(P, MPA_ERR_UNSUPPORTED, "a call of the eight-wave checkpointed traceback class");
	if (H.n_reg_glob > 1 && (size_t)H.tb_max * 2 > (size_t)kn.tb_budget) return refuse(P, MPA_ERR_UNSUPPORTED, "more than one traceback chunk");
	P.cnt = DpPlan::Counts{ (size_t)H.n, (size_t)H.n_ext, (size_t)H.n_glob, (size_t)H.n_prep, (size_t)H.n_ewaves, 0 };
	P.glob_ids.assign(glob_ids, glob_ids + H.n_glob);
	P.n_reg_glob = (size_t)H.n_reg_glob, P.n_lite = (size_t)H.n_lite;
	for (int c = 0; c < kNumExtPacked; ++c) P.ext[c] = WaveRange{ (int)H.ew_first[c], (int)H.ew_cnt[c] };
	for (int c = 0; c < kNumExtWide; ++c) P.ext_wide[c] = WaveRange{ (int)H.ew_first[DPP_EW_SPLIT8 + c], (int)H.ew_cnt[DPP_EW_SPLIT8 + c] };
	P.ext128 = WaveRange{ (int)H.ew_first[DPP_EW_128], (int)H.ew_cnt[DPP_EW_128] };
	for (int c = 0; c < 4; ++c) P.lite[c] = WaveRange{ (int)H.ew_first[DPP_EW_LITE + c], (int)H.ew_cnt[DPP_EW_LITE + c] };
	P.lite_w4 = WaveRange{ (int)H.ew_first[DPP_EW_LITE + 4], (int)H.ew_cnt[DPP_EW_LITE + 4] };
	for (int c = 0; c < 5; ++c) P.walk_cnt[c] = (int32_t)H.walk_cnt[c];
	for (int g = 0; g < 16; ++g) P.ext_calls[g] = H.run_cnt[g];
	P.max_nl = (int32_t)H.max_nl, P.max_nl_ext = (int32_t)H.max_nl_ext;
	P.rec_total = H.rec_total, P.rec_pad = H.rec_pad, P.prof_total = H.prof_total, P.cig_total = H.cig_total, P.bnd_total = H.bnd_total, P.hkey_total = 0;
	P.lite_total = H.lite_total, P.ck_total = H.ck_total, P.tb_max = H.tb_max;
	P.key_stride = H.key_stride, P.n_wide_groups = H.n_wide_groups, P.n_split = H.n_split, P.n_bound = H.n_bound;
	P.xg_bytes = (size_t)P.n_bound * P.key_stride * 16, P.xg_tail = (2 * (size_t)P.n_split + 1) * 4;
	if (build_pen_table(opt->ie_coef, std::max(P.max_nl_ext, 2), &P.pen) < 0) { P.on_device = false; return refuse(P, MPA_ERR_UNSUPPORTED, "ie_coef produces too many penalty steps"); }
	if (H.n_reg_glob > 0) {
		DpTbChunk r;
		r.first = 0, r.last = (size_t)H.n_reg_glob, r.tb_words = H.tb_max, r.n_list = (size_t)H.n_reg_glob, r.n_waves = (size_t)H.n_gw;
		for (int c = 0; c < 8; ++c) r.cls[c] = WaveRange{ (int)H.gw_first[c], (int)H.gw_cnt[c] };
		P.chunks.push_back(r);
	}
	P.q_bytes = q->q_off[q->n_seq] - q->q_off[0];
	size_buffers(P, H.n, round_args_bytes);
	P.round_has_glob = !P.chunks.empty();
	P.n_units = (size_t)H.n_units, P.n_group = 0, P.sz.units = P.n_units * sizeof(DpUnit);
	if (sizeof(DpUnit) * P.n_units > P.up.off - P.up.units) return refuse(P, MPA_ERR_HIP, "internal: more DP units than the staging buffer holds");
	// the statistics (dp_plan_stats): sums of the classify stage
	mpa_dp_stats_t &st = P.stats = mpa_dp_stats_t();
	const bool round = P.n_units > 0;
	st.n_ext = H.n_ext, st.n_glob = H.n_glob, st.cells_ext = H.st[DPP_ST_CELLS_EXT], st.cells_glob = H.st[DPP_ST_CELLS_GLOB];
	st.alg_bytes_ext = H.st[DPP_ST_BYTES_EXT], st.alg_bytes_glob = H.st[DPP_ST_BYTES_GLOB], st.rows_prep = P.rec_total;
	st.n_ckpt = H.st[DPP_ST_N_CKPT], st.cells_ckpt = H.st[DPP_ST_CELLS_CKPT], st.n_ckpt_wide = H.st[DPP_ST_N_WIDE], st.cells_ckpt_wide = H.st[DPP_ST_CELLS_WIDE];
	st.cells_ext_round = round ? st.cells_ext : 0, st.cells_glob_round = round ? st.cells_glob - H.st[DPP_ST_CELLS_OWN] : 0;
	return MPA_OK;
}

int dp_plan_model(const mpa_dp_task_t *in, int64_t n, const int64_t *ctg_len, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn,
                  size_t round_args_bytes, DpPlan &P, std::vector<DpUnit> &units)
{
	P = DpPlan();
	if (const char *why = dp_plan_device_declines(opt, kn, n)) return refuse(P, MPA_ERR_UNSUPPORTED, why);
	int64_t max_nl = 0, max_al = 0;
	const int64_t prep_bound = dp_plan_prep_bound(in, n, &max_nl, &max_al);
	if (!dp_unit_costs_fit(max_nl, max_al)) return refuse(P, MPA_ERR_UNSUPPORTED, "unit costs that do not fit the sort key");
	// the pools at the bounds the driver uses (dev_dp_plan), the scratch a team of one needs
	const size_t N = (size_t)n, U = (size_t)dp_units_bound(n, kn.split_wide != 0);
	std::vector<DTask> tasks(N);
	std::vector<PrepChunk> chunks((size_t)prep_bound + 1);
	std::vector<ExtWave> waves(N + 16);
	std::vector<int32_t> list(N), wlist(N), gids(N);
	std::vector<GlobWave> gw(N);
	std::vector<DpUnit> out(U), ubuf(U);
	std::vector<uint64_t> key(N), skey, ukey(U), uskey;
	std::vector<DpSums> bsum(N);
	DpDevHead H;
	memset(&H, 0, sizeof(H));
	DpDevPlan D;
	D.n = n, D.n_ubound = (int64_t)U, D.n_ctg = n_ctg, D.n_seq = q->n_seq, D.opt = dp_plan_opt(opt), D.kn = kn, D.raw = in, D.q_off = q->q_off, D.ctg_len = ctg_len;
	D.tasks = tasks.data(), D.chunks = chunks.data(), D.waves = waves.data(), D.list = list.data(), D.gw = gw.data(), D.units = out.data(), D.wlist = wlist.data();
	D.key = key.data(), D.bsum = bsum.data(), D.ubuf = ubuf.data(), D.ukey = ukey.data(), D.gids = gids.data(), D.head = &H;
	const TeamOne one;
	for (int64_t b = 0; b < n; ++b) dpp_classify(one, D, b);
	skey = key, std::sort(skey.begin(), skey.end()), D.skey = skey.data();
	for (int64_t b = 0; b < n; ++b) dpp_sums(one, D, b);
	dpp_mid(one, D);
	for (int64_t b = 0; b < n; ++b) dpp_layout(one, D, b);
	for (int64_t b = 0; b < (int64_t)U; ++b) dpp_units(one, D, b);
	uskey = ukey, std::sort(uskey.begin(), uskey.end()), D.uskey = uskey.data();
	for (int64_t b = 0; b < H.n_units; ++b) dpp_units_out(one, D, b);
	if (dp_plan_from_head(H, gids.data(), q, opt, kn, round_args_bytes, P)) return P.rc;
	// what the device would have left in the pools
	P.tasks = tasks, P.prep.assign(chunks.begin(), chunks.begin() + H.n_prep), P.ewaves.assign(waves.begin(), waves.begin() + H.n_ewaves);
	if (!P.chunks.empty()) P.chunks[0].list.assign(list.begin(), list.begin() + H.n_reg_glob), P.chunks[0].waves.assign(gw.begin(), gw.begin() + H.n_gw);
	P.ext_ids.resize((size_t)H.n_ext);
	for (int64_t p = 0; p < H.n_ext; ++p) P.ext_ids[(size_t)p] = dp_key_call(skey[(size_t)p]);
	units.assign(out.begin(), out.begin() + H.n_units);
	return MPA_OK;
}

} // namespace mpa
