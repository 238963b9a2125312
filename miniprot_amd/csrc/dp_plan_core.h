// dp_plan_core.h -- what the planner of a DP round knows about ONE call and ONE unit, and the stages of the device planner (DESIGN.md
// section 4.11).  Host and device compile the same text: dp_plan.cpp (the host planner, and the model: the stages with a team of one)
// and dp_plan_kernels.hip (the stages with a 256-lane workgroup as team).  No HIP, no std:: containers, no globals.
#pragma once
#include <cstdint>
#include "../../include/mpamd.h"
#include "dp_device.h"

#define MPA_DPP_HD __host__ __device__ static inline

namespace mpa {

// ---- what a class means for packing (DpClass, dp_device.h)
static const int kNumExtPacked = 7;                                   // X_16 .. X_SPLIT4: the classes of the packed int16 sweeps every plan may hold, in ascending width
static const int kNumExtWide = 2;                                     // X_SPLIT8, X_SPLIT12: the same sweep over 8 / 12 workgroups (DpPlanKnobs::split_wide)
// the packed classes in ascending width: X_16 .. X_SPLIT4, X_SPLIT8, X_SPLIT12 (k = 0 .. kNumExtPacked + kNumExtWide - 1); X_128 is X_W2's other shape
MPA_DPP_HD int ext_class_at(int k) { return k < kNumExtPacked ? k : (int)X_SPLIT8 + (k - kNumExtPacked); }
MPA_DPP_HD bool ext_is_split(int cls) { return cls == X_SPLIT2 || cls == X_SPLIT4 || cls == X_SPLIT8 || cls == X_SPLIT12; }   // workgroups hand column blocks over through HBM
MPA_DPP_HD bool ext_is_wide_group(int cls) { return cls == X_W2 || cls == X_W4 || ext_is_split(cls); }        // a group of waves per pair of calls, with per-row keys
MPA_DPP_HD int ext_lanes(int cls) { return cls == X_16 ? 16 : cls == X_32 ? 32 : 64; }                       // lanes per call
MPA_DPP_HD int ext_waves(int cls)                                                                            // waves per group: 1, 1, 1, 2, 4, 8, 16; 32, 48
{
	return cls == X_SPLIT8 ? 32 : cls == X_SPLIT12 ? 48 : cls <= X_64 || cls == X_128 ? 1 : 1 << (cls - X_64);
}
MPA_DPP_HD int ext_columns(int cls) { return cls == X_128 ? 128 : ext_lanes(cls) * ext_waves(cls); }         // columns the class covers (= profile row width)
MPA_DPP_HD int ext_calls_per_wave(int cls) { return cls == X_128 ? 1 : 2 * (64 / ext_lanes(cls)); }          // ... per wave or group: two calls per lane
// the narrowest class that covers ncol columns; split_wide: X_SPLIT8 / X_SPLIT12 beyond 1024 columns, else X_HUGE
MPA_DPP_HD int ext_class_of(int32_t ncol, bool split_wide = false)
{
	for (int k = 0; k < kNumExtPacked + (split_wide ? kNumExtWide : 0); ++k) if (ncol <= ext_columns(ext_class_at(k))) return ext_class_at(k);
	return X_HUGE;
}
MPA_DPP_HD int tb_class_of(int32_t ncol) { int c = T_16; while (c < T_MB && ncol > (16 << c)) ++c; return c; }   // 16, 32, ... 1024 columns, then block-major
MPA_DPP_HD int tb_calls_per_wave(int cls) { return cls == T_16 ? 4 : cls == T_32 ? 2 : 1; }                  // the plain traceback sweep: one call per group of lanes
MPA_DPP_HD int lite_columns(int cls) { return 16 << (cls - T_LITE16); }                                      // 16, 32, 64, 128, 256, 512
MPA_DPP_HD int lite_calls_per_wave(int cls) { return cls == T_LITE128 ? 1 : cls == T_LITE_W4 || cls == T_LITE_W8 ? 2 : 2 * (64 / lite_columns(cls)); }
// dwords of extension bits / checkpoints of one packed-sweep descriptor whose longest call has max_nl rows (layout: dp_device.h)
MPA_DPP_HD int64_t lite_bits_dwords(int cls, int32_t max_nl)
{
	return cls == T_LITE_W8 ? lite_group_bits_dwords(MPA_LITE_W8_WAVES, max_nl) : cls == T_LITE_W4 ? lite_wide_bits_dwords(max_nl) : ((int64_t)max_nl / 3 + 2) * 64;
}
MPA_DPP_HD int64_t lite_ckpt_dwords(int cls, int32_t max_nl)
{
	return cls == T_LITE_W8 ? lite_group_ckpt_dwords(MPA_LITE_W8_WAVES, max_nl) : cls == T_LITE_W4 ? lite_wide_ckpt_dwords(max_nl) : (int64_t)(max_nl > 3 ? (max_nl - 3) / MPA_TB_BLOCK : 0) * 9 * 64;
}

// values the executor has when it plans (the environment is read by the executor: at context creation, or once per process)
struct DpPlanKnobs {
	int32_t lite_min = 384, lite_wide = 0;      // checkpointed traceback: from this many rows; 129..256 columns included
	int32_t lite_w8 = 0;                        // ... 257..512 columns included (MPA_DP_LITE_W8; independent of lite_wide; not with the pool)
	int32_t no_split = 0;                       // repeated round: no inter-workgroup hand-off
	int32_t split_wide = 0;                     // MPA_DP_SPLIT_WIDE: 1025..3072-column extension calls on X_SPLIT8 / X_SPLIT12 (not with the pool, not in a repeated round)
	int32_t antidiag = 0;                       // (measurement) the 32-column extension class runs on k_ext_antidiag
	int32_t pool = 0;                           // the worker pool takes the round's units (MPA_DP_POOL)
	int32_t ext_dual = 1, unit_prio = 1;        // MPA_DP_EXT_DUAL, MPA_DP_PRIO
	int64_t tb_budget = (int64_t)8 << 30;       // bytes of traceback matrix per chunk
};

// ---- the per-call rules of classify()
// An extension call of fewer than three rows has no row to sweep (the first swept row is row 2): the reference fails its own assertion
// there (nasw-sse.c:441), and with assertions compiled out it returns (nt_len 0, aa_len al + 1, score INT32_MIN).  That triple is this
// operator's contract (include/mpamd.h).  The planner gives such a call the class X_NONE -- no wave descriptor, no unit, no kernel ever
// sees it -- and dp_result_of() (dp_results_core.h) writes the triple, on the host and on the device.
MPA_DPP_HD bool dp_ext_unswept(int32_t flag, int32_t nl) { return (flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) != 0 && nl < 3; }
// the scalar options a call's class depends on; max_mat: the largest entry of the scoring matrix
struct DpPlanOpt { int32_t go, ge, fs, xdrop, end_bonus, max_mat; };
MPA_DPP_HD DpPlanOpt dp_plan_opt(const mpa_dpopt_t *opt)
{
	int32_t max_mat = 0;
	for (int k = 0; k < 484; ++k) max_mat = max_mat > opt->mat[k] ? max_mat : opt->mat[k];
	return DpPlanOpt{ opt->go, opt->ge, opt->fs, opt->xdrop, opt->end_bonus, max_mat };
}
// parameter guards: outside these the packed-int16 kernels would not be bit-exact
MPA_DPP_HD bool dp_opt_supported(const DpPlanOpt &o)
{
	return !(o.go < 0 || o.go > 32000 || o.ge < 0 || o.ge > 16000 || o.fs < 0 || o.fs > 16000 || o.xdrop < 0 || o.xdrop > 32000 ||
	         o.end_bonus < 0 || o.end_bonus > 1000 || (o.ge > 255 && o.go + o.ge > 32000));
}
// Gap-extension / frameshift penalties above 255 (-E / -F of the reference's command line, main.c:133,136) do not fit the byte
// the row records give them.  Such a run keeps the records' layout -- the byte then flags a stop codon -- and sweeps every call
// with the kernels that read it that way (glob_cands<K, true>): the stand-alone traceback kernels and, for extension calls,
// the block-major one-wave sweep (k_ext_huge); the packed round kernel is not used.  Slow, exact, and nobody's default.
MPA_DPP_HD bool dp_wide_ge(const DpPlanOpt &o) { return o.ge > 255 || o.fs > 255; }

// why a call is refused (0: it is not)
enum DpRefusal : int32_t { DP_CALL_OK = 0, DP_CALL_MALFORMED, DP_CALL_OUTSIDE, DP_CALL_EXT_TOO_WIDE, DP_CALL_GLOB_TOO_WIDE, DP_CALL_NO_CIGAR };

// One call: the DTask without its offsets, its class and profile width.  ctg_len(c): the length of contig c; q_off: the batch's query
// offsets (n_seq + 1).  *is_ext: an extension call (else a traceback call).  Returns a DpRefusal; t is complete only for DP_CALL_OK.
template<typename CtgLen>
MPA_DPP_HD int dp_classify_call(const mpa_dp_task_t &x, int32_t k, int32_t n_ctg, CtgLen ctg_len, int32_t n_seq, const int64_t *q_off, const DpPlanOpt &o, const DpPlanKnobs &kn,
                            DTask &t, bool *is_ext)
{
	*is_ext = (x.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) != 0;
	if (x.nl < 0 || x.al <= 0 || x.qid < 0 || x.qid >= n_seq || x.io < 0 || x.io > 32000) return DP_CALL_MALFORMED;
	// the kernels address the resident genome and the query buffer with these: a window or a protein slice that leaves its
	// contig / its query would read foreign memory (or fault the context), so it is refused here
	if (x.vid < 0 || x.vid >= 2 * n_ctg || x.nt_off < 0 || x.nt_off + (int64_t)x.nl > ctg_len(x.vid >> 1) ||
	    x.aa_off < 0 || (int64_t)x.aa_off + x.al > q_off[x.qid + 1] - q_off[x.qid])
		return DP_CALL_OUTSIDE;
	const bool wide_ge = dp_wide_ge(o);
	t.nt_off = x.nt_off, t.vid = x.vid, t.nl = x.nl, t.al = x.al, t.flag = x.flag, t.io = x.io;
	t.q_off = q_off[x.qid] + x.aa_off - q_off[0];     // relative to the slice the executor uploads
	t.ncol = (x.al + 7) / 8 * 8;
	t.out_idx = k;
	// (the int32 sweeps keep the striped reference's lane segments apart by offsets of 2^20 in their scans: column * ge must stay
	// below; checked where it matters: the traceback sweeps and the block-major extension sweep)
	const bool seg_overflow = (int64_t)t.ncol * o.ge >= (1 << 19);
	// The packed int16 kernels run their gap scan on h + j*ge with saturating adds and hold go + j*ge in int16, which is only the
	// reference's value while nothing can reach the int16 limits.  Calls that could -- with BLOSUM62 and ge = 1 more than ~2900
	// columns, always of the huge class; with a large -E or -O already at a few dozen columns -- go to the int32 sweeps, which
	// clamp every operation like the reference does: k_ext_huge for extension calls, the plain traceback sweep for the others.
	const bool may_saturate = (int64_t)x.al * o.max_mat + (int64_t)t.ncol * o.ge + (o.end_bonus > 0 ? o.end_bonus : 0) > 32000 || o.go + (int64_t)t.ncol * o.ge > 32000;
	const bool packed_ok = !wide_ge && !may_saturate;
	if (*is_ext) {
		int cls = ext_class_of(t.ncol, kn.split_wide && !kn.pool && !kn.no_split);
		if (kn.no_split && ext_is_split(cls)) cls = X_HUGE;         // repeated round: no inter-workgroup hand-off (see mpa_dp_run)
		if (!packed_ok) cls = X_HUGE;
		if (cls == X_HUGE && seg_overflow) return DP_CALL_EXT_TOO_WIDE;
		t.pw = cls == X_HUGE ? t.ncol : ext_columns(cls);
		// 65..128 columns: one wave per call instead of a two-wave group per pair of calls (MPA_DP_EXT_DUAL=0: the two-wave groups)
		if (cls == X_W2 && kn.ext_dual && !kn.antidiag) cls = X_128;
		if (dp_ext_unswept(x.flag, x.nl)) cls = X_NONE;             // nothing to sweep: answered by the result rule (the refusals above stay)
		t.cls = cls;
	} else {
		if (!(x.flag & MPA_F_CIGAR)) return DP_CALL_NO_CIGAR;
		if (seg_overflow) return DP_CALL_GLOB_TOO_WIDE;
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
		// 257..512 columns under the same predicate with lite_w8 (MPA_DP_LITE_W8=1, a knob of its own): an eight-wave group per pair of calls
		else if (many_rows && t.cls == T_W8 && kn.lite_w8 && !kn.pool) t.cls = T_LITE_W8, t.pw = lite_columns(T_LITE_W8);
	}
	return DP_CALL_OK;
}

// ---- the order of the calls of one list: class ascending, rows descending, index ascending
MPA_DPP_HD bool dp_call_before(int32_t x_cls, int32_t x_nl, int32_t a, int32_t y_cls, int32_t y_nl, int32_t b)
{
	return x_cls != y_cls ? x_cls < y_cls : x_nl != y_nl ? x_nl > y_nl : a < b;
}
// ... as one unique 64-bit key for n <= 2^20 (nl >= 0): every extension call before every traceback call.  g = the list and the class
#define MPA_DPPLAN_MAX_N ((int64_t)1 << 20)
#define MPA_DPPLAN_KEY_BITS 56
MPA_DPP_HD int dp_key_group(bool is_ext, int32_t cls) { return is_ext ? cls : 16 + cls; }                     // < 32
MPA_DPP_HD uint64_t dp_call_key(bool is_ext, int32_t cls, int32_t nl, int32_t k)
{
	return (uint64_t)dp_key_group(is_ext, cls) << 51 | (uint64_t)(0x7fffffff - nl) << 20 | (uint32_t)k;
}
MPA_DPP_HD int32_t dp_key_call(uint64_t key) { return (int32_t)(key & 0xfffff); }
MPA_DPP_HD int dp_key_g(uint64_t key) { return (int)(key >> 51); }

// ---- the units of a round (unit_costs() of dp_plan.cpp)
// cost model: nanoseconds per row of a unit's longest call, by kind (measured: profiles/r06_dp_ns_per_row.txt, r06_wide_ns_per_row.txt)
enum : int64_t { NS_EXT_NARROW = 160, NS_EXT_WIDE = 270, NS_EXT_SPLIT = 310, NS_EXT128 = 200, NS_LITE = 170, NS_LITE128 = 200, NS_LITE_W4 = 280, NS_GLOB = 430, NS_GLOB_WIDE = 510 };
// (worker pool: the one-wave kinds are units of ONE wave descriptor each, taken by single waves; without the pool a
// workgroup's four waves take four neighbours of the sorted list)
MPA_DPP_HD int dp_per_narrow(bool pool) { return pool ? 1 : 4; }
// an extension class X_16 .. X_SPLIT4, X_128, X_SPLIT8, X_SPLIT12: the kind of its units, how many neighbouring descriptors share one, nanoseconds per row
// (worker pool: a workgroup goes on to its next unit, so all four waves must leave a unit through the same barriers -- a
// 65..128-column group then takes a whole workgroup on the four-wave body, its waves 2 and 3 on dead columns)
MPA_DPP_HD int dp_ext_unit_kind(int cls, bool pool)
{
	return cls <= X_64 ? U_EXT16 + cls : cls == X_W2 ? (pool ? (int)U_EXT_W4 : (int)U_EXT_W2) : cls == X_W4 ? (int)U_EXT_W4 : cls == X_128 ? (int)U_EXT128 : (int)U_EXT_SPLIT;
}
MPA_DPP_HD int dp_ext_unit_per(int cls, bool pool) { return cls <= X_64 || cls == X_128 ? dp_per_narrow(pool) : cls == X_W2 ? (pool ? 1 : 2) : 1; }
// (X_SPLIT8 / X_SPLIT12 take NS_EXT_SPLIT: profiles/split_wide_ns_per_row.txt has 294-299 ns per row for a lone pair of them next to 293 for
// the 1024-column groups in the same run, whose constant this is)
MPA_DPP_HD int64_t dp_ext_unit_ns(int cls) { return cls <= X_64 ? NS_EXT_NARROW : cls <= X_W4 ? NS_EXT_WIDE : cls == X_128 ? NS_EXT128 : NS_EXT_SPLIT; }
MPA_DPP_HD int dp_ext_unit_blocks(int cls) { return ext_is_split(cls) ? ext_waves(cls) / 4 : 1; }              // workgroups (units) per group: 2, 4, 8, 12
// the split classes in the order their groups and boundaries are numbered, widest first (k = 0 .. 3)
static const int kNumExtSplit = 4;
MPA_DPP_HD int ext_split_at(int k) { return k == 0 ? (int)X_SPLIT12 : k == 1 ? (int)X_SPLIT8 : k == 2 ? (int)X_SPLIT4 : (int)X_SPLIT2; }
// the packed sweeps of the checkpointed classes T_LITE16 .. T_LITE128 (T_LITE_W4 has its own launch)
MPA_DPP_HD int dp_lite_unit_kind(int cls) { return U_LITE16 + (cls - T_LITE16); }
MPA_DPP_HD int64_t dp_lite_unit_ns(int cls) { return cls == T_LITE128 ? NS_LITE128 : NS_LITE; }
// the plain sweeps of the first traceback chunk, T_16 .. T_MB
MPA_DPP_HD bool dp_glob_in_round(int cls) { return cls != T_W8 && cls != T_W16; }                            // (the 512/1024-thread classes keep their own launch)
MPA_DPP_HD int dp_glob_unit_kind(int cls, bool pool) { return cls <= T_64 ? U_GLOB16 + cls : cls == T_MB ? (int)U_GLOB_MB : cls == T_W4 || pool ? (int)U_GLOB_W4 : (int)U_GLOB_W2; }
MPA_DPP_HD int dp_glob_unit_per(int cls, bool pool) { return cls == T_W2 ? (pool ? 1 : 2) : cls == T_W4 ? 1 : dp_per_narrow(pool); }
MPA_DPP_HD int64_t dp_glob_unit_cost(int cls, int32_t max_nl, int32_t ncol_first)
{
	int64_t cost = (int64_t)max_nl * (cls == T_W2 || cls == T_W4 ? NS_GLOB_WIDE : NS_GLOB);
	if (cls == T_MB) cost *= (ncol_first + 63) / 64;
	return cost;
}
// the units that bound the round's duration issue ahead of the short ones they share a SIMD with (s_setprio in k_dp_round)
MPA_DPP_HD int32_t dp_unit_prio(int64_t cost, int64_t cost_max) { return cost * 2 >= cost_max ? 3 : cost * 4 >= cost_max ? 2 : cost * 10 >= cost_max ? 1 : 0; }

// =====================================================================================================================================
// The device planner: the stages of DESIGN.md section 4.11.  A stage is called by every member of a team with the number of its block;
// member r of block b works on item b * Team::W + r.  What a team must offer:
//   W (members), rank(), sync() (a barrier that also orders the team's memory), exscan<K>(v, total) (v becomes the sum of the members
//   before this one, total the team's sum, in every member), add(dst, v) (adds the TEAM's sum of v to *dst: every member calls it),
//   flag(dst, bits) (ors bits into *dst: any member, any time).
// TeamOne below is the host's; the device's is a workgroup (dp_plan_kernels.hip).
template<int K> struct DpVec { int64_t v[K]; };

struct TeamOne {
	static const int W = 1;
	int rank() const { return 0; }
	void sync() const {}
	template<int K> void exscan(DpVec<K> &v, DpVec<K> &total) const { total = v; for (int k = 0; k < K; ++k) v.v[k] = 0; }
	void add(int64_t *dst, int64_t v) const { *dst += v; }
	void flag(int64_t *dst, int64_t bits) const { *dst |= bits; }
};

enum : int64_t { DPP_REFUSED = 1, DPP_HUGE = 2, DPP_LITE_W8 = 4 };   // DpDevHead::status: a call the host planner refuses; a call of class X_HUGE; of class T_LITE_W8
enum { DPP_S_REC = 0, DPP_S_PROF, DPP_S_PREP, DPP_S_CIG, DPP_S_BND, DPP_S_TB, DPP_NSUM };                 // what the layout scans, in sorted order
enum { DPP_ST_CELLS_EXT = 0, DPP_ST_BYTES_EXT, DPP_ST_CELLS_GLOB, DPP_ST_BYTES_GLOB, DPP_ST_N_CKPT, DPP_ST_CELLS_CKPT, DPP_ST_N_WIDE, DPP_ST_CELLS_WIDE, DPP_ST_CELLS_OWN, DPP_NST };
typedef DpVec<DPP_NSUM> DpSums;

// wave descriptor classes in the order of ExtWave[]: X_16 .. X_SPLIT4, X_SPLIT8, X_SPLIT12, X_128, T_LITE16 .. T_LITE128, T_LITE_W4
// (the wide groups X_W2 .. X_SPLIT12 are neighbours: their row keys are indexed by descriptor, from the first X_W2 group)
#define MPA_DPPLAN_EW 15
enum { DPP_EW_SPLIT8 = 7, DPP_EW_SPLIT12 = 8, DPP_EW_128 = 9, DPP_EW_LITE = 10 };
MPA_DPP_HD int dp_ew_ext_class(int e) { return e < 7 ? e : e == DPP_EW_SPLIT8 ? (int)X_SPLIT8 : e == DPP_EW_SPLIT12 ? (int)X_SPLIT12 : (int)X_128; }   // e < DPP_EW_LITE
MPA_DPP_HD int dp_ew_of_ext_class(int cls) { return cls < 7 ? cls : cls == X_SPLIT8 ? (int)DPP_EW_SPLIT8 : cls == X_SPLIT12 ? (int)DPP_EW_SPLIT12 : cls == X_128 ? (int)DPP_EW_128 : -1; }
MPA_DPP_HD int dp_ew_group(int e) { return e < DPP_EW_LITE ? dp_key_group(true, dp_ew_ext_class(e)) : dp_key_group(false, T_LITE16 + (e - DPP_EW_LITE)); }
MPA_DPP_HD int dp_ew_of_group(int g) { return g < 16 ? dp_ew_of_ext_class(g) : g >= 16 + T_LITE16 && g <= 16 + T_LITE_W4 ? DPP_EW_LITE + (g - 16 - T_LITE16) : -1; }   // -1: no ExtWave class
MPA_DPP_HD int dp_ew_per(int e) { return e < DPP_EW_LITE ? ext_calls_per_wave(dp_ew_ext_class(e)) : lite_calls_per_wave(T_LITE16 + (e - DPP_EW_LITE)); }

// one run of units that are built alike (unit_costs() adds them in this order)
struct DpUnitSeg {
	int32_t kind, first, cnt, per;              // descriptors [first, first + cnt), `per` neighbours share a unit
	int32_t n_blk, sgroup0, xg0, xg_step;       // split groups: units per group; number and first boundary of the segment's first group; boundaries per group
	int32_t glob_cls;                           // >= 0: GlobWave descriptors of this traceback class (cost by dp_glob_unit_cost)
	int32_t cpw;                                // calls per descriptor
	int64_t ns, pos0, ufirst;                   // nanoseconds per row; sorted position of the first descriptor's first call; first unit
};
#define MPA_DPPLAN_SEGS 24

// What the planner leaves besides the pools: counts, totals, ranges.  All int64 so that the block is one array for the download.
struct DpDevHead {
	int64_t status;
	int64_t run_first[32], run_cnt[32];         // the sorted list by dp_key_group: positions [first, first + cnt)
	int64_t tot[DPP_NSUM];
	int64_t st[DPP_NST];                        // statistics sums (dp_plan_stats)
	int64_t n, n_ext, n_glob, n_reg_glob, n_lite, n_prep, n_ewaves, n_gw, n_units;
	int64_t max_nl, max_nl_ext, rec_total, rec_pad, prof_total, cig_total, bnd_total, lite_total, ck_total, tb_max;
	int64_t key_stride, n_wide_groups, n_split, n_bound;
	int64_t ew_first[MPA_DPPLAN_EW], ew_cnt[MPA_DPPLAN_EW];
	int64_t gw_first[8], gw_cnt[8];
	int64_t walk_cnt[5];
	int64_t n_seg, cost_max;
	DpUnitSeg seg[MPA_DPPLAN_SEGS];
};

// the unit order as one unique key: cost descending, construction index ascending
#define MPA_DPPLAN_COST_BITS 39
#define MPA_DPPLAN_UNIT_BITS 24
MPA_DPP_HD uint64_t dp_unit_key(int64_t cost, int64_t u) { return (uint64_t)((((int64_t)1 << MPA_DPPLAN_COST_BITS) - 1) - cost) << MPA_DPPLAN_UNIT_BITS | (uint64_t)u; }
MPA_DPP_HD int64_t dp_unit_key_cost(uint64_t key) { return (((int64_t)1 << MPA_DPPLAN_COST_BITS) - 1) - (int64_t)(key >> MPA_DPPLAN_UNIT_BITS); }
MPA_DPP_HD int64_t dp_unit_key_index(uint64_t key) { return (int64_t)(key & (((uint64_t)1 << MPA_DPPLAN_UNIT_BITS) - 1)); }
// the largest cost a unit of calls with at most max_nl rows and max_al residues can have: the planner declines when it does not fit the key
MPA_DPP_HD bool dp_unit_costs_fit(int64_t max_nl, int64_t max_al)
{
	const int64_t blocks = (max_al + 7 + 63) / 64 + 1;
	return max_nl < ((int64_t)1 << 31) && max_nl * NS_GLOB_WIDE * blocks < ((int64_t)1 << MPA_DPPLAN_COST_BITS);
}
// units a round of n calls can have at most (the executor's staging section has the same bound: 4 n_ew + n_glob + 64, and with
// split_wide 8 more for every X_SPLIT12 group, 4 more for every X_SPLIT8 group)
MPA_DPP_HD int64_t dp_units_bound(int64_t n, bool split_wide = false) { return (split_wide ? 12 : 4) * n + 64; }

// everything the stages read and write
struct DpDevPlan {
	int64_t n, n_ubound;                        // calls; entries of ubuf / ukey / uskey (dp_units_bound: the unit sort is sized before the plan is known)
	int32_t n_ctg, n_seq;
	DpPlanOpt opt;
	DpPlanKnobs kn;
	const mpa_dp_task_t *raw;                   // [n]
	const int64_t *q_off, *ctg_len;             // [n_seq + 1], [n_ctg]
	// the executor's pools
	DTask *tasks; PrepChunk *chunks; ExtWave *waves; int32_t *list; GlobWave *gw; DpUnit *units; int32_t *wlist;
	// scratch: call keys unsorted / sorted, block sums, units in construction order, unit keys unsorted / sorted
	uint64_t *key, *skey; DpSums *bsum; DpUnit *ubuf; uint64_t *ukey, *uskey;
	int32_t *gids;                              // [n_glob] the sorted traceback calls (plain sweep, then checkpointed): for the host
	DpDevHead *head;
};
MPA_DPP_HD int64_t dp_blocks(int64_t items, int w) { return (items + w - 1) / w; }

// ---- stage 1, classify: one member per call
template<typename Team> MPA_DPP_HD void dpp_classify(const Team &tm, const DpDevPlan &D, int64_t b)
{
	const int64_t k = b * Team::W + tm.rank();
	int64_t st[DPP_NST];
	for (int i = 0; i < DPP_NST; ++i) st[i] = 0;
	if (k < D.n) {
		DTask t = DTask();
		bool is_ext = true;
		const int64_t *cl = D.ctg_len;
		const int why = dp_classify_call(D.raw[k], (int32_t)k, D.n_ctg, [cl](int32_t c) { return cl[c]; }, D.n_seq, D.q_off, D.opt, D.kn, t, &is_ext);
		if (why != DP_CALL_OK) {                                 // (the host planner will say why: a harmless call takes its place in the later stages)
			tm.flag(&D.head->status, DPP_REFUSED);
			t = DTask(), t.al = 1, t.ncol = 8, t.pw = 16, t.cls = X_16, t.out_idx = (int32_t)k, is_ext = true;
		}
		if (is_ext && t.cls == X_HUGE) tm.flag(&D.head->status, DPP_HUGE);
		// (the later stages do not know the eight-wave checkpointed class: the round goes to the host planner, and until the host has
		// seen the flag the call stands in the stages as the plain T_W8 call it would be without the knob)
		if (!is_ext && t.cls == T_LITE_W8) tm.flag(&D.head->status, DPP_LITE_W8), t.cls = T_W8, t.pw = t.ncol;
		D.tasks[k] = t;
		D.key[k] = dp_call_key(is_ext, t.cls, t.nl, (int32_t)k);
		// the statistics that follow from the plan (cells = (nl-2) * 8*ceil(al/8); algorithmic bytes per call)
		const int64_t cells = (int64_t)(t.nl > 2 ? t.nl - 2 : 0) * t.ncol;
		if (is_ext) st[DPP_ST_CELLS_EXT] = cells, st[DPP_ST_BYTES_EXT] = (t.nl + 1) / 2 + t.al + 12;
		else {
			st[DPP_ST_CELLS_GLOB] = cells, st[DPP_ST_BYTES_GLOB] = (t.nl + 1) / 2 + t.al + 12 + 2 * cells + 2 * ((int64_t)t.nl + t.al);
			if (t.cls == T_LITE_W4) st[DPP_ST_N_WIDE] = 1, st[DPP_ST_CELLS_WIDE] = cells;
			else if (is_checkpointed(t.cls)) st[DPP_ST_N_CKPT] = 1, st[DPP_ST_CELLS_CKPT] = cells;
			if (!dp_glob_in_round(t.cls)) st[DPP_ST_CELLS_OWN] = cells;
		}
	}
	for (int i = 0; i < DPP_NST; ++i) tm.add(&D.head->st[i], st[i]);
}

// what the call at sorted position p adds to the six running sums
MPA_DPP_HD DpSums dpp_call_sums(const DTask &t, int g)
{
	DpSums s;
	for (int i = 0; i < DPP_NSUM; ++i) s.v[i] = 0;
	s.v[DPP_S_REC] = t.nl, s.v[DPP_S_PROF] = (int64_t)22 * t.pw, s.v[DPP_S_PREP] = (t.nl + MPA_PREP_CHUNK_ROWS - 1) / MPA_PREP_CHUNK_ROWS;
	if (g >= 16) {
		s.v[DPP_S_CIG] = (int64_t)t.nl + t.al + 4;
		if (t.cls == T_MB) s.v[DPP_S_BND] = t.nl;
		if (!is_checkpointed(t.cls)) s.v[DPP_S_TB] = (int64_t)t.nl * t.ncol;
	}
	return s;
}

// ---- stage 2, behind the sort: the runs of the sorted list and every block's sums
template<typename Team> MPA_DPP_HD void dpp_sums(const Team &tm, const DpDevPlan &D, int64_t b)
{
	const int64_t p = b * Team::W + tm.rank();
	DpSums s, total;
	for (int i = 0; i < DPP_NSUM; ++i) s.v[i] = 0;
	if (p < D.n) {
		const uint64_t key = D.skey[p];
		const int g = dp_key_g(key);
		s = dpp_call_sums(D.tasks[dp_key_call(key)], g);
		if (p == 0 || dp_key_g(D.skey[p - 1]) != g) D.head->run_first[g] = p;
		if (p == D.n - 1 || dp_key_g(D.skey[p + 1]) != g) D.head->run_cnt[g] = p + 1;   // (the run's end: dpp_head takes the first off)
	}
	tm.exscan(s, total);
	if (tm.rank() == 0) D.bsum[b] = total;
}

// rows of the call at sorted position p
MPA_DPP_HD int32_t dpp_nl_at(const DpDevPlan &D, int64_t p) { return D.tasks[dp_key_call(D.skey[p])].nl; }

// ---- stage 3 (ONE team): the block sums scanned; counts, ranges and totals; the checkpointed descriptors' bit words and checkpoints
template<typename Team> MPA_DPP_HD void dpp_mid(const Team &tm, const DpDevPlan &D)
{
	DpDevHead &H = *D.head;
	const int64_t nb = dp_blocks(D.n, Team::W);
	DpSums carry;
	for (int i = 0; i < DPP_NSUM; ++i) carry.v[i] = 0;
	for (int64_t b0 = 0; b0 < nb; b0 += Team::W) {
		const int64_t b = b0 + tm.rank();
		DpSums s, total;
		for (int i = 0; i < DPP_NSUM; ++i) s.v[i] = 0;
		if (b < nb) s = D.bsum[b];
		tm.exscan(s, total);
		for (int i = 0; i < DPP_NSUM; ++i) s.v[i] += carry.v[i], carry.v[i] += total.v[i];
		if (b < nb) D.bsum[b] = s;
	}
	if (tm.rank() == 0) {
		for (int i = 0; i < DPP_NSUM; ++i) H.tot[i] = carry.v[i];
		for (int g = 0; g < 32; ++g) if (H.run_cnt[g]) H.run_cnt[g] -= H.run_first[g];
		H.n = D.n, H.n_ext = H.n_glob = H.n_reg_glob = H.n_lite = 0, H.max_nl = H.max_nl_ext = 0;
		for (int g = 0; g < 32; ++g) {
			if (!H.run_cnt[g]) continue;
			const int64_t nl = dpp_nl_at(D, H.run_first[g]);              // (a run starts with its longest call)
			H.max_nl = H.max_nl > nl ? H.max_nl : nl;
			if (g < 16) H.n_ext += H.run_cnt[g], H.max_nl_ext = H.max_nl_ext > nl ? H.max_nl_ext : nl;
			else if (is_checkpointed(g - 16)) H.n_lite += H.run_cnt[g], H.walk_cnt[g - 16 - T_LITE16] = H.run_cnt[g];
			else H.n_reg_glob += H.run_cnt[g];
		}
		H.n_glob = H.n_reg_glob + H.n_lite;
		H.n_prep = H.tot[DPP_S_PREP], H.prof_total = H.tot[DPP_S_PROF], H.cig_total = H.tot[DPP_S_CIG], H.bnd_total = H.tot[DPP_S_BND], H.tb_max = H.tot[DPP_S_TB];
		H.rec_pad = H.max_nl + 96 + (D.kn.antidiag ? 64 : 0);        // kernels prefetch records up to 48 rows past a call's end (the anti-diagonal prototype: 128)
		H.rec_total = H.tot[DPP_S_REC] + H.rec_pad;
		// wave descriptors by class; per-row keys of the wide extension kernels: [group][2 halves][key_stride]
		int64_t at = 0;
		H.key_stride = 0, H.n_wide_groups = 0;
		for (int e = 0; e < MPA_DPPLAN_EW; ++e) {
			const int g = dp_ew_group(e);
			H.ew_first[e] = at, H.ew_cnt[e] = dp_blocks(H.run_cnt[g], dp_ew_per(e)), at += H.ew_cnt[e];
			if (e < DPP_EW_LITE && ext_is_wide_group(dp_ew_ext_class(e)) && H.ew_cnt[e]) {
				const int64_t nl = dpp_nl_at(D, H.run_first[g]);
				H.key_stride = H.key_stride > nl ? H.key_stride : nl, H.n_wide_groups += H.ew_cnt[e];
			}
		}
		H.n_ewaves = at;
		H.key_stride = (H.key_stride + 64) & ~(int64_t)63;
		// split classes: boundary granules (n_blk - 1 boundaries per group: 11, 7, 3, 1)
		H.n_split = H.n_bound = 0;
		for (int k = 0; k < kNumExtSplit; ++k) {
			const int64_t cnt = H.ew_cnt[dp_ew_of_ext_class(ext_split_at(k))];
			H.n_split += cnt, H.n_bound += cnt * (dp_ext_unit_blocks(ext_split_at(k)) - 1);
		}
		// the waves of the plain sweep's one chunk, by class
		at = 0;
		for (int c = T_16; c <= T_MB; ++c) H.gw_first[c] = at, H.gw_cnt[c] = dp_blocks(H.run_cnt[16 + c], tb_calls_per_wave(c)), at += H.gw_cnt[c];
		H.n_gw = at;
		// the unit segments, in the order of construction
		int ns = 0;
		int64_t u = 0;
		const bool pool = D.kn.pool != 0;
		auto ext_seg = [&](int e, int kind, int per, int64_t nanos) {
			if (!H.ew_cnt[e]) return;
			DpUnitSeg &S = H.seg[ns++];
			S.kind = kind, S.first = (int32_t)H.ew_first[e], S.cnt = (int32_t)H.ew_cnt[e], S.per = per, S.n_blk = 1, S.sgroup0 = S.xg0 = S.xg_step = 0, S.glob_cls = -1;
			S.cpw = dp_ew_per(e), S.ns = nanos, S.pos0 = H.run_first[dp_ew_group(e)], S.ufirst = u;
			u += dp_blocks(S.cnt, per);
		};
		for (int cls = X_16; cls <= X_64; ++cls)
			if (!(cls == X_32 && D.kn.antidiag)) ext_seg(cls, dp_ext_unit_kind(cls, pool), dp_ext_unit_per(cls, pool), dp_ext_unit_ns(cls));
		ext_seg(X_W2, dp_ext_unit_kind(X_W2, pool), dp_ext_unit_per(X_W2, pool), dp_ext_unit_ns(X_W2));
		ext_seg(X_W4, dp_ext_unit_kind(X_W4, pool), dp_ext_unit_per(X_W4, pool), dp_ext_unit_ns(X_W4));
		int32_t sgroup = 0, xg = 0;                                   // split groups and their boundaries are numbered widest class first
		for (int k = 0; k < kNumExtSplit; ++k) {
			const int cls = ext_split_at(k), e = dp_ew_of_ext_class(cls);
			if (!H.ew_cnt[e]) continue;
			ext_seg(e, dp_ext_unit_kind(cls, pool), 1, dp_ext_unit_ns(cls));
			DpUnitSeg &S = H.seg[ns - 1];
			S.n_blk = dp_ext_unit_blocks(cls), S.sgroup0 = sgroup, S.xg0 = xg, S.xg_step = S.n_blk - 1;
			u += (int64_t)S.cnt * (S.n_blk - 1);
			sgroup += S.cnt, xg += S.cnt * S.xg_step;
		}
		ext_seg(DPP_EW_128, dp_ext_unit_kind(X_128, pool), dp_ext_unit_per(X_128, pool), dp_ext_unit_ns(X_128));
		for (int c = 0; c < 4; ++c) ext_seg(DPP_EW_LITE + c, dp_lite_unit_kind(T_LITE16 + c), dp_per_narrow(pool), dp_lite_unit_ns(T_LITE16 + c));
		if (H.n_reg_glob > 0 && !dp_wide_ge(D.opt))                  // the first chunk's calls ride in the round's one launch
			for (int cls = T_16; cls <= T_MB; ++cls) {
				if (!dp_glob_in_round(cls) || !H.gw_cnt[cls]) continue;
				DpUnitSeg &S = H.seg[ns++];
				S.kind = dp_glob_unit_kind(cls, pool), S.first = (int32_t)H.gw_first[cls], S.cnt = (int32_t)H.gw_cnt[cls], S.per = dp_glob_unit_per(cls, pool);
				S.n_blk = 1, S.sgroup0 = S.xg0 = S.xg_step = 0, S.glob_cls = cls, S.cpw = tb_calls_per_wave(cls), S.ns = 0, S.pos0 = H.run_first[16 + cls], S.ufirst = u;
				u += dp_blocks(S.cnt, S.per);
			}
		H.n_seg = ns, H.n_units = u;
	}
	tm.sync();
	// checkpointed descriptors: a scan over their bit words and checkpoints, in descriptor order
	const int64_t d0 = H.ew_first[DPP_EW_LITE], nd = H.n_ewaves - d0;
	DpVec<2> run;
	run.v[0] = run.v[1] = 0;
	for (int64_t k0 = 0; k0 < nd; k0 += Team::W) {
		const int64_t d = d0 + k0 + tm.rank();
		DpVec<2> s, total;
		s.v[0] = s.v[1] = 0;
		if (d < H.n_ewaves) {
			int e = DPP_EW_LITE;
			while (e + 1 < MPA_DPPLAN_EW && d >= H.ew_first[e + 1]) ++e;
			const int cls = T_LITE16 + (e - DPP_EW_LITE);
			const int32_t max_nl = dpp_nl_at(D, H.run_first[16 + cls] + (d - H.ew_first[e]) * dp_ew_per(e));
			s.v[0] = lite_bits_dwords(cls, max_nl), s.v[1] = lite_ckpt_dwords(cls, max_nl);
		}
		tm.exscan(s, total);
		if (d < H.n_ewaves) D.waves[d].lite_off = run.v[0] + s.v[0], D.waves[d].ck_off = run.v[1] + s.v[1];
		run.v[0] += total.v[0], run.v[1] += total.v[1];
	}
	if (tm.rank() == 0) H.lite_total = run.v[0], H.ck_total = run.v[1];
}

// ---- stage 4, lay out: every offset of every call, the prep chunks, the wave descriptors, the lists
template<typename Team> MPA_DPP_HD void dpp_layout(const Team &tm, const DpDevPlan &D, int64_t b)
{
	const DpDevHead &H = *D.head;
	const int64_t p = b * Team::W + tm.rank();
	DpSums s, total;
	for (int i = 0; i < DPP_NSUM; ++i) s.v[i] = 0;
	int g = 0;
	int32_t id = 0;
	if (p < D.n) {
		const uint64_t key = D.skey[p];
		g = dp_key_g(key), id = dp_key_call(key);
		s = dpp_call_sums(D.tasks[id], g);
	}
	const int64_t n_prep = s.v[DPP_S_PREP];
	tm.exscan(s, total);
	if (p >= D.n) return;
	const DpSums base = D.bsum[b];
	for (int i = 0; i < DPP_NSUM; ++i) s.v[i] += base.v[i];
	DTask &t = D.tasks[id];
	t.rec_off = s.v[DPP_S_REC], t.prof_off = s.v[DPP_S_PROF];
	for (int64_t r = 0; r < n_prep; ++r) D.chunks[s.v[DPP_S_PREP] + r] = PrepChunk{ id, (int32_t)(r * MPA_PREP_CHUNK_ROWS) };
	const int64_t rel = p - H.run_first[g], cnt = H.run_cnt[g];
	if (g >= 16) {
		t.cig_cap = t.nl + t.al + 4, t.cig_off = s.v[DPP_S_CIG];
		if (t.cls == T_MB) t.bnd_off = s.v[DPP_S_BND];
		const int64_t gi = p - H.n_ext;
		D.gids[gi] = id;
		if (!is_checkpointed(t.cls)) {
			// the chunk of the plain sweep: its call list is the sorted order, its waves take neighbours of one class
			t.tb_off = s.v[DPP_S_TB];
			D.list[gi] = id;
			const int per = tb_calls_per_wave(t.cls);
			GlobWave &w = D.gw[H.gw_first[t.cls] + rel / per];
			const int slot = (int)(rel % per);
			w.task[slot] = id;
			if (slot == 0) {
				w.max_nl = t.nl, w.pad_[0] = w.pad_[1] = w.pad_[2] = 0;
				for (int j = (int)(cnt - rel < per ? cnt - rel : per); j < 4; ++j) w.task[j] = -1;
			}
		} else D.wlist[gi - H.n_reg_glob] = id;
	}
	const int e = dp_ew_of_group(g);
	if (e >= 0) {
		// descriptor k of a class takes the calls [k * per, (k + 1) * per) of the class's run; checkpointed classes: slot numbers, bit words, checkpoints
		const int per = dp_ew_per(e);
		ExtWave &w = D.waves[H.ew_first[e] + rel / per];
		const int slot = (int)(rel % per);
		w.task[slot] = id;
		if (slot == 0) {
			w.max_nl = t.nl, w.pad_[0] = w.pad_[1] = w.pad_[2] = 0, w.rec_base = t.rec_off;     // (sorted: the first call of a wave has the smallest offset)
			if (e < DPP_EW_LITE) w.lite_off = w.ck_off = 0;
			for (int j = (int)(cnt - rel < per ? cnt - rel : per); j < 8; ++j) w.task[j] = -1;
		}
		if (e >= DPP_EW_LITE) t.flag |= slot << MPA_LITE_SLOT_SHIFT, t.tb_off = w.lite_off, t.bnd_off = w.ck_off;
	}
}

// ---- stage 5, units: one member per unit, in the order of construction; its cost and its place in that order as the sort key
template<typename Team> MPA_DPP_HD void dpp_units(const Team &tm, const DpDevPlan &D, int64_t b)
{
	const DpDevHead &H = *D.head;
	const int64_t u = b * Team::W + tm.rank();
	if (u >= H.n_units) {                                       // (behind the round's units: keys that sort last)
		if (u < D.n_ubound) D.ukey[u] = ~(uint64_t)0;
		return;
	}
	int si = 0;
	while (si + 1 < H.n_seg && u >= H.seg[si + 1].ufirst) ++si;
	const DpUnitSeg &S = H.seg[si];
	const int64_t j = u - S.ufirst;
	const int32_t k = (int32_t)(S.n_blk > 1 ? j / S.n_blk : j * S.per);       // the unit's first descriptor, counted from the segment's
	const uint64_t first_key = D.skey[S.pos0 + (int64_t)k * S.cpw];
	const DTask &t0 = D.tasks[dp_key_call(first_key)];
	DpUnit out;
	out.kind = S.kind, out.first = S.first + k, out.count = S.n_blk > 1 ? 1 : (S.cnt - k < S.per ? S.cnt - k : S.per), out.prio = 0;
	out.blk = S.n_blk > 1 ? (int32_t)(j % S.n_blk) : 0, out.n_blk = S.n_blk;
	out.sgroup = S.n_blk > 1 ? S.sgroup0 + k : 0, out.xg_first = S.n_blk > 1 ? S.xg0 + S.xg_step * k : 0;
	const int64_t cost = S.glob_cls >= 0 ? dp_glob_unit_cost(S.glob_cls, t0.nl, t0.ncol) : (int64_t)t0.nl * S.ns;
	D.ubuf[u] = out;
	D.ukey[u] = dp_unit_key(cost, u);
}

// ---- stage 6, behind the unit sort: the unit list costliest first, priorities relative to the largest cost
template<typename Team> MPA_DPP_HD void dpp_units_out(const Team &tm, const DpDevPlan &D, int64_t b)
{
	DpDevHead &H = *D.head;
	const int64_t u = b * Team::W + tm.rank();
	if (u >= H.n_units) return;
	const int64_t cost_max = dp_unit_key_cost(D.uskey[0]);
	const uint64_t key = D.uskey[u];
	DpUnit out = D.ubuf[dp_unit_key_index(key)];
	if (D.kn.unit_prio) out.prio = dp_unit_prio(dp_unit_key_cost(key), cost_max);
	D.units[u] = out;
	if (u == 0) H.cost_max = cost_max;
}

} // namespace mpa
