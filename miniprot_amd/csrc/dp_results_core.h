// dp_results_core.h -- what stands behind a DP round's one wait, for the host and for the device: the rule that
// turns one call's outputs into the caller's result record, the dense CIGAR pool's offsets as an exclusive scan over the sorted traceback
// calls, and the three bounds the device planner sizes its pools by before it knows the plan.  Host and device compile the same text:
// dp_exec.hip's dp_assemble() (the rule), dp_results_kernels.hip (the stages with a 256-lane workgroup as team), span_kernels.hip (the
// bounds, one lane per task) and the model (the stages with a team of one).  No HIP, no std:: containers, no globals.
#pragma once
#include "dp_plan_core.h"

namespace mpa {

// ---- the bounds of a task list: what dp_plan_prep_bound() returns, for one task and joined
struct DpTaskBounds { int64_t prep, max_nl, max_al; };      // sum of ceil(nl / 1024); largest nl; largest al
MPA_DPP_HD DpTaskBounds dp_task_bounds_of(int32_t nl_, int32_t al)
{
	const int64_t nl = nl_ > 0 ? nl_ : 0;
	return DpTaskBounds{ (nl + MPA_PREP_CHUNK_ROWS - 1) / MPA_PREP_CHUNK_ROWS, nl, al > 0 ? (int64_t)al : 0 };
}
MPA_DPP_HD void dp_task_bounds_join(DpTaskBounds &a, const DpTaskBounds &b)
{
	a.prep += b.prep, a.max_nl = a.max_nl > b.max_nl ? a.max_nl : b.max_nl, a.max_al = a.max_al > b.max_al ? a.max_al : b.max_al;
}
// ... of n tasks with a team of one
MPA_DPP_HD DpTaskBounds dp_task_bounds(const mpa_dp_task_t *in, int64_t n)
{
	DpTaskBounds b{ 0, 0, 0 };
	for (int64_t k = 0; k < n; ++k) dp_task_bounds_join(b, dp_task_bounds_of(in[k].nl, in[k].al));
	return b;
}

// ---- the rule: call k's record from its mode and shape and from what the kernels left.  An extension call takes its lengths and score
// from its ExtOut and has no CIGAR; a traceback call covers its whole window and slice, its score and word count are the sweep's and the
// walk's, its words start at dense_off in the dense pool.  Only what the call's mode needs is read.  An extension call of fewer than three
// rows (class X_NONE: no kernel swept it, its ExtOut was never written) is (0, al + 1, INT32_MIN), the contract of include/mpamd.h.
MPA_DPP_HD mpa_dp_rst_t dp_result_of(int32_t flag, int32_t nl, int32_t al, int64_t k, const ExtOut *eo, const int32_t *sc, const int32_t *nc, int64_t dense_off)
{
	mpa_dp_rst_t o;
	if (dp_ext_unswept(flag, nl)) o.nt_len = 0, o.aa_len = al + 1, o.score = INT32_MIN, o.n_cigar = 0, o.cigar_off = 0;
	else if (flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) o.nt_len = eo[k].nt_len, o.aa_len = eo[k].aa_len, o.score = eo[k].score, o.n_cigar = 0, o.cigar_off = 0;
	else o.nt_len = nl, o.aa_len = al, o.score = sc[k], o.n_cigar = nc[k], o.cigar_off = dense_off;
	return o;
}

// ---- the stages, for a team as dp_plan_core.h describes it (W, rank(), exscan<K>())
enum { DPR_H_POOL = 0, DPR_H_BAD, DPR_NHEAD };              // the header: words of the dense pool; traceback calls whose word count is outside [0, cig_cap]
struct DpResDev {
	int64_t n, n_glob;                          // calls; traceback calls
	const DTask *tasks;                         // [n] mode and shape of every call (flag, nl, al, cig_cap)
	const int32_t *gids;                        // [n_glob] the traceback calls in the order the planner left them
	const ExtOut *eo;                           // [n]
	const int32_t *sc, *nc;                     // [n] score and CIGAR words of the traceback calls
	int64_t *off;                               // [n_glob] first word of sorted traceback call g in the dense pool
	int64_t *call_off;                          // [n] ... by call (written for traceback calls only)
	int64_t *bsum;                              // [dp_blocks(n_glob, W)] block sums, then their exclusive scan
	int64_t *head;                              // [DPR_NHEAD]
	mpa_dp_rst_t *rst;                          // [n]
};
MPA_DPP_HD int64_t dpr_words_at(const DpResDev &R, int64_t g) { return g < R.n_glob ? (int64_t)R.nc[R.gids[g]] : 0; }

// stage 1: every block's words
template<typename Team> MPA_DPP_HD void dpr_sums(const Team &tm, const DpResDev &R, int64_t b)
{
	DpVec<1> s, total;
	s.v[0] = dpr_words_at(R, b * Team::W + tm.rank());
	tm.exscan(s, total);
	if (tm.rank() == 0) R.bsum[b] = total.v[0];
}
// stage 2 (ONE team): the block sums scanned, the pool's total
template<typename Team> MPA_DPP_HD void dpr_mid(const Team &tm, const DpResDev &R)
{
	const int64_t nb = dp_blocks(R.n_glob, Team::W);
	int64_t carry = 0;
	for (int64_t b0 = 0; b0 < nb; b0 += Team::W) {
		const int64_t b = b0 + tm.rank();
		DpVec<1> s, total;
		s.v[0] = b < nb ? R.bsum[b] : 0;
		tm.exscan(s, total);
		if (b < nb) R.bsum[b] = carry + s.v[0];
		carry += total.v[0];
	}
	if (tm.rank() == 0) R.head[DPR_H_POOL] = carry;
}
// stage 3: the offsets, by sorted position and by call
template<typename Team> MPA_DPP_HD void dpr_offsets(const Team &tm, const DpResDev &R, int64_t b)
{
	const int64_t g = b * Team::W + tm.rank();
	DpVec<1> s, total;
	s.v[0] = dpr_words_at(R, g);
	const int64_t words = s.v[0];
	tm.exscan(s, total);
	if (g >= R.n_glob) return;
	const int32_t id = R.gids[g];
	const int64_t at = R.bsum[b] + s.v[0];
	R.off[g] = at, R.call_off[id] = at;
	if (words < 0 || words > R.tasks[id].cig_cap) R.head[DPR_H_BAD] = 1;       // (any member, the same value)
}
// stage 4: one member per call, its record
template<typename Team> MPA_DPP_HD void dpr_records(const Team &tm, const DpResDev &R, int64_t b)
{
	const int64_t k = b * Team::W + tm.rank();
	if (k >= R.n) return;
	const DTask &t = R.tasks[k];
	const bool is_ext = (t.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) != 0;
	R.rst[k] = dp_result_of(t.flag, t.nl, t.al, k, R.eo, R.sc, R.nc, is_ext ? 0 : R.call_off[k]);
}

// the four stages with a team of one (the model, and the hook without a context)
MPA_DPP_HD void dp_results_model(const DpResDev &R)
{
	const TeamOne tm;
	R.head[DPR_H_POOL] = R.head[DPR_H_BAD] = 0;
	for (int64_t b = 0; b < R.n_glob; ++b) dpr_sums(tm, R, b);
	dpr_mid(tm, R);
	for (int64_t b = 0; b < R.n_glob; ++b) dpr_offsets(tm, R, b);
	for (int64_t b = 0; b < R.n; ++b) dpr_records(tm, R, b);
}

} // namespace mpa
