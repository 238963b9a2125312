// dp_plan.h -- the plan of one mpa_dp_run() call: everything the executor (dp_exec.hip) uploads, sizes and launches that follows
// from the calls' shapes alone -- (nl, al, flag, io, vid, nt_off, aa_off, qid), contig and query lengths, the scoring options and
// a few knobs.  Host only: no HIP, no context, no globals; an error comes back as (code, message) in the plan.  What the planner knows
// about one call and one unit is dp_plan_core.h, which the device planner (MPA_GPU_DPPLAN, dp_plan_kernels.hip) compiles too.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mpamd.h"
#include "dp_device.h"
#include "dp_plan_core.h"       // the per-call and per-unit rules, the packing helpers, DpPlanKnobs; the stages of the device planner

namespace mpa {

struct WaveRange { int first = 0, cnt = 0; };                       // descriptors [first, first + cnt) of ExtWave[] / of a chunk's GlobWave[]

// one traceback chunk: the calls glob_ids[first, last) of the plain sweep, bounded by the traceback budget
struct DpTbChunk {
	size_t first = 0, last = 0;
	int64_t tb_words = 0;
	// filled by dp_plan_chunk_waves():
	std::vector<int32_t> list;                  // the calls in wave order: what k_backtrack walks
	std::vector<GlobWave> waves;
	size_t n_list = 0, n_waves = 0;             // ... their lengths (a plan made on the device has only these: the lists are in the pools)
	WaveRange cls[8];                           // by DpClass T_16 .. T_MB
};

struct DpPlan {
	int rc = MPA_OK;
	std::string err;
	// A plan made on the device (dev_dp_plan, dp_exec.hip): tasks, prep, ewaves, the chunk's list and waves, the units and the walk list are
	// in the executor's pools already and the vectors below stay empty, except glob_ids.  The counts hold for both kinds of plan.
	bool on_device = false;
	struct Counts { size_t n = 0, n_ext = 0, n_glob = 0, n_prep = 0, n_ewaves = 0, n_huge = 0; } cnt;
	bool wide_ge = false;                       // ge or fs above 255: the int32 sweeps take every call
	std::vector<DTask> tasks;                   // indexed like the caller's array
	std::vector<int32_t> ext_ids, glob_ids;     // sorted by (class, rows descending, index); glob_ids: plain sweep [0, n_reg_glob), then checkpointed
	size_t n_reg_glob = 0, n_lite = 0;
	int64_t ext_calls[16] = { 0 };              // extension calls per DpClass
	std::vector<PrepChunk> prep;
	std::vector<ExtWave> ewaves;
	WaveRange ext[kNumExtPacked], ext128, lite[4], lite_w4;   // ... its parts: X_16 .. X_SPLIT4, X_128, T_LITE16 .. T_LITE128, T_LITE_W4
	WaveRange ext_wide[kNumExtWide];            // ... and X_SPLIT8, X_SPLIT12 (split_wide), whose descriptors lie between X_SPLIT4's and X_128's
	WaveRange lite_w8;                          // ... and T_LITE_W8 (lite_w8), behind T_LITE_W4's
	std::vector<int32_t> huge_ids;              // X_HUGE calls, with one GlobWave each
	std::vector<GlobWave> huge_waves;
	PenTable pen;
	std::vector<DpTbChunk> chunks;
	// the round: every extension unit, the packed sweeps of the checkpointed calls and (round_has_glob) the first chunk's plain sweeps
	bool round_has_glob = false;
	size_t n_units = 0, n_group = 0;            // (dp_plan_units) costliest first; with the pool: whole-workgroup units [0, n_group), then the one-wave units
	int32_t walk_cnt[5] = { 0, 0, 0, 0, 0 };    // walk launches: calls per class T_LITE16 .. T_LITE_W4, consecutive in glob_ids behind n_reg_glob
	int32_t walk_cnt_w8 = 0;                    // ... and of T_LITE_W8, the sixth list behind them (k_walk_w8)
	// totals (units as in DTask) and what follows from them
	int32_t max_nl = 0, max_nl_ext = 0;
	int64_t rec_total = 0, rec_pad = 0, prof_total = 0, cig_total = 0, bnd_total = 0, hkey_total = 0, lite_total = 0, ck_total = 0, tb_max = 0;
	int64_t key_stride = 0, n_wide_groups = 0;  // row keys of the wide extension classes: [group][2 halves][key_stride]
	int64_t n_split = 0, n_bound = 0;           // split groups, their boundaries; granules then counters in the xg pool
	size_t xg_bytes = 0, xg_tail = 0;
	int64_t q_bytes = 0;
	// bytes every device pool is asked for
	struct Pools { size_t tasks, chunks, qseq, rec, prof, waves, extout, tb, cig, ncig, lite, ckpt, wlist, score, rowkey, bnd, hkey, list, xg, units; } sz = {};
	// sections of the pinned staging block (host -> device) and of the download block
	struct Up { size_t tasks, chunks, q, waves, list, gw, units, off, ids, args, wl, end; } up = {};
	struct Down { size_t eo, sc, nc, err, wb, end; } dn = {};
	mpa_dp_stats_t stats = {};                  // (dp_plan_stats) counts, cells, algorithmic bytes (without the CIGARs' own), rows_prep; the *_round cells hold if a round is launched
};

// The plan comes in the stages the executor needs it in.  dp_plan(): everything the first upload and the pool sizes depend on -- the
// n calls of `in` classified, sorted and laid out, waves, chunk boundaries, sizes and staging sections.  Contig c is
// *(int64_t*)((char*)ctg_len + c * ctg_stride) long; q->q_off and q->n_seq are read (not q->seqs); round_args_bytes: the size of the
// worker pool's argument block, which has a section of the staging block.  Returns plan.rc.
int dp_plan(const mpa_dp_task_t *in, int64_t n, const int64_t *ctg_len, size_t ctg_stride, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn,
            size_t round_args_bytes, DpPlan &plan);
// ... then, while the device works on the uploads: the call list and waves of traceback chunk ri,
void dp_plan_chunk_waves(DpPlan &plan, size_t ri);
// the round's unit list into out (room: plan.up.off - plan.up.units bytes; needs chunk 0's waves when plan.round_has_glob), returns plan.rc,
int dp_plan_units(DpPlan &plan, const DpPlanKnobs &kn, DpUnit *out);
// and the statistics (behind dp_plan_units: the *_round cells depend on whether the round has units).
void dp_plan_stats(DpPlan &plan);
// A plan from what the device planner left (DpDevHead): every count, total and range, the penalty table, pool sizes and staging
// sections with size_buffers()'s arithmetic, the statistics.  glob_ids: the sorted traceback calls (n_glob of the head).  Returns
// plan.rc; MPA_ERR_UNSUPPORTED (plan.err says why) when the plan is one the device planner declines: X_HUGE calls, a refused call, more
// than one traceback chunk.
int dp_plan_from_head(const DpDevHead &head, const int32_t *glob_ids, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn, size_t round_args_bytes, DpPlan &plan);
// why the device planner does not take a round before looking at its calls (nullptr: it does)
const char *dp_plan_device_declines(const mpa_dpopt_t *opt, const DpPlanKnobs &kn, int64_t n);
// The model of the device planner: its stages (dp_plan_core.h) with a team of one on host memory, into a plan whose vectors hold what
// the device would have left in the pools; units: the round's unit list.  Returns as dp_plan_from_head.
int dp_plan_model(const mpa_dp_task_t *in, int64_t n, const int64_t *ctg_len, int32_t n_ctg, const mpa_qbatch_t *q, const mpa_dpopt_t *opt, const DpPlanKnobs &kn,
                  size_t round_args_bytes, DpPlan &plan, std::vector<DpUnit> &units);
// pool bounds of the device planner, which sizes before it knows the plan: prep chunks of the n calls of `in` at most
int64_t dp_plan_prep_bound(const mpa_dp_task_t *in, int64_t n, int64_t *max_nl, int64_t *max_al);
// (MPA_DP_TOP) one line naming the round's costliest units by kind
std::string dp_plan_top(const DpPlan &plan, const DpPlanKnobs &kn);
// the whole plan as mpa_dbg_dp_plan() hands it out (mpamd.h): runs the later stages, returns the bytes it takes (written when they fit cap)
// or plan.rc
// (wide: as mpa_dbg_dp_plan_wide() does, mpamd_dbg.h: five more words behind everything else; w8: as mpa_dbg_dp_plan_w8() does: three
// more behind those -- first and count of T_LITE_W8's descriptors, the calls of its walk list)
int64_t dp_plan_serialize(DpPlan &plan, const DpPlanKnobs &kn, void *buf, int64_t cap, bool wide = false, bool w8 = false);
// ... the serialisation alone, of a plan whose later stages have run (dp_plan_serialize, or the device planner's vectors filled in)
int64_t dp_plan_write(const DpPlan &plan, const std::vector<DpUnit> &units, void *buf, int64_t cap, bool wide = false, bool w8 = false);

// ---- dp_exec.hip, for the test hook mpa_dbg_dp_plan_device (dpplan_dbg.cpp)
size_t dp_round_args_bytes();            // the size of the worker pool's argument block: the model's round_args_bytes
// ... and for mpa_dbg_dp_last_classes: extension calls per DpClass in the plan of the context's last mpa_dp_run
void dp_last_ext_calls(const mpa_ctx_t *ctx, int64_t ext_calls[16]);
// ... and for mpa_dbg_dp_last_huge: the last mpa_dp_run's X_HUGE calls on the one-wave kernel, on the workgroup kernel, the latter's blocks and passes
void dp_last_huge(const mpa_ctx_t *ctx, int64_t out[4]);
// ... and for mpa_dbg_dp_last_mb: the last mpa_dp_run's T_MB traceback calls swept on one wave, on workgroups, the latter's blocks and passes
void dp_last_mb(const mpa_ctx_t *ctx, int64_t out[4]);
// ... and for mpa_dbg_dp_last_w8: the last mpa_dp_run's T_LITE_W8 calls, their padded cells, the groups k_lite_w8 swept, the blocks k_walk_w8 recomputed
void dp_last_w8(const mpa_ctx_t *ctx, int64_t out[4]);
// the device planner on a context, what it left serialised like dp_plan_serialize; 1: it declined (the last error says why)
int64_t dev_dp_plan_dbg(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *in,
                        const DpPlanKnobs &kn, void *buf, int64_t cap, bool wide = false);

} // namespace mpa
