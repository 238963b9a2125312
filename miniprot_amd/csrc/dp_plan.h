// dp_plan.h -- the plan of one mpa_dp_run() call: everything the executor (dp_exec.hip) uploads, sizes and launches that follows
// from the calls' shapes alone -- (nl, al, flag, io, vid, nt_off, aa_off, qid), contig and query lengths, the scoring options and
// a few knobs.  Host only: no HIP, no context, no globals; an error comes back as (code, message) in the plan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mpamd.h"
#include "dp_device.h"

namespace mpa {

// ---- what a class means for packing (DpClass, dp_device.h)
static const int kNumExtPacked = 7;                                   // X_16 .. X_SPLIT4: the classes of the packed int16 sweeps, in ascending width
inline int ext_lanes(int cls) { return cls == X_16 ? 16 : cls == X_32 ? 32 : 64; }                       // lanes per call
inline int ext_waves(int cls) { return cls <= X_64 || cls == X_128 ? 1 : 1 << (cls - X_64); }            // waves per group: 1, 1, 1, 2, 4, 8, 16
inline int ext_columns(int cls) { return cls == X_128 ? 128 : ext_lanes(cls) * ext_waves(cls); }         // columns the class covers (= profile row width)
inline int ext_calls_per_wave(int cls) { return cls == X_128 ? 1 : 2 * (64 / ext_lanes(cls)); }          // ... per wave or group: two calls per lane
inline int ext_class_of(int32_t ncol) { for (int c = X_16; c <= X_SPLIT4; ++c) if (ncol <= ext_columns(c)) return c; return X_HUGE; }
inline int tb_class_of(int32_t ncol) { int c = T_16; while (c < T_MB && ncol > (16 << c)) ++c; return c; }   // 16, 32, ... 1024 columns, then block-major
inline int tb_calls_per_wave(int cls) { return cls == T_16 ? 4 : cls == T_32 ? 2 : 1; }                  // the plain traceback sweep: one call per group of lanes
inline int lite_columns(int cls) { return 16 << (cls - T_LITE16); }                                      // 16, 32, 64, 128, 256
inline int lite_calls_per_wave(int cls) { return cls == T_LITE128 ? 1 : cls == T_LITE_W4 ? 2 : 2 * (64 / lite_columns(cls)); }
// dwords of extension bits / checkpoints of one packed-sweep descriptor whose longest call has max_nl rows (layout: dp_device.h)
inline int64_t lite_bits_dwords(int cls, int32_t max_nl) { return cls == T_LITE_W4 ? lite_wide_bits_dwords(max_nl) : ((int64_t)max_nl / 3 + 2) * 64; }
inline int64_t lite_ckpt_dwords(int cls, int32_t max_nl) { return cls == T_LITE_W4 ? lite_wide_ckpt_dwords(max_nl) : (int64_t)(max_nl > 3 ? (max_nl - 3) / MPA_TB_BLOCK : 0) * 9 * 64; }

// values the executor has when it plans (the environment is read by the executor: at context creation, or once per process)
struct DpPlanKnobs {
	int32_t lite_min = 384, lite_wide = 0;      // checkpointed traceback: from this many rows; 129..256 columns included
	int32_t no_split = 0;                       // repeated round: no inter-workgroup hand-off
	int32_t antidiag = 0;                       // (measurement) the 32-column extension class runs on k_ext_antidiag
	int32_t pool = 0;                           // the worker pool takes the round's units (MPA_DP_POOL)
	int32_t ext_dual = 1, unit_prio = 1;        // MPA_DP_EXT_DUAL, MPA_DP_PRIO
	int64_t tb_budget = (int64_t)8 << 30;       // bytes of traceback matrix per chunk
};

struct WaveRange { int first = 0, cnt = 0; };                       // descriptors [first, first + cnt) of ExtWave[] / of a chunk's GlobWave[]

// one traceback chunk: the calls glob_ids[first, last) of the plain sweep, bounded by the traceback budget
struct DpTbChunk {
	size_t first = 0, last = 0;
	int64_t tb_words = 0;
	// filled by dp_plan_chunk_waves():
	std::vector<int32_t> list;                  // the calls in wave order: what k_backtrack walks
	std::vector<GlobWave> waves;
	WaveRange cls[8];                           // by DpClass T_16 .. T_MB
};

struct DpPlan {
	int rc = MPA_OK;
	std::string err;
	bool wide_ge = false;                       // ge or fs above 255: the int32 sweeps take every call
	std::vector<DTask> tasks;                   // indexed like the caller's array
	std::vector<int32_t> ext_ids, glob_ids;     // sorted by (class, rows descending, index); glob_ids: plain sweep [0, n_reg_glob), then checkpointed
	size_t n_reg_glob = 0, n_lite = 0;
	std::vector<PrepChunk> prep;
	std::vector<ExtWave> ewaves;
	WaveRange ext[kNumExtPacked], ext128, lite[4], lite_w4;   // ... its parts: X_16 .. X_SPLIT4, X_128, T_LITE16 .. T_LITE128, T_LITE_W4
	std::vector<int32_t> huge_ids;              // X_HUGE calls, with one GlobWave each
	std::vector<GlobWave> huge_waves;
	PenTable pen;
	std::vector<DpTbChunk> chunks;
	// the round: every extension unit, the packed sweeps of the checkpointed calls and (round_has_glob) the first chunk's plain sweeps
	bool round_has_glob = false;
	size_t n_units = 0, n_group = 0;            // (dp_plan_units) costliest first; with the pool: whole-workgroup units [0, n_group), then the one-wave units
	int32_t walk_cnt[5] = { 0, 0, 0, 0, 0 };    // walk launches: calls per class T_LITE16 .. T_LITE_W4, consecutive in glob_ids behind n_reg_glob
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
// (MPA_DP_TOP) one line naming the round's costliest units by kind
std::string dp_plan_top(const DpPlan &plan, const DpPlanKnobs &kn);
// the whole plan as mpa_dbg_dp_plan() hands it out (mpamd.h): runs the later stages, returns the bytes it takes (written when they fit cap)
// or plan.rc
int64_t dp_plan_serialize(DpPlan &plan, const DpPlanKnobs &kn, void *buf, int64_t cap);

} // namespace mpa
