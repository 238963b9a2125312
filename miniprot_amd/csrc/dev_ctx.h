// dev_ctx.h -- the HOST side that the device units of the library share (dev_ctx.hip, seed_run.hip, refine_run.hip, index_run.hip,
// dp_exec.hip, stats_run.hip): the device context with its memory pools, what dev_ctx.hip offers the stage drivers, and the chain tail of
// seed_run.hip that the refinement uses too.  Each unit compiles its own kernels; a kernel is launched only by the unit that
// defines it, everything across units goes through the host functions declared here and in mpa_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <time.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <thread>
#include <atomic>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpa_internal.h"
#include "host_core.h"
#include "dp_device.h"
#include "dp_plan.h"
#include "stream_plan.h"
#include "chain_core.h"
#include "dev_layout.h"
#include "dev_common.h"

namespace mpa {

struct DpPool;                            // the DP worker pool's block of device memory (dp_kernels.hip): the context only holds the pointer

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return MPA_ERR_HIP; } } while (0)

// bytes of HBM this process holds through the pools below and the resident index, and how often a pool had to grow
// (mpa_device_bytes / mpa_pool_growths: bench.py's hbm_resident_gb and pool_growth_events).  Process-wide, defined ONCE in dev_ctx.hip
extern std::atomic<long long> g_dev_bytes, g_pool_growths;
extern thread_local bool tl_alloc_failed;                 // the last pool request of this thread could not be met (device seeding then declines instead of failing)

// A block of device memory and its owner: freed when the owner goes, counted in g_dev_bytes while it is held.  take() and release()
// are the only places that count.  Movable, so that a block built in a local can be handed over; not copyable.
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	// high-water mark of this pool over all contexts that play the same part in the stream pipeline (DP lane, seeder, planner):
	// the batches of a job are alike, so what one lane needed for its pool the others will need too -- a context that has to
	// (re)allocate sizes the pool for the largest request any of them has seen, and the first batches of a stream do the growing
	// once for everybody instead of once per context (a growth is a hipFree: it waits for the whole device)
	std::atomic<size_t> *hint = nullptr;
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); cap = o.cap, p = o.p; o.p = nullptr, o.cap = 0; } return *this; }   // (p last: a table is tested by its pointer)
	~DevBuf() { release(); }
	int ensure(size_t bytes);                // (dev_ctx.hip) at least `bytes`, with slack and the siblings' hint
	int ensure_exact(size_t bytes);          // exactly `bytes` (the caller has added its own slack)
	hipError_t take(size_t bytes);           // (dev_ctx.hip) what it holds goes, then a block of exactly `bytes`: no slack, no hint, no growth counted, tl_alloc_failed untouched
	void release() { if (p) { (void)hipFree(p); g_dev_bytes -= (long long)cap; } p = nullptr, cap = 0; }
	template<typename T> T *as() { return (T*)p; }
};

// a pool of a device context: it can only be declared with the registry of its owner and its name, so a context has no pool that
// its report, its hints and mpa_dbg_ctx_pools do not know.  The registry lists the pools in declaration order, which is the same
// in every context of a process: the position is the pool's identity across contexts (the siblings' hints).
struct CtxPool;
struct PoolRegistry { std::vector<CtxPool*> all; };
struct CtxPool : DevBuf {
	const char *const name;
	CtxPool(PoolRegistry &reg, const char *name_) : name(name_) { reg.all.push_back(this); }
	CtxPool(CtxPool &&) = delete;             // (the registry holds its address)
};

// a table of the resident index: exactly as large as it was asked for, read as a pointer to its elements
template<typename T> struct DevTable : DevBuf {
	operator T*() const { return (T*)p; }
};

struct DeviceIndex {
	int device = -1;
	DevTable<uint8_t> seq;
	DevTable<int64_t> ctg_off, ctg_len;
	DevTable<uint8_t> spsc;                   // splice-score track (--spsc), uploaded with the genome when the index has one
	// uploaded on first use (dev_index_table):
	DevTable<uint32_t> kb;                    // k-mer occurrence lists (block ids): the first GPU seeding call
	DevTable<int64_t> ki;                     // bucket offsets of the k-mer table: the first device sketch (dev_sketch_jobs)
	DevTable<uint32_t> bo;                    // block offset of every (contig, strand): the first device regions call (k_regions)
};

struct HostPinned {
	void *p = nullptr;
	size_t cap = 0;
	HostPinned() = default;
	HostPinned(const HostPinned &) = delete;
	HostPinned &operator=(const HostPinned &) = delete;
	~HostPinned() { release(); }
	int ensure(size_t bytes) {
		if (bytes <= cap) return MPA_OK;
		release();
		const size_t want = bytes * 3 / 2 + 4096;   // (re-pinning host memory is slow: grow in big steps)
		if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; set_error("hipHostMalloc failed"); return MPA_ERR_HIP; }
		cap = want;
		return MPA_OK;
	}
	void release() { if (p) (void)hipHostFree(p); p = nullptr, cap = 0; }
	template<typename T> T *as() { return (T*)p; }
};

// What a seeding call leaves for the planning stage: pinned host memory only.  In the stream pipeline the device pools belong to
// the SEEDER (two of them), the results to the batch (one holder per batch between the start of its seeding and the end of its
// planning), so that a batch waiting to be planned does not pin down a full set of device pools.
struct SeedHold { HostPinned h_pos, h_f, h_pred, h_a, h_U, h_A, h_R, h_P; };   // h_R (MPA_GPU_REGIONS=1): region records | refinement limits | regions per query
                                                                                // h_P (MPA_GPU_PLANS=1): regions | plans | round-1 tasks | gap segments | counts per query

// The groups of a context's memory, one per stage.  Each starts with the registry of its context, which the context hands it
// (`SeedBufs seed{ pools }`); a pool is `CtxPool name{ reg, "name" }`, a pinned block a plain HostPinned member.
struct SeedBufs {
	PoolRegistry &reg;
	CtxPool jobs{ reg, "jobs" }, f{ reg, "f" }, pred{ reg, "pred" }, mark{ reg, "mark" }, flag{ reg, "flag" }, idx{ reg, "idx" }, tmp{ reg, "tmp" }, cfirst{ reg, "cfirst" };
	HostPinned h_jobs;
	SeedHold own;                                                          // results of a call without a holder of its own (blocking path, refinement)
	CtxPool r_win{ reg, "r_win" }, r_chunk{ reg, "r_chunk" }, r_words{ reg, "r_words" }, r_hits{ reg, "r_hits" }, r_count{ reg, "r_count" };   // refinement scan
	CtxPool r_gmap{ reg, "r_gmap" };                                     // ... the k-mer tables of long queries (k_refine_gmap_build), grow-only
	HostPinned h_rhits;
	CtxPool pf_qfirst2{ reg, "pf_qfirst2" }, val64[2]{ { reg, "val64_0" }, { reg, "val64_1" } };   // first kept anchor of every query; the kept anchors' values
	// k_seed_sift: segments + per-query tables, list cursors, per-segment results, dense keys
	CtxPool s_meta{ reg, "s_meta" }, s_cur{ reg, "s_cur" }, s_cur2{ reg, "s_cur2" }, s_kept{ reg, "s_kept" }, s_base{ reg, "s_base" }, s_out{ reg, "s_out" }, s_flag{ reg, "s_flag" }, dkey{ reg, "dkey" };
	HostPinned h_meta, h_back;                                             // ... their staging (up) and qfirst2 / flags / cfirst (down)
	// device sketch (sketch_exec.hip): residue table + q_off + protein text; count and bucket per position; per-query counts, prefixes, cut-offs, flags
	CtxPool k_in{ reg, "k_in" }, k_cnt{ reg, "k_cnt" }, k_bkt{ reg, "k_bkt" }, k_q{ reg, "k_q" };
	HostPinned h_kin, h_kout;                                              // ... its staging (up) and qfirst / jfirst / cut-offs / flags (down)
	CtxPool rg{ reg, "rg" };                                             // device regions (k_regions): records, limits and per-query scratch, carved up per call
	CtxPool pl{ reg, "pl" };                                             // device plans (k_plans): records and per-query scratch, carved up per call
	CtxPool x_all{ reg, "x_all" };                                       // device chaining: views, extraction scratch, survivors, main-chain state, chains (carved up per call)
	CtxPool rx_all{ reg, "rx_all" }, rx_keys{ reg, "rx_keys" };        // device refinement: pairing tables, pair keys (two buffers), chain state (carved up per call)
	HostPinned h_xoff;                                                     // ... offsets of the chains of every query (down)
	// chain forward pass (k_chain_fwd, k_chain_fwd_wave: list of long runs + its counter)
	CtxPool c_a{ reg, "c_a" }, c_f{ reg, "c_f" }, c_pred{ reg, "c_pred" }, c_mark{ reg, "c_mark" }, c_flag{ reg, "c_flag" }, c_first{ reg, "c_first" }, c_long{ reg, "c_long" };
	HostPinned hc_a, hc_f, hc_pred;
};

// a DP round (dp_exec.hip, gs32_exec.hip)
struct RoundBufs {
	PoolRegistry &reg;
	CtxPool tasks{ reg, "tasks" }, waves{ reg, "waves" }, chunks{ reg, "chunks" }, qseq{ reg, "qseq" }, rec{ reg, "rec" }, prof{ reg, "prof" }, tb{ reg, "tb" }, cig{ reg, "cig" }, ncig{ reg, "ncig" }, score{ reg, "score" };
	CtxPool extout{ reg, "extout" }, bnd{ reg, "bnd" }, list{ reg, "list" }, rowkey{ reg, "rowkey" }, cigd{ reg, "cigd" }, cigoff{ reg, "cigoff" }, hkey{ reg, "hkey" }, xg{ reg, "xg" }, units{ reg, "units" };
	CtxPool lite{ reg, "lite" }, ckpt{ reg, "ckpt" }, wlist{ reg, "wlist" };   // checkpointed traceback (dp_device.h): extension-bit words, checkpoints, the calls the walk takes
	HostPinned h_up, h_down, h_pool;          // staging of a DP round's descriptors (host -> device) and of its results: no pageable copies, one wait
};

// the DP worker pool (dp_kernels.hip, k_dp_worker).  The pool itself belongs to the ROOT context of a device ...
struct WorkerBufs {
	PoolRegistry &reg;
	DpPool *dp_pool = nullptr;                // (root) slots + arguments of every lane, one block of device memory
	std::mutex pool_mu;                       // (root) guards pool creation, slot numbers and the interval list
	int pool_slots = 0;                       // (root) slots handed out
	hipEvent_t pool_base = nullptr;           // (root) time zero of the worker launches' intervals
	std::vector<std::pair<float, float>> pool_iv;   // (root) [start, end) of every finished worker launch of the device, ms since pool_base
	// ... a slot, a generation counter, a word of pinned host memory and a worker stream belong to every context that runs DP rounds
	int dp_slot = -1;
	unsigned int dp_gen = 0;
	int32_t *dp_done = nullptr;               // pinned: receives the generation of a round when its last unit has finished
	hipStream_t worker_stream = nullptr;      // the lane's worker launches (never waited for by a round: its workers may be busy with other lanes' units)
	hipEvent_t arm_ev = nullptr;
	struct WorkerLaunch { hipEvent_t e0, e1; };
	std::vector<WorkerLaunch> wl_busy, wl_free;   // event pairs of worker launches not yet harvested / free for reuse
	CtxPool dp_trace{ reg, "dp_trace" };      // (MPA_DP_TRACE) per-unit start/end ticks of the current round
};

// the walks over finished alignments (stats_run.hip): grow-only, allocated by the first call that asks for them
struct WalkBufs {
	PoolRegistry &reg;
	// alignment statistics (MPA_GPU_STATS=1)
	CtxPool st_in{ reg, "st_in" }, st_out{ reg, "st_out" };   // tables | jobs | CIGAR words | protein text; per-alignment records | features
	HostPinned h_stats_up, h_stats_down;      // ... their staging: one block up, one block down
	// cs strings (MPA_GPU_CS=1): what goes up shares st_in / h_stats_up
	CtxPool cs_out{ reg, "cs_out" };          // lengths | slots
	HostPinned h_cs_down;
	// residue rows (MPA_GPU_ROWS=1): the same again
	CtxPool rows_out{ reg, "rows_out" };      // records | slots
	HostPinned h_rows_down;
};

// accepted spans and region CIGARs (stats_run.hip, MPA_GPU_SPANS=1): grow-only, allocated by the first call that asks for them
struct SpanBufs {
	PoolRegistry &reg;
	CtxPool sp_in{ reg, "sp_in" }, sp_mid{ reg, "sp_mid" }, sp_out{ reg, "sp_out" };   // tables | plans | gap segments | round-1 results | text; k_spans' scratch; count | records | round-2 tasks
	CtxPool sp_pool1{ reg, "sp_pool1" };      // the batch's round-1 CIGAR pool, kept across round 2 (which overwrites cigd)
	CtxPool sp_in2{ reg, "sp_in2" }, sp_asm{ reg, "sp_asm" }, sp_cig{ reg, "sp_cig" };   // round-2 results | slot offsets (| a caller's round-2 pool); per-plan records; the assembled CIGARs
	HostPinned h_sp_up, h_sp_down, h_sp_up2, h_sp_down2;
	struct SpansKeep { Piece<SpansPlan> plan; Piece<SegRec> seg; Piece<mpa_dp_rst_t> rst1; Piece<SpanRec> rec; int64_t n_plan = -1, n_pool1 = 0; } sp_keep;   // what dev_spans_round1 left for dev_spans_assemble
};

// the device planner of a DP round (dp_exec.hip, MPA_GPU_DPPLAN=1): grow-only, allocated by the first call that asks for them
struct PlannerBufs {
	PoolRegistry &reg;
	CtxPool dpp{ reg, "dpp" };                // raw tasks | query offsets | keys | block sums | units | the header and the sorted traceback calls | sort scratch
	HostPinned h_dpp_up, h_dpp_down;          // ... its staging: one block up, one block down
};

// ranking and flat result of a batch (stats_run.hip, MPA_GPU_FINISH=1; FinishLayout): grow-only, allocated by the first call that asks for them
struct FinishBufs {
	PoolRegistry &reg;
	CtxPool fin_in{ reg, "fin_in" }, fin_mid{ reg, "fin_mid" };   // what goes up; ranks, counts, their prefix and the large queries' scratch
	HostPinned h_fin_up, h_fin_down;          // the block that goes up; the flat result, which k_finish_scan and k_finish_gather write directly
	int64_t last[6] = { 0, 0, 0, 0, 0, 0 };   // of the last call: queries, hits in, hits kept, bytes down, queries ranked in HBM scratch, host waits (mpa_dbg_finish_last)
};

// the output text of a batch (stats_run.hip, MPA_GPU_FORMAT; FormatLayout): grow-only, allocated by the first call that asks for them
struct FormatBufs {
	PoolRegistry &reg;
	CtxPool fmt_in{ reg, "fmt_in" }, fmt_mid{ reg, "fmt_mid" };   // what goes up; a place per hit, the queries' sums and their prefix
	HostPinned h_fmt_up, h_fmt_down;          // the block that goes up; totals, id places and text, which k_format_scan and k_format_write write directly
	int64_t last[6] = { 0, 0, 0, 0, 0, 0 };   // of the last call: queries, hits printed, text bytes, id fields, host waits, declined while sizing (mpa_dbg_format_last)
};

// What the environment says about every context of a pipeline: filled once for a root (ctx_knobs_from_env), handed to a sibling by
// one assignment, read by dp_plan_knobs().  A new knob is a field here and a line there.
struct CtxKnobs {
	size_t tb_budget = (size_t)8 << 30;       // bytes of traceback matrix per k_glob launch (MPA_TB_BUDGET_MB)
	int lite_min = 384;                       // rows from which a traceback call of <= 256 columns is checkpointed (MPA_DP_LITE_MIN; 0: never)
	int lite_wide = 0;                        // ... 129..256 columns included (MPA_DP_LITE_WIDE; 0, the default until it has been measured: those keep the plain sweep)
	int split_wide = 0;                       // 1025..3072-column extension calls on X_SPLIT8 / X_SPLIT12 instead of k_ext_huge (MPA_DP_SPLIT_WIDE; 0, the default until it has been measured)
	int huge_wg = 0;                          // X_HUGE calls of hwg::MIN_BLOCKS column blocks or more on k_ext_huge_wg, one wave per block (MPA_DP_HUGE_WG; 0, the default until it has been measured)
	int lite_w8 = 0;                          // ... 257..512 columns included, on eight-wave groups (MPA_DP_LITE_W8; 0 until measured; independent of lite_wide; off with the worker pool)
	int mb_wg = 0;                            // traceback calls of class T_MB on k_glob_mb_wg, one wave per block, instead of one wave per call (MPA_DP_MB_WG; 0; off with the worker pool)
};

} // namespace mpa

using namespace mpa;

struct mpa_ctx_s {
	int device = 0;
	hipStream_t stream = nullptr;
	static const int kSide = 16;              // side streams: every kernel class of a batch runs concurrently
	hipStream_t side[kSide] = {};
	hipEvent_t ev[6] = {};
	hipEvent_t fork_ev = nullptr;
	hipEvent_t lev[2 * kSide] = {};           // start/stop pair per side-stream launch
	hipEvent_t wait_ev = nullptr;             // blocking-sync event: a host thread that waits for the device SLEEPS (wait_stream)
	int side_off = 0;                         // first side stream a round uses (lets the DP lanes of a stream of batches sit on different hardware queues)
	hipStream_t seed_stream = nullptr;        // high-priority stream of the seeding kernels: short, and must not queue behind DP tails
	CtxKnobs knobs;
	// ---- the contexts of a device: a root and the siblings it owns
	mpa_ctx_s *root = nullptr;                // the context this one is a sibling of (nullptr: a root)
	std::vector<mpa_ctx_s*> siblings;         // extra contexts on the same device for concurrent sub-batches (owned)
	// ---- what the stream plan (stream_plan.h) says about this context; the defaults are a context outside a stream of batches
	bool one_stream = false;                  // a seeder or planner of a planned layout: its seeding stream IS its main stream
	int side_cap = kSide;                     // side streams a DP round may create (0: its side launches take the main stream) ...
	int side_cls = 0;                         // ... and their priority class (StreamClass)
	std::unique_ptr<mpa::StreamPlan> splan;   // (root context only) the plan its siblings were created by (mpa_dbg_stream_plan)
	// ---- device memory: every pool registers here when it is declared, in the order of the groups below
	PoolRegistry pools;
	std::unique_ptr<std::atomic<size_t>[]> hints;   // (root context only) high-water marks: [role][pool], 3 x pools.all.size() (ctx_set_role)
	SeedBufs seed{ pools };                   // the seeding, chaining and refinement stages (seed_run.hip, refine_run.hip)
	std::vector<std::unique_ptr<SeedHold>> holds;   // result holders of the stream pipeline's batches (ctx_seed_hold)
	RoundBufs round{ pools };
	WorkerBufs worker{ pools };
	WalkBufs walks{ pools };
	SpanBufs spans{ pools };
	PlannerBufs planner{ pools };
	FinishBufs finish{ pools };
	FormatBufs format{ pools };
	// ---- what the DP rounds of this context did
	mpa_dp_stats_t stats = {};
	mpa_dp_stats_t total = {};
	int64_t last_huge[4] = { 0, 0, 0, 0 };    // the last mpa_dp_run's X_HUGE calls on the one-wave kernel, on the workgroup kernel, the latter's column blocks and passes (mpa_dbg_dp_last_huge)
	int64_t last_w8[4] = { 0, 0, 0, 0 };      // the last mpa_dp_run's T_LITE_W8 calls, their padded cells, the groups k_lite_w8 swept, the blocks k_walk_w8 recomputed (mpa_dbg_dp_last_w8)
	int64_t last_mb[4] = { 0, 0, 0, 0 };      // the last mpa_dp_run's T_MB traceback calls swept on one wave, on workgroups (k_glob_mb_wg), the latter's column blocks and passes (mpa_dbg_dp_last_mb)
	int64_t last_ext_calls[16] = { 0 };       // extension calls per DpClass in the last mpa_dp_run (mpa_dbg_dp_last_classes)
	bool no_split = false;                    // this mpa_dp_run() repeats a round whose workgroup hand-off timed out: 512/1024-column calls go to k_ext_huge
	int64_t handoff_retries = 0;              // how often that has happened on this context (mpa_dp_handoff_retries)
	std::atomic<int64_t> n_waits{0};          // host waits on this context's streams so far (wait_stream): a resident DP round reports its own
	bool antidiag = false;                    // (measurement) the 32-column extension class runs on the anti-diagonal prototype, k_ext_antidiag (mpa_dbg_antidiag)
	// ---- the device index build (index_run.hip)
	mpa_idx_build_stats_t idx_stats = {};     // what the last device index build on this context did (mpa_idx_build_last_stats)
	std::vector<int64_t> idx_hist;            // ... and the histogram it planned its passes from (empty: one pass)
	int64_t idx_budget_dbg = 0;               // (tests) exact key budget of the device index build in bytes, 0 = the default (mpa_dbg_idx_build_budget)
};

namespace mpa {

// ---- rocPRIM through a scratch pool: ask for the scratch size, grow the pool, call.  `exact`: the pool grows to the size asked for
// and no further (the index build in passes budgets its memory to the byte); otherwise with the pools' slack.
// (Not for scratch that is no pool of its own: the device planner's two sorts work in a piece of `dpp` carved before either runs,
// dp_exec.hip, and ask rocPRIM themselves; nor for calls that share one sizing -- the refinement's two scans, the pass build's first sort.)
template<typename In, typename Out, typename T> static int dev_exclusive_scan(DevBuf &scratch, bool exact, In in, Out out, T init, size_t n, hipStream_t s)
{
	size_t bytes = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, rocprim::plus<T>(), s));
	if (int rc = exact ? scratch.ensure_exact(bytes + 256) : scratch.ensure(bytes + 256)) return rc;
	HIP_TRY(rocprim::exclusive_scan(scratch.p, bytes, in, out, init, n, rocprim::plus<T>(), s));
	return MPA_OK;
}
// keys_in[n] sorted by bits [bit0, bit1) into keys_out[n]
template<typename K> static int dev_sort_keys(DevBuf &scratch, bool exact, K *keys_in, K *keys_out, size_t n, unsigned bit0, unsigned bit1, hipStream_t s)
{
	size_t bytes = 0;
	HIP_TRY(rocprim::radix_sort_keys(nullptr, bytes, keys_in, keys_out, n, bit0, bit1, s));
	if (int rc = exact ? scratch.ensure_exact(bytes + 256) : scratch.ensure(bytes + 256)) return rc;
	HIP_TRY(rocprim::radix_sort_keys(scratch.p, bytes, keys_in, keys_out, n, bit0, bit1, s));
	return MPA_OK;
}

// ---- dev_ctx.hip, for the stage drivers
hipError_t wait_stream(mpa_ctx_t *ctx, hipStream_t s);                                   // wait for a stream, asleep
hipError_t upload_large(void *dst, const void *src, size_t bytes, hipStream_t s);       // a large host array into device memory through pinned slices
hipError_t dev_index_table(mpa_ctx_t *ctx, DevBuf &t, const void *src, size_t bytes, const char *note);   // a table of the resident index, uploaded on first use
void ensure_seed_stream(mpa_ctx_t *ctx);                                                 // ctx->seed_stream, created on first use
hipError_t create_stream_in_class(hipStream_t *s, int cls);                              // a non-blocking stream of a StreamClass (stream_plan.h)
hipError_t ensure_dynamic_lds(const void *fn, int device, size_t bytes);                 // hipFuncSetAttribute(MaxDynamicSharedMemorySize), once per (kernel, device)
void ctx_pool_report(mpa_ctx_t *root);
void pool_harvest(mpa_ctx_t *ctx, bool wait);                                            // (dp_exec.hip) the finished worker launches of a context's DP pool
// (stats_run.hip: dev_aln_walks_stage / dev_aln_walks and the dev_spans_* calls are declared in mpa_internal.h, where the host pipeline that
// calls them sees them)

// ---- the chain tail (seed_run.hip): what the three device chaining routes -- behind the pre-chain (dev_chains_on_device), without one
// (dev_seed_direct) and the refinement (dev_refine_chains) -- do alike, and the forward pass dev_chain_forward shares with them
PreParams pre_params(const ChainParams &cp);              // mp_chain's parameters as the forward-pass kernels take them
// One allocation (x_all) per call, cut into typed pieces by a Carve (carve.h) of 256-byte alignment.  What one extraction works
// in and leaves is an ExtractCarve (dev_layout.h: carve_extract_scratch for mark .. status, carve_extract_counts for the counts and
// their prefixes; out_a / out_u are pieces the route places, the deliberate aliases of the pre-chain's dead view included), the
// forward pass's arrays a ChainFwdCarve (carve_chain_fwd, carve_chain_runs); a kernel gets piece.in(X).
// k_seed_fill -> k_chain_fwd -> k_chain_fwd_wave on stream s over the n anchors `a` of n_prob problems (first / cnt as k_chain_fwd
// takes them).  Runs longer than serial_run get a wavefront each, through the list `runs` (long_cap entries) and its counter n_runs,
// which the caller has zeroed on s; flag is only initialised.
int chain_fwd_launch(hipStream_t s, const uint64_t *a, int64_t n, const int64_t *first, const int64_t *cnt, int32_t n_prob, const PreParams &pp, int32_t serial_run,
                     const ChainFwdBufs &b);
// the views of all problems on the device (ExtractArgs, seed_exec.hip): sparse (v_pos, ntot_first) or dense (both null)
struct ChainViewDev { const int64_t *first, *cnt, *ntot_first; const int32_t *v_pos, *v_f, *v_pred; const uint64_t *v_a; };
// k_chain_extract for n_prob problems on stream s, X = x_all.  prof_label != nullptr: with MPA_TIMING=2 the launch is profiled per phase
// and reported under that label.
int chain_extract_launch(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, const ChainParams &p, int32_t n_prob, int32_t set_only,
                         const char *prof_label);
// chain_extract_launch (chains, not the set) -> k_offsets2 -> offsets and status down (one wait) -> the chains of all problems, densely,
// into the pinned memory of H (k_chain_pack).  status_error != nullptr: a problem that needs the host ends the call with that error
// (MPA_ERR_UNSUPPORTED) before anything is packed; otherwise *h_status (pinned, valid until the context's next chain tail) tells the caller.
// regions != nullptr (MPA_GPU_REGIONS=1, the main round of a seeding route): k_regions + k_region_pack take k_chain_pack's place -- the
// regions of every problem (records, refinement limits, their number: RegionsTail) come down instead of its chains, out.A / out.U stay
// null, a_first / u_first still count what was left on the device.  A pool or pinned block that cannot grow: `done` stays false and
// the chains are packed as without it.
// plans != nullptr (MPA_GPU_PLANS=1, the refinement): k_plans + k_plan_pack take k_chain_pack's place -- the problems are the
// refinement windows of n_query queries (window w of query q: h_win0[q] <= w < h_win0[q + 1]), and what comes down are every query's
// regions, plans, round-1 tasks and gap segments (PlansTail).  The caller has uploaded what the d_ pointers name.  Declined as the
// regions are: `done` stays false and the chains are packed.
struct ChainTailOut { std::vector<int64_t> &a_first, &u_first; const uint64_t *&A, *&U; };
struct PlansTail {
	PlansParams p;
	int32_t n_query;
	const PlansWindow *d_win;            // [n_prob]
	const int64_t *d_win0, *d_qoff;      // [n_query + 1] first window; first residue in d_text
	const uint8_t *d_text, *d_tabs;      // the protein text; codon table | aa20 | matrix (ALN_TAB_BYTES)
	const uint8_t *d_seq;                // the resident genome and its contig table
	const int64_t *d_ctg_off, *d_ctg_len;
	bool done;
	const RegionRec *R; const PlanRec *P; const mpa_dp_task_t *T; const SegRec *S; const PlansCounts *N;   // pinned (H.h_P): see RefineChains
};
struct RegionsTail { RegionsParams p; const uint32_t *d_bo; bool done; const RegionRec *R; const uint64_t *E; const int32_t *n_reg; };
int chain_extract_pack(mpa_ctx_t *ctx, hipStream_t s, char *X, const ExtractCarve &c, const ChainViewDev &v, const ChainParams &p, int32_t n_prob, SeedHold &H,
                       const char *prof_label, const char *status_error, ChainTailOut out, const int32_t **h_status, RegionsTail *regions = nullptr, PlansTail *plans = nullptr);

} // namespace mpa
