// dp_exec.hip -- host-side executor of the batched spliced DP: the implementation of mpa_dp_run().
//
// A batch of ns_global_gs16b() calls (nasw.h:135; call sites align.c:73,288,293,322,327) is planned on the host (dp_plan.cpp: classes,
// order, pool layout, waves, traceback chunks, the round's unit list -- nothing of it needs the device) and then enqueued as
//   1. one upload from a pinned staging block, k_prep_rows / k_prep_prof (per-row records + query profiles, written once to HBM),
//   2. ONE k_dp_round launch for every DP unit of the round: the extension calls of every class up to 1024 columns, the packed
//      sweeps of the checkpointed traceback and the plain traceback sweeps of the first traceback chunk, costliest unit first
//      (MPA_DP_POOL=1: the units go to the resident workers of the device's pool, k_dp_worker, instead),
//   3. next to it on side streams: k_ext_huge + k_ext_replay (wider calls, and whatever the int16 sweeps may not take), k_lite_wide
//      (129..256-column checkpointed calls), the 512/1024-thread traceback classes, the anti-diagonal prototype,
//   4. k_backtrack per traceback chunk (chunks after the first: stand-alone k_glob_* launches, serial), k_walk for the
//      checkpointed calls, one download, one host wait, k_cigar_gather,
// bracketed by HIP events (mpa_dp_last_stats feeds bench.py's roofline record).  mpa_dp_run_impl is that list of phases.  The
// seeding-stage drivers (dev_prechain_forward, dev_refine_scan; kernels in seed_exec.hip) live here too.  There is no CPU
// fallback here by design.
#include <hip/hip_runtime.h>
#include <time.h>
#include <algorithm>
#include <functional>
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
#include "chain_core.h"
#include "dp_kernels.hip"
#include "dp_antidiag.hip"
#include "seed_exec.hip"
#include "sketch_exec.hip"

namespace mpa {

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return MPA_ERR_HIP; } } while (0)

// bytes of HBM this process holds through the pools below and the resident index, and how often a pool had to grow
// (mpa_device_bytes / mpa_pool_growths: bench.py's hbm_resident_gb and pool_growth_events)
static std::atomic<long long> g_dev_bytes{0}, g_pool_growths{0};
static thread_local bool tl_alloc_failed = false;         // the last pool request of this thread could not be met (device seeding then declines instead of failing)

struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	// high-water mark of this pool over all contexts that play the same part in the stream pipeline (DP lane, seeder, planner):
	// the batches of a job are alike, so what one lane needed for its pool the others will need too -- a context that has to
	// (re)allocate sizes the pool for the largest request any of them has seen, and the first batches of a stream do the growing
	// once for everybody instead of once per context (a growth is a hipFree: it waits for the whole device)
	std::atomic<size_t> *hint = nullptr;
	int ensure(size_t bytes) {
		const size_t asked = bytes;
		if (hint) {
			size_t h = hint->load(std::memory_order_relaxed);
			while (bytes > h && !hint->compare_exchange_weak(h, bytes, std::memory_order_relaxed)) {}
			if (bytes <= cap) return MPA_OK;
			// (the siblings' high-water mark is a guess about batches to come, not a need: it is taken only while it stays within
			// twice the request -- one outlier batch on one lane must not make every lane's pool that large for the rest of the job)
			if (h > bytes && h <= 2 * bytes) bytes = h;
		}
		if (bytes <= cap) return MPA_OK;
		const double t0 = now_ms();
		// (free, then allocate: measured -- round 3, call 18 -- a pool that keeps its old block until the stream is over and only
		// hipMalloc()s pays 25 ms per growth instead of 6: the allocator hands the block just freed straight back, a fresh one is
		// mapped)
		if (p) { (void)hipFree(p); g_dev_bytes -= (long long)cap; ++g_pool_growths; }
		p = nullptr, cap = 0;
		// (round 5 tried an arena -- a few 8-GB chunks carved up on the host instead of ~180 hipMallocs in a cold run's first second:
		// no gain, the cost of a cold start is the VOLUME of device memory the driver maps, ~100 GB in ~2.5 s, however it is asked for:
		// profiles/r05_cli_cold_start.txt)
		// (generous: growing a pool is a hipFree, which waits for the whole device and stalls every pipeline stage; the batches of a
		// job are alike, so a third of slack makes the first allocation of a pool its last in nearly all cases -- but slack and hint
		// are wishes: when the device cannot give that much, the bare request is tried before the call fails)
		size_t want = bytes;
		want += std::max<size_t>(want / 8, std::min<size_t>(want / 3, (size_t)256 << 20)) + 4096;   // a third of slack up to 256 MB, an eighth beyond (round 4: every pool carried a third: 100 GB per rank)
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b - (free_b >> 4)) want = asked + 4096;
		hipError_t e = hipMalloc(&p, want);
		if (e != hipSuccess && want > asked + 4096) { (void)hipGetLastError(); want = asked + 4096; e = hipMalloc(&p, want); }
		if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr, tl_alloc_failed = true; set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); return MPA_ERR_HIP; }
		cap = want;
		g_dev_bytes += (long long)cap;
		timing_note("    pool growth (device)", now_ms() - t0);
		return MPA_OK;
	}
	// exactly `bytes` (the caller has added its own slack)
	int ensure_exact(size_t bytes) {
		if (bytes <= cap) return MPA_OK;
		if (p) { (void)hipFree(p); g_dev_bytes -= (long long)cap; ++g_pool_growths; }
		p = nullptr, cap = 0;
		if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr, tl_alloc_failed = true; set_error("hipMalloc(" + std::to_string(bytes) + ") failed"); return MPA_ERR_HIP; }
		cap = bytes;
		g_dev_bytes += (long long)cap;
		return MPA_OK;
	}
	void release() { if (p) { (void)hipFree(p); g_dev_bytes -= (long long)cap; } p = nullptr, cap = 0; }
	template<typename T> T *as() { return (T*)p; }
};

struct DeviceIndex {
	int device = -1;
	uint8_t *seq = nullptr;
	int64_t *ctg_off = nullptr, *ctg_len = nullptr;
	uint32_t *kb = nullptr;                   // k-mer occurrence lists (block ids), uploaded on first GPU seeding call
	size_t kb_bytes = 0;
	int64_t *ki = nullptr;                    // bucket offsets of the k-mer table, uploaded on the first device sketch (dev_sketch_jobs)
	size_t ki_bytes = 0;
	uint8_t *spsc = nullptr;                  // splice-score track (--spsc), uploaded with the genome when the index has one
	size_t seq_bytes = 0, spsc_bytes = 0;     // bytes counted into g_dev_bytes for the genome and the track
};

struct HostPinned {
	void *p = nullptr;
	size_t cap = 0;
	int ensure(size_t bytes) {
		if (bytes <= cap) return MPA_OK;
		if (p) (void)hipHostFree(p);
		p = nullptr, cap = 0;
		const size_t want = bytes * 3 / 2 + 4096;   // (re-pinning host memory is slow: grow in big steps)
		if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc failed"); return MPA_ERR_HIP; }
		cap = want;
		return MPA_OK;
	}
	void release() { if (p) (void)hipHostFree(p); p = nullptr, cap = 0; }
	template<typename T> T *as() { return (T*)p; }
};

// What a seeding call leaves for the planning stage: pinned host memory only.  In the stream pipeline the device pools belong to
// the SEEDER (two of them), the results to the batch (one holder per batch between the start of its seeding and the end of its
// planning), so that a batch waiting to be planned does not pin down a full set of device pools.
struct SeedHold { HostPinned h_pos, h_f, h_pred, h_a, h_U, h_A; };

struct SeedBufs {
	DevBuf jobs, f, pred, mark, flag, idx, tmp, cfirst;
	HostPinned h_jobs;
	SeedHold own;                                                          // results of a call without a holder of its own (blocking path, refinement)
	DevBuf r_win, r_chunk, r_words, r_hits, r_count;      // refinement scan
	DevBuf r_gmap;                                        // ... the k-mer tables of long queries (k_refine_gmap_build), grow-only
	HostPinned h_rhits;
	DevBuf pf_qfirst2, val64[2];                                            // first kept anchor of every query; the kept anchors' values
	DevBuf s_meta, s_cur, s_cur2, s_kept, s_base, s_out, s_flag, dkey;      // k_seed_sift: segments + per-query tables, list cursors, per-segment results, dense keys
	HostPinned h_meta, h_back;                                             // ... their staging (up) and qfirst2 / flags / cfirst (down)
	DevBuf k_in, k_cnt, k_bkt, k_q;                                         // device sketch (sketch_exec.hip): residue table + q_off + protein text; count and bucket per position; per-query counts, prefixes, cut-offs, flags
	HostPinned h_kin, h_kout;                                              // ... its staging (up) and qfirst / jfirst / cut-offs / flags (down)
	DevBuf x_all;                                                          // device chaining: views, extraction scratch, survivors, main-chain state, chains (carved up per call)
	DevBuf rx_all, rx_keys;                                                // device refinement: pairing tables, pair keys (two buffers), chain state (carved up per call)
	HostPinned h_xoff;                                                     // ... offsets of the chains of every query (down)
	DevBuf c_a, c_f, c_pred, c_mark, c_flag, c_first, c_long;        // chain forward pass (k_chain_fwd, k_chain_fwd_wave: list of long runs + its counter)
	HostPinned hc_a, hc_f, hc_pred;
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
	DevBuf tasks, waves, chunks, qseq, rec, prof, tb, cig, ncig, score, extout, bnd, list, rowkey, cigd, cigoff, hkey, xg, units;
	DevBuf lite, ckpt, wlist;                 // checkpointed traceback (dp_device.h): extension-bit words, checkpoints, the calls the walk takes
	HostPinned h_up, h_down, h_pool;          // staging of a DP round's descriptors (host -> device) and of its results: no pageable copies, one wait
	mpa_dp_stats_t stats = {};
	mpa_dp_stats_t total = {};
	size_t tb_budget = (size_t)8 << 30;       // bytes of traceback matrix per k_glob launch
	int lite_min = 384;                       // rows from which a traceback call of <= 256 columns is checkpointed (MPA_DP_LITE_MIN; 0: never)
	int lite_wide = 0;                        // ... 129..256 columns included (MPA_DP_LITE_WIDE; 0, the default until it has been measured: those keep the plain sweep)
	std::vector<mpa_ctx_s*> siblings;         // extra contexts on the same device for concurrent sub-batches (owned)
	SeedBufs seed;                            // buffers of the GPU seeding stage (seed_exec.hip)
	hipEvent_t wait_ev = nullptr;             // blocking-sync event: a host thread that waits for the device SLEEPS (wait_stream)
	int side_off = 0;                         // first side stream a round uses (lets the DP lanes of a stream of batches sit on different hardware queues)
	hipStream_t seed_stream = nullptr;        // high-priority stream of the seeding kernels: short, and must not queue behind DP tails
	bool no_split = false;                    // this mpa_dp_run() repeats a round whose workgroup hand-off timed out: 512/1024-column calls go to k_ext_huge
	int64_t handoff_retries = 0;              // how often that has happened on this context (mpa_dp_handoff_retries)
	std::vector<SeedHold*> holds;             // result holders of the stream pipeline's batches (owned; ctx_seed_hold)
	struct PoolHints { std::atomic<size_t> dev[3][96]; };
	PoolHints *hints = nullptr;               // (root context only, owned) high-water marks per pipeline role and pool
	mpa_idx_build_stats_t idx_stats = {};     // what the last device index build on this context did (mpa_idx_build_last_stats)
	std::vector<int64_t> idx_hist;            // ... and the histogram it planned its passes from (empty: one pass)
	int64_t idx_budget_dbg = 0;               // (tests) exact key budget of the device index build in bytes, 0 = the default (mpa_dbg_idx_build_budget)
	bool antidiag = false;                    // (measurement) the 32-column extension class runs on the anti-diagonal prototype, k_ext_antidiag (mpa_dbg_antidiag)
	// ---- DP worker pool (dp_kernels.hip, k_dp_worker).  The pool itself belongs to the ROOT context of a device ...
	mpa_ctx_s *root = nullptr;                // the context this one is a sibling of (nullptr: a root)
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
	DevBuf dp_trace;                          // (MPA_DP_TRACE) per-unit start/end ticks of the current round
};

namespace mpa {

// every device pool of a context, in a fixed order (the index is the pool's identity across contexts)
template<typename F> static void ctx_each_devbuf(mpa_ctx_s *ctx, F f)
{
	SeedBufs &B = ctx->seed;
	DevBuf *all[] = { &ctx->tasks, &ctx->waves, &ctx->chunks, &ctx->qseq, &ctx->rec, &ctx->prof, &ctx->tb, &ctx->cig, &ctx->ncig,
	                  &ctx->score, &ctx->extout, &ctx->bnd, &ctx->list, &ctx->rowkey, &ctx->cigd, &ctx->cigoff, &ctx->hkey, &ctx->xg, &ctx->units,
	                  &B.jobs, &B.f, &B.pred, &B.mark, &B.flag, &B.idx, &B.tmp, &B.cfirst,
	                  &B.r_win, &B.r_chunk, &B.r_words, &B.r_hits, &B.r_count,
	                  &B.c_a, &B.c_f, &B.c_pred, &B.c_mark, &B.c_flag, &B.c_first, &B.c_long,
	                  &B.pf_qfirst2, &B.val64[0], &B.val64[1],
	                  &B.s_meta, &B.s_cur, &B.s_cur2, &B.s_kept, &B.s_base, &B.s_out, &B.s_flag, &B.dkey, &B.x_all, &B.rx_all, &B.rx_keys,
	                  &ctx->lite, &ctx->ckpt, &ctx->wlist, &B.k_in, &B.k_cnt, &B.k_bkt, &B.k_q, &B.r_gmap };
	int k = 0;
	for (DevBuf *b : all) f(*b, k++);
}

// Wait for everything enqueued on a stream -- asleep.  hipStreamSynchronize() spins on the completion signal by default; a
// pipeline keeps eight or nine host threads waiting for the device at any time (DP lanes, seeders, planners), and on a host
// that gives the process a CPU quota (16 cores per GPU on the boxes this was measured on) spinning waiters eat the very cores
// the host stages need.  An event created with hipEventBlockingSync makes the runtime block on the signal instead.
// Measured (round 3): even the "blocking" hipEventSynchronize costs a waiting thread about half a core, so the wait polls the
// event and SLEEPS 100 us between polls after a short burst of immediate ones.
static hipError_t wait_stream(mpa_ctx_t *ctx, hipStream_t s)
{
	if (!ctx->wait_ev) return hipStreamSynchronize(s);
	hipError_t e = hipEventRecord(ctx->wait_ev, s);
	if (e != hipSuccess) return e;
	for (int polls = 0;; ++polls) {
		e = hipEventQuery(ctx->wait_ev);
		if (e != hipErrorNotReady) return e;
		if (polls >= 8) {
			static const long nap_ns = [] { const char *e = getenv("MPA_POLL_US"); const long v = e ? atol(e) : 100; return (v < 1 ? 1 : v > 5000 ? 5000 : v) * 1000L; }();
			struct timespec ts = { 0, nap_ns };
			nanosleep(&ts, nullptr);
		}
	}
}

// A large host array into device memory.  The index arrays are views into the mapped .mpi (page cache) or pageable vectors: a
// plain hipMemcpy stages them through the runtime's own bounce buffer on ONE thread (measured, round 4: the 7.6 GB of a 3 Gbp
// index cost most of the 4.3 s a cold command-line run spends before it maps anything).  Here four host threads copy 32-MB slices
// into two pinned buffers in turn while the DMA engine drains the other one.
static hipError_t upload_large(void *dst, const void *src, size_t bytes, hipStream_t s)
{
	const size_t kSlice = (size_t)32 << 20;
	if (bytes < 4 * kSlice) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
	void *pin[2] = { nullptr, nullptr };
	hipEvent_t done[2] = { nullptr, nullptr };
	hipError_t e = hipSuccess;
	for (int k = 0; k < 2 && e == hipSuccess; ++k) { e = hipHostMalloc(&pin[k], kSlice, hipHostMallocDefault); if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming); }
	if (e == hipSuccess) {
		const int kThreads = 4;
		size_t at = 0;
		for (int k = 0; at < bytes && e == hipSuccess; ++k, at += kSlice) {
			const int b = k & 1;
			const size_t n = std::min(kSlice, bytes - at);
			if (k >= 2) e = hipEventSynchronize(done[b]);              // the copy that last used this buffer has left it
			if (e != hipSuccess) break;
			std::thread th[kThreads];
			const size_t part = (n + kThreads - 1) / kThreads;
			for (int t = 0; t < kThreads; ++t)
				th[t] = std::thread([=] { const size_t o = (size_t)t * part; if (o < n) memcpy((char*)pin[b] + o, (const char*)src + at + o, std::min(part, n - o)); });
			for (auto &t : th) t.join();
			e = hipMemcpyAsync((char*)dst + at, pin[b], n, hipMemcpyHostToDevice, s);
			if (e == hipSuccess) e = hipEventRecord(done[b], s);
		}
		if (e == hipSuccess) e = hipStreamSynchronize(s);
	}
	for (int k = 0; k < 2; ++k) { if (done[k]) (void)hipEventDestroy(done[k]); if (pin[k]) (void)hipHostFree(pin[k]); }
	if (e != hipSuccess) { (void)hipGetLastError(); return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }   // (no pinned memory to be had: the plain copy)
	return hipSuccess;
}

// The seeding / refinement kernels of a context run on a stream of their own, created with the device's highest priority: they are
// short and a pipeline stage waits for each of them (MPA_PRIO_SEED=0: normal priority; MPA_PRIO_MAIN=1: the contexts' main streams
// -- the DP lanes' prep kernels, walks and copies -- get the high priority too).
static void ensure_seed_stream(mpa_ctx_t *ctx)
{
	if (ctx->seed_stream) return;
	static const bool high = [] { const char *e = getenv("MPA_PRIO_SEED"); return !e || atoi(e) != 0; }();
	int least = 0, greatest = 0;
	(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
	if (hipStreamCreateWithPriority(&ctx->seed_stream, hipStreamNonBlocking, high ? greatest : least) != hipSuccess) ctx->seed_stream = ctx->stream;
}

int dev_upload_index(mpa_ctx_t *ctx, mpa_idx_s *mi)
{
	if (ctx->device < 0 || ctx->device >= mpa_idx_s::kMaxDevices) { set_error("device number beyond what an index keeps copies for"); return MPA_ERR_UNSUPPORTED; }
	static std::mutex mu[mpa_idx_s::kMaxDevices];             // one per device: the pipelines of several devices upload side by side
	std::lock_guard<std::mutex> g(mu[ctx->device]);
	if (mi->dev[ctx->device]) return MPA_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	DeviceIndex *d = new DeviceIndex();
	d->device = ctx->device;
	// (an upload that fails half-way gives everything back: the caller may retry, e.g. on the host path, and must not leak HBM)
	struct Undo { DeviceIndex *d; ~Undo() { if (!d) return; (void)hipFree(d->seq); (void)hipFree(d->ctg_off); (void)hipFree(d->ctg_len); (void)hipFree(d->spsc); delete d; } } undo{ d };
	const size_t n = mi->ctg.size();
	std::vector<int64_t> off(n), len(n);
	for (size_t i = 0; i < n; ++i) off[i] = mi->ctg[i].off, len[i] = mi->ctg[i].len;
	HIP_TRY(hipMalloc((void**)&d->seq, mi->seq.size() + 16));
	HIP_TRY(hipMalloc((void**)&d->ctg_off, n * 8 + 8));
	HIP_TRY(hipMalloc((void**)&d->ctg_len, n * 8 + 8));
	{ const double t0 = now_ms(); HIP_TRY(upload_large(d->seq, mi->seq.data(), mi->seq.size(), ctx->stream)); timing_note("index upload: packed genome", now_ms() - t0); }
	HIP_TRY(hipMemcpy(d->ctg_off, off.data(), n * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d->ctg_len, len.data(), n * 8, hipMemcpyHostToDevice));
	if (!mi->spsc.empty()) {
		HIP_TRY(hipMalloc((void**)&d->spsc, mi->spsc.size() + 16));
		HIP_TRY(hipMemcpy(d->spsc, mi->spsc.data(), mi->spsc.size(), hipMemcpyHostToDevice));
	}
	d->seq_bytes = mi->seq.size() + 16, d->spsc_bytes = mi->spsc.empty() ? 0 : mi->spsc.size() + 16;   // (what was added is what dev_free_index takes off again)
	mi->dev[ctx->device] = d;
	undo.d = nullptr;
	g_dev_bytes += (long long)(d->seq_bytes + d->spsc_bytes);
	return MPA_OK;
}

void dev_free_index(mpa_idx_s *mi)
{
	for (DeviceIndex *&d : mi->dev) {
		if (!d) continue;
		(void)hipSetDevice(d->device);
		(void)hipFree(d->seq); (void)hipFree(d->ctg_off); (void)hipFree(d->ctg_len);
		g_dev_bytes -= (long long)(d->seq_bytes + d->spsc_bytes);
		if (d->kb) { (void)hipFree(d->kb); g_dev_bytes -= (long long)d->kb_bytes; }
		if (d->ki) { (void)hipFree(d->ki); g_dev_bytes -= (long long)d->ki_bytes; }
		if (d->spsc) (void)hipFree(d->spsc);
		delete d;
		d = nullptr;
	}
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember it per (kernel, device), under a lock -- several
// DP lanes and seeders get here at once, and a process may hold contexts on several devices
static hipError_t ensure_dynamic_lds(const void *fn, int device, size_t bytes)
{
	static std::mutex mu;
	static std::vector<std::pair<const void*, int>> done;
	std::lock_guard<std::mutex> g(mu);
	for (auto &d : done) if (d.first == fn && d.second == device) return hipSuccess;
	const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
	if (e == hipSuccess) done.emplace_back(fn, device);
	return e;
}

template<int NW> static hipError_t launch_glob_wide(const GlobArgs &a, int n_groups, hipStream_t s, bool wide_ge = false)
{
	const size_t lds = (size_t)NW * 22 * 64 * 2 + 2 * NW * 16 + 64 * 4;
	if (wide_ge) hipLaunchKernelGGL((k_glob_wide<NW, true>), dim3(n_groups), dim3(NW * 64), lds, s, a);
	else hipLaunchKernelGGL((k_glob_wide<NW, false>), dim3(n_groups), dim3(NW * 64), lds, s, a);
	return hipGetLastError();
}

} // namespace mpa

extern "C" {

// traceback classes T_16, T_32, T_64 (16/32/64 lanes) and T_MB (block-major, > 1024 columns) in one launch; a.waves = whole array
// (the traceback chunks after the first, which do not ride in the round's launch)
static hipError_t launch_glob_narrow(const GlobArgs &a, const int *first, const int *cnt, hipStream_t s, bool wide_ge = false)
{
	const size_t lds = (size_t)22 * 64 * 2 + (size_t)4 * 32 * 4;
	NarrowMap m{};
	const int cls[4] = { T_16, T_32, T_64, T_MB };
	int total = 0;
	for (int k = 0; k < 4; ++k) m.first[k] = first[cls[k]], m.cnt[k] = cnt[cls[k]], total += cnt[cls[k]];
	if (wide_ge) hipLaunchKernelGGL(k_glob_narrow<true>, dim3((unsigned)total), dim3(64), lds, s, a, m);
	else hipLaunchKernelGGL(k_glob_narrow<false>, dim3((unsigned)total), dim3(64), lds, s, a, m);
	return hipGetLastError();
}

} // namespace mpa

extern "C" {

int mpa_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

mpa_ctx_t *mpa_ctx_create(int device)
{
	int n = mpa_device_count();
	if (n <= 0 || device < 0 || device >= n) {
		set_error("no usable HIP device (the MI355X DP kernels have no CPU fallback)");
		return nullptr;
	}
	if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
	mpa_ctx_s *ctx = new mpa_ctx_s();
	ctx->device = device;
	static const bool main_high = [] { const char *e = getenv("MPA_PRIO_MAIN"); return e && atoi(e) != 0; }();
	int least = 0, greatest = 0;
	(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
	bool ok = (main_high ? hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) == hipSuccess;
	for (auto &e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	for (auto &e : ctx->lev) ok = ok && hipEventCreate(&e) == hipSuccess;
	ok = ok && hipEventCreate(&ctx->fork_ev) == hipSuccess;
	ok = ok && hipEventCreateWithFlags(&ctx->wait_ev, hipEventBlockingSync | hipEventDisableTiming) == hipSuccess;
	if (!ok) {                                            // a null handle would silently alias the legacy default stream
		set_error("creating the context's HIP streams/events failed");
		mpa_ctx_destroy(ctx);
		return nullptr;
	}
	if (const char *s = getenv("MPA_TB_BUDGET_MB")) ctx->tb_budget = (size_t)atoll(s) << 20;
	if (const char *s = getenv("MPA_DP_LITE_MIN")) ctx->lite_min = atoi(s);
	if (const char *s = getenv("MPA_DP_LITE_WIDE")) ctx->lite_wide = atoi(s) != 0;
	return ctx;
}

void mpa_ctx_destroy(mpa_ctx_t *ctx)
{
	if (!ctx) return;
	for (mpa_ctx_s *sb : ctx->siblings) mpa_ctx_destroy(sb);
	ctx->siblings.clear();
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	if (ctx->worker_stream) { (void)hipStreamSynchronize(ctx->worker_stream); (void)hipStreamDestroy(ctx->worker_stream); }   // (workers exit by themselves once no slot has a unit left)
	for (auto *v : { &ctx->wl_busy, &ctx->wl_free }) { for (auto &w : *v) { (void)hipEventDestroy(w.e0); (void)hipEventDestroy(w.e1); } v->clear(); }
	if (ctx->arm_ev) (void)hipEventDestroy(ctx->arm_ev);
	if (ctx->dp_done) (void)hipHostFree(ctx->dp_done);
	if (ctx->pool_base) (void)hipEventDestroy(ctx->pool_base);
	if (ctx->dp_pool) (void)hipFree(ctx->dp_pool);
	ctx->dp_trace.release();
	SeedBufs &B = ctx->seed;
	ctx_each_devbuf(ctx, [](DevBuf &b, int) { b.release(); });
	for (HostPinned *h : { &B.h_jobs, &B.h_rhits, &B.hc_a, &B.hc_f, &B.hc_pred, &B.h_meta, &B.h_back, &B.h_xoff, &B.h_kin, &B.h_kout, &ctx->h_up, &ctx->h_down, &ctx->h_pool }) h->release();
	auto drop_hold = [](SeedHold &H) { for (HostPinned *h : { &H.h_pos, &H.h_f, &H.h_pred, &H.h_a, &H.h_U, &H.h_A }) h->release(); };
	drop_hold(B.own);
	for (SeedHold *H : ctx->holds) { drop_hold(*H); delete H; }
	ctx->holds.clear();
	delete ctx->hints, ctx->hints = nullptr;
	for (auto &e : ctx->ev) if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->lev) if (e) (void)hipEventDestroy(e);
	if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
	if (ctx->wait_ev) (void)hipEventDestroy(ctx->wait_ev);
	for (auto &st : ctx->side) if (st) (void)hipStreamDestroy(st);
	if (ctx->seed_stream && ctx->seed_stream != ctx->stream) (void)hipStreamDestroy(ctx->seed_stream);
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;
}

int mpa_idx_to_device(mpa_ctx_t *ctx, mpa_idx_t *mi) { return dev_upload_index(ctx, mi); }

int mpa_idx_build_kmers_device(mpa_ctx_t *ctx, mpa_idx_t *mi)
{
	if (!ctx) { set_error("no device context"); return MPA_ERR_NO_DEVICE; }
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return dev_index_build(ctx, mi); });
}

} // extern "C"

namespace mpa {
// k-th sibling of a context: same device, own streams and buffers, created on first use
mpa_ctx_t *ctx_sibling(mpa_ctx_t *ctx, int k)
{
	if (k <= 0) return ctx;
	while ((int)ctx->siblings.size() < k) {
		mpa_ctx_t *sb = mpa_ctx_create(ctx->device);
		if (!sb) return nullptr;
		sb->tb_budget = ctx->tb_budget;
		sb->lite_min = ctx->lite_min;
		sb->lite_wide = ctx->lite_wide;
		sb->root = ctx;
		ctx->siblings.push_back(sb);
	}
	return ctx->siblings[k - 1];
}
void ctx_set_side_offset(mpa_ctx_t *ctx, int off) { ctx->side_off = off; }
// `ctx` (the root itself or one of its siblings) plays part `role` of the root's stream pipeline: 0 DP lane, 1 seeder, 2 planner
void ctx_set_role(mpa_ctx_t *root, mpa_ctx_t *ctx, int role)
{
	if (!root->hints) {
		root->hints = new mpa_ctx_s::PoolHints();
		for (auto &r : root->hints->dev) for (auto &h : r) h.store(0);
	}
	mpa_ctx_s::PoolHints *H = root->hints;
	ctx_each_devbuf(ctx, [&](DevBuf &b, int k) { b.hint = k < 96 ? &H->dev[role][k] : nullptr; });
}
SeedHold *ctx_seed_hold(mpa_ctx_t *ctx, int k)
{
	while ((int)ctx->holds.size() <= k) ctx->holds.push_back(new SeedHold());
	return ctx->holds[(size_t)k];
}

// (MPA_TIMING) the device pools of a root context and its siblings, largest first: where the HBM of a pipeline goes
void ctx_pool_report(mpa_ctx_t *root)
{
	static const char *const kName[] = { "tasks", "waves", "chunks", "qseq", "rec", "prof", "tb", "cig", "ncig", "score", "extout", "bnd", "list", "rowkey", "cigd", "cigoff", "hkey", "xg", "units",
		"s.jobs", "s.f", "s.pred", "s.mark", "s.flag", "s.idx", "s.tmp", "s.cfirst", "s.r_win", "s.r_chunk", "s.r_words", "s.r_hits", "s.r_count",
		"s.c_a", "s.c_f", "s.c_pred", "s.c_mark", "s.c_flag", "s.c_first", "s.c_long", "s.pf_qfirst2", "s.val64_0", "s.val64_1",
		"s.s_meta", "s.s_cur", "s.s_cur2", "s.s_kept", "s.s_base", "s.s_out", "s.s_flag", "s.dkey", "s.x_all", "s.rx_all", "s.rx_keys", "lite", "ckpt", "wlist" };
	std::vector<mpa_ctx_t*> all{ root };
	for (mpa_ctx_t *sb : root->siblings) all.push_back(sb);
	size_t grand = 0;
	for (size_t c = 0; c < all.size(); ++c) {
		size_t tot = 0;
		std::vector<std::pair<size_t, int>> big;
		ctx_each_devbuf(all[c], [&](DevBuf &b, int k) { tot += b.cap; if (b.cap >= ((size_t)64 << 20)) big.push_back({ b.cap, k }); });
		std::sort(big.rbegin(), big.rend());
		fprintf(stderr, "[mpa-pools] context %zu: %.2f GB;", c, tot / 1e9);
		for (auto &x : big) fprintf(stderr, " %s %.2f", x.second < (int)(sizeof(kName) / sizeof(kName[0])) ? kName[x.second] : "?", x.first / 1e9);
		fprintf(stderr, "\n");
		grand += tot;
	}
	fprintf(stderr, "[mpa-pools] all contexts of the pipeline: %.2f GB of pools (+ the resident index)\n", grand / 1e9);
}

void pool_harvest(mpa_ctx_t *ctx, bool wait);
void ctx_absorb_sibling_stats(mpa_ctx_t *ctx)
{
	if (timing_on()) ctx_pool_report(ctx->root ? ctx->root : ctx);
	pool_harvest(ctx, true);
	for (mpa_ctx_s *sb : ctx->siblings) {
		pool_harvest(sb, true);
		mpa_dp_stats_t &t = ctx->total, &u = sb->total;
		t.n_ext += u.n_ext, t.n_glob += u.n_glob, t.cells_ext += u.cells_ext, t.cells_glob += u.cells_glob, t.rows_prep += u.rows_prep;
		t.alg_bytes_ext += u.alg_bytes_ext, t.alg_bytes_glob += u.alg_bytes_glob;
		t.ms_prep += u.ms_prep, t.ms_ext += u.ms_ext, t.ms_glob += u.ms_glob, t.ms_backtrack += u.ms_backtrack, t.ms_total += u.ms_total;
		t.launches_ext += u.launches_ext, t.launches_glob += u.launches_glob;
		t.cells_ext_round += u.cells_ext_round, t.cells_glob_round += u.cells_glob_round, t.ms_round += u.ms_round, t.launches_round += u.launches_round;
		t.n_ckpt_wide += u.n_ckpt_wide, t.cells_ckpt_wide += u.cells_ckpt_wide;
		u = mpa_dp_stats_t();
		ctx->handoff_retries += sb->handoff_retries, sb->handoff_retries = 0;
	}
}
} // namespace mpa

namespace mpa {
// dev_prechain_forward() with k_seed_sift (the default).  The caller has uploaded the jobs.  Per-anchor memory: 16 bytes of
// staging; everything behind the sift is sized by the kept anchors.  The result arrays are written by k_seed_compact straight
// into pinned host memory (no copy kernels, no second pass over HBM).
static int dev_chains_on_device(mpa_ctx_t *ctx, int32_t n_query, int64_t m, int64_t n2, int nb, const uint64_t *key, const uint64_t *val, const int64_t *d_qfirst,
                                const int32_t *h_flag, const ChainParams &pre, const ChainParams &mainp, PrechainSparse &out, SeedHold &H);

// The sift of a batch up to the host's first look at it: segments, k_seed_sift, k_sift_offsets, the per-query first kept anchor
// and the hand-back flags down (one wait).  reach < 0: the pre-chain's keep rule (same or adjacent block, halved staging for large
// queries); reach >= 0: the main chain's reach, full staging (k_seed_sift<4096, true>).  n_seg == 0 / n2 == 0: nothing (kept).
struct SiftFront {
	int32_t n_seg = 0;
	int64_t n2 = 0;                                          // kept anchors of the batch
	const SiftSeg *d_segs = nullptr;
	const int64_t *d_qfirst = nullptr;
	uint64_t *stage0 = nullptr, *stage1 = nullptr;
	int64_t *h_qfirst2 = nullptr, *h_cfirst = nullptr;       // pinned: first kept anchor of every query; room for one more prefix array
	int32_t *h_flag = nullptr;                               // pinned: the sift's hand-back flags
	size_t meta_q = 0;
	double t_sift = 0;
};
static int dev_sift_front(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, int nb, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs, int64_t n_jobs,
                          PrechainSparse &out, double t_begin, const int64_t *jfirst_in, int32_t reach, SiftFront &F)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	if (n_block >= 0x7fffffffu) { set_error("GPU seeding: more than 2^31 blocks"); return MPA_ERR_UNSUPPORTED; }
	// ---- segments: a query's block space in pieces of ~seg_target anchors (evenly, the kernel adapts inside a segment)
	const int64_t seg_target = [] { const char *e = getenv("MPA_SIFT_SEG"); const int64_t v = e ? atoll(e) : 49152; return v < 256 ? (int64_t)256 : v; }();   // (read per call: the tests flip it)
	static thread_local std::vector<SiftSeg> segs;
	static thread_local std::vector<int64_t> jfirst;
	static thread_local std::vector<int32_t> qseg;
	segs.clear();
	int64_t n_cur = 0;                                         // cursors: one per (segment, list of its query)
	static thread_local std::vector<int64_t> sfirst;          // first staging slot of every query (sift_stage_slots)
	jfirst.assign((size_t)n_query + 1, 0), qseg.assign((size_t)n_query + 1, 0), sfirst.assign((size_t)n_query + 1, 0);
	for (int32_t q = 0; q < n_query; ++q) sfirst[(size_t)q + 1] = sfirst[(size_t)q] + (reach >= 0 ? qfirst[q + 1] - qfirst[q] : sift_stage_slots(qfirst[q + 1] - qfirst[q]));
	const int64_t n_stage = sfirst[(size_t)n_query];
	if (jfirst_in) jfirst.assign(jfirst_in, jfirst_in + n_query + 1);      // (the jobs were made on the device: dev_sketch_jobs counted them)
	else {
		for (int64_t j = 0; j < n_jobs; ++j) ++jfirst[(size_t)jobs[j].qid + 1];
		for (int32_t q = 0; q < n_query; ++q) jfirst[(size_t)q + 1] += jfirst[(size_t)q];
	}
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t na = qfirst[q + 1] - qfirst[q];
		qseg[(size_t)q] = (int32_t)segs.size();
		if (na == 0) continue;
		if (na >= (int64_t)1 << 31) { set_error("GPU seeding: a query with more than 2^31 anchors"); return MPA_ERR_UNSUPPORTED; }
		const int64_t nl_q = jfirst[(size_t)q + 1] - jfirst[(size_t)q];
		if (nl_q > (1 << 20)) { set_error("GPU seeding: a query with more than 2^20 seeds"); return MPA_ERR_UNSUPPORTED; }
		const int64_t ns = std::min<int64_t>((na + seg_target - 1) / seg_target, n_block);
		for (int64_t k = 0; k < ns; ++k) {
			const uint32_t lo = (uint32_t)((uint64_t)n_block * (uint64_t)k / (uint64_t)ns), hi = (uint32_t)((uint64_t)n_block * (uint64_t)(k + 1) / (uint64_t)ns);
			if (hi > lo) {
				if (n_cur > INT32_MAX - nl_q) { set_error("GPU seeding: too many (segment, seed) cursors in one batch"); return MPA_ERR_UNSUPPORTED; }
				segs.push_back(SiftSeg{ q, lo, hi, (int32_t)n_cur });
				n_cur += nl_q;
			}
		}
	}
	qseg[(size_t)n_query] = (int32_t)segs.size();
	const int32_t n_seg = (int32_t)segs.size();
	if (n_seg == 0) return MPA_OK;                             // (F.n_seg stays 0)
	// one pinned block up: qfirst | jfirst | sfirst | segments | qseg
	const size_t meta_q = ((size_t)n_query + 1) * 8, seg_bytes = (size_t)n_seg * sizeof(SiftSeg);
	const size_t off_jf = meta_q, off_sf = 2 * meta_q, off_seg = 3 * meta_q, off_qs = off_seg + seg_bytes, meta_bytes = off_qs + ((size_t)n_query + 1) * 4;
	int rc;
	// (round 6: the two staging arrays of the sift -- 8 B per staging slot each, dead once k_sift_copy has packed the kept anchors --
	// live at the front of the chaining block, which is carved up only behind that copy: 4.4 GB less per seeder at genome scale)
	const size_t stage_bytes = ((size_t)n_stage * 8 + 64 + 255) & ~(size_t)255;
	if ((rc = B.h_meta.ensure(meta_bytes))) return rc;
	char *hm = B.h_meta.as<char>();
	memcpy(hm, qfirst, meta_q), memcpy(hm + off_jf, jfirst.data(), meta_q), memcpy(hm + off_sf, sfirst.data(), meta_q), memcpy(hm + off_seg, segs.data(), seg_bytes), memcpy(hm + off_qs, qseg.data(), ((size_t)n_query + 1) * 4);
	if ((rc = B.s_meta.ensure(meta_bytes)) || (rc = B.s_cur.ensure((size_t)n_cur * 4 + 16)) || (rc = B.s_cur2.ensure((size_t)n_cur * 4 + 16)) ||
	    (rc = B.s_kept.ensure((size_t)n_seg * 4)) || (rc = B.s_base.ensure((size_t)n_seg * 8)) || (rc = B.s_out.ensure(((size_t)n_seg + 1) * 8)) ||
	    (rc = B.s_flag.ensure((size_t)n_query * 4 + 16)) || (rc = B.pf_qfirst2.ensure(meta_q)) || (rc = B.cfirst.ensure(meta_q)) ||
	    (rc = B.x_all.ensure(2 * stage_bytes)) || (rc = B.h_back.ensure(2 * meta_q + (size_t)n_query * 4 + 64))) return rc;
	uint64_t *const stage0 = B.x_all.as<uint64_t>(), *const stage1 = (uint64_t*)(B.x_all.as<char>() + stage_bytes);
	HIP_TRY(hipMemcpyAsync(B.s_meta.p, hm, meta_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.s_flag.p, 0, (size_t)n_query * 4 + 16, s));
	const char *dm = B.s_meta.as<char>();
	const int64_t *d_qfirst = (const int64_t*)dm, *d_jfirst = (const int64_t*)(dm + off_jf), *d_sfirst = (const int64_t*)(dm + off_sf);
	const SiftSeg *d_segs = (const SiftSeg*)(dm + off_seg);
	const int32_t *d_qseg = (const int32_t*)(dm + off_qs);
	// (MPA_SIFT_CAP=2048, measurement: ranges of half the size need 18 KB of LDS instead of 37 KB -- a workgroup then fits next to
	// four DP workgroups on a CU -- and touch the lists twice as often)
	static const int sift_cap = [] { const char *e = getenv("MPA_SIFT_CAP"); return e ? atoi(e) : 4096; }();
	if (reach >= 0)
		hipLaunchKernelGGL((k_seed_sift<4096, true, uint32_t>), dim3((unsigned)n_seg), dim3(SIFT_THREADS), 0, s, d_segs, B.jobs.as<SeedJobDev>(), d_jfirst, d_qfirst, d_sfirst, d->kb, n_block, nb,
		                   B.s_cur.as<int32_t>(), B.s_cur2.as<int32_t>(), stage0, stage1, B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(),
		                   B.s_flag.as<int32_t>(), (uint32_t)reach);
	else if (sift_cap == 2048)
		hipLaunchKernelGGL(k_seed_sift<2048>, dim3((unsigned)n_seg), dim3(SIFT_THREADS), 0, s, d_segs, B.jobs.as<SeedJobDev>(), d_jfirst, d_qfirst, d_sfirst, d->kb, n_block, nb,
		                   B.s_cur.as<int32_t>(), B.s_cur2.as<int32_t>(), stage0, stage1, B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(),
		                   B.s_flag.as<int32_t>());
	else
	hipLaunchKernelGGL(k_seed_sift<4096>, dim3((unsigned)n_seg), dim3(SIFT_THREADS), 0, s, d_segs, B.jobs.as<SeedJobDev>(), d_jfirst, d_qfirst, d_sfirst, d->kb, n_block, nb,
	                   B.s_cur.as<int32_t>(), B.s_cur2.as<int32_t>(), stage0, stage1, B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(),
	                   B.s_flag.as<int32_t>());
	hipLaunchKernelGGL(k_sift_offsets, dim3(1), dim3(256), 0, s, d_segs, n_seg, n_query, d_qseg, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_out.as<int64_t>(),
	                   B.pf_qfirst2.as<int64_t>());
	HIP_TRY(hipGetLastError());
	int64_t *h_qfirst2 = B.h_back.as<int64_t>(), *h_cfirst = h_qfirst2 + (n_query + 1);
	int32_t *h_flag = (int32_t*)(h_cfirst + (n_query + 1));
	HIP_TRY(hipMemcpyAsync(h_qfirst2, B.pf_qfirst2.p, meta_q, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_flag, B.s_flag.p, (size_t)n_query * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const double t_sift = now_ms();
	timing_note("    seed: segments + sift (wait)", t_sift - t_begin);
	int32_t n_declined = 0;
	for (int32_t q = 0; q < n_query; ++q) n_declined += h_flag[q] != 0;
	if (n_declined) {
		out.on_host.assign((size_t)n_query, 0);
		for (int32_t q = 0; q < n_query; ++q) out.on_host[(size_t)q] = h_flag[q] != 0;
	}
	F.n_seg = n_seg, F.n2 = h_qfirst2[n_query], F.d_segs = d_segs, F.d_qfirst = d_qfirst, F.stage0 = stage0, F.stage1 = stage1;
	F.h_qfirst2 = h_qfirst2, F.h_cfirst = h_cfirst, F.h_flag = h_flag, F.meta_q = meta_q, F.t_sift = t_sift;
	return MPA_OK;
}

static int dev_prechain_forward_sift(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, const PreParams &pp, int nb, int32_t n_query, const int64_t *qfirst,
                                     const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, double t_begin, const ChainParams *pre_cp, const ChainParams *main_cp, SeedHold &H,
                                     const int64_t *jfirst_in = nullptr)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	SiftFront F;
	int rc = dev_sift_front(ctx, d, n_block, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, jfirst_in, -1, F);
	if (rc != MPA_OK || F.n_seg == 0 || F.n2 == 0) return rc;
	const int32_t n_seg = F.n_seg;
	const int64_t n2 = F.n2;
	const SiftSeg *d_segs = F.d_segs;
	const int64_t *d_qfirst = F.d_qfirst;
	uint64_t *const stage0 = F.stage0, *const stage1 = F.stage1;
	int64_t *h_cfirst = F.h_cfirst;
	const int32_t *h_flag = F.h_flag;
	const size_t meta_q = F.meta_q;
	const double t_sift = F.t_sift;
	if ((rc = B.dkey.ensure((size_t)n2 * 8)) || (rc = B.val64[0].ensure((size_t)n2 * 8)) || (rc = B.f.ensure((size_t)n2 * 4)) || (rc = B.pred.ensure((size_t)n2 * 4)) ||
	    (rc = B.mark.ensure((size_t)n2 * 4)) || (rc = B.flag.ensure((size_t)n2 * 4)) || (rc = B.idx.ensure((size_t)n2 * 4))) return rc;
	const unsigned nblk = (unsigned)((n2 + 255) / 256);
	const uint64_t *key = B.dkey.as<uint64_t>();
	const uint64_t *val = B.val64[0].as<uint64_t>();
	hipLaunchKernelGGL(k_sift_copy, dim3((unsigned)n_seg), dim3(256), 0, s, d_segs, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(), B.s_out.as<int64_t>(),
	                   stage0, stage1, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>());
	hipLaunchKernelGGL(k_seed_fill, dim3(nblk), dim3(256), 0, s, n2, pp.kmer, B.f.as<int32_t>(), B.pred.as<int32_t>(), B.mark.as<int32_t>(), B.flag.as<uint32_t>());
	hipLaunchKernelGGL(k_prechain_fwd<uint64_t>, dim3(nblk), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), pp, B.f.as<int32_t>(), B.pred.as<int32_t>(),
	                   B.mark.as<int32_t>(), B.flag.as<uint32_t>());
	HIP_TRY(hipGetLastError());
	size_t scan_bytes = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, B.flag.as<uint32_t>(), B.idx.as<uint32_t>(), 0u, (size_t)n2, rocprim::plus<uint32_t>(), s));
	if ((rc = B.tmp.ensure(scan_bytes + 256))) return rc;
	HIP_TRY(rocprim::exclusive_scan(B.tmp.p, scan_bytes, B.flag.as<uint32_t>(), B.idx.as<uint32_t>(), 0u, (size_t)n2, rocprim::plus<uint32_t>(), s));
	hipLaunchKernelGGL(k_seed_bounds, dim3((unsigned)(n_query / 256 + 1)), dim3(256), 0, s, B.pf_qfirst2.as<int64_t>(), n_query, n2, B.idx.as<uint32_t>(), B.flag.as<uint32_t>(),
	                   B.cfirst.as<int64_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h_cfirst, B.cfirst.p, meta_q, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const double t_kernels = now_ms();
	memcpy(out.cfirst.data(), h_cfirst, meta_q);
	const int64_t m = out.cfirst[n_query];
	out.m = m;
	timing_note("    seed: copy + pre-chain + scan (wait)", t_kernels - t_sift);
	if (m == 0) return MPA_OK;
	// both chaining rounds on the device (main_cp == nullptr: the caller wants the pre-chain's linked anchors, as rounds 1-2 did)
	{
		if (main_cp && pre_cp) {
			rc = dev_chains_on_device(ctx, n_query, m, n2, nb, key, val, d_qfirst, h_flag, *pre_cp, *main_cp, out, H);
			if (rc != MPA_ERR_UNSUPPORTED) { timing_note("    seed: chains on the device", now_ms() - t_kernels); return rc; }
		}
	}
	if ((rc = H.h_pos.ensure((size_t)m * 4)) || (rc = H.h_f.ensure((size_t)m * 4)) || (rc = H.h_pred.ensure((size_t)m * 4)) || (rc = H.h_a.ensure((size_t)m * 8))) return rc;
	hipLaunchKernelGGL((k_seed_compact<uint64_t, true>), dim3(nblk), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), B.flag.as<uint32_t>(), B.idx.as<uint32_t>(),
	                   B.f.as<int32_t>(), B.pred.as<int32_t>(), H.h_pos.as<int32_t>(), H.h_f.as<int32_t>(), H.h_pred.as<int32_t>(), H.h_a.as<uint64_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(wait_stream(ctx, s));
	out.pos = H.h_pos.as<int32_t>(), out.f = H.h_f.as<int32_t>(), out.pred = H.h_pred.as<int32_t>(), out.a = H.h_a.as<uint64_t>();
	timing_note("    seed: compact into pinned memory", now_ms() - t_kernels);
	return MPA_OK;
}

// Both chaining rounds of every query on the device, behind the forward pass of the pre-chain (map.c:186-196):
//   k_seed_compact      the linked anchors of every query as a sparse view (position in the full list, f, pred, anchor), in HBM
//   k_chain_extract     pre-chain extraction (set): the survivors of every query, ascending
//   k_chain_fwd         forward pass of the main chain over them (block anchors, max_dist_x = max_intron)
//   k_chain_extract     main-chain extraction: chains (score, count) and their anchors, sorted by first target position
//   k_offsets2 + k_chain_pack   the chains of all queries, densely, into pinned host memory
// What travels back is what mp_reg_gen_from_block() consumes (a few hundred anchors per query) instead of every linked anchor
// (~11 000 per query at 3 Gbp), and the host no longer spends a core-second per mini-batch on chaining.
// key/val: the kept anchors (dense, sorted), with B.f / B.pred / B.flag / B.idx / B.cfirst from the pre-chain's forward pass.
static int dev_chains_on_device(mpa_ctx_t *ctx, int32_t n_query, int64_t m, int64_t n2, int nb, const uint64_t *key, const uint64_t *val, const int64_t *d_qfirst,
                                const int32_t *h_flag, const ChainParams &pre, const ChainParams &mainp, PrechainSparse &out, SeedHold &H)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	if (mainp.bbit != pre.bbit || mainp.kmer != pre.kmer) { set_error("device chains: pre-chain and main chain disagree on the anchors"); return MPA_ERR_UNSUPPORTED; }
	// ---- one allocation, carved up: everything is indexed like the view (m entries), `ends` and `stack` have extras per problem
	const size_t M = (size_t)m, NQ = (size_t)n_query;
	size_t at = 0;
	auto carve = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
	const size_t o_vpos = carve(M * 8), o_vf = o_vpos + M * 4, o_vpred = carve(M * 4), o_va = carve(M * 8);
	const size_t o_mark = carve(M * 4), o_order = carve(M * 4), o_ends = carve((M + 64 * NQ + 64) * sizeof(Pair64)), o_tail8 = carve(M * sizeof(Pair64)),
	             o_items = carve(M * sizeof(SparseItem)), o_moved = carve(M * sizeof(SparseItem)), o_merged = carve(M * sizeof(SparseItem)),
	             o_kept = carve(M), o_stack = carve((M / 64 + 6 * NQ + 16) * sizeof(SortRange));
	// (the chain layout's scratch -- packed anchors, sorted u, first positions -- is only live after the sort replay and the
	// extraction: k_chain_extract puts it into the problem's own `moved` and `merged` lists)
	const size_t o_pre_a = carve(M * 8), o_pre_u = carve(M * 8), o_pre_na = carve(NQ * 8 + 8), o_pre_nu = carve(NQ * 8 + 8), o_status = carve(NQ * 4 + 16);
	const size_t o_mf = carve(M * 4), o_mpred = carve(M * 4), o_mmark = carve(M * 4);
	const int32_t kSerialRun = 48;                          // longer runs of the main chain get a wavefront each (k_chain_fwd_wave)
	const size_t long_cap = M / (size_t)(kSerialRun + 1) + 16, o_long = carve(long_cap * sizeof(LongRun)), o_nlong = carve(64);
	// (the main chains go where the pre-chain's view was: it is dead once the pre-chain has been extracted)
	const size_t o_out_a = o_va, o_out_u = o_vpos, o_na = carve(NQ * 8 + 8), o_nu = carve(NQ * 8 + 8), o_offa = carve(NQ * 8 + 16), o_offu = carve(NQ * 8 + 16);
	int rc;
	if ((rc = B.x_all.ensure(at))) return rc;                // (ensure() adds a third of slack: a re-allocation is a hipFree, which waits for the whole device)
	char *X = B.x_all.as<char>();
	HIP_TRY(hipMemsetAsync(X + o_status, 0, NQ * 4 + 16, s));
	const unsigned nblk2 = (unsigned)((n2 + 255) / 256), nblkm = (unsigned)((m + 255) / 256);
	// the sparse view of the pre-chain's forward pass
	hipLaunchKernelGGL((k_seed_compact<uint64_t, true>), dim3(nblk2), dim3(256), 0, s, key, val, n2, nb, B.pf_qfirst2.as<int64_t>(), B.flag.as<uint32_t>(), B.idx.as<uint32_t>(),
	                   B.f.as<int32_t>(), B.pred.as<int32_t>(), (int32_t*)(X + o_vpos), (int32_t*)(X + o_vf), (int32_t*)(X + o_vpred), (uint64_t*)(X + o_va));
	ExtractArgs xa;
	xa.first = B.cfirst.as<int64_t>(), xa.cnt = nullptr, xa.ntot_first = d_qfirst;
	xa.v_pos = (const int32_t*)(X + o_vpos), xa.v_f = (const int32_t*)(X + o_vf), xa.v_pred = (const int32_t*)(X + o_vpred), xa.v_a = (const uint64_t*)(X + o_va);
	xa.mark = (int32_t*)(X + o_mark), xa.order = (int32_t*)(X + o_order), xa.ends = (Pair64*)(X + o_ends), xa.tail8 = (Pair64*)(X + o_tail8);
	xa.items = (SparseItem*)(X + o_items), xa.moved = (SparseItem*)(X + o_moved), xa.merged = (SparseItem*)(X + o_merged);
	xa.kept = (uint8_t*)(X + o_kept), xa.stack = (SortRange*)(X + o_stack);
	xa.a_out = (uint64_t*)(X + o_pre_a), xa.u_out = (uint64_t*)(X + o_pre_u), xa.n_a = (int64_t*)(X + o_pre_na), xa.n_u = (int64_t*)(X + o_pre_nu);
	xa.status = (int32_t*)(X + o_status), xa.p = pre, xa.set_only = 1;
	// MPA_TIMING=2 (debug): per-phase wall clock of the extraction kernel, averaged over the problems of the launch
	static const bool prof = [] { const char *e = getenv("MPA_TIMING"); return e && atoi(e) >= 2; }();
	long long *d_prof = nullptr;
	auto prof_begin = [&]() -> int {
		if (!prof) return MPA_OK;
		HIP_TRY(hipMalloc((void**)&d_prof, NQ * 128 + 64));
		HIP_TRY(hipMemsetAsync(d_prof, 0, NQ * 128, s));
		const int n_prof = (int)NQ;
		HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof_n), &n_prof, sizeof(n_prof), 0, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof), &d_prof, sizeof(d_prof), 0, hipMemcpyHostToDevice, s));
		return MPA_OK;
	};
	auto prof_end = [&](const char *what) -> int {
		if (!prof) return MPA_OK;
		std::vector<long long> h(NQ * 16);
		HIP_TRY(hipMemcpyAsync(h.data(), d_prof, NQ * 128, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		double sum[4] = { 0, 0, 0, 0 }, sub[4] = { 0, 0, 0, 0 }, mx = 0;
		int64_t cnt = 0, cnt2 = 0;
		std::vector<std::pair<double, size_t>> by_time;
		for (size_t q = 0; q < NQ; ++q) {
			const long long *t = &h[q * 16];
			if (!t[4] || !t[0]) continue;
			for (int k = 0; k < 4; ++k) sum[k] += (double)(t[k + 1] - t[k]) * 1e-5;   // 100 MHz ticks -> ms
			mx = std::max(mx, (double)(t[4] - t[0]) * 1e-5), ++cnt;
			by_time.emplace_back((double)(t[4] - t[0]) * 1e-5, q);
			if (t[5] && t[6] && t[7]) {                            // the two-level sort replay: its parts (stamps 5-7 lie between 0 and 1)
				sub[0] += (double)(t[5] - t[0]) * 1e-5, sub[1] += (double)(t[6] - t[5]) * 1e-5;
				sub[2] += (double)(t[7] - t[6]) * 1e-5, sub[3] += (double)(t[1] - t[7]) * 1e-5, ++cnt2;
			}
		}
		fprintf(stderr, "[mpa-extract-prof] %s: %lld problems; mean ms: sort replay %.2f, trees %.2f, extraction %.2f, output %.2f; slowest problem %.2f ms\n", what, (long long)cnt,
		        sum[0] / std::max<int64_t>(cnt, 1), sum[1] / std::max<int64_t>(cnt, 1), sum[2] / std::max<int64_t>(cnt, 1), sum[3] / std::max<int64_t>(cnt, 1), mx);
		if (cnt2) fprintf(stderr, "[mpa-extract-prof]   two-level replay (%lld problems): level-1 placement %.2f, level-1 walk %.2f, merge %.2f, level 2 %.2f ms\n", (long long)cnt2,
		                  sub[0] / cnt2, sub[1] / cnt2, sub[2] / cnt2, sub[3] / cnt2);
		if (!by_time.empty()) {                                   // the distribution, and what the slowest problems look like
			std::sort(by_time.begin(), by_time.end());
			const size_t n = by_time.size();
			fprintf(stderr, "[mpa-extract-prof]   problem ms: p50 %.2f p90 %.2f p99 %.2f max %.2f\n", by_time[n / 2].first, by_time[n * 9 / 10].first, by_time[n * 99 / 100].first, by_time[n - 1].first);
			for (size_t k = 0; k < std::min<size_t>(n, 6); ++k) {
				const size_t q = by_time[n - 1 - k].second;
				const long long *t = &h[q * 16];
				fprintf(stderr, "[mpa-extract-prof]   slow #%zu: %.2f ms (replay %.2f [lvl2 %.2f] trees %.2f extraction %.2f output %.2f); view %lld, non-roots %lld, high scores %lld, largest level-2 bucket %lld, merged %lld\n", k,
				        by_time[n - 1 - k].first, (double)(t[1] - t[0]) * 1e-5, t[7] ? (double)(t[1] - t[7]) * 1e-5 : 0.0, (double)(t[2] - t[1]) * 1e-5, (double)(t[3] - t[2]) * 1e-5, (double)(t[4] - t[3]) * 1e-5,
				        t[8], t[9], t[10], t[11], t[12]);
			}
			const size_t q = by_time[n / 2].second;
			const long long *t = &h[q * 16];
			fprintf(stderr, "[mpa-extract-prof]   median problem: view %lld, non-roots %lld, high scores %lld, largest level-2 bucket %lld, merged %lld\n", t[8], t[9], t[10], t[11], t[12]);
		}
		long long *none = nullptr;
		HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_extract_prof), &none, sizeof(none), 0, hipMemcpyHostToDevice, s));
		HIP_TRY(wait_stream(ctx, s));
		HIP_TRY(hipDeviceSynchronize());                   // (debug facility: an extraction launched by another context may still be stamping into the buffer)
		(void)hipFree(d_prof), d_prof = nullptr;
		return MPA_OK;
	};
	if ((rc = prof_begin())) return rc;
	hipLaunchKernelGGL(k_chain_extract, dim3((unsigned)n_query), dim3(64), EXTRACT_LDS_BYTES, s, xa, n_query);
	HIP_TRY(hipGetLastError());
	if ((rc = prof_end("pre-chain"))) return rc;
	// the main chain over the survivors: forward pass ...
	PreParams pm;
	pm.max_dist_x = std::max(mainp.max_dist_x, mainp.bw), pm.max_dist_y = mainp.max_dist_y;
	if (pm.max_dist_y < mainp.bw && !mainp.is_spliced) pm.max_dist_y = mainp.bw;
	pm.bw = mainp.bw, pm.max_skip = mainp.max_skip, pm.max_iter = mainp.max_iter, pm.kmer = mainp.kmer, pm.bbit = mainp.bbit;
	pm.is_spliced = mainp.is_spliced, pm.coef_log = mainp.coef_log, pm.max_dblock = pm.max_dist_x >> mainp.bbit;
	hipLaunchKernelGGL(k_seed_fill, dim3(nblkm), dim3(256), 0, s, m, pm.kmer, (int32_t*)(X + o_mf), (int32_t*)(X + o_mpred), (int32_t*)(X + o_mmark), (uint32_t*)(X + o_mark));
	HIP_TRY(hipMemsetAsync(X + o_nlong, 0, 64, s));
	hipLaunchKernelGGL(k_chain_fwd, dim3(nblkm), dim3(256), 0, s, (const uint64_t*)(X + o_pre_a), m, B.cfirst.as<int64_t>(), (const int64_t*)(X + o_pre_na), n_query, pm,
	                   (int32_t*)(X + o_mf), (int32_t*)(X + o_mpred), (int32_t*)(X + o_mmark), kSerialRun, (LongRun*)(X + o_long), (unsigned int*)(X + o_nlong), (unsigned int)long_cap);
	hipLaunchKernelGGL(k_chain_fwd_wave, dim3((unsigned)std::min<size_t>(long_cap, 65536)), dim3(64), 0, s, (const uint64_t*)(X + o_pre_a), (const LongRun*)(X + o_long),
	                   (const unsigned int*)(X + o_nlong), (unsigned int)long_cap, pm, (int32_t*)(X + o_mf), (int32_t*)(X + o_mpred), (int32_t*)(X + o_mmark));
	HIP_TRY(hipGetLastError());
	// ... and extraction: dense views over the survivors
	xa.cnt = (const int64_t*)(X + o_pre_na), xa.ntot_first = nullptr;
	xa.v_pos = nullptr, xa.v_f = (const int32_t*)(X + o_mf), xa.v_pred = (const int32_t*)(X + o_mpred), xa.v_a = (const uint64_t*)(X + o_pre_a);
	xa.a_out = (uint64_t*)(X + o_out_a), xa.u_out = (uint64_t*)(X + o_out_u), xa.n_a = (int64_t*)(X + o_na), xa.n_u = (int64_t*)(X + o_nu);
	xa.p = mainp, xa.set_only = 0;
	if ((rc = prof_begin())) return rc;
	hipLaunchKernelGGL(k_chain_extract, dim3((unsigned)n_query), dim3(64), EXTRACT_LDS_BYTES, s, xa, n_query);
	if ((rc = prof_end("main chain"))) return rc;
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, (const int64_t*)(X + o_na), (const int64_t*)(X + o_nu), n_query, (int64_t*)(X + o_offa), (int64_t*)(X + o_offu));
	HIP_TRY(hipGetLastError());
	// offsets + status down, then the chains themselves straight into pinned memory
	const size_t offb = (NQ + 1) * 8;
	if ((rc = B.h_xoff.ensure(2 * offb + NQ * 4 + 64))) return rc;
	int64_t *h_offa = B.h_xoff.as<int64_t>(), *h_offu = h_offa + (NQ + 1);
	int32_t *h_status = (int32_t*)(h_offu + (NQ + 1));
	HIP_TRY(hipMemcpyAsync(h_offa, X + o_offa, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_offu, X + o_offu, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_status, X + o_status, NQ * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t tot_a = h_offa[n_query], tot_u = h_offu[n_query];
	if ((rc = H.h_A.ensure((size_t)tot_a * 8 + 64)) || (rc = H.h_U.ensure((size_t)tot_u * 8 + 64))) return rc;
	if (tot_a > 0 || tot_u > 0) {
		hipLaunchKernelGGL(k_chain_pack, dim3((unsigned)n_query), dim3(256), 0, s, B.cfirst.as<int64_t>(), (const int64_t*)(X + o_na), (const int64_t*)(X + o_nu),
		                   (const int64_t*)(X + o_offa), (const int64_t*)(X + o_offu), (const uint64_t*)(X + o_out_a), (const uint64_t*)(X + o_out_u),
		                   H.h_A.as<uint64_t>(), H.h_U.as<uint64_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(wait_stream(ctx, s));
	}
	out.a_first.assign(h_offa, h_offa + n_query + 1), out.u_first.assign(h_offu, h_offu + n_query + 1);
	out.A = H.h_A.as<uint64_t>(), out.U = H.h_U.as<uint64_t>();
	out.has_chains = true;
	bool any = !out.on_host.empty();
	for (int32_t q = 0; q < n_query && !any; ++q) any = h_status[q] != 0;
	if (any) {
		if (out.on_host.empty()) out.on_host.assign(NQ, 0);
		for (int32_t q = 0; q < n_query; ++q) if (h_status[q] || (h_flag && h_flag[q])) out.on_host[(size_t)q] = 1;
	}
	return MPA_OK;
}

// Seeding without a pre-chain (map.c:186 skips it with -S and --no-pre-chain), on the seeding stream:
//   k_seed_sift<4096, true>   the anchors of every query in sorted order, those kept that have another one within the main chain's reach
//   k_sift_offsets, k_sift_copy   ... densely; k_sift_anchors: block << 32 | query position, and the rank the sift carried
//   k_chain_fwd + k_chain_fwd_wave   forward pass of the MAIN chain over the kept anchors (the kernels of dev_chains_on_device, unchanged)
//   k_chain_extract     main-chain extraction from a SPARSE view: every kept anchor at its rank in the query's full list (set_only = 0)
//   k_offsets2 + k_chain_pack   the chains of all queries, densely, into pinned host memory
// The view holds ALL kept anchors, not only those the pass linked: a kept anchor without a link is a root like an absent one, the
// extraction steps over both alike, and a second compaction would cost a scan and a pass over the view to save part of one.
// Exact because a dropped anchor has no anchor of its query within max_dist_x: it has no predecessor, is nobody's predecessor and
// lies in no window that a kept anchor's max_skip / max_iter walk visits -- what a sparse view may leave out (chain_core.h).
// pm: the main chain's parameters as the forward pass takes them (pm.max_dblock = the sift's reach).
static int dev_seed_direct_impl(mpa_ctx_t *ctx, DeviceIndex *d, uint32_t n_block, const PreParams &pm, int nb, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs,
                                int64_t n_jobs, PrechainSparse &out, double t_begin, const ChainParams &mainp, SeedHold &H, const int64_t *jfirst_in, SiftKept *kept)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	SiftFront F;
	int rc = dev_sift_front(ctx, d, n_block, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, jfirst_in, pm.max_dblock, F);
	if (rc != MPA_OK || F.n_seg == 0) return rc;
	if (kept) for (int32_t q = 0; q < n_query; ++q) kept->flag[(size_t)q] = F.h_flag[q] != 0;
	if (F.n2 == 0) return MPA_OK;
	const int64_t n2 = F.n2;
	const size_t M = (size_t)n2, NQ = (size_t)n_query;
	if ((rc = B.dkey.ensure(M * 8)) || (rc = B.val64[0].ensure(M * 8))) return rc;
	hipLaunchKernelGGL(k_sift_copy, dim3((unsigned)F.n_seg), dim3(256), 0, s, F.d_segs, B.s_flag.as<int32_t>(), B.s_kept.as<uint32_t>(), B.s_base.as<int64_t>(), B.s_out.as<int64_t>(),
	                   F.stage0, F.stage1, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>());
	HIP_TRY(hipGetLastError());
	if (kept) {                                                // (test hook: the kept anchors of every query, as the chain would take them)
		std::vector<uint64_t> hk(M), hv(M);
		HIP_TRY(hipMemcpyAsync(hk.data(), B.dkey.p, M * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(hv.data(), B.val64[0].p, M * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		kept->first.assign(F.h_qfirst2, F.h_qfirst2 + n_query + 1), kept->a.resize(M);
		for (size_t i = 0; i < M; ++i) kept->a[i] = (hk[i] & ((1ULL << nb) - 1)) << 32 | (uint32_t)hv[i];
		return MPA_OK;
	}
	// ---- one allocation, carved up, as in dev_chains_on_device: the view (= the forward pass's own arrays), the extraction's scratch, the chains
	size_t at = 0;
	auto carve = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
	const size_t o_vpos = carve(M * 4), o_vf = carve(M * 4), o_vpred = carve(M * 4), o_va = carve(M * 8), o_fmark = carve(M * 4);
	const size_t o_mark = carve(M * 4), o_order = carve(M * 4), o_ends = carve((M + 64 * NQ + 64) * sizeof(Pair64)), o_tail8 = carve(M * sizeof(Pair64)),
	             o_items = carve(M * sizeof(SparseItem)), o_moved = carve(M * sizeof(SparseItem)), o_merged = carve(M * sizeof(SparseItem)),
	             o_kept = carve(M), o_stack = carve((M / 64 + 6 * NQ + 16) * sizeof(SortRange)), o_status = carve(NQ * 4 + 16);
	const int32_t kSerialRun = 48;                          // longer runs get a wavefront each (k_chain_fwd_wave)
	const size_t long_cap = M / (size_t)(kSerialRun + 1) + 16, o_long = carve(long_cap * sizeof(LongRun)), o_nlong = carve(64);
	const size_t o_out_a = carve(M * 8), o_out_u = carve(M * 8), o_na = carve(NQ * 8 + 8), o_nu = carve(NQ * 8 + 8), o_offa = carve(NQ * 8 + 16), o_offu = carve(NQ * 8 + 16);
	// (the sift's staging sits at the front of this block: if the block has to move, k_sift_copy must have read it first)
	if (at > B.x_all.cap) HIP_TRY(wait_stream(ctx, s));
	if ((rc = B.x_all.ensure(at))) return rc;
	char *X = B.x_all.as<char>();
	const unsigned nblk = (unsigned)((n2 + 255) / 256);
	const int64_t *d_first = B.pf_qfirst2.as<int64_t>();       // first kept anchor of every query (k_sift_offsets)
	HIP_TRY(hipMemsetAsync(X + o_status, 0, NQ * 4 + 16, s));
	HIP_TRY(hipMemsetAsync(X + o_nlong, 0, 64, s));
	hipLaunchKernelGGL(k_sift_anchors, dim3(nblk), dim3(256), 0, s, B.dkey.as<uint64_t>(), B.val64[0].as<uint64_t>(), n2, nb, (uint64_t*)(X + o_va), (int32_t*)(X + o_vpos));
	hipLaunchKernelGGL(k_seed_fill, dim3(nblk), dim3(256), 0, s, n2, pm.kmer, (int32_t*)(X + o_vf), (int32_t*)(X + o_vpred), (int32_t*)(X + o_fmark), (uint32_t*)(X + o_mark));
	hipLaunchKernelGGL(k_chain_fwd, dim3(nblk), dim3(256), 0, s, (const uint64_t*)(X + o_va), n2, d_first, (const int64_t*)nullptr, n_query, pm,
	                   (int32_t*)(X + o_vf), (int32_t*)(X + o_vpred), (int32_t*)(X + o_fmark), kSerialRun, (LongRun*)(X + o_long), (unsigned int*)(X + o_nlong), (unsigned int)long_cap);
	hipLaunchKernelGGL(k_chain_fwd_wave, dim3((unsigned)std::min<size_t>(long_cap, 65536)), dim3(64), 0, s, (const uint64_t*)(X + o_va), (const LongRun*)(X + o_long),
	                   (const unsigned int*)(X + o_nlong), (unsigned int)long_cap, pm, (int32_t*)(X + o_vf), (int32_t*)(X + o_vpred), (int32_t*)(X + o_fmark));
	HIP_TRY(hipGetLastError());
	ExtractArgs xa;
	xa.first = d_first, xa.cnt = nullptr, xa.ntot_first = F.d_qfirst;
	xa.v_pos = (const int32_t*)(X + o_vpos), xa.v_f = (const int32_t*)(X + o_vf), xa.v_pred = (const int32_t*)(X + o_vpred), xa.v_a = (const uint64_t*)(X + o_va);
	xa.mark = (int32_t*)(X + o_mark), xa.order = (int32_t*)(X + o_order), xa.ends = (Pair64*)(X + o_ends), xa.tail8 = (Pair64*)(X + o_tail8);
	xa.items = (SparseItem*)(X + o_items), xa.moved = (SparseItem*)(X + o_moved), xa.merged = (SparseItem*)(X + o_merged);
	xa.kept = (uint8_t*)(X + o_kept), xa.stack = (SortRange*)(X + o_stack);
	xa.a_out = (uint64_t*)(X + o_out_a), xa.u_out = (uint64_t*)(X + o_out_u), xa.n_a = (int64_t*)(X + o_na), xa.n_u = (int64_t*)(X + o_nu);
	xa.status = (int32_t*)(X + o_status), xa.p = mainp, xa.set_only = 0;
	hipLaunchKernelGGL(k_chain_extract, dim3((unsigned)n_query), dim3(64), EXTRACT_LDS_BYTES, s, xa, n_query);
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, (const int64_t*)(X + o_na), (const int64_t*)(X + o_nu), n_query, (int64_t*)(X + o_offa), (int64_t*)(X + o_offu));
	HIP_TRY(hipGetLastError());
	// offsets + status down, then the chains themselves straight into pinned memory
	const size_t offb = (NQ + 1) * 8;
	if ((rc = B.h_xoff.ensure(2 * offb + NQ * 4 + 64))) return rc;
	int64_t *h_offa = B.h_xoff.as<int64_t>(), *h_offu = h_offa + (NQ + 1);
	int32_t *h_status = (int32_t*)(h_offu + (NQ + 1));
	HIP_TRY(hipMemcpyAsync(h_offa, X + o_offa, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_offu, X + o_offu, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_status, X + o_status, NQ * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t tot_a = h_offa[n_query], tot_u = h_offu[n_query];
	if ((rc = H.h_A.ensure((size_t)tot_a * 8 + 64)) || (rc = H.h_U.ensure((size_t)tot_u * 8 + 64))) return rc;
	if (tot_a > 0 || tot_u > 0) {
		hipLaunchKernelGGL(k_chain_pack, dim3((unsigned)n_query), dim3(256), 0, s, d_first, (const int64_t*)(X + o_na), (const int64_t*)(X + o_nu),
		                   (const int64_t*)(X + o_offa), (const int64_t*)(X + o_offu), (const uint64_t*)(X + o_out_a), (const uint64_t*)(X + o_out_u),
		                   H.h_A.as<uint64_t>(), H.h_U.as<uint64_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(wait_stream(ctx, s));
	}
	out.a_first.assign(h_offa, h_offa + n_query + 1), out.u_first.assign(h_offu, h_offu + n_query + 1);
	out.A = H.h_A.as<uint64_t>(), out.U = H.h_U.as<uint64_t>();
	out.has_chains = true;
	bool any = !out.on_host.empty();                           // (the sift's hand-backs are in there already: dev_sift_front)
	for (int32_t q = 0; q < n_query && !any; ++q) any = h_status[q] != 0;
	if (any) {
		if (out.on_host.empty()) out.on_host.assign(NQ, 0);
		for (int32_t q = 0; q < n_query; ++q) if (h_status[q] || F.h_flag[q]) out.on_host[(size_t)q] = 1;
	}
	timing_note("    seed: copy + main chain on the device", now_ms() - F.t_sift);
	return MPA_OK;
}

// GPU seeding for one mini-batch: anchors -> sort -> forward pass of the pre-chain -> the anchors that have a neighbour.
// jobs: the kept seeds of all queries (qid ascending, within a query ascending query position, dst = running anchor
// offset); qfirst[n_query + 1]: first anchor of every query.  out: per query a sparse ChainView's arrays
// (pred = index into the query's part of the view, -1 for none).
// pre_p == nullptr: the direct route (dev_seed_direct) -- no pre-chain, the sift keeps by the reach of the main chain *main
static int dev_seed_entry(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams *pre_p, int32_t n_query, const int64_t *qfirst,
                          const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, const ChainParams *main, SeedHold *hold, const int64_t *jfirst_dev, SiftKept *kept)
{
	const int64_t n = qfirst[n_query];
	out.cfirst.assign((size_t)n_query + 1, 0);
	out.pos = out.f = out.pred = nullptr, out.a = nullptr, out.m = 0, out.on_host.clear();
	out.has_chains = false, out.U = out.A = nullptr, out.u_first.clear(), out.a_first.clear();
	if (!pre_p) {                                              // (no anchors: no chains -- the planners take that from the device's result like any other)
		out.has_chains = !kept, out.u_first.assign((size_t)n_query + 1, 0), out.a_first.assign((size_t)n_query + 1, 0);
		if (kept) kept->first.assign((size_t)n_query + 1, 0), kept->a.clear(), kept->flag.assign((size_t)n_query, 0);
	}
	if (n == 0 || n_jobs == 0) return MPA_OK;
	const ChainParams &pre = pre_p ? *pre_p : *main;
	if (pre.bbit <= 0) { set_error("GPU seeding needs block anchors (bbit > 0)"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	if (!d->kb) {
		static std::mutex mu[mpa_idx_s::kMaxDevices];            // (per device, like dev_upload_index)
		std::lock_guard<std::mutex> g(mu[ctx->device]);
		if (!d->kb) {
			uint32_t *p = nullptr;
			HIP_TRY(hipMalloc((void**)&p, mi->kb.size() * 4 + 16));
			{ const double t0 = now_ms(); HIP_TRY(upload_large(p, mi->kb.data(), mi->kb.size() * 4, ctx->stream)); timing_note("index upload: occurrence lists", now_ms() - t0); }
			d->kb = p, d->kb_bytes = mi->kb.size() * 4 + 16;
			g_dev_bytes += (long long)d->kb_bytes;
		}
	}
	PreParams pp;
	pp.max_dist_x = std::max(pre.max_dist_x, pre.bw), pp.max_dist_y = pre.max_dist_y;
	if (pp.max_dist_y < pre.bw && !pre.is_spliced) pp.max_dist_y = pre.bw;
	pp.bw = pre.bw, pp.max_skip = pre.max_skip, pp.max_iter = pre.max_iter, pp.kmer = pre.kmer, pp.bbit = pre.bbit;
	pp.is_spliced = pre.is_spliced, pp.coef_log = pre.coef_log, pp.max_dblock = pp.max_dist_x >> pre.bbit;   // (direct route: the main chain's parameters, as dev_chains_on_device derives them)
	int nb = 1, qb = 1;
	while ((1ULL << nb) < (uint64_t)mi->n_block + (uint64_t)pp.max_dblock + 2) ++nb;
	while ((1LL << qb) < n_query) ++qb;
	if (nb + qb > 64) { set_error("GPU pre-chain: too many queries x blocks for a 64-bit key"); return MPA_ERR_UNSUPPORTED; }
	if (pre_p && pp.max_dblock != 1) { set_error("GPU seeding: the sift assumes a pre-chain that reaches one block"); return MPA_ERR_UNSUPPORTED; }
	{	// the working set is ~60 bytes per anchor (sift: 16 of staging, the rest sized by the kept ones); a batch that does not fit
		// stays on the host (the caller falls back).  Direct route: the staging is full -- 16 B per anchor where the halved one takes 8 --
		// and the rule keeps every second anchor or more, 36 B each, before the chaining block is carved: 56 B per anchor
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			const SeedBufs &Bc = ctx->seed;
			const size_t have = Bc.f.cap + Bc.pred.cap + Bc.mark.cap + Bc.flag.cap + Bc.idx.cap + Bc.tmp.cap + Bc.x_all.cap + Bc.dkey.cap + Bc.val64[0].cap;
			if ((size_t)n * (pre_p ? 40 : 56) > have + free_b - (free_b >> 3)) { set_error("GPU seeding: batch too large for device memory"); return MPA_ERR_UNSUPPORTED; }
		}
	}
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const double t_begin = now_ms();
	// ---- upload the seed jobs (jfirst_dev: dev_sketch_jobs of this context has left them in B.jobs)
	if (!jfirst_dev) {
		if (B.h_jobs.ensure((size_t)n_jobs * sizeof(SeedJobDev)) != MPA_OK) return MPA_ERR_HIP;
		SeedJobDev *hj = B.h_jobs.as<SeedJobDev>();
		for (int64_t i = 0; i < n_jobs; ++i) hj[i] = SeedJobDev{ jobs[i].kb_off, jobs[i].dst, jobs[i].cnt, jobs[i].qpos, jobs[i].qid, 0 };
		if (B.jobs.ensure((size_t)n_jobs * sizeof(SeedJobDev)) != MPA_OK) return MPA_ERR_HIP;
		HIP_TRY(hipMemcpyAsync(B.jobs.p, hj, (size_t)n_jobs * sizeof(SeedJobDev), hipMemcpyHostToDevice, s));
	}
	// merge the occurrence lists per query in block order, keep what has a neighbour (k_seed_sift, seed_exec.hip)
	tl_alloc_failed = false;
	const int rc = pre_p ? dev_prechain_forward_sift(ctx, d, mi->n_block, pp, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, &pre, main, hold ? *hold : B.own, jfirst_dev)
	                     : dev_seed_direct_impl(ctx, d, mi->n_block, pp, nb, n_query, qfirst, jobs, n_jobs, out, t_begin, *main, hold ? *hold : B.own, jfirst_dev, kept);
	// a pool that could not grow (the admission check above is an estimate): the batch is seeded on the host, as for any batch
	// that does not fit -- nothing has been handed to the caller yet
	if (rc == MPA_ERR_HIP && tl_alloc_failed) { (void)hipStreamSynchronize(s); return MPA_ERR_UNSUPPORTED; }
	return rc;
}
int dev_prechain_forward(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &pre, int32_t n_query, const int64_t *qfirst,
                         const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, const ChainParams *main, SeedHold *hold, const int64_t *jfirst_dev)
{
	return dev_seed_entry(ctx, mi, &pre, n_query, qfirst, jobs, n_jobs, out, main, hold, jfirst_dev, nullptr);
}
// Seeding without a pre-chain (-S, --no-pre-chain; MPA_GPU_SEED_NOPRE): sift by the main chain's reach, then the main chain itself
// (dev_seed_direct_impl).  Same contract as dev_prechain_forward(main != nullptr): out.has_chains, out.on_host.  kept != nullptr
// (test hook): stop behind the sift and hand out the kept anchors instead.
int dev_seed_direct(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &mainp, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs, int64_t n_jobs,
                    PrechainSparse &out, SeedHold *hold, const int64_t *jfirst_dev, SiftKept *kept)
{
	return dev_seed_entry(ctx, mi, nullptr, n_query, qfirst, jobs, n_jobs, out, &mainp, hold, jfirst_dev, kept);
}

// ki[] next to kb[] in HBM, on the first device sketch of a device.  The host array may be a misaligned view into a mapped .mpi:
// it is only ever copied byte-wise.  No device memory for it: the caller sketches on the host.
static int ensure_dev_ki(mpa_ctx_t *ctx, mpa_idx_s *mi, DeviceIndex *d)
{
	if (d->ki) return MPA_OK;
	static std::mutex mu[mpa_idx_s::kMaxDevices];            // (per device, like dev_upload_index)
	std::lock_guard<std::mutex> g(mu[ctx->device]);
	if (d->ki) return MPA_OK;
	int64_t *p = nullptr;
	const size_t bytes = mi->ki.size() * 8;
	if (hipMalloc((void**)&p, bytes + 16) != hipSuccess) { (void)hipGetLastError(); set_error("GPU sketch: no device memory for the bucket offsets"); return MPA_ERR_UNSUPPORTED; }
	const double t0 = now_ms();
	const hipError_t e = upload_large(p, (const void*)mi->ki.data(), bytes, ctx->stream);
	if (e != hipSuccess) { (void)hipFree(p); set_error(std::string("GPU sketch: uploading the bucket offsets: ") + hipGetErrorString(e)); return MPA_ERR_HIP; }
	timing_note("index upload: bucket offsets", now_ms() - t0);
	d->ki = p, d->ki_bytes = bytes + 16;
	g_dev_bytes += (long long)d->ki_bytes;
	return MPA_OK;
}

static int dev_sketch_jobs_impl(mpa_ctx_t *ctx, mpa_idx_s *mi, DeviceIndex *d, int32_t max_occ, const mpa_qbatch_t *q, SketchResult &out)
{
	SeedBufs &B = ctx->seed;
	hipStream_t s = ctx->seed_stream;
	const int32_t n_query = q->n_seq;
	const int64_t base = q->q_off[0], L = q->q_off[n_query] - base;
	const size_t NQ = (size_t)n_query, mq = (NQ + 1) * 8, fq = (NQ * 4 + 15) & ~(size_t)15;
	// one pinned block up: residue table | q_off (from 0) | protein text
	const size_t off_qo = 256, off_tx = off_qo + mq, up_bytes = off_tx + (size_t)L + 16;
	int rc;
	if ((rc = B.h_kin.ensure(up_bytes)) || (rc = B.k_in.ensure(up_bytes)) || (rc = B.k_cnt.ensure((size_t)L * 4 + 16)) || (rc = B.k_bkt.ensure((size_t)L * 4 + 16)) ||
	    (rc = B.k_q.ensure(4 * mq + 2 * fq)) || (rc = B.h_kout.ensure(2 * mq + 2 * fq)) || (rc = B.jobs.ensure(((size_t)L + 1) * sizeof(SeedJobDev)))) return rc;   // (a position ends at most one seed)
	char *hu = B.h_kin.as<char>();
	memcpy(hu, tab_aa13(), 256);
	{ int64_t *qo = (int64_t*)(hu + off_qo); for (int32_t i = 0; i <= n_query; ++i) qo[i] = q->q_off[i] - base; }
	if (L > 0) memcpy(hu + off_tx, q->seqs + base, (size_t)L);
	HIP_TRY(hipMemcpyAsync(B.k_in.p, hu, off_tx + (size_t)L, hipMemcpyHostToDevice, s));
	const char *din = B.k_in.as<char>();
	char *dq = B.k_q.as<char>();
	int64_t *d_na = (int64_t*)dq, *d_nk = (int64_t*)(dq + mq), *d_qfirst = (int64_t*)(dq + 2 * mq), *d_jfirst = (int64_t*)(dq + 3 * mq);
	int32_t *d_mo = (int32_t*)(dq + 4 * mq), *d_flag = (int32_t*)(dq + 4 * mq + fq);
	SketchParams sp;
	sp.n_bucket = (int64_t)mi->ki.size(), sp.n_kb = mi->n_kb, sp.kmer = mi->opt.kmer, sp.mod_bit = mi->opt.mod_bit, sp.max_occ = max_occ, sp.pad = 0;
	const unsigned nwg = (unsigned)((n_query + SKETCH_WAVES - 1) / SKETCH_WAVES);
	hipLaunchKernelGGL(k_sketch_count, dim3(nwg), dim3(64 * SKETCH_WAVES), 0, s, (const uint8_t*)(din + off_tx), (const int64_t*)(din + off_qo), n_query, (const uint8_t*)din,
	                   (const int64_t*)d->ki, sp, B.k_cnt.as<int32_t>(), B.k_bkt.as<uint32_t>(), d_na, d_nk, d_mo, d_flag);
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, (const int64_t*)d_na, (const int64_t*)d_nk, n_query, d_qfirst, d_jfirst);
	hipLaunchKernelGGL(k_sketch_emit, dim3(nwg), dim3(64 * SKETCH_WAVES), 0, s, (const int64_t*)(din + off_qo), n_query, (const int64_t*)d->ki, B.k_cnt.as<int32_t>(),
	                   B.k_bkt.as<uint32_t>(), (const int64_t*)d_qfirst, (const int64_t*)d_jfirst, (const int32_t*)d_mo, (const int32_t*)d_flag, B.jobs.as<SeedJobDev>());
	HIP_TRY(hipGetLastError());
	// qfirst | jfirst | cut-offs | flags: contiguous on the device, one copy, one wait
	char *hd = B.h_kout.as<char>();
	HIP_TRY(hipMemcpyAsync(hd, dq + 2 * mq, 2 * mq + 2 * fq, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	out.qfirst = (const int64_t*)hd, out.jfirst = (const int64_t*)(hd + mq), out.max_occ = (const int32_t*)(hd + 2 * mq), out.flag = (const int32_t*)(hd + 2 * mq + fq);
	out.n_anchor = out.qfirst[n_query], out.n_jobs = out.jfirst[n_query];
	for (int32_t i = 0; i < n_query; ++i) out.n_flagged += out.flag[i] != 0;
	return MPA_OK;
}

// The sketch stage of a mini-batch on the device (sketch_exec.hip): protein text up, the seed jobs of every query left in the
// seeder context's B.jobs for dev_prechain_forward(jfirst_dev), the two prefix arrays, cut-offs and flags back.  out points into
// pinned memory of the context, valid until its next sketch.  MPA_ERR_UNSUPPORTED: the caller runs the host stage.
int dev_sketch_jobs(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t max_occ, const mpa_qbatch_t *q, SketchResult &out)
{
	out = SketchResult();
	const mpa_idxopt_t &io = mi->opt;
	if (q->n_seq <= 0) { set_error("GPU sketch: an empty batch"); return MPA_ERR_UNSUPPORTED; }
	if (io.kmer < 1 || io.kmer > 7) { set_error("GPU sketch: k-mers of 1..7 residues only"); return MPA_ERR_UNSUPPORTED; }
	if (io.mod_bit < 0 || io.mod_bit >= 4 * io.kmer || mi->ki.size() != (size_t)1 << (4 * io.kmer - io.mod_bit)) { set_error("GPU sketch: the index has no k-mer table of 2^(4k - M) buckets"); return MPA_ERR_UNSUPPORTED; }
	if (q->q_off[q->n_seq] - q->q_off[0] >= (int64_t)INT32_MAX) { set_error("GPU sketch: too many seeds in a batch for 32-bit job indices"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	int rc = ensure_dev_ki(ctx, mi, d);
	if (rc != MPA_OK) return rc;
	ensure_seed_stream(ctx);
	tl_alloc_failed = false;
	rc = dev_sketch_jobs_impl(ctx, mi, d, max_occ, q, out);
	if (rc == MPA_ERR_HIP && tl_alloc_failed) { (void)hipStreamSynchronize(ctx->seed_stream); out = SketchResult(); return MPA_ERR_UNSUPPORTED; }   // (a pool could not grow: host stage)
	return rc;
}

// test hook (mpa_dbg_seed_jobs): the first n_jobs records of B.jobs, and the bucket that rides in their pad field
int dev_sketch_fetch(mpa_ctx_t *ctx, int64_t n_jobs, SeedJob *jobs, int32_t *bucket)
{
	if (n_jobs <= 0) return MPA_OK;
	SeedBufs &B = ctx->seed;
	if ((size_t)n_jobs * sizeof(SeedJobDev) > B.jobs.cap) { set_error("dev_sketch_fetch: more jobs than the context holds"); return MPA_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<SeedJobDev> h((size_t)n_jobs);
	HIP_TRY(hipMemcpyAsync(h.data(), B.jobs.p, (size_t)n_jobs * sizeof(SeedJobDev), hipMemcpyDeviceToHost, ctx->seed_stream));
	HIP_TRY(wait_stream(ctx, ctx->seed_stream));
	for (int64_t i = 0; i < n_jobs; ++i) {
		const SeedJobDev &j = h[(size_t)i];
		jobs[i] = SeedJob{ j.kb_off, j.dst, j.cnt, j.qpos, j.qid }, bucket[i] = j.pad;
	}
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// mp_idx_build's k-mer table on the device (index.c:52-136): scan (count, then emit), one radix sort of all keys, unique,
// bucket histogram + scan.  Leaves kb[] resident for the seeding kernels.  MPA_ERR_UNSUPPORTED (the caller builds on the host):
// parameters outside the kernel's range, or not enough device memory for the keys of this genome.
//
// The keys cost 44 bytes each while they are sorted (two key buffers, the sort's scratch, flags, a 64-bit scan, kb).  When that
// exceeds the budget, dev_index_build_passes builds the table in passes: a key is bucket << 32 | block, so the keys of a contiguous
// range of buckets give a contiguous slice of kb[] and that range's part of the bucket counts, and the ranges in ascending order
// concatenate into the bytes of the one-pass build.  A histogram of the keys over the top min(bucket bits, 12) bits of the bucket
// (k_index_scan<INDEX_HIST>) lets the host plan the fewest ranges that fit (idx_plan_passes); every pass counts and emits the keys of its
// range only (the RANGED instantiations), sorts, de-duplicates, adds to the one cnt[] array (indexed by absolute bucket) and hands its
// slice of kb[] to the host; the whole kb[] goes up once at the end, into the exact allocation a one-pass build leaves.
struct IndexPassEnv {
	mpa_ctx_t *ctx; mpa_idx_s *mi; DeviceIndex *d; hipStream_t s;
	IndexScanArgs a; size_t lds; int64_t n_chunk, n_keys; int bucket_bits; int64_t budget;
	DevBuf *b_count, *b_off, *b_tmp;
	double t0;
};

static int dev_index_build_passes(const IndexPassEnv &E)
{
	mpa_ctx_t *ctx = E.ctx;
	mpa_idx_s *mi = E.mi;
	hipStream_t s = E.s;
	const int64_t n_chunk = E.n_chunk;
	const size_t n_bucket = (size_t)1 << E.bucket_bits;
	const int hist_bits = std::min(E.bucket_bits, 12), hist_shift = E.bucket_bits - hist_bits, n_bin = 1 << hist_bits;
	const bool timed = timing_on();
	double ms_scan = 0;
	auto scan_clock = [&](double t) -> int { if (timed) { HIP_TRY(hipStreamSynchronize(s)); ms_scan += now_ms() - t; } return MPA_OK; };
	DevBuf b_hist, b_keys, b_keys2, b_flag, b_idx, b_kbp, b_cnt, b_ki;
	auto release_all = [&]() { for (DevBuf *b : { &b_hist, &b_keys, &b_keys2, &b_flag, &b_idx, &b_kbp, &b_cnt, &b_ki }) b->release(); };
	struct Guard { std::function<void()> f; ~Guard() { f(); } } guard{ release_all };
	int rc;
	// 1. the histogram
	if ((rc = b_hist.ensure_exact((size_t)n_bin * 8))) return rc;
	HIP_TRY(hipMemsetAsync(b_hist.p, 0, (size_t)n_bin * 8, s));
	double tc = timed ? now_ms() : 0;
	IndexPassArgs r{ n_chunk, b_hist.as<unsigned long long>(), hist_shift, n_bin, 0u, 0u };
	hipLaunchKernelGGL((k_index_scan<INDEX_HIST, false>), dim3((unsigned)std::min<int64_t>(n_chunk, 2048)), dim3(256), E.lds + (size_t)n_bin * 4, s, E.a, (uint32_t*)nullptr,
	                   (const uint64_t*)nullptr, (uint64_t*)nullptr, r);
	HIP_TRY(hipGetLastError());
	if ((rc = scan_clock(tc))) return rc;
	std::vector<int64_t> hist((size_t)n_bin);
	HIP_TRY(hipMemcpyAsync(hist.data(), b_hist.p, (size_t)n_bin * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	b_hist.release();
	int64_t hist_sum = 0, max_bin = 0;
	int32_t arg_max = 0;
	for (int32_t b = 0; b < n_bin; ++b) { hist_sum += hist[b]; if (hist[b] > max_bin) max_bin = hist[b], arg_max = b; }
	if (hist_sum != E.n_keys) { set_error("index build: the histogram of the keys does not add up to their count"); return MPA_ERR_HIP; }
	// 2. the plan
	const int64_t budget_keys = E.budget / 44;
	std::vector<int32_t> first_bin((size_t)n_bin + 1);
	const int32_t n_pass = idx_plan_passes(hist.data(), n_bin, budget_keys, first_bin.data());
	ctx->idx_stats.hist_bits = hist_bits, ctx->idx_stats.max_bin_keys = max_bin;
	ctx->idx_hist = hist;
	if (n_pass < 0) {
		set_error("index build: bin " + std::to_string(arg_max) + " of the " + std::to_string(n_bin) + "-bin key histogram holds " + std::to_string(max_bin) + " keys and would need " +
		          std::to_string(max_bin * 44) + " bytes of device memory, the budget is " + std::to_string(E.budget));
		return MPA_ERR_UNSUPPORTED;
	}
	int64_t max_pass = 0;
	std::vector<int64_t> pass_keys((size_t)n_pass, 0);
	for (int32_t p = 0; p < n_pass; ++p) {
		for (int32_t b = first_bin[p]; b < first_bin[p + 1]; ++b) pass_keys[p] += hist[b];
		max_pass = std::max(max_pass, pass_keys[p]);
	}
	// 3. the passes, over buffers sized once for the fullest of them
	if ((rc = b_keys.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_keys2.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_flag.ensure_exact((size_t)max_pass * 4 + 16)) ||
	    (rc = b_idx.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_kbp.ensure_exact((size_t)max_pass * 4 + 16)) || (rc = b_cnt.ensure_exact(n_bucket * 8)) ||
	    (rc = b_ki.ensure_exact(n_bucket * 8))) return rc;
	{
		size_t tmp_bytes = 0;
		HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)max_pass, 0u, 32u + (unsigned)E.bucket_bits, s));
		if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
	}
	HIP_TRY(hipMemsetAsync(b_cnt.p, 0, n_bucket * 8, s));
	std::vector<uint32_t> kb_new;
	kb_new.reserve((size_t)E.n_keys);                          // (an upper bound: the distinct keys are fewer)
	int64_t n_kb = 0;
	for (int32_t p = 0; p < n_pass; ++p) {
		const int64_t nk = pass_keys[p];
		if (nk == 0) continue;
		r.hist = nullptr, r.bin_lo = (uint32_t)first_bin[p], r.bin_hi = (uint32_t)first_bin[p + 1];
		tc = timed ? now_ms() : 0;
		hipLaunchKernelGGL((k_index_scan<INDEX_COUNT, true>), dim3((unsigned)n_chunk), dim3(256), E.lds, s, E.a, E.b_count->as<uint32_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr, r);
		HIP_TRY(hipGetLastError());
		if ((rc = scan_clock(tc))) return rc;
		{
			size_t tmp_bytes = 0;
			auto in = rocprim::make_transform_iterator(E.b_count->as<uint32_t>(), U32ToU64());
			HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, in, E.b_off->as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, rocprim::plus<uint64_t>(), s));
			if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
			HIP_TRY(rocprim::exclusive_scan(E.b_tmp->p, tmp_bytes, in, E.b_off->as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, rocprim::plus<uint64_t>(), s));
		}
		// (the emit pass writes at these offsets: they must add up to what the buffers were sized for)
		uint64_t last_off = 0;
		uint32_t last_cnt = 0;
		HIP_TRY(hipMemcpyAsync(&last_off, E.b_off->as<uint64_t>() + (n_chunk - 1), 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(&last_cnt, E.b_count->as<uint32_t>() + (n_chunk - 1), 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		if ((int64_t)(last_off + last_cnt) != nk) { set_error("index build: a pass counts other keys than the histogram gave it"); return MPA_ERR_HIP; }
		tc = timed ? now_ms() : 0;
		hipLaunchKernelGGL((k_index_scan<INDEX_EMIT, true>), dim3((unsigned)n_chunk), dim3(256), E.lds, s, E.a, (uint32_t*)nullptr, E.b_off->as<uint64_t>(), b_keys.as<uint64_t>(), r);
		HIP_TRY(hipGetLastError());
		if ((rc = scan_clock(tc))) return rc;
		{
			size_t tmp_bytes = 0;
			HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)nk, 0u, 32u + (unsigned)E.bucket_bits, s));
			if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
			HIP_TRY(rocprim::radix_sort_keys(E.b_tmp->p, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)nk, 0u, 32u + (unsigned)E.bucket_bits, s));
		}
		const uint64_t *sorted = b_keys2.as<uint64_t>();
		const unsigned nblk = (unsigned)((nk + 255) / 256);
		hipLaunchKernelGGL(k_index_flag, dim3(nblk), dim3(256), 0, s, sorted, nk, b_flag.as<uint32_t>());
		{
			size_t tmp_bytes = 0;
			auto in = rocprim::make_transform_iterator(b_flag.as<uint32_t>(), U32ToU64());
			HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, in, b_idx.as<uint64_t>(), (uint64_t)0, (size_t)nk, rocprim::plus<uint64_t>(), s));
			if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
			HIP_TRY(rocprim::exclusive_scan(E.b_tmp->p, tmp_bytes, in, b_idx.as<uint64_t>(), (uint64_t)0, (size_t)nk, rocprim::plus<uint64_t>(), s));
		}
		uint64_t last_idx = 0;
		uint32_t last_flag = 0;
		HIP_TRY(hipMemcpyAsync(&last_idx, b_idx.as<uint64_t>() + (nk - 1), 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(&last_flag, b_flag.as<uint32_t>() + (nk - 1), 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		const int64_t n_kb_pass = (int64_t)(last_idx + last_flag);
		if (n_kb_pass < 1 || n_kb_pass > nk) { set_error("index build: a pass has more distinct keys than keys"); return MPA_ERR_HIP; }
		hipLaunchKernelGGL(k_index_compact, dim3(nblk), dim3(256), 0, s, sorted, nk, b_flag.as<uint32_t>(), b_idx.as<uint64_t>(), b_kbp.as<uint32_t>(), b_cnt.as<unsigned long long>());
		HIP_TRY(hipGetLastError());
		kb_new.resize((size_t)(n_kb + n_kb_pass));
		HIP_TRY(hipMemcpyAsync(kb_new.data() + n_kb, b_kbp.p, (size_t)n_kb_pass * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		n_kb += n_kb_pass;
	}
	// 4. bucket boundaries from the counts of all passes; the pass buffers go before the whole kb[] comes up
	{
		size_t tmp_bytes = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, rocprim::plus<uint64_t>(), s));
		if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(E.b_tmp->p, tmp_bytes, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, rocprim::plus<uint64_t>(), s));
	}
	std::vector<int64_t> ki_new(n_bucket);
	HIP_TRY(hipMemcpyAsync(ki_new.data(), b_ki.p, n_bucket * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	release_all();
	uint32_t *d_kb = nullptr;
	HIP_TRY(hipMalloc((void**)&d_kb, (size_t)n_kb * 4 + 16));
	struct KbGuard { uint32_t *&p; hipStream_t s; ~KbGuard() { if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); } } } kb_guard{ d_kb, s };
	HIP_TRY(hipMemcpyAsync(d_kb, kb_new.data(), (size_t)n_kb * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(wait_stream(ctx, s));
	DeviceIndex *d = E.d;
	mi->ki.swap(ki_new), mi->kb.swap(kb_new), mi->n_kb = n_kb;
	if (d->kb) { (void)hipFree(d->kb); g_dev_bytes -= (long long)d->kb_bytes; }
	if (d->ki) { (void)hipFree(d->ki); g_dev_bytes -= (long long)d->ki_bytes; d->ki = nullptr, d->ki_bytes = 0; }
	d->kb = d_kb, d->kb_bytes = (size_t)n_kb * 4 + 16;
	g_dev_bytes += (long long)d->kb_bytes;
	d_kb = nullptr;
	ctx->idx_stats.n_pass = n_pass, ctx->idx_stats.max_pass_keys = max_pass;
	if (timed) {
		char note[64];
		snprintf(note, sizeof note, "index build on the GPU (%d passes)", (int)n_pass);
		timing_note("    index scans of all passes", ms_scan);
		timing_note(note, now_ms() - E.t0);
	}
	return MPA_OK;
}

int dev_index_build(mpa_ctx_t *ctx, mpa_idx_s *mi)
{
	const int32_t n_strand = (int32_t)mi->ctg.size() * 2;
	const mpa_idxopt_t &io = mi->opt;
	const int bucket_bits = io.kmer * 4 - io.mod_bit;
	if (n_strand == 0 || io.kmer < 1 || io.kmer > 7 || io.mod_bit < 0 || bucket_bits < 1 || bucket_bits > 28 || io.bbit < 0 || io.bbit > 20 || io.min_aa_len < io.kmer ||
	    io.min_aa_len > 1000) { set_error("index build: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	hipStream_t s = ctx->stream;
	std::vector<int64_t> chunk_first((size_t)n_strand + 1, 0);
	for (int32_t j = 0; j < n_strand; ++j) chunk_first[j + 1] = chunk_first[j] + (mi->ctg[j >> 1].len + REFINE_CHUNK - 1) / REFINE_CHUNK;
	const int64_t n_chunk = chunk_first[n_strand];
	if (n_chunk == 0 || n_chunk > 0x7fffffff) { set_error("index build: genome too small or too large for one launch"); return MPA_ERR_UNSUPPORTED; }
	const size_t n_bucket = (size_t)1 << bucket_bits;
	DevBuf b_first, b_bo, b_count, b_off, b_keys, b_keys2, b_flag, b_idx, b_tmp, b_cnt, b_ki;
	auto release_all = [&]() { for (DevBuf *b : { &b_first, &b_bo, &b_count, &b_off, &b_keys, &b_keys2, &b_flag, &b_idx, &b_tmp, &b_cnt, &b_ki }) b->release(); };
	struct Guard { std::function<void()> f; ~Guard() { f(); } } guard{ release_all };
	int rc;
	if ((rc = b_first.ensure(((size_t)n_strand + 1) * 8)) || (rc = b_bo.ensure((size_t)n_strand * 4 + 4)) || (rc = b_count.ensure((size_t)n_chunk * 4 + 4)) ||
	    (rc = b_off.ensure(((size_t)n_chunk + 1) * 8))) return rc;
	HIP_TRY(hipMemcpyAsync(b_first.p, chunk_first.data(), ((size_t)n_strand + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(b_bo.p, mi->bo.data(), (size_t)n_strand * 4, hipMemcpyHostToDevice, s));
	IndexScanArgs a;
	a.g = DevGenome{ d->seq, d->ctg_off, d->ctg_len, nullptr, mi->l_seq };
	a.chunk_first = b_first.as<int64_t>(), a.bo = b_bo.as<uint32_t>();
	a.n_strand = n_strand, a.kmer = io.kmer, a.mod_bit = io.mod_bit, a.bbit = io.bbit, a.min_aa_len = io.min_aa_len, a.halo = (3 * io.min_aa_len + 2 + 15) & ~15;
	for (int c = 0; c < 64; ++c) a.rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	const size_t lds = (size_t)REFINE_CHUNK + 2 * (size_t)a.halo;
	const double t0 = now_ms();
	ctx->idx_stats = mpa_idx_build_stats_t{}, ctx->idx_stats.n_pass = 1;
	ctx->idx_hist.clear();
	hipLaunchKernelGGL((k_index_scan<INDEX_COUNT, false>), dim3((unsigned)n_chunk), dim3(256), lds, s, a, b_count.as<uint32_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr, IndexPassArgs{});
	HIP_TRY(hipGetLastError());
	// exclusive scan of the per-chunk counts (as 64-bit offsets)
	{
		size_t tmp_bytes = 0;
		auto in = rocprim::make_transform_iterator(b_count.as<uint32_t>(), U32ToU64());
		HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, in, b_off.as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, rocprim::plus<uint64_t>(), s));
		if ((rc = b_tmp.ensure(tmp_bytes + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(b_tmp.p, tmp_bytes, in, b_off.as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, rocprim::plus<uint64_t>(), s));
	}
	uint64_t last_off = 0;
	uint32_t last_cnt = 0;
	HIP_TRY(hipMemcpyAsync(&last_off, b_off.as<uint64_t>() + (n_chunk - 1), 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(&last_cnt, b_count.as<uint32_t>() + (n_chunk - 1), 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t n_keys = (int64_t)(last_off + last_cnt);
	if (n_keys == 0) { mi->ki.assign(n_bucket, 0), mi->kb.clear(), mi->n_kb = 0; return MPA_OK; }
	{	// two key buffers, flags, scan, kb: ~40 bytes per key.  The budget for them is 7/8 of the free memory less the two bucket
		// tables, which every build needs; MPA_IDX_BUILD_MB (read on every call: for users who share a device) and the tests' hook cap it
		size_t free_b = 0, total_b = 0;
		int64_t budget = INT64_MAX;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			if (n_bucket * 16 > free_b - (free_b >> 3)) { set_error("index build: not enough device memory for the bucket tables of this index"); return MPA_ERR_UNSUPPORTED; }
			budget = (int64_t)(free_b - (free_b >> 3) - n_bucket * 16);
		}
		const char *e = getenv("MPA_IDX_BUILD_MB");
		if (e && atoll(e) > 0) budget = std::min<int64_t>(budget, atoll(e) << 20);
		if (ctx->idx_budget_dbg > 0) budget = std::min(budget, ctx->idx_budget_dbg);
		ctx->idx_stats.n_keys = n_keys, ctx->idx_stats.max_pass_keys = n_keys, ctx->idx_stats.budget_bytes = budget;
		if (n_keys > budget / 44) {
			ctx->idx_stats.n_pass = 0, ctx->idx_stats.max_pass_keys = 0;
			return dev_index_build_passes(IndexPassEnv{ ctx, mi, d, s, a, lds, n_chunk, n_keys, bucket_bits, budget, &b_count, &b_off, &b_tmp, t0 });
		}
	}
	if ((rc = b_keys.ensure((size_t)n_keys * 8)) || (rc = b_keys2.ensure((size_t)n_keys * 8))) return rc;
	hipLaunchKernelGGL((k_index_scan<INDEX_EMIT, false>), dim3((unsigned)n_chunk), dim3(256), lds, s, a, (uint32_t*)nullptr, b_off.as<uint64_t>(), b_keys.as<uint64_t>(), IndexPassArgs{});
	HIP_TRY(hipGetLastError());
	int nb = 1;
	while ((1ULL << nb) < (uint64_t)mi->n_block + 1) ++nb;
	{
		size_t tmp_bytes = 0;
		HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)n_keys, 0u, 32u + (unsigned)bucket_bits, s));
		if ((rc = b_tmp.ensure(tmp_bytes + 256))) return rc;
		HIP_TRY(rocprim::radix_sort_keys(b_tmp.p, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)n_keys, 0u, 32u + (unsigned)bucket_bits, s));
	}
	(void)nb;
	b_keys.release();
	const uint64_t *sorted = b_keys2.as<uint64_t>();
	if ((rc = b_flag.ensure((size_t)n_keys * 4)) || (rc = b_idx.ensure((size_t)n_keys * 8)) || (rc = b_cnt.ensure(n_bucket * 8)) || (rc = b_ki.ensure(n_bucket * 8))) return rc;
	const unsigned nblk = (unsigned)((n_keys + 255) / 256);
	hipLaunchKernelGGL(k_index_flag, dim3(nblk), dim3(256), 0, s, sorted, n_keys, b_flag.as<uint32_t>());
	{
		size_t tmp_bytes = 0;
		auto in = rocprim::make_transform_iterator(b_flag.as<uint32_t>(), U32ToU64());
		HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, in, b_idx.as<uint64_t>(), (uint64_t)0, (size_t)n_keys, rocprim::plus<uint64_t>(), s));
		if ((rc = b_tmp.ensure(tmp_bytes + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(b_tmp.p, tmp_bytes, in, b_idx.as<uint64_t>(), (uint64_t)0, (size_t)n_keys, rocprim::plus<uint64_t>(), s));
	}
	uint64_t last_idx = 0;
	uint32_t last_flag = 0;
	HIP_TRY(hipMemcpyAsync(&last_idx, b_idx.as<uint64_t>() + (n_keys - 1), 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(&last_flag, b_flag.as<uint32_t>() + (n_keys - 1), 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t n_kb = (int64_t)(last_idx + last_flag);
	uint32_t *d_kb = nullptr;
	HIP_TRY(hipMalloc((void**)&d_kb, (size_t)n_kb * 4 + 16));
	struct KbGuard { uint32_t *&p; hipStream_t s; ~KbGuard() { if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); } } } kb_guard{ d_kb, s };   // freed on every error path below
	HIP_TRY(hipMemsetAsync(b_cnt.p, 0, n_bucket * 8, s));
	hipLaunchKernelGGL(k_index_compact, dim3(nblk), dim3(256), 0, s, sorted, n_keys, b_flag.as<uint32_t>(), b_idx.as<uint64_t>(), d_kb, b_cnt.as<unsigned long long>());
	{
		size_t tmp_bytes = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, rocprim::plus<uint64_t>(), s));
		if ((rc = b_tmp.ensure(tmp_bytes + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(b_tmp.p, tmp_bytes, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, rocprim::plus<uint64_t>(), s));
	}
	HIP_TRY(hipGetLastError());
	// (into temporaries: a copy that fails must not leave the index with a half-filled table)
	std::vector<int64_t> ki_new(n_bucket);
	std::vector<uint32_t> kb_new((size_t)n_kb);
	HIP_TRY(hipMemcpyAsync(ki_new.data(), b_ki.p, n_bucket * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(kb_new.data(), d_kb, (size_t)n_kb * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	mi->ki.swap(ki_new), mi->kb.swap(kb_new), mi->n_kb = n_kb;
	if (d->kb) { (void)hipFree(d->kb); g_dev_bytes -= (long long)d->kb_bytes; }
	if (d->ki) { (void)hipFree(d->ki); g_dev_bytes -= (long long)d->ki_bytes; d->ki = nullptr, d->ki_bytes = 0; }   // (the new table's offsets go up with the first device sketch)
	d->kb = d_kb, d->kb_bytes = (size_t)n_kb * 4 + 16;     // stays resident for the seeding kernels
	g_dev_bytes += (long long)d->kb_bytes;
	d_kb = nullptr;                                        // (ownership moved: the guard lets go)
	timing_note("index build on the GPU", now_ms() - t0);
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// Forward pass of mp_chain for a batch of chaining problems on the device (k_chain_fwd): the main chain of every query of a
// mini-batch, or the refinement chains of its regions.  The caller writes the sorted anchors of all problems, back to back,
// into io.a (pinned memory of the context) and finds f / pred (index inside the problem) in io.f / io.pred afterwards.
int dev_chain_buffers(mpa_ctx_t *ctx, int64_t n, ChainIO &io)
{
	SeedBufs &B = ctx->seed;
	int rc;
	if ((rc = B.hc_a.ensure((size_t)n * 8 + 64)) || (rc = B.hc_f.ensure((size_t)n * 4 + 64)) || (rc = B.hc_pred.ensure((size_t)n * 4 + 64))) return rc;
	io.a = B.hc_a.as<uint64_t>(), io.f = B.hc_f.as<int32_t>(), io.pred = B.hc_pred.as<int32_t>();
	return MPA_OK;
}

int dev_chain_forward(mpa_ctx_t *ctx, const ChainParams &cp, int32_t n_prob, const int64_t *first, const ChainIO &io)
{
	const int64_t n = first[n_prob];
	if (n == 0 || n_prob == 0) return MPA_OK;
	if (n_prob > (1 << 30) || cp.kmer < 0) { set_error("chain forward pass: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	for (int32_t q = 0; q < n_prob; ++q)
		if (first[q + 1] - first[q] > INT32_MAX - 2) { set_error("chain forward pass: a problem has too many anchors"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	PreParams pp;
	pp.max_dist_x = std::max(cp.max_dist_x, cp.bw), pp.max_dist_y = cp.max_dist_y;
	if (pp.max_dist_y < cp.bw && !cp.is_spliced) pp.max_dist_y = cp.bw;
	pp.bw = cp.bw, pp.max_skip = cp.max_skip, pp.max_iter = cp.max_iter, pp.kmer = cp.kmer, pp.bbit = cp.bbit;
	pp.is_spliced = cp.is_spliced, pp.coef_log = cp.coef_log, pp.max_dblock = pp.max_dist_x >> cp.bbit;
	int rc;
	if ((rc = B.c_a.ensure((size_t)n * 8)) || (rc = B.c_f.ensure((size_t)n * 4)) || (rc = B.c_pred.ensure((size_t)n * 4)) || (rc = B.c_mark.ensure((size_t)n * 4)) ||
	    (rc = B.c_flag.ensure((size_t)n * 4)) || (rc = B.c_first.ensure(((size_t)n_prob + 1) * 8))) return rc;
	// runs longer than this get a wavefront each (k_chain_fwd_wave); MPA_CHAIN_SERIAL_RUN overrides (tests: 4 = almost every run)
	const int32_t serial_run = [] { const char *e = getenv("MPA_CHAIN_SERIAL_RUN"); return e ? std::max(1, atoi(e)) : 48; }();
	const size_t long_cap = (size_t)n / (size_t)(serial_run + 1) + 16;
	if ((rc = B.c_long.ensure(64 + long_cap * sizeof(LongRun)))) return rc;
	unsigned int *d_nlong = B.c_long.as<unsigned int>();
	LongRun *d_long = (LongRun*)(B.c_long.as<char>() + 64);
	HIP_TRY(hipMemsetAsync(d_nlong, 0, 64, s));
	HIP_TRY(hipMemcpyAsync(B.c_a.p, io.a, (size_t)n * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(B.c_first.p, first, ((size_t)n_prob + 1) * 8, hipMemcpyHostToDevice, s));
	const unsigned nblk = (unsigned)((n + 255) / 256);
	hipLaunchKernelGGL(k_seed_fill, dim3(nblk), dim3(256), 0, s, n, pp.kmer, B.c_f.as<int32_t>(), B.c_pred.as<int32_t>(), B.c_mark.as<int32_t>(), B.c_flag.as<uint32_t>());
	hipLaunchKernelGGL(k_chain_fwd, dim3(nblk), dim3(256), 0, s, B.c_a.as<uint64_t>(), n, B.c_first.as<int64_t>(), (const int64_t*)nullptr, n_prob, pp, B.c_f.as<int32_t>(), B.c_pred.as<int32_t>(),
	                   B.c_mark.as<int32_t>(), serial_run, d_long, d_nlong, (unsigned int)long_cap);
	hipLaunchKernelGGL(k_chain_fwd_wave, dim3((unsigned)std::min<size_t>(long_cap, 65536)), dim3(64), 0, s, B.c_a.as<uint64_t>(), (const LongRun*)d_long, (const unsigned int*)d_nlong,
	                   (unsigned int)long_cap, pp, B.c_f.as<int32_t>(), B.c_pred.as<int32_t>(), B.c_mark.as<int32_t>());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(io.f, B.c_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(io.pred, B.c_pred.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));                       // (first[] may be pageable memory of the caller: it is consumed by now)
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// MPA_REFINE_GMAP_MIN: from how many entries (groups in dev_refine_chains, k-mers in dev_refine_scan) a query's k-mer table lives in
// device memory instead of LDS.  Unset = lds_max + 1, the first size the LDS classes do not take; a smaller number sends more
// queries there (1 = every query: the tests); "off" = none, and a batch with a longer query is declined.  Read on every call.
// Returns the threshold, or -1 for "off".
static int64_t refine_gmap_min(int64_t lds_max)
{
	const char *e = getenv("MPA_REFINE_GMAP_MIN");
	if (!e || !*e) return lds_max + 1;
	if (!strcmp(e, "off")) return -1;
	const long long v = atoll(e);
	return v < 1 ? lds_max + 1 : std::min<int64_t>(v, lds_max + 1);
}
// The tables of a call's long queries: slots per query (power of two >= 2 x entries, at least 1 024), their places in the pool.
struct GmapPlan {
	std::vector<int32_t> long_q;          // the queries that get a table
	std::vector<int64_t> desc;            // [n_query] first slot << 8 | log2 slots (0 for the others)
	int64_t n_slots = 0, max_entries = 0;
	void add(int32_t q, int64_t entries) {
		int lg = 10;
		while ((1LL << lg) < 2 * entries) ++lg;
		long_q.push_back(q), desc[(size_t)q] = n_slots << 8 | lg;
		n_slots += 1LL << lg, max_entries = std::max(max_entries, entries);
	}
};
// memset + build of the tables on stream s: d_first / d_words = the entries of every query on the device, d_long / d_desc = the plan
static int gmap_build(SeedBufs &B, hipStream_t s, const GmapPlan &gp, const int64_t *d_first, const uint32_t *d_words, const int32_t *d_long, const int64_t *d_desc)
{
	HIP_TRY(hipMemsetAsync(B.r_gmap.p, 0xff, (size_t)gp.n_slots * 8, s));
	const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (gp.max_entries + 255) / 256));
	for (size_t k = 0; k < gp.long_q.size(); k += 65535)            // (gridDim.y)
		hipLaunchKernelGGL(k_refine_gmap_build, dim3(gx, (unsigned)std::min<size_t>(65535, gp.long_q.size() - k)), dim3(256), 0, s, d_first, d_words, d_long + k, d_desc, B.r_gmap.as<uint32_t>());
	HIP_TRY(hipGetLastError());
	return MPA_OK;
}

// Refinement scan of a mini-batch's region windows on the device (k_refine_scan).  qw_first/qwords: the k-mer words
// of every query.  out.first[w] .. out.first[w+1]: the hits (hash << 32 | window position) of window w, unsorted.
// Windows of a query with more than 4 096 k-mers (MPA_REFINE_GMAP_MIN) go to a second launch that probes the query's table in
// device memory (k_refine_scan_gset).  MPA_ERR_UNSUPPORTED (the caller scans on the host): k too large.
int dev_refine_scan(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t n_query, const int64_t *qw_first, const uint32_t *qwords,
                    int64_t n_win, const RefineWindow *wins, RefineHits &out)
{
	out.first.assign((size_t)n_win + 1, 0);
	out.hits.clear();
	if (n_win == 0) return MPA_OK;
	static_assert(REFINE_HALO == kRefineHaloBases, "dev_refine_in_range() states the halo of the scan kernels");
	if (!dev_refine_in_range(kmer, min_aa_len)) { set_error("refinement scan: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	const int64_t gmin = refine_gmap_min(4096);
	GmapPlan gp;
	gp.desc.assign((size_t)n_query, 0);
	std::vector<uint8_t> q_used((size_t)n_query, 0);
	for (int64_t k = 0; k < n_win; ++k) if (wins[k].len > 0) q_used[(size_t)wins[k].qid] = 1;
	int64_t max_words = 0;                                     // ... of the queries whose set goes to LDS
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t nw = qw_first[q + 1] - qw_first[q];
		if (gmin > 0 && nw >= gmin) { if (q_used[(size_t)q]) gp.add(q, nw); }
		else max_words = std::max(max_words, nw);
	}
	int hs_log2 = 10;
	while ((1LL << hs_log2) < 2 * max_words) ++hs_log2;
	if (hs_log2 > 13) { set_error("refinement scan: query too long for the LDS k-mer set"); return MPA_ERR_UNSUPPORTED; }
	const size_t n_long = gp.long_q.size();
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	// windows, chunks, the queries' k-mer words: laid out in ONE pinned block and uploaded with one copy (pageable copies are
	// staged by the runtime, synchronously and spinning)
	int64_t n_pos = 0, n_chunk = 0;
	for (int64_t k = 0; k < n_win; ++k) n_pos += wins[k].len, n_chunk += (wins[k].len + REFINE_CHUNK - 1) / REFINE_CHUNK;
	if (n_chunk == 0) return MPA_OK;
	const unsigned long long cap = (unsigned long long)(n_pos / 64 + (1 << 20));   // ~0.04 % of the positions hit on random sequence
	const int64_t n_words = qw_first[n_query];
	auto al64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t o_win = 0, o_chunk = al64((size_t)n_win * sizeof(RefineWindowDev)), o_qf = o_chunk + al64((size_t)n_chunk * sizeof(RefineChunk)),
	             o_words = o_qf + al64(((size_t)n_query + 1) * 8), o_gd = o_words + al64((size_t)n_words * 4 + 16), o_lq = o_gd + al64((size_t)n_query * 8 + 8),
	             up_bytes = o_lq + al64(n_long * 4 + 4);
	int rc;
	if ((rc = B.h_meta.ensure(up_bytes + 64)) || (rc = B.r_win.ensure(up_bytes)) || (rc = B.r_hits.ensure((size_t)cap * 16)) || (rc = B.r_count.ensure(16)) ||
	    (rc = B.h_back.ensure(64)) || (n_long && (rc = B.r_gmap.ensure((size_t)gp.n_slots * 8)))) return rc;
	char *hm = B.h_meta.as<char>();
	int64_t c_lds = 0;                                         // the chunks of the LDS launch come first, then those of the long queries' windows
	{
		RefineWindowDev *dw = (RefineWindowDev*)(hm + o_win);
		RefineChunk *ch = (RefineChunk*)(hm + o_chunk);
		int64_t c = 0;
		for (int pass = 0; pass < 2; ++pass) {
			for (int64_t k = 0; k < n_win; ++k) {
				if (pass == 0) dw[k] = RefineWindowDev{ wins[k].as, wins[k].qid, wins[k].vid, wins[k].len, 0 };
				if ((gp.desc[(size_t)wins[k].qid] != 0) != (pass == 1)) continue;
				for (int32_t st = 0; st < wins[k].len; st += REFINE_CHUNK) ch[c++] = RefineChunk{ (int32_t)k, st };
			}
			if (pass == 0) c_lds = c;
		}
		memcpy(hm + o_qf, qw_first, ((size_t)n_query + 1) * 8);
		memcpy(hm + o_words, qwords, (size_t)n_words * 4);
		memcpy(hm + o_gd, gp.desc.data(), (size_t)n_query * 8);
		if (n_long) memcpy(hm + o_lq, gp.long_q.data(), n_long * 4);
	}
	HIP_TRY(hipMemcpyAsync(B.r_win.p, hm, up_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.r_count.p, 0, 16, s));
	RefineTab rt;
	for (int c = 0; c < 64; ++c) rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, nullptr, mi->l_seq };
	const size_t lds = ((size_t)4 << hs_log2) + REFINE_CHUNK + 2 * REFINE_HALO;
	const char *dm = B.r_win.as<char>();
	if (c_lds > 0)
		hipLaunchKernelGGL(k_refine_scan, dim3((unsigned)c_lds), dim3(256), lds, s, dg, (const RefineWindowDev*)(dm + o_win), (const RefineChunk*)(dm + o_chunk),
		                   (const int64_t*)(dm + o_qf), (const uint32_t*)(dm + o_words), rt, kmer, min_aa_len, hs_log2, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap);
	if (n_chunk > c_lds) {
		if ((rc = gmap_build(B, s, gp, (const int64_t*)(dm + o_qf), (const uint32_t*)(dm + o_words), (const int32_t*)(dm + o_lq), (const int64_t*)(dm + o_gd)))) return rc;
		hipLaunchKernelGGL(k_refine_scan_gset, dim3((unsigned)(n_chunk - c_lds)), dim3(256), REFINE_CHUNK + 2 * REFINE_HALO, s, dg, (const RefineWindowDev*)(dm + o_win),
		                   (const RefineChunk*)(dm + o_chunk) + c_lds, rt, kmer, min_aa_len, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap,
		                   RefineGmap{ B.r_gmap.as<uint2>(), (const int64_t*)(dm + o_gd) });
		if (timing_on()) fprintf(stderr, "[mpa-timing]     refine scan: global-set launch (%zu queries, %lld chunks)\n", n_long, (long long)(n_chunk - c_lds));
	}
	HIP_TRY(hipGetLastError());
	unsigned long long *h_n = B.h_back.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(h_n, B.r_count.p, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const unsigned long long n_hits = *h_n;
	if (n_hits > cap) { set_error("refinement scan: more hits than the buffer holds"); return MPA_ERR_UNSUPPORTED; }
	if (n_hits == 0) return MPA_OK;
	if ((rc = B.h_rhits.ensure((size_t)n_hits * 16)) != MPA_OK) return rc;
	HIP_TRY(hipMemcpyAsync(B.h_rhits.p, B.r_hits.p, (size_t)n_hits * 16, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	// group by window (counting sort)
	const uint4 *h = B.h_rhits.as<uint4>();
	for (unsigned long long k = 0; k < n_hits; ++k) ++out.first[(size_t)h[k].x + 1];
	for (int64_t k = 0; k < n_win; ++k) out.first[(size_t)k + 1] += out.first[(size_t)k];
	out.hits.resize((size_t)n_hits);
	std::vector<int64_t> at(out.first.begin(), out.first.end() - 1);
	for (unsigned long long k = 0; k < n_hits; ++k) out.hits[(size_t)at[h[k].x]++] = (uint64_t)h[k].z << 32 | h[k].y;
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// mp_refine_reg (map.c:32-96) for all windows of a mini-batch on the device: see the kernels in seed_exec.hip ("Refinement
// pairing on the device") and k_chain_fwd / k_chain_fwd_wave / k_chain_extract.  MPA_ERR_UNSUPPORTED: outside the kernels' range
// (the caller refines on the host).  out.on_host[w] = 1: this window alone is the host's (2^22 bases or more, or a query with a
// position of 2^22 or more -- the sort key window << 44 | position << 22 | query position holds neither); its chains come back empty.
// A query with more groups than the largest LDS map takes (MPA_REFINE_GMAP_MIN) gets its map in device memory: a fourth launch.
int dev_refine_chains(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t max_ava, const ChainParams &cp, int32_t n_query, const RefineGroupsHost &G,
                      int64_t n_win, const RefineWindow *wins, RefineChains &out)
{
	out.u_first.assign((size_t)n_win + 1, 0), out.a_first.assign((size_t)n_win + 1, 0);
	out.U = out.A = nullptr;
	out.on_host.assign((size_t)n_win, 0);
	if (n_win == 0) return MPA_OK;
	if (!dev_refine_in_range(kmer, min_aa_len) || cp.bbit != 0) { set_error("device refinement: parameters outside the kernels' range"); return MPA_ERR_UNSUPPORTED; }
	if (n_win >= (1 << 20)) { set_error("device refinement: more than 2^20 windows in a batch"); return MPA_ERR_UNSUPPORTED; }
	const int64_t gmin = refine_gmap_min(2048);
	// which windows the device takes, and the size class of every query that has one: 0..2 = LDS map of 1 024 / 2 048 / 4 096 slots, 3 = map in device memory
	std::vector<uint8_t> q_far((size_t)n_query, 0);
	std::vector<int8_t> q_cls((size_t)n_query, -1);
	for (int32_t q = 0; q < n_query; ++q) {
		const int64_t g0 = G.qg_first[(size_t)q], g1 = G.qg_first[(size_t)q + 1];
		const size_t p0 = g0 < g1 ? G.gfirst[(size_t)g0] : 0, p1 = g0 < g1 ? (size_t)G.gfirst[(size_t)g1 - 1] + G.gcount[(size_t)g1 - 1] : 0;
		for (size_t k = p0; k < p1; ++k) if (G.qpos[k] >= (1u << 22)) { q_far[(size_t)q] = 1; break; }
	}
	GmapPlan gp;
	gp.desc.assign((size_t)n_query, 0);
	int64_t n_long_win = 0;
	for (int64_t k = 0; k < n_win; ++k) {
		const size_t q = (size_t)wins[k].qid;
		if (wins[k].len >= (1 << 22) || q_far[q]) { out.on_host[(size_t)k] = 1; continue; }
		if (q_cls[q] < 0) {
			const int64_t ng = G.qg_first[q + 1] - G.qg_first[q];
			if (gmin > 0 && ng >= gmin) q_cls[q] = 3, gp.add((int32_t)q, ng);
			else if (2 * ng > 4096) { set_error("device refinement: query too long for the LDS k-mer map"); return MPA_ERR_UNSUPPORTED; }
			else q_cls[q] = 2 * ng <= 1024 ? 0 : 2 * ng <= 2048 ? 1 : 2;
		}
		n_long_win += q_cls[q] == 3;
	}
	const size_t n_long = gp.long_q.size();
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	SeedBufs &B = ctx->seed;
	ensure_seed_stream(ctx);
	hipStream_t s = ctx->seed_stream;
	const double t0 = now_ms();
	// ---- one pinned block up: windows | chunks | wg_first | qg_first | gword | gfirst | gcount | qpos
	static const int n_super = [] { const char *e = getenv("MPA_REFINE_SUPER"); const int v = e ? atoi(e) : REFINE_SUPER; return v < 1 ? 1 : v > 16 ? 16 : v; }();
	int64_t n_pos = 0, n_chunk = 0, wg_total = 0;
	for (int64_t k = 0; k < n_win; ++k) {
		if (out.on_host[(size_t)k]) continue;
		n_pos += wins[k].len, n_chunk += (wins[k].len + n_super * REFINE_CHUNK - 1) / (n_super * REFINE_CHUNK);   // (a workgroup sweeps n_super chunks of its window)
	}
	if (n_chunk == 0) return MPA_OK;
	const unsigned long long cap = (unsigned long long)(n_pos / 64 + (1 << 20));
	const size_t n_group = G.gword.size(), n_qpos = G.qpos.size(), NW = (size_t)n_win, NQ = (size_t)n_query;
	auto al64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t o_win = 0, o_chunk = al64(NW * sizeof(RefineWindowDev)), o_wg = o_chunk + al64((size_t)n_chunk * sizeof(RefineChunk)), o_qg = o_wg + al64((NW + 1) * 8),
	             o_gw = o_qg + al64((NQ + 1) * 8), o_gf = o_gw + al64(n_group * 4 + 4), o_gc = o_gf + al64(n_group * 4 + 4), o_qp = o_gc + al64(n_group * 4 + 4),
	             o_gd = o_qp + al64(n_qpos * 4 + 4), o_lq = o_gd + al64(NQ * 8 + 8), up_bytes = o_lq + al64(n_long * 4 + 4);
	int rc;
	int64_t cls_end[4] = { 0, 0, 0, 0 };                       // chunks of the windows whose query's map has 1 024 / 2 048 / 4 096 LDS slots, or lives in device memory, end here
	if ((rc = B.h_meta.ensure(up_bytes + 64)) || (rc = B.r_win.ensure(up_bytes)) || (rc = B.r_hits.ensure((size_t)cap * 16)) || (rc = B.r_count.ensure(16)) ||
	    (rc = B.h_back.ensure(256)) || (n_long && (rc = B.r_gmap.ensure((size_t)gp.n_slots * 8)))) return rc;
	char *hm = B.h_meta.as<char>();
	{
		RefineWindowDev *dw = (RefineWindowDev*)(hm + o_win);
		RefineChunk *ch = (RefineChunk*)(hm + o_chunk);
		int64_t *wg = (int64_t*)(hm + o_wg);
		for (int64_t k = 0; k < n_win; ++k) {
			dw[k] = RefineWindowDev{ wins[k].as, wins[k].qid, wins[k].vid, wins[k].len, 0 };
			wg[k] = wg_total;
			if (!out.on_host[(size_t)k]) wg_total += G.qg_first[(size_t)wins[k].qid + 1] - G.qg_first[(size_t)wins[k].qid];   // (a window of the host has no workgroup, no hits, no pairs: an empty problem)
		}
		wg[n_win] = wg_total;
		// the workgroups of a window, grouped by the size of its query's k-mer map (1 024 / 2 048 / 4 096 slots, or a table in device
		// memory): one launch per size, so that the windows of ordinary proteins take 13 KB of LDS per workgroup and not the 37 KB the
		// longest protein of the LDS classes needs
		int64_t c = 0;
		for (int cls = 0; cls < 4; ++cls) {
			for (int64_t k = 0; k < n_win; ++k) {
				if (out.on_host[(size_t)k] || q_cls[(size_t)wins[k].qid] != cls) continue;
				for (int32_t st = 0; st < wins[k].len; st += n_super * REFINE_CHUNK) ch[c++] = RefineChunk{ (int32_t)k, st };
			}
			cls_end[cls] = c;
		}
		memcpy(hm + o_qg, G.qg_first.data(), (NQ + 1) * 8);
		if (n_group) memcpy(hm + o_gw, G.gword.data(), n_group * 4), memcpy(hm + o_gf, G.gfirst.data(), n_group * 4), memcpy(hm + o_gc, G.gcount.data(), n_group * 4);
		if (n_qpos) memcpy(hm + o_qp, G.qpos.data(), n_qpos * 4);
		memcpy(hm + o_gd, gp.desc.data(), NQ * 8);
		if (n_long) memcpy(hm + o_lq, gp.long_q.data(), n_long * 4);
	}
	// device tables: per (window, group) hit counts and per-window pair counts, zeroed
	size_t at = 0;
	auto carve = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
	const size_t o_wcnt = carve(((size_t)wg_total + 1) * 4), o_wpairs = carve((NW + 2) * 4), o_first = carve((NW + 2) * 8);
	const size_t zero_bytes = at;
	if ((rc = B.rx_all.ensure(at))) return rc;
	HIP_TRY(hipMemcpyAsync(B.r_win.p, hm, up_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemsetAsync(B.r_count.p, 0, 16, s));
	HIP_TRY(hipMemsetAsync(B.rx_all.p, 0, zero_bytes, s));
	RefineTab rt;
	for (int c = 0; c < 64; ++c) rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, nullptr, mi->l_seq };
	const char *dm = B.r_win.as<char>();
	RefineGroups gr{ (const int64_t*)(dm + o_qg), (const uint32_t*)(dm + o_gw), (const uint32_t*)(dm + o_gf), (const uint32_t*)(dm + o_gc), (const uint32_t*)(dm + o_qp) };
	const int64_t *d_wg = (const int64_t*)(dm + o_wg);
	char *R = B.rx_all.as<char>();
	uint32_t *d_wcnt = (uint32_t*)(R + o_wcnt), *d_wpairs = (uint32_t*)(R + o_wpairs);
	int64_t *d_first = (int64_t*)(R + o_first);
	HIP_TRY(ensure_dynamic_lds((const void*)k_refine_scan_map, ctx->device, 48 * 1024));
	for (int cls = 0; cls < 3; ++cls) {
		const int64_t c_first = cls ? cls_end[cls - 1] : 0, c_n = cls_end[cls] - c_first;
		if (c_n == 0) continue;
		const int hs = 10 + cls;
		const size_t lds = ((size_t)8 << hs) + 2 * (REFINE_CHUNK + 2 * REFINE_HALO);   // k-mer map, bases, codons
		hipLaunchKernelGGL(k_refine_scan_map, dim3((unsigned)c_n), dim3(256), lds, s, dg, (const RefineWindowDev*)(dm + o_win), (const RefineChunk*)(dm + o_chunk) + c_first, gr, d_wg, rt,
		                   kmer, min_aa_len, hs, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap, d_wcnt, (int32_t)n_super);
	}
	if (cls_end[3] > cls_end[2]) {                             // the long queries: their tables once per batch, then the scan that probes them (LDS: bases + codons)
		if ((rc = gmap_build(B, s, gp, gr.qg_first, gr.gword, (const int32_t*)(dm + o_lq), (const int64_t*)(dm + o_gd)))) return rc;
		hipLaunchKernelGGL(k_refine_scan_gmap, dim3((unsigned)(cls_end[3] - cls_end[2])), dim3(256), 2 * (REFINE_CHUNK + 2 * REFINE_HALO), s, dg, (const RefineWindowDev*)(dm + o_win),
		                   (const RefineChunk*)(dm + o_chunk) + cls_end[2], gr, d_wg, rt, kmer, min_aa_len, B.r_hits.as<uint4>(), B.r_count.as<unsigned long long>(), cap, d_wcnt, (int32_t)n_super,
		                   RefineGmap{ B.r_gmap.as<uint2>(), (const int64_t*)(dm + o_gd) });
		if (timing_on()) fprintf(stderr, "[mpa-timing]     refine: global-map class (%zu queries, %lld windows)\n", n_long, (long long)n_long_win);
	}
	HIP_TRY(hipGetLastError());
	unsigned long long *h_n = B.h_back.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(h_n, B.r_count.p, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t n_hits = (int64_t)*h_n;
	if ((unsigned long long)n_hits > cap) { set_error("device refinement: more hits than the buffer holds"); return MPA_ERR_UNSUPPORTED; }
	timing_note("    refine: scan (wait)", now_ms() - t0);
	if (n_hits == 0) return MPA_OK;
	// ---- pairs: count, offsets, emit, sort, decode
	const double t1 = now_ms();
	if ((rc = B.r_chunk.ensure((size_t)n_hits * 4 + 16)) || (rc = B.r_words.ensure((size_t)n_hits * 8 + 16))) return rc;   // pairs per hit, and where they go
	uint32_t *d_pc = B.r_chunk.as<uint32_t>();
	uint64_t *d_po = B.r_words.as<uint64_t>();
	const unsigned nbh = (unsigned)((n_hits + 255) / 256);
	hipLaunchKernelGGL(k_refine_pair_count, dim3(nbh), dim3(256), 0, s, B.r_hits.as<uint4>(), n_hits, d_wg, d_wcnt, gr.gcount, max_ava, d_pc, d_wpairs);
	HIP_TRY(hipGetLastError());
	{
		size_t tb = 0, tb2 = 0;
		auto in = rocprim::make_transform_iterator((const uint32_t*)d_pc, U32ToU64());
		auto inw = rocprim::make_transform_iterator((const uint32_t*)d_wpairs, U32ToU64());
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, d_po, (uint64_t)0, (size_t)n_hits, rocprim::plus<uint64_t>(), s));
		HIP_TRY(rocprim::exclusive_scan(nullptr, tb2, inw, (uint64_t*)d_first, (uint64_t)0, NW + 1, rocprim::plus<uint64_t>(), s));
		if ((rc = B.tmp.ensure(std::max(tb, tb2) + 256))) return rc;
		HIP_TRY(rocprim::exclusive_scan(B.tmp.p, tb, in, d_po, (uint64_t)0, (size_t)n_hits, rocprim::plus<uint64_t>(), s));
		HIP_TRY(rocprim::exclusive_scan(B.tmp.p, tb2, inw, (uint64_t*)d_first, (uint64_t)0, NW + 1, rocprim::plus<uint64_t>(), s));
	}
	int64_t *h_np = (int64_t*)(h_n + 1);
	HIP_TRY(hipMemcpyAsync(h_np, d_first + n_win, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	const int64_t np = *h_np;
	if (np == 0) return MPA_OK;
	if ((rc = B.rx_keys.ensure((size_t)np * 24 + 64))) return rc;
	uint64_t *keys0 = B.rx_keys.as<uint64_t>(), *keys1 = keys0 + np, *d_a = keys1 + np;
	hipLaunchKernelGGL(k_refine_pair_emit, dim3(nbh), dim3(256), 0, s, B.r_hits.as<uint4>(), n_hits, (const uint32_t*)d_pc, (const uint64_t*)d_po, gr, keys0);
	HIP_TRY(hipGetLastError());
	{
		int wbits = 1;
		while ((1LL << wbits) < n_win) ++wbits;
		size_t tb = 0;
		HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, keys0, keys1, (size_t)np, 0u, (unsigned)(44 + wbits), s));
		if ((rc = B.tmp.ensure(tb + 256))) return rc;
		HIP_TRY(rocprim::radix_sort_keys(B.tmp.p, tb, keys0, keys1, (size_t)np, 0u, (unsigned)(44 + wbits), s));
	}
	const unsigned nbp = (unsigned)((np + 255) / 256);
	hipLaunchKernelGGL(k_refine_pair_decode, dim3(nbp), dim3(256), 0, s, (const uint64_t*)keys1, np, d_a);
	HIP_TRY(hipGetLastError());
	// ---- the chains of every window: forward pass (base resolution), extraction, pack
	PreParams pm;
	pm.max_dist_x = std::max(cp.max_dist_x, cp.bw), pm.max_dist_y = cp.max_dist_y;
	if (pm.max_dist_y < cp.bw && !cp.is_spliced) pm.max_dist_y = cp.bw;
	pm.bw = cp.bw, pm.max_skip = cp.max_skip, pm.max_iter = cp.max_iter, pm.kmer = cp.kmer, pm.bbit = cp.bbit;
	pm.is_spliced = cp.is_spliced, pm.coef_log = cp.coef_log, pm.max_dblock = pm.max_dist_x >> cp.bbit;
	const size_t M = (size_t)np;
	size_t xat = 0;
	auto xcarve = [&](size_t bytes) { const size_t o = xat; xat += (bytes + 255) & ~(size_t)255; return o; };
	const size_t x_mark = xcarve(M * 4), x_order = xcarve(M * 4), x_ends = xcarve((M + 64 * NW + 64) * sizeof(Pair64)), x_tail8 = xcarve(M * sizeof(Pair64)),
	             x_items = xcarve(M * sizeof(SparseItem)), x_moved = xcarve(M * sizeof(SparseItem)), x_merged = xcarve(M * sizeof(SparseItem)), x_kept = xcarve(M), x_stack = xcarve((M / 64 + 6 * NW + 16) * sizeof(SortRange)), x_status = xcarve(NW * 4 + 16), x_f = xcarve(M * 4), x_pred = xcarve(M * 4),
	             x_fm = xcarve(M * 4), x_outa = xcarve(M * 8), x_outu = xcarve(M * 8), x_na = xcarve(NW * 8 + 8), x_nu = xcarve(NW * 8 + 8), x_offa = xcarve(NW * 8 + 16), x_offu = xcarve(NW * 8 + 16);
	const int32_t kSerialRun = 48;
	const size_t long_cap = M / (size_t)(kSerialRun + 1) + 16, x_long = xcarve(long_cap * sizeof(LongRun)), x_nlong = xcarve(64);
	if ((rc = B.x_all.ensure(xat))) return rc;
	char *X = B.x_all.as<char>();
	HIP_TRY(hipMemsetAsync(X + x_status, 0, NW * 4 + 16, s));
	HIP_TRY(hipMemsetAsync(X + x_nlong, 0, 64, s));
	hipLaunchKernelGGL(k_seed_fill, dim3(nbp), dim3(256), 0, s, np, pm.kmer, (int32_t*)(X + x_f), (int32_t*)(X + x_pred), (int32_t*)(X + x_fm), (uint32_t*)(X + x_mark));
	hipLaunchKernelGGL(k_chain_fwd, dim3(nbp), dim3(256), 0, s, (const uint64_t*)d_a, np, (const int64_t*)d_first, (const int64_t*)nullptr, (int32_t)n_win, pm, (int32_t*)(X + x_f), (int32_t*)(X + x_pred),
	                   (int32_t*)(X + x_fm), kSerialRun, (LongRun*)(X + x_long), (unsigned int*)(X + x_nlong), (unsigned int)long_cap);
	hipLaunchKernelGGL(k_chain_fwd_wave, dim3((unsigned)std::min<size_t>(long_cap, 65536)), dim3(64), 0, s, (const uint64_t*)d_a, (const LongRun*)(X + x_long), (const unsigned int*)(X + x_nlong),
	                   (unsigned int)long_cap, pm, (int32_t*)(X + x_f), (int32_t*)(X + x_pred), (int32_t*)(X + x_fm));
	HIP_TRY(hipGetLastError());
	ExtractArgs xa;
	xa.first = d_first, xa.cnt = nullptr, xa.ntot_first = nullptr;
	xa.v_pos = nullptr, xa.v_f = (const int32_t*)(X + x_f), xa.v_pred = (const int32_t*)(X + x_pred), xa.v_a = (const uint64_t*)d_a;
	xa.mark = (int32_t*)(X + x_mark), xa.order = (int32_t*)(X + x_order), xa.ends = (Pair64*)(X + x_ends), xa.tail8 = (Pair64*)(X + x_tail8);
	xa.items = (SparseItem*)(X + x_items), xa.moved = (SparseItem*)(X + x_moved), xa.merged = (SparseItem*)(X + x_merged);
	xa.kept = (uint8_t*)(X + x_kept), xa.stack = (SortRange*)(X + x_stack);
	xa.a_out = (uint64_t*)(X + x_outa), xa.u_out = (uint64_t*)(X + x_outu), xa.n_a = (int64_t*)(X + x_na), xa.n_u = (int64_t*)(X + x_nu);
	xa.status = (int32_t*)(X + x_status), xa.p = cp, xa.set_only = 0;
	hipLaunchKernelGGL(k_chain_extract, dim3((unsigned)n_win), dim3(64), EXTRACT_LDS_BYTES, s, xa, (int32_t)n_win);
	hipLaunchKernelGGL(k_offsets2, dim3(1), dim3(256), 0, s, (const int64_t*)(X + x_na), (const int64_t*)(X + x_nu), (int32_t)n_win, (int64_t*)(X + x_offa), (int64_t*)(X + x_offu));
	HIP_TRY(hipGetLastError());
	const size_t offb = (NW + 1) * 8;
	if ((rc = B.h_xoff.ensure(2 * offb + NW * 4 + 64))) return rc;
	int64_t *h_offa = B.h_xoff.as<int64_t>(), *h_offu = h_offa + (NW + 1);
	int32_t *h_status = (int32_t*)(h_offu + (NW + 1));
	HIP_TRY(hipMemcpyAsync(h_offa, X + x_offa, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_offu, X + x_offu, offb, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h_status, X + x_status, NW * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	for (size_t w = 0; w < NW; ++w) if (h_status[w]) { set_error("device refinement: a chain extraction needs the host"); return MPA_ERR_UNSUPPORTED; }   // (dense views never do)
	const int64_t tot_a = h_offa[n_win], tot_u = h_offu[n_win];
	SeedHold &H = B.own;
	if ((rc = H.h_A.ensure((size_t)tot_a * 8 + 64)) || (rc = H.h_U.ensure((size_t)tot_u * 8 + 64))) return rc;
	if (tot_a > 0 || tot_u > 0) {
		hipLaunchKernelGGL(k_chain_pack, dim3((unsigned)n_win), dim3(256), 0, s, (const int64_t*)d_first, (const int64_t*)(X + x_na), (const int64_t*)(X + x_nu), (const int64_t*)(X + x_offa),
		                   (const int64_t*)(X + x_offu), (const uint64_t*)(X + x_outa), (const uint64_t*)(X + x_outu), H.h_A.as<uint64_t>(), H.h_U.as<uint64_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(wait_stream(ctx, s));
	}
	out.a_first.assign(h_offa, h_offa + n_win + 1), out.u_first.assign(h_offu, h_offu + n_win + 1);
	out.A = H.h_A.as<uint64_t>(), out.U = H.h_U.as<uint64_t>();
	timing_note("    refine: pairs + chains (wait)", now_ms() - t1);
	return MPA_OK;
}
} // namespace mpa

namespace mpa {
// ---- DP worker pool: host side (the kernels and the protocol are in dp_kernels.hip, "The DP worker pool")
// MPA_DP_POOL=1 selects the pool; the default is one k_dp_round launch per round.  Measured (profiles/r05_experiments.txt): with
// identical sweep code the pool is level with the launches on the DP-bound config 5 (1.05-1.14 M against 1.09 M residues/s), 5-10 %
// behind on config 3 (19.4-19.8 M against 20.0-21.9 M) and a third behind on config 2 (17-ms batches: arming, the second host
// round trip and the L2 write-back weigh).  The hardware's workgroup dispatcher already IS a work-conserving queue across the
// launches in flight -- a slot that a finished unit frees goes to the oldest pending workgroup of ANY launch -- so what the pool
// adds (units taken wave by wave, a bounded DP population) buys no throughput here, and its round latency is longer because the
// rounds in flight share the workers instead of being served in order of arrival.
static bool dp_pool_enabled()
{
	static const bool on = [] { const char *e = getenv("MPA_DP_POOL"); return e && atoi(e) != 0; }();
	return on;
}
// resident worker workgroups the pool admits (MPA_DP_WORKERS).  The workers ask for a fifth of a CU's LDS plus a little, so four
// fit per CU (1 024 on the chip); the default keeps three per CU busy and leaves the fourth slot to the workgroups that arrive,
// find the pool full and leave -- and registers and LDS to the seeding kernels of the batches behind.
static int dp_pool_budget()
{
	static const int b = [] { const char *e = getenv("MPA_DP_WORKERS"); const int v = e ? atoi(e) : 768; return v < 1 ? 1 : v; }();
	return b;
}
// MPA_DP_TRACE=<file>: every unit of every round appends "slot generation unit kind priority start end" (100-MHz device ticks);
// tools/dp_trace.py turns that into resident units over time
static const char *dp_trace_path()
{
	static const char *p = [] { const char *e = getenv("MPA_DP_TRACE"); return e && *e ? e : (const char*)nullptr; }();
	return p;
}
// the calling context's slot, done word and worker stream (created on its first round); the device's pool on the first of all
static int pool_attach(mpa_ctx_t *ctx)
{
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	std::lock_guard<std::mutex> g(root->pool_mu);
	if (!root->dp_pool) {
		DpPool *p = nullptr;
		HIP_TRY(hipMalloc((void**)&p, sizeof(DpPool)));
		HIP_TRY(hipMemset(p, 0, sizeof(DpPool)));
		const int32_t budget = dp_pool_budget();
		HIP_TRY(hipMemcpy(&p->ctl.budget, &budget, 4, hipMemcpyHostToDevice));
		const int32_t acq = [] { const char *e = getenv("MPA_DP_ACQUIRE"); return e ? atoi(e) : 2; }();
		HIP_TRY(hipMemcpy(&p->ctl.acquire_mode, &acq, 4, hipMemcpyHostToDevice));
		HIP_TRY(hipEventCreate(&root->pool_base));
		HIP_TRY(hipEventRecord(root->pool_base, root->stream));
		root->dp_pool = p;
	}
	if (ctx->dp_slot < 0) {
		if (root->pool_slots >= MPA_DP_SLOTS) { set_error("more than " + std::to_string(MPA_DP_SLOTS) + " contexts of one device run DP rounds"); return MPA_ERR_UNSUPPORTED; }
		HIP_TRY(hipHostMalloc((void**)&ctx->dp_done, 64, hipHostMallocDefault));
		*(volatile int32_t*)ctx->dp_done = 0;
		HIP_TRY(hipStreamCreateWithFlags(&ctx->worker_stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&ctx->arm_ev, hipEventDisableTiming));
		ctx->dp_slot = root->pool_slots++;
	}
	return MPA_OK;
}
// durations of the context's worker launches that have ended (wait: of all of them -- only when no round is pending anywhere, the
// workers then leave within microseconds) into the context's totals and the device's interval list
void pool_harvest(mpa_ctx_t *ctx, bool wait)
{
	if (ctx->wl_busy.empty()) return;
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	(void)hipSetDevice(ctx->device);
	if (wait) (void)wait_stream(ctx, ctx->worker_stream);
	size_t keep = 0;
	for (size_t k = 0; k < ctx->wl_busy.size(); ++k) {
		mpa_ctx_s::WorkerLaunch w = ctx->wl_busy[k];
		float a = 0, b = 0;
		if (hipEventQuery(w.e1) == hipSuccess && hipEventElapsedTime(&a, root->pool_base, w.e0) == hipSuccess && hipEventElapsedTime(&b, root->pool_base, w.e1) == hipSuccess) {
			ctx->total.ms_round += (double)(b - a), ctx->total.launches_round++;
			{ std::lock_guard<std::mutex> g(root->pool_mu); root->pool_iv.emplace_back(a, b); }
			ctx->wl_free.push_back(w);
		} else ctx->wl_busy[keep++] = w;
	}
	(void)hipGetLastError();
	ctx->wl_busy.resize(keep);
}
// A round for the pool: the round's arguments (ha: pinned) and units into the lane's slot of the device's pool, the slot armed in
// stream order behind everything the round reads, the lane's workers launched (a worker takes any lane's units: their stream is
// never waited for by a round -- a round is complete when its last unit says so in pinned memory).  The unit list is in
// ctx->units already: whole-workgroup units [0, n_group), then the one-wave units.  *gen: what pool_wait_round waits for.
static int pool_launch_round(mpa_ctx_t *ctx, hipStream_t s, const ExtArgs &ea, const ExtWideArgs &wa, const GlobArgs &ga, DpRoundArgs *ha,
                             size_t n_units, size_t n_group, size_t round_lds, unsigned int *gen)
{
	int rc;
	if ((rc = pool_attach(ctx))) return rc;
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	DpPool *pool = root->dp_pool;
	int n_slots;
	{ std::lock_guard<std::mutex> g(root->pool_mu); n_slots = root->pool_slots; }
	ha->ea = ea, ha->wa = wa, ha->ga = ga, ha->units = ctx->units.as<DpUnit>(), ha->n_group = (int32_t)n_group, ha->pad_ = 0;
	HIP_TRY(hipMemcpyAsync(&pool->args[ctx->dp_slot], ha, sizeof(DpRoundArgs), hipMemcpyHostToDevice, s));
	long long *d_trace = nullptr;
	if (dp_trace_path()) {
		if ((rc = ctx->dp_trace.ensure(n_units * 16))) return rc;
		HIP_TRY(hipMemsetAsync(ctx->dp_trace.p, 0, n_units * 16, s));
		d_trace = ctx->dp_trace.as<long long>();
	}
	*gen = ++ctx->dp_gen;
	hipLaunchKernelGGL(k_dp_arm, dim3(1), dim3(1), 0, s, pool, ctx->dp_slot, (int)n_group, (int)(n_units - n_group), *gen, ctx->dp_done, d_trace);
	HIP_TRY(hipGetLastError());
	// The workers go out on the lane's own stream (what follows the round on that stream then also waits for this launch's
	// workers to run out of units of ANY lane; measured level with a stream of their own, 19.6 against 19.7 M residues/s).
	// MPA_DP_WORKER_STREAM=1: a worker stream per lane -- one more stream per lane for HIP to deal hardware queues to, and
	// when that stream lands on a queue another context's long kernels use, every round waits for them (the evidence run of
	// round 5 measured 6.5 M residues/s that way: profiles/r05_experiments.txt).
	static const bool own_stream = [] { const char *e = getenv("MPA_DP_WORKER_STREAM"); return e && atoi(e) != 0; }();
	hipStream_t ws = own_stream ? ctx->worker_stream : s;
	if (own_stream) {
		HIP_TRY(hipEventRecord(ctx->arm_ev, s));
		HIP_TRY(hipStreamWaitEvent(ws, ctx->arm_ev, 0));
	}
	mpa_ctx_s::WorkerLaunch wl;
	if (!ctx->wl_free.empty()) wl = ctx->wl_free.back(), ctx->wl_free.pop_back();
	else { HIP_TRY(hipEventCreate(&wl.e0)); HIP_TRY(hipEventCreate(&wl.e1)); }
	HIP_TRY(ensure_dynamic_lds((const void*)k_dp_worker, ctx->device, round_lds));
	static const int launch_cap = [] { const char *e = getenv("MPA_DP_LAUNCH_WORKERS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : dp_pool_budget(); }();
	// a workgroup serves one workgroup unit at a time, or four one-wave units side by side
	const unsigned grid = (unsigned)std::min<size_t>(n_group + (n_units - n_group + 3) / 4, (size_t)launch_cap);
	HIP_TRY(hipEventRecord(wl.e0, ws));
	hipLaunchKernelGGL(k_dp_worker, dim3(grid), dim3(256), round_lds, ws, pool, ctx->dp_slot, n_slots);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(wl.e1, ws));
	ctx->wl_busy.push_back(wl);
	return MPA_OK;
}
// the round is complete when the last of its units has stored the round's generation into the lane's pinned word
static int pool_wait_round(mpa_ctx_t *ctx, hipStream_t s, unsigned int gen, const DpUnit *units, size_t n_units)
{
	volatile int32_t *d = ctx->dp_done;
	const double t0 = now_ms();
	for (int polls = 0; (unsigned int)*d != gen; ++polls) {
		if (polls >= 8) { struct timespec ts = { 0, 100000L }; nanosleep(&ts, nullptr); }
		if ((polls & 1023) == 1023) {
			if (now_ms() - t0 > 120000.0) { set_error("DP worker pool: a round did not complete within two minutes"); return MPA_ERR_HIP; }
			const hipError_t e = hipStreamQuery(s);                            // (a fault in a worker kernel shows up here, not in the word)
			if (e != hipSuccess && e != hipErrorNotReady) { set_error(std::string("DP worker launch: ") + hipGetErrorString(e)); return MPA_ERR_HIP; }
		}
	}
	hipLaunchKernelGGL(k_l2_writeback, dim3(128), dim3(64), 0, s);       // the units' results out of the L2s, before anything enqueued behind reads them
	HIP_TRY(hipGetLastError());
	if (const char *path = dp_trace_path()) {                             // (debug) one line per unit: who ran when
		std::vector<long long> tr(2 * n_units);
		HIP_TRY(hipMemcpy(tr.data(), ctx->dp_trace.p, n_units * 16, hipMemcpyDeviceToHost));
		static std::mutex tmu;
		std::lock_guard<std::mutex> g(tmu);
		if (FILE *f = fopen(path, "a")) {
			for (size_t k = 0; k < n_units; ++k)
				fprintf(f, "%d\t%u\t%zu\t%d\t%d\t%lld\t%lld\n", ctx->dp_slot, gen, k, units[k].kind, units[k].prio, tr[2 * k], tr[2 * k + 1]);
			fclose(f);
		}
	}
	return MPA_OK;
}
// time during which at least one worker launch of the device was running
static double pool_union_ms(mpa_ctx_s *root, bool reset)
{
	std::lock_guard<std::mutex> g(root->pool_mu);
	std::vector<std::pair<float, float>> iv = root->pool_iv;
	if (reset) root->pool_iv.clear();
	std::sort(iv.begin(), iv.end());
	double sum = 0, lo = 0, hi = -1;
	for (auto &x : iv) {
		if (hi < 0) { lo = x.first, hi = x.second; continue; }
		if (x.first <= hi) { hi = std::max<double>(hi, x.second); continue; }
		sum += hi - lo, lo = x.first, hi = x.second;
	}
	if (hi >= 0) sum += hi - lo;
	return sum;
}
} // namespace mpa

extern "C" {

void mpa_dp_last_stats(const mpa_ctx_t *ctx, mpa_dp_stats_t *st) { *st = ctx->stats; }
void mpa_dp_total_stats(mpa_ctx_t *ctx, mpa_dp_stats_t *st, int reset)
{
	pool_harvest(ctx, true);
	mpa_ctx_s *root = ctx->root ? ctx->root : ctx;
	const double u = pool_union_ms(root, reset != 0);
	if (st) *st = ctx->total, st->ms_round_union = u;
	if (reset) ctx->total = mpa_dp_stats_t();
}

#define MPA_RETRY_NO_SPLIT (-100)   /* internal: repeat the round without split extension calls */

// What the phases of one mpa_dp_run() call share: the plan, the staging blocks, the kernels' argument structs, which side streams
// carry what, and the event times collected so far.
struct DpRun {
	mpa_ctx_t *ctx;
	hipStream_t s;
	DpPlan &plan;
	DpPlanKnobs kn;
	char *hup = nullptr, *hdn = nullptr;        // pinned staging: host -> device (plan.up), device -> host (plan.dn)
	DpConst dc;
	ExtArgs ea;
	ExtWideArgs wa;
	GlobArgs ga;
	GlobWave *d_hw = nullptr;                   // the huge calls' waves and list, behind their keys
	int32_t *d_hlist = nullptr;
	struct Launch { int side; bool is_ext; };
	std::vector<Launch> launches;               // side-stream launches so far (side = index of the stream and of its event pair)
	int l12_side = -1;                          // ... the one of the T_LITE_W4 sweep
	bool round_launched = false;
	bool pool_pending = false;                  // (worker pool) a round is armed and not yet known to be complete ...
	unsigned int pool_gen = 0;                  // ... its generation
	int64_t pool_n = 0;                         // words of the dense CIGAR pool
	float ms_glob = 0, ms_bt = 0;
	bool glob_timed = false;                    // ev[3..5] hold a chunk's sweep and walk not yet added to ms_glob / ms_bt
	double t_mark = 0;
	void mark(const char *what) { const double t = now_ms(); timing_note(what, t - t_mark); t_mark = t; }   // (MPA_TIMING: wall clock between marks)
	hipEvent_t ev_round(int k) const { return ctx->lev[2 * (mpa_ctx_s::kSide - 1) + k]; }                    // the last event pair times the round's launch
	hipStream_t side_stream(int k) const { hipStream_t st = ctx->side[(k + ctx->side_off) % mpa_ctx_s::kSide]; return st ? st : s; }
	void add_chunk_times() { float a = 0, b = 0; (void)hipEventElapsedTime(&a, ctx->ev[3], ctx->ev[4]); (void)hipEventElapsedTime(&b, ctx->ev[4], ctx->ev[5]); ms_glob += a, ms_bt += b; }
};

// fork: the next side stream (created when first used), waiting for fork_ev, its start event recorded
static hipStream_t begin_side(DpRun &R, bool is_ext)
{
	mpa_ctx_t *ctx = R.ctx;
	const int k = (int)R.launches.size();
	// (side streams are created when first used: HIP deals hardware queues to streams in creation order, and sixteen idle side
	// streams per context pushed the main streams of later contexts onto queues that other contexts' long kernels were using)
	hipStream_t &slot = ctx->side[(k + ctx->side_off) % mpa_ctx_s::kSide];
	if (!slot && hipStreamCreateWithFlags(&slot, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); slot = nullptr; }
	hipStream_t st = R.side_stream(k);
	(void)hipStreamWaitEvent(st, ctx->fork_ev, 0);
	(void)hipEventRecord(ctx->lev[2 * k], st);
	R.launches.push_back(DpRun::Launch{ k, is_ext });
	return st;
}
static void end_side(DpRun &R) { const int k = R.launches.back().side; (void)hipEventRecord(R.ctx->lev[2 * k + 1], R.side_stream(k)); }

// ---- 2. pools and staging at the sizes the plan asks for
static int dp_size_pools(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	const DpPlan::Pools &z = R.plan.sz;
	int rc;
	if ((rc = ctx->tasks.ensure(z.tasks)) || (rc = ctx->chunks.ensure(z.chunks)) || (rc = ctx->qseq.ensure(z.qseq)) || (rc = ctx->rec.ensure(z.rec)) || (rc = ctx->prof.ensure(z.prof)) ||
	    (rc = ctx->waves.ensure(z.waves)) || (rc = ctx->extout.ensure(z.extout)) || (rc = ctx->tb.ensure(z.tb)) || (rc = ctx->cig.ensure(z.cig)) || (rc = ctx->ncig.ensure(z.ncig)) ||
	    (rc = ctx->lite.ensure(z.lite)) || (rc = ctx->ckpt.ensure(z.ckpt)) || (rc = ctx->wlist.ensure(z.wlist)) || (rc = ctx->score.ensure(z.score)) || (rc = ctx->rowkey.ensure(z.rowkey)) ||
	    (rc = ctx->bnd.ensure(z.bnd)) || (rc = ctx->hkey.ensure(z.hkey)) || (rc = ctx->list.ensure(z.list)))
		return rc;
	// Everything the device needs from the host goes through ONE pinned staging buffer (plan.up), so that no copy is
	// staged by the runtime and the host never waits for one: a DP round is enqueued in one go and waited for once.
	if ((rc = ctx->h_up.ensure(R.plan.up.end + 256))) return rc;
	R.hup = ctx->h_up.as<char>();
	return MPA_OK;
}

// ---- 3. staging filled; uploads, memsets and the prep kernels enqueued
static int dp_upload_and_prep(DpRun &R, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	char *hup = R.hup;
	const size_t b_tasks = sizeof(DTask) * P.tasks.size(), b_chunks = sizeof(PrepChunk) * P.prep.size(), b_waves = sizeof(ExtWave) * P.ewaves.size();
	memcpy(hup + P.up.tasks, P.tasks.data(), b_tasks);
	memcpy(hup + P.up.chunks, P.prep.data(), b_chunks);
	memcpy(hup + P.up.q, q->seqs + q->q_off[0], (size_t)P.q_bytes);
	memcpy(hup + P.up.waves, P.ewaves.data(), b_waves);
	R.mark("    dp: buffers");
	HIP_TRY(hipMemcpyAsync(ctx->tasks.p, hup + P.up.tasks, b_tasks, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(ctx->chunks.p, hup + P.up.chunks, b_chunks, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(ctx->qseq.p, hup + P.up.q, P.q_bytes, hipMemcpyHostToDevice, s));
	if (!P.ewaves.empty()) HIP_TRY(hipMemcpyAsync(ctx->waves.p, hup + P.up.waves, b_waves, hipMemcpyHostToDevice, s));
	// (k_prep_rows writes every row of every call; only the padding the kernels prefetch behind the last call is cleared)
	HIP_TRY(hipMemsetAsync((char*)ctx->rec.p + (size_t)(P.rec_total - P.rec_pad) * 4, 0, (size_t)P.rec_pad * 4, s));
	if (P.n_wide_groups) HIP_TRY(hipMemsetAsync(ctx->rowkey.p, 0, (size_t)(P.n_wide_groups * 2 * P.key_stride * 4), s));
	// split classes: boundary granules, then the per-group completion counters and the error flag; all zero before the launch (a granule's tag is row + 1)
	if (P.n_split) {
		int rc;
		if ((rc = ctx->xg.ensure(P.sz.xg))) return rc;
		HIP_TRY(hipMemsetAsync(ctx->xg.p, 0, P.xg_bytes + P.xg_tail, s));
	}
	// extension calls wider than 1024 columns: keys (zeroed), then one GlobWave and one list entry per call
	if (!P.huge_ids.empty()) {
		const size_t n_huge = P.huge_ids.size();
		HIP_TRY(hipMemsetAsync(ctx->hkey.p, 0, (size_t)P.hkey_total * 8, s));
		R.d_hw = (GlobWave*)((char*)ctx->hkey.p + (((size_t)P.hkey_total * 8 + 15) & ~(size_t)15));
		R.d_hlist = (int32_t*)(R.d_hw + n_huge);
		HIP_TRY(hipMemcpyAsync(R.d_hw, P.huge_waves.data(), sizeof(GlobWave) * n_huge, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(R.d_hlist, P.huge_ids.data(), 4 * n_huge, hipMemcpyHostToDevice, s));
		HIP_TRY(wait_stream(ctx, s));                  // (pageable sources; the calls are rare)
	}

	DevTables tabs;
	memcpy(tabs.aa20, tab_aa20(), 256);
	memcpy(tabs.codon, tab_codon(), 64);
	memcpy(tabs.mat, opt->mat, 484);
	DpConst &dc = R.dc;
	dc.go = opt->go, dc.ge = opt->ge, dc.fs = opt->fs, dc.xdrop = opt->xdrop, dc.end_bonus = opt->end_bonus;
	for (int k = 0; k < 6; ++k) dc.sp[k] = opt->sp[k];
	dc.sp_null_bonus = opt->sp_null_bonus;
	dc.wide_ge = P.wide_ge ? 1 : 0;
	DevGenome dg{ mi->dev[ctx->device]->seq, mi->dev[ctx->device]->ctg_off, mi->dev[ctx->device]->ctg_len, mi->dev[ctx->device]->spsc, mi->l_seq };

	// per-row records and profiles
	// (measured, round 4: putting these two on a high-priority stream of their own gives every DP lane a second active hardware
	// queue, and with ten more queues in use the round kernels are time-sliced: 41 -> 72 ms per launch.  They stay in the lane's
	// own queue; MPA_SHORT_KERNEL raises their wave priority instead.)
	HIP_TRY(hipEventRecord(ctx->ev[0], s));
	if (!P.prep.empty())
		hipLaunchKernelGGL(k_prep_rows, dim3((unsigned)P.prep.size()), dim3(256), 0, s, dg, ctx->tasks.as<DTask>(), ctx->chunks.as<PrepChunk>(), ctx->rec.as<uint32_t>(), dc, tabs);
	hipLaunchKernelGGL(k_prep_prof, dim3((unsigned)P.tasks.size()), dim3(256), 0, s, ctx->tasks.as<DTask>(), ctx->qseq.as<char>(), ctx->prof.as<int16_t>(), tabs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(ctx->ev[1], s));
	R.mark("    dp: uploads + prep enqueued");

	// the kernels' arguments
	ExtArgs &ea = R.ea;
	ea.tasks = ctx->tasks.as<DTask>(), ea.rec = ctx->rec.as<uint32_t>(), ea.prof = ctx->prof.as<int16_t>(), ea.out = ctx->extout.as<ExtOut>();
	ea.c = dc, ea.pen = P.pen;
	ea.lite = ctx->lite.as<uint32_t>(), ea.ckpt = ctx->ckpt.as<uint32_t>(), ea.score = ctx->score.as<int32_t>();
	ea.waves = ctx->waves.as<ExtWave>();
	ExtWideArgs &wa = R.wa;
	wa.tasks = ea.tasks, wa.rec = ea.rec, wa.prof = ea.prof, wa.out = ea.out, wa.c = dc, wa.pen = P.pen, wa.key_stride = P.key_stride;
	wa.xg = P.n_split ? ctx->xg.as<unsigned long long>() : nullptr;
	wa.done = P.n_split ? (int32_t*)((char*)ctx->xg.p + P.xg_bytes) : nullptr;
	wa.ticket = P.n_split ? wa.done + P.n_split : nullptr;
	wa.err = P.n_split ? wa.ticket + P.n_split : nullptr;
	wa.waves = ctx->waves.as<ExtWave>();                // absolute descriptor indices: the rowkey slot of group g is g - first wide group
	wa.rowkey = ctx->rowkey.as<uint32_t>() - (int64_t)P.ext[X_W2].first * 2 * P.key_stride;
	GlobArgs &ga = R.ga;
	ga.tasks = ctx->tasks.as<DTask>(), ga.rec = ctx->rec.as<uint32_t>(), ga.prof = ctx->prof.as<int16_t>();
	ga.tb = ctx->tb.as<uint16_t>(), ga.bnd = ctx->bnd.as<int4>(), ga.score = ctx->score.as<int32_t>(), ga.c = dc, ga.rowkey64 = nullptr, ga.waves = nullptr;
	return MPA_OK;
}

// ---- 4. what runs next to the round on side streams: the anti-diagonal prototype, the huge calls, the T_LITE_W4 sweep
static int dp_side_launches(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	// fork: every side launch waits for the prep kernels, so the long single-wave tails overlap instead of adding up
	HIP_TRY(hipEventRecord(ctx->fork_ev, R.s));
	if (ctx->antidiag && P.ext[X_32].cnt > 0) {                        // (measurement) the 32-column class on the anti-diagonal prototype, one wave per block
		hipStream_t st = begin_side(R, true);
		hipLaunchKernelGGL(k_ext_antidiag, dim3((unsigned)P.ext[X_32].cnt), dim3(64), EXT_ANTIDIAG_LDS, st, R.ea, P.ext[X_32].first);
		HIP_TRY(hipGetLastError());
		end_side(R);
		ctx->stats.launches_ext++;
	}
	if (!P.huge_ids.empty()) {                                         // block-major sweep with the traceback kernel's arithmetic, then the replay
		const unsigned n_huge = (unsigned)P.huge_ids.size();
		GlobArgs ha;
		ha.tasks = ctx->tasks.as<DTask>(), ha.waves = R.d_hw, ha.rec = ctx->rec.as<uint32_t>(), ha.prof = ctx->prof.as<int16_t>();
		ha.tb = nullptr, ha.bnd = ctx->bnd.as<int4>(), ha.score = nullptr, ha.c = R.dc, ha.rowkey64 = ctx->hkey.as<unsigned long long>();
		hipStream_t st = begin_side(R, true);
		if (P.wide_ge) hipLaunchKernelGGL(k_ext_huge<true>, dim3(n_huge), dim3(64), (size_t)22 * 64 * 2 + 4 * 32 * 4, st, ha);
		else hipLaunchKernelGGL(k_ext_huge<false>, dim3(n_huge), dim3(64), (size_t)22 * 64 * 2 + 4 * 32 * 4, st, ha);
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_ext_replay, dim3(n_huge), dim3(64), 0, st, ctx->tasks.as<DTask>(), R.d_hlist, (int32_t)n_huge,
		                   ctx->hkey.as<unsigned long long>(), ctx->extout.as<ExtOut>(), R.dc, P.pen);
		HIP_TRY(hipGetLastError());
		end_side(R);
		ctx->stats.launches_ext++;
	}
	// the packed sweep of the 129..256-column checkpointed class (unit kind U_LITE_W4): a 256-thread launch of its own next to the
	// round, on a side stream (at most two are taken at this point, by the launches above); the walk waits for it
	if (P.lite_w4.cnt > 0) {
		hipStream_t st = begin_side(R, false);
		hipLaunchKernelGGL(k_lite_wide, dim3((unsigned)P.lite_w4.cnt), dim3(MPA_LITE_WIDE_WAVES * 64), 0, st, R.ea, P.lite_w4.first);
		HIP_TRY(hipGetLastError());
		end_side(R), R.l12_side = R.launches.back().side;
		ctx->stats.launches_glob++;
	}
	return MPA_OK;
}

// Workgroups of the round kernel per CU, enforced through the LDS it asks for (MPA_DP_WG_PER_CU, default 3).  Round 6: the
// kernel takes 124 VGPRs (the asm rows of ext_narrow keep the whole DP state of eight calls in registers and nothing is
// spilled), so three workgroups hold 372 of each SIMD's 512 registers -- what four workgroups of the 95-register kernel of
// rounds 4-5 held (384) -- and the seeding kernels of the next batches stay co-resident.  One more workgroup than wanted must
// NOT fit; what is left of the LDS stays free for the seeding kernels.
static size_t dp_round_lds()
{
	static const size_t round_lds = [] {
		const char *e = getenv("MPA_DP_WG_PER_CU");
		int want = e ? atoi(e) : 3;
		if (want < 1) want = 1;
		if (want > 4) want = 4;
		const size_t pad = (((size_t)160 * 1024 / (want + 1)) + 256) & ~(size_t)255;
		return pad > DP_ROUND_LDS ? pad : DP_ROUND_LDS;
	}();
	return round_lds;
}

// every DP unit of the round (dp_plan_units, built straight into the staging block) in ONE k_dp_round launch on the context's main stream -- or handed to the worker pool;
// d_gw: the first traceback chunk's waves when they ride in the round
static int dp_launch_round(DpRun &R, GlobWave *d_gw)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	DpUnit *units = (DpUnit*)(R.hup + P.up.units);          // (pinned: the copy below needs no wait)
	int rc;
	if ((rc = dp_plan_units(P, R.kn, units))) { set_error(P.err); return rc; }
	const size_t n_units = P.n_units;
	if (n_units == 0) return MPA_OK;
	static const bool show_top = [] { const char *e = getenv("MPA_DP_TOP"); return e && atoi(e) != 0; }();
	if (show_top) fputs(dp_plan_top(P, R.kn).c_str(), stderr);
	if ((rc = ctx->units.ensure(P.sz.units))) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->units.p, units, P.sz.units, hipMemcpyHostToDevice, s));
	R.ga.waves = d_gw;
	const size_t round_lds = dp_round_lds();
	if (dp_pool_enabled()) {
		if ((rc = pool_launch_round(ctx, s, R.ea, R.wa, R.ga, (DpRoundArgs*)(R.hup + P.up.args), n_units, P.n_group, round_lds, &R.pool_gen))) return rc;
		R.pool_pending = true;
	} else {
		if (round_lds > 48 * 1024) HIP_TRY(ensure_dynamic_lds((const void*)k_dp_round, ctx->device, round_lds));
		HIP_TRY(hipEventRecord(R.ev_round(0), s));
		hipLaunchKernelGGL(k_dp_round, dim3((unsigned)n_units), dim3(256), round_lds, s, R.ea, R.wa, R.ga, ctx->units.as<DpUnit>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(R.ev_round(1), s));
	}
	R.round_launched = true;
	ctx->stats.launches_ext++;
	return MPA_OK;
}

// launch, then (worker pool) wait until the round's units are done
static int dp_round(DpRun &R, GlobWave *d_gw, const char *what)
{
	int rc;
	if ((rc = dp_launch_round(R, d_gw)) != MPA_OK) return rc;
	R.mark(what);
	if (R.pool_pending) {
		if ((rc = pool_wait_round(R.ctx, R.s, R.pool_gen, (const DpUnit*)(R.hup + R.plan.up.units), R.plan.n_units)) != MPA_OK) return rc;
		R.pool_pending = false;
	}
	if (dp_pool_enabled()) R.mark("    dp: round (units done)");
	return MPA_OK;
}

// one stand-alone launch of a chunk's plain traceback sweep: T_16, T_32, T_64 and T_MB share one ("narrow", cls < 0), every wide class has its own
static hipError_t launch_glob_class(DpRun &R, const DpTbChunk &r, GlobWave *d_gw, int cls, hipStream_t st)
{
	GlobArgs &ga = R.ga;
	const bool wide_ge = R.plan.wide_ge;
	if (cls < 0) {
		int first[8], cnt[8];
		for (int c = 0; c < 8; ++c) first[c] = r.cls[c].first, cnt[c] = r.cls[c].cnt;
		ga.waves = d_gw;
		return launch_glob_narrow(ga, first, cnt, st, wide_ge);
	}
	ga.waves = d_gw + r.cls[cls].first;
	switch (cls) {
	case T_W2: return launch_glob_wide<2>(ga, r.cls[cls].cnt, st, wide_ge);
	case T_W4: return launch_glob_wide<4>(ga, r.cls[cls].cnt, st, wide_ge);
	case T_W8: return launch_glob_wide<8>(ga, r.cls[cls].cnt, st, wide_ge);
	default: return launch_glob_wide<16>(ga, r.cls[cls].cnt, st, wide_ge);
	}
}

// ---- 5. the chunks of the plain traceback sweep, each followed by k_backtrack; the round's launch rides with the first
static int dp_tb_chunks(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	char *hup = R.hup;
	int rc;
	for (size_t ri = 0; ri < P.chunks.size(); ++ri) {
		dp_plan_chunk_waves(P, ri);
		const DpTbChunk &r = P.chunks[ri];
		if (ri > 0) {                                                    // later chunks reuse the traceback buffer (and its staging): join everything first
			for (auto &l : R.launches) (void)hipStreamWaitEvent(s, ctx->lev[2 * l.side + 1], 0);
			HIP_TRY(wait_stream(ctx, s));
			R.add_chunk_times();                                           // (the previous chunk's sweep and walk)
		}
		int32_t *d_list = ctx->list.as<int32_t>();
		GlobWave *d_gw = (GlobWave*)((char*)ctx->list.p + ((P.tasks.size() * 4 + 63) & ~(size_t)63));
		memcpy(hup + P.up.list, r.list.data(), r.list.size() * 4);
		memcpy(hup + P.up.gw, r.waves.data(), r.waves.size() * sizeof(GlobWave));
		HIP_TRY(hipMemcpyAsync(d_list, hup + P.up.list, r.list.size() * 4, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(d_gw, hup + P.up.gw, r.waves.size() * sizeof(GlobWave), hipMemcpyHostToDevice, s));
		R.mark("    dp: traceback lists enqueued");
		R.ga.tb = ctx->tb.as<uint16_t>();
		HIP_TRY(hipEventRecord(ctx->ev[3], s));
		// every launch on its own stream (next to the extension classes in the first chunk); the walk needs them all
		HIP_TRY(hipEventRecord(ctx->fork_ev, s));
		const size_t first_glob_launch = R.launches.size();
		const bool in_round = ri == 0 && P.round_has_glob;
		const int order[5] = { T_W16, T_W8, T_W4, T_W2, -1 };
		for (int cls : order) {
			if (in_round && cls < T_W8) continue;                            // (only the 512/1024-thread traceback classes keep their own launch)
			if (cls >= 0 ? !r.cls[cls].cnt : !(r.cls[T_16].cnt + r.cls[T_32].cnt + r.cls[T_64].cnt + r.cls[T_MB].cnt)) continue;
			if ((int)R.launches.size() >= mpa_ctx_s::kSide - 1) {            // out of side streams (the last event pair times the round's launch): main stream
				HIP_TRY(launch_glob_class(R, r, d_gw, cls, s));
			} else {
				hipStream_t st = begin_side(R, false);
				HIP_TRY(launch_glob_class(R, r, d_gw, cls, st));
				end_side(R);
			}
			ctx->stats.launches_glob++;
		}
		if (in_round) {                                        // (behind the 512/1024-thread classes' own launches: with the worker pool the host waits here)
			ctx->stats.launches_glob++;
			if ((rc = dp_round(R, d_gw, "    dp: units up, round launched")) != MPA_OK) return rc;
		}
		for (size_t k = first_glob_launch; k < R.launches.size(); ++k) (void)hipStreamWaitEvent(s, ctx->lev[2 * R.launches[k].side + 1], 0);
		HIP_TRY(hipEventRecord(ctx->ev[4], s));
		hipLaunchKernelGGL(k_backtrack, dim3((unsigned)r.list.size()), dim3(64), 0, s, ctx->tasks.as<DTask>(), d_list, (int32_t)r.list.size(),
		                   ctx->tb.as<uint16_t>(), ctx->cig.as<uint32_t>(), ctx->ncig.as<int32_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(ctx->ev[5], s));
		R.glob_timed = true;                                              // (ev[3..5] are read after the next wait)
	}
	if (!R.round_launched && (rc = dp_round(R, nullptr, "    dp: (round without traceback launched)")) != MPA_OK) return rc;
	return MPA_OK;
}

// ---- 6. the walk of the checkpointed traceback: behind the round that swept its calls
static int dp_walk(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	if (!P.n_lite) return MPA_OK;
	memcpy(R.hup + P.up.wl, P.glob_ids.data() + P.n_reg_glob, 4 * P.n_lite);
	HIP_TRY(hipMemcpyAsync(ctx->wlist.p, R.hup + P.up.wl, 4 * P.n_lite, hipMemcpyHostToDevice, s));
	WalkArgs wk;
	wk.ga = R.ga, wk.ga.waves = nullptr, wk.list = ctx->wlist.as<int32_t>(), wk.n_list = (int32_t)P.n_lite;
	wk.lite = ctx->lite.as<uint32_t>(), wk.ckpt = ctx->ckpt.as<uint32_t>(), wk.cig = ctx->cig.as<uint32_t>(), wk.n_cigar = ctx->ncig.as<int32_t>();
	wk.n_blocks = (unsigned long long*)((char*)ctx->wlist.p + ((P.n_lite * 4 + 63) & ~(size_t)63));
	HIP_TRY(hipMemsetAsync(wk.n_blocks, 0, 8, s));
	// (the list is sorted by class: one launch per class, with the LDS that class's block of direction words needs)
	size_t at = 0;
	for (int cls = T_LITE16; cls <= T_LITE_W4; ++cls) {
		const size_t n_c = (size_t)P.walk_cnt[cls - T_LITE16];
		if (n_c == 0) continue;
		wk.list = ctx->wlist.as<int32_t>() + at, wk.n_list = (int32_t)n_c;
		if (cls == T_LITE_W4) {                                            // behind their own sweep; more LDS than a launch gets unasked
			if (R.l12_side >= 0) (void)hipStreamWaitEvent(s, ctx->lev[2 * R.l12_side + 1], 0);
			HIP_TRY(ensure_dynamic_lds((const void*)k_walk, ctx->device, WALK_LDS(256)));
		}
		hipLaunchKernelGGL(k_walk, dim3((unsigned)n_c), dim3(64), WALK_LDS(lite_columns(cls)), s, wk);
		at += n_c;
	}
	HIP_TRY(hipGetLastError());
	ctx->stats.launches_glob++;
	return MPA_OK;
}

// ---- 7. join the side streams; results into pinned memory behind the last kernel (extension outputs, traceback scores and
// CIGAR lengths, hand-off error flag, the walk's block count); the one wait of the round; kernel times
static int dp_join_and_download(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	const size_t n = P.tasks.size();
	for (auto &l : R.launches) (void)hipStreamWaitEvent(s, ctx->lev[2 * l.side + 1], 0);
	HIP_TRY(hipEventRecord(ctx->ev[2], s));
	int rc;
	if ((rc = ctx->h_down.ensure(P.dn.end))) return rc;
	char *hdn = R.hdn = ctx->h_down.as<char>();
	*(int32_t*)(hdn + P.dn.err) = 0;
	if (!P.ext_ids.empty()) HIP_TRY(hipMemcpyAsync(hdn + P.dn.eo, ctx->extout.p, sizeof(ExtOut) * n, hipMemcpyDeviceToHost, s));
	if (!P.glob_ids.empty()) {
		HIP_TRY(hipMemcpyAsync(hdn + P.dn.sc, ctx->score.p, n * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(hdn + P.dn.nc, ctx->ncig.p, n * 4, hipMemcpyDeviceToHost, s));
	}
	if (P.n_split) HIP_TRY(hipMemcpyAsync(hdn + P.dn.err, R.wa.err, 4, hipMemcpyDeviceToHost, s));
	*(unsigned long long*)(hdn + P.dn.wb) = 0;
	if (P.n_lite) HIP_TRY(hipMemcpyAsync(hdn + P.dn.wb, (char*)ctx->wlist.p + ((P.n_lite * 4 + 63) & ~(size_t)63), 8, hipMemcpyDeviceToHost, s));
	R.mark("    dp: round enqueued");
	HIP_TRY(wait_stream(ctx, s));
	R.mark("    dp: round (wait)");
	if (R.glob_timed) R.add_chunk_times();
	float ms_ext_sum = 0;                                                 // sum of the per-launch durations of the extension kernels
	if (R.round_launched && !dp_pool_enabled()) {
		(void)hipEventElapsedTime(&ms_ext_sum, R.ev_round(0), R.ev_round(1));
		ctx->stats.ms_round = ms_ext_sum, ctx->stats.launches_round = 1;
	}
	if (dp_pool_enabled()) pool_harvest(ctx, false);                    // (worker launches that have ended: into the context's totals)
	for (auto &l : R.launches) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ctx->lev[2 * l.side], ctx->lev[2 * l.side + 1]);
		if (l.is_ext) ms_ext_sum += ms;
		else if (l.side == R.l12_side) R.ms_glob += ms;                  // (the 129..256-column packed sweep: a traceback sweep like the chunks')
	}
	ctx->stats.ms_ext = ms_ext_sum;
	return MPA_OK;
}

// ---- 8. the real CIGARs gathered into a dense pool on the device (the slots were sized for the worst case, nl+al+4 words each:
// only that goes over PCIe); the caller's result records
static int dp_assemble(DpRun &R, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool)
{
	mpa_ctx_t *ctx = R.ctx;
	DpPlan &P = R.plan;
	hipStream_t s = R.s;
	const size_t n_glob = P.glob_ids.size();
	const ExtOut *eo = (const ExtOut*)(R.hdn + P.dn.eo);
	const int32_t *sc = (const int32_t*)(R.hdn + P.dn.sc), *nc = (const int32_t*)(R.hdn + P.dn.nc);
	int64_t &pool_n = R.pool_n;
	int64_t *dense_off = (int64_t*)(R.hup + P.up.off);                    // (the staging buffer's earlier sections have been consumed)
	for (size_t g = 0; g < n_glob; ++g) dense_off[g] = pool_n, pool_n += nc[P.glob_ids[g]];
	uint32_t *pool = (uint32_t*)malloc((size_t)(pool_n > 0 ? pool_n : 1) * 4);
	if (pool_n > 0) {
		int rc;
		if ((rc = ctx->cigd.ensure((size_t)pool_n * 4)) || (rc = ctx->cigoff.ensure(n_glob * 12 + 64)) || (rc = ctx->h_pool.ensure((size_t)pool_n * 4))) { free(pool); return rc; }
		int64_t *d_off = ctx->cigoff.as<int64_t>();
		int32_t *d_ids = (int32_t*)(d_off + n_glob);
		memcpy(R.hup + P.up.ids, P.glob_ids.data(), n_glob * 4);
		HIP_TRY(hipMemcpyAsync(d_off, dense_off, n_glob * 8, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(d_ids, R.hup + P.up.ids, n_glob * 4, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(k_cigar_gather, dim3((unsigned)n_glob), dim3(64), 0, s, ctx->tasks.as<DTask>(), d_ids, d_off, (int32_t)n_glob,
		                   ctx->ncig.as<int32_t>(), ctx->cig.as<uint32_t>(), ctx->cigd.as<uint32_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(ctx->h_pool.p, ctx->cigd.p, (size_t)pool_n * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		memcpy(pool, ctx->h_pool.p, (size_t)pool_n * 4);
	}
	std::vector<int64_t> off_of(P.tasks.size(), 0);
	for (size_t k = 0; k < n_glob; ++k) off_of[P.glob_ids[k]] = dense_off[k];
	for (size_t k = 0; k < P.tasks.size(); ++k) {
		const DTask &t = P.tasks[k];
		mpa_dp_rst_t &o = rst[k];
		if (t.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) {
			o.nt_len = eo[k].nt_len, o.aa_len = eo[k].aa_len, o.score = eo[k].score, o.n_cigar = 0, o.cigar_off = 0;
		} else {
			o.nt_len = t.nl, o.aa_len = t.al, o.score = sc[k], o.n_cigar = nc[k], o.cigar_off = off_of[k];
		}
	}
	if (cigar_pool) *cigar_pool = pool; else free(pool);
	if (n_pool) *n_pool = pool_n;
	return MPA_OK;
}

// ---- 9. statistics: the plan's counts, cells and bytes, the event times, the context's totals
static void dp_statistics(DpRun &R)
{
	mpa_ctx_t *ctx = R.ctx;
	mpa_dp_stats_t &st = ctx->stats;
	dp_plan_stats(R.plan);
	const mpa_dp_stats_t &ps = R.plan.stats;
	st.n_ext = ps.n_ext, st.n_glob = ps.n_glob, st.cells_ext = ps.cells_ext, st.cells_glob = ps.cells_glob, st.rows_prep = ps.rows_prep;
	st.alg_bytes_ext = ps.alg_bytes_ext, st.alg_bytes_glob = ps.alg_bytes_glob + 4 * R.pool_n;   // (+ the CIGARs' own words)
	st.n_ckpt = ps.n_ckpt, st.cells_ckpt = ps.cells_ckpt, st.n_ckpt_wide = ps.n_ckpt_wide, st.cells_ckpt_wide = ps.cells_ckpt_wide;
	st.cells_ext_round = ps.cells_ext_round, st.cells_glob_round = ps.cells_glob_round;
	st.walk_blocks = (int64_t)*(const unsigned long long*)(R.hdn + R.plan.dn.wb);
	float ms = 0;
	(void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]); st.ms_prep = ms;
	st.ms_glob = R.ms_glob, st.ms_backtrack = R.ms_bt;
	timing_note("    dp: GPU prep kernels", st.ms_prep);
	timing_note("    dp: GPU round kernel", st.ms_round);
	timing_note("    dp: GPU walk", R.ms_bt);
	{ float w = 0; (void)hipEventElapsedTime(&w, ctx->ev[0], ctx->ev[2]); st.ms_total = w; }   // wall time of the whole batch on the device
	mpa_dp_stats_t &t = ctx->total;
	t.n_ext += st.n_ext, t.n_glob += st.n_glob, t.cells_ext += st.cells_ext, t.cells_glob += st.cells_glob, t.rows_prep += st.rows_prep;
	t.alg_bytes_ext += st.alg_bytes_ext, t.alg_bytes_glob += st.alg_bytes_glob;
	t.n_ckpt += st.n_ckpt, t.cells_ckpt += st.cells_ckpt, t.walk_blocks += st.walk_blocks;
	t.n_ckpt_wide += st.n_ckpt_wide, t.cells_ckpt_wide += st.cells_ckpt_wide;
	t.ms_prep += st.ms_prep, t.ms_ext += st.ms_ext, t.ms_glob += st.ms_glob, t.ms_backtrack += st.ms_backtrack, t.ms_total += st.ms_total;
	t.launches_ext += st.launches_ext, t.launches_glob += st.launches_glob;
	t.cells_ext_round += st.cells_ext_round, t.cells_glob_round += st.cells_glob_round, t.ms_round += st.ms_round, t.launches_round += st.launches_round;
}

// the executor's knobs as the planner takes them (the environment: read when the context was created, or once per process)
static DpPlanKnobs dp_plan_knobs(const mpa_ctx_t *ctx)
{
	static const bool ext_dual = [] { const char *e = getenv("MPA_DP_EXT_DUAL"); return !e || atoi(e) != 0; }();
	static const bool unit_prio = [] { const char *e = getenv("MPA_DP_PRIO"); return !e || atoi(e) != 0; }();   // (MPA_DP_PRIO=0: measurement)
	DpPlanKnobs kn;
	kn.lite_min = ctx->lite_min, kn.lite_wide = ctx->lite_wide, kn.no_split = ctx->no_split, kn.antidiag = ctx->antidiag, kn.pool = dp_pool_enabled();
	kn.ext_dual = ext_dual, kn.unit_prio = unit_prio, kn.tb_budget = (int64_t)ctx->tb_budget;
	return kn;
}

static int mpa_dp_run_impl(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q,
               int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool)
{
	if (cigar_pool) *cigar_pool = nullptr;
	if (n_pool) *n_pool = 0;
	if (!ctx) { set_error("no device context"); return MPA_ERR_NO_DEVICE; }
	if (ctx->device >= mpa_idx_s::kMaxDevices || !mi->dev[ctx->device]) { set_error("index is not resident on this context's device (call mpa_idx_to_device)"); return MPA_ERR_ARG; }
	ctx->stats = mpa_dp_stats_t();
	if (n <= 0) return MPA_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	const double t_begin = now_ms();
	int rc;
	// 1. plan
	DpPlan plan;
	const DpPlanKnobs kn = dp_plan_knobs(ctx);
	if ((rc = dp_plan(in, n, mi->ctg.empty() ? nullptr : &mi->ctg[0].len, sizeof(mi->ctg[0]), (int32_t)mi->ctg.size(), q, opt, kn, sizeof(DpRoundArgs), plan))) { set_error(plan.err); return rc; }
	timing_note("  dp: classify/sort/layout", now_ms() - t_begin);
	DpRun R{ ctx, ctx->stream, plan, kn };
	R.t_mark = now_ms();
	if ((rc = dp_size_pools(R)) ||                             // 2. pools and staging
	    (rc = dp_upload_and_prep(R, mi, opt, q)) ||            // 3. uploads, memsets, prep
	    (rc = dp_side_launches(R)) ||                          // 4. next to the round: anti-diagonal, huge, T_LITE_W4 sweep
	    (rc = dp_tb_chunks(R)) ||                              // 5. traceback chunks with the round's launch
	    (rc = dp_walk(R)) ||                                   // 6. walk
	    (rc = dp_join_and_download(R)))                        // 7. join, download, the one wait
		return rc;
	// a boundary hand-off that never arrived (bounded spin in the kernel): the producer workgroup was running (it drew its
	// ticket first) but made no progress for seconds -- a stalled hardware queue under oversubscription.  Nothing of this round
	// has been handed to the caller yet: mpa_dp_run() repeats it with those calls on the one-wave path (k_ext_huge, same bits).
	static const bool test_fail = [] { const char *e = getenv("MPA_TEST_HANDOFF_FAIL"); return e && atoi(e) != 0; }();
	if (*(const int32_t*)(R.hdn + plan.dn.err) || (test_fail && plan.n_split && !ctx->no_split)) {
		set_error("k_ext_wide_split: a column-block hand-off between workgroups timed out"); return MPA_RETRY_NO_SPLIT;
	}
	timing_note("  dp: upload+kernels (wall)", now_ms() - t_begin);
	const double t_res = now_ms();
	if ((rc = dp_assemble(R, rst, cigar_pool, n_pool))) return rc;   // 8. CIGAR gather, results
	timing_note("  dp: download+assemble", now_ms() - t_res);
	dp_statistics(R);                                           // 9.
	return MPA_OK;
}

int mpa_dp_run(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q,
               int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&] {
		int rc = mpa_dp_run_impl(ctx, mi, opt, q, n, in, rst, cigar_pool, n_pool);
		if (rc == MPA_RETRY_NO_SPLIT) {
			ctx->no_split = true, ++ctx->handoff_retries;
			rc = mpa_dp_run_impl(ctx, mi, opt, q, n, in, rst, cigar_pool, n_pool);
			ctx->no_split = false;
			if (rc == MPA_RETRY_NO_SPLIT) rc = MPA_ERR_HIP;
		}
		return rc;
	});
}

int64_t mpa_dp_handoff_retries(const mpa_ctx_t *ctx) { return ctx ? ctx->handoff_retries : 0; }
void mpa_dbg_antidiag(mpa_ctx_t *ctx, int on) { if (ctx) ctx->antidiag = on != 0; }
int64_t mpa_dbg_dp_plan(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                        const int64_t *knobs, void *buf, int64_t cap)
{
	return mpa::guarded<int64_t>(MPA_ERR_HIP, [&]() -> int64_t {
		DpPlanKnobs kn;
		kn.lite_min = (int32_t)knobs[0], kn.lite_wide = (int32_t)knobs[1], kn.no_split = (int32_t)knobs[2], kn.antidiag = (int32_t)knobs[3], kn.pool = (int32_t)knobs[4];
		kn.ext_dual = (int32_t)knobs[5], kn.unit_prio = (int32_t)knobs[6], kn.tb_budget = knobs[7];
		const mpa_qbatch_t q{ n_seq, nullptr, q_off };
		DpPlan plan;
		int64_t r = dp_plan(tasks, n, ctg_len, sizeof(int64_t), n_ctg, &q, opt, kn, sizeof(DpRoundArgs), plan);
		if (r == MPA_OK) r = dp_plan_serialize(plan, kn, buf, cap);
		if (r < 0) set_error(plan.err);
		return r;
	});
}
void mpa_idx_build_last_stats(const mpa_ctx_t *ctx, mpa_idx_build_stats_t *st) { if (st) *st = ctx ? ctx->idx_stats : mpa_idx_build_stats_t{}; }
void mpa_dbg_idx_build_budget(mpa_ctx_t *ctx, int64_t bytes) { if (ctx) ctx->idx_budget_dbg = bytes > 0 ? bytes : 0; }
int32_t mpa_dbg_idx_build_hist(const mpa_ctx_t *ctx, int64_t *hist, int32_t cap)
{
	if (!ctx) return 0;
	const int32_t n = (int32_t)ctx->idx_hist.size();
	if (hist && cap > 0) memcpy(hist, ctx->idx_hist.data(), (size_t)std::min(n, cap) * 8);
	return n;
}
int64_t mpa_device_bytes(void) { return (int64_t)g_dev_bytes.load(); }
int64_t mpa_pool_growths(void) { return (int64_t)g_pool_growths.load(); }

} // extern "C"

#include "gs32_exec.hip"
