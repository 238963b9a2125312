// dev_ctx.hip -- the device context of the library (dev_ctx.h): creation and destruction, its memory pools and the process-wide
// counters behind them, the sleeping stream wait, the upload of the index, the sibling contexts of a stream pipeline and their shared
// pool hints.  No kernels: the stages are seed_run.hip, refine_run.hip, index_run.hip, dp_exec.hip and stats_run.hip.
#include "dev_ctx.h"

namespace mpa {

std::atomic<long long> g_dev_bytes{0}, g_pool_growths{0};
thread_local bool tl_alloc_failed = false;

int DevBuf::ensure(size_t bytes)
{
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
	if (p) ++g_pool_growths;
	release();
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
	hipError_t e = take(want);
	if (e != hipSuccess && want > asked + 4096) { want = asked + 4096; e = take(want); }
	if (e != hipSuccess) { tl_alloc_failed = true; set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); return MPA_ERR_HIP; }
	timing_note("    pool growth (device)", now_ms() - t0);
	return MPA_OK;
}

int DevBuf::ensure_exact(size_t bytes)
{
	if (bytes <= cap) return MPA_OK;
	if (p) ++g_pool_growths;
	if (take(bytes) != hipSuccess) { tl_alloc_failed = true; set_error("hipMalloc(" + std::to_string(bytes) + ") failed"); return MPA_ERR_HIP; }
	return MPA_OK;
}

hipError_t DevBuf::take(size_t bytes)
{
	release();
	const hipError_t e = hipMalloc(&p, bytes);
	if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
	cap = bytes;
	g_dev_bytes += (long long)cap;
	return hipSuccess;
}

// Wait for everything enqueued on a stream -- asleep.  hipStreamSynchronize() spins on the completion signal by default; a
// pipeline keeps eight or nine host threads waiting for the device at any time (DP lanes, seeders, planners), and on a host
// that gives the process a CPU quota (16 cores per GPU on the boxes this was measured on) spinning waiters eat the very cores
// the host stages need.  An event created with hipEventBlockingSync makes the runtime block on the signal instead.
// Measured (round 3): even the "blocking" hipEventSynchronize costs a waiting thread about half a core, so the wait polls the
// event and SLEEPS 100 us between polls after a short burst of immediate ones.
hipError_t wait_stream(mpa_ctx_t *ctx, hipStream_t s)
{
	ctx->n_waits.fetch_add(1, std::memory_order_relaxed);
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
hipError_t upload_large(void *dst, const void *src, size_t bytes, hipStream_t s)
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
// (a seeder or planner of a planned layout has one stream, created in the plan's class: stream_plan.h)
void ensure_seed_stream(mpa_ctx_t *ctx)
{
	if (ctx->seed_stream) return;
	if (ctx->one_stream) { ctx->seed_stream = ctx->stream; return; }
	static const bool high = [] { const char *e = getenv("MPA_PRIO_SEED"); return !e || atoi(e) != 0; }();
	int least = 0, greatest = 0;
	(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
	if (hipStreamCreateWithPriority(&ctx->seed_stream, hipStreamNonBlocking, high ? greatest : least) != hipSuccess) ctx->seed_stream = ctx->stream;
}

hipError_t create_stream_in_class(hipStream_t *s, int cls)
{
	if (cls == SC_NORMAL) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
	int least = 0, greatest = 0;
	(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
	return hipStreamCreateWithPriority(s, hipStreamNonBlocking, cls == SC_HIGH ? greatest : least);
}

// GPU_MAX_HW_QUEUES as the process sees it when its first context is created (the library's constructor sets 16 where the variable is
// unset: tables.cpp); the runtime reads it when it initialises, which is not later than that
int ctx_hw_queues(void)
{
	static const int q = [] { const char *e = getenv("GPU_MAX_HW_QUEUES"); const int v = e && *e ? atoi(e) : 4; return v < 1 ? 4 : v; }();
	return q;
}

int dev_upload_index(mpa_ctx_t *ctx, mpa_idx_s *mi)
{
	if (ctx->device < 0 || ctx->device >= mpa_idx_s::kMaxDevices) { set_error("device number beyond what an index keeps copies for"); return MPA_ERR_UNSUPPORTED; }
	static std::mutex mu[mpa_idx_s::kMaxDevices];             // one per device: the pipelines of several devices upload side by side
	std::lock_guard<std::mutex> g(mu[ctx->device]);
	if (mi->dev[ctx->device]) return MPA_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	// (an upload that fails half-way gives everything back with the record: the caller may retry, e.g. on the host path, and must not leak HBM)
	std::unique_ptr<DeviceIndex> d(new DeviceIndex());
	d->device = ctx->device;
	const size_t n = mi->ctg.size();
	std::vector<int64_t> off(n), len(n);
	for (size_t i = 0; i < n; ++i) off[i] = mi->ctg[i].off, len[i] = mi->ctg[i].len;
	HIP_TRY(d->seq.take(mi->seq.size() + 16));
	HIP_TRY(d->ctg_off.take(n * 8 + 8));
	HIP_TRY(d->ctg_len.take(n * 8 + 8));
	{ const double t0 = now_ms(); HIP_TRY(upload_large(d->seq, mi->seq.data(), mi->seq.size(), ctx->stream)); timing_note("index upload: packed genome", now_ms() - t0); }
	HIP_TRY(hipMemcpy(d->ctg_off, off.data(), n * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d->ctg_len, len.data(), n * 8, hipMemcpyHostToDevice));
	if (!mi->spsc.empty()) {
		HIP_TRY(d->spsc.take(mi->spsc.size() + 16));
		HIP_TRY(hipMemcpy(d->spsc, mi->spsc.data(), mi->spsc.size(), hipMemcpyHostToDevice));
	}
	mi->dev[ctx->device] = d.release();
	return MPA_OK;
}

// Table `t` of this device's resident index (kb, ki, bo), uploaded on first use: `bytes` of `src` into an allocation 16 bytes longer.
// Several seeders get here at once: one of them uploads, under the device's lock, and the table shows only when it is complete.
// hipErrorOutOfMemory: no device memory for it; another error: the copy's.  What the caller makes of either is its own business.
hipError_t dev_index_table(mpa_ctx_t *ctx, DevBuf &t, const void *src, size_t bytes, const char *note)
{
	if (t.p) return hipSuccess;
	static std::mutex mu[mpa_idx_s::kMaxDevices];             // (per device, like dev_upload_index)
	std::lock_guard<std::mutex> g(mu[ctx->device]);
	if (t.p) return hipSuccess;
	DevBuf up;
	if (up.take(bytes + 16) != hipSuccess) return hipErrorOutOfMemory;
	const double t0 = now_ms();
	const hipError_t e = upload_large(up.p, src, bytes, ctx->stream);
	if (e != hipSuccess) { (void)hipGetLastError(); return e; }
	timing_note(note, now_ms() - t0);
	t = std::move(up);
	return hipSuccess;
}

void dev_free_index(mpa_idx_s *mi)
{
	for (DeviceIndex *&d : mi->dev) {
		if (!d) continue;
		(void)hipSetDevice(d->device);
		delete d;
		d = nullptr;
	}
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember it per (kernel, device), under a lock -- several
// DP lanes and seeders get here at once, and a process may hold contexts on several devices
hipError_t ensure_dynamic_lds(const void *fn, int device, size_t bytes)
{
	static std::mutex mu;
	static std::vector<std::pair<const void*, int>> done;
	std::lock_guard<std::mutex> g(mu);
	for (auto &d : done) if (d.first == fn && d.second == device) return hipSuccess;
	const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
	if (e == hipSuccess) done.emplace_back(fn, device);
	return e;
}

} // namespace mpa

extern "C" {

int mpa_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// the context knobs as the environment sets them (read for every context that is created for itself; a sibling takes its root's)
static CtxKnobs ctx_knobs_from_env(void)
{
	CtxKnobs k;
	if (const char *s = getenv("MPA_TB_BUDGET_MB")) k.tb_budget = (size_t)atoll(s) << 20;
	if (const char *s = getenv("MPA_DP_LITE_MIN")) k.lite_min = atoi(s);
	if (const char *s = getenv("MPA_DP_LITE_WIDE")) k.lite_wide = atoi(s) != 0;
	if (const char *s = getenv("MPA_DP_LITE_W8")) k.lite_w8 = atoi(s) != 0;
	if (const char *s = getenv("MPA_DP_SPLIT_WIDE")) k.split_wide = atoi(s) != 0;
	if (const char *s = getenv("MPA_DP_HUGE_WG")) k.huge_wg = atoi(s) != 0;
	if (const char *s = getenv("MPA_DP_MB_WG")) k.mb_wg = atoi(s) != 0;
	return k;
}

// cls < 0: a context of its own (mpa_ctx_create) -- a normal main stream, or a high one with MPA_PRIO_MAIN=1; otherwise the class
// the stream plan gives this context's main stream
static mpa_ctx_t *ctx_create_in_class(int device, int cls)
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
	(void)ctx_hw_queues();
	bool ok = create_stream_in_class(&ctx->stream, cls >= 0 ? cls : main_high ? SC_HIGH : SC_NORMAL) == hipSuccess;
	for (auto &e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	for (auto &e : ctx->lev) ok = ok && hipEventCreate(&e) == hipSuccess;
	ok = ok && hipEventCreate(&ctx->fork_ev) == hipSuccess;
	ok = ok && hipEventCreateWithFlags(&ctx->wait_ev, hipEventBlockingSync | hipEventDisableTiming) == hipSuccess;
	if (!ok) {                                            // a null handle would silently alias the legacy default stream
		set_error("creating the context's HIP streams/events failed");
		mpa_ctx_destroy(ctx);
		return nullptr;
	}
	ctx->knobs = ctx_knobs_from_env();
	return ctx;
}

mpa_ctx_t *mpa_ctx_create(int device) { return ctx_create_in_class(device, -1); }

void mpa_ctx_destroy(mpa_ctx_t *ctx)
{
	if (!ctx) return;
	for (mpa_ctx_s *sb : ctx->siblings) mpa_ctx_destroy(sb);
	ctx->siblings.clear();
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	WorkerBufs &W = ctx->worker;
	if (W.worker_stream) { (void)hipStreamSynchronize(W.worker_stream); (void)hipStreamDestroy(W.worker_stream); }   // (workers exit by themselves once no slot has a unit left)
	for (auto *v : { &W.wl_busy, &W.wl_free }) { for (auto &w : *v) { (void)hipEventDestroy(w.e0); (void)hipEventDestroy(w.e1); } v->clear(); }
	if (W.arm_ev) (void)hipEventDestroy(W.arm_ev);
	if (W.dp_done) (void)hipHostFree(W.dp_done);
	if (W.pool_base) (void)hipEventDestroy(W.pool_base);
	if (W.dp_pool) (void)hipFree(W.dp_pool);
	for (auto &e : ctx->ev) if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->lev) if (e) (void)hipEventDestroy(e);
	if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
	if (ctx->wait_ev) (void)hipEventDestroy(ctx->wait_ev);
	for (auto &st : ctx->side) if (st) (void)hipStreamDestroy(st);
	if (ctx->seed_stream && ctx->seed_stream != ctx->stream) (void)hipStreamDestroy(ctx->seed_stream);
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;                                            // (its pools, pinned blocks and result holders go with their members)
}

int mpa_idx_to_device(mpa_ctx_t *ctx, mpa_idx_t *mi) { return dev_upload_index(ctx, mi); }

int64_t mpa_device_bytes(void) { return (int64_t)g_dev_bytes.load(); }
int64_t mpa_pool_growths(void) { return (int64_t)g_pool_growths.load(); }

} // extern "C"

namespace mpa {
// one more sibling of a root: same device, own streams and pools, the root's knobs (cls: as ctx_create_in_class takes it)
static mpa_ctx_t *ctx_add_sibling(mpa_ctx_t *root, int cls)
{
	mpa_ctx_t *sb = ctx_create_in_class(root->device, cls);
	if (!sb) return nullptr;
	sb->root = root;
	sb->knobs = root->knobs;
	root->siblings.push_back(sb);
	return sb;
}
// k-th sibling of a context, created on first use
mpa_ctx_t *ctx_sibling(mpa_ctx_t *ctx, int k)
{
	if (k <= 0) return ctx;
	while ((int)ctx->siblings.size() < k) if (!ctx_add_sibling(ctx, -1)) return nullptr;
	return ctx->siblings[k - 1];
}
void ctx_set_side_offset(mpa_ctx_t *ctx, int off) { ctx->side_off = off; }

const StreamPlan *ctx_stream_plan(const mpa_ctx_t *root) { return root ? root->splan.get() : nullptr; }

// Siblings 1 .. lanes - 1 are the DP lanes behind the root (lane 0, whose normal main stream exists), then the seeders, then the
// planners: the plan's creation order.  Between two streams of batches nothing is in flight on a sibling, so a plan that differs from
// the one they were made by (another layout, other stage counts) replaces them, pools included.
int ctx_apply_stream_plan(mpa_ctx_t *root, int n_lanes, int n_seed, int n_plan, int layout)
{
	const StreamPlan p = stream_plan(ctx_hw_queues(), n_lanes, n_seed, n_plan, layout);
	const int n_sib = p.n_lanes - 1 + p.n_seed + p.n_plan;
	if (!root->splan || memcmp(root->splan.get(), &p, sizeof p) != 0) {
		for (mpa_ctx_s *sb : root->siblings) mpa_ctx_destroy(sb);
		root->siblings.clear();
		for (auto &st : root->side) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }   // (the root's own, of the old plan's class)
		if (!root->splan) root->splan.reset(new StreamPlan());
		*root->splan = p;
	}
	auto entry = [&](int k, const StreamSlot *&main, bool &lane) {       // sibling k (>= 1) of the plan
		lane = k < p.n_lanes;
		main = lane ? &p.lane[k] : k < p.n_lanes + p.n_seed ? &p.seed_main[k - p.n_lanes] : &p.plan_main[k - p.n_lanes - p.n_seed];
	};
	root->side_cap = p.side_cap[0], root->side_cls = p.side_cls[0];
	while ((int)root->siblings.size() < n_sib) {
		const int k = (int)root->siblings.size() + 1;
		const StreamSlot *main; bool lane;
		entry(k, main, lane);
		mpa_ctx_t *sb = ctx_add_sibling(root, p.layout == SL_LEGACY ? -1 : main->cls);
		if (!sb) return MPA_ERR_HIP;
		sb->one_stream = !lane && p.layout != SL_LEGACY;
		if (lane) sb->side_cap = p.side_cap[k], sb->side_cls = p.side_cls[k];
	}
	return MPA_OK;
}
// `ctx` (the root itself or one of its siblings) plays part `role` of the root's stream pipeline: 0 DP lane, 1 seeder, 2 planner.
// The hint table has a slot per role and registered pool: every context registers the same pools in the same order.
void ctx_set_role(mpa_ctx_t *root, mpa_ctx_t *ctx, int role)
{
	const size_t n = ctx->pools.all.size();
	if (!root->hints) root->hints.reset(new std::atomic<size_t>[3 * n]());
	for (size_t k = 0; k < n; ++k) ctx->pools.all[k]->hint = &root->hints[(size_t)role * n + k];
}
SeedHold *ctx_seed_hold(mpa_ctx_t *ctx, int k)
{
	while ((int)ctx->holds.size() <= k) ctx->holds.emplace_back(new SeedHold());
	return ctx->holds[(size_t)k].get();
}

// the registered device pools of a root context (sibling 0) or of its sibling number `sibling`: their names and capacities in
// registration order, as many as fit `cap`; returns their number, or -1 without such a context (mpa_dbg_ctx_pools)
int32_t ctx_pool_list(const mpa_ctx_t *ctx, int32_t sibling, const char **names, int64_t *caps, int32_t cap)
{
	if (!ctx || sibling < 0 || sibling > (int32_t)ctx->siblings.size()) return -1;
	const PoolRegistry &R = (sibling ? ctx->siblings[(size_t)sibling - 1] : ctx)->pools;
	for (size_t k = 0; k < R.all.size() && (int32_t)k < cap; ++k) names[k] = R.all[k]->name, caps[k] = (int64_t)R.all[k]->cap;
	return (int32_t)R.all.size();
}

// (MPA_TIMING) the device pools of a root context and its siblings, largest first: where the HBM of a pipeline goes
void ctx_pool_report(mpa_ctx_t *root)
{
	std::vector<mpa_ctx_t*> all{ root };
	for (mpa_ctx_t *sb : root->siblings) all.push_back(sb);
	size_t grand = 0;
	for (size_t c = 0; c < all.size(); ++c) {
		size_t tot = 0;
		std::vector<std::pair<size_t, const char*>> big;
		for (const CtxPool *b : all[c]->pools.all) { tot += b->cap; if (b->cap >= ((size_t)64 << 20)) big.push_back({ b->cap, b->name }); }
		std::stable_sort(big.begin(), big.end(), [](auto &x, auto &y) { return x.first > y.first; });
		fprintf(stderr, "[mpa-pools] context %zu: %.2f GB;", c, tot / 1e9);
		for (auto &x : big) fprintf(stderr, " %s %.2f", x.second, x.first / 1e9);
		fprintf(stderr, "\n");
		grand += tot;
	}
	fprintf(stderr, "[mpa-pools] all contexts of the pipeline: %.2f GB of pools (+ the resident index)\n", grand / 1e9);
}

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
