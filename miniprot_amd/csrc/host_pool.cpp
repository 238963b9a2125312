// host_pool.cpp -- the persistent worker pools behind parallel_for() (host_batch.h) and the calling thread's place among them.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include "host_batch.h"

namespace mpa {

// A small persistent worker pool: the stage machine calls parallel_for several times per batch and thread
// creation would otherwise cost more than some of the stages.
class WorkerPool {
public:
	// never destroyed: workers outlive main().  One pool per lane, so that the pipeline stages of mpa_map_batches()
	// (seeding of the next batch / DP-round bookkeeping / flattening + formatting of the previous one) can each run
	// their own parallel region at the same time.
	static const int kPools = 24 * 8;                   // 24 lanes per pipeline (mpa_map_batches), up to eight pipelines per process (mpa_map_batches_multi)
	static WorkerPool &get(int lane) { static WorkerPool *p = new WorkerPool[kPools]; return p[lane % kPools]; }
	void run(int n_threads, int64_t n, const std::function<void(int64_t)> &fn) {
		if (n_threads <= 1 || n <= 1) { for (int64_t i = 0; i < n; ++i) fn(i); return; }
		std::unique_lock<std::mutex> run_lock(run_mu_);              // one parallel region at a time
		ensure(n_threads - 1);
		{
			std::lock_guard<std::mutex> g(mu_);
			fn_ = &fn, n_ = n, next_.store(0), active_ = std::min<int>(n_threads - 1, (int)workers_.size()), pending_ = active_, ++epoch_;
		}
		cv_.notify_all();
		work();
		std::unique_lock<std::mutex> g(mu_);
		done_cv_.wait(g, [&] { return pending_ == 0; });
		fn_ = nullptr;
	}
private:
	void ensure(int k) {
		while ((int)workers_.size() < k) {
			const int id = (int)workers_.size();
			workers_.emplace_back([this, id] { loop(id); });
			workers_.back().detach();
		}
	}
	void work() { CpuSpan cs(label_); for (;;) { int64_t i = next_.fetch_add(1); if (i >= n_) break; (*fn_)(i); } }
public:
	const char *label_ = "pool (outside a stream)";     // what the CPU time of this pool's parallel regions is booked under (MPA_TIMING)
private:
	void loop(int id) {
		uint64_t seen = 0;
		for (;;) {
			std::unique_lock<std::mutex> g(mu_);
			cv_.wait(g, [&] { return epoch_ != seen && id < active_; });
			seen = epoch_;
			g.unlock();
			work();
			g.lock();
			if (--pending_ == 0) done_cv_.notify_all();
		}
	}
	std::mutex mu_, run_mu_;
	std::condition_variable cv_, done_cv_;
	std::vector<std::thread> workers_;
	const std::function<void(int64_t)> *fn_ = nullptr;
	int64_t n_ = 0;
	std::atomic<int64_t> next_{0};
	int active_ = 0, pending_ = 0;
	uint64_t epoch_ = 0;
};

static thread_local int tl_pool_lane = 0;
static thread_local int tl_thread_div = 1;          // pipeline stages with light host work take a fraction of the threads
void parallel_run(int n_threads, int64_t n, const std::function<void(int64_t)> &fn)
{
	WorkerPool::get(tl_pool_lane).run(std::max(1, n_threads / tl_thread_div), n, fn);
}

// A stage thread of the stream pipeline (host_pipeline.cpp) takes a pool of its own, a share of the threads and a label for the pool's
// CPU time; pool_stage_leave() puts the calling thread back where every other thread is (pool 0, all the threads)
void pool_stage_enter(int lane, int thread_div, const char *label)
{
	tl_pool_lane = lane, tl_thread_div = thread_div;
	WorkerPool::get(tl_pool_lane).label_ = label;
}
void pool_stage_leave() { tl_thread_div = 1, tl_pool_lane = 0; }

} // namespace mpa
