// host_pipeline.h -- the scheduler of the stream pipeline (mpa_map_batches, host_pipeline.cpp) on its own: who may start which batch
// when, the early end of a job, first-error-wins.  Standard library only: the stage bodies come in as callbacks, so the same code
// runs against stubs on a CPU (tests/pipeline_check.cpp, under ThreadSanitizer and AddressSanitizer) and against the device.
// A job's batches go through five stages in slots k = 0, 1, ... (slot k = the k-th batch claimed): sketch (1 thread; it also claims)
// -> seed (n_seed threads) -> plan (n_plan threads) -> DP rounds (n_lanes threads, lane 0 is the caller's) -> finish (1 thread, in
// slot order).  One mutex, one condition variable; the waits are commented where they stand, and why the pipeline is this deep is
// with the defaults in host_pipeline.cpp (its plan_ahead constant was 0 and is gone from the planner's wait).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mpa {

enum StreamStage { STREAM_SKETCH = 0, STREAM_SEED, STREAM_PLAN, STREAM_DP, STREAM_FINISH };
struct StreamShape {
	int32_t n_batches;                 // batches of the job (a claim names one of them)
	int n_lanes, n_seed, n_plan;       // threads of the DP, seeding and planning stages
	int rc_bad_claim, rc_exception;    // the caller's codes for a repeated or surplus claim and for an exception in a stage thread
};
// Every callback runs outside the scheduler's lock.  An int result is 0 or the error code that ends the job; its message is then
// read with last_error() on the same thread.
struct StreamStages {
	std::function<int32_t()> claim;                                        // the next batch of the job, or < 0: none left
	std::function<int(int32_t k, int32_t g)> sketch;                       // slot k gets batch g
	std::function<int(int sd, int32_t k, int holder)> seed;                // seeder sd, holder = k % (n_seed + n_plan)
	std::function<void(int pl, int32_t k)> plan;
	std::function<int(int d, int32_t k)> dp;
	std::function<void(int32_t k, int32_t g, int32_t j)> finish;           // j: ordinal of the batch among those this call maps
	std::function<void(StreamStage st, int i, const std::function<void()> &loop)> thread;   // wraps the whole loop of thread i of a stage: calls loop() once
	std::function<std::string()> last_error;
};
struct StreamResult {
	int rc = 0;
	std::string err;                   // the first error's message
	int32_t n_mapped = 0;              // batches claimed; order[j] = the batch with ordinal j.  Both stay empty on error
	std::vector<int32_t> order;
};

class Stream {
public:
	Stream(const StreamShape &shape, const StreamStages &stages)
		: S(shape), F(stages), n_seed_ctx(shape.n_seed + shape.n_plan), slot((size_t)shape.n_batches), taken((size_t)shape.n_batches, 0), n_total(shape.n_batches) {}
	// Runs the job; lane 0 of the DP stage on the calling thread.  Every thread has been joined when it returns.
	void run(StreamResult &out)
	{
		{
			Threads th{ this, {} };
			try {
				th.t.reserve((size_t)(2 + S.n_seed + S.n_plan + S.n_lanes));
				th.start(STREAM_SKETCH, 0, &Stream::sketcher);
				for (int sd = 0; sd < S.n_seed; ++sd) th.start(STREAM_SEED, sd, &Stream::seeder);
				for (int pl = 0; pl < S.n_plan; ++pl) th.start(STREAM_PLAN, pl, &Stream::planner);
				th.start(STREAM_FINISH, 0, &Stream::finisher);
				for (int d = 1; d < S.n_lanes; ++d) th.start(STREAM_DP, d, &Stream::dp_lane);
			} catch (const std::exception &e) { fail(S.rc_exception, std::string("stream threads: ") + e.what()); }
			stage_thread(STREAM_DP, 0, &Stream::dp_lane);
		}
		out = StreamResult();
		out.rc = rc_all, out.err = err;
		if (rc_all != 0) return;
		out.n_mapped = n_claimed;
		out.order.assign((size_t)n_total, -1);
		for (int32_t k = 0; k < n_total; ++k) out.order[(size_t)slot[k].j] = slot[k].g;
	}
	// batches sketched (or being sketched) that no seeder has taken yet; what the sketcher's wait bounds (for the claim callback of a test)
	int32_t sketched_ahead() { std::lock_guard<std::mutex> g(mu); return n_created - next_seed; }

private:
	struct Slot {
		int32_t g = 0, j = 0;                             // index into the job's batches; ordinal of the batch among those this call maps
		bool sketched = false, seeded = false, begun = false, dp_done = false;
	};
	// The stage threads.  Whatever ends run() -- a thread that could not be started, too -- they are joined, not destroyed joinable
	// (std::terminate): leaving by an exception raises the error flag first, which every wait below looks at.
	struct Threads {
		Stream *s;
		std::vector<std::thread> t;
		void start(StreamStage st, int i, void (Stream::*loop)(int)) { t.emplace_back([this, st, i, loop] { s->stage_thread(st, i, loop); }); }
		~Threads()
		{
			if (std::uncaught_exceptions() > 0) s->fail(s->S.rc_exception, "stream threads: left by an exception");
			for (std::thread &x : t) if (x.joinable()) x.join();
		}
	};
	const StreamShape S;
	const StreamStages &F;
	const int n_seed_ctx;                                 // holders: one per batch that can be between the start of seeding and the end of planning
	std::vector<Slot> slot;
	std::vector<uint8_t> taken;                           // batches a claim has handed out already
	std::mutex mu;
	std::condition_variable cv;
	int32_t n_dp_done = 0, n_planned = 0, next_seed = 0, next_plan = 0, next_dp = 0;
	int32_t n_total;                                      // units this call maps: shrinks to the number created when the job runs out (guarded by mu)
	int32_t n_created = 0, n_claimed = 0;                 // units created so far; batches taken
	bool exhausted = false;
	int rc_all = 0;
	std::string err;

	void fail(int rc, const std::string &msg) { std::lock_guard<std::mutex> g(mu); if (rc_all == 0) rc_all = rc, err = msg; cv.notify_all(); }
	// (an exception inside a stage thread -- out of memory, say -- must become an error code, not std::terminate)
	void stage_thread(StreamStage st, int i, void (Stream::*loop)(int))
	{
		static const char *const kName[5] = { "sketch stage", "seeding stage", "planning stage", "DP lane", "output stage" };
		try { F.thread(st, i, [this, i, loop] { (this->*loop)(i); }); }
		catch (const std::exception &e) { fail(S.rc_exception, std::string(kName[st]) + ": " + e.what()); }
	}
	// Sketcher: the host half of seeding as a stage of its own, one or two batches ahead of the seeders.  It also claims the job's batches.
	void sketcher(int)
	{
		for (;;) {
			int32_t k, want;
			{	// stay at most n_seed + 1 batches ahead of the seeders
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return rc_all != 0 || n_created - next_seed <= S.n_seed; });
				if (rc_all != 0) return;
			}
			{	// (a claim may be a round trip to another process: outside the pipeline's lock)
				want = F.claim();
				std::lock_guard<std::mutex> g(mu);
				if (want < 0 || want >= S.n_batches) { exhausted = true, n_total = n_created; cv.notify_all(); return; }   // the job has no batch left
				// (a claim function that hands a batch out twice -- a counter that was not reset, a wrong job key -- would run the
				// slots, results[] and order[] past the caller's arrays: an error, not heap corruption)
				if (n_created >= S.n_batches || taken[(size_t)want]) {
					if (rc_all == 0) rc_all = S.rc_bad_claim, err = "mpa_map_batches_claim: claim() returned batch " + std::to_string(want) + " twice (or more batches than the job has)";
					exhausted = true, n_total = n_created; cv.notify_all(); return;
				}
				taken[(size_t)want] = 1;
				k = n_created;
				slot[(size_t)k].g = want, slot[(size_t)k].j = n_claimed;
				++n_created, ++n_claimed;
			}
			const int rc = F.sketch(k, want);
			if (rc != 0) { fail(rc, F.last_error()); return; }
			std::lock_guard<std::mutex> g(mu);
			slot[k].sketched = true;
			cv.notify_all();
		}
	}
	void seeder(int sd)
	{
		for (;;) {
			int32_t k;
			{	// a free seeder takes the next sketched batch in input order; its result lives in a holder until the batch is planned:
				// wait for the batch that had this holder before
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return rc_all != 0 || (next_seed < n_created && slot[next_seed].sketched) || (exhausted && next_seed >= n_total); });
				if (rc_all != 0 || !(next_seed < n_created && slot[next_seed].sketched)) return;
				k = next_seed++;
				cv.notify_all();                                      // (the sketcher may go one further)
				cv.wait(g, [&] { return rc_all != 0 || k < n_seed_ctx || slot[k - n_seed_ctx].begun; });
				if (rc_all != 0) return;
			}
			const int rc = F.seed(sd, k, k % n_seed_ctx);
			if (rc != 0) { fail(rc, F.last_error()); return; }
			std::lock_guard<std::mutex> g(mu);
			slot[k].seeded = true;
			cv.notify_all();
		}
	}
	void planner(int pl)
	{
		for (;;) {
			int32_t k;
			{	// stay a bounded number of batches ahead of the ones in their DP rounds (planned batches hold their windows and tasks)
				std::unique_lock<std::mutex> g(mu);
				if (next_plan >= n_total) return;
				k = next_plan++;
				cv.wait(g, [&] { return rc_all != 0 || k >= n_total || (slot[k].seeded && k <= n_dp_done + S.n_lanes + S.n_plan - 1); });
				if (rc_all != 0 || k >= n_total) return;           // (k >= n_total: the job ran out before this slot was claimed)
			}
			F.plan(pl, k);
			std::lock_guard<std::mutex> g(mu);
			slot[k].begun = true, ++n_planned;
			cv.notify_all();
		}
	}
	// a lane that is free takes the next batch in input order (a static deal would leave lanes idle behind a slow batch)
	void dp_lane(int d)
	{
		for (;;) {
			int32_t k;
			{
				std::unique_lock<std::mutex> g(mu);
				if (next_dp >= n_total) return;
				k = next_dp++;
				cv.wait(g, [&] { return rc_all != 0 || k >= n_total || slot[k].begun; });
				if (rc_all != 0 || k >= n_total) return;
			}
			const int rc = F.dp(d, k);
			if (rc != 0) { fail(rc, F.last_error()); return; }
			std::lock_guard<std::mutex> g(mu);
			slot[k].dp_done = true, ++n_dp_done;
			cv.notify_all();
		}
	}
	void finisher(int)
	{
		for (int32_t k = 0; k < (int32_t)slot.size(); ++k) {
			{
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return rc_all != 0 || k >= n_total || slot[k].dp_done; });
				if (k >= n_total || !slot[k].dp_done) return;
			}
			F.finish(k, slot[k].g, slot[k].j);                   // (batches finish in slot order)
		}
	}
};

static inline void run_stream(const StreamShape &shape, const StreamStages &stages, StreamResult &out) { Stream(shape, stages).run(out); }

} // namespace mpa
