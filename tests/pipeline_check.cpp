// pipeline_check.cpp -- the scheduler of the stream pipeline (miniprot_amd/csrc/host_pipeline.h) against stub stages, stand-alone: built
// by tests/test_pipeline_cpu.py under ThreadSanitizer and under AddressSanitizer + UBSan.  Every stub sleeps 0-200 us and appends to
// an event log; after every run the log is checked against what the scheduler's waits promise (the numbered checks in check_run).
// Jobs: in input order, shuffled claims, an early end (none claimed included), a repeated or surplus claim, an error code or a
// std::runtime_error from a stage at a random slot.  Shapes: lanes 1..8, seeders 1..4, planners 1..6 (the corners always), 0..20 batches.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include "host_pipeline.h"

using namespace mpa;

enum { RC_BAD_CLAIM = -2, RC_EXCEPTION = -5, RC_STAGE = -10 };   // RC_STAGE - stage: what a stub returns
enum Kind { IN_ORDER = 0, SHUFFLED, EARLY_END, BAD_CLAIM, STAGE_ERROR, STAGE_THROW, N_KIND };
static const char *const kStageName[5] = { "sketch stage", "seeding stage", "planning stage", "DP lane", "output stage" };

struct Event { int stage, end, who; int32_t k, g, j; };   // end: 0 = the callback began, 1 = it returned

struct Job {
	StreamShape shape;
	Kind kind;
	std::vector<int32_t> claims;       // what claim() hands out, then -1 for ever
	int fail_stage = -1;               // STAGE_ERROR / STAGE_THROW: where
	int32_t fail_slot = -1;
};

static thread_local std::string tl_err;
static thread_local std::mt19937 tl_rng;
static std::atomic<uint32_t> g_thread_seed{ 1 };
static long g_bad = 0;
static void bad(const Job &J, const char *what, long a = 0, long b = 0)
{
	++g_bad;
	fprintf(stderr, "VIOLATION (%d batches, %d lanes, %d seeders, %d planners, kind %d, fail %d@%d): %s [%ld %ld]\n", J.shape.n_batches, J.shape.n_lanes, J.shape.n_seed,
	        J.shape.n_plan, (int)J.kind, J.fail_stage, J.fail_slot, what, a, b);
}

struct Run {
	const Job &J;
	std::mutex mu;                     // the log's own lock
	std::vector<Event> log;
	std::atomic<int> inside[5][8];     // callbacks of stage s, thread i that are running
	std::atomic<int> threads_in{ 0 }, threads_out{ 0 }, twice{ 0 }, ahead_max{ 0 };
	size_t n_claim_calls = 0;          // (the sketcher's thread only)
	Stream *stream = nullptr;

	explicit Run(const Job &j) : J(j) { for (auto &s : inside) for (auto &x : s) x = 0; }
	void note(int stage, int end, int who, int32_t k, int32_t g = -1, int32_t j = -1) { std::lock_guard<std::mutex> l(mu); log.push_back(Event{ stage, end, who, k, g, j }); }
	// the body of every stub: begin, sleep, fail if this is the place, end
	int stub(int stage, int who, int32_t k, int32_t g = -1, int32_t j = -1)
	{
		struct In { std::atomic<int> &n; std::atomic<int> &twice; In(std::atomic<int> &n_, std::atomic<int> &t) : n(n_), twice(t) { if (n.fetch_add(1) != 0) ++twice; } ~In() { --n; } };
		In in(inside[stage][who], twice);
		note(stage, 0, who, k, g, j);
		std::this_thread::sleep_for(std::chrono::microseconds(tl_rng() % 201));
		if (stage == J.fail_stage && k == J.fail_slot) {
			if (J.kind == STAGE_THROW) throw std::runtime_error("boom at slot " + std::to_string(k));
			tl_err = "stub stage " + std::to_string(stage) + " failed at slot " + std::to_string(k);
			return RC_STAGE - stage;
		}
		note(stage, 1, who, k, g, j);
		return 0;
	}
	void go(StreamResult &res)
	{
		StreamStages F;
		F.claim = [&]() -> int32_t {
			const int a = stream->sketched_ahead();
			if (a > ahead_max) ahead_max = a;
			return n_claim_calls < J.claims.size() ? J.claims[n_claim_calls++] : -1;
		};
		F.sketch = [&](int32_t k, int32_t g) { return stub(STREAM_SKETCH, 0, k, g); };
		F.seed = [&](int sd, int32_t k, int h) { return stub(STREAM_SEED, sd, k, -1, h); };
		F.plan = [&](int pl, int32_t k) { (void)stub(STREAM_PLAN, pl, k); };
		F.dp = [&](int d, int32_t k) { return stub(STREAM_DP, d, k); };
		F.finish = [&](int32_t k, int32_t g, int32_t j) { (void)stub(STREAM_FINISH, 0, k, g, j); };
		F.thread = [&](StreamStage, int, const std::function<void()> &loop) {
			struct Count { std::atomic<int> &out; ~Count() { ++out; } } c{ threads_out };
			++threads_in;
			tl_rng.seed(g_thread_seed++);
			loop();
		};
		F.last_error = [] { return tl_err; };
		Stream s(J.shape, F);
		stream = &s;
		s.run(res);
	}
};

static void check_run(const Job &J, Run &R, const StreamResult &res)
{
	const StreamShape &S = J.shape;
	const int32_t n = S.n_batches, m = (int32_t)(J.kind == BAD_CLAIM ? J.claims.size() - 1 : J.claims.size());   // m: batches claimed in good order
	const int n_ctx = S.n_seed + S.n_plan;
	const bool fails = J.kind == BAD_CLAIM || J.kind == STAGE_ERROR || J.kind == STAGE_THROW;
	// every thread was started, has left and is joined (run() returned and the count of wrappers left equals those entered)
	if (R.threads_in != 2 + S.n_seed + S.n_plan + S.n_lanes || R.threads_out != R.threads_in) bad(J, "stage threads started / left", R.threads_in, R.threads_out);
	// 6. no seeder, planner or lane index inside its callback twice at once
	if (R.twice != 0) bad(J, "6: a stage thread's callback ran twice at once", R.twice);
	// 4. at a claim, slots created but not taken by a seeder <= n_seed
	if (R.ahead_max > S.n_seed) bad(J, "4: the sketcher ran ahead of the seeders", R.ahead_max, S.n_seed);
	// where each event of each slot is in the log
	std::vector<std::vector<long>> at((size_t)n, std::vector<long>(10, -1));
	long n_dp_end = 0, last_finish = -1;
	for (long i = 0; i < (long)R.log.size(); ++i) {
		const Event &e = R.log[(size_t)i];
		if (e.k < 0 || e.k >= m) { bad(J, "1: a slot that was never claimed", e.k, e.stage); continue; }
		long &x = at[(size_t)e.k][(size_t)(2 * e.stage + e.end)];
		if (x >= 0) bad(J, "1: a stage ran twice for one slot", e.k, e.stage);
		x = i;
		if (e.end) { if (e.stage == STREAM_DP) ++n_dp_end; continue; }
		const std::vector<long> &a = at[(size_t)e.k];
		// 1. ... in that order: a stage begins after the one before it has returned
		if (e.stage > 0 && a[(size_t)(2 * e.stage - 1)] < 0) bad(J, "1: a stage began before the one before it ended", e.k, e.stage);
		if ((e.stage == STREAM_SKETCH || e.stage == STREAM_FINISH) && e.g != J.claims[(size_t)e.k]) bad(J, "1/2: the slot's batch is not the one claimed", e.k, e.g);
		// 3. the seed of slot k begins after the plan of slot k - (n_seed + n_plan) has ended: one batch per holder
		if (e.stage == STREAM_SEED) {
			if (e.j != e.k % n_ctx) bad(J, "3: holder index", e.k, e.j);
			if (e.k >= n_ctx && at[(size_t)(e.k - n_ctx)][2 * STREAM_PLAN + 1] < 0) bad(J, "3: seeding began while the holder's last batch was not planned", e.k);
		}
		// 5. the plan of slot k begins only when k <= DP rounds finished + n_lanes + n_plan - 1
		if (e.stage == STREAM_PLAN && e.k > n_dp_end + S.n_lanes + S.n_plan - 1) bad(J, "5: the planner ran ahead of the DP lanes", e.k, n_dp_end);
		// 2. finish in slot order, ordinal = claim order
		if (e.stage == STREAM_FINISH) {
			if (e.k != last_finish + 1 || (e.k > 0 && at[(size_t)(e.k - 1)][2 * STREAM_FINISH + 1] < 0)) bad(J, "2: finish out of slot order", e.k, last_finish);
			if (e.j != e.k) bad(J, "2: ordinal is not the claim order", e.k, e.j);
			last_finish = e.k;
		}
	}
	if (!fails) {
		// 1. every claimed batch through all five stages; 2. / 7. n_mapped, order[], no error (an early end and an empty job included)
		for (int32_t k = 0; k < m; ++k) for (int x = 0; x < 10; ++x) if (at[(size_t)k][(size_t)x] < 0) bad(J, "1: a claimed batch missed a stage", k, x);
		if (res.rc != 0 || !res.err.empty()) bad(J, "7: an error where none was made", res.rc);
		if (res.n_mapped != m || (int32_t)res.order.size() != m) bad(J, "2/7: n_mapped", res.n_mapped, m);
		else for (int32_t j = 0; j < m; ++j) if (res.order[(size_t)j] != J.claims[(size_t)j]) bad(J, "2: order[]", j, res.order[(size_t)j]);
		if (R.n_claim_calls != (size_t)m) bad(J, "claims made", (long)R.n_claim_calls, m);
		return;
	}
	// 8. / 9. the first (here: the only) error comes back with its message, nothing else does
	std::string want;
	int want_rc;
	if (J.kind == BAD_CLAIM) want_rc = RC_BAD_CLAIM, want = "mpa_map_batches_claim: claim() returned batch " + std::to_string(J.claims.back()) + " twice (or more batches than the job has)";
	else if (J.kind == STAGE_ERROR) want_rc = RC_STAGE - J.fail_stage, want = "stub stage " + std::to_string(J.fail_stage) + " failed at slot " + std::to_string(J.fail_slot);
	else want_rc = RC_EXCEPTION, want = std::string(kStageName[J.fail_stage]) + ": boom at slot " + std::to_string(J.fail_slot);
	if (res.rc != want_rc) bad(J, "8/9: error code", res.rc, want_rc);
	if (res.err != want) { bad(J, "8/9: message"); fprintf(stderr, "  got  '%s'\n  want '%s'\n", res.err.c_str(), want.c_str()); }
	if (res.n_mapped != 0 || !res.order.empty()) bad(J, "8/9: a result left behind", res.n_mapped);
}

int main()
{
	std::mt19937 rng(20240611);
	long n_runs = 0;
	const auto t0 = std::chrono::steady_clock::now();
	auto one = [&](int32_t n, int lanes, int seeders, int planners, Kind kind, int stage_of_5) {
		Job J;
		J.shape = StreamShape{ n, lanes, seeders, planners, RC_BAD_CLAIM, RC_EXCEPTION };
		J.kind = kind;
		std::vector<int32_t> all((size_t)n);
		for (int32_t i = 0; i < n; ++i) all[(size_t)i] = i;
		if (kind != IN_ORDER) std::shuffle(all.begin(), all.end(), rng);
		if (n == 0 && kind != IN_ORDER) J.kind = kind = EARLY_END;        // (nothing to repeat, nowhere to fail)
		if (kind == EARLY_END) all.resize(n ? rng() % (uint32_t)n : 0);       // m < n, none included
		if (kind == BAD_CLAIM) {                                              // some claims, then one of them again (after all n: a surplus claim)
			all.resize(1 + rng() % (uint32_t)n);
			all.push_back(all[rng() % all.size()]);
		}
		J.claims = all;
		if (kind == STAGE_ERROR) { static const int st[3] = { STREAM_SKETCH, STREAM_SEED, STREAM_DP }; J.fail_stage = st[stage_of_5 % 3]; }
		if (kind == STAGE_THROW) J.fail_stage = stage_of_5 % 5;
		if (J.fail_stage >= 0) J.fail_slot = (int32_t)(rng() % (uint32_t)n);
		Run R(J);
		StreamResult res;
		R.go(res);
		check_run(J, R, res);
		++n_runs;
	};
	// the corners with every kind of job, every failing stage and the smallest and largest jobs
	static const int corner[2][3] = { { 1, 1, 1 }, { 8, 4, 6 } };
	for (const auto &c : corner)
		for (int32_t n : { 0, 1, 2, 9, 20 })
			for (int kind = 0; kind < N_KIND; ++kind)
				for (int st = 0; st < (kind == STAGE_ERROR ? 3 : kind == STAGE_THROW ? 5 : 1); ++st) one(n, c[0], c[1], c[2], (Kind)kind, st);
	for (int i = 0; i < 300; ++i)
		one((int32_t)(rng() % 21), 1 + (int)(rng() % 8), 1 + (int)(rng() % 4), 1 + (int)(rng() % 6), (Kind)(rng() % N_KIND), (int)(rng() % 15));
	const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	printf("%ld runs in %.1f s, %ld violations\n", n_runs, sec, g_bad);
	return g_bad == 0 ? 0 : 1;
}
