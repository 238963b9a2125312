// dpresults_check.cpp -- the result stages of a DP round (miniprot_amd/csrc/dp_results_core.h) against the host loop they replace, as a
// stand-alone program for AddressSanitizer and UBSan (tests/test_dp_results_cpu.py compiles it together with dp_plan.cpp and runs it).
// Random tables with made-up kernel outputs go through the stages with a team of one and with a team of 256 threads (a barrier and a
// shared array stand in for the workgroup's LDS); every output sits in a heap block of exactly the bound the driver sizes it by
// (ResLayout, dp_exec.hip): n_glob offsets, n offsets by call, one block sum per team-sized block of traceback calls plus one, the
// header, n records -- so a write past a bound is a heap overflow the sanitizer reports.  The bounds reduction's shared code is compared
// with dp_plan_prep_bound.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <thread>
#include <vector>
#include <pthread.h>
#include "dp_plan.h"
#include "dp_results_core.h"

using namespace mpa;

static int n_bad = 0, n_tables = 0;

// a team of W host threads
struct TeamThreads {
	static const int W = 256;
	struct Shared { pthread_barrier_t bar; int64_t v[W][DPP_NSUM]; };
	Shared *sh;
	int r;
	int rank() const { return r; }
	void sync() const { pthread_barrier_wait(&sh->bar); }
	template<int K> void exscan(DpVec<K> &v, DpVec<K> &total) const
	{
		sync();                                                  // (the previous scan's values have been read)
		for (int k = 0; k < K; ++k) sh->v[r][k] = v.v[k];
		sync();
		for (int k = 0; k < K; ++k) {
			int64_t before = 0, tot = 0;
			for (int w = 0; w < W; ++w) { before += w < r ? sh->v[w][k] : 0; tot += sh->v[w][k]; }
			v.v[k] = before, total.v[k] = tot;
		}
	}
};

static void run_threads(const DpResDev &R)
{
	auto sh = std::make_unique<TeamThreads::Shared>();
	pthread_barrier_init(&sh->bar, nullptr, TeamThreads::W);
	R.head[DPR_H_POOL] = R.head[DPR_H_BAD] = 0;
	const int64_t nb = dp_blocks(R.n_glob, TeamThreads::W), nc = dp_blocks(R.n, TeamThreads::W);
	std::vector<std::thread> th;
	for (int r = 0; r < TeamThreads::W; ++r)
		th.emplace_back([&, r] {
			const TeamThreads tm{ sh.get(), r };
			for (int64_t b = 0; b < nb; ++b) dpr_sums(tm, R, b);
			tm.sync();
			dpr_mid(tm, R);
			tm.sync();
			for (int64_t b = 0; b < nb; ++b) {
				// (a member behind the list's end leaves dpr_offsets behind the scan, like a lane of the workgroup)
				dpr_offsets(tm, R, b);
			}
			tm.sync();
			for (int64_t b = 0; b < nc; ++b) dpr_records(tm, R, b);
		});
	for (auto &t : th) t.join();
	pthread_barrier_destroy(&sh->bar);
}

static void check(const char *what, std::mt19937_64 &rng, size_t n, int ext_of_16, int32_t nc_max, bool threads)
{
	std::vector<mpa_dp_task_t> tasks(n);
	std::vector<ExtOut> eo(n);
	std::vector<int32_t> sc(n), nc(n), gids;
	for (size_t k = 0; k < n; ++k) {
		mpa_dp_task_t &t = tasks[k];
		memset(&t, 0, sizeof(t));
		const bool ext = (int)(rng() % 16) < ext_of_16;
		t.nl = (int32_t)(rng() % 2500), t.al = 1 + (int32_t)(rng() % 1100), t.flag = ext ? (rng() & 1 ? MPA_F_EXT_LEFT : MPA_F_EXT_RIGHT) : MPA_F_CIGAR;
		eo[k] = ExtOut{ (int32_t)(rng() % 100000), (int32_t)(rng() % 30000), (int32_t)(rng() % 200000) - 100000, (int32_t)(rng() % 4) };
		sc[k] = (int32_t)(rng() % 200000) - 100000, nc[k] = rng() % 5 == 0 ? 0 : (int32_t)(rng() % (uint64_t)nc_max);
		if (!ext) gids.push_back((int32_t)k);
	}
	for (size_t k = gids.size(); k > 1; --k) std::swap(gids[k - 1], gids[rng() % k]);
	const size_t n_glob = gids.size();
	// the host loop as dp_assemble() had it before the shared rule
	std::vector<mpa_dp_rst_t> want(n);
	std::vector<int64_t> dense_off(n_glob), off_of(n, 0);
	int64_t pool_n = 0;
	for (size_t g = 0; g < n_glob; ++g) dense_off[g] = pool_n, pool_n += nc[gids[g]];
	for (size_t g = 0; g < n_glob; ++g) off_of[gids[g]] = dense_off[g];
	for (size_t k = 0; k < n; ++k) {
		const mpa_dp_task_t &t = tasks[k];
		mpa_dp_rst_t &o = want[k];
		if ((t.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) && t.nl < 3) o.nt_len = 0, o.aa_len = t.al + 1, o.score = INT32_MIN, o.n_cigar = 0, o.cigar_off = 0;   // (no row to sweep: mpamd.h)
		else if (t.flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT)) o.nt_len = eo[k].nt_len, o.aa_len = eo[k].aa_len, o.score = eo[k].score, o.n_cigar = 0, o.cigar_off = 0;
		else o.nt_len = t.nl, o.aa_len = t.al, o.score = sc[k], o.n_cigar = nc[k], o.cigar_off = off_of[k];
	}
	// the stages, every output in a block of exactly its bound
	std::vector<DTask> dt(n);
	for (size_t k = 0; k < n; ++k) dt[k] = DTask(), dt[k].flag = tasks[k].flag, dt[k].nl = tasks[k].nl, dt[k].al = tasks[k].al, dt[k].cig_cap = nc_max;
	const int w = threads ? TeamThreads::W : TeamOne::W;
	std::unique_ptr<int64_t[]> off(new int64_t[n_glob]), call_off(new int64_t[n]), bsum(new int64_t[(size_t)dp_blocks((int64_t)n_glob, w) + 1]), head(new int64_t[DPR_NHEAD]);
	std::unique_ptr<mpa_dp_rst_t[]> rst(new mpa_dp_rst_t[n]);
	std::unique_ptr<int32_t[]> g_exact(new int32_t[n_glob]);
	for (size_t g = 0; g < n_glob; ++g) g_exact[g] = gids[g];
	memset(rst.get(), 0xee, sizeof(mpa_dp_rst_t) * n);
	DpResDev R;
	R.n = (int64_t)n, R.n_glob = (int64_t)n_glob, R.tasks = dt.data(), R.gids = g_exact.get(), R.eo = eo.data(), R.sc = sc.data(), R.nc = nc.data();
	R.off = off.get(), R.call_off = call_off.get(), R.bsum = bsum.get(), R.head = head.get(), R.rst = rst.get();
	if (threads) run_threads(R); else dp_results_model(R);
	++n_tables;
	if (memcmp(rst.get(), want.data(), sizeof(mpa_dp_rst_t) * n)) { size_t k = 0; while (!memcmp(&rst[k], &want[k], sizeof(mpa_dp_rst_t))) ++k; printf("%s: record %zu of %zu differs\n", what, k, n), ++n_bad; }
	if (head[DPR_H_POOL] != pool_n) printf("%s: %ld words in the pool, the host loop has %ld\n", what, (long)head[DPR_H_POOL], (long)pool_n), ++n_bad;
	if (head[DPR_H_BAD]) printf("%s: a word count flagged as outside its slot\n", what), ++n_bad;
	for (size_t g = 0; g < n_glob; ++g) if (off[g] != dense_off[g]) { printf("%s: offset %zu differs\n", what, g), ++n_bad; break; }
	// the bounds
	int64_t max_nl = 0, max_al = 0;
	const int64_t prep = dp_plan_prep_bound(tasks.data(), (int64_t)n, &max_nl, &max_al);
	const DpTaskBounds b = dp_task_bounds(tasks.data(), (int64_t)n);
	if (b.prep != prep || b.max_nl != max_nl || b.max_al != max_al) printf("%s: bounds (%ld, %ld, %ld), dp_plan_prep_bound has (%ld, %ld, %ld)\n", what, (long)b.prep, (long)b.max_nl, (long)b.max_al, (long)prep, (long)max_nl, (long)max_al), ++n_bad;
}

int main()
{
	std::mt19937_64 rng(20262);
	const size_t edge[10] = { 1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025 };
	for (int round = 0; round < 60; ++round) {
		const size_t n = round < 10 ? edge[round] : 1 + (size_t)(rng() % 4000);
		const int ext_of_16 = round % 7 == 3 ? 16 : round % 7 == 4 || round < 10 ? 0 : 8;       // only extension calls; only traceback calls (the edges count them); mixed
		char what[80];
		snprintf(what, sizeof(what), "table %d (%zu calls), team of one", round, n);
		check(what, rng, n, ext_of_16, 3600, false);
	}
	for (int round = 0; round < 14; ++round) {
		const size_t n = round < 10 ? edge[round] : 1 + (size_t)(rng() % 1500);
		char what[80];
		snprintf(what, sizeof(what), "table %d (%zu calls), team of 256 threads", round, n);
		check(what, rng, n, round == 10 ? 16 : round < 10 ? 0 : 8, 3600, true);
	}
	check("a pool of more than 2^31 words, team of one", rng, 7, 0, 0x7fffffff, false);
	check("a pool of more than 2^31 words, team of 256 threads", rng, 7, 0, 0x7fffffff, true);
	// the prep chunk's edges
	{
		const int32_t nls[7] = { 0, 1, 1023, 1024, 1025, -3, 2048 };
		std::vector<mpa_dp_task_t> t(7);
		memset(t.data(), 0, sizeof(mpa_dp_task_t) * 7);
		for (int k = 0; k < 7; ++k) t[k].nl = nls[k], t[k].al = k == 5 ? -1 : 10 * k;
		int64_t a = 0, b = 0;
		const int64_t prep = dp_plan_prep_bound(t.data(), 7, &a, &b);
		const DpTaskBounds bd = dp_task_bounds(t.data(), 7);
		if (prep != 7 || bd.prep != prep || bd.max_nl != a || bd.max_al != b) printf("prep chunk edges: (%ld, %ld, %ld) against (%ld, %ld, %ld)\n", (long)bd.prep, (long)bd.max_nl, (long)bd.max_al, (long)prep, (long)a, (long)b), ++n_bad;
	}
	printf("%d tables, %d mismatches\n", n_tables, n_bad);
	return n_bad != 0;
}
