// dpsplit_check.cpp -- the 2048- and 3072-column extension classes (X_SPLIT8, X_SPLIT12; DpPlanKnobs::split_wide) through the host planner
// and through the stages of the device planner (miniprot_amd/csrc/dp_plan_core.h), as a stand-alone program for AddressSanitizer and
// UBSan (tests/test_dp_split_wide_cpu.py compiles it together with dp_plan.cpp and runs it).  The stages run with a team of one and with
// a team of 256 threads (a barrier and a shared array stand in for the workgroup's LDS); every pool they write sits in a heap block of
// exactly the bound the driver sizes it by (dev_dp_plan_run, dp_exec.hip) -- n tasks, the prep-chunk bound + 1, n + 16 wave
// descriptors, n list entries, traceback waves and walk entries, dp_units_bound(n, split_wide) units and unit keys -- so a write past a
// bound is a heap overflow the sanitizer reports.  The serialised plans (with the five words of the *_wide hooks) must be equal byte
// for byte; what the planner's own numbers promise is checked on the host plan: n_bound, the units of every split group, the row-key
// slots of the wide groups.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <thread>
#include <vector>
#include <pthread.h>
#include "dp_plan.h"

using namespace mpa;

static const int64_t kCtg[3] = { 6000, 9000, 4000 };
static const int64_t kQ[5] = { 0, 3100, 3800, 4100, 6800 };       // query lengths 3100, 700, 300, 2700
static int n_bad = 0, n_planned = 0, n_declined = 0;

// max_mat: the largest matrix entry (11: the guard stops near 2 660 residues; 4: every width up to 3 072 columns is admitted)
static mpa_dpopt_t options(int max_mat)
{
	mpa_dpopt_t o;
	memset(&o, 0, sizeof(o));
	o.go = 11, o.ge = 1, o.fs = 23, o.xdrop = 100, o.end_bonus = 5, o.ie_coef = 0.5f;
	for (int k = 0; k < 484; ++k) o.mat[k] = (int8_t)(k % 23 == 0 ? max_mat : -(k % 5));
	return o;
}

static mpa_dp_task_t call(std::mt19937_64 &rng, bool ext, int32_t al, int32_t nl)
{
	auto below = [&rng](int64_t n) { return (int64_t)(rng() % (uint64_t)n); };
	mpa_dp_task_t t;
	memset(&t, 0, sizeof(t));
	int32_t qid;
	do qid = (int32_t)below(4); while (kQ[qid + 1] - kQ[qid] < al);
	const int32_t cid = (int32_t)below(3);
	t.nl = nl, t.al = al, t.qid = qid, t.aa_off = (int32_t)below(kQ[qid + 1] - kQ[qid] - al + 1);
	t.vid = 2 * cid + (int32_t)below(2), t.nt_off = below(kCtg[cid] - nl + 1);
	t.flag = ext ? (below(2) ? MPA_F_EXT_LEFT : MPA_F_EXT_RIGHT) : MPA_F_CIGAR, t.io = 10 + (int32_t)below(31), t.tag = 0;
	return t;
}

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
	void add(int64_t *dst, int64_t v) const { __atomic_fetch_add(dst, v, __ATOMIC_RELAXED); }
	void flag(int64_t *dst, int64_t bits) const { __atomic_fetch_or(dst, bits, __ATOMIC_RELAXED); }
};

// the stages in the driver's order, the two sorts by the team's first member
template<typename Team> static void stages(const Team &tm, DpDevPlan &D)
{
	const int64_t nb = dp_blocks(D.n, Team::W), nu = dp_blocks(D.n_ubound, Team::W);
	for (int64_t b = 0; b < nb; ++b) dpp_classify(tm, D, b);
	tm.sync();
	if (tm.rank() == 0) std::copy(D.key, D.key + D.n, D.skey), std::sort(D.skey, D.skey + D.n);
	tm.sync();
	for (int64_t b = 0; b < nb; ++b) dpp_sums(tm, D, b);
	tm.sync();
	dpp_mid(tm, D);
	tm.sync();
	for (int64_t b = 0; b < nb; ++b) dpp_layout(tm, D, b);
	tm.sync();
	for (int64_t b = 0; b < nu; ++b) dpp_units(tm, D, b);
	tm.sync();
	if (tm.rank() == 0) std::copy(D.ukey, D.ukey + D.n_ubound, D.uskey), std::sort(D.uskey, D.uskey + D.n_ubound);
	tm.sync();
	for (int64_t b = 0; b < dp_blocks(D.head->n_units, Team::W); ++b) dpp_units_out(tm, D, b);
}

// the stages on pools of exactly the driver's bounds; the plan and its units as dp_plan_model leaves them
static int run_stages(const std::vector<mpa_dp_task_t> &in, const mpa_qbatch_t &q, const mpa_dpopt_t &opt, const DpPlanKnobs &kn, bool threads, DpPlan &P, std::vector<DpUnit> &units)
{
	const int64_t n = (int64_t)in.size();
	P = DpPlan();
	if (dp_plan_device_declines(&opt, kn, n)) { P.rc = MPA_ERR_UNSUPPORTED; return P.rc; }
	int64_t max_nl = 0, max_al = 0;
	const int64_t prep_bound = dp_plan_prep_bound(in.data(), n, &max_nl, &max_al);
	if (!dp_unit_costs_fit(max_nl, max_al)) { P.rc = MPA_ERR_UNSUPPORTED; return P.rc; }
	const size_t N = (size_t)n, U = (size_t)dp_units_bound(n, kn.split_wide != 0), nb = (size_t)dp_blocks(n, threads ? TeamThreads::W : 1);
	std::unique_ptr<DTask[]> tasks(new DTask[N]);
	std::unique_ptr<PrepChunk[]> chunks(new PrepChunk[(size_t)prep_bound + 1]);
	std::unique_ptr<ExtWave[]> waves(new ExtWave[N + 16]);
	std::unique_ptr<int32_t[]> list(new int32_t[N]), wlist(new int32_t[N]), gids(new int32_t[N]);
	std::unique_ptr<GlobWave[]> gw(new GlobWave[N]);
	std::unique_ptr<DpUnit[]> out(new DpUnit[U]), ubuf(new DpUnit[U]);
	std::unique_ptr<uint64_t[]> key(new uint64_t[N]), skey(new uint64_t[N]), ukey(new uint64_t[U]), uskey(new uint64_t[U]);
	std::unique_ptr<DpSums[]> bsum(new DpSums[nb]);
	std::unique_ptr<DpDevHead> H(new DpDevHead);
	memset(H.get(), 0, sizeof(DpDevHead));
	DpDevPlan D;
	D.n = n, D.n_ubound = (int64_t)U, D.n_ctg = 3, D.n_seq = q.n_seq, D.opt = dp_plan_opt(&opt), D.kn = kn, D.raw = in.data(), D.q_off = q.q_off, D.ctg_len = kCtg;
	D.tasks = tasks.get(), D.chunks = chunks.get(), D.waves = waves.get(), D.list = list.get(), D.gw = gw.get(), D.units = out.get(), D.wlist = wlist.get();
	D.key = key.get(), D.skey = skey.get(), D.bsum = bsum.get(), D.ubuf = ubuf.get(), D.ukey = ukey.get(), D.uskey = uskey.get(), D.gids = gids.get(), D.head = H.get();
	if (threads) {
		auto sh = std::make_unique<TeamThreads::Shared>();
		pthread_barrier_init(&sh->bar, nullptr, TeamThreads::W);
		std::vector<std::thread> th;
		for (int r = 0; r < TeamThreads::W; ++r) th.emplace_back([&, r] { const TeamThreads tm{ sh.get(), r }; stages(tm, D); });
		for (auto &t : th) t.join();
		pthread_barrier_destroy(&sh->bar);
	} else stages(TeamOne(), D);
	if (dp_plan_from_head(*H, gids.get(), &q, &opt, kn, 640, P)) return P.rc;
	P.tasks.assign(tasks.get(), tasks.get() + N), P.prep.assign(chunks.get(), chunks.get() + H->n_prep), P.ewaves.assign(waves.get(), waves.get() + H->n_ewaves);
	if (!P.chunks.empty()) P.chunks[0].list.assign(list.get(), list.get() + H->n_reg_glob), P.chunks[0].waves.assign(gw.get(), gw.get() + H->n_gw);
	units.assign(out.get(), out.get() + H->n_units);
	return MPA_OK;
}

// what the numbers of a host plan promise the executor and the kernel
static void check_numbers(const char *what, const DpPlan &P, const std::vector<DpUnit> &units)
{
	const int64_t n8 = P.ext_wide[0].cnt, n12 = P.ext_wide[1].cnt, n4 = P.ext[X_SPLIT4].cnt, n2 = P.ext[X_SPLIT2].cnt;
	if (P.n_split != n8 + n12 + n4 + n2 || P.n_bound != 7 * n8 + 11 * n12 + 3 * n4 + n2) printf("%s: n_split %ld, n_bound %ld\n", what, (long)P.n_split, (long)P.n_bound), ++n_bad;
	if (P.xg_bytes != (size_t)P.n_bound * (size_t)P.key_stride * 16 || P.xg_tail != (2 * (size_t)P.n_split + 1) * 4) printf("%s: xg bytes\n", what), ++n_bad;
	// wide groups are neighbours from the first X_W2 descriptor: the row-key slot of a group is its descriptor minus that
	const int first_wide = P.ext[X_W2].first;
	int64_t end_wide = first_wide;
	for (int cls = X_W2; cls <= X_SPLIT4; ++cls) end_wide += P.ext[cls].cnt;
	if (n8 && P.ext_wide[0].first != end_wide) printf("%s: X_SPLIT8 descriptors are not behind X_SPLIT4's\n", what), ++n_bad;
	end_wide += n8;
	if (n12 && P.ext_wide[1].first != end_wide) printf("%s: X_SPLIT12 descriptors are not behind X_SPLIT8's\n", what), ++n_bad;
	end_wide += n12;
	if (end_wide - first_wide != P.n_wide_groups) printf("%s: %ld wide groups, %ld descriptors\n", what, (long)P.n_wide_groups, (long)(end_wide - first_wide)), ++n_bad;
	// every split group: n_blk units, blocks 0 .. n_blk - 1, one group number, n_blk - 1 boundaries of its own
	std::vector<int> seen_group((size_t)P.n_split, 0), seen_bound((size_t)P.n_bound, 0);
	std::vector<std::vector<int>> blocks(P.ewaves.size());
	for (const DpUnit &u : units) {
		if (u.kind != U_EXT_SPLIT) continue;
		const int cls = P.tasks[P.ewaves[u.first].task[0]].cls;
		if (u.n_blk != dp_ext_unit_blocks(cls) || u.blk < 0 || u.blk >= u.n_blk || u.sgroup < 0 || u.sgroup >= P.n_split || u.xg_first < 0 || u.xg_first + u.n_blk - 1 > P.n_bound) {
			printf("%s: a unit of descriptor %d: blk %d of %d, group %d, boundary %d\n", what, u.first, u.blk, u.n_blk, u.sgroup, u.xg_first), ++n_bad;
			return;
		}
		blocks[u.first].push_back(u.blk);
		if (u.blk == 0) { ++seen_group[u.sgroup]; for (int b = 0; b + 1 < u.n_blk; ++b) ++seen_bound[u.xg_first + b]; }
		if (u.first - first_wide < 0 || u.first - first_wide >= P.n_wide_groups) printf("%s: descriptor %d has no row-key slot\n", what, u.first), ++n_bad;
		for (int h = 0; h < 2; ++h) if (P.ewaves[u.first].task[h] >= 0 && P.tasks[P.ewaves[u.first].task[h]].ncol > 256 * u.n_blk) printf("%s: a call wider than its group\n", what), ++n_bad;
	}
	for (int v : seen_group) if (v != 1) { printf("%s: a split group number used %d times\n", what, v), ++n_bad; break; }
	for (int v : seen_bound) if (v != 1) { printf("%s: a boundary used %d times\n", what, v), ++n_bad; break; }
	for (size_t d = 0; d < blocks.size(); ++d) {
		if (blocks[d].empty()) continue;
		std::vector<int> b = blocks[d];
		std::sort(b.begin(), b.end());
		for (size_t k = 0; k < b.size(); ++k) if (b[k] != (int)k) { printf("%s: descriptor %zu: blocks are not 0 .. n_blk - 1\n", what, d), ++n_bad; break; }
		if ((int)b.size() != dp_ext_unit_blocks(P.tasks[P.ewaves[d].task[0]].cls)) printf("%s: descriptor %zu has %zu units\n", what, d, b.size()), ++n_bad;
	}
	if (sizeof(DpUnit) * units.size() > P.up.off - P.up.units) printf("%s: the staging section holds fewer units than the plan has\n", what), ++n_bad;
}

static void check(const char *what, const std::vector<mpa_dp_task_t> &tasks, const mpa_dpopt_t &opt, const DpPlanKnobs &kn, bool expect_decline)
{
	const mpa_qbatch_t q{ 4, nullptr, kQ };
	DpPlan host;
	if (dp_plan(tasks.data(), (int64_t)tasks.size(), kCtg, sizeof(int64_t), 3, &q, &opt, kn, 640, host)) { printf("%s: the host planner refused: %s\n", what, host.err.c_str()), ++n_bad; return; }
	const int64_t need = dp_plan_serialize(host, kn, nullptr, 0, true);
	std::vector<char> a((size_t)(need > 0 ? need : 0));
	if (need <= 0 || dp_plan_serialize(host, kn, a.data(), need, true) != need) { printf("%s: the host plan does not serialise\n", what), ++n_bad; return; }
	{
		std::vector<DpUnit> hu((host.up.off - host.up.units) / sizeof(DpUnit));
		dp_plan_units(host, kn, hu.data());
		hu.resize(host.n_units);
		check_numbers(what, host, hu);
	}
	for (int threads = 0; threads < 2; ++threads) {
		DpPlan model;
		std::vector<DpUnit> units;
		const int rc = run_stages(tasks, q, opt, kn, threads != 0, model, units);
		if (expect_decline) {
			if (rc != MPA_ERR_UNSUPPORTED) printf("%s: expected a decline, got %d\n", what, rc), ++n_bad;
			++n_declined;
			continue;
		}
		if (rc != MPA_OK) { printf("%s: the stages returned %d (%s)\n", what, rc, model.err.c_str()), ++n_bad; continue; }
		const int64_t got = dp_plan_write(model, units, nullptr, 0, true);
		if (need != got) { printf("%s: %ld bytes from the stages, %ld from the host planner\n", what, (long)got, (long)need), ++n_bad; continue; }
		std::vector<char> b((size_t)need);
		dp_plan_write(model, units, b.data(), need, true);
		if (memcmp(a.data(), b.data(), (size_t)need)) {
			size_t k = 0;
			while (a[k] == b[k]) ++k;
			printf("%s (team of %d): the plans differ first at byte %zu of %ld\n", what, threads ? TeamThreads::W : 1, k, (long)need), ++n_bad;
		}
		++n_planned;
	}
}

int main()
{
	std::mt19937_64 rng(20263);
	const mpa_dpopt_t opt11 = options(11), opt4 = options(4);
	const int32_t widths[10] = { 16, 64, 128, 256, 512, 1024, 1536, 2048, 2600, 3072 }, few[4] = { 3, 384, 1024, 2000 };
	for (int round = 0; round < 16; ++round) {
		const size_t n = round < 6 ? (size_t)round + 1 : 1 + (size_t)(rng() % 1500);
		DpPlanKnobs kn;
		kn.split_wide = round % 5 != 4, kn.lite_min = round % 3 == 0 ? 3 : 384, kn.lite_wide = round % 2, kn.ext_dual = round % 4 != 0, kn.unit_prio = round % 7 != 0;
		const bool low_mat = round % 2 == 1;                           // (3 072 columns need the matrix whose largest entry is 4)
		const int n_w = !kn.split_wide ? 6 : low_mat ? 10 : 9;
		std::vector<mpa_dp_task_t> tasks;
		for (size_t k = 0; k < n; ++k) {
			const bool ext = round % 6 == 3 ? true : rng() % 4 != 0;
			const bool wide = ext && (round < 6 || rng() % 8 == 0);        // (the first tables: wide calls only -- lone calls, pairs, odd counts)
			const int32_t hi = widths[wide ? 6 + rng() % (uint64_t)(n_w > 6 ? n_w - 6 : 1) : rng() % 6];
			const int32_t lo = wide && n_w > 6 ? 1025 : 1;
			const int32_t top = n_w > 6 ? hi : std::min(hi, 1024);
			const int32_t al = ext ? lo + (int32_t)(rng() % (uint64_t)(top - lo + 1)) : 1 + (int32_t)(rng() % 300);
			const int32_t nl = round % 4 == 1 ? few[rng() % 4] : 3 + (int32_t)(rng() % 2498);
			tasks.push_back(call(rng, ext, al, nl));
		}
		char what[64];
		snprintf(what, sizeof(what), "random table %d (%zu calls)", round, n);
		check(what, tasks, low_mat ? opt4 : opt11, kn, false);
	}
	// the edges of the two classes, each width once (empty halves) and twice
	{
		DpPlanKnobs kn;
		kn.split_wide = 1;
		std::vector<mpa_dp_task_t> tasks;
		for (int32_t al : { 1024, 1025, 2040, 2041, 2048, 2049, 3065, 3072 }) for (int k = 0; k < (al % 2 ? 1 : 2); ++k) tasks.push_back(call(rng, true, al, 300 + al % 7));
		check("class edges", tasks, opt4, kn, false);
		std::vector<mpa_dp_task_t> t2 = tasks;
		t2.push_back(call(rng, true, 3073, 300));
		check("3 073 residues: X_HUGE", t2, opt4, kn, true);
		check("past the int16 guard: X_HUGE", tasks, opt11, kn, true);           // (3 072 residues x 11)
		DpPlanKnobs k2 = kn; k2.split_wide = 0; check("knob off: X_HUGE", tasks, opt4, k2, true);
	}
	printf("%d tables planned, %d declined, %d mismatches\n", n_planned, n_declined, n_bad);
	return n_bad != 0;
}
