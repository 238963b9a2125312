// dpplan_check.cpp -- the stages of the device planner of a DP round (miniprot_amd/csrc/dp_plan_core.h) against the host planner, as a
// stand-alone program for AddressSanitizer and UBSan (tests/test_dp_plan_model_cpu.py compiles it together with dp_plan.cpp and runs it).
// dp_plan_model() runs the stages with a team of one and keeps every pool the device planner writes in a heap block of exactly the
// bound the driver sizes it by (dev_dp_plan, dp_exec.hip) -- n tasks, sum of ceil(nl / 1024) + 1 prep chunks, n + 16 wave descriptors,
// n list entries and traceback waves, 4 n + 64 units, n walk entries -- so a write past a bound is a heap overflow the sanitizer
// reports.  Random tables of up to 5 000 calls; the serialised plans must be equal byte for byte.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "dp_plan.h"

using namespace mpa;

static const int64_t kCtg[3] = { 6000, 9000, 4000 };
static const int64_t kQ[5] = { 0, 1200, 1900, 2200, 3350 };       // query lengths 1200, 700, 300, 1150
static int n_bad = 0, n_planned = 0, n_declined = 0;

static mpa_dpopt_t options()
{
	mpa_dpopt_t o;
	memset(&o, 0, sizeof(o));
	o.go = 11, o.ge = 1, o.fs = 23, o.xdrop = 100, o.end_bonus = 5, o.ie_coef = 0.5f;
	for (int k = 0; k < 484; ++k) o.mat[k] = (int8_t)(k % 23 == 0 ? 11 : -(k % 5));
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

// both planners on one table; the plans must serialise alike, or the model must decline where `expect_decline` says so
static void check(const char *what, const std::vector<mpa_dp_task_t> &tasks, const mpa_dpopt_t &opt, const DpPlanKnobs &kn, bool expect_decline)
{
	const mpa_qbatch_t q{ 4, nullptr, kQ };
	DpPlan model;
	std::vector<DpUnit> units;
	const int rc = dp_plan_model(tasks.data(), (int64_t)tasks.size(), kCtg, 3, &q, &opt, kn, 640, model, units);
	if (expect_decline) {
		if (rc != MPA_ERR_UNSUPPORTED) printf("%s: expected a decline, got %d\n", what, rc), ++n_bad;
		++n_declined;
		return;
	}
	if (rc != MPA_OK) { printf("%s: the model returned %d (%s)\n", what, rc, model.err.c_str()), ++n_bad; return; }
	DpPlan host;
	if (dp_plan(tasks.data(), (int64_t)tasks.size(), kCtg, sizeof(int64_t), 3, &q, &opt, kn, 640, host)) { printf("%s: the host planner refused: %s\n", what, host.err.c_str()), ++n_bad; return; }
	const int64_t need = dp_plan_serialize(host, kn, nullptr, 0);
	const int64_t got = dp_plan_write(model, units, nullptr, 0);
	if (need != got || need <= 0) { printf("%s: %ld bytes from the model, %ld from the host planner\n", what, (long)got, (long)need), ++n_bad; return; }
	std::vector<char> a((size_t)need), b((size_t)need);
	dp_plan_serialize(host, kn, a.data(), need), dp_plan_write(model, units, b.data(), need);
	if (memcmp(a.data(), b.data(), (size_t)need)) {
		size_t k = 0;
		while (a[k] == b[k]) ++k;
		printf("%s: the plans differ first at byte %zu of %ld\n", what, k, (long)need), ++n_bad;
	}
	++n_planned;
}

int main()
{
	std::mt19937_64 rng(20261);
	const mpa_dpopt_t opt = options();
	const int32_t widths[8] = { 16, 32, 64, 128, 256, 512, 1024, 1100 }, few[4] = { 3, 384, 1024, 2000 }, edge[4] = { 3, 1023, 1024, 1025 };
	for (int round = 0; round < 60; ++round) {
		const size_t n = round < 8 ? (size_t)round + 1 : 1 + (size_t)(rng() % 5000);
		DpPlanKnobs kn;
		kn.lite_min = round % 3 == 0 ? 3 : 384, kn.lite_wide = round % 2, kn.ext_dual = round % 5 != 0, kn.unit_prio = round % 7 != 0;
		const bool few_rows = round % 4 == 1;                          // (ties: the index decides)
		std::vector<mpa_dp_task_t> tasks;
		for (size_t k = 0; k < n; ++k) {
			const bool ext = round % 11 == 3 ? true : round % 11 == 4 ? false : (rng() & 1) != 0;
			const int32_t hi = widths[rng() % (ext ? 7 : 8)];
			const int32_t al = 1 + (int32_t)(rng() % (uint64_t)hi);
			const int32_t nl = few_rows ? few[rng() % 4] : rng() % 16 == 0 ? edge[rng() % 4] : 3 + (int32_t)(rng() % 2498);
			tasks.push_back(call(rng, ext, al, nl));
		}
		char what[64];
		snprintf(what, sizeof(what), "random table %d (%zu calls)", round, n);
		check(what, tasks, opt, kn, false);
	}
	// what the device planner declines
	{
		std::vector<mpa_dp_task_t> tasks = { call(rng, true, 30, 100), call(rng, false, 30, 100), call(rng, true, 500, 300) };
		DpPlanKnobs kn;
		check("three calls", tasks, opt, kn, false);
		// extension calls of fewer than three rows are swept by nobody (class X_NONE): planned alike at every width, 1 100 columns included
		{
			std::vector<mpa_dp_task_t> t3 = tasks;
			for (int32_t nl = 0; nl < 3; ++nl)
				for (int32_t al : { 1, 16, 17, 64, 65, 128, 129, 256, 257, 512, 1024, 1025, 1100 }) t3.push_back(call(rng, true, al, nl)), t3.push_back(call(rng, false, al > 300 ? 300 : al, nl));
			for (int k = 0; k < 40; ++k) t3.push_back(call(rng, (rng() & 1) != 0, 1 + (int32_t)(rng() % 1000), 3 + (int32_t)(rng() % 900)));
			check("extension calls of fewer than three rows", t3, opt, kn, false);
			DpPlanKnobs k3 = kn; k3.lite_min = 3, k3.lite_wide = 1; check("... with the checkpointed classes from three rows", t3, opt, k3, false);
			check("only such calls", std::vector<mpa_dp_task_t>(t3.begin() + 3, t3.begin() + 3 + 2), opt, kn, false);
		}
		DpPlanKnobs k2 = kn; k2.pool = 1; check("pool", tasks, opt, k2, true);
		k2 = kn, k2.antidiag = 1; check("antidiag", tasks, opt, k2, true);
		k2 = kn, k2.no_split = 1; check("no_split", tasks, opt, k2, true);
		mpa_dpopt_t o2 = opt; o2.ge = 300; check("wide ge", tasks, o2, kn, true);
		o2 = opt, o2.xdrop = -1; check("options", tasks, o2, kn, true);
		std::vector<mpa_dp_task_t> t2 = tasks; t2.push_back(call(rng, true, 1100, 300)); check("X_HUGE", t2, opt, kn, true);
		t2 = tasks, t2[1].al = 0; check("malformed", t2, opt, kn, true);
		t2 = tasks, t2[1].nl = -5; check("negative rows", t2, opt, kn, true);
		t2 = tasks, t2[0].vid = 6; check("no such contig", t2, opt, kn, true);
		t2 = tasks, t2[0].vid = 4, t2[0].nt_off = kCtg[2] - 99; check("window past its contig", t2, opt, kn, true);
		t2 = tasks, t2[1].flag = 0; check("global without CIGAR", t2, opt, kn, true);
		t2 = tasks, t2.push_back(call(rng, false, 200, 2000)); k2 = kn, k2.tb_budget = 1 << 16; check("two traceback chunks", t2, opt, k2, true);
		check("no calls", std::vector<mpa_dp_task_t>(), opt, kn, true);
	}
	printf("%d tables planned, %d declined, %d mismatches\n", n_planned, n_declined, n_bad);
	return n_bad != 0;
}
