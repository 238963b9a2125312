// stream_plan.cpp -- the policy of stream_plan.h.  Host only: no HIP, no context, no globals.
#include <algorithm>
#include "stream_plan.h"

namespace mpa {

static StreamPlan legacy_plan(StreamPlan p)
{
	p.layout = SL_LEGACY;
	const int L = p.n_lanes, S = p.n_seed, P = p.n_plan;
	for (int i = 0; i < L; ++i) p.lane[i] = { SC_NORMAL, i }, p.side_cap[i] = StreamPlan::kMaxSide, p.side_cls[i] = SC_NORMAL;
	// (the seed streams come on first use, seeders' before planners' in a stream of batches: their ranks are the order of first use)
	for (int k = 0; k < S; ++k) p.seed_main[k] = { SC_NORMAL, L + k }, p.seed_seed[k] = { SC_HIGH, L + S + P + k };
	for (int k = 0; k < P; ++k) p.plan_main[k] = { SC_NORMAL, L + S + k }, p.plan_seed[k] = { SC_HIGH, L + S + P + S + k };
	p.n_streams = L + 2 * (S + P);
	return p;
}

StreamPlan stream_plan(int q, int n_lanes, int n_seed, int n_plan, int layout)
{
	StreamPlan p = {};
	p.q = std::max(1, std::min(q, 32));
	p.n_lanes = std::max(1, std::min(n_lanes, (int)StreamPlan::kMaxLanes));
	p.n_seed = std::max(1, std::min(n_seed, (int)StreamPlan::kMaxSeed));
	p.n_plan = std::max(1, std::min(n_plan, (int)StreamPlan::kMaxPlan));
	const int Q = p.q, L = p.n_lanes, S = p.n_seed, P = p.n_plan;
	if (layout != SL_A && layout != SL_B && layout != SL_C) layout = SL_LEGACY;
	if (layout == SL_LEGACY || Q >= L + S + P) return legacy_plan(p);   // a queue for every busy stream: today's layout, stream for stream
	p.layout = layout;
	int in_cls[3] = { 0, 0, 0 }, lanes_in[3] = { 0, 0, 0 }, rank = 0;
	// lanes first in their class, one per queue; a lane beyond Q goes to the next class with a queue that carries no lane
	static const int kPref[3] = { SC_NORMAL, SC_HIGH, SC_LOW };
	for (int i = 0; i < L; ++i) {
		int c = SC_NORMAL;
		if (layout != SL_C) {
			c = -1;
			for (int k : kPref) if (lanes_in[k] < Q) { c = k; break; }
			if (c < 0) { c = SC_NORMAL; for (int k : kPref) if (lanes_in[k] < lanes_in[c]) c = k; }   // more lanes than 3 Q queues: the emptiest class
		}
		p.lane[i] = { c, rank++ }, ++in_cls[c], ++lanes_in[c];
	}
	// a seeder or planner has ONE stream: its main stream is its seeding stream
	for (int k = 0; k < S; ++k) p.seed_main[k] = p.seed_seed[k] = { SC_HIGH, rank++ }, ++in_cls[SC_HIGH];
	const int plan_cls = layout == SL_A ? SC_LOW : layout == SL_B ? SC_NORMAL : SC_HIGH;
	for (int k = 0; k < P; ++k) p.plan_main[k] = p.plan_seed[k] = { plan_cls, rank++ }, ++in_cls[plan_cls];
	p.n_streams = rank;
	// side streams: never in a class where every queue carries a lane; in a class with lanes only on the queues still free, dealt out
	// lane by lane; in a class without lanes (they double up with planners at worst) Q of them, and at least one per lane
	const int sc = layout == SL_C && in_cls[SC_NORMAL] < Q ? SC_NORMAL : SC_LOW;
	const int free_q = std::max(0, Q - in_cls[sc]);
	const bool no_lane = lanes_in[sc] == 0;
	const int deal = lanes_in[sc] >= Q ? 0 : free_q > 0 ? free_q : no_lane ? Q : 0;
	for (int i = 0; i < L; ++i) {
		int cap = deal / L + (i < deal % L ? 1 : 0);
		if (cap == 0 && no_lane) cap = 1;
		p.side_cap[i] = std::min(cap, (int)StreamPlan::kMaxSide), p.side_cls[i] = sc;
	}
	return p;
}

int64_t stream_plan_words(const StreamPlan &p, int32_t *out, int64_t cap)
{
	const int64_t n = 6 + 4 * ((int64_t)p.n_lanes + p.n_seed + p.n_plan);
	if (!out || cap < n) return n;
	int32_t *w = out;
	*w++ = p.q, *w++ = p.n_lanes, *w++ = p.n_seed, *w++ = p.n_plan, *w++ = p.layout, *w++ = p.n_streams;
	for (int i = 0; i < p.n_lanes; ++i) *w++ = p.lane[i].cls, *w++ = p.lane[i].rank, *w++ = p.side_cap[i], *w++ = p.side_cls[i];
	for (int k = 0; k < p.n_seed; ++k) *w++ = p.seed_main[k].cls, *w++ = p.seed_main[k].rank, *w++ = p.seed_seed[k].cls, *w++ = p.seed_seed[k].rank;
	for (int k = 0; k < p.n_plan; ++k) *w++ = p.plan_main[k].cls, *w++ = p.plan_main[k].rank, *w++ = p.plan_seed[k].cls, *w++ = p.plan_seed[k].rank;
	return n;
}

int stream_layout_of(const char *env)
{
	if (!env || !*env) return kStreamLayoutDefault;
	switch (env[0]) {
	case '0': return SL_LEGACY;
	case 'A': case 'a': return SL_A;
	case 'B': case 'b': return SL_B;
	case 'C': case 'c': return SL_C;
	default: return kStreamLayoutDefault;
	}
}

} // namespace mpa
