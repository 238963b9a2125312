// stream_dbg.cpp -- mpa_dbg_stream_plan and mpa_dbg_stream_plan_for (include/mpamd_dbg.h), the test hooks of the stream plan
// (stream_plan.h): the plan a context's last stream of batches created its sibling contexts by, and the plan of the module for given
// numbers.  Built into libmpamd_dbg.so: the C ABI of libmpamd.so stays what it was.
#include "mpa_internal.h"
#include "stream_plan.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

extern "C" int64_t mpa_dbg_stream_plan(const mpa_ctx_t *ctx, int32_t *out, int64_t cap)
{
	if (!ctx) { set_error("mpa_dbg_stream_plan: no context"); return MPA_ERR_ARG; }
	const StreamPlan *p = ctx_stream_plan(ctx);
	return p ? stream_plan_words(*p, out, cap) : 0;
}

extern "C" int64_t mpa_dbg_stream_plan_for(int32_t q, int32_t n_lanes, int32_t n_seed, int32_t n_plan, const char *layout, int32_t *out, int64_t cap)
{
	return stream_plan_words(stream_plan(q > 0 ? q : ctx_hw_queues(), n_lanes, n_seed, n_plan, stream_layout_of(layout)), out, cap);
}
