// dpplan_dbg.cpp -- mpa_dbg_dp_plan_device (include/mpamd_dbg.h), the test hook of MPA_GPU_DPPLAN: a task table through the device planner
// of a DP round (dev_dp_plan_dbg of dp_exec.hip) or, without a context, through its model -- the same stages with a team of one on the
// host (dp_plan_model of dp_plan.cpp).  Built into libmpamd_dbg.so: the C ABI of libmpamd.so stays what it was.
#include <vector>
#include "mpa_internal.h"
#include "dp_plan.h"
#include "ext_huge_wg_core.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

// knobs[8] of the hooks (knobs[9] of the *_wide ones: split_wide, as the executor passes it -- off with the pool and in a repeated round)
static DpPlanKnobs knobs_of(const int64_t *knobs, bool wide)
{
	DpPlanKnobs kn;
	kn.lite_min = (int32_t)knobs[0], kn.lite_wide = (int32_t)knobs[1], kn.no_split = (int32_t)knobs[2], kn.antidiag = (int32_t)knobs[3], kn.pool = (int32_t)knobs[4];
	kn.ext_dual = (int32_t)knobs[5], kn.unit_prio = (int32_t)knobs[6], kn.tb_budget = knobs[7];
	kn.split_wide = wide && knobs[8] && !kn.pool && !kn.no_split;
	return kn;
}

static int64_t plan_device(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n,
                           const mpa_dp_task_t *tasks, const int64_t *knobs, void *buf, int64_t cap, bool wide)
{
	return mpa::guarded<int64_t>(MPA_ERR_HIP, [&]() -> int64_t {
		if (!opt || !q_off || !knobs || n_seq < 0 || n_ctg < 0 || (n_ctg > 0 && !ctg_len) || (n > 0 && !tasks)) { set_error("mpa_dbg_dp_plan_device: missing arguments"); return MPA_ERR_ARG; }
		const DpPlanKnobs kn = knobs_of(knobs, wide);
		const mpa_qbatch_t q{ n_seq, nullptr, q_off };
		if (ctx) return dev_dp_plan_dbg(ctx, opt, n_ctg, ctg_len, &q, n, tasks, kn, buf, cap, wide);
		DpPlan plan;
		std::vector<DpUnit> units;
		const int rc = dp_plan_model(tasks, n, ctg_len, n_ctg, &q, opt, kn, dp_round_args_bytes(), plan, units);
		if (rc == MPA_ERR_UNSUPPORTED) { set_error("device DP plan: " + plan.err); return MPA_DBG_DP_PLAN_DECLINED; }
		if (rc != MPA_OK) { set_error(plan.err); return rc; }
		return dp_plan_write(plan, units, buf, cap, wide);
	});
}

extern "C" int64_t mpa_dbg_dp_plan_device(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n,
                                          const mpa_dp_task_t *tasks, const int64_t *knobs, void *buf, int64_t cap)
{
	return plan_device(ctx, opt, n_ctg, ctg_len, n_seq, q_off, n, tasks, knobs, buf, cap, false);
}

extern "C" int64_t mpa_dbg_dp_plan_device_wide(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n,
                                               const mpa_dp_task_t *tasks, const int64_t *knobs, void *buf, int64_t cap)
{
	return plan_device(ctx, opt, n_ctg, ctg_len, n_seq, q_off, n, tasks, knobs, buf, cap, true);
}

extern "C" int64_t mpa_dbg_dp_plan_wide(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                                        const int64_t *knobs, void *buf, int64_t cap)
{
	return mpa::guarded<int64_t>(MPA_ERR_HIP, [&]() -> int64_t {
		if (!opt || !q_off || !knobs || n_seq < 0 || n_ctg < 0 || (n_ctg > 0 && !ctg_len) || (n > 0 && !tasks)) { set_error("mpa_dbg_dp_plan_wide: missing arguments"); return MPA_ERR_ARG; }
		const DpPlanKnobs kn = knobs_of(knobs, true);
		const mpa_qbatch_t q{ n_seq, nullptr, q_off };
		DpPlan plan;
		int64_t r = dp_plan(tasks, n, ctg_len, sizeof(int64_t), n_ctg, &q, opt, kn, dp_round_args_bytes(), plan);
		if (r == MPA_OK) r = dp_plan_serialize(plan, kn, buf, cap, true);
		if (r < 0) set_error(plan.err);
		return r;
	});
}

// (knobs[10]: the nine of mpa_dbg_dp_plan_wide, then lite_w8 as the executor passes it -- off with the pool)
extern "C" int64_t mpa_dbg_dp_plan_w8(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                                      const int64_t *knobs, void *buf, int64_t cap)
{
	return mpa::guarded<int64_t>(MPA_ERR_HIP, [&]() -> int64_t {
		if (!opt || !q_off || !knobs || n_seq < 0 || n_ctg < 0 || (n_ctg > 0 && !ctg_len) || (n > 0 && !tasks)) { set_error("mpa_dbg_dp_plan_w8: missing arguments"); return MPA_ERR_ARG; }
		DpPlanKnobs kn = knobs_of(knobs, true);
		kn.lite_w8 = knobs[9] && !kn.pool;
		const mpa_qbatch_t q{ n_seq, nullptr, q_off };
		DpPlan plan;
		int64_t r = dp_plan(tasks, n, ctg_len, sizeof(int64_t), n_ctg, &q, opt, kn, dp_round_args_bytes(), plan);
		if (r == MPA_OK) r = dp_plan_serialize(plan, kn, buf, cap, true, true);
		if (r < 0) set_error(plan.err);
		return r;
	});
}

extern "C" int mpa_dbg_dp_last_classes(const mpa_ctx_t *ctx, int64_t ext_calls[16])
{
	if (!ctx || !ext_calls) { set_error("mpa_dbg_dp_last_classes: missing arguments"); return MPA_ERR_ARG; }
	dp_last_ext_calls(ctx, ext_calls);
	return MPA_OK;
}

extern "C" int mpa_dbg_dp_last_huge(const mpa_ctx_t *ctx, int64_t out[4])
{
	if (!ctx || !out) { set_error("mpa_dbg_dp_last_huge: missing arguments"); return MPA_ERR_ARG; }
	dp_last_huge(ctx, out);
	return MPA_OK;
}

extern "C" int mpa_dbg_dp_last_mb(const mpa_ctx_t *ctx, int64_t out[4])
{
	if (!ctx || !out) { set_error("mpa_dbg_dp_last_mb: missing arguments"); return MPA_ERR_ARG; }
	dp_last_mb(ctx, out);
	return MPA_OK;
}

extern "C" int mpa_dbg_dp_last_w8(const mpa_ctx_t *ctx, int64_t out[4])
{
	if (!ctx || !out) { set_error("mpa_dbg_dp_last_w8: missing arguments"); return MPA_ERR_ARG; }
	dp_last_w8(ctx, out);
	return MPA_OK;
}

extern "C" void mpa_dbg_dp_huge_wg_info(int32_t out[3])
{
	if (out) out[0] = hwg::W, out[1] = hwg::R, out[2] = hwg::MIN_BLOCKS;
}
