// round2_dbg.cpp -- mpa_dbg_dp_run_resident (include/mpamd_dbg.h), the test hook of MPA_GPU_ROUND2: a task table through a DP round that is
// planned from device-resident tasks and assembles its results on the device (dev_dp_run_resident_dbg of dp_exec.hip) or, without a
// context, made-up kernel outputs through the stages of dp_results_core.h with a team of one.  Built into libmpamd_dbg.so: the C ABI of
// libmpamd.so stays what it was.
#include <vector>
#include "mpa_internal.h"
#include "dp_plan.h"
#include "dp_results_core.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

namespace mpa {
int dev_dp_run_resident_dbg(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *in, mpa_dp_rst_t *rst,
                            uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec);
}

extern "C" int mpa_dbg_dp_run_resident(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *tasks,
                                       const mpa_dbg_dp_outputs_t *made_up, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec)
{
	return mpa::guarded<int>(MPA_ERR_HIP, [&]() -> int {
		if (cigar_pool) *cigar_pool = nullptr;
		if (n_pool) *n_pool = 0;
		if (n <= 0 || !tasks || !rst || !rec || !cigar_pool) { set_error("mpa_dbg_dp_run_resident: missing arguments"); return MPA_ERR_ARG; }
		for (int k = 0; k < MPA_DBG_ROUND2_REC; ++k) rec[k] = 0;
		if (ctx) {
			if (!mi || !opt || !q) { set_error("mpa_dbg_dp_run_resident: missing arguments"); return MPA_ERR_ARG; }
			return dev_dp_run_resident_dbg(ctx, mi, opt, q, n, tasks, rst, cigar_pool, n_pool, rec);
		}
		// without a context: the bounds and the four stages with a team of one, on the outputs the caller made up
		const mpa_dbg_dp_outputs_t *m = made_up;
		if (!m || !m->ext_out || !m->score || !m->n_cigar || m->n_glob < 0 || m->n_glob > n || (m->n_glob > 0 && !m->gids)) { set_error("mpa_dbg_dp_run_resident: no outputs to assemble"); return MPA_ERR_ARG; }
		std::vector<uint8_t> seen((size_t)n, 0);
		for (int64_t g = 0; g < m->n_glob; ++g) {
			const int32_t id = m->gids[g];
			if (id < 0 || id >= n || seen[(size_t)id] || (tasks[id].flag & (MPA_F_EXT_LEFT | MPA_F_EXT_RIGHT))) { set_error("mpa_dbg_dp_run_resident: gids is not a list of distinct traceback calls"); return MPA_ERR_ARG; }
			seen[(size_t)id] = 1;
		}
		const DpTaskBounds bd = dp_task_bounds(tasks, n);
		rec[7] = bd.prep, rec[8] = bd.max_nl, rec[9] = bd.max_al;
		std::vector<DTask> dt((size_t)n);
		for (int64_t k = 0; k < n; ++k) { DTask &t = dt[(size_t)k]; t = DTask(); t.flag = tasks[k].flag, t.nl = tasks[k].nl, t.al = tasks[k].al, t.cig_cap = INT32_MAX; }
		std::vector<int64_t> off((size_t)m->n_glob + 1), call_off((size_t)n), bsum((size_t)m->n_glob + 1), head(DPR_NHEAD);
		DpResDev R;
		R.n = n, R.n_glob = m->n_glob, R.tasks = dt.data(), R.gids = m->gids, R.eo = (const ExtOut*)m->ext_out, R.sc = m->score, R.nc = m->n_cigar;
		R.off = off.data(), R.call_off = call_off.data(), R.bsum = bsum.data(), R.head = head.data(), R.rst = rst;
		dp_results_model(R);
		rec[10] = head[DPR_H_POOL];
		if (n_pool) *n_pool = head[DPR_H_POOL];
		return MPA_OK;
	});
}
