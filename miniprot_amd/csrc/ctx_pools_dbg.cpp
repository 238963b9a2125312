// ctx_pools_dbg.cpp -- mpa_dbg_ctx_pools (include/mpamd_dbg.h), the test hook of the contexts' pool registry (dev_ctx.h): the device
// pools a context or one of its siblings has registered, by name and capacity.  Built into libmpamd_dbg.so: the C ABI of libmpamd.so
// stays what it was.
#include "mpa_internal.h"
#include "../../include/mpamd_dbg.h"

using namespace mpa;

extern "C" int32_t mpa_dbg_ctx_pools(const mpa_ctx_t *ctx, int32_t sibling, const char **names, int64_t *caps, int32_t cap)
{
	if (!ctx) { set_error("mpa_dbg_ctx_pools: no context"); return MPA_ERR_ARG; }
	const int32_t n = ctx_pool_list(ctx, sibling, names, caps, names && caps ? cap : 0);
	if (n < 0) { set_error("mpa_dbg_ctx_pools: the context has no sibling of that number"); return MPA_ERR_ARG; }
	return n;
}
