// box.cpp -- tyr_query_box: batched box-overlap queries on the ctx's scene (include/tyr_c.h "Box-overlap queries"; the kernel
// is hip/box.hip).  A query like the multi-hit queries of host/hits.cpp: it reads and writes no render state, runs on the
// caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket and its `done`
// event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/box.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_box(tyr_ctx* c, uint32_t n, const float* lo, const float* hi, uint32_t max_prims, uint32_t flags, const tyr_box_out* out, void* stream) {
	const bool any = (flags & TYR_QUERY_BOX_ANY) != 0u;
	if (!c || n >= (1u << 31) || (flags & ~TYR_QUERY_BOX_ANY) != 0u || max_prims > TYR_QUERY_BOX_MAX || (any && max_prims != 0u))
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!lo || !hi || !out || !out->count || (max_prims > 0u && !out->prim))
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	BoxParams P{};
	query_fields(P, c, L);
	P.lo = lo;
	P.hi = hi;
	P.count = out->count;
	P.prim = max_prims > 0u ? out->prim : nullptr;
	P.n = n;
	P.maxPrims = max_prims;
	launch_box(P, any, c->numCUs, c->launchCache, L.s);
	return L.close();
}
