// tri.cpp -- tyr_query_tri: batched triangle-overlap queries on the ctx's scene (include/tyr_c.h "Triangle-overlap queries"; the
// kernel is hip/tri.hip).  A query like the box queries of host/box.cpp: it reads and writes no render state, runs on the
// caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket and its `done`
// event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/tri.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_tri(tyr_ctx* ctx, uint32_t n, const float* a, const float* b, const float* c, uint32_t max_prims, uint32_t flags, const tyr_tri_out* out, void* stream) {
	const bool any = (flags & TYR_QUERY_TRI_ANY) != 0u;
	if (!ctx || n >= (1u << 31) || (flags & ~(TYR_QUERY_TRI_ANY | TYR_QUERY_TRI_SKIP_SHARED)) != 0u || max_prims > TYR_QUERY_TRI_MAX || (any && max_prims != 0u))
		return TYR_ERR_INVALID;
	if (!ctx->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!a || !b || !c || !out || !out->count || (max_prims > 0u && !out->prim))
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(ctx, stream))
		return rc;

	TriParams P{};
	query_fields(P, ctx, L);
	P.a = a;
	P.b = b;
	P.c = c;
	P.count = out->count;
	P.prim = max_prims > 0u ? out->prim : nullptr;
	P.n = n;
	P.maxPrims = max_prims;
	P.skipShared = (flags & TYR_QUERY_TRI_SKIP_SHARED) != 0u ? 1u : 0u;
	launch_tri(P, any, ctx->numCUs, ctx->launchCache, L.s);
	return L.close();
}
