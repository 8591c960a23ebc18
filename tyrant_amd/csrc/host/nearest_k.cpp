// nearest_k.cpp -- tyr_query_nearest_k: batched k-nearest and within-radius triangle queries on the ctx's scene
// (include/tyr_c.h "k-nearest queries"; the kernel is hip/nearest_k.hip).  A query like tyr_query_nearest of host/nearest.cpp:
// it reads and writes no render state, runs on the caller's stream and goes through the same per-stream bookkeeping
// (QueryLaunch: the stream's chunk ticket and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/nearest_k.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_nearest_k(tyr_ctx* c, uint32_t n, const float* points, const float* max_dist, uint32_t k, uint32_t flags, const tyr_nearest_k_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u || k == 0u || k > TYR_QUERY_NEAREST_K_MAX)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!points || !out || !out->dist2 || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	NearestKParams P{};
	query_fields(P, c, L);
	P.points = points;
	P.maxDist = max_dist;
	P.dist2 = out->dist2;
	P.prim = out->prim;
	P.count = out->count;
	P.uv = out->uv;
	P.region = out->region;
	P.point = out->point;
	P.n = n;
	P.k = k;
	launch_nearest_k(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
