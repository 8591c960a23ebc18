// nearest.cpp -- tyr_query_nearest: batched closest-point queries on the ctx's scene (include/tyr_c.h "Closest-point
// queries"; the kernel is hip/nearest.hip).  A query like the ray queries of host/query.cpp: it reads and writes no render
// state, runs on the caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket
// and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/nearest.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_nearest(tyr_ctx* c, uint32_t n, const float* points, const float* max_dist, uint32_t flags, const tyr_nearest_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u)
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

	NearestParams P{};
	query_fields(P, c, L);
	P.points = points;
	P.maxDist = max_dist;
	P.dist2 = out->dist2;
	P.prim = out->prim;
	P.uv = out->uv;
	P.region = out->region;
	P.point = out->point;
	P.n = n;
	launch_nearest(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
