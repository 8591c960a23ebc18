// tri_distance.cpp -- tyr_query_tri_distance: batched closest-triangle distance queries on the ctx's scene (include/tyr_c.h
// "Closest-triangle queries"; the kernel is hip/tri_distance.hip).  A query like the closest-segment queries of
// host/segment.cpp: it reads and writes no render state, runs on the caller's stream and goes through the same per-stream
// bookkeeping (QueryLaunch: the stream's chunk ticket and its `done` event, which tyr_query_error, tyr_scene_refit and
// tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/tri_distance.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_tri_distance(tyr_ctx* c, uint32_t n, const float* a, const float* b, const float* cc, const float* max_dist, uint32_t flags, const tyr_tri_distance_out* out,
                           void* stream) {
	if (!c || n >= (1u << 31) || (flags & ~TYR_QUERY_TRI_SKIP_SHARED) != 0u)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!a || !b || !cc || !out || !out->dist2 || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	TriDistanceParams P{};
	query_fields(P, c, L);
	P.a = a;
	P.b = b;
	P.c = cc;
	P.maxDist = max_dist;
	P.dist2 = out->dist2;
	P.prim = out->prim;
	P.feature = out->feature;
	P.region = out->region;
	P.onQuery = out->on_query;
	P.onTriangle = out->on_triangle;
	P.n = n;
	P.skipShared = (flags & TYR_QUERY_TRI_SKIP_SHARED) ? 1u : 0u;
	launch_tri_distance(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
