// segment.cpp -- tyr_query_segment: batched closest-segment queries on the ctx's scene (include/tyr_c.h "Closest-segment
// queries"; the kernel is hip/segment.hip).  A query like the closest-point queries of host/nearest.cpp: it reads and writes no
// render state, runs on the caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk
// ticket and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/segment.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_segment(tyr_ctx* c, uint32_t n, const float* p, const float* q, const float* max_dist, uint32_t flags, const tyr_segment_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!p || !q || !out || !out->dist2 || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	SegmentParams P{};
	query_fields(P, c, L);
	P.p = p;
	P.q = q;
	P.maxDist = max_dist;
	P.dist2 = out->dist2;
	P.prim = out->prim;
	P.s = out->s;
	P.feature = out->feature;
	P.region = out->region;
	P.onSegment = out->on_segment;
	P.onTriangle = out->on_triangle;
	P.n = n;
	launch_segment(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
