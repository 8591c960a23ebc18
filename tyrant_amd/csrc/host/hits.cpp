// hits.cpp -- tyr_query_hits: batched multi-hit ray queries on the ctx's scene (include/tyr_c.h "Multi-hit queries"; the
// kernel is hip/hits.hip).  A query like the ray queries of host/query.cpp: it reads and writes no render state, runs on the
// caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket and its `done`
// event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/hits.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_hits(tyr_ctx* c, uint32_t n, const float* origins, const float* directions, const float* tmax, uint32_t max_hits, uint32_t flags, const tyr_hits_out* out, void* stream) {
	if (!c || n >= (1u << 31) || (flags & ~TYR_QUERY_TWO_SIDED) != 0u || max_hits == 0u || max_hits > TYR_QUERY_HITS_MAX)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!origins || !directions || !out || !out->count || !out->t || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	HitsParams P{};
	query_fields(P, c, L);
	P.origins = origins;
	P.directions = directions;
	P.tmax = tmax;
	P.count = out->count;
	P.t = out->t;
	P.prim = out->prim;
	P.uv = out->uv;
	P.side = out->side;
	P.backCount = out->back_count;
	P.n = n;
	P.maxHits = max_hits;
	launch_hits(P, (flags & TYR_QUERY_TWO_SIDED) != 0u, c->numCUs, c->launchCache, L.s);
	return L.close();
}
