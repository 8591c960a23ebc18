// sweep.cpp -- tyr_query_sweep: batched swept-sphere queries on the ctx's scene (include/tyr_c.h "Swept-sphere queries"; the
// kernel is hip/sweep.hip).  A query like the closest-point queries of host/nearest.cpp: it reads and writes no render state,
// runs on the caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket and its
// `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/sweep.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_sweep(tyr_ctx* c, uint32_t n, const float* origins, const float* directions, const float* radius, const float* tmax, uint32_t flags,
                    const tyr_sweep_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!origins || !directions || !radius || !out || !out->t || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	SweepParams P{};
	query_fields(P, c, L);
	P.origins = origins;
	P.directions = directions;
	P.radius = radius;
	P.tmax = tmax;
	P.t = out->t;
	P.prim = out->prim;
	P.region = out->region;
	P.point = out->point;
	P.center = out->center;
	P.normal = out->normal;
	P.n = n;
	launch_sweep(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
