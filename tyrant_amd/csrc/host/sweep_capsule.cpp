// sweep_capsule.cpp -- tyr_query_sweep_capsule: batched swept-capsule queries on the ctx's scene (include/tyr_c.h "Swept-capsule
// queries"; the kernel is hip/sweep_capsule.hip).  A query like the swept spheres of host/sweep.cpp: it reads and writes no
// render state, runs on the caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk
// ticket and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <hip/hip_runtime.h>

#include "../hip/sweep_capsule.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_sweep_capsule(tyr_ctx* c, uint32_t n, const float* p, const float* q, const float* directions, const float* radius, const float* tmax,
                            uint32_t flags, const tyr_sweep_capsule_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!p || !q || !directions || !radius || !out || !out->t || !out->prim)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	SweepCapsuleParams P{};
	query_fields(P, c, L);
	P.p = p;
	P.q = q;
	P.directions = directions;
	P.radius = radius;
	P.tmax = tmax;
	P.t = out->t;
	P.prim = out->prim;
	P.s = out->s;
	P.feature = out->feature;
	P.region = out->region;
	P.point = out->point;
	P.center = out->center;
	P.normal = out->normal;
	P.n = n;
	launch_sweep_capsule(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
