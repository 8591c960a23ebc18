// nearest_k.cpp -- tyr_query_nearest_k: batched k-nearest and within-radius triangle queries on the ctx's scene
// (include/tyr_c.h "k-nearest queries"; the kernel is hip/nearest_k.hip).  A query like tyr_query_nearest of host/nearest.cpp:
// it reads and writes no render state, runs on the caller's stream and goes through the same per-stream bookkeeping
// (query_ticket: the stream's chunk ticket and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
#include <algorithm>

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
	DeviceScope scope;
	HIPCHK(hipGetDevice(&scope.prev));
	if (int rc = use_device(c))
		return rc;
	hipStream_t s = nullptr;
	tyr_ctx::QueryStream* qs = nullptr;
	uint32_t* ticket = nullptr;
	if (int rc = query_ticket(c, stream, s, qs, ticket))
		return rc;

	NearestKParams P{};
	P.scene = c->scene;
	P.scene.nStaged = std::min(c->scene.nStaged, static_cast<uint32_t>(std::max(c->tuning.stagedNodes, 0))); // as the render's launches stage them
	P.points = points;
	P.maxDist = max_dist;
	P.dist2 = out->dist2;
	P.prim = out->prim;
	P.count = out->count;
	P.uv = out->uv;
	P.region = out->region;
	P.point = out->point;
	P.ticket = ticket;
	P.error = c->dQuery;
	P.n = n;
	P.k = k;
	launch_nearest_k(P, c->numCUs, c->launchCache, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(qs->done, s));
	return TYR_OK;
}
