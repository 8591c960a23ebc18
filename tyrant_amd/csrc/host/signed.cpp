// signed.cpp -- tyr_query_signed and tyr_bake_sdf: signed distances to the ctx's scene (include/tyr_c.h "Signed-distance
// queries"; the kernels are hip/signed.hip).  Queries like those of host/nearest.cpp and host/winding.cpp, whose two contracts
// they join: no render state, the caller's stream, the same per-stream bookkeeping (QueryLaunch: the stream's chunk ticket and
// its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).  The bake is two launches on that stream
// with nothing for the host to wait for between them: the list of near bricks the first one leaves for the second, and its
// length, stay on the device, in scratch the ctx keeps from call to call.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../hip/signed.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// room for nBricks indices behind the count word; a list that has to grow waits for the bake that may still read the old one
int sdf_list(tyr_ctx* c, size_t nBricks) {
	if (!c->sdfDone)
		HIPCHK(hipEventCreateWithFlags(&c->sdfDone, hipEventDisableTiming));
	if (c->dSdfList && c->sdfListCap >= nBricks)
		return TYR_OK;
	HIPCHK(hipEventSynchronize(c->sdfDone));
	dev_free(c->dSdfList);
	c->sdfListCap = 0;
	if (int rc = dev_alloc(c->dSdfList, nBricks + 1))
		return rc;
	c->sdfListCap = nBricks;
	return TYR_OK;
}

} // namespace

namespace tyr {
namespace drv {

void sdf_free(tyr_ctx* c) {
	if (c->sdfDone) {
		(void)hipEventSynchronize(c->sdfDone);
		(void)hipEventDestroy(c->sdfDone);
		c->sdfDone = nullptr;
	}
	dev_free(c->dSdfList);
	c->sdfListCap = 0;
}

} // namespace drv
} // namespace tyr

int tyr_query_signed(tyr_ctx* c, uint32_t n, const float* points, const float* max_dist, float accuracy, uint32_t flags, const tyr_signed_out* out, void* stream) {
	if (!c || n >= (1u << 31) || flags != 0u || !(accuracy >= 0.0f))
		return TYR_ERR_INVALID;
	if (!(c->cfg.flags & TYR_FLAG_WINDING))
		return TYR_ERR_UNSUPPORTED;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!points || !out || !out->sd)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	SignedParams P{};
	query_fields(P, c, L);
	P.wnodes = c->winding.nodes;
	P.nWNodes = c->winding.nNodes; // 0: a scene without triangles, every w = 0
	P.accuracy = accuracy;
	P.points = points;
	P.maxDist = max_dist;
	P.sd = out->sd;
	P.prim = out->prim;
	P.point = out->point;
	P.gradient = out->gradient;
	P.w = out->w;
	P.n = n;
	launch_signed(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}

int tyr_bake_sdf(tyr_ctx* c, const tyr_sdf_grid* grid, uint32_t flags, const tyr_sdf_out* out, void* stream) {
	if (!c || !grid || flags != 0u || !out || !out->sd)
		return TYR_ERR_INVALID;
	if (!(std::isfinite(grid->cell) && grid->cell > 0.0f && std::isfinite(grid->band) && grid->band > 0.0f && grid->accuracy >= 0.0f))
		return TYR_ERR_INVALID;
	uint64_t voxels = 1;
	for (int k = 0; k < 3; ++k) {
		if (!std::isfinite(grid->origin[k]) || grid->dims[k] == 0u)
			return TYR_ERR_INVALID;
		voxels *= grid->dims[k]; // (each factor and every partial product below 2^31, or refused: no overflow of 64 bits)
		if (voxels >= (1ull << 31))
			return TYR_ERR_INVALID;
	}
	if (!(c->cfg.flags & TYR_FLAG_WINDING))
		return TYR_ERR_UNSUPPORTED;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;

	SdfParams P{};
	uint64_t nBricks = 1;
	for (int k = 0; k < 3; ++k) {
		P.origin[k] = grid->origin[k];
		P.dims[k] = grid->dims[k];
		P.bricks[k] = (grid->dims[k] + 3u) / 4u;
		nBricks *= P.bricks[k];
	}
	P.nBricks = static_cast<uint32_t>(nBricks);
	P.cell = grid->cell;
	P.band = grid->band;
	P.accuracy = grid->accuracy;
	{
		// binary32, one operation at a time (the header's rule; this file is built with -ffp-contract=off)
		volatile float k = 2.625f * grid->cell;
		volatile float r = grid->band + k;
		P.reach = r;
	}
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;
	if (int rc = sdf_list(c, P.nBricks))
		return rc;
	HIPCHK(hipStreamWaitEvent(L.s, c->sdfDone, 0)); // the bake before this one, on whatever stream: the list is the ctx's
	HIPCHK(hipMemsetAsync(c->dSdfList, 0, sizeof(uint32_t), L.s));
	query_fields(P, c, L);
	P.wnodes = c->winding.nodes;
	P.nWNodes = c->winding.nNodes;
	P.sd = out->sd;
	P.prim = out->prim;
	P.stats = out->stats;
	P.nearList = c->dSdfList;
	launch_sdf_bricks(P, c->numCUs, c->launchCache, L.s);
	if (int rc = L.close())
		return rc;
	if (int rc = L.open(c, stream)) // (clears the stream's ticket behind the first launch)
		return rc;
	P.ticket = L.ticket;
	launch_sdf_voxels(P, c->numCUs, c->launchCache, L.s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->sdfDone, L.s));
	return L.close();
}
