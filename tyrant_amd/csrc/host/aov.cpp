// aov.cpp -- tyr_render_aov: first-hit guide buffers (albedo, normal, depth, ids) of the ctx's current camera and frame
// (include/tyr_c.h "AOV buffers"; the kernel is hip/aov.hip).  The pass behaves like a query (host/query.cpp): it runs on the
// caller's stream with a ticket word of that stream, its stack overflow bit goes to tyr_query_error, and a later refit or
// scene change waits for it.  No render state is read back or written: the camera basis is computed here, not stored.
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../hip/aov.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_render_aov(tyr_ctx* c, uint32_t spp, const tyr_aov_out* out, void* stream) {
	if (!c || !out || spp == 0 || (!out->albedo && !out->normal && !out->depth && !out->prim && !out->geom))
		return TYR_ERR_INVALID;
	if (static_cast<uint64_t>(spp) * c->localPixels >= (1ull << 32)) // the tickets s * P + p are 32-bit, as k_primary's
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	DeviceScope scope;
	HIPCHK(hipGetDevice(&scope.prev));
	if (int rc = use_device(c))
		return rc;
	hipStream_t s = nullptr;
	tyr_ctx::QueryStream* qs = nullptr;
	uint32_t* ticket = nullptr;
	if (int rc = query_ticket(c, stream, s, qs, ticket))
		return rc;

	AovParams P{};
	P.scene = c->scene;
	P.scene.nStaged = std::min(c->scene.nStaged, static_cast<uint32_t>(std::max(c->tuning.stagedNodes, 0))); // as the render's launches stage them
	std::memcpy(P.spheres, c->spheres, sizeof(P.spheres));
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.rank = c->cfg.rank;
	P.nranks = c->cfg.nranks;
	P.localRows = c->localRows;
	P.frame = c->frame;
	std::memcpy(P.camPos, c->cam.position, 12);
	std::memcpy(P.camDir, c->cam.direction, 12);
	camera_basis(c, P.camRight, P.camUp);
	P.focalDistance = c->cam.focalDistance;
	P.lensRadius = c->cam.lensRadius;
	P.palette = (c->cfg.flags & TYR_FLAG_TRIANGLE_COLORS) ? c->dPalette : nullptr;
	P.albedo = out->albedo;
	P.normal = out->normal;
	P.depth = out->depth;
	P.prim = out->prim;
	P.geom = out->geom;
	P.ticket = ticket;
	P.error = c->dQuery;
	P.nPixels = c->localPixels;
	P.spp = spp;
	launch_aov(P, c->numCUs, c->launchCache, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(qs->done, s));
	return TYR_OK;
}
