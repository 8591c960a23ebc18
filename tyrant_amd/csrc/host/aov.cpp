// aov.cpp -- tyr_render_aov: first-hit guide buffers (albedo, normal, depth, ids) of the ctx's current camera and frame, and
// tyr_render_aov_chain: the same guides taken behind mirrors and glass (include/tyr_c.h "AOV buffers" and "Specular-chain
// guides"; the kernels are hip/aov.hip).  Each pass behaves like a query (host/query.cpp): it runs on the
// caller's stream with a ticket word of that stream, its stack overflow bit goes to tyr_query_error, and a later refit or
// scene change waits for it.  No render state is read back or written: the camera basis is computed here, not stored.
#include <cstring>

#include <hip/hip_runtime.h>

#include "../hip/aov.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// the checks, the opened launch and the kernel argument both passes share; `any`: the caller asked for some output
int aov_setup(tyr_ctx* c, uint32_t spp, const tyr_aov_out* out, bool any, void* stream, QueryLaunch& L, AovParams& P) {
	if (!c || !out || spp == 0 || !any)
		return TYR_ERR_INVALID;
	if (static_cast<uint64_t>(spp) * c->localPixels >= (1ull << 32)) // the tickets s * P + p are 32-bit, as k_primary's
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (int rc = L.open(c, stream))
		return rc;

	query_fields(P, c, L);
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
	P.nPixels = c->localPixels;
	P.spp = spp;
	return TYR_OK;
}

} // namespace

int tyr_render_aov(tyr_ctx* c, uint32_t spp, const tyr_aov_out* out, void* stream) {
	QueryLaunch L;
	AovParams P{};
	const bool any = out && (out->albedo || out->normal || out->depth || out->prim || out->geom);
	if (int rc = aov_setup(c, spp, out, any, stream, L, P))
		return rc;
	launch_aov(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}

int tyr_render_aov_chain(tyr_ctx* c, uint32_t spp, uint32_t max_chain, const tyr_aov_out* out, const tyr_aov_chain_out* ext, void* stream) {
	if (max_chain > TYR_AOV_CHAIN_MAX)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	AovChainParams P{};
	const bool any = out && (out->albedo || out->normal || out->depth || out->prim || out->geom || (ext && (ext->chain || ext->end_prim || ext->end_geom || ext->length0 || ext->depth_first)));
	if (int rc = aov_setup(c, spp, out, any, stream, L, P.a))
		return rc;
	if (ext) {
		P.chain = ext->chain;
		P.endPrim = ext->end_prim;
		P.endGeom = ext->end_geom;
		P.length0 = ext->length0;
		P.depthFirst = ext->depth_first;
	}
	P.maxChain = max_chain;
	P.triMaterials = (c->cfg.flags & TYR_FLAG_TRIANGLE_MATERIALS) ? 1u : 0u;
	launch_aov_chain(P, c->numCUs, c->launchCache, L.s);
	return L.close();
}
