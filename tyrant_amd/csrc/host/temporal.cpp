// temporal.cpp -- tyr_render_motion / tyr_render_motion_chain: motion vectors and the expected previous depth of the ctx's current AOV frame; and
// tyr_temporal: the reprojected accumulation of frames with a history the ctx owns (include/tyr_c.h "Motion vectors" and
// "Temporal reprojection"; the kernels are hip/temporal.hip).
// The motion pass behaves like a query (host/aov.cpp): it reads the uploaded triangles on the caller's stream, and a later
// refit or scene change waits for it.  The temporal pass behaves like tyr_denoise (host/denoise.cpp): it needs no scene, and
// since the history belongs to the ctx, each call waits on its stream for the previous call's event.  Neither touches render
// state; the camera bases are computed here, not stored.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../hip/temporal.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// the defaults (tyr_temporal_params NULL); how they were chosen: DESIGN.md "Temporal reprojection"
constexpr uint32_t kDefaultMaxHistory = 16;
constexpr float kDefaultDepthTolerance = 0.05f;
constexpr float kDefaultNormalCos = 0.9f;

// position, direction, basis and the basis' squared lengths of a camera, as the projection reads them
void camera_fields(const tyr_ctx* c, const tyr_camera& cam, float pos[3], float dir[3], float right[3], float up[3], float& FF, float& RR, float& UU) {
	std::memcpy(pos, cam.position, 12);
	std::memcpy(dir, cam.direction, 12);
	camera_basis(c, cam, right, up);
	FF = dot(ld3(dir), ld3(dir));
	RR = dot(ld3(right), ld3(right));
	UU = dot(ld3(up), ld3(up));
}

// both motion passes; via: tyr_render_motion_chain's chain inputs, or null
int render_motion(tyr_ctx* c, const tyr_motion_in* in, const tyr_motion_chain_in* via, const tyr_motion_out* out, void* stream) {
	if (!c || !in || !out || !in->prim || !in->geom || !in->prev_camera || (!out->motion && !out->prev_depth))
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	QueryLaunch L; // (for its `done` event: a refit waits for the pass; the ticket word goes unused)
	if (int rc = L.open(c, stream))
		return rc;

	MotionParams P{};
	P.tris = c->scene.tris;
	P.nPrims = c->scene.nPrims;
	std::memcpy(P.spheres, c->spheres, sizeof(P.spheres));
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.rank = c->cfg.rank;
	P.nranks = c->cfg.nranks;
	P.localRows = c->localRows;
	P.frame = c->frame;
	camera_fields(c, c->cam, P.camPos, P.camDir, P.camRight, P.camUp, P.camFF, P.camRR, P.camUU);
	P.focalDistance = c->cam.focalDistance;
	P.lensRadius = c->cam.lensRadius;
	camera_fields(c, *in->prev_camera, P.prevPos, P.prevDir, P.prevRight, P.prevUp, P.prevFF, P.prevRR, P.prevUU);
	P.prim = in->prim;
	P.geom = in->geom;
	P.prevPrims = reinterpret_cast<const float*>(in->prev_prims);
	P.motion = out->motion;
	P.prevDepth = out->prev_depth;
	if (c->localPixels != 0) {
		if (via)
			launch_motion_chain(P, via->chain, via->length0, L.s);
		else
			launch_motion(P, L.s);
	}
	return L.close();
}

} // namespace

int tyr_render_motion(tyr_ctx* c, const tyr_motion_in* in, const tyr_motion_out* out, void* stream) { return render_motion(c, in, nullptr, out, stream); }

int tyr_render_motion_chain(tyr_ctx* c, const tyr_motion_in* in, const tyr_motion_chain_in* via, const tyr_motion_out* out, void* stream) {
	if (!via || !via->chain || !via->length0)
		return TYR_ERR_INVALID;
	return render_motion(c, in, via, out, stream);
}

int tyr_temporal(tyr_ctx* c, const tyr_temporal_in* in, const tyr_temporal_params* params, void* device_rgba_out, float* history_len_out, void* stream) {
	if (!c || !in || !in->albedo || !in->normal || !in->depth || !in->motion || !in->prev_depth || !device_rgba_out)
		return TYR_ERR_INVALID;
	tyr_temporal_params p{ kDefaultMaxHistory, kDefaultDepthTolerance, kDefaultNormalCos, 0u };
	if (params)
		p = *params;
	if (!reprojection_ok(p.max_history, p.depth_tolerance, p.normal_cos) || (p.flags & ~TYR_TEMPORAL_RESET) != 0u)
		return TYR_ERR_INVALID;
	const float4* accum = in->accum ? reinterpret_cast<const float4*>(in->accum) : c->blit;
	if (!accum)
		return TYR_ERR_NO_BUFFER;
	FilterLaunch L;
	if (int rc = L.open(c, c->temporal, stream))
		return rc;
	const size_t n = static_cast<size_t>(c->cfg.width) * c->cfg.height;
	if (int rc = L.buffer(c->dTemporal, 4 * n))
		return rc;

	TemporalParams P{};
	P.haveHistory = L.history((p.flags & TYR_TEMPORAL_RESET) != 0u);
	const uint32_t prev = L.prev, next = L.next;
	P.accum = accum;
	P.albedo = in->albedo;
	P.normal = in->normal;
	P.depth = in->depth;
	P.motion = reinterpret_cast<const float2*>(in->motion);
	P.prevDepth = in->prev_depth;
	P.histIn[0] = c->dTemporal + 2 * prev * n;
	P.histIn[1] = c->dTemporal + (2 * prev + 1) * n;
	P.histOut[0] = c->dTemporal + 2 * next * n;
	P.histOut[1] = c->dTemporal + (2 * next + 1) * n;
	P.out = static_cast<float4*>(device_rgba_out);
	P.lenOut = history_len_out;
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.maxHistory = static_cast<float>(p.max_history);
	P.depthTolerance = p.depth_tolerance;
	P.normalCos = p.normal_cos;
	launch_temporal(P, L.s);
	return L.close();
}
