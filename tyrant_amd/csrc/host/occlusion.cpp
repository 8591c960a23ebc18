// occlusion.cpp -- tyr_query_occlusion: batched ambient-occlusion queries on the ctx's scene (include/tyr_c.h "Occlusion
// queries"; the kernels are hip/occlusion.hip).  A query like those of host/query.cpp and host/hits.cpp: it reads and writes no
// render state, runs on the caller's stream and goes through the same per-stream bookkeeping (QueryLaunch: the stream's chunk
// ticket and its `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for).
//
// A work item is a (point, sample) pair with a 32-bit index, so a batch goes out as launches of whole points with at most 2^31
// items each -- one launch for every batch below 2^31 / samples points.  The counts and mask words are cleared on the stream in
// front of the first launch: the kernel only ever adds to them.
#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../hip/occlusion.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

int tyr_query_occlusion(tyr_ctx* c, uint32_t n, const float* points, const float* normals, const float* max_dist, uint32_t samples, float bias, uint32_t seed, uint32_t flags,
                        const tyr_occlusion_out* out, void* stream) {
	if (!c || n >= (1u << 31) || (flags & ~TYR_QUERY_SPHERES) != 0u || samples == 0u || samples > TYR_QUERY_OCCLUSION_MAX_SAMPLES || !std::isfinite(bias))
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!points || !normals || !out || !out->visible || (out->bent && !out->mask))
		return TYR_ERR_INVALID;

	OcclusionParams P{};
	P.points = points;
	P.normals = normals;
	P.maxDist = max_dist;
	P.visible = out->visible;
	P.mask = out->mask;
	P.origin = out->origin;
	P.direction = out->direction;
	P.samples = samples;
	P.bias = bias;
	P.seed = seed;

	const size_t words = (samples + 31u) / 32u;
	const uint32_t pointsPerLaunch = (1u << 31) / samples; // whole points, at most 2^31 items
	QueryLaunch L;
	for (uint32_t first = 0; first < n; first += pointsPerLaunch) {
		if (int rc = L.open(c, stream)) // (every launch: its ticket word is zero when it starts)
			return rc;
		if (first == 0) {
			HIPCHK(hipMemsetAsync(out->visible, 0, static_cast<size_t>(n) * sizeof(uint32_t), L.s));
			if (out->mask)
				HIPCHK(hipMemsetAsync(out->mask, 0, static_cast<size_t>(n) * words * sizeof(uint32_t), L.s));
		}
		query_fields(P, c, L);
		P.first = first;
		P.n = std::min(pointsPerLaunch, n - first) * samples;
		launch_occlusion(P, (flags & TYR_QUERY_SPHERES) != 0u, c->numCUs, c->launchCache, L.s);
		if (int rc = L.close())
			return rc;
	}
	if (out->bent) {
		OcclusionBentParams B{};
		B.points = points;
		B.normals = normals;
		B.mask = out->mask;
		B.bent = out->bent;
		B.nPoints = n;
		B.samples = samples;
		B.bias = bias;
		B.seed = seed;
		launch_occlusion_bent(B, L.s);
		return L.close(); // (a record of its own: `done` has to lie behind this pass too)
	}
	return TYR_OK;
}
