// occlusion.hpp -- launch interface of the batched ambient-occlusion queries (hip/occlusion.hip) for host/occlusion.cpp.
#pragma once

#include "kernels.hpp"
#include "query.hpp"

namespace tyr {

// by-value kernel argument of k_occlusion.  Every array is the caller's whole batch, in device memory, indexed with 64-bit
// offsets; a launch covers the `n / samples` points from `first` on.
struct OcclusionParams {
	DevScene scene;
	tyr_sphere spheres[TYR_NUM_SPHERES];
	const float* points;   // nPoints x 3
	const float* normals;  // nPoints x 3
	const float* maxDist;  // nPoints, or null: VERY_FAR (kernel.cu:15)
	uint32_t* visible;     // nPoints, zero at launch
	uint32_t* mask;        // nPoints x ((samples + 31) / 32), zero at launch, or null
	float* origin;         // nPoints x 3, or null
	float* direction;      // nPoints x samples x 3, or null
	uint32_t* ticket;      // the launch's chunk ticket (zero at launch)
	uint32_t* error;       // the ctx's query error bits
	uint32_t n;            // items of this launch: its points x samples, <= 2^31
	uint32_t samples;
	uint32_t first;        // index in the caller's batch of this launch's first point
	float bias;
	uint32_t seed;
};

// by-value kernel argument of k_occlusion_bent: one thread per point of the whole batch
struct OcclusionBentParams {
	const float* points;
	const float* normals;
	const uint32_t* mask;
	float* bent; // nPoints x 3
	uint32_t nPoints;
	uint32_t samples;
	float bias;
	uint32_t seed;
};

void launch_occlusion(const OcclusionParams& P, bool spheres, int numCUs, LaunchCache& lc, hipStream_t stream);
void launch_occlusion_bent(const OcclusionBentParams& P, hipStream_t stream);

} // namespace tyr
