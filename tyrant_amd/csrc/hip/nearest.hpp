// nearest.hpp -- launch interface of the batched closest-point queries (hip/nearest.hip) for host/nearest.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct NearestParams {
	DevScene scene;
	const float* points;  // n x 3
	const float* maxDist; // n, or null: no bound
	float* dist2;         // n
	int32_t* prim;        // n
	float* uv;            // n x 2, or null
	uint8_t* region;      // n, or null
	float* point;         // n x 3, or null
	uint32_t* ticket;     // the launch's chunk ticket (zero at launch)
	uint32_t* error;      // the ctx's query error bits
	uint32_t n;
};

void launch_nearest(const NearestParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
