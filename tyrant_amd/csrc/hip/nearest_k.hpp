// nearest_k.hpp -- launch interface of the batched k-nearest / within-radius queries (hip/nearest_k.hip) for host/nearest_k.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct NearestKParams {
	DevScene scene;
	const float* points;  // n x 3
	const float* maxDist; // n, or null: no bound
	float* dist2;         // n x k: a point's row is its k-buffer while the point is in flight
	int32_t* prim;        // n x k: likewise
	uint32_t* count;      // n, or null (then the kernel without a counter runs)
	float* uv;            // n x k x 2, or null
	uint8_t* region;      // n x k, or null
	float* point;         // n x k x 3, or null
	uint32_t* ticket;     // the launch's chunk ticket (zero at launch)
	uint32_t* error;      // the ctx's query error bits
	uint32_t n;
	uint32_t k;           // 1 .. TYR_QUERY_NEAREST_K_MAX
};

void launch_nearest_k(const NearestKParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
