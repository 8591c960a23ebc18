// tri_distance.hpp -- launch interface of the batched closest-triangle distance queries (hip/tri_distance.hip) for
// host/tri_distance.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct TriDistanceParams {
	DevScene scene;
	const float* a;       // n x 3
	const float* b;       // n x 3
	const float* c;       // n x 3
	const float* maxDist; // n, or null: +inf
	float* dist2;         // n
	int32_t* prim;        // n
	uint8_t* feature;     // n, or null
	uint8_t* region;      // n, or null
	float* onQuery;       // n x 3, or null
	float* onTriangle;    // n x 3, or null
	uint32_t* ticket;     // the launch's chunk ticket (zero at launch)
	uint32_t* error;      // the ctx's query error bits
	uint32_t n;
	uint32_t skipShared;  // TYR_QUERY_TRI_SKIP_SHARED: a scene triangle with a corner equal to one of the query's is no candidate
};

void launch_tri_distance(const TriDistanceParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
