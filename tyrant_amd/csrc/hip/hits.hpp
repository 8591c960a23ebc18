// hits.hpp -- launch interface of the batched multi-hit ray queries (hip/hits.hip) for host/hits.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct HitsParams {
	DevScene scene;
	const float* origins;    // n x 3
	const float* directions; // n x 3
	const float* tmax;       // n, or null: VERY_FAR (kernel.cu:15)
	uint32_t* count;         // n
	float* t;                // n x maxHits: a ray's row is its k-buffer while the ray is in flight
	int32_t* prim;           // n x maxHits: likewise
	float* uv;               // n x maxHits x 2, or null
	uint8_t* side;           // n x maxHits, or null
	uint32_t* backCount;     // n, or null
	uint32_t* ticket;        // the launch's chunk ticket (zero at launch)
	uint32_t* error;         // the ctx's query error bits
	uint32_t n;
	uint32_t maxHits;        // 1 .. TYR_QUERY_HITS_MAX
};

void launch_hits(const HitsParams& P, bool twoSided, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
