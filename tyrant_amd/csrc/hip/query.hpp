// query.hpp -- launch interface of the batched ray queries (hip/query.hip) for host/query.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

constexpr uint32_t kQueryErrStackOverflow = 1u; // tyr_query_error bit 1: a traversal stack overflowed (bvh.h:124's 64 entries)

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct QueryParams {
	DevScene scene;
	tyr_sphere spheres[TYR_NUM_SPHERES];
	const float* origins;    // n x 3
	const float* directions; // n x 3
	const float* tmax;       // n, or null: VERY_FAR (kernel.cu:15)
	float* t;                // closest hit: n
	int32_t* prim;           // n
	int32_t* geom;           // n, or null
	float* uv;               // n x 2, or null
	uint8_t* occluded;       // any hit: n
	uint32_t* ticket;        // the launch's chunk ticket (zero at launch)
	uint32_t* error;         // the ctx's query error bits
	uint32_t n;
};

void launch_query(const QueryParams& P, bool any, bool spheres, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
