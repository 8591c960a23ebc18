// tri.hpp -- launch interface of the batched triangle-overlap queries (hip/tri.hip) for host/tri.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct TriParams {
	DevScene scene;
	const float* a;      // n x 3: the query triangles' corners
	const float* b;      // n x 3
	const float* c;      // n x 3
	uint32_t* count;     // n
	int32_t* prim;       // n x maxPrims: a query's row is its working buffer while the query is in flight; unused when maxPrims == 0
	uint32_t* ticket;    // the launch's chunk ticket (zero at launch)
	uint32_t* error;     // the ctx's query error bits
	uint32_t n;
	uint32_t maxPrims;   // 0 .. TYR_QUERY_TRI_MAX; 0 with `any`
	uint32_t skipShared; // TYR_QUERY_TRI_SKIP_SHARED: rule 0 of the member test applies
};

void launch_tri(const TriParams& P, bool any, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
