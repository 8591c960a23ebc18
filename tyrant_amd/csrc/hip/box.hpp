// box.hpp -- launch interface of the batched box-overlap queries (hip/box.hip) for host/box.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct BoxParams {
	DevScene scene;
	const float* lo;   // n x 3
	const float* hi;   // n x 3
	uint32_t* count;   // n
	int32_t* prim;     // n x maxPrims: a box's row is its working buffer while the box is in flight; unused when maxPrims == 0
	uint32_t* ticket;  // the launch's chunk ticket (zero at launch)
	uint32_t* error;   // the ctx's query error bits
	uint32_t n;
	uint32_t maxPrims; // 0 .. TYR_QUERY_BOX_MAX; 0 with `any`
};

void launch_box(const BoxParams& P, bool any, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
