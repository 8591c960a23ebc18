// segment.hpp -- launch interface of the batched closest-segment queries (hip/segment.hip) for host/segment.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct SegmentParams {
	DevScene scene;
	const float* p;       // n x 3
	const float* q;       // n x 3
	const float* maxDist; // n, or null: +inf
	float* dist2;         // n
	int32_t* prim;        // n
	float* s;             // n, or null
	uint8_t* feature;     // n, or null
	uint8_t* region;      // n, or null
	float* onSegment;     // n x 3, or null
	float* onTriangle;    // n x 3, or null
	uint32_t* ticket;     // the launch's chunk ticket (zero at launch)
	uint32_t* error;      // the ctx's query error bits
	uint32_t n;
};

void launch_segment(const SegmentParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
