// sweep_capsule.hpp -- launch interface of the batched swept-capsule queries (hip/sweep_capsule.hip) for host/sweep_capsule.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct SweepCapsuleParams {
	DevScene scene;
	const float* p;          // n x 3
	const float* q;          // n x 3
	const float* directions; // n x 3
	const float* radius;     // n
	const float* tmax;       // n, or null: 1
	float* t;                // n
	int32_t* prim;           // n
	float* s;                // n, or null
	uint8_t* feature;        // n, or null
	uint8_t* region;         // n, or null
	float* point;            // n x 3, or null
	float* center;           // n x 3, or null
	float* normal;           // n x 3, or null
	uint32_t* ticket;        // the launch's chunk ticket (zero at launch)
	uint32_t* error;         // the ctx's query error bits
	uint32_t n;
};

void launch_sweep_capsule(const SweepCapsuleParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
