// query_common.hpp -- the pieces of the persistent ray-query loop (hip/query.hip) that the AOV pass (hip/aov.hip) shares:
// its launch constants, the wave's lane-state ballots and the chunked ticket feed.
#pragma once

#include "device_common.hpp"

namespace tyr {

constexpr int kQueryStackLds = 12;  // LDS stack entries per lane: 24,576 B (closest) + 7,168 B staged nodes, five blocks per CU
constexpr uint32_t kQueryMinTraversing = 32; // leave the descent below this many descending lanes when leaves or a refill wait
constexpr uint32_t kQueryRefillMinIdle = 16; // refill a wave once this many lanes are free

__device__ __forceinline__ bool q_is_leaf(uint32_t ref) { return (ref & kRefLeaf) && ref < kRefPop; }
__device__ __forceinline__ unsigned long long q_traversing(uint32_t ref) { return __builtin_amdgcn_ballot_w64((int)ref >= 0) | __builtin_amdgcn_ballot_w64(ref == kRefPop); }
__device__ __forceinline__ unsigned long long q_at_leaf(uint32_t ref) { return __builtin_amdgcn_ballot_w64((ref & kRefLeaf) != 0u) & __builtin_amdgcn_ballot_w64(ref < kRefPop); }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff(); }

// one wave's private range of ray indices [next, end), drawn `chunk` rays at a time from the launch's ticket word
struct QueryFeed {
	uint32_t next, end, chunk;
	__device__ __forceinline__ void init(uint32_t n) {
		next = end = 0;
		// small batches: smaller chunks, so that the rays spread over more waves (never below one wave's worth)
		const uint32_t waves = gridDim.x * (blockDim.x / 64u);
		chunk = 256;
		while (chunk > 64 && (unsigned long long)waves * chunk > n)
			chunk >>= 1;
	}
	// false once the batch is used up
	__device__ __forceinline__ bool draw(uint32_t* ticket, uint32_t n, uint32_t lane) {
		uint32_t t = 0;
		if (lane == 0)
			t = atomicAdd(ticket, 1u);
		t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
		const unsigned long long start = (unsigned long long)t * chunk;
		if (start >= n)
			return false;
		next = (uint32_t)start;
		end = (start + chunk < n) ? (uint32_t)(start + chunk) : n;
		return true;
	}
};


} // namespace tyr
