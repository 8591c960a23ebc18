// adaptive.hpp -- launch interface of adaptive sampling (hip/adaptive.hip) for host/adaptive.cpp: the build of a sample map's
// ticket list, and the allocator that turns an error estimate into a sample map.  (The camera-ray kernel that reads the list is
// one of primary_rays' kernels: hip/frame.hip k_primary_mapped, hip/kernels.hpp launch_primary_mapped.)
#pragma once

#include "kernels.hpp"

namespace tyr {

// where the map of one tyr_set_sample_map call is read and what its first pass leaves for the host
struct SampleMapArgs {
	const uint32_t* map;  // width * height, indexed y * W + x
	uint32_t W, localRows, rank, nranks;
	uint32_t* counts;     // [localPixels]: the map at the ctx's local pixels
	uint32_t* summary;    // [kMapSummaryWords + kMaxSpp + 1]: T (two words, low first), the largest count, a bad-value flag, then hist[v]
};
constexpr uint32_t kMaxSpp = 65535u;
constexpr uint32_t kMapSummaryWords = 4u;
constexpr uint32_t kCompactTile = 1024u; // elements per block of the list build's compaction (256 threads x 4 rounds)

void launch_map_hist(const SampleMapArgs& A, uint32_t localPixels, hipStream_t stream);
// pass s of L from the list `in` (nullptr: the local pixels 0 .. n - 1 in order) of n entries: the stable compaction by
// counts[p] > s, written at out.  blockCnt: ceil(n / kCompactTile) words of scratch.  outLimit: room at out (a guard).
void launch_pass_compact(const uint32_t* in, uint32_t n, const uint32_t* counts, uint32_t s, uint32_t* out, uint32_t outLimit, uint32_t* blockCnt, hipStream_t stream);
// `copies` more copies of the n-entry pass at list + src, written from list + dst on (passes that no count ends in between)
void launch_pass_repeat(uint32_t* list, uint32_t src, uint32_t n, uint32_t dst, uint32_t copies, uint32_t total, hipStream_t stream);
// passes sFirst .. maxSpp - 1 of L in one block, from pass sFirst - 1 (nIn < kCompactTile entries at in)
void launch_pass_tail(uint32_t* list, const uint32_t* in, uint32_t nIn, const uint32_t* counts, uint32_t sFirst, uint32_t maxSpp, uint32_t outOff, uint32_t total, hipStream_t stream);

// tyr_allocate_samples (include/tyr_c.h): one max-reduction, the quantised weights' 64-bit inclusive scan, the extras
struct AllocateArgs {
	const float* error;      // width * height, indexed y * W + x
	uint32_t* mapOut;        // width * height (only the ctx's rows are written)
	uint32_t W, localRows, rank, nranks, localPixels;
	uint32_t minSpp, maxSpp;
	uint32_t extra;          // E = total - min_spp * P when that is positive, else 0
	unsigned long long* scan;      // [localPixels]: the inclusive scan of the weights inside each kCompactTile block
	unsigned long long* blockSum;  // [ceil(localPixels / kCompactTile)]: the blocks' totals, then their exclusive prefixes
	uint32_t* maxBits;             // the largest usable error's bits (a non-negative float: its bits order like the value)
	unsigned long long* totalOut;  // sum of the map written
};
void launch_allocate(const AllocateArgs& A, hipStream_t stream);

} // namespace tyr
