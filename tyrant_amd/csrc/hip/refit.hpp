// refit.hpp -- launch interface of the BVH refit (hip/refit.hip) for host/refit.cpp, and the plan a TYR_FLAG_REFIT upload keeps.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../../include/tyr_c.h"

namespace tyr {

constexpr uint32_t kRefitRangeNodes = 2048; // a subtree of at most this many nodes is refitted by one block, in LDS
constexpr uint32_t kRefitErrNonFinite = 1u; // the validate pass's error bits
constexpr uint32_t kRefitErrMaterial = 2u;

// What an upload with TYR_FLAG_REFIT leaves on the device (all hipMalloc'ed, owned by the ctx; host/refit.cpp):
//   nodes     the reference's node array as uploaded (after a refit: with the refitted boxes)
//   slotNode  per quad slot (record * 4 + slot) the node whose box the slot holds; -1: an empty slot or a synthetic chain's
//             everythingBox, which a refit never writes
//   pairNode  per pair side (pair * 2 + side) the node whose box it holds (only when the ctx keeps pair nodes)
//   ranges    the cut: subtrees of at most kRefitRangeNodes nodes, { begin, end, height of begin, 0 }
//   height    per node: 0 for a leaf, else 1 + the larger height of its children (range nodes only: below kRefitRangeNodes)
//   top       the nodes above the cut, by height then index; topLevel[l] .. topLevel[l + 1] = those of the l-th height
//   err       the validate pass's error word
struct RefitPlan {
	tyr_bvh_node* nodes = nullptr;
	int32_t* slotNode = nullptr;
	int32_t* pairNode = nullptr;
	uint4* ranges = nullptr;
	uint16_t* height = nullptr;
	int32_t* top = nullptr;
	uint32_t* topLevel = nullptr;
	uint32_t* err = nullptr;
	int32_t nNodes = 0;
	uint32_t nSlots = 0, nPairSides = 0, nRanges = 0, nTop = 0, nTopLevels = 0;
	size_t bytes = 0; // device memory of all of the above (tyr_scene_info.device_bytes)
};

// by-value kernel argument
struct RefitArgs {
	const tyr_triangle* prims; // n records, device
	const tyr_bbox* bboxes;    // n boxes, device, or null: the boxes of tyr_triangle_bboxes's rule
	int32_t n;
	tyr_bvh_node* nodes;
	const uint16_t* height;
	const uint4* ranges;
	const int32_t* top;
	const uint32_t* topLevel;
	uint32_t nTopLevels;
	const int32_t* slotNode;
	uint32_t nSlots;
	const int32_t* pairNode;
	uint32_t nPairSides;
	float4* quads; // the ctx's records
	float4* pairs;
	float4* tris;
	uint32_t* err;
};

// validate pass: error bits to A.err (zeroed by the caller); nothing else is written
void launch_refit_validate(const RefitArgs& A, hipStream_t stream);
// the refit itself: triangles, subtrees, top, scatter into the records (A.err must have come back zero)
void launch_refit(const RefitArgs& A, uint32_t nRanges, hipStream_t stream);

} // namespace tyr
