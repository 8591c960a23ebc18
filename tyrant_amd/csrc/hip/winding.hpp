// winding.hpp -- launch interface of the winding-number queries (hip/winding.hip) for host/winding.cpp, and the moment tree a
// TYR_FLAG_WINDING upload keeps beside the scene (include/tyr_c.h "Winding numbers").
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../../include/tyr_c.h"

namespace tyr {

// One record per node of the reference's node array, in its order: everything a lane of k_winding reads of a node, as four
// 16-byte loads of one 64-byte line.  a / b: a leaf's first primitive and primitive count; an interior node's skip -- the index
// behind its subtree -- and 0.  (A leaf's skip is the next index: the array is depth-first, so it needs no word of its own.)
struct alignas(64) WindingNode {
	double p[3]; // the expansion centre
	double N[3]; // the summed area vector
	double r2;   // the squared reach of the node's box from p
	uint32_t a, b;
};
static_assert(sizeof(WindingNode) == 64, "k_winding reads a node as four dwordx4");

// What an upload with TYR_FLAG_WINDING leaves on the device (owned by the ctx; host/winding.cpp)
struct WindingTree {
	WindingNode* nodes = nullptr;
	double* S = nullptr; // per node: the summed area (tyr_scene_moments reports it; the query does not read it)
	int32_t nNodes = 0;
	size_t bytes = 0;    // device memory of the above (tyr_scene_info.device_bytes)
};

// by-value kernel argument of the build's passes
struct WindingBuildArgs {
	const tyr_bvh_node* src; // the reference's node array, device
	const float4* tris;      // the ctx's triangle records, 3 x float4 each, array order
	int32_t nNodes;
	uint32_t nPrims;
	WindingNode* nodes;
	double* S;
	int32_t* parent;             // scratch, nNodes, all -1 at launch
	uint32_t* arrived;           // scratch, nNodes, zero at launch
	unsigned long long* moments; // scratch, nNodes x 8 words: N xyz, S, M xyz as binary64 bits
};

// by-value kernel argument of k_winding; every array is the caller's whole batch, in device memory
struct WindingParams {
	const WindingNode* nodes;
	const float4* tris;
	const float* points; // n x 3
	float* w;            // n
	uint32_t* terms;     // n x 2, or null
	uint32_t n;
	int32_t nNodes;
	float accuracy;
};

// parents, then leaves and the walk to the root; all on `stream`, which the caller drains
void launch_winding_build(const WindingBuildArgs& A, hipStream_t stream);
void launch_winding(const WindingParams& P, hipStream_t stream);

} // namespace tyr
