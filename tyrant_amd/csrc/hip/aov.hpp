// aov.hpp -- launch interface of the first-hit AOV pass (hip/aov.hip) for host/aov.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument.  The frame, sharding and camera fields carry FrameParams' names: camera_seed / camera_focus /
// camera_lens (hip/device_common.hpp) read them from either struct.
struct AovParams {
	DevScene scene;
	tyr_sphere spheres[TYR_NUM_SPHERES];
	uint32_t W, H;
	uint32_t rank, nranks;
	uint32_t localRows;
	uint32_t frame;
	float camPos[3], camDir[3], camRight[3], camUp[3];
	float focalDistance, lensRadius;
	const float4* palette; // TYR_FLAG_TRIANGLE_COLORS: a triangle's albedo is its palette colour; null: (1, 1, 1)
	// full-frame outputs (y * W + x), each optional
	float* albedo;         // x 3
	float* normal;         // x 3
	float* depth;
	int32_t* prim;
	int32_t* geom;
	uint32_t* ticket;      // the launch's chunk ticket (zero at launch)
	uint32_t* error;       // the ctx's query error bits
	uint32_t nPixels;      // W * localRows: the ctx's own pixels
	uint32_t spp;          // spp * nPixels < 2^32
};

// by-value kernel argument of the specular-chain pass (tyr_render_aov_chain): the first-hit pass's, and what the chain adds
struct AovChainParams {
	AovParams a;           // albedo, normal, depth: of the surface the chain ends on; prim, geom: sample 0's first hit
	int32_t* chain;        // full-frame outputs of sample 0, each optional: specular bounces followed
	int32_t* endPrim;      // identity of the surface it ended on (-1 / -1: it left the scene)
	int32_t* endGeom;
	float* length0;        // its summed path length (VERY_FAR: it left the scene)
	float* depthFirst;     // the first-hit pass's depth
	uint32_t maxChain;     // 0 .. TYR_AOV_CHAIN_MAX
	uint32_t triMaterials; // TYR_FLAG_TRIANGLE_MATERIALS: a triangle's material is its record's, else DIFF
};

void launch_aov(const AovParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);
void launch_aov_chain(const AovChainParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);

} // namespace tyr
