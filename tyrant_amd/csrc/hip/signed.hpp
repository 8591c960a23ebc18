// signed.hpp -- launch interface of the signed-distance queries and the SDF grid bake (hip/signed.hip) for host/signed.cpp.
#pragma once

#include "kernels.hpp"
#include "winding.hpp"

namespace tyr {

// by-value kernel argument of k_query_signed.  Every array is the caller's, in device memory, indexed with 64-bit offsets.
struct SignedParams {
	DevScene scene;
	const WindingNode* wnodes; // the ctx's moment tree
	const float* points;       // n x 3
	const float* maxDist;      // n, or null: no bound
	float* sd;                 // n
	int32_t* prim;             // n, or null
	float* point;              // n x 3, or null
	float* gradient;           // n x 3, or null
	float* w;                  // n, or null
	uint32_t* ticket;          // the launch's chunk ticket (zero at launch)
	uint32_t* error;           // the ctx's query error bits
	uint32_t n;
	int32_t nWNodes; // 0: a scene without triangles, every w = 0
	float accuracy;
};

// by-value kernel argument of the bake's two launches
struct SdfParams {
	DevScene scene;
	const WindingNode* wnodes;
	float* sd;          // nz * ny * nx, x fastest
	int32_t* prim;      // the same shape, or null
	uint32_t* stats;    // 2, or null: near bricks, far bricks
	uint32_t* nearList; // the ctx's scratch: word 0 the number of near bricks (zero at the first launch), then their indices
	uint32_t* ticket;   // the launch's ticket (zero at launch)
	uint32_t* error;
	float origin[3];
	float cell, band, reach, accuracy;
	uint32_t dims[3];   // voxels per axis
	uint32_t bricks[3]; // bricks per axis
	uint32_t nBricks;
	int32_t nWNodes;
};

void launch_signed(const SignedParams& P, int numCUs, LaunchCache& lc, hipStream_t stream);
void launch_sdf_bricks(const SdfParams& P, int numCUs, LaunchCache& lc, hipStream_t stream); // far / near per brick, far bricks filled
void launch_sdf_voxels(const SdfParams& P, int numCUs, LaunchCache& lc, hipStream_t stream); // the near bricks' voxels; needs the first launch's list

} // namespace tyr
