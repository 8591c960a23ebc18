// temporal.hpp -- launch interface of the motion-vector pass and the temporal reprojection (hip/temporal.hip) for
// host/temporal.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument of tyr_render_motion.  The frame, sharding and camera fields carry FrameParams' names:
// camera_seed / camera_focus / camera_lens (hip/device_common.hpp) read them from this struct too.
struct MotionParams {
	const float4* tris;    // the uploaded triangles, 3 float4 each (DevScene::tris)
	uint32_t nPrims;
	tyr_sphere spheres[TYR_NUM_SPHERES];
	uint32_t W, H;
	uint32_t rank, nranks;
	uint32_t localRows;
	uint32_t frame;
	float camPos[3], camDir[3], camRight[3], camUp[3];
	float focalDistance, lensRadius;
	float camFF, camRR, camUU;    // F.F, R.R, U.U of the current camera (float32 on the host)
	float prevPos[3], prevDir[3], prevRight[3], prevUp[3];
	float prevFF, prevRR, prevUU; // ... and of the previous one
	const int32_t* prim;   // full frame (y * W + x): tyr_render_aov's sample-0 identity
	const int32_t* geom;
	const float* prevPrims; // 10 floats per 40-byte tyr_triangle record, or null: the geometry did not move
	float* motion;          // x 2, or null
	float* prevDepth;       // or null
};

// by-value kernel argument of tyr_temporal
struct TemporalParams {
	const float4* accum;  // W * H: rgb sums, a = sample count
	const float* albedo;  // x 3
	const float* normal;  // x 3
	const float* depth;
	const float2* motion;
	const float* prevDepth;
	const float4* histIn[2];  // the last call's history: (u.xyz, n), (normal.xyz, depth); unread when !haveHistory
	float4* histOut[2];       // this call's
	float4* out;              // the caller's frame
	float* lenOut;            // or null
	uint32_t W, H;
	float maxHistory;
	float depthTolerance;
	float normalCos;
	bool haveHistory;
};

void launch_motion(const MotionParams& P, hipStream_t stream);
void launch_motion_chain(const MotionParams& P, const int32_t* chain, const float* length0, hipStream_t stream); // full-frame, as prim / geom
void launch_temporal(const TemporalParams& P, hipStream_t stream);

} // namespace tyr
