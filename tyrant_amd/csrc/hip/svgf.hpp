// svgf.hpp -- launch interface of the variance-guided spatiotemporal filter (hip/svgf.hip) for host/svgf.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument of every launch of one tyr_svgf call
struct SvgfParams {
	const float4* accum;  // W * H: rgb sums, a = sample count
	const float* albedo;  // x 3
	const float* normal;  // x 3
	const float* depth;
	const float2* motion;
	const float* prevDepth;
	// the last call's history: (u.xyz, n) with u pass 0's output, (normal.xyz, depth), (m1, m2); unread when !haveHistory
	const float4* histIn[2];
	const float2* histMomIn;
	float4* histOut[2];       // this call's
	float2* histMomOut;       // (m1, m2) of valid pixels, (0, -1) elsewhere
	float4* illum[2];         // ping-pong: (u.xyz, var) of valid pixels, (0, 0, 0, -1) elsewhere
	float4* out;              // the caller's frame
	float* varOut;            // or null
	uint32_t W, H;
	float maxHistory;
	float depthTolerance;
	float normalCos;
	float sl2;                // sigma_luminance^2
	float kz;                 // 1 / sigma_depth^2
	uint32_t normalPowerLog2;
	uint32_t passes;
	bool haveHistory;
	bool resolve;
};

void launch_svgf(const SvgfParams& P, hipStream_t stream);

} // namespace tyr
