// denoise.hpp -- launch interface of the a-trous denoiser (hip/denoise.hip) for host/denoise.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument of every launch of one tyr_denoise call
struct DenoiseParams {
	const float4* accum;  // W * H: rgb sums, a = sample count
	const float* albedo;  // x 3
	const float* normal;  // x 3
	const float* depth;
	float4* illum[2];     // ping-pong: (u.xyz, state) with state 1 valid, -1 background, 0 no sample (A == 0)
	float4* guide;        // (n.xyz, depth)
	float4* out;          // the caller's frame
	uint32_t W, H;
	float kc;             // 1 / sigma_color^2: pass j uses kc * 4^j
	float kz;             // 1 / sigma_depth^2
	uint32_t normalPowerLog2;
	uint32_t passes;
	bool resolve;
};

void launch_denoise(const DenoiseParams& P, hipStream_t stream);

} // namespace tyr
