// taa.hpp -- launch interface of temporal anti-aliasing (hip/taa.hip) for host/taa.cpp.
#pragma once

#include "kernels.hpp"

namespace tyr {

// by-value kernel argument of the one launch of a tyr_taa call
struct TaaParams {
	const float4* color;   // W * H: the resolved frame, a != 0 on pixels that were seen
	const float* depth;
	const float2* motion;
	const float* prevDepth;
	const float4* histIn;  // the last call's output (rgb, validity 1 / 0); unread when !haveHistory
	float4* histOut;       // this call's
	float4* out;           // the caller's frame, or null (in place: the host copies histOut over it behind the launch)
	uint32_t W, H;
	float alpha;
	float gamma;
	bool haveHistory;
	bool bilinear;
};

void launch_taa(const TaaParams& P, hipStream_t stream);

} // namespace tyr
