// svgf.cpp -- tyr_svgf: the variance-guided spatiotemporal filter of a frame (include/tyr_c.h "SVGF"; the kernels are
// hip/svgf.hip).  It behaves like tyr_temporal (host/temporal.cpp): it needs no scene and touches no render state, and since
// the history and the scratch belong to the ctx, each call waits on its stream for the previous call's event.  Its history is
// its own: tyr_temporal's history and tyr_denoise's scratch are neither read nor written.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../hip/svgf.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// the defaults (tyr_svgf_params NULL); how they were chosen: DESIGN.md "SVGF", profiles/svgf_bench_c3.json
constexpr uint32_t kDefaultMaxHistory = 8;
constexpr float kDefaultDepthTolerance = 0.05f;
constexpr float kDefaultNormalCos = 0.9f;
constexpr uint32_t kDefaultPasses = 3;
constexpr float kDefaultSigmaLuminance = 2.0f;
constexpr float kDefaultSigmaDepth = 0.02f;
constexpr uint32_t kDefaultNormalPowerLog2 = 7;

} // namespace

int tyr_svgf(tyr_ctx* c, const tyr_svgf_in* in, const tyr_svgf_params* params, void* device_rgba_out, float* variance_out, void* stream) {
	if (!c || !in || !in->albedo || !in->normal || !in->depth || !in->motion || !in->prev_depth || !device_rgba_out)
		return TYR_ERR_INVALID;
	tyr_svgf_params p{ kDefaultMaxHistory, kDefaultDepthTolerance, kDefaultNormalCos, kDefaultPasses, kDefaultSigmaLuminance, kDefaultSigmaDepth, kDefaultNormalPowerLog2, 0u };
	if (params)
		p = *params;
	if (!reprojection_ok(p.max_history, p.depth_tolerance, p.normal_cos) || p.passes < 1 || p.passes > kMaxPasses || p.normal_power_log2 > kMaxNormalPowerLog2 ||
	    (p.flags & ~(TYR_SVGF_RESET | TYR_SVGF_RESOLVE)) != 0u)
		return TYR_ERR_INVALID;
	if (!positive_finite(p.sigma_luminance) || !positive_finite(p.sigma_depth))
		return TYR_ERR_INVALID;
	const float sl2 = p.sigma_luminance * p.sigma_luminance;
	const float sz2 = p.sigma_depth * p.sigma_depth;
	const float kz = 1.0f / sz2;
	if (!positive_finite(sl2) || !positive_finite(kz))
		return TYR_ERR_INVALID;
	const float4* accum = in->accum ? reinterpret_cast<const float4*>(in->accum) : c->blit;
	if (!accum)
		return TYR_ERR_NO_BUFFER;
	FilterLaunch L;
	if (int rc = L.open(c, c->svgf, stream))
		return rc;
	const size_t n = static_cast<size_t>(c->cfg.width) * c->cfg.height;
	// (a call that fails part of the way keeps what it allocated: the next one completes it, and starts without a history)
	if (int rc = L.buffer(c->dSvgfHist, 4 * n))
		return rc;
	if (int rc = L.buffer(c->dSvgfMom, 2 * n))
		return rc;
	if (int rc = L.buffer(c->dSvgfIllum, 2 * n))
		return rc;

	SvgfParams P{};
	P.haveHistory = L.history((p.flags & TYR_SVGF_RESET) != 0u);
	const uint32_t prev = L.prev, next = L.next;
	P.accum = accum;
	P.albedo = in->albedo;
	P.normal = in->normal;
	P.depth = in->depth;
	P.motion = reinterpret_cast<const float2*>(in->motion);
	P.prevDepth = in->prev_depth;
	P.histIn[0] = c->dSvgfHist + 2 * prev * n;
	P.histIn[1] = c->dSvgfHist + (2 * prev + 1) * n;
	P.histMomIn = c->dSvgfMom + prev * n;
	P.histOut[0] = c->dSvgfHist + 2 * next * n;
	P.histOut[1] = c->dSvgfHist + (2 * next + 1) * n;
	P.histMomOut = c->dSvgfMom + next * n;
	P.illum[0] = c->dSvgfIllum;
	P.illum[1] = c->dSvgfIllum + n;
	P.out = static_cast<float4*>(device_rgba_out);
	P.varOut = variance_out;
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.maxHistory = static_cast<float>(p.max_history);
	P.depthTolerance = p.depth_tolerance;
	P.normalCos = p.normal_cos;
	P.sl2 = sl2;
	P.kz = kz;
	P.normalPowerLog2 = p.normal_power_log2;
	P.passes = p.passes;
	P.resolve = (p.flags & TYR_SVGF_RESOLVE) != 0u;
	launch_svgf(P, L.s);
	return L.close();
}
