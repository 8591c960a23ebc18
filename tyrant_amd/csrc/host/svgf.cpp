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
constexpr uint32_t kMaxHistory = 1024, kMaxPasses = 8, kMaxNormalPowerLog2 = 10;

bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

} // namespace

namespace tyr {
namespace drv {

void svgf_free(tyr_ctx* c) {
	if (c->svgfDone) {
		(void)hipEventSynchronize(c->svgfDone);
		(void)hipEventDestroy(c->svgfDone);
		c->svgfDone = nullptr;
	}
	dev_free(c->dSvgfHist);
	dev_free(c->dSvgfMom);
	dev_free(c->dSvgfIllum);
	c->svgfHave = false;
}

} // namespace drv
} // namespace tyr

int tyr_svgf(tyr_ctx* c, const tyr_svgf_in* in, const tyr_svgf_params* params, void* device_rgba_out, float* variance_out, void* stream) {
	if (!c || !in || !in->albedo || !in->normal || !in->depth || !in->motion || !in->prev_depth || !device_rgba_out)
		return TYR_ERR_INVALID;
	tyr_svgf_params p{ kDefaultMaxHistory, kDefaultDepthTolerance, kDefaultNormalCos, kDefaultPasses, kDefaultSigmaLuminance, kDefaultSigmaDepth, kDefaultNormalPowerLog2, 0u };
	if (params)
		p = *params;
	if (p.max_history < 1 || p.max_history > kMaxHistory || !positive_finite(p.depth_tolerance) || !(p.normal_cos >= -1.f && p.normal_cos <= 1.f) || p.passes < 1 ||
	    p.passes > kMaxPasses || p.normal_power_log2 > kMaxNormalPowerLog2 || (p.flags & ~(TYR_SVGF_RESET | TYR_SVGF_RESOLVE)) != 0u)
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
	DeviceScope scope;
	if (int rc = scope.enter(c))
		return rc;
	const size_t n = static_cast<size_t>(c->cfg.width) * c->cfg.height;
	if (!c->dSvgfHist || !c->dSvgfMom || !c->dSvgfIllum) {
		c->svgfHave = false;
		if (!c->dSvgfHist)
			if (int rc = dev_alloc(c->dSvgfHist, 4 * n))
				return rc;
		if (!c->dSvgfMom)
			if (int rc = dev_alloc(c->dSvgfMom, 2 * n))
				return rc;
		if (!c->dSvgfIllum)
			if (int rc = dev_alloc(c->dSvgfIllum, 2 * n))
				return rc;
	}
	if (!c->svgfDone)
		HIPCHK(hipEventCreateWithFlags(&c->svgfDone, hipEventDisableTiming));
	const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
	HIPCHK(hipStreamWaitEvent(s, c->svgfDone, 0)); // the previous call's history and scratch (a no-op before the first record)

	const uint32_t prev = c->svgfCur, next = prev ^ 1u;
	SvgfParams P{};
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
	P.haveHistory = c->svgfHave && (p.flags & TYR_SVGF_RESET) == 0u;
	P.resolve = (p.flags & TYR_SVGF_RESOLVE) != 0u;
	launch_svgf(P, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(c->svgfDone, s));
	c->svgfCur = next;
	c->svgfHave = true;
	return TYR_OK;
}
