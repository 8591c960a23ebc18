// denoise.cpp -- tyr_denoise: the edge-avoiding a-trous filter of a frame guided by the AOV buffers (include/tyr_c.h
// "Denoiser"; the kernels are hip/denoise.hip).  Like a query it runs on the caller's stream and touches no render state; it
// needs no scene.  The scratch belongs to the ctx, so each call waits on its stream for the previous call's event: FilterLaunch,
// the bracket that all the frame passes share, is defined here.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../hip/denoise.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// the defaults (tyr_denoise_params NULL); how they were chosen: DESIGN.md "Denoiser", profiles/denoise_bench_c3.json
constexpr uint32_t kDefaultPasses = 5;
constexpr float kDefaultSigmaColor = 32.0f;
constexpr float kDefaultSigmaDepth = 0.02f;
constexpr uint32_t kDefaultNormalPowerLog2 = 7;

// 1 / (sigma * sigma) in float32, or 0 when sigma is not positive and finite or the result is not finite
float inv_square(float sigma) {
	if (!positive_finite(sigma))
		return 0.f;
	const float sq = sigma * sigma;
	const float k = 1.0f / sq;
	return std::isfinite(k) ? k : 0.f;
}

} // namespace

namespace tyr {
namespace drv {

int FilterLaunch::open(tyr_ctx* c, FilterState& state, void* stream) {
	if (int rc = scope.enter(c))
		return rc;
	st = &state;
	if (!st->done)
		HIPCHK(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
	s = stream ? static_cast<hipStream_t>(stream) : c->stream;
	HIPCHK(hipStreamWaitEvent(s, st->done, 0));
	return TYR_OK;
}

int FilterLaunch::close() {
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(st->done, s));
	if (pingPong) {
		st->cur = next;
		st->have = true;
	}
	return TYR_OK;
}

void filters_free(tyr_ctx* c) {
	for (FilterState* st : { &c->denoise, &c->temporal, &c->svgf, &c->taa, &c->alloc }) {
		if (st->done) {
			(void)hipEventSynchronize(st->done);
			(void)hipEventDestroy(st->done);
		}
		*st = FilterState{};
	}
	dev_free(c->dDenoise);
	dev_free(c->dTemporal);
	dev_free(c->dSvgfHist);
	dev_free(c->dSvgfMom);
	dev_free(c->dSvgfIllum);
	dev_free(c->dTaaHist);
	dev_free(c->dAllocScratch);
}

bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

bool reprojection_ok(uint32_t maxHistory, float depthTolerance, float normalCos) {
	return maxHistory >= 1 && maxHistory <= kMaxHistory && positive_finite(depthTolerance) && normalCos >= -1.f && normalCos <= 1.f;
}

} // namespace drv
} // namespace tyr

int tyr_denoise(tyr_ctx* c, const tyr_denoise_in* in, const tyr_denoise_params* params, void* device_rgba_out, void* stream) {
	if (!c || !in || !in->albedo || !in->normal || !in->depth || !device_rgba_out)
		return TYR_ERR_INVALID;
	tyr_denoise_params p{ kDefaultPasses, kDefaultSigmaColor, kDefaultSigmaDepth, kDefaultNormalPowerLog2, 0u };
	if (params)
		p = *params;
	if (p.passes < 1 || p.passes > kMaxPasses || p.normal_power_log2 > kMaxNormalPowerLog2 || (p.flags & ~TYR_DENOISE_RESOLVE) != 0u)
		return TYR_ERR_INVALID;
	const float kc = inv_square(p.sigma_color), kz = inv_square(p.sigma_depth);
	if (kc == 0.f || kz == 0.f || !std::isfinite(kc * static_cast<float>(1u << (2u * (p.passes - 1u)))))
		return TYR_ERR_INVALID;
	const float4* accum = in->accum ? reinterpret_cast<const float4*>(in->accum) : c->blit;
	if (!accum)
		return TYR_ERR_NO_BUFFER;
	FilterLaunch L;
	if (int rc = L.open(c, c->denoise, stream))
		return rc;
	const size_t n = static_cast<size_t>(c->cfg.width) * c->cfg.height;
	if (int rc = L.buffer(c->dDenoise, 3 * n))
		return rc;

	DenoiseParams P{};
	P.accum = accum;
	P.albedo = in->albedo;
	P.normal = in->normal;
	P.depth = in->depth;
	P.illum[0] = c->dDenoise;
	P.illum[1] = c->dDenoise + n;
	P.guide = c->dDenoise + 2 * n;
	P.out = static_cast<float4*>(device_rgba_out);
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.kc = kc;
	P.kz = kz;
	P.normalPowerLog2 = p.normal_power_log2;
	P.passes = p.passes;
	P.resolve = (p.flags & TYR_DENOISE_RESOLVE) != 0u;
	launch_denoise(P, L.s);
	return L.close();
}
