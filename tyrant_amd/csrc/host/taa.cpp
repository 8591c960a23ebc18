// taa.cpp -- tyr_taa: temporal anti-aliasing of a resolved frame (include/tyr_c.h "Temporal anti-aliasing"; the kernel is
// hip/taa.hip).  It behaves like tyr_svgf (host/svgf.cpp): it needs no scene and touches no render state, and since the
// history belongs to the ctx, each call waits on its stream for the previous call's event.  Its history is its own: the
// histories and scratch of tyr_temporal, tyr_svgf and tyr_denoise are neither read nor written.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../hip/taa.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

// the defaults (tyr_taa_params NULL); how they were chosen: DESIGN.md "Temporal anti-aliasing", profiles/taa_bench_c3.json
constexpr float kDefaultAlpha = 0.2f;
constexpr float kDefaultGamma = 1.5f;

} // namespace

int tyr_taa(tyr_ctx* c, const tyr_taa_in* in, const tyr_taa_params* params, void* device_rgba_out, void* stream) {
	if (!c || !in || !in->color || !in->depth || !in->motion || !in->prev_depth || !device_rgba_out)
		return TYR_ERR_INVALID;
	tyr_taa_params p{ kDefaultAlpha, kDefaultGamma, 0u };
	if (params)
		p = *params;
	if (!(p.alpha > 0.f && p.alpha <= 1.f) || !(p.gamma >= 0.f && std::isfinite(p.gamma)) || (p.flags & ~(TYR_TAA_RESET | TYR_TAA_BILINEAR)) != 0u)
		return TYR_ERR_INVALID;
	FilterLaunch L;
	if (int rc = L.open(c, c->taa, stream))
		return rc;
	const size_t n = static_cast<size_t>(c->cfg.width) * c->cfg.height;
	if (int rc = L.buffer(c->dTaaHist, 2 * n))
		return rc;

	// in place: lanes read their neighbours' colours, so the kernel writes the history plane alone and a copy follows it
	const bool inPlace = device_rgba_out == static_cast<const void*>(in->color);
	TaaParams P{};
	P.color = reinterpret_cast<const float4*>(in->color);
	P.depth = in->depth;
	P.motion = reinterpret_cast<const float2*>(in->motion);
	P.prevDepth = in->prev_depth;
	P.haveHistory = L.history((p.flags & TYR_TAA_RESET) != 0u);
	P.histIn = c->dTaaHist + L.prev * n;
	P.histOut = c->dTaaHist + L.next * n;
	P.out = inPlace ? nullptr : static_cast<float4*>(device_rgba_out);
	P.W = c->cfg.width;
	P.H = c->cfg.height;
	P.alpha = p.alpha;
	P.gamma = p.gamma;
	P.bilinear = (p.flags & TYR_TAA_BILINEAR) != 0u;
	launch_taa(P, L.s);
	if (inPlace) {
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(device_rgba_out, P.histOut, n * sizeof(float4), hipMemcpyDeviceToDevice, L.s));
	}
	return L.close();
}
