// winding.cpp -- tyr_query_winding and tyr_scene_moments: generalised winding numbers of the ctx's scene (include/tyr_c.h
// "Winding numbers"; the kernels are hip/winding.hip).  A ctx with TYR_FLAG_WINDING keeps a moment tree beside its scene
// (hip/winding.hpp WindingTree), built on the device by every upload path and rebuilt by tyr_scene_refit.  The query is one like
// those of host/query.cpp: no render state, the caller's stream, the same per-stream bookkeeping (QueryLaunch: the stream's
// `done` event, which tyr_scene_refit, a scene change and tyr_destroy wait for; its ticket word goes unused -- the points are
// dealt by block index).
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "../hip/winding.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace tyr {
namespace drv {

void winding_free(tyr_ctx* c) {
	dev_free(c->winding.nodes);
	dev_free(c->winding.S);
	c->winding = WindingTree{};
}

int winding_build(tyr_ctx* c, const tyr_bvh_node* dNodes, const tyr_bvh_node* hostNodes, int32_t nNodes) {
	if (!(c->cfg.flags & TYR_FLAG_WINDING))
		return TYR_OK;
	WindingTree& W = c->winding;
	if (W.nNodes != nNodes)
		winding_free(c);
	if (nNodes <= 0 || c->scene.nPrims == 0)
		return TYR_OK;
	const size_t n = static_cast<size_t>(nNodes);
	tyr_bvh_node* staged = nullptr;
	int32_t* parent = nullptr;
	uint32_t* arrived = nullptr;
	unsigned long long* moments = nullptr;
	auto build = [&]() -> int {
		int rc;
		if (!W.nodes) {
			if ((rc = dev_alloc(W.nodes, n)) || (rc = dev_alloc(W.S, n)))
				return rc;
			W.nNodes = nNodes;
			W.bytes = n * (sizeof(WindingNode) + sizeof(double));
		}
		if (!dNodes) {
			if ((rc = dev_alloc(staged, n)))
				return rc;
			HIPCHK(hipMemcpyAsync(staged, hostNodes, n * sizeof(tyr_bvh_node), hipMemcpyHostToDevice, c->stream));
		}
		if ((rc = dev_alloc(parent, n)) || (rc = dev_alloc(arrived, n)) || (rc = dev_alloc(moments, n * 8)))
			return rc;
		HIPCHK(hipMemsetAsync(parent, 0xFF, n * sizeof(int32_t), c->stream));
		HIPCHK(hipMemsetAsync(arrived, 0, n * sizeof(uint32_t), c->stream));
		WindingBuildArgs A{};
		A.src = dNodes ? dNodes : staged;
		A.tris = c->dTris;
		A.nNodes = nNodes;
		A.nPrims = c->scene.nPrims;
		A.nodes = W.nodes;
		A.S = W.S;
		A.parent = parent;
		A.arrived = arrived;
		A.moments = moments;
		launch_winding_build(A, c->stream);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(c->stream));
		return TYR_OK;
	};
	const int rc = build();
	if (rc)
		(void)hipStreamSynchronize(c->stream);
	dev_free(staged);
	dev_free(parent);
	dev_free(arrived);
	dev_free(moments);
	if (rc)
		winding_free(c);
	return rc;
}

} // namespace drv
} // namespace tyr

int tyr_query_winding(tyr_ctx* c, uint32_t n, const float* points, float accuracy, float* w_out, uint32_t* terms_out, void* stream) {
	if (!c || n >= (1u << 31) || !(accuracy >= 0.0f))
		return TYR_ERR_INVALID;
	if (!(c->cfg.flags & TYR_FLAG_WINDING))
		return TYR_ERR_UNSUPPORTED;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!points || !w_out)
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	WindingParams P{};
	P.nodes = c->winding.nodes;
	P.tris = c->dTris;
	P.points = points;
	P.w = w_out;
	P.terms = terms_out;
	P.n = n;
	P.nNodes = c->winding.nNodes; // 0: a scene without triangles, every w = 0
	P.accuracy = accuracy;
	launch_winding(P, L.s);
	return L.close();
}

int tyr_scene_moments(tyr_ctx* c, int32_t first, int32_t count, double* host_out) {
	if (!c || first < 0 || count < 0)
		return TYR_ERR_INVALID;
	if (!(c->cfg.flags & TYR_FLAG_WINDING))
		return TYR_ERR_UNSUPPORTED;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (static_cast<int64_t>(first) + count > c->winding.nNodes)
		return TYR_ERR_INVALID;
	if (count == 0)
		return TYR_OK;
	if (!host_out)
		return TYR_ERR_INVALID;
	DeviceScope scope;
	if (int rc = scope.enter(c))
		return rc;
	try {
		std::vector<WindingNode> rec(static_cast<size_t>(count));
		std::vector<double> S(static_cast<size_t>(count));
		HIPCHK(hipMemcpy(rec.data(), c->winding.nodes + first, rec.size() * sizeof(WindingNode), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(S.data(), c->winding.S + first, S.size() * sizeof(double), hipMemcpyDeviceToHost));
		for (size_t i = 0; i < rec.size(); ++i) {
			double* o = host_out + 8 * i;
			o[0] = rec[i].p[0], o[1] = rec[i].p[1], o[2] = rec[i].p[2];
			o[3] = rec[i].N[0], o[4] = rec[i].N[1], o[5] = rec[i].N[2];
			o[6] = rec[i].r2;
			o[7] = S[i];
		}
	} catch (const std::bad_alloc&) {
		return TYR_ERR_OOM;
	}
	return TYR_OK;
}
