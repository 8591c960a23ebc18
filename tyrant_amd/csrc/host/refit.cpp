// refit.cpp -- tyr_scene_refit (include/tyr_c.h "refit"): new triangles in the shape of the tree a ctx holds; the kernels are
// hip/refit.hip.  An upload with TYR_FLAG_REFIT keeps a plan (hip/refit.hpp RefitPlan): the reference's node array in HBM, the
// node behind every quad slot and pair side (from the layout pass that wrote them, host or device), and the cut that schedules
// the bottom-up pass -- subtrees of at most kRefitRangeNodes nodes (the reference's array is depth-first with left child =
// index + 1, bvh.cpp:195-202, so every subtree is a contiguous range) and the nodes above them, grouped by height.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "../hip/refit.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

struct Schedule {
	std::vector<uint4> ranges;
	std::vector<uint16_t> height;
	std::vector<int32_t> top;
	std::vector<uint32_t> topLevel;
};

// the cut and the heights of a tree the layout pass has accepted (children behind their parent, inside its subtree)
void schedule(const tyr_bvh_node* nodes, int32_t nNodes, Schedule& S) {
	const size_t nN = static_cast<size_t>(nNodes);
	std::vector<uint32_t> h(nN, 0);
	for (size_t i = nN; i-- > 0;)
		if (nodes[i].primitiveCount == 0)
			h[i] = 1u + std::max(h[i + 1], h[static_cast<size_t>(nodes[i].offset)]);
	S.height.resize(nN);
	for (size_t i = 0; i < nN; ++i)
		S.height[i] = static_cast<uint16_t>(std::min<uint32_t>(h[i], 0xFFFFu)); // (range nodes stay below kRefitRangeNodes)
	std::vector<std::pair<int32_t, int32_t>> work{ { 0, nNodes } }; // subtree [begin, end)
	std::vector<std::pair<uint32_t, int32_t>> top;                  // (height, node)
	while (!work.empty()) {
		const auto r = work.back();
		work.pop_back();
		const tyr_bvh_node& n = nodes[r.first];
		if (static_cast<uint32_t>(r.second - r.first) <= kRefitRangeNodes || n.primitiveCount > 0) {
			S.ranges.push_back(make_uint4(static_cast<uint32_t>(r.first), static_cast<uint32_t>(r.second), h[static_cast<size_t>(r.first)], 0u));
			continue;
		}
		top.push_back({ h[static_cast<size_t>(r.first)], r.first });
		work.push_back({ n.offset, r.second });
		work.push_back({ r.first + 1, n.offset });
	}
	std::sort(S.ranges.begin(), S.ranges.end(), [](const uint4& a, const uint4& b) { return a.x < b.x; });
	std::sort(top.begin(), top.end());
	for (size_t k = 0; k < top.size(); ++k) {
		if (k == 0 || top[k].first != top[k - 1].first)
			S.topLevel.push_back(static_cast<uint32_t>(k));
		S.top.push_back(top[k].second);
	}
	S.topLevel.push_back(static_cast<uint32_t>(top.size()));
}

template <class T>
int upload(T*& d, const T* h, size_t count, size_t& bytes) {
	if (count == 0)
		return TYR_OK;
	if (int rc = dev_alloc(d, count))
		return rc;
	bytes += count * sizeof(T);
	if (h)
		HIPCHK(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
	return TYR_OK;
}

} // namespace

namespace tyr {
namespace drv {

void refit_free(tyr_ctx* c) {
	RefitPlan& R = c->refit;
	dev_free(R.nodes);
	dev_free(R.slotNode);
	dev_free(R.pairNode);
	dev_free(R.ranges);
	dev_free(R.height);
	dev_free(R.top);
	dev_free(R.topLevel);
	dev_free(R.err);
	R = RefitPlan{};
}

int refit_keep(tyr_ctx* c, const tyr_bvh_node* nodes, const tyr_bvh_node* dNodes, int32_t nNodes, const int32_t* slotNode, int32_t*& dSlotNode, uint32_t nSlots,
               const int32_t* pairNode, uint32_t nPairSides) {
	refit_free(c);
	RefitPlan& R = c->refit;
	int32_t* adopted = dSlotNode;
	dSlotNode = nullptr;
	int rc = TYR_OK;
	try {
		std::vector<tyr_bvh_node> readBack;
		if (!nodes) {
			readBack.resize(static_cast<size_t>(nNodes));
			if (const hipError_t e = hipMemcpy(readBack.data(), dNodes, readBack.size() * sizeof(tyr_bvh_node), hipMemcpyDeviceToHost))
				throw static_cast<int>(e);
			nodes = readBack.data();
		}
		Schedule S;
		schedule(nodes, nNodes, S);
		R.nNodes = nNodes;
		R.nSlots = nSlots;
		R.nPairSides = nPairSides;
		R.nRanges = static_cast<uint32_t>(S.ranges.size());
		R.nTop = static_cast<uint32_t>(S.top.size());
		R.nTopLevels = static_cast<uint32_t>(S.topLevel.size() - 1);
		if ((rc = upload(R.nodes, dNodes ? nullptr : nodes, static_cast<size_t>(nNodes), R.bytes)))
			throw rc;
		if (dNodes)
			if (const hipError_t e = hipMemcpy(R.nodes, dNodes, static_cast<size_t>(nNodes) * sizeof(tyr_bvh_node), hipMemcpyDeviceToDevice))
				throw static_cast<int>(e);
		if (adopted) {
			R.slotNode = adopted;
			adopted = nullptr;
			R.bytes += static_cast<size_t>(nSlots) * sizeof(int32_t);
		} else if ((rc = upload(R.slotNode, slotNode, nSlots, R.bytes))) {
			throw rc;
		}
		if ((rc = upload(R.pairNode, pairNode, nPairSides, R.bytes)) || (rc = upload(R.ranges, S.ranges.data(), S.ranges.size(), R.bytes)) ||
		    (rc = upload(R.height, S.height.data(), S.height.size(), R.bytes)) || (rc = upload(R.top, S.top.data(), S.top.size(), R.bytes)) ||
		    (rc = upload(R.topLevel, S.topLevel.data(), S.topLevel.size(), R.bytes)) || (rc = upload(R.err, static_cast<const uint32_t*>(nullptr), 1, R.bytes)))
			throw rc;
	} catch (int e) {
		rc = e;
	} catch (const std::bad_alloc&) {
		rc = TYR_ERR_OOM;
	}
	dev_free(adopted);
	if (rc)
		refit_free(c);
	return rc;
}

} // namespace drv
} // namespace tyr

int tyr_scene_refit(tyr_ctx* c, const tyr_triangle* prims, const tyr_bbox* bboxes, int32_t nPrims, uint32_t flags, void* stream, tyr_bvh_node* nodes_out) {
	if (!c || (flags & ~TYR_REFIT_DEVICE) != 0u || nPrims < 0)
		return TYR_ERR_INVALID;
	if (!(c->cfg.flags & TYR_FLAG_REFIT))
		return TYR_ERR_UNSUPPORTED;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (static_cast<uint32_t>(nPrims) != c->scene.nPrims)
		return TYR_ERR_INVALID;
	if (nPrims == 0)
		return TYR_OK; // an empty scene: nothing to move
	if (!prims)
		return TYR_ERR_INVALID;
	RefitPlan& R = c->refit;
	if (!R.nodes)
		return TYR_ERR_UNSUPPORTED; // (the upload could not keep its plan and said so)
	DeviceScope scope;
	if (int rc = scope.enter(c))
		return rc;
	hipStream_t s = c->stream;
	// drop_scene's rules: behind everything queued on the ctx's stream (stream order) and the ctx's queries on other streams
	for (const auto& q : c->queryStreams)
		HIPCHK(hipStreamWaitEvent(s, q.done, 0));
	const size_t n = static_cast<size_t>(nPrims);
	tyr_triangle* dPrims = nullptr;
	tyr_bbox* dBoxes = nullptr;
	struct Staging {
		tyr_triangle*& p;
		tyr_bbox*& b;
		~Staging() {
			dev_free(p);
			dev_free(b);
		}
	} staging{ dPrims, dBoxes };
	RefitArgs A{};
	if (flags & TYR_REFIT_DEVICE) {
		hipStream_t cs = stream ? static_cast<hipStream_t>(stream) : s;
		if (cs != s) {
			hipEvent_t ready = nullptr;
			HIPCHK(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
			const hipError_t e1 = hipEventRecord(ready, cs);
			const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(s, ready, 0) : e1;
			(void)hipEventDestroy(ready);
			HIPCHK(e2);
		}
		A.prims = prims;
		A.bboxes = bboxes;
	} else {
		if (int rc = dev_alloc(dPrims, n))
			return rc;
		HIPCHK(hipMemcpyAsync(dPrims, prims, n * sizeof(tyr_triangle), hipMemcpyHostToDevice, s));
		if (bboxes) {
			if (int rc = dev_alloc(dBoxes, n))
				return rc;
			HIPCHK(hipMemcpyAsync(dBoxes, bboxes, n * sizeof(tyr_bbox), hipMemcpyHostToDevice, s));
		}
		A.prims = dPrims;
		A.bboxes = dBoxes;
	}
	A.n = nPrims;
	A.nodes = R.nodes;
	A.height = R.height;
	A.ranges = R.ranges;
	A.top = R.top;
	A.topLevel = R.topLevel;
	A.nTopLevels = R.nTopLevels;
	A.slotNode = R.slotNode;
	A.nSlots = R.nSlots;
	A.pairNode = R.pairNode;
	A.nPairSides = R.nPairSides;
	A.quads = c->dQuads;
	A.pairs = c->dNodes;
	A.tris = c->dTris;
	A.err = R.err;
	// 1. validate: nothing is written unless every record passes
	uint32_t err = 0;
	HIPCHK(hipMemsetAsync(R.err, 0, sizeof(uint32_t), s));
	launch_refit_validate(A, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(&err, R.err, sizeof err, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (err)
		return TYR_ERR_INVALID;
	// 2. triangles, subtrees, top, records; the root box back to the host (the rays' cull test, DevScene::rootMin / rootMax)
	launch_refit(A, R.nRanges, s);
	HIPCHK(hipGetLastError());
	tyr_bbox root{};
	HIPCHK(hipMemcpyAsync(&root, R.nodes, sizeof root, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	std::memcpy(c->scene.rootMin, root.bounds[0], 12);
	std::memcpy(c->scene.rootMax, root.bounds[1], 12);
	if (int rc = winding_build(c, R.nodes, nullptr, R.nNodes)) // TYR_FLAG_WINDING: the moments of the new triangles and boxes
		return rc;
	if (nodes_out)
		HIPCHK(hipMemcpy(nodes_out, R.nodes, static_cast<size_t>(R.nNodes) * sizeof(tyr_bvh_node), hipMemcpyDeviceToHost));
	return TYR_OK;
}
