// nearest.hip -- batched closest-point queries on the uploaded scene (tyr_query_nearest, host/nearest.cpp): for each of the
// caller's points, read in place from an n x 3 float array, the triangle of the scene that is nearest, how far away it is
// and where on it (include/tyr_c.h "Closest-point queries": an argmin over all triangles with no traversal order in it).
//
// One point to a lane on a persistent grid, with the ray queries' pieces (hip/query_common.hpp, hip/traverse.hpp): the
// chunked ticket feed, the first nStaged quad records in LDS, the LdsStack with its private spill arrays, triangle_load, the
// flat lane states (interior ref | leaf ref | kRefPop | kRefDone).  The traversal is not a ray's: a quad step orders the four
// slots by their boxes' distance to the point, descends into the nearest and pushes the others farthest first (at most three
// pushes per record, so quadMaxStack bounds the depth as it does for rays); the bound is the best value found so far, and an
// entry is tested against it again when it is popped.  The records' visit-order bits are for rays and play no part.
//
// Pruning never changes the answer: the key, its slack (kSlackFar2 = 256.f * kUlpHalf of far2, kSlackCoord = 64.f * kUlpHalf
// of farInf * max |p_k|) and the pair's value are hip/nearest_common.hpp's, shared with hip/nearest_k.hip; the descent is the
// keyed one of hip/query_common.hpp (keyed_round), which sweep.hip and segment.hip use too.
#include "nearest.hpp"
#include "nearest_common.hpp"

namespace tyr {

namespace {

static_assert(kSlackFar2 == 256.f * kUlpHalf && kSlackCoord == 64.f * kUlpHalf, "the constants named at the head of this file");

// the point a lane has in flight and what it has found so far
struct NearestLane {
	float px, py, pz;
	float c1;     // kSlackCoord * max |p_k|
	float best;   // the smallest value so far; bound2 until a triangle is accepted
	int prim;     // its triangle, -1: none
	uint32_t ref; // the lane's state
};

} // namespace

__global__ void __launch_bounds__(kBlock, 5) k_query_nearest(const NearestParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	NearestLane q = {};
	q.ref = kRefDone;
	q.prim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// a finished point's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const NearestParams& P = kernarg_view<NearestParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = item;
		const f3 p = mk3(q.px, q.py, q.pz);
		NearestValue w;
		w.F = q.best, w.u = w.v = 0.f, w.region = 0u, w.c = p;
		if (q.prim >= 0)
			w = nearest_value<true>(triangle_load(sc.tris, (uint32_t)q.prim), p); // the winner's operations once more: the same value
		P.dist2[i] = w.F;
		P.prim[i] = q.prim;
		if (P.uv)
			reinterpret_cast<float2*>(P.uv)[i] = make_float2(w.u, w.v);
		if (P.region)
			P.region[i] = (uint8_t)w.region;
		if (P.point) {
			P.point[3 * i + 0] = w.c.x;
			P.point[3 * i + 1] = w.c.y;
			P.point[3 * i + 2] = w.c.z;
		}
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	// a triangle of a reached leaf: the smallest pair (value, index) so far stays
	auto take = [](NearestLane& q, float F, int prim) {
		if (F < q.best || (F == q.best && prim < q.prim)) {
			q.best = F;
			q.prim = prim;
		}
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<NearestParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const NearestParams& P = kernarg_view<NearestParams>();
			const size_t i3 = 3 * (size_t)item;
			q.px = P.points[i3 + 0], q.py = P.points[i3 + 1], q.pz = P.points[i3 + 2];
			const float md = P.maxDist ? P.maxDist[item] : kInf;
			// a point with a NaN or infinite coordinate, or a NaN or negative max_dist: not a query (dist2 = +inf)
			const bool valid = finite3(q.px, q.py, q.pz) && md >= 0;
			q.best = valid ? md * md : kInf;
			q.prim = -1;
			q.c1 = kSlackCoord * __builtin_fmaxf(__builtin_fmaxf(fabsf(q.px), fabsf(q.py)), __builtin_fmaxf(fabsf(q.pz), 1e-30f));
			st.reset();
			live = true;
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly points that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished points, while points remain
		n_traverse(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; }, take);
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<NearestParams>().error);
}

void launch_nearest(const NearestParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_nearest, P, P.n, numCUs, lc.perCU[kLcNearest][0], stream);
}

} // namespace tyr
