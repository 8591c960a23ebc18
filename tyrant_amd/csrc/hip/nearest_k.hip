// nearest_k.hip -- batched k-nearest and within-radius triangle queries on the uploaded scene (tyr_query_nearest_k,
// host/nearest_k.cpp): for each of the caller's points, read in place from an n x 3 float array, the k triangles with the
// smallest values inside the point's bound, in order, and how many triangles lie inside the bound at all (include/tyr_c.h
// "k-nearest queries": the smallest pairs (value, index) over all triangles, with no traversal order in it).
//
// It joins two kernels.  From hip/nearest.hip, through hip/nearest_common.hpp: the pair's value, the distance-ordered descent
// on the queries' persistent grid and its rounding-safe pruning key, with the lane's `best` read as a pruning bound B --
// the worst value the row keeps once the row is full, the point's bound2 before that, and bound2 throughout when the count
// is asked for, since every member has to be met then (the kernel is compiled in both forms: the one without a count
// carries no counter and no second bound).  A box is skipped on key > B: one at exactly B is visited, because a tie with a
// lower index displaces the worst entry.  From hip/hits.hip: the per-item k-buffer.  It is the point's own row of the
// caller's dist2 and prim arrays -- lane-private memory for as long as the point is in flight, so program order is all the
// ordering it needs, of any length up to TYR_QUERY_NEAREST_K_MAX without a register array (indexed dynamically it would live
// in scratch) and without LDS that would cost the loop its blocks per CU.  The fill level and the worst kept pair stay in
// registers: the common case -- the row is full and the triangle is farther -- is one compare and touches no memory.  uv,
// region and the closest point of the kept entries are computed from their records when the point finishes.
#include "nearest_k.hpp"
#include "nearest_common.hpp"

namespace tyr {

namespace {

// the point a lane has in flight and what it has found so far
struct NearestKLane {
	float px, py, pz;
	float c1;       // kSlackCoord * max |p_k|
	float best;     // the pruning bound B: bound2 (+inf: not a query), without a count the worst kept value once the row is full
	uint32_t ref;   // the lane's state
	uint32_t fill;  // entries of the row in use
	float worstF;   // with a count (B stays bound2): the last entry's value once the row is full, bound2 before
	int worstPrim;  // the last entry's triangle once the row is full, -1 before: a value equal to bound2 is no member
	uint32_t count; // |W| so far
};

} // namespace

template <bool COUNT>
__global__ void __launch_bounds__(kBlock, 5) k_query_nearest_k(const NearestKParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	NearestKLane q = {};
	q.ref = kRefDone;
	q.worstPrim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// A pair that belongs into the point's row (`take` has turned away what a full row does not): the entries
	// behind its place move up by one, the last one out of a full row.  The row is this lane's alone until the point finishes.
	auto offer = [&](float F, int prim) {
		const NearestKParams& P = kernarg_view<NearestKParams>();
		const uint32_t K = P.k;
		const size_t base = (size_t)item * K; // (64-bit offsets: n * k floats pass 2^32 bytes)
		float* rowF = P.dist2 + base;
		int32_t* rowP = P.prim + base;
		uint32_t j = q.fill < K ? q.fill : K - 1u; // the slot that opens: the row's end, or the worst entry's
		while (j > 0u) {
			const float pf = rowF[j - 1u];
			int32_t pp = rowP[j - 1u];
			__asm__ volatile("" : "+v"(pp)); // both loads in flight before the compare: left alone, the index is loaded behind it, a second round trip per entry
			if (pf < F || (pf == F && pp < prim))
				break;
			rowF[j] = pf;
			rowP[j] = pp;
			--j;
		}
		rowF[j] = F;
		rowP[j] = prim;
		if (q.fill < K)
			q.fill += 1u;
		if (q.fill == K) {
			const float w = rowF[K - 1u];
			if (COUNT)
				q.worstF = w;
			else
				q.best = w; // the bound shrinks to the worst kept value
			q.worstPrim = rowP[K - 1u];
		}
	};

	// a triangle of a reached leaf: a member is counted (COUNT) and, unless the row is full of nearer pairs, offered
	auto take = [&](NearestKLane&, float F, int prim) {
		if (COUNT) {
			if (!(F < q.best)) // not inside the bound (or a NaN)
				return;
			q.count += 1u;
		}
		const float worst = COUNT ? q.worstF : q.best;
		if (!(F < worst)) // not nearer than the worst kept entry (bound2 while the row has room): farther, or a tie that the index decides
			if (F > worst || prim > q.worstPrim || F != F)
				return;
		offer(F, prim);
	};

	// a finished point's answer: uv, region and closest point of the kept entries from their records, the unused entries of its
	// row, and the count
	auto finish = [&]() {
		const NearestKParams& P = kernarg_view<NearestKParams>(); // (read where it lies: not held in scalar registers through the descent)
		const uint32_t K = P.k;
		const size_t base = (size_t)item * K;
		const f3 p = mk3(q.px, q.py, q.pz);
		if (COUNT)
			P.count[item] = q.count;
		for (uint32_t j = 0; j < K; ++j) {
			const size_t e = base + j;
			NearestValue w;
			w.F = 0.f, w.u = w.v = 0.f, w.region = 0u, w.c = p;
			if (j < q.fill) {
				if (P.uv || P.region || P.point)
					w = nearest_value<true>(triangle_load(sc.tris, (uint32_t)P.prim[e]), p); // the kept pair's operations once more: the same value
			} else {
				P.dist2[e] = q.best; // (the row is not full: B is still bound2, or +inf for what is not a query)
				P.prim[e] = -1;
			}
			if (P.uv)
				reinterpret_cast<float2*>(P.uv)[e] = make_float2(w.u, w.v);
			if (P.region)
				P.region[e] = (uint8_t)w.region;
			if (P.point) {
				P.point[3 * e + 0] = w.c.x;
				P.point[3 * e + 1] = w.c.y;
				P.point[3 * e + 2] = w.c.z;
			}
		}
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<NearestKParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const NearestKParams& P = kernarg_view<NearestKParams>();
			const size_t i3 = 3 * (size_t)item;
			q.px = P.points[i3 + 0], q.py = P.points[i3 + 1], q.pz = P.points[i3 + 2];
			const float md = P.maxDist ? P.maxDist[item] : kInf;
			// a point with a NaN or infinite coordinate, or a NaN or negative max_dist: not a query (dist2 = +inf)
			const bool valid = finite3(q.px, q.py, q.pz) && md >= 0;
			q.best = valid ? md * md : kInf;
			q.worstF = q.best;
			q.worstPrim = -1;
			q.fill = q.count = 0u;
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
	q_report_overflow(overflow, lane, kernarg_view<NearestKParams>().error);
}

void launch_nearest_k(const NearestKParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(P.count ? k_query_nearest_k<true> : k_query_nearest_k<false>, P, P.n, numCUs, lc.perCU[kLcNearestK][P.count ? 1 : 0], stream);
}

} // namespace tyr
