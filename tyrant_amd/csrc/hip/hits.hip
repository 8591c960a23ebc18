// hits.hip -- batched multi-hit ray queries on the uploaded scene (tyr_query_hits, host/hits.cpp): for each of the caller's
// rays, read in place from n x 3 float arrays, how many surfaces the segment (1e-3, tmax - 1e-3) goes through and the nearest
// max_hits of them in order (include/tyr_c.h "Multi-hit queries": a set over the triangles the reference's any-hit traversal
// would test if it never returned early, with no visit order in it).
//
// One ray to a lane on the queries' persistent grid, with their pieces (hip/query_common.hpp, hip/traverse.hpp): the chunked
// ticket feed, the first nStaged quad records in LDS, the LdsStack without entry distances, and the any-hit form of the ray
// queries' descent (ray_descent<true>) -- test_quad in node order against a bound that never shrinks (the ray's tmax), so that no entry is re-tested when
// it is popped and the set of leaves reached does not depend on the order (hip/traverse.hpp "Exactness").  No leaf ends a
// ray: `count` needs the whole segment.
//
// What is new is the leaf side.  Every primitive of a reached leaf is tested and counted, and a hit is offered to the
// lane's k-buffer: the max_hits smallest pairs (t, prim) so far, sorted.  The buffer is the ray's own row of the caller's t
// and prim arrays -- lane-private memory for as long as the ray is in flight, so program order is all the ordering it needs,
// and of any length up to TYR_QUERY_HITS_MAX without a register array (indexed dynamically it would live in scratch) and
// without LDS that would cost the loop its blocks per CU.  The fill level and the worst kept t stay in registers: the common
// case -- the buffer is full and the hit is farther -- is one compare and touches no memory.  An insertion moves the row's
// tail up by one entry through global memory; it happens at most once per hit and, on a full buffer, only for hits that
// belong into the answer.  u, v and the side of the kept entries are computed from their records when the ray finishes.
#include "device_common.hpp"
#include "hits.hpp"
#include "query_common.hpp"

namespace tyr {

namespace {

// the value of a (ray, triangle) pair: loader.h:21-46 operation by operation (triangle_test, hip/traverse.hpp), and with
// TWO_SIDED the same operations for a negative determinant -- 1 / det of the actual det -- instead of the cull
template <bool TWO_SIDED>
__device__ __forceinline__ float hit_value(const TriData& td, f3 o, f3 d, bool& back, float& uOut, float& vOut) {
	const f3 vert = mk3(td.a.x, td.a.y, td.a.z);
	const f3 e1 = mk3(td.a.w, td.b.x, td.b.y);
	const f3 e2 = mk3(td.b.z, td.b.w, td.c.x);
	const f3 pvec = cross(d, e2);
	const float det = dot(e1, pvec);
	if (TWO_SIDED ? (fabsf(det) < 0.0000001f) : (det < 0.0000001f))
		return 0.0f;
	back = TWO_SIDED && det < 0;
	const float invDet = 1 / det;
	const f3 tvec = o - vert;
	const float u = dot(tvec, pvec) * invDet;
	if (u < 0 || u > 1)
		return 0.0f;
	const f3 qvec = cross(tvec, e1);
	const float v = dot(d, qvec) * invDet;
	if (v < 0 || u + v > 1)
		return 0.0f;
	uOut = u;
	vOut = v;
	return dot(e2, qvec) * invDet;
}

// the ray a lane has in flight and what it has found so far
struct HitsLane {
	float ox, oy, oz, dx, dy, dz, ix, iy, iz; // origin, direction, 1 / direction (bvh.h:216)
	bool regular;                             // ray_is_regular: test_quad's finite-1/d form applies
	float tmax;                               // the bound at every node and in the accept rule
	uint32_t ref;                             // the lane's state
	uint32_t count, back;                     // |H| so far, and its members with a negative determinant
	uint32_t fill;                            // entries of the k-buffer in use
	float worstT;                             // the last entry's t once the buffer is full, +inf before (an accepted t is finite)
	int worstPrim;                            // ... and its triangle
};

// One round of the wave's traversal: the ray queries' any-hit descent (ray_descent<true>, hip/query_common.hpp), then one leaf
// per lane that is at one: every primitive in array order, each accepted hit (bvh.h:229) counted and handed to
// `offer(t, prim)`.
template <bool TWO_SIDED, class CanRefill, class Offer>
__device__ __forceinline__ void h_traverse(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, HitsLane& q, bool live, CanRefill canRefill, Offer offer) {
	const uint32_t nStaged = sc.nStaged;
	const float4* quads = pinned_quads(sc);
	const bool allRegular = (__ballot(live && !q.regular) == 0ull);
	const RayConst r = { mk3(q.ox, q.oy, q.oz), mk3(q.dx, q.dy, q.dz), mk3(q.ix, q.iy, q.iz), q.ix < 0, q.iy < 0, q.iz < 0 }; // bvh.h:216-217
	uint32_t ref = ray_descent<true>(quads, st, stagedNodes, nStaged, r, allRegular, q.tmax, q.ref, canRefill);
	if (ref_is_leaf(ref)) {
		leaf_prims<false>(sc.tris, ref, [&](const TriData& cur, int prim) {
			bool back = false;
			float u, v;
			const float t = hit_value<TWO_SIDED>(cur, r.o, r.d, back, u, v);
			if (t > kEpsilon && ((q.tmax - t) > kEpsilon)) { // bvh.h:229
				q.count += 1u;
				q.back += back ? 1u : 0u;
				if (!(t < q.worstT)) // full, and not nearer than the worst kept entry: farther, or a tie that the index decides
					if (t > q.worstT || prim > q.worstPrim)
						return;
				offer(t, prim);
			}
		});
		ref = kRefPop;
	}
	q.ref = ref;
}

} // namespace

template <bool TWO_SIDED>
__global__ void __launch_bounds__(kBlock, 5) k_query_hits(const HitsParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, false)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	HitsLane q = {};
	q.ref = kRefDone;
	uint32_t ray = 0;
	bool live = false, overflow = false;

	// A hit that belongs into the ray's row (h_traverse has turned away what a full row does not take): the entries behind
	// its place move up by one, the last one out of a full row.  The row is this lane's alone until the ray finishes.
	auto offer = [&](float t, int prim) {
		const HitsParams& P = kernarg_view<HitsParams>();
		const uint32_t K = P.maxHits;
		const size_t base = (size_t)ray * K; // (64-bit offsets: n * max_hits floats pass 2^32 bytes)
		float* rowT = P.t + base;
		int32_t* rowP = P.prim + base;
		uint32_t j = q.fill < K ? q.fill : K - 1u; // the slot that opens: the row's end, or the worst entry's
		while (j > 0u) {
			const float pt = rowT[j - 1u];
			const int32_t pp = rowP[j - 1u];
			if (pt < t || (pt == t && pp < prim))
				break;
			rowT[j] = pt;
			rowP[j] = pp;
			--j;
		}
		rowT[j] = t;
		rowP[j] = prim;
		if (q.fill < K)
			q.fill += 1u;
		if (q.fill == K) {
			q.worstT = rowT[K - 1u];
			q.worstPrim = rowP[K - 1u];
		}
	};

	// a finished ray's answer: the counts, the unused entries of its row, and u, v, side of the kept ones from their records
	auto finish = [&]() {
		const HitsParams& P = kernarg_view<HitsParams>(); // (read where it lies: not held in scalar registers through the descent)
		const uint32_t K = P.maxHits;
		const size_t base = (size_t)ray * K;
		P.count[ray] = q.count;
		if (P.backCount)
			P.backCount[ray] = q.back;
		const f3 o = mk3(q.ox, q.oy, q.oz), d = mk3(q.dx, q.dy, q.dz);
		for (uint32_t j = 0; j < K; ++j) {
			float u = 0.f, v = 0.f;
			bool back = false;
			if (j < q.fill) {
				if (P.uv || P.side)
					hit_value<TWO_SIDED>(triangle_load(sc.tris, (uint32_t)P.prim[base + j]), o, d, back, u, v); // the kept hit's operations once more: the same values
			} else {
				P.t[base + j] = q.tmax;
				P.prim[base + j] = -1;
			}
			if (P.uv)
				reinterpret_cast<float2*>(P.uv)[base + j] = make_float2(u, v);
			if (P.side)
				P.side[base + j] = back ? 1 : 0;
		}
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<HitsParams>().ticket; });
		if (fresh != kNoItem) {
			ray = fresh;
			const HitsParams& P = kernarg_view<HitsParams>();
			const size_t i3 = 3 * (size_t)ray;
			q.ox = P.origins[i3 + 0], q.oy = P.origins[i3 + 1], q.oz = P.origins[i3 + 2];
			q.dx = P.directions[i3 + 0], q.dy = P.directions[i3 + 1], q.dz = P.directions[i3 + 2];
			q.tmax = P.tmax ? P.tmax[ray] : kVeryFar;
			const RayConst nr = make_ray(mk3(q.ox, q.oy, q.oz), mk3(q.dx, q.dy, q.dz));
			q.ix = nr.inv.x, q.iy = nr.inv.y, q.iz = nr.inv.z;
			q.regular = ray_is_regular(nr);
			q.count = q.back = q.fill = 0u;
			q.worstT = __builtin_inff();
			q.worstPrim = -1;
			st.reset();
			live = true;
			// a ray with a NaN or infinite component is not a query (and never enters a box)
			const bool valid = finite3(q.ox, q.oy, q.oz) && finite3(q.dx, q.dy, q.dz);
			q.ref = valid ? root_ref(sc, nr, q.tmax) : kRefDone;
			if (q.ref != kRefDone)
				q.ref = sc.quadRootRef;
			if (q.ref == kRefDone)
				finish(); // missed the root box, or not a ray
		}
		if (feed.top_up(live)) // mostly rays that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished rays, while rays remain
		h_traverse<TWO_SIDED>(sc, st, stagedNodes, q, live, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; }, offer);
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<HitsParams>().error);
}

void launch_hits(const HitsParams& P, bool twoSided, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(twoSided ? k_query_hits<true> : k_query_hits<false>, P, P.n, numCUs, lc.perCU[kLcHits][twoSided ? 1 : 0], stream);
}

} // namespace tyr
