// tri.hip -- batched triangle-overlap queries on the uploaded scene (tyr_query_tri, host/tri.cpp): for each of the caller's
// triangles (corners P0, P1, P2, read in place from three n x 3 float arrays), how many triangles of the scene it touches and the
// lowest max_prims build-order indices of them, or with TYR_QUERY_TRI_ANY whether it touches any (include/tyr_c.h
// "Triangle-overlap queries": a set over all triangles of the uploaded array with no traversal order in it, the member test three
// box axes in binary32 and a 17-axis separating axis test in binary64, so that tests/tri_ref.py reproduces each word by brute
// force).
//
// One query to a lane on the queries' persistent grid, with their pieces (hip/query_common.hpp, hip/traverse.hpp): the chunked
// ticket feed, the first nStaged quad records in LDS, the LdsStack without entry distances, triangle_load, the flat lane states
// (interior ref | leaf ref | kRefPop | kRefDone).
//
// The descent is box.hip's, the same text (overlap_round, hip/query_common.hpp): four closed interval tests of a slot's
// box against the query's binary32 bounding box, descend into the first slot that passes in node order and push the others so that
// they pop in node order.  Pruning is exact and needs no slack: a node's stored box contains the corners Q0, Q1, Q2 of every
// triangle below it, so a slot whose box misses the query's bounding box on some axis holds only triangles that rule 1 of the
// member test separates on that axis.
//
// The leaf step tests every primitive in array order: rule 0 (with TYR_QUERY_TRI_SKIP_SHARED) and rule 1 as binary32 compares of
// the corners, the seventeen axes of rule 2 in binary64 behind them -- the scene triangle's plane first, which is what separates
// most pairs whose boxes meet.  The lane holds the nine corner floats and recomputes the bounding box from them where it needs
// it (v_min3 / v_max3: six instructions a quad step, six registers fewer through the binary64 leaf).  Members are counted; without
// ANY they are offered to the query's row of the caller's prim array, kept ascending by hits.hip's insertion keyed on the index
// alone, the fill level and the largest kept index in registers as in box.hip.  With ANY the first member ends the query.
#include "tri.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

// ---- the member test of a (query, scene triangle) pair: include/tyr_c.h "Triangle-overlap queries", rule 2 -------------------

// Does `axis` separate {p0, p1, p2} from {q0 = 0, q1, q2}?  All points go through the same dotd(axis, x).  q0 = Q0 - Q0 is +0 for a
// finite corner and dotd(axis, 0) is a zero of either sign: as an operand of <, of min and of max it is 0.0 itself, the one term
// that is dropped.
__device__ __forceinline__ bool axis_separates(d3 axis, d3 p0, d3 p1, d3 p2, d3 q1, d3 q2) {
	const double a = dotd(axis, p0), b = dotd(axis, p1), c = dotd(axis, p2);
	const double u = dotd(axis, q1), v = dotd(axis, q2);
	const double pmin = mind(mind(a, b), c), pmax = maxd(maxd(a, b), c);
	const double qmin = mind(mind(0.0, u), v), qmax = maxd(maxd(0.0, u), v);
	return pmax < qmin || qmax < pmin;
}

// rule 2 for a pair that rules 0 and 1 let through: P the query's binary32 corners, Q the scene triangle's
__device__ __forceinline__ bool tri_member(float p0x, float p0y, float p0z, float p1x, float p1y, float p1z, float p2x, float p2y, float p2z, float q0x, float q0y, float q0z,
                                           float q1x, float q1y, float q1z, float q2x, float q2y, float q2z) {
	const d3 Q0 = {(double)q0x, (double)q0y, (double)q0z};
	const d3 p0 = {(double)p0x - Q0.x, (double)p0y - Q0.y, (double)p0z - Q0.z};
	const d3 p1 = {(double)p1x - Q0.x, (double)p1y - Q0.y, (double)p1z - Q0.z};
	const d3 p2 = {(double)p2x - Q0.x, (double)p2y - Q0.y, (double)p2z - Q0.z};
	const d3 q0 = {0.0, 0.0, 0.0};
	const d3 q1 = {(double)q1x - Q0.x, (double)q1y - Q0.y, (double)q1z - Q0.z};
	const d3 q2 = {(double)q2x - Q0.x, (double)q2y - Q0.y, (double)q2z - Q0.z};
	// the scene triangle's plane, then the query's
	const d3 f0 = q1 - q0;
	const d3 m = crossd(f0, q2 - q0);
	if (axis_separates(m, p0, p1, p2, q1, q2))
		return false;
	const d3 e0 = p1 - p0;
	const d3 n = crossd(e0, p2 - p0);
	if (axis_separates(n, p0, p1, p2, q1, q2))
		return false;
	// the nine edge crosses, the query's edge outer
	const d3 e1 = p2 - p1, e2 = p0 - p2;
	const d3 f1 = q2 - q1, f2 = q0 - q2;
	if (axis_separates(crossd(e0, f0), p0, p1, p2, q1, q2) || axis_separates(crossd(e0, f1), p0, p1, p2, q1, q2) || axis_separates(crossd(e0, f2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(crossd(e1, f0), p0, p1, p2, q1, q2) || axis_separates(crossd(e1, f1), p0, p1, p2, q1, q2) || axis_separates(crossd(e1, f2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(crossd(e2, f0), p0, p1, p2, q1, q2) || axis_separates(crossd(e2, f1), p0, p1, p2, q1, q2) || axis_separates(crossd(e2, f2), p0, p1, p2, q1, q2))
		return false;
	// the six in-plane axes: what separates coplanar triangles
	if (axis_separates(crossd(n, e0), p0, p1, p2, q1, q2) || axis_separates(crossd(n, e1), p0, p1, p2, q1, q2) || axis_separates(crossd(n, e2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(crossd(m, f0), p0, p1, p2, q1, q2) || axis_separates(crossd(m, f1), p0, p1, p2, q1, q2) || axis_separates(crossd(m, f2), p0, p1, p2, q1, q2))
		return false;
	return true;
}

__device__ __forceinline__ float min3f(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// the query a lane has in flight and what it has found so far
struct TriLane {
	float ax, ay, az, bx, by, bz, cx, cy, cz; // P0, P1, P2
	uint32_t ref;   // the lane's state
	uint32_t count; // |W| so far
	uint32_t fill;  // entries of the row in use
	int worst;      // the last entry once the row is full, INT_MAX before; -1 for a row of no entries: a larger index is turned away
};

// the query's binary32 bounding box
struct TriBox {
	float lx, ly, lz, hx, hy, hz;
};

__device__ __forceinline__ TriBox box_of(const TriLane& q) {
	return {min3f(q.ax, q.bx, q.cx), min3f(q.ay, q.by, q.cy), min3f(q.az, q.bz, q.cz), max3f(q.ax, q.bx, q.cx), max3f(q.ay, q.by, q.cy), max3f(q.az, q.bz, q.cz)};
}

// a box against the query's: closed intervals on the three axes
__device__ __forceinline__ bool box_overlaps(const TriBox& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	return lox <= q.hx && hix >= q.lx && loy <= q.hy && hiy >= q.ly && loz <= q.hz && hiz >= q.lz;
}

// One round of the wave's traversal: the overlap descent (overlap_round, hip/query_common.hpp) on the query's bounding box, then
// one leaf per lane that is at one, primitives in array order, each member counted and handed to `offer(prim)`.
template <bool ANY, class CanRefill, class Offer>
__device__ __forceinline__ void t_traverse(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, TriLane& q, bool skipShared, CanRefill canRefill,
                                           Offer offer) {
	q.ref = overlap_round(
		sc, st, stagedNodes, q.ref, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return box_overlaps(box_of(q), lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			const TriBox bb = box_of(q);
			return leaf_prims<ANY>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				const CornerBox t = tri_corner_box(cur);
				const f3 q0 = t.a, q1 = t.b, q2 = t.c;
				// rule 1, the coordinate axes: exact comparisons of the inputs
				bool member = box_overlaps(bb, t.lox, t.hix, t.loy, t.hiy, t.loz, t.hiz);
				// rule 0: a corner of the query equal to a corner of the triangle (==: -0 equals +0)
				if (member && skipShared) {
					const bool s0 = (q.ax == q0.x && q.ay == q0.y && q.az == q0.z) || (q.ax == q1.x && q.ay == q1.y && q.az == q1.z) || (q.ax == q2.x && q.ay == q2.y && q.az == q2.z);
					const bool s1 = (q.bx == q0.x && q.by == q0.y && q.bz == q0.z) || (q.bx == q1.x && q.by == q1.y && q.bz == q1.z) || (q.bx == q2.x && q.by == q2.y && q.bz == q2.z);
					const bool s2 = (q.cx == q0.x && q.cy == q0.y && q.cz == q0.z) || (q.cx == q1.x && q.cy == q1.y && q.cz == q1.z) || (q.cx == q2.x && q.cy == q2.y && q.cz == q2.z);
					member = !(s0 || s1 || s2);
				}
				member = member && tri_member(q.ax, q.ay, q.az, q.bx, q.by, q.bz, q.cx, q.cy, q.cz, q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z);
				if (member) {
					q.count += 1u;
					if (!ANY && prim <= q.worst) // (a full row, or one of no entries, turns a larger index away)
						offer(prim);
				}
				return member;
			});
		});
}

} // namespace

template <bool ANY>
__global__ void __launch_bounds__(kBlock, 4) k_query_tri(const TriParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, false)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();
	const bool skipShared = P0.skipShared != 0u;

	TriLane q = {};
	q.ref = kRefDone;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// A member that belongs into the query's row (t_traverse has turned away what a full row does not take): the entries behind
	// its place move up by one, the last one out of a full row.  The row is this lane's alone until the query finishes.
	auto offer = [&](int prim) {
		const TriParams& P = kernarg_view<TriParams>();
		const uint32_t K = P.maxPrims;
		int32_t* row = P.prim + (size_t)item * K; // (64-bit offsets: n * max_prims entries pass 2^32 bytes)
		uint32_t j = q.fill < K ? q.fill : K - 1u; // the slot that opens: the row's end, or the largest entry's
		while (j > 0u) {
			const int32_t pp = row[j - 1u];
			if (pp < prim)
				break;
			row[j] = pp;
			--j;
		}
		row[j] = prim;
		if (q.fill < K)
			q.fill += 1u;
		if (q.fill == K)
			q.worst = row[K - 1u];
	};

	// a finished query's answer: the count and the unused entries of its row
	auto finish = [&]() {
		const TriParams& P = kernarg_view<TriParams>(); // (read where it lies: not held in scalar registers through the descent)
		P.count[item] = q.count;
		if (!ANY) {
			const uint32_t K = P.maxPrims;
			const size_t base = (size_t)item * K;
			for (uint32_t j = q.fill; j < K; ++j)
				P.prim[base + j] = -1;
		}
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<TriParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const TriParams& P = kernarg_view<TriParams>();
			const size_t i3 = 3 * (size_t)item;
			q.ax = P.a[i3 + 0], q.ay = P.a[i3 + 1], q.az = P.a[i3 + 2];
			q.bx = P.b[i3 + 0], q.by = P.b[i3 + 1], q.bz = P.b[i3 + 2];
			q.cx = P.c[i3 + 0], q.cy = P.c[i3 + 1], q.cz = P.c[i3 + 2];
			q.count = q.fill = 0u;
			q.worst = (!ANY && P.maxPrims != 0u) ? 0x7fffffff : -1;
			st.reset();
			live = true;
			// every component finite, or it is not a triangle
			const bool valid = finite3(q.ax, q.ay, q.az) && finite3(q.bx, q.by, q.bz) && finite3(q.cx, q.cy, q.cz);
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly queries that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished queries, while queries remain
		t_traverse<ANY>(sc, st, stagedNodes, q, skipShared, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; },
		                offer);
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<TriParams>().error);
}

void launch_tri(const TriParams& P, bool any, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(any ? k_query_tri<true> : k_query_tri<false>, P, P.n, numCUs, lc.perCU[kLcTri][any ? 1 : 0], stream);
}

} // namespace tyr
