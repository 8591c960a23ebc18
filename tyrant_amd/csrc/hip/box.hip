// box.hip -- batched box-overlap queries on the uploaded scene (tyr_query_box, host/box.cpp): for each of the caller's
// axis-aligned boxes [lo, hi], read in place from n x 3 float arrays, how many triangles of the scene it touches and the lowest
// max_prims build-order indices of them, or with TYR_QUERY_BOX_ANY whether it touches any (include/tyr_c.h "Box-overlap
// queries": a set over all triangles of the uploaded array with no traversal order in it, the member test a 13-axis separating
// axis test in binary64 in a fixed order, so that tests/box_ref.py reproduces each word by brute force).
//
// One box to a lane on the queries' persistent grid, with their pieces (hip/query_common.hpp, hip/traverse.hpp): the chunked
// ticket feed, the first nStaged quad records in LDS, the LdsStack without entry distances, triangle_load, the flat lane states
// (interior ref | leaf ref | kRefPop | kRefDone).
//
// The descent is the overlap one (overlap_round, hip/query_common.hpp), shared with tri.hip: the record's seven vectors
// (fetch_quad, hip/traverse.hpp), four closed interval tests of a slot's box against [lo, hi] in binary32 -- this unit's
// box_overlaps -- descend into the first slot that passes in node order and push the others so that they pop in node order.
// There is no key, no sort and no entry distance: the bound is the box and never changes, so a popped entry is always taken.
// Pruning is exact and needs no slack: a node's stored box contains the corners
// A, B, C of every triangle below it, and a member's corners do not all lie beyond one face of [lo, hi] (rule 1 of the member
// test) -- so a slot whose box fails the closed interval test on some axis holds no member.  An unused slot's box lies at
// +infinity (lo = +inf fails `lo <= hi_k`), a synthetic record's from -inf to +inf (passes).
//
// The leaf step tests every primitive in array order: rule 1 as binary32 compares of the record's corners (the same comparisons
// as the widened ones), rules 2 and 3 in binary64 behind them.  Members are counted; without ANY they are offered to the box's
// row of the caller's prim array, kept ascending by hits.hip's insertion keyed on the index alone -- lane-private memory for as
// long as the box is in flight.  The fill level and the largest kept index stay in registers: a full row turns a larger index
// away with one compare.  In trees from this project's builders members arrive ascending and an insertion is an append
// (tests/test_box_query.py asserts it on the fixtures' trees); the insertion is correct for any order.  With ANY the first
// member ends the box.
#include "box.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

// ---- the member test of a (box, triangle) pair: include/tyr_c.h "Box-overlap queries", rules 2 and 3 -------------------------

// An edge axis a = cross(unit_i, f) with the zeros and ones multiplied out: with (u, v) the two other components in cyclic
// order a_u = -f_v, a_v = f_u and a_i = 0.  The terms of the zero component are +-0 in every sum of the definition and change
// no comparison; IEEE addition commutes, so one form serves the three units.
__device__ __forceinline__ bool edge_axis_separates(double fu, double fv, double e1u, double e1v, double e2u, double e2v, double lu, double hu, double lv, double hv) {
	const double au = -fv, av = fu;
	const double p1 = au * e1u + av * e1v, p2 = au * e2u + av * e2v;
	const double pmax = maxd(maxd(0.0, p1), p2), pmin = mind(mind(0.0, p1), p2);
	const double ul = au * lu, uh = au * hu, vl = av * lv, vh = av * hv;
	const double bmin = mind(ul, uh) + mind(vl, vh), bmax = maxd(ul, uh) + maxd(vl, vh);
	return pmax < bmin || pmin > bmax;
}

// rules 2 and 3 for a pair that no box axis separates; A, B, C the binary32 corners, lo / hi the box
__device__ __forceinline__ bool box_member(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float lox, float loy, float loz, float hix, float hiy,
                                           float hiz) {
	const double Ax = (double)ax, Ay = (double)ay, Az = (double)az;
	const double e1x = (double)bx - Ax, e1y = (double)by - Ay, e1z = (double)bz - Az;
	const double e2x = (double)cx - Ax, e2y = (double)cy - Ay, e2z = (double)cz - Az;
	const double lx = (double)lox - Ax, ly = (double)loy - Ay, lz = (double)loz - Az;
	const double hx = (double)hix - Ax, hy = (double)hiy - Ay, hz = (double)hiz - Az;
	// the plane: a = cross(e1', e2'), the triangle projects to 0
	{
		const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
		const double xl = nx * lx, xh = nx * hx, yl = ny * ly, yh = ny * hy, zl = nz * lz, zh = nz * hz;
		const double bmin = (mind(xl, xh) + mind(yl, yh)) + mind(zl, zh), bmax = (maxd(xl, xh) + maxd(yl, yh)) + maxd(zl, zh);
		if (0.0 < bmin || 0.0 > bmax)
			return false;
	}
	// the nine edge axes: unit x, y, z (outer) by f = e1', e2' - e1', e2' (inner)
	const double gx = e2x - e1x, gy = e2y - e1y, gz = e2z - e1z;
	if (edge_axis_separates(e1y, e1z, e1y, e1z, e2y, e2z, ly, hy, lz, hz) || edge_axis_separates(gy, gz, e1y, e1z, e2y, e2z, ly, hy, lz, hz) ||
	    edge_axis_separates(e2y, e2z, e1y, e1z, e2y, e2z, ly, hy, lz, hz))
		return false;
	if (edge_axis_separates(e1z, e1x, e1z, e1x, e2z, e2x, lz, hz, lx, hx) || edge_axis_separates(gz, gx, e1z, e1x, e2z, e2x, lz, hz, lx, hx) ||
	    edge_axis_separates(e2z, e2x, e1z, e1x, e2z, e2x, lz, hz, lx, hx))
		return false;
	if (edge_axis_separates(e1x, e1y, e1x, e1y, e2x, e2y, lx, hx, ly, hy) || edge_axis_separates(gx, gy, e1x, e1y, e2x, e2y, lx, hx, ly, hy) ||
	    edge_axis_separates(e2x, e2y, e1x, e1y, e2x, e2y, lx, hx, ly, hy))
		return false;
	return true;
}

// the box a lane has in flight and what it has found so far
struct BoxLane {
	float lx, ly, lz, hx, hy, hz;
	uint32_t ref;   // the lane's state
	uint32_t count; // |W| so far
	uint32_t fill;  // entries of the row in use
	int worst;      // the last entry once the row is full, INT_MAX before; -1 for a row of no entries: a larger index is turned away
};

// a slot's box against the lane's: closed intervals on the three axes
__device__ __forceinline__ bool box_overlaps(const BoxLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	return lox <= q.hx && hix >= q.lx && loy <= q.hy && hiy >= q.ly && loz <= q.hz && hiz >= q.lz;
}

// One round of the wave's traversal: the overlap descent (overlap_round, hip/query_common.hpp) on box_overlaps, then one leaf
// per lane that is at one, primitives in array order, each member counted and handed to `offer(prim)`.
template <bool ANY, class CanRefill, class Offer>
__device__ __forceinline__ void b_traverse(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, BoxLane& q, CanRefill canRefill, Offer offer) {
	q.ref = overlap_round(
		sc, st, stagedNodes, q.ref, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return box_overlaps(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			return leaf_prims<ANY>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				const CornerBox t = tri_corner_box(cur);
				// rule 1, the box axes: exact comparisons of the inputs
				const bool member = box_overlaps(q, t.lox, t.hix, t.loy, t.hiy, t.loz, t.hiz) &&
				                    box_member(t.a.x, t.a.y, t.a.z, t.b.x, t.b.y, t.b.z, t.c.x, t.c.y, t.c.z, q.lx, q.ly, q.lz, q.hx, q.hy, q.hz);
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
__global__ void __launch_bounds__(kBlock, 5) k_query_box(const BoxParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, false)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	BoxLane q = {};
	q.ref = kRefDone;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// A member that belongs into the box's row (b_traverse has turned away what a full row does not take): the entries behind
	// its place move up by one, the last one out of a full row.  The row is this lane's alone until the box finishes.
	auto offer = [&](int prim) {
		const BoxParams& P = kernarg_view<BoxParams>();
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

	// a finished box's answer: the count and the unused entries of its row
	auto finish = [&]() {
		const BoxParams& P = kernarg_view<BoxParams>(); // (read where it lies: not held in scalar registers through the descent)
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
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<BoxParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const BoxParams& P = kernarg_view<BoxParams>();
			const size_t i3 = 3 * (size_t)item;
			q.lx = P.lo[i3 + 0], q.ly = P.lo[i3 + 1], q.lz = P.lo[i3 + 2];
			q.hx = P.hi[i3 + 0], q.hy = P.hi[i3 + 1], q.hz = P.hi[i3 + 2];
			q.count = q.fill = 0u;
			q.worst = (!ANY && P.maxPrims != 0u) ? 0x7fffffff : -1;
			st.reset();
			live = true;
			// every component finite and lo <= hi on every axis, or it is not a box (a comparison with a NaN is false)
			const bool valid = finite3(q.lx, q.ly, q.lz) && finite3(q.hx, q.hy, q.hz) && q.lx <= q.hx && q.ly <= q.hy && q.lz <= q.hz;
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly boxes that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished boxes, while boxes remain
		b_traverse<ANY>(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; }, offer);
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<BoxParams>().error);
}

void launch_box(const BoxParams& P, bool any, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(any ? k_query_box<true> : k_query_box<false>, P, P.n, numCUs, lc.perCU[kLcBox][any ? 1 : 0], stream);
}

} // namespace tyr
