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
// The quad step is this unit's own: the record's seven vectors as n_traverse loads them (hip/nearest_common.hpp), four closed
// interval tests of a slot's box against [lo, hi] in binary32, descend into the first slot that passes in node order and push
// the others so that they pop in node order.  There is no key, no sort and no entry distance: the bound is the box and never
// changes, so a popped entry is always taken.  Pruning is exact and needs no slack: a node's stored box contains the corners
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

namespace tyr {

namespace {

// ---- the member test of a (box, triangle) pair: include/tyr_c.h "Box-overlap queries", rules 2 and 3 -------------------------

__device__ __forceinline__ double mind(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double maxd(double a, double b) { return b > a ? b : a; }

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

// One round of the wave's traversal: the descent, one pop attempt and one quad step per lane per trip, until no lane descends
// -- or fewer than kQueryMinTraversing do and a lane is at a leaf or `canRefill()` says enough lanes could start new work; then
// one leaf per lane that is at one, primitives in array order, each member counted and handed to `offer(prim)`.
template <bool ANY, class CanRefill, class Offer>
__device__ __forceinline__ void b_traverse(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, BoxLane& q, CanRefill canRefill, Offer offer) {
	const uint32_t nStaged = sc.nStaged;
	// (the quad array's address as an opaque global-memory pointer: see q_traverse)
	auto held = (const __attribute__((address_space(1))) float4*)sc.quads;
	__asm__ volatile("" : "+s"(held));
	const float4* quads = (const float4*)held;
	uint32_t ref = q.ref;
	for (;;) {
		const uint32_t nTrav = (uint32_t)__popcll(lanes_traversing(ref));
		if (nTrav == 0)
			break;
		if (nTrav < kQueryMinTraversing) {
			const bool anyLeaf = lanes_at_leaf(ref) != 0ull;
			if (anyLeaf || canRefill(ref))
				break;
		}
		if (ref == kRefPop) {
			uint32_t pr;
			float pt;
			ref = st.pop(pr, pt) ? pr : kRefDone; // (no entry distance and a constant bound: a popped entry is always taken)
		}
		if ((int)ref >= 0) {
			const uint32_t idx = ref & kQuadIndexMask;
			float4 x01, x23, y01, y23, z01, z23, rf;
			if (idx < nStaged) { // (explicit LDS pointers and a tail of its own: see test_quad)
#if defined(__HIP_DEVICE_COMPILE__)
				typedef __attribute__((address_space(3))) const float4* lds_f4;
				const lds_f4 c = (lds_f4)stagedNodes + idx;
#else
				const float4* c = stagedNodes + idx; // host pass of the same source: never executed
#endif
				x01 = c[0 * kStagedNodes], x23 = c[1 * kStagedNodes], y01 = c[2 * kStagedNodes], y23 = c[3 * kStagedNodes];
				z01 = c[4 * kStagedNodes], z23 = c[5 * kStagedNodes], rf = c[6 * kStagedNodes];
				__asm__ volatile("" : "+v"(rf.x));
			} else {
				const float4* n = quads + 8 * idx;
				x01 = n[0], x23 = n[1], y01 = n[2], y23 = n[3], z01 = n[4], z23 = n[5], rf = n[6];
			}
			const uint32_t r0 = __float_as_uint(rf.x), r1 = __float_as_uint(rf.y), r2 = __float_as_uint(rf.z), r3 = __float_as_uint(rf.w);
			const bool p0 = box_overlaps(q, x01.x, x01.y, y01.x, y01.y, z01.x, z01.y);
			const bool p1 = box_overlaps(q, x01.z, x01.w, y01.z, y01.w, z01.z, z01.w);
			const bool p2 = box_overlaps(q, x23.x, x23.y, y23.x, y23.y, z23.x, z23.y);
			const bool p3 = box_overlaps(q, x23.z, x23.w, y23.z, y23.w, z23.z, z23.w);
			// every passing slot but the first goes onto the stack, the last in node order first: they pop in node order
			const lanemask h0 = lanes_where(p0), h1 = lanes_where(p1), h2 = lanes_where(p2), h3 = lanes_where(p3);
			const lanemask any01 = h0 | h1, any012 = any01 | h2;
			st.push3(h3 & any012, r3, 0.f, h2 & any01, r2, 0.f, h1 & h0, r1, 0.f);
			ref = p0 ? r0 : p1 ? r1 : p2 ? r2 : p3 ? r3 : kRefPop;
		}
	}
	if (ref_is_leaf(ref)) {
		const uint32_t off = ref & (kMaxPrimOffset - 1);
		const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
		bool found = false;
		TriData tri = triangle_load(sc.tris, off);
		for (uint32_t i = 0; i < cnt && !(ANY && found); ++i) {
			const TriData cur = tri; // the next primitive of the leaf is on its way while this one is tested
			if (i + 1 < cnt)
				tri = triangle_load(sc.tris, off + i + 1);
			// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
			const float ax = cur.a.x, ay = cur.a.y, az = cur.a.z;
			const float bx = ax + cur.a.w, by = ay + cur.b.x, bz = az + cur.b.y;
			const float cx = ax + cur.b.z, cy = ay + cur.b.w, cz = az + cur.c.x;
			// rule 1, the box axes: exact comparisons of the inputs
			if (!box_overlaps(q, __builtin_fminf(__builtin_fminf(ax, bx), cx), __builtin_fmaxf(__builtin_fmaxf(ax, bx), cx), __builtin_fminf(__builtin_fminf(ay, by), cy),
			                  __builtin_fmaxf(__builtin_fmaxf(ay, by), cy), __builtin_fminf(__builtin_fminf(az, bz), cz), __builtin_fmaxf(__builtin_fmaxf(az, bz), cz)))
				continue;
			if (!box_member(ax, ay, az, bx, by, bz, cx, cy, cz, q.lx, q.ly, q.lz, q.hx, q.hy, q.hz))
				continue;
			q.count += 1u;
			if (ANY)
				found = true;
			else if ((int)(off + i) <= q.worst) // (a full row, or one of no entries, turns a larger index away)
				offer((int)(off + i));
		}
		ref = found ? kRefDone : kRefPop;
	}
	q.ref = ref;
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
