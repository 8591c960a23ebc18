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
// The quad step is box.hip's, a private copy of it (that unit's kernels stay as they are): four closed interval tests of a slot's
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

namespace tyr {

namespace {

// ---- the member test of a (query, scene triangle) pair: include/tyr_c.h "Triangle-overlap queries", rule 2 -------------------

struct D3 {
	double x, y, z;
};

__device__ __forceinline__ double mind(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double maxd(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ D3 sub(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(const D3& a, const D3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// Does `axis` separate {p0, p1, p2} from {q0 = 0, q1, q2}?  All points go through the same dot(axis, x).  q0 = Q0 - Q0 is +0 for a
// finite corner and dot(axis, 0) is a zero of either sign: as an operand of <, of min and of max it is 0.0 itself, the one term
// that is dropped.
__device__ __forceinline__ bool axis_separates(const D3& axis, const D3& p0, const D3& p1, const D3& p2, const D3& q1, const D3& q2) {
	const double a = dot(axis, p0), b = dot(axis, p1), c = dot(axis, p2);
	const double u = dot(axis, q1), v = dot(axis, q2);
	const double pmin = mind(mind(a, b), c), pmax = maxd(maxd(a, b), c);
	const double qmin = mind(mind(0.0, u), v), qmax = maxd(maxd(0.0, u), v);
	return pmax < qmin || qmax < pmin;
}

// rule 2 for a pair that rules 0 and 1 let through: P the query's binary32 corners, Q the scene triangle's
__device__ __forceinline__ bool tri_member(float p0x, float p0y, float p0z, float p1x, float p1y, float p1z, float p2x, float p2y, float p2z, float q0x, float q0y, float q0z,
                                           float q1x, float q1y, float q1z, float q2x, float q2y, float q2z) {
	const D3 Q0 = {(double)q0x, (double)q0y, (double)q0z};
	const D3 p0 = {(double)p0x - Q0.x, (double)p0y - Q0.y, (double)p0z - Q0.z};
	const D3 p1 = {(double)p1x - Q0.x, (double)p1y - Q0.y, (double)p1z - Q0.z};
	const D3 p2 = {(double)p2x - Q0.x, (double)p2y - Q0.y, (double)p2z - Q0.z};
	const D3 q0 = {0.0, 0.0, 0.0};
	const D3 q1 = {(double)q1x - Q0.x, (double)q1y - Q0.y, (double)q1z - Q0.z};
	const D3 q2 = {(double)q2x - Q0.x, (double)q2y - Q0.y, (double)q2z - Q0.z};
	// the scene triangle's plane, then the query's
	const D3 f0 = sub(q1, q0);
	const D3 m = cross(f0, sub(q2, q0));
	if (axis_separates(m, p0, p1, p2, q1, q2))
		return false;
	const D3 e0 = sub(p1, p0);
	const D3 n = cross(e0, sub(p2, p0));
	if (axis_separates(n, p0, p1, p2, q1, q2))
		return false;
	// the nine edge crosses, the query's edge outer
	const D3 e1 = sub(p2, p1), e2 = sub(p0, p2);
	const D3 f1 = sub(q2, q1), f2 = sub(q0, q2);
	if (axis_separates(cross(e0, f0), p0, p1, p2, q1, q2) || axis_separates(cross(e0, f1), p0, p1, p2, q1, q2) || axis_separates(cross(e0, f2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(cross(e1, f0), p0, p1, p2, q1, q2) || axis_separates(cross(e1, f1), p0, p1, p2, q1, q2) || axis_separates(cross(e1, f2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(cross(e2, f0), p0, p1, p2, q1, q2) || axis_separates(cross(e2, f1), p0, p1, p2, q1, q2) || axis_separates(cross(e2, f2), p0, p1, p2, q1, q2))
		return false;
	// the six in-plane axes: what separates coplanar triangles
	if (axis_separates(cross(n, e0), p0, p1, p2, q1, q2) || axis_separates(cross(n, e1), p0, p1, p2, q1, q2) || axis_separates(cross(n, e2), p0, p1, p2, q1, q2))
		return false;
	if (axis_separates(cross(m, f0), p0, p1, p2, q1, q2) || axis_separates(cross(m, f1), p0, p1, p2, q1, q2) || axis_separates(cross(m, f2), p0, p1, p2, q1, q2))
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

// One round of the wave's traversal, as box.hip's b_traverse: the descent, one pop attempt and one quad step per lane per trip,
// until no lane descends -- or fewer than kQueryMinTraversing do and a lane is at a leaf or `canRefill()` says enough lanes could
// start new work; then one leaf per lane that is at one, primitives in array order, each member counted and handed to
// `offer(prim)`.
template <bool ANY, class CanRefill, class Offer>
__device__ __forceinline__ void t_traverse(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, TriLane& q, bool skipShared, CanRefill canRefill,
                                           Offer offer) {
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
			const TriBox bb = box_of(q);
			const bool p0 = box_overlaps(bb, x01.x, x01.y, y01.x, y01.y, z01.x, z01.y);
			const bool p1 = box_overlaps(bb, x01.z, x01.w, y01.z, y01.w, z01.z, z01.w);
			const bool p2 = box_overlaps(bb, x23.x, x23.y, y23.x, y23.y, z23.x, z23.y);
			const bool p3 = box_overlaps(bb, x23.z, x23.w, y23.z, y23.w, z23.z, z23.w);
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
		const TriBox bb = box_of(q);
		TriData tri = triangle_load(sc.tris, off);
		for (uint32_t i = 0; i < cnt && !(ANY && found); ++i) {
			const TriData cur = tri; // the next primitive of the leaf is on its way while this one is tested
			if (i + 1 < cnt)
				tri = triangle_load(sc.tris, off + i + 1);
			// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
			const float q0x = cur.a.x, q0y = cur.a.y, q0z = cur.a.z;
			const float q1x = q0x + cur.a.w, q1y = q0y + cur.b.x, q1z = q0z + cur.b.y;
			const float q2x = q0x + cur.b.z, q2y = q0y + cur.b.w, q2z = q0z + cur.c.x;
			// rule 1, the coordinate axes: exact comparisons of the inputs
			if (!box_overlaps(bb, min3f(q0x, q1x, q2x), max3f(q0x, q1x, q2x), min3f(q0y, q1y, q2y), max3f(q0y, q1y, q2y), min3f(q0z, q1z, q2z), max3f(q0z, q1z, q2z)))
				continue;
			// rule 0: a corner of the query equal to a corner of the triangle (==: -0 equals +0)
			if (skipShared) {
				const bool s0 = (q.ax == q0x && q.ay == q0y && q.az == q0z) || (q.ax == q1x && q.ay == q1y && q.az == q1z) || (q.ax == q2x && q.ay == q2y && q.az == q2z);
				const bool s1 = (q.bx == q0x && q.by == q0y && q.bz == q0z) || (q.bx == q1x && q.by == q1y && q.bz == q1z) || (q.bx == q2x && q.by == q2y && q.bz == q2z);
				const bool s2 = (q.cx == q0x && q.cy == q0y && q.cz == q0z) || (q.cx == q1x && q.cy == q1y && q.cz == q1z) || (q.cx == q2x && q.cy == q2y && q.cz == q2z);
				if (s0 || s1 || s2)
					continue;
			}
			if (!tri_member(q.ax, q.ay, q.az, q.bx, q.by, q.bz, q.cx, q.cy, q.cz, q0x, q0y, q0z, q1x, q1y, q1z, q2x, q2y, q2z))
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
