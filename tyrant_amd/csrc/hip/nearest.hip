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
// Pruning never changes the answer (DESIGN.md "Closest-point queries" derives the constants).  A box is skipped only when
//     lb2 - (kSlackFar2 * far2 + c1 * farInf)  >  best
// with lb2 / far2 the squared distance from the point to the box / to its farthest corner, farInf the largest per-axis
// distance to a corner and c1 = kSlackCoord * max |p_k|: the first term covers what the definition's value may undercut the
// true distance by (16 * 2^-24 * S^2, S <= 2 far) and the rounding of lb2 itself, the second that the stored boxes hold
// fl(vert + e1) where the definition's triangle has vert + e1.  `>`: a box at exactly the best value is still visited, since
// ties go to the lower index wherever it lies.
#include "device_common.hpp"
#include "nearest.hpp"
#include "query_common.hpp"

namespace tyr {

namespace {

constexpr float kUlpHalf = 5.9604644775390625e-8f; // 2^-24
constexpr float kSlackFar2 = 256.f * kUlpHalf;     // of far2: 76 needed with the value's cap of 16 (3.4x), 35 with the measured 5.7
constexpr float kSlackCoord = 64.f * kUlpHalf;     // of farInf * max |p_k|: 6 needed
constexpr float kInf = __builtin_inff();

// the value of a (point, triangle) pair: include/tyr_c.h "Closest-point queries", operation by operation (Ericson's
// closest-point test, the clamp, the squared length of what is left)
struct NearestValue {
	float F, u, v;
	uint32_t region;
	f3 c;
};
template <bool FULL>
__device__ __forceinline__ NearestValue nearest_value(const TriData& td, f3 p) {
	const f3 vert = mk3(td.a.x, td.a.y, td.a.z);
	const f3 e1 = mk3(td.a.w, td.b.x, td.b.y);
	const f3 e2 = mk3(td.b.z, td.b.w, td.c.x);
	const f3 ap = p - vert, bp = ap - e1, cp = ap - e2;
	const float d1 = dot(e1, ap), d2 = dot(e2, ap);
	const float d3 = dot(e1, bp), d4 = dot(e2, bp);
	const float d5 = dot(e1, cp), d6 = dot(e2, cp);
	const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
	const float g = d4 - d3, h = d5 - d6;
	// the first rule that holds (a comparison with a NaN is false)
	const bool r1 = d1 <= 0 && d2 <= 0;
	const bool r2 = d3 >= 0 && d4 <= d3;
	const bool r3 = vc <= 0 && d1 >= 0 && d3 <= 0;
	const bool r4 = d6 >= 0 && d5 <= d6;
	const bool r5 = vb <= 0 && d2 >= 0 && d6 <= 0;
	const bool r6 = va <= 0 && g >= 0 && h >= 0;
	const uint32_t rule = r1 ? 1u : r2 ? 2u : r3 ? 3u : r4 ? 4u : r5 ? 5u : r6 ? 6u : 7u;
	// the one division of the rule that holds, through selected operands (its result depends on them alone)
	const float num = rule == 3u ? d1 : rule == 5u ? d2 : rule == 6u ? g : 1.f;
	const float den = rule == 3u ? d1 - d3 : rule == 5u ? d2 - d6 : rule == 6u ? g + h : (va + vb) + vc;
	const float x = num / den;
	const float u = rule == 2u ? 1.f : rule == 3u ? x : rule == 6u ? 1.f - x : rule == 7u ? vb * x : 0.f;
	const float v = rule == 4u ? 1.f : (rule == 5u || rule == 6u) ? x : rule == 7u ? vc * x : 0.f;
	// the clamp: whatever rounding did, a point of the triangle (a NaN becomes 0)
	const float u1 = u > 0 ? u : 0.f, u2 = u1 < 1 ? u1 : 1.f;
	const float r = 1.f - u2;
	const float v1 = v > 0 ? v : 0.f, v2 = v1 < r ? v1 : r;
	const f3 q = mk3((ap.x - e1.x * u2) - e2.x * v2, (ap.y - e1.y * u2) - e2.y * v2, (ap.z - e1.z * u2) - e2.z * v2);
	NearestValue o;
	o.F = dot(q, q);
	if (FULL) {
		o.u = u2;
		o.v = v2;
		o.region = rule == 3u ? 4u : rule == 4u ? 3u : rule == 7u ? 0u : rule; // vertices 1 2 3, edges 4 5 6, the face 0
		o.c = mk3((vert.x + e1.x * u2) + e2.x * v2, (vert.y + e1.y * u2) + e2.y * v2, (vert.z + e1.z * u2) + e2.z * v2);
	}
	return o;
}

// the point a lane has in flight and what it has found so far
struct NearestLane {
	float px, py, pz;
	float c1;     // kSlackCoord * max |p_k|
	float best;   // the smallest value so far; bound2 until a triangle is accepted
	int prim;     // its triangle, -1: none
	uint32_t ref; // the lane's state
};

// a slot's box against the point: the pruning key lb2 - slack (see the head of this file); +inf for a slot that is skipped
__device__ __forceinline__ float box_key(const NearestLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	const float ax = lox - q.px, bx = q.px - hix, ay = loy - q.py, by = q.py - hiy, az = loz - q.pz, bz = q.pz - hiz;
	// (a synthetic record's boxes run from -inf to +inf: both differences are -inf, the distance 0, never NaN)
	const float dx = __builtin_fmaxf(__builtin_fmaxf(ax, bx), 0.f), dy = __builtin_fmaxf(__builtin_fmaxf(ay, by), 0.f), dz = __builtin_fmaxf(__builtin_fmaxf(az, bz), 0.f);
	const float fx = __builtin_fmaxf(fabsf(ax), fabsf(bx)), fy = __builtin_fmaxf(fabsf(ay), fabsf(by)), fz = __builtin_fmaxf(fabsf(az), fabsf(bz));
	const float lb2 = (dx * dx + dy * dy) + dz * dz;
	const float far2 = (fx * fx + fy * fy) + fz * fz;
	const float farInf = __builtin_fmaxf(__builtin_fmaxf(fx, fy), fz);
	const float slack = kSlackFar2 * far2 + q.c1 * farInf; // (c1 > 0: an infinite farInf gives +inf, not 0 * inf)
	const float key = lb2 - slack;
	// an unused slot's box is at +infinity: its lb2 is +inf, and with an infinite slack the key would be NaN
	return (lb2 < kInf && key <= q.best) ? key : kInf;
}

#define TYR_NEAREST_SWAP(a, b)                         \
	{                                                  \
		const bool s_ = k##a > k##b;                   \
		const float tk_ = s_ ? k##b : k##a;            \
		const uint32_t tr_ = s_ ? r##b : r##a;         \
		k##b = s_ ? k##a : k##b, r##b = s_ ? r##a : r##b; \
		k##a = tk_, r##a = tr_;                        \
	}

// One round of the wave's traversal, the shape of q_traverse (hip/query_common.hpp): the descent, one pop attempt and one quad
// step per lane per trip, until no lane descends -- or fewer than kQueryMinTraversing do and a lane is at a leaf or
// `canRefill()` says enough lanes could start new work; then one leaf per lane that is at one, primitives in array order.
template <class CanRefill>
__device__ __forceinline__ void n_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, NearestLane& q, CanRefill canRefill) {
	const uint32_t nStaged = sc.nStaged;
	// (the quad array's address as an opaque global-memory pointer: see q_traverse)
	auto held = (const __attribute__((address_space(1))) float4*)sc.quads;
	__asm__ volatile("" : "+s"(held));
	const float4* quads = (const float4*)held;
	const f3 p = mk3(q.px, q.py, q.pz);
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
			float pk;
			if (st.pop(pr, pk)) {
				if (pk <= q.best) // the entry's key against what has been found since it was pushed
					ref = pr;
			} else {
				ref = kRefDone;
			}
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
			uint32_t r0 = __float_as_uint(rf.x), r1 = __float_as_uint(rf.y), r2 = __float_as_uint(rf.z), r3 = __float_as_uint(rf.w);
			float k0 = box_key(q, x01.x, x01.y, y01.x, y01.y, z01.x, z01.y);
			float k1 = box_key(q, x01.z, x01.w, y01.z, y01.w, z01.z, z01.w);
			float k2 = box_key(q, x23.x, x23.y, y23.x, y23.y, z23.x, z23.y);
			float k3 = box_key(q, x23.z, x23.w, y23.z, y23.w, z23.z, z23.w);
			// the four by key, nearest first: a sorting network of selects (skipped slots carry +inf and end up last)
			TYR_NEAREST_SWAP(0, 1)
			TYR_NEAREST_SWAP(2, 3)
			TYR_NEAREST_SWAP(0, 2)
			TYR_NEAREST_SWAP(1, 3)
			TYR_NEAREST_SWAP(1, 2)
			st.push3(lanes_where(k3 < kInf), r3, k3, lanes_where(k2 < kInf), r2, k2, lanes_where(k1 < kInf), r1, k1);
			ref = k0 < kInf ? r0 : kRefPop;
		}
	}
	if (ref_is_leaf(ref)) {
		const uint32_t off = ref & (kMaxPrimOffset - 1);
		const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
		TriData tri = triangle_load(sc.tris, off);
		for (uint32_t i = 0; i < cnt; ++i) {
			const TriData cur = tri; // the next primitive of the leaf is on its way while this one is evaluated
			if (i + 1 < cnt)
				tri = triangle_load(sc.tris, off + i + 1);
			const float F = nearest_value<false>(cur, p).F;
			const int prim = (int)(off + i);
			if (F < q.best || (F == q.best && prim < q.prim)) {
				q.best = F;
				q.prim = prim;
			}
		}
		ref = kRefPop;
	}
	q.ref = ref;
}

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
		n_traverse(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<NearestParams>().error);
}

void launch_nearest(const NearestParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	const Tuning t{}; // the occupancy query's answer, never a tuning override: queries do not follow the render's launch shape
	hipLaunchKernelGGL(k_query_nearest, dim3(persistent_blocks(k_query_nearest, P.n, t, numCUs, lc.perCU[kLcNearest][0])), dim3(kBlock), 0, stream, P);
}

} // namespace tyr
