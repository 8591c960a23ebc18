// query_common.hpp -- what the batched queries on the uploaded scene and the guide passes (hip/aov.hip) share, once: the staged
// top nodes, the chunked ticket feed, the overflow report, and a round of the wave's traversal with its pieces -- the pinned
// quad pointer, the exit test, the leaf iterator, a triangle's corner box -- built into three descents:
//   keyed_round    a bound that shrinks: slots keyed, sorted, re-tested when popped   (nearest, nearest_k, sweep, segment)
//   overlap_round  a bound that never changes: slots tested, node order               (box, tri)
//   ray_descent    test_quad against a ray; q_traverse adds the ray queries' leaf     (query, occlusion, aov; hits)
// A kernel supplies what a lane's item is (a caller's ray, a pixel's samples, a point, a box), its slot test, what it does
// with a leaf and where its answer goes; its outer loop (refill, top_up, finish) is its own.  The lane states are those of
// k_trace_flat (hip/traverse.hpp: interior ref | leaf ref | kRefPop | kRefDone).
#pragma once

#include "device_common.hpp"
#include "query.hpp"

namespace tyr {

constexpr int kQueryStackLds = 12;  // LDS stack entries per lane: 24,576 B (closest) + 7,168 B staged nodes, five blocks per CU
constexpr uint32_t kQueryMinTraversing = 32; // leave the descent below this many descending lanes when leaves or a refill wait
constexpr uint32_t kQueryRefillMinIdle = 16; // refill a wave once this many lanes are free

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff(); }

// the first nStaged quad records into the block's 7 * kStagedNodes LDS array, vector-major (hip/traverse.hpp kStagedNodes)
__device__ __forceinline__ void q_stage_nodes(float4* stagedNodes, const DevScene& sc) {
	const uint32_t nStaged = sc.nStaged;
	for (uint32_t i = threadIdx.x; i < 7 * nStaged; i += kBlock) {
		const uint32_t v = i / nStaged, k = i - v * nStaged;
		stagedNodes[v * kStagedNodes + k] = sc.quads[8 * k + v];
	}
	__syncthreads();
}

constexpr uint32_t kNoItem = ~0u; // no index: a batch of n <= 2^32 - 1 items ends at index 2^32 - 2

// one wave's private range of item indices [next, end), drawn `chunk` items at a time from the launch's ticket word
struct QueryFeed {
	uint32_t next, end, chunk, n;
	bool exhausted; // the batch is used up: nothing more to draw
	__device__ __forceinline__ void init(uint32_t nItems) {
		next = end = 0;
		n = nItems;
		exhausted = (n == 0);
		// small batches: smaller chunks, so that the items spread over more waves (never below one wave's worth)
		const uint32_t waves = gridDim.x * (blockDim.x / 64u);
		chunk = 256;
		while (chunk > 64 && (unsigned long long)waves * chunk > n)
			chunk >>= 1;
	}
	// false once the batch is used up
	__device__ __forceinline__ bool draw(uint32_t* ticket, uint32_t lane) {
		uint32_t t = 0;
		if (lane == 0)
			t = atomicAdd(ticket, 1u);
		t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
		const unsigned long long start = (unsigned long long)t * chunk;
		if (start >= n)
			return false;
		next = (uint32_t)start;
		end = (start + chunk < n) ? (uint32_t)(start + chunk) : n;
		return true;
	}
	// Once kQueryRefillMinIdle lanes of the wave are idle (!live): deals the next indices to them by rank, drawing chunks as
	// they run out.  Returns the index a lane was handed, kNoItem on every other lane (by value: with the index written
	// through a reference the guide kernels shuffled 30-odd registers around every finished ray).  `ticket()` is the launch's
	// ticket word, asked for at each draw (a kernarg_view read: not held in scalar registers through the descent).
	template <class Ticket>
	__device__ __forceinline__ uint32_t refill(bool live, uint32_t lane, Ticket ticket) {
		const unsigned long long idleMask = __ballot(!live);
		const uint32_t nIdle = (uint32_t)__popcll(idleMask);
		uint32_t item = kNoItem;
		if (!exhausted && nIdle >= kQueryRefillMinIdle) {
			const uint32_t rank = lanes_below(idleMask);
			uint32_t got = 0;
			while (got < nIdle) {
				if (next == end && !draw(ticket(), lane)) {
					exhausted = true;
					break;
				}
				const uint32_t avail = end - next, room = nIdle - got;
				const uint32_t take = avail < room ? avail : room;
				if (!live && rank >= got && rank < got + take)
					item = next + (rank - got);
				next += take;
				got += take;
			}
		}
		return item;
	}
	// after a refill whose items mostly ended at once: worth topping the wave up again before it descends
	__device__ __forceinline__ bool top_up(bool live) const {
		return !exhausted && (uint32_t)__popcll(__ballot(live)) < kQueryMinTraversing && (uint32_t)__popcll(__ballot(!live)) >= kQueryRefillMinIdle;
	}
};

// the ray a lane has in flight and what it has found so far
struct QueryRay {
	float ox, oy, oz, dx, dy, dz, ix, iy, iz; // origin, direction, 1 / direction (bvh.h:120)
	bool regular;                             // ray_is_regular: test_quad's finite-1/d form applies
	float dist;                               // closest hit: the nearest accepted distance so far; any hit: tmax
	uint32_t ref;                             // the lane's state
	int prim, sphere;                         // closest hit: the winning triangle (hitTri) or sphere, -1: none
	bool hitTri, occluded;                    // occluded: any hit's answer
	__device__ __forceinline__ void start(const RayConst& r, float bound) {
		ox = r.o.x, oy = r.o.y, oz = r.o.z, dx = r.d.x, dy = r.d.y, dz = r.d.z, ix = r.inv.x, iy = r.inv.y, iz = r.inv.z;
		regular = ray_is_regular(r);
		dist = bound;
		prim = sphere = -1;
		hitTri = occluded = false;
	}
};

// the sphere half of intersect_scene (kernel.cu:130-135): the seven spheres in reverse order, the nearest below q.dist
__device__ __forceinline__ void q_spheres_closest(const tyr_sphere* spheres, const RayConst& r, QueryRay& q) {
#pragma unroll
	for (int s = TYR_NUM_SPHERES; s--;) {
		const float d = sphere_intersect(spheres[s], r.o, r.d);
		if (d && d < q.dist) {
			q.dist = d;
			q.sphere = s;
		}
	}
}

// ---- the pieces of a round of the wave's traversal, for every descent on the quad tree ----------------------------------------
// A round is: the descent -- per trip the exit test, one pop attempt, one record fetch (fetch_quad, hip/traverse.hpp), a test
// of the record's four slots and the pushes -- and then one leaf per lane that is at one.  Lane states are k_trace_flat's
// (hip/traverse.hpp: interior ref | leaf ref | kRefPop | kRefDone); a lane without an item in the tree holds kRefDone.

// The quad array's address, read here into a global-memory pointer that is opaque from here on: as a plain read of the
// by-value argument it is rematerialised where scalar registers run short -- in the guide kernels an s_load and its wait
// in every trip of the descent.  (Address space 1: through a generic pointer the node loads would become flat loads.)
__device__ __forceinline__ const float4* pinned_quads(const DevScene& sc) {
	auto held = (const __attribute__((address_space(1))) float4*)sc.quads;
	__asm__ volatile("" : "+s"(held));
	return (const float4*)held;
}

// The exit test of the descent: no lane descends -- or fewer than kQueryMinTraversing do and a lane is at a leaf or
// `canRefill(ref)` says enough lanes could start new work.
template <class CanRefill>
__device__ __forceinline__ bool descent_ends(uint32_t ref, CanRefill canRefill) {
	const uint32_t nTrav = (uint32_t)__popcll(lanes_traversing(ref));
	return nTrav == 0 || (nTrav < kQueryMinTraversing && (lanes_at_leaf(ref) != 0ull || canRefill(ref)));
}

// A leaf's primitives in array order, each handed to `body(cur, prim)` while the next one's record is on its way.  STOPS: the
// body returns "found" and a true ends the leaf (the ANY forms); otherwise its result, if any, is not looked at.
template <bool STOPS, class Body>
__device__ __forceinline__ bool leaf_prims(const float4* __restrict__ tris, uint32_t leaf, Body body) {
	const uint32_t off = leaf & (kMaxPrimOffset - 1);
	const uint32_t cnt = ((leaf >> 26) & 31u) + 1u;
	bool found = false;
	TriData tri = triangle_load(tris, off);
	for (uint32_t i = 0; i < cnt && !(STOPS && found); ++i) {
		const TriData cur = tri;
		if (i + 1 < cnt)
			tri = triangle_load(tris, off + i + 1);
		if constexpr (STOPS)
			found = body(cur, (int)(off + i));
		else
			body(cur, (int)(off + i));
	}
	return found;
}

// The corners tyr_triangle_bboxes bounds -- vert and the binary32 sums vert + e1, vert + e2 -- and their box: what a leaf of
// the stored tree bounds, so a slot's test applies to a single triangle as it stands.
struct CornerBox {
	f3 a, b, c;
	float lox, hix, loy, hiy, loz, hiz;
};
__device__ __forceinline__ CornerBox tri_corner_box(const TriData& t) {
	CornerBox o;
	o.a = mk3(t.a.x, t.a.y, t.a.z);
	o.b = mk3(t.a.x + t.a.w, t.a.y + t.b.x, t.a.z + t.b.y);
	o.c = mk3(t.a.x + t.b.z, t.a.y + t.b.w, t.a.z + t.c.x);
	o.lox = __builtin_fminf(__builtin_fminf(o.a.x, o.b.x), o.c.x), o.hix = __builtin_fmaxf(__builtin_fmaxf(o.a.x, o.b.x), o.c.x);
	o.loy = __builtin_fminf(__builtin_fminf(o.a.y, o.b.y), o.c.y), o.hiy = __builtin_fmaxf(__builtin_fmaxf(o.a.y, o.b.y), o.c.y);
	o.loz = __builtin_fminf(__builtin_fminf(o.a.z, o.b.z), o.c.z), o.hiz = __builtin_fmaxf(__builtin_fmaxf(o.a.z, o.b.z), o.c.z);
	return o;
}

// ---- the two box descents ------------------------------------------------------------------------------------------------------

// one compare-exchange of the keyed descent's sorting network: afterwards ka <= kb, each key with its reference
__device__ __forceinline__ void key_swap(float& ka, uint32_t& ra, float& kb, uint32_t& rb) {
	const bool s = ka > kb;
	const float tk = s ? kb : ka;
	const uint32_t tr = s ? rb : ra;
	kb = s ? ka : kb, rb = s ? ra : rb;
	ka = tk, ra = tr;
}

// One round of a query whose bound shrinks as it finds things (nearest, nearest_k, sweep, segment).  `keyOf(lox, hix, loy, hiy,
// loz, hiz)` is a slot's key, a lower bound of every value below the slot, +inf for a slot that is skipped.  A quad step
// orders the four slots by key, descends into the nearest and pushes the others farthest first; a popped entry is taken if
// its key is still `<= bound`, the lane's bound as the round begins (it changes at leaves only).  `leaf(ref)` takes a reached
// leaf.  Returns the lane's new state.
// The re-test is written `pk <= bound` for every caller, where hip/segment.hip used to write `!(pk > bound)`: the two differ
// only for a NaN, and neither side is one.  A key is pushed only when `key < +inf` holds, which a NaN fails.  A bound starts
// as max_dist * max_dist behind `max_dist >= 0`, as +inf, or as a finite tmax, and later takes only values that passed
// `value < bound` or `value == bound` (the kernels' take rules), which a NaN fails too.
template <class CanRefill, class KeyOf, class Leaf>
__device__ __forceinline__ uint32_t keyed_round(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, uint32_t ref, float bound, CanRefill canRefill, KeyOf keyOf,
                                                Leaf leaf) {
	constexpr float kSkipped = __builtin_inff();
	const uint32_t nStaged = sc.nStaged;
	const float4* quads = pinned_quads(sc);
	while (!descent_ends(ref, canRefill)) {
		if (ref == kRefPop) {
			uint32_t pr;
			float pk;
			if (st.pop(pr, pk)) {
				if (pk <= bound) // the entry's key against what has been found since it was pushed
					ref = pr;
			} else {
				ref = kRefDone;
			}
		}
		if ((int)ref >= 0) {
			QuadRecord n;
			fetch_quad<true>(n, quads, ref, stagedNodes, nStaged);
			uint32_t r0 = __float_as_uint(n.rf.x), r1 = __float_as_uint(n.rf.y), r2 = __float_as_uint(n.rf.z), r3 = __float_as_uint(n.rf.w);
			float k0 = keyOf(n.x01.x, n.x01.y, n.y01.x, n.y01.y, n.z01.x, n.z01.y);
			float k1 = keyOf(n.x01.z, n.x01.w, n.y01.z, n.y01.w, n.z01.z, n.z01.w);
			float k2 = keyOf(n.x23.x, n.x23.y, n.y23.x, n.y23.y, n.z23.x, n.z23.y);
			float k3 = keyOf(n.x23.z, n.x23.w, n.y23.z, n.y23.w, n.z23.z, n.z23.w);
			// the four by key, nearest first: a sorting network of selects (skipped slots carry +inf and end up last)
			key_swap(k0, r0, k1, r1);
			key_swap(k2, r2, k3, r3);
			key_swap(k0, r0, k2, r2);
			key_swap(k1, r1, k3, r3);
			key_swap(k1, r1, k2, r2);
			st.push3(lanes_where(k3 < kSkipped), r3, k3, lanes_where(k2 < kSkipped), r2, k2, lanes_where(k1 < kSkipped), r1, k1);
			ref = k0 < kSkipped ? r0 : kRefPop;
		}
	}
	if (ref_is_leaf(ref)) {
		leaf(ref);
		ref = kRefPop;
	}
	return ref;
}

// One round of a query whose bound never changes (box, tri).  `overlaps(lox, hix, loy, hiy, loz, hiz)` says whether a slot can
// hold a member.  A quad step descends into the first slot that passes in node order and pushes the others, the last first, so
// that they pop in node order; there is no key, no sort and no entry distance, and a popped entry is always taken.
// `leaf(ref)` takes a reached leaf and returns whether the lane's item is finished with it (the ANY forms' first member).
// Returns the lane's new state.
template <class CanRefill, class Overlaps, class Leaf>
__device__ __forceinline__ uint32_t overlap_round(const DevScene& sc, LdsStack<kQueryStackLds, false>& st, const float4* stagedNodes, uint32_t ref, CanRefill canRefill, Overlaps overlaps,
                                                  Leaf leaf) {
	const uint32_t nStaged = sc.nStaged;
	const float4* quads = pinned_quads(sc);
	while (!descent_ends(ref, canRefill)) {
		if (ref == kRefPop) {
			uint32_t pr;
			float pt;
			ref = st.pop(pr, pt) ? pr : kRefDone;
		}
		if ((int)ref >= 0) {
			QuadRecord n;
			fetch_quad<true>(n, quads, ref, stagedNodes, nStaged);
			const uint32_t r0 = __float_as_uint(n.rf.x), r1 = __float_as_uint(n.rf.y), r2 = __float_as_uint(n.rf.z), r3 = __float_as_uint(n.rf.w);
			const bool p0 = overlaps(n.x01.x, n.x01.y, n.y01.x, n.y01.y, n.z01.x, n.z01.y);
			const bool p1 = overlaps(n.x01.z, n.x01.w, n.y01.z, n.y01.w, n.z01.z, n.z01.w);
			const bool p2 = overlaps(n.x23.x, n.x23.y, n.y23.x, n.y23.y, n.z23.x, n.z23.y);
			const bool p3 = overlaps(n.x23.z, n.x23.w, n.y23.z, n.y23.w, n.z23.z, n.z23.w);
			const lanemask h0 = lanes_where(p0), h1 = lanes_where(p1), h2 = lanes_where(p2), h3 = lanes_where(p3);
			const lanemask any01 = h0 | h1, any012 = any01 | h2;
			st.push3(h3 & any012, r3, 0.f, h2 & any01, r2, 0.f, h1 & h0, r1, 0.f);
			ref = p0 ? r0 : p1 ? r1 : p2 ? r2 : p3 ? r3 : kRefPop;
		}
	}
	if (ref_is_leaf(ref))
		ref = leaf(ref) ? kRefDone : kRefPop;
	return ref;
}

// ---- the ray queries' round ----------------------------------------------------------------------------------------------------

// The descent of a ray: test_quad against `bound` (closest hit: the nearest accepted distance so far; any hit: tmax, which never
// shrinks), in the reference's visit order with entry distances (!ANY) or in node order without (ANY: no entry is re-tested when
// it is popped, and the set of leaves reached does not depend on the order, hip/traverse.hpp "Exactness").
template <bool ANY, class CanRefill>
__device__ __forceinline__ uint32_t ray_descent(const float4* quads, LdsStack<kQueryStackLds, !ANY>& st, const float4* stagedNodes, uint32_t nStaged, const RayConst& r, bool allRegular,
                                                float bound, uint32_t ref, CanRefill canRefill) {
	for (;;) {
		// (descent_ends' test, written out: called as a function here it costs every ray kernel two vector registers, and
		// k_query_hits<false> a wave per SIMD with them -- profiles/query_descent_refactor_isa.txt)
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
			if (st.pop(pr, pt)) {
				if (ANY || pt < bound) // the pop-time half of Bbox.h:61 (any hit keeps no entry distance: always taken)
					ref = pr;
			} else {
				ref = kRefDone;
			}
		}
		if ((int)ref >= 0) {
			const QuadHits h = allRegular ? test_quad<true, !ANY, true>(quads, ref, r, bound, stagedNodes, nStaged) : test_quad<false, !ANY, true>(quads, ref, r, bound, stagedNodes, nStaged);
			const lanemask any01 = h.hit[0] | h.hit[1], any012 = any01 | h.hit[2];
			st.push3(h.hit[3] & any012, h.ref[3], h.t[3], h.hit[2] & any01, h.ref[2], h.t[2], h.hit[1] & h.hit[0], h.ref[1], h.t[1]);
			ref = lane_in(h.hit[0]) ? h.ref[0] : lane_in(h.hit[1]) ? h.ref[1] : lane_in(h.hit[2]) ? h.ref[2] : lane_in(h.hit[3]) ? h.ref[3] : kRefPop;
		}
	}
	return ref;
}

// One round of the ray queries and guide passes (`live`: the lane holds an item): the descent, then one leaf per lane that is at
// one: bvh.h:129-140 (closest hit) / bvh.h:229-238 (any hit), primitives in array order.  The accept rules of these kernels are
// the two in the leaf below.
template <bool ANY, class CanRefill>
__device__ __forceinline__ void q_traverse(const DevScene& sc, LdsStack<kQueryStackLds, !ANY>& st, const float4* stagedNodes, QueryRay& q, bool live, CanRefill canRefill) {
	const uint32_t nStaged = sc.nStaged;
	const float4* quads = pinned_quads(sc);
	const bool allRegular = (__ballot(live && !q.regular) == 0ull);
	const RayConst r = { mk3(q.ox, q.oy, q.oz), mk3(q.dx, q.dy, q.dz), mk3(q.ix, q.iy, q.iz), q.ix < 0, q.iy < 0, q.iz < 0 }; // bvh.h:120-121
	uint32_t ref = ray_descent<ANY>(quads, st, stagedNodes, nStaged, r, allRegular, q.dist, q.ref, canRefill);
	if (ref_is_leaf(ref)) {
		const bool found = leaf_prims<true>(sc.tris, ref, [&](const TriData& cur, int prim) {
			const float t = triangle_test(cur, r);
			if (ANY)
				return t > kEpsilon && ((q.dist - t) > kEpsilon); // bvh.h:232-236
			if (t > kEpsilon && t < q.dist && ((q.dist - t) > kEpsilon)) { // bvh.h:133-137
				q.prim = prim;
				q.dist = t;
				q.hitTri = true;
			}
			return false;
		});
		q.occluded = q.occluded || found;
		ref = found ? kRefDone : kRefPop;
	}
	q.ref = ref;
}

// the launch's end: one error bit for the wave if a lane's stack overflowed (bvh.h:124's 64 entries)
__device__ __forceinline__ void q_report_overflow(bool overflow, uint32_t lane, uint32_t* error) {
	if (__ballot(overflow) != 0ull && lane == 0)
		atomicOr(error, kQueryErrStackOverflow);
}

} // namespace tyr
