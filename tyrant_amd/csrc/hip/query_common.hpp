// query_common.hpp -- the persistent per-lane traversal loop of the ray queries (hip/query.hip) and of the guide passes
// (hip/aov.hip), once: the staged top nodes, the chunked ticket feed, the descent with its exit test, the leaf loop with the
// accept rule, the spheres' closest-hit pre-test and the overflow report.  A kernel supplies what a lane's item is (a
// caller's ray, a pixel's samples), how its ray is made and where its answer goes; the lane states are those of k_trace_flat
// (hip/traverse.hpp: interior ref | leaf ref | kRefPop | kRefDone).
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

// One round of the wave's traversal (`live`: the lane holds an item; a lane without a ray in the tree has q.ref == kRefDone).
// The descent, one pop attempt and one quad test per lane per trip, until no lane descends -- or fewer than
// kQueryMinTraversing do and a lane is at a leaf or `canRefill()` says enough lanes could start new work; then one leaf per
// lane that is at one: bvh.h:129-140 (closest hit) / bvh.h:229-238 (any hit), primitives in array order.  The accept rules
// of these kernels are the two in the leaf loop below.
template <bool ANY, class CanRefill>
__device__ __forceinline__ void q_traverse(const DevScene& sc, LdsStack<kQueryStackLds, !ANY>& st, const float4* stagedNodes, QueryRay& q, bool live, CanRefill canRefill) {
	const uint32_t nStaged = sc.nStaged;
	// The quad array's address, read here into a global-memory pointer that is opaque from here on: as a plain read of the
	// by-value argument it is rematerialised where scalar registers run short -- in the guide kernels an s_load and its wait
	// in every trip of the descent.  (Address space 1: through a generic pointer the node loads would become flat loads.)
	auto held = (const __attribute__((address_space(1))) float4*)sc.quads;
	__asm__ volatile("" : "+s"(held));
	const float4* quads = (const float4*)held;
	const bool allRegular = (__ballot(live && !q.regular) == 0ull);
	const RayConst r = { mk3(q.ox, q.oy, q.oz), mk3(q.dx, q.dy, q.dz), mk3(q.ix, q.iy, q.iz), q.ix < 0, q.iy < 0, q.iz < 0 }; // bvh.h:120-121
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
			if (st.pop(pr, pt)) {
				if (pt < q.dist) // the pop-time half of Bbox.h:61 (any hit keeps no entry distance: -inf, always taken)
					ref = pr;
			} else {
				ref = kRefDone;
			}
		}
		if ((int)ref >= 0) {
			const QuadHits h = allRegular ? test_quad<true, !ANY, true>(quads, ref, r, q.dist, stagedNodes, nStaged) : test_quad<false, !ANY, true>(quads, ref, r, q.dist, stagedNodes, nStaged);
			const lanemask any01 = h.hit[0] | h.hit[1], any012 = any01 | h.hit[2];
			st.push3(h.hit[3] & any012, h.ref[3], h.t[3], h.hit[2] & any01, h.ref[2], h.t[2], h.hit[1] & h.hit[0], h.ref[1], h.t[1]);
			ref = lane_in(h.hit[0]) ? h.ref[0] : lane_in(h.hit[1]) ? h.ref[1] : lane_in(h.hit[2]) ? h.ref[2] : lane_in(h.hit[3]) ? h.ref[3] : kRefPop;
		}
	}
	if (ref_is_leaf(ref)) {
		const uint32_t off = ref & (kMaxPrimOffset - 1);
		const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
		bool found = false;
		TriData tri = triangle_load(sc.tris, off);
		for (uint32_t i = 0; i < cnt && !found; ++i) {
			const TriData cur = tri; // the next primitive of the leaf is on its way while this one is tested
			if (i + 1 < cnt)
				tri = triangle_load(sc.tris, off + i + 1);
			const float t = triangle_test(cur, r);
			if (ANY) {
				found = (t > kEpsilon && ((q.dist - t) > kEpsilon)); // bvh.h:232-236
			} else if (t > kEpsilon && t < q.dist && ((q.dist - t) > kEpsilon)) { // bvh.h:133-137
				q.prim = (int)(off + i);
				q.dist = t;
				q.hitTri = true;
			}
		}
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
