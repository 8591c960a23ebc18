// nearest_common.hpp -- what the point queries share (hip/nearest.hip: the nearest triangle; hip/nearest_k.hip: the k nearest
// and those within a radius): the value of a (point, triangle) pair, the pruning key of a box with its slack, and the round
// of traversal that orders a quad record's four slots by that key and takes a leaf's primitives.  Device code of the two
// units only.
//
// Pruning never changes the answer (DESIGN.md "Closest-point queries" derives the constants).  A box is skipped only when
//     lb2 - (kSlackFar2 * far2 + c1 * farInf)  >  bound
// with lb2 / far2 the squared distance from the point to the box / to its farthest corner, farInf the largest per-axis
// distance to a corner and c1 = kSlackCoord * max |p_k|: the first term covers what the definition's value may undercut the
// true distance by (16 * 2^-24 * S^2, S <= 2 far) and the rounding of lb2 itself, the second that the stored boxes hold
// fl(vert + e1) where the definition's triangle has vert + e1.  `>`: a box at exactly the bound is still visited, since
// ties go to the lower index wherever it lies.  The bound is the lane's `best`: the best value so far for the nearest
// triangle, the worst value a point's row keeps (or its radius) for the k nearest.
#pragma once

#include "device_common.hpp"
#include "query_common.hpp"

namespace tyr {

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

// A slot's box against a lane's point: the pruning key lb2 - slack (see the head of this file); +inf for a slot that is
// skipped.  Lane: px, py, pz, c1 = kSlackCoord * max |p_k|, and best, the bound.
template <class Lane>
__device__ __forceinline__ float box_key(const Lane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
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
// `canRefill()` says enough lanes could start new work; then one leaf per lane that is at one, primitives in array order,
// each one's value handed to `take(q, F, prim)`.  A quad step orders the four slots by their keys, descends into the nearest
// and pushes the others farthest first; a popped entry's key is tested against the bound again.
template <class Lane, class CanRefill, class Take>
__device__ __forceinline__ void n_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, Lane& q, CanRefill canRefill, Take take) {
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
			take(q, F, (int)(off + i));
		}
		ref = kRefPop;
	}
	q.ref = ref;
}

} // namespace tyr
