// nearest_common.hpp -- what the point queries share (hip/nearest.hip: the nearest triangle; hip/nearest_k.hip: the k nearest
// and those within a radius): the value of a (point, triangle) pair, the pruning key of a box with its slack, and the round
// of traversal: the keyed descent of hip/query_common.hpp on that key, and a leaf's primitives.  Device code of the two
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

// One round of the wave's traversal: the keyed descent (keyed_round, hip/query_common.hpp) on box_key against the lane's
// `best`, then one leaf per lane that is at one, each primitive's value handed to `take(q, F, prim)`.
template <class Lane, class CanRefill, class Take>
__device__ __forceinline__ void n_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, Lane& q, CanRefill canRefill, Take take) {
	const f3 p = mk3(q.px, q.py, q.pz);
	q.ref = keyed_round(
		sc, st, stagedNodes, q.ref, q.best, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return box_key(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) { leaf_prims<false>(sc.tris, leaf, [&](const TriData& cur, int prim) { take(q, nearest_value<false>(cur, p).F, prim); }); });
}

} // namespace tyr
