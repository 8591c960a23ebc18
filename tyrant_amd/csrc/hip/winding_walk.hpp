// winding_walk.hpp -- the stackless walk of the moment tree that sums a point's winding series (include/tyr_c.h "Winding
// numbers"), with the pieces it is made of: a triangle record widened, a triangle's solid angle, a node's record read.  Device
// code of hip/winding.hip (k_winding, and load_tri in the tree's build) and hip/signed.hip (the signed-distance kernels, which
// walk for a lane once its closest-point descent is done): one text, so both sum the same words in the same order.
#pragma once

#include "detmath.hpp"
#include "vecmath64.hpp"
#include "winding.hpp"

namespace tyr {

// a triangle record of the ctx (bvh_layout.cpp "triangles"), widened
__device__ __forceinline__ void load_tri(const float4* __restrict__ tris, uint32_t t, d3& v, d3& e1, d3& e2) {
	const float4 q0 = tris[3 * (size_t)t + 0], q1 = tris[3 * (size_t)t + 1], q2 = tris[3 * (size_t)t + 2];
	v = mk3d((double)q0.x, (double)q0.y, (double)q0.z);
	e1 = mk3d((double)q0.w, (double)q1.x, (double)q1.y);
	e2 = mk3d((double)q1.z, (double)q1.w, (double)q2.x);
}

// the signed solid angle of triangle (v, e1, e2) at q (Van Oosterom and Strackee)
__device__ __forceinline__ double omega(d3 q, d3 v, d3 e1, d3 e2) {
	const d3 a = v - q, b = (v + e1) - q, c = (v + e2) - q;
	const double la = __builtin_sqrt(dotd(a, a)), lb = __builtin_sqrt(dotd(b, b)), lc = __builtin_sqrt(dotd(c, c));
	const double det = dotd(a, crossd(b, c));
	const double den = ((la * lb) * lc + dotd(a, b) * lc) + (dotd(b, c) * la + dotd(c, a) * lb);
	return 2.0 * dm::atan2_det(det, den);
}

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// The series of q over the first nNodes records, B2 = accuracy^2: no stack -- a node is either summed as a dipole or as its
// triangles and left through its skip index, or entered at the next index.  With the sum, the terms that were added.
struct WindingSum {
	double sum;
	uint32_t dipoles, triangles;
};
__device__ __forceinline__ WindingSum winding_sum(const WindingNode* nodes, const float4* tris, uint32_t nNodes, const d3& q, double B2) {
	uint32_t dipoles = 0, triangles = 0; // (in front of the sum, as k_winding had them: the other order swaps two register pairs in winding.s)
	double sum = 0.0;
	for (uint32_t i = 0; i < nNodes;) {
		const double2* rec = reinterpret_cast<const double2*>(nodes + i);
		const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
		const unsigned long long ab = (unsigned long long)__double_as_longlong(r3.y);
		const uint32_t a = (uint32_t)ab, b = (uint32_t)(ab >> 32);
		const d3 d = mk3d(r0.x, r0.y, r1.x) - q;
		const double d2 = dotd(d, d);
		uint32_t next = b > 0u ? i + 1u : a;
		if (d2 > B2 * r3.x) {
			sum += dotd(d, mk3d(r1.y, r2.x, r2.y)) / (d2 * __builtin_sqrt(d2));
			++dipoles;
		} else if (b > 0u) {
			for (uint32_t t = a; t < a + b; ++t) {
				d3 v, e1, e2;
				load_tri(tris, t, v, e1, e2);
				sum += omega(q, v, e1, e2);
			}
			triangles += b;
		} else {
			next = i + 1u;
		}
		i = next > i ? next : nNodes; // (indices only ever grow: the walk ends whatever the records hold)
	}
	return WindingSum{ sum, dipoles, triangles };
}

} // namespace tyr
