// segment_value.hpp -- the value of a (segment, triangle) pair of the closest-segment queries (include/tyr_c.h "Closest-segment
// queries"), for the units that evaluate it: hip/segment.hip, and hip/sweep_capsule.hip for a capsule's initial overlap.
#pragma once

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

constexpr double kSegInfD = __builtin_inf();

// ---- the value of a (segment, triangle) pair: include/tyr_c.h "Closest-segment queries", operation by operation -------------

struct SegValue {
	double F; // +inf: the pair has no value (no finite input gives that)
	double s;
	uint32_t feature, region;
	d3 x, y; // on the segment, on the triangle
};

template <bool FULL>
__device__ __forceinline__ SegValue segment_value(const TriData& td, d3 P0, d3 P1) {
	// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
	const d3 A = mk3d((double)td.a.x, (double)td.a.y, (double)td.a.z);
	const d3 B = mk3d((double)(td.a.x + td.a.w), (double)(td.a.y + td.b.x), (double)(td.a.z + td.b.y));
	const d3 C = mk3d((double)(td.a.x + td.b.z), (double)(td.a.y + td.b.w), (double)(td.a.z + td.c.x));
	const d3 e1 = B - A, e2 = C - A;
	const d3 d = P1 - P0;
	SegValue o_;
	o_.F = kSegInfD, o_.s = 0.0, o_.feature = 0u, o_.region = 0u, o_.x = o_.y = mk3d(0.0, 0.0, 0.0);
	auto at = [&](double s) { return mk3d(P0.x + s * d.x, P0.y + s * d.y, P0.z + s * d.z); };
	auto offer = [&](bool ok, double F, double s, uint32_t feature, uint32_t region, d3 x, d3 y) {
		if (ok && F < o_.F) { // strict: of equal F the lower feature code stays
			o_.F = F;
			if (FULL)
				o_.s = s, o_.feature = feature, o_.region = region, o_.x = x, o_.y = y;
		}
	};
	const d3 ap0 = P0 - A;
	// feature 0: the segment crosses the triangle
	{
		const d3 n = crossd(e1, e2);
		const double nn = dotd(n, n);
		const double h0 = dotd(n, ap0), h1 = dotd(n, P1 - A);
		const double s = h0 / (h0 - h1);
		const d3 x = at(s);
		const d3 w = x - A;
		const double bv = dotd(crossd(w, e2), n), bw = dotd(crossd(e1, w), n);
		const bool sides = (h0 <= 0.0 && h1 >= 0.0) || (h0 >= 0.0 && h1 <= 0.0);
		offer(nn > 0.0 && h0 != h1 && sides && bv >= 0.0 && bw >= 0.0 && (bv + bw) <= nn, 0.0, s, 0u, 0u, x, x);
	}
	// features 1 and 2: an endpoint -- Ericson's closest-point test and clamp ("Closest-point queries") in binary64
	auto endpoint = [&](uint32_t feature, double s, d3 ap) {
		const d3 bp = ap - e1, cp = ap - e2;
		const double d1 = dotd(e1, ap), d2 = dotd(e2, ap);
		const double d3_ = dotd(e1, bp), d4 = dotd(e2, bp);
		const double d5 = dotd(e1, cp), d6 = dotd(e2, cp);
		const double vc = d1 * d4 - d3_ * d2, vb = d5 * d2 - d1 * d6, va = d3_ * d6 - d5 * d4;
		const double g = d4 - d3_, h = d5 - d6;
		const bool r1 = d1 <= 0 && d2 <= 0;
		const bool r2 = d3_ >= 0 && d4 <= d3_;
		const bool r3 = vc <= 0 && d1 >= 0 && d3_ <= 0;
		const bool r4 = d6 >= 0 && d5 <= d6;
		const bool r5 = vb <= 0 && d2 >= 0 && d6 <= 0;
		const bool r6 = va <= 0 && g >= 0 && h >= 0;
		const uint32_t rule = r1 ? 1u : r2 ? 2u : r3 ? 3u : r4 ? 4u : r5 ? 5u : r6 ? 6u : 7u;
		// the one division of the rule that holds, through selected operands (its result depends on them alone)
		const double num = rule == 3u ? d1 : rule == 5u ? d2 : rule == 6u ? g : 1.0;
		const double den = rule == 3u ? d1 - d3_ : rule == 5u ? d2 - d6 : rule == 6u ? g + h : (va + vb) + vc;
		const double x = num / den;
		const double u = rule == 2u ? 1.0 : rule == 3u ? x : rule == 6u ? 1.0 - x : rule == 7u ? vb * x : 0.0;
		const double v = rule == 4u ? 1.0 : (rule == 5u || rule == 6u) ? x : rule == 7u ? vc * x : 0.0;
		const double u1 = u > 0 ? u : 0.0, u2 = u1 < 1 ? u1 : 1.0;
		const double rem = 1.0 - u2;
		const double v1 = v > 0 ? v : 0.0, v2 = v1 < rem ? v1 : rem;
		const d3 q = mk3d((ap.x - e1.x * u2) - e2.x * v2, (ap.y - e1.y * u2) - e2.y * v2, (ap.z - e1.z * u2) - e2.z * v2);
		const double F = dotd(q, q);
		d3 px = mk3d(0.0, 0.0, 0.0), py = px;
		uint32_t region = 0u;
		if (FULL) {
			region = rule == 3u ? 4u : rule == 4u ? 3u : rule == 7u ? 0u : rule; // vertices 1 2 3, edges 4 5 6, the face 0
			px = at(s);
			py = mk3d((A.x + e1.x * u2) + e2.x * v2, (A.y + e1.y * u2) + e2.y * v2, (A.z + e1.z * u2) + e2.z * v2);
		}
		offer(true, F, s, feature, region, px, py);
	};
	endpoint(1u, 0.0, ap0);
	endpoint(2u, 1.0, P1 - A);
	// features 3, 4 and 5: an edge Q0 -> Q1 -- Ericson's closest points of two segments, exact tests against zero
	const double a = dotd(d, d);
	auto edge = [&](uint32_t feature, d3 Q0, d3 e, d3 r, uint32_t code, uint32_t code0, uint32_t code1) {
		const double ee = dotd(e, e), f = dotd(e, r), c = dotd(d, r), b = dotd(d, e);
		const double den = a * ee - b * b;
		double s, t;
		if (a == 0.0 && ee == 0.0) {
			s = 0.0, t = 0.0;
		} else if (a == 0.0) {
			s = 0.0, t = clamp01(f / ee);
		} else if (ee == 0.0) {
			t = 0.0, s = clamp01(-c / a);
		} else {
			s = den > 0.0 ? clamp01((b * f - c * ee) / den) : 0.0;
			const double tn = b * s + f;
			if (tn < 0.0)
				t = 0.0, s = clamp01(-c / a);
			else if (tn > ee)
				t = 1.0, s = clamp01((b - c) / a);
			else
				t = tn / ee;
		}
		const d3 x = at(s);
		const d3 y = mk3d(Q0.x + e.x * t, Q0.y + e.y * t, Q0.z + e.z * t);
		const d3 xy = x - y;
		offer(true, dotd(xy, xy), s, feature, (t > 0.0 && t < 1.0) ? code : (t >= 1.0 ? code1 : code0), x, y);
	};
	edge(3u, A, e1, ap0, 4u, 1u, 2u);
	edge(4u, A, e2, ap0, 5u, 1u, 3u);
	edge(5u, B, C - B, P0 - B, 6u, 2u, 3u);
	return o_;
}

} // namespace tyr
