// tri_distance.hip -- batched closest-triangle distance queries on the uploaded scene (tyr_query_tri_distance,
// host/tri_distance.cpp): for each of the caller's triangles (a, b, c) the triangle of the scene that comes nearest to it, the
// squared distance, and where on the two triangles it is attained (include/tyr_c.h "Closest-triangle queries": an argmin over
// all triangles with no traversal order in it, every operation binary64 in a fixed order, so that tests/tri_distance_ref.py
// reproduces each word by brute force).
//
// One query to a lane on a persistent grid, from the shared pieces (hip/query_common.hpp, hip/traverse.hpp): the chunked ticket
// feed, the first nStaged quad records in LDS, the LdsStack with its private spill arrays, triangle_load, the keyed descent
// (keyed_round: a quad step keys each of the four slots, orders them by key, descends into the nearest and pushes the others
// farthest first; an entry is tested against the bound again when it is popped).  This unit supplies the key and what is done
// with a leaf.
//
// A slot's key is a binary32 lower bound of the squared distance between the query triangle and the slot's box: the distance
// between the box and the query's own axis-aligned box (the query lies inside its box), reduced by
//     kTdSlack * M + kTdFloor,     M = sum over the axes of max(|qlo_k|, |qhi_k|) + max(|lo_k|, |hi_k|),   kTdSlack = 16 * 2^-24
// and squared.  The boxes bound exactly the corners the value is defined on and the value is binary64, so the reduction has to
// cover only the key's own binary32 roundings (at most 5 * 2^-24 * M by DESIGN.md "Closest-triangle queries"; kTdFloor, 2^-70,
// is for squares that underflow); the last squaring and best = (float)F round the same way, so they keep the order.  A slot is
// skipped only when key > best: a box at exactly the bound is still visited, since ties go to the lower index wherever it lies.
// In a leaf, a triangle with no lower index than the one held is also left out at key == best: it could only tie, and the
// tie is the held one's.
// fmaxf drops a NaN and takes 0 over -inf, so a synthetic record's box from -inf to +inf has no gap and is visited.
#include "tri_distance.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

constexpr float kTdUlp = 5.9604644775390625e-8f;    // 2^-24
constexpr float kTdSlack = 16.f * kTdUlp;            // of M, on the distance: 5 needed (3.2x)
constexpr float kTdFloor = 8.470329472543003e-22f;  // 2^-70: what squares that underflow can add to a distance, 8x
constexpr float kTdInf = __builtin_inff();
constexpr double kTdInfD = __builtin_inf();

// ---- the value of a (query, scene triangle) pair: include/tyr_c.h "Closest-triangle queries", operation by operation --------

struct TdValue {
	double F; // +inf: the pair has no value (no finite input gives that)
	uint32_t feature, region;
	d3 x, y; // on the query, on the scene triangle
};

__device__ __forceinline__ d3 along(d3 o, double s, d3 d) { return mk3d(o.x + s * d.x, o.y + s * d.y, o.z + s * d.z); }

// the segment block's feature 0 of the segment S0 + s d against the triangle (T0, t1, t2) with normal n, nn = dot(n, n);
// h0 = dot(n, S0 - T0), h1 = dot(n, S1 - T0) are the caller's.  True: x is the crossing.
__device__ __forceinline__ bool td_crossing(d3 n, double nn, d3 T0, d3 t1, d3 t2, double h0, double h1, d3 S0, d3 d, d3& x) {
	const double s = h0 / (h0 - h1);
	x = along(S0, s, d);
	const d3 w = x - T0;
	const double bv = dotd(crossd(w, t2), n), bw = dotd(crossd(t1, w), n);
	const bool sides = (h0 <= 0.0 && h1 >= 0.0) || (h0 >= 0.0 && h1 <= 0.0);
	return nn > 0.0 && h0 != h1 && sides && bv >= 0.0 && bw >= 0.0 && (bv + bw) <= nn;
}

// Ericson's closest-point test and clamp ("Closest-point queries") in binary64 for the point T0 + ap against the triangle
// (T0, t1, t2): F, and with FULL the region and the clamped point c
template <bool FULL>
__device__ __forceinline__ double td_closest(d3 ap, d3 t1, d3 t2, d3 T0, uint32_t& region, d3& c) {
	const d3 bp = ap - t1, cp = ap - t2;
	const double d1 = dotd(t1, ap), d2 = dotd(t2, ap);
	const double d3_ = dotd(t1, bp), d4 = dotd(t2, bp);
	const double d5 = dotd(t1, cp), d6 = dotd(t2, cp);
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
	const d3 q = mk3d((ap.x - t1.x * u2) - t2.x * v2, (ap.y - t1.y * u2) - t2.y * v2, (ap.z - t1.z * u2) - t2.z * v2);
	if (FULL) {
		region = rule == 3u ? 4u : rule == 4u ? 3u : rule == 7u ? 0u : rule; // vertices 1 2 3, edges 4 5 6, the face 0
		c = mk3d((T0.x + t1.x * u2) + t2.x * v2, (T0.y + t1.y * u2) + t2.y * v2, (T0.z + t1.z * u2) + t2.z * v2);
	}
	return dotd(q, q);
}

// Ericson's closest points of the segments S0 + s d (a = dot(d, d)) and Q0 + t e, r = S0 - Q0, exact tests against zero
__device__ __forceinline__ double td_edges(d3 S0, d3 d, double a, d3 Q0, d3 e, d3 r, double& t, d3& x, d3& y) {
	const double ee = dotd(e, e), f = dotd(e, r), c = dotd(d, r), b = dotd(d, e);
	const double den = a * ee - b * b;
	double s;
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
	x = along(S0, s, d);
	y = mk3d(Q0.x + e.x * t, Q0.y + e.y * t, Q0.z + e.z * t);
	const d3 xy = x - y;
	return dotd(xy, xy);
}

__device__ __forceinline__ d3 widen(f3 v) { return mk3d((double)v.x, (double)v.y, (double)v.z); }

// The 21 candidates.  The contract offers them in the order of their codes with a strict <, which is the least pair (F, code);
// here they are evaluated in another order -- the scene's corners and edges against the query first, then one trip per query
// corner P_i for the codes i, 6 + i and 12 + 3 i + j, the corners rotating through the same registers -- and offered by that
// pair, so that only the operands of one trip are live at a time (DESIGN.md "Closest-triangle queries": evaluated in code order
// with every shared operand held, the leaf does not fit the register file).  Every operation has the contract's operands.
template <bool FULL>
__device__ __forceinline__ TdValue tri_distance_value(const TriData& td, f3 p0, f3 p1, f3 p2) {
	// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
	const d3 A = mk3d((double)td.a.x, (double)td.a.y, (double)td.a.z);
	const d3 B = mk3d((double)(td.a.x + td.a.w), (double)(td.a.y + td.b.x), (double)(td.a.z + td.b.y));
	const d3 C = mk3d((double)(td.a.x + td.b.z), (double)(td.a.y + td.b.w), (double)(td.a.z + td.c.x));
	const d3 e1 = B - A, e2 = C - A, e3 = C - B; // the scene triangle's edges G0, G1, G2
	TdValue o_;
	o_.F = kTdInfD, o_.feature = 0u, o_.region = 0u, o_.x = o_.y = mk3d(0.0, 0.0, 0.0);
	auto offer = [&](bool ok, double F, uint32_t feature, uint32_t region, d3 x, d3 y) {
		if (FULL) {
			if (ok && (F < o_.F || (F == o_.F && feature < o_.feature))) // of equal F the lower code stays (+inf is never offered below code 0)
				o_.F = F, o_.feature = feature, o_.region = region, o_.x = x, o_.y = y;
		} else if (ok && F < o_.F) {
			o_.F = F;
		}
	};
	d3 x, y;
	uint32_t region = 0u;
	{
		const d3 P0 = widen(p0);
		const d3 u1 = widen(p1) - P0, u2 = widen(p2) - P0; // the query as a triangle (P0, u1, u2)
		const d3 vp0 = A - P0, vp1 = B - P0, vp2 = C - P0; // scene corners relative to P0
		const d3 m = crossd(u1, u2);
		const double mm = dotd(m, m);
		const double k0 = dotd(m, vp0), k1 = dotd(m, vp1), k2 = dotd(m, vp2);
		// codes 3-5: a scene edge crosses the query triangle
		offer(td_crossing(m, mm, P0, u1, u2, k0, k1, A, e1, x), 0.0, 3u, 4u, x, x);
		offer(td_crossing(m, mm, P0, u1, u2, k0, k2, A, e2, x), 0.0, 4u, 5u, x, x);
		offer(td_crossing(m, mm, P0, u1, u2, k1, k2, B, e3, x), 0.0, 5u, 6u, x, x);
		// codes 9-11: a scene corner against the query triangle
		double F = td_closest<FULL>(vp0, u1, u2, P0, region, x);
		offer(true, F, 9u, 1u, x, A);
		F = td_closest<FULL>(vp1, u1, u2, P0, region, x);
		offer(true, F, 10u, 2u, x, B);
		F = td_closest<FULL>(vp2, u1, u2, P0, region, x);
		offer(true, F, 11u, 3u, x, C);
	}
	const d3 n = crossd(e1, e2);
	const double nn = dotd(n, n);
	f3 cur = p0, nxt = p1, oth = p2;
#pragma unroll 1
	for (uint32_t i = 0u; i < 3u; ++i) {
		if (!FULL && o_.F == 0.0) // nothing is less than 0 (F is a sum of squares), and the walk needs F alone
			break;
		const d3 S0 = widen(cur), S1 = widen(nxt);
		const d3 d = S1 - S0;      // the query's edge E_i as a segment: P1 - P0, P2 - P1, P0 - P2
		const d3 ra = S0 - A;      // ap_i
		// code i: the query edge crosses the scene triangle
		offer(td_crossing(n, nn, A, e1, e2, dotd(n, ra), dotd(n, S1 - A), S0, d, x), 0.0, i, 0u, x, x);
		// code 6 + i: the query corner against the scene triangle
		double F = td_closest<FULL>(ra, e1, e2, A, region, y);
		offer(true, F, 6u + i, region, S0, y);
		// codes 12 + 3 i + j: the edge pairs
		const double a = dotd(d, d);
		double t;
		F = td_edges(S0, d, a, A, e1, ra, t, x, y);
		offer(true, F, 12u + 3u * i, (t > 0.0 && t < 1.0) ? 4u : (t >= 1.0 ? 2u : 1u), x, y);
		F = td_edges(S0, d, a, A, e2, ra, t, x, y);
		offer(true, F, 13u + 3u * i, (t > 0.0 && t < 1.0) ? 5u : (t >= 1.0 ? 3u : 1u), x, y);
		F = td_edges(S0, d, a, B, e3, S0 - B, t, x, y);
		offer(true, F, 14u + 3u * i, (t > 0.0 && t < 1.0) ? 6u : (t >= 1.0 ? 3u : 2u), x, y);
		const f3 was = cur;
		cur = nxt, nxt = oth, oth = was;
	}
	return o_;
}

// ---- the pruning key --------------------------------------------------------------------------------------------------------

// the query a lane has in flight and what it has found so far
struct TdLane {
	float ax, ay, az, bx, by, bz, cx, cy, cz;
	float lox, hix, loy, hiy, loz, hiz; // the query's own box
	float ms;                           // sum over the axes of max(|qlo_k|, |qhi_k|)
	float best;                         // the smallest F32 so far; bound2 until a triangle is accepted
	int prim;                           // its triangle, -1: none
	uint32_t ref;                       // the lane's state
};

__device__ __forceinline__ void td_lane_setup(TdLane& q) {
	q.lox = __builtin_fminf(__builtin_fminf(q.ax, q.bx), q.cx), q.hix = __builtin_fmaxf(__builtin_fmaxf(q.ax, q.bx), q.cx);
	q.loy = __builtin_fminf(__builtin_fminf(q.ay, q.by), q.cy), q.hiy = __builtin_fmaxf(__builtin_fmaxf(q.ay, q.by), q.cy);
	q.loz = __builtin_fminf(__builtin_fminf(q.az, q.bz), q.cz), q.hiz = __builtin_fmaxf(__builtin_fmaxf(q.az, q.bz), q.cz);
	q.ms = (__builtin_fmaxf(fabsf(q.lox), fabsf(q.hix)) + __builtin_fmaxf(fabsf(q.loy), fabsf(q.hiy))) + __builtin_fmaxf(fabsf(q.loz), fabsf(q.hiz));
}

// A box against a lane's query: the pruning key (see the head of this file); +inf for a box that is skipped.
__device__ __forceinline__ float tri_distance_key(const TdLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	// box against the query's box (fmaxf drops a NaN and takes 0 over -inf: a synthetic record's box has no gap)
	const float gx = __builtin_fmaxf(0.f, __builtin_fmaxf(lox - q.hix, q.lox - hix));
	const float gy = __builtin_fmaxf(0.f, __builtin_fmaxf(loy - q.hiy, q.loy - hiy));
	const float gz = __builtin_fmaxf(0.f, __builtin_fmaxf(loz - q.hiz, q.loz - hiz));
	const float D = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
	const float M = q.ms + ((__builtin_fmaxf(fabsf(lox), fabsf(hix)) + __builtin_fmaxf(fabsf(loy), fabsf(hiy))) + __builtin_fmaxf(fabsf(loz), fabsf(hiz)));
	const float l0 = D - (kTdSlack * M + kTdFloor);
	const float lb = l0 > 0.f ? l0 : 0.f; // (inf - inf: 0)
	const float key = lb * lb;
	// (an unused slot's box is at +infinity)
	return (lox < kTdInf && !(key > q.best)) ? key : kTdInf;
}

// a triangle of a reached leaf: the smallest pair (F32, index) so far stays; F32 at the bound is no winner
__device__ __forceinline__ void td_take(TdLane& q, double F, int prim) {
	const float F32 = (float)F;
	if (F32 < q.best || (F32 == q.best && prim < q.prim)) {
		q.best = F32;
		q.prim = prim;
	}
}

__device__ __forceinline__ bool td_same(float px, float py, float pz, f3 v) { return px == v.x && py == v.y && pz == v.z; }

// One round of the wave's traversal: the keyed descent (keyed_round, hip/query_common.hpp) on tri_distance_key against the
// lane's `best`, then one leaf per lane that is at one, primitives in array order.
template <class CanRefill>
__device__ __forceinline__ void d_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, TdLane& q, bool skipShared, CanRefill canRefill) {
	q.ref = keyed_round(
		sc, st, stagedNodes, q.ref, q.best, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return tri_distance_key(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			const f3 P0 = mk3(q.ax, q.ay, q.az), P1 = mk3(q.bx, q.by, q.bz), P2 = mk3(q.cx, q.cy, q.cz);
			leaf_prims<false>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				// the triangle's own three-corner box against the bound, as a slot's, and rule 0 of "Triangle-overlap queries"
				// (==: -0 equals +0): the binary64 evaluation only behind them
				const CornerBox t = tri_corner_box(cur);
				// (a triangle that does not come before the one held wins only with F32 < best, strictly, and F32 is never below
				// its key: with key >= best it is left out -- after a contact, best = 0, every later triangle of a higher index)
				const float key = tri_distance_key(q, t.lox, t.hix, t.loy, t.hiy, t.loz, t.hiz);
				bool take = key < kTdInf && (key < q.best || prim < q.prim);
				if (take && skipShared) {
					const bool s0 = td_same(q.ax, q.ay, q.az, t.a) || td_same(q.ax, q.ay, q.az, t.b) || td_same(q.ax, q.ay, q.az, t.c);
					const bool s1 = td_same(q.bx, q.by, q.bz, t.a) || td_same(q.bx, q.by, q.bz, t.b) || td_same(q.bx, q.by, q.bz, t.c);
					const bool s2 = td_same(q.cx, q.cy, q.cz, t.a) || td_same(q.cx, q.cy, q.cz, t.b) || td_same(q.cx, q.cy, q.cz, t.c);
					take = !(s0 || s1 || s2);
				}
				if (take)
					td_take(q, tri_distance_value<false>(cur, P0, P1, P2).F, prim);
			});
		});
}

} // namespace

// Two blocks per CU: the 21-candidate binary64 leaf holds more than the 168 registers three waves per SIMD would leave it
// (DESIGN.md "Closest-triangle queries").
__global__ void __launch_bounds__(kBlock, 2) k_query_tri_distance(const TriDistanceParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();
	const bool skipShared = P0.skipShared != 0u;

	TdLane q = {};
	q.ref = kRefDone;
	q.prim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// a finished query's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const TriDistanceParams& P = kernarg_view<TriDistanceParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = item;
		// none or invalid: the bound (+inf for an invalid query) and a as given
		float dist2 = q.best;
		uint32_t feature = 0u, region = 0u;
		float xx = q.ax, xy = q.ay, xz = q.az, yx = q.ax, yy = q.ay, yz = q.az;
		if (q.prim >= 0) {
			const TdValue w = tri_distance_value<true>(triangle_load(sc.tris, (uint32_t)q.prim), mk3(q.ax, q.ay, q.az), mk3(q.bx, q.by, q.bz), mk3(q.cx, q.cy, q.cz)); // the winner's operations once more: the same value
			dist2 = (float)w.F;
			feature = w.feature, region = w.region;
			xx = (float)w.x.x, xy = (float)w.x.y, xz = (float)w.x.z;
			yx = (float)w.y.x, yy = (float)w.y.y, yz = (float)w.y.z;
		}
		P.dist2[i] = dist2;
		P.prim[i] = q.prim;
		if (P.feature)
			P.feature[i] = (uint8_t)feature;
		if (P.region)
			P.region[i] = (uint8_t)region;
		if (P.onQuery)
			P.onQuery[3 * i + 0] = xx, P.onQuery[3 * i + 1] = xy, P.onQuery[3 * i + 2] = xz;
		if (P.onTriangle)
			P.onTriangle[3 * i + 0] = yx, P.onTriangle[3 * i + 1] = yy, P.onTriangle[3 * i + 2] = yz;
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<TriDistanceParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const TriDistanceParams& P = kernarg_view<TriDistanceParams>();
			const size_t i3 = 3 * (size_t)item;
			q.ax = P.a[i3 + 0], q.ay = P.a[i3 + 1], q.az = P.a[i3 + 2];
			q.bx = P.b[i3 + 0], q.by = P.b[i3 + 1], q.bz = P.b[i3 + 2];
			q.cx = P.c[i3 + 0], q.cy = P.c[i3 + 1], q.cz = P.c[i3 + 2];
			const float md = P.maxDist ? P.maxDist[item] : kTdInf;
			// a NaN or infinite component of a corner, or a NaN or negative max_dist: not a query (dist2 = +inf)
			const bool valid = finite3(q.ax, q.ay, q.az) && finite3(q.bx, q.by, q.bz) && finite3(q.cx, q.cy, q.cz) && md >= 0;
			q.best = valid ? md * md : kTdInf;
			q.prim = -1;
			td_lane_setup(q);
			st.reset();
			live = true;
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
		d_traverse(sc, st, stagedNodes, q, skipShared, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<TriDistanceParams>().error);
}

void launch_tri_distance(const TriDistanceParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_tri_distance, P, P.n, numCUs, lc.perCU[kLcTriDistance][0], stream);
}

} // namespace tyr
