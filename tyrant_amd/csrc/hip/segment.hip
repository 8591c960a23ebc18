// segment.hip -- batched closest-segment queries on the uploaded scene (tyr_query_segment, host/segment.cpp): for each of the
// caller's segments p -> q the triangle of the scene that comes nearest to it, the squared distance, and where on the segment
// and on the triangle it is attained (include/tyr_c.h "Closest-segment queries": an argmin over all triangles with no traversal
// order in it, every operation binary64 in a fixed order, so that tests/segment_ref.py reproduces each word by brute force).
//
// One segment to a lane on a persistent grid, with the point queries' pieces (hip/query_common.hpp, hip/traverse.hpp): the
// chunked ticket feed, the first nStaged quad records in LDS, the LdsStack with its private spill arrays, triangle_load, the
// flat lane states (interior ref | leaf ref | kRefPop | kRefDone).  The descent is the keyed one of the point queries and the
// sweeps (keyed_round, hip/query_common.hpp): a quad step keys each of the four slots, orders them by key, descends into the
// nearest and pushes the others farthest first; an entry is tested against the bound again when it is popped.  This unit
// supplies the key and what is done with a leaf.
//
// A slot's key is a binary32 lower bound of the squared distance between the segment and the slot's box, the larger of
//   (a) the distance between the box and the segment's own axis-aligned box (the segment lies inside its box), and
//   (b) the distance of the box's centre to the segment minus the box's half diagonal (the triangle inequality: every point
//       of the box is within the half diagonal of the centre) -- what prunes for a long diagonal segment, whose own box is
//       most of the scene,
// taken as a distance, reduced by
//     kSegSlack * M + kSegFloor,     M = sum over the axes of max(|p_k|, |q_k|) + max(|lo_k|, |hi_k|),   kSegSlack = 64 * 2^-24
// and squared.  The boxes bound exactly the corners the value is defined on and the value is binary64, so the reduction has
// to cover only the key's own binary32 roundings (at most 22 * 2^-24 * M by DESIGN.md "Closest-segment queries"; kSegFloor,
// 2^-70, is for products that underflow); the last squaring and best = (float)F round the same way, so they keep the order.
// A slot is skipped only when key > best: a box at exactly the bound is still visited, since ties go to the lower index
// wherever it lies.  (b) needs a point of the segment near the centre; with magnitudes at which its parameter could overflow or
// underflow (M >= 2^60, |d|^2 < 2^-100) it is left out.  A NaN (the centre of a synthetic record's box from -inf to +inf) fails
// every comparison that would raise the key.
#include "segment.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

constexpr float kSegUlp = 5.9604644775390625e-8f;   // 2^-24
constexpr float kSegSlack = 64.f * kSegUlp;          // of M, on the distance: 22 needed (2.9x)
constexpr float kSegFloor = 8.470329472543003e-22f;  // 2^-70: what products that underflow can add to a distance, 8x
constexpr float kSegBig = 1.152921504606847e18f;     // 2^60: above it bound (b)'s products could overflow
constexpr float kSegTiny = 7.888609052210118e-31f;   // 2^-100: below it |d|^2 has lost precision to underflow
constexpr float kSegInf = __builtin_inff();
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

// ---- the pruning key --------------------------------------------------------------------------------------------------------

// the segment a lane has in flight and what it has found so far
struct SegLane {
	float px, py, pz, qx, qy, qz;
	float dx, dy, dz; // q - p
	float rdd;        // 1 / |d|^2 for bound (b); NaN: (b) is left out
	float ms;         // sum over the axes of max(|p_k|, |q_k|)
	float best;       // the smallest F32 so far; bound2 until a triangle is accepted
	int prim;         // its triangle, -1: none
	uint32_t ref;     // the lane's state
};

__device__ __forceinline__ void segment_lane_setup(SegLane& q) {
	q.dx = q.qx - q.px, q.dy = q.qy - q.py, q.dz = q.qz - q.pz;
	const float dd = (q.dx * q.dx + q.dy * q.dy) + q.dz * q.dz;
	q.ms = (__builtin_fmaxf(fabsf(q.px), fabsf(q.qx)) + __builtin_fmaxf(fabsf(q.py), fabsf(q.qy))) + __builtin_fmaxf(fabsf(q.pz), fabsf(q.qz));
	q.rdd = (dd >= kSegTiny && q.ms < kSegBig) ? 1.f / dd : __uint_as_float(0x7fc00000u);
}

// A box against a lane's segment: the pruning key (see the head of this file); +inf for a box that is skipped.
__device__ __forceinline__ float segment_key(const SegLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	// (a) box against the segment's box (fmaxf drops a NaN and takes 0 over -inf: a synthetic record's box has no gap)
	const float gx = __builtin_fmaxf(0.f, __builtin_fmaxf(lox - __builtin_fmaxf(q.px, q.qx), __builtin_fminf(q.px, q.qx) - hix));
	const float gy = __builtin_fmaxf(0.f, __builtin_fmaxf(loy - __builtin_fmaxf(q.py, q.qy), __builtin_fminf(q.py, q.qy) - hiy));
	const float gz = __builtin_fmaxf(0.f, __builtin_fmaxf(loz - __builtin_fmaxf(q.pz, q.qz), __builtin_fminf(q.pz, q.qz) - hiz));
	const float da = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
	// (b) the centre against the segment, less the half diagonal
	const float cx = 0.5f * (lox + hix), cy = 0.5f * (loy + hiy), cz = 0.5f * (loz + hiz);
	const float hx = 0.5f * (hix - lox), hy = 0.5f * (hiy - loy), hz = 0.5f * (hiz - loz);
	const float hd = __builtin_sqrtf((hx * hx + hy * hy) + hz * hz);
	const float mx = cx - q.px, my = cy - q.py, mz = cz - q.pz;
	const float t0 = ((mx * q.dx + my * q.dy) + mz * q.dz) * q.rdd;
	const float t1 = t0 > 0.f ? t0 : 0.f, t = t1 < 1.f ? t1 : 1.f;
	const float wx = mx - t * q.dx, wy = my - t * q.dy, wz = mz - t * q.dz;
	const float db = __builtin_sqrtf((wx * wx + wy * wy) + wz * wz) - hd;
	const float M = q.ms + ((__builtin_fmaxf(fabsf(lox), fabsf(hix)) + __builtin_fmaxf(fabsf(loy), fabsf(hiy))) + __builtin_fmaxf(fabsf(loz), fabsf(hiz)));
	const float D = (q.rdd == q.rdd && M < kSegBig && db > da) ? db : da; // (a NaN in db: false)
	const float l0 = D - (kSegSlack * M + kSegFloor);
	const float lb = l0 > 0.f ? l0 : 0.f; // (inf - inf: 0)
	const float key = lb * lb;
	// (an unused slot's box is at +infinity)
	return (lox < kSegInf && !(key > q.best)) ? key : kSegInf;
}

// a triangle of a reached leaf: the smallest pair (F32, index) so far stays; F32 at the bound is no winner
__device__ __forceinline__ void segment_take(SegLane& q, double F, int prim) {
	const float F32 = (float)F;
	if (F32 < q.best || (F32 == q.best && prim < q.prim)) {
		q.best = F32;
		q.prim = prim;
	}
}

// One round of the wave's traversal: the keyed descent (keyed_round, hip/query_common.hpp) on segment_key against the lane's
// `best`, then one leaf per lane that is at one, primitives in array order.
template <class CanRefill>
__device__ __forceinline__ void g_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, SegLane& q, CanRefill canRefill) {
	q.ref = keyed_round(
		sc, st, stagedNodes, q.ref, q.best, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return segment_key(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			const d3 P0 = mk3d((double)q.px, (double)q.py, (double)q.pz), P1 = mk3d((double)q.qx, (double)q.qy, (double)q.qz);
			leaf_prims<false>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				// the triangle's own three-corner box against the bound, as a slot's: the binary64 evaluation only behind it
				const CornerBox b = tri_corner_box(cur);
				if (segment_key(q, b.lox, b.hix, b.loy, b.hiy, b.loz, b.hiz) < kSegInf)
					segment_take(q, segment_value<false>(cur, P0, P1).F, prim);
			});
		});
}

} // namespace

__global__ void __launch_bounds__(kBlock, 3) k_query_segment(const SegmentParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	SegLane q = {};
	q.ref = kRefDone;
	q.prim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false;

	// a finished segment's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const SegmentParams& P = kernarg_view<SegmentParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = item;
		// none or invalid: the bound (+inf for an invalid segment) and p as given
		float dist2 = q.best, s = 0.f;
		uint32_t feature = 0u, region = 0u;
		float xx = q.px, xy = q.py, xz = q.pz, yx = q.px, yy = q.py, yz = q.pz;
		if (q.prim >= 0) {
			const d3 A0 = mk3d((double)q.px, (double)q.py, (double)q.pz), A1 = mk3d((double)q.qx, (double)q.qy, (double)q.qz);
			const SegValue w = segment_value<true>(triangle_load(sc.tris, (uint32_t)q.prim), A0, A1); // the winner's operations once more: the same value
			dist2 = (float)w.F, s = (float)w.s;
			feature = w.feature, region = w.region;
			xx = (float)w.x.x, xy = (float)w.x.y, xz = (float)w.x.z;
			yx = (float)w.y.x, yy = (float)w.y.y, yz = (float)w.y.z;
		}
		P.dist2[i] = dist2;
		P.prim[i] = q.prim;
		if (P.s)
			P.s[i] = s;
		if (P.feature)
			P.feature[i] = (uint8_t)feature;
		if (P.region)
			P.region[i] = (uint8_t)region;
		if (P.onSegment)
			P.onSegment[3 * i + 0] = xx, P.onSegment[3 * i + 1] = xy, P.onSegment[3 * i + 2] = xz;
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
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<SegmentParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const SegmentParams& P = kernarg_view<SegmentParams>();
			const size_t i3 = 3 * (size_t)item;
			q.px = P.p[i3 + 0], q.py = P.p[i3 + 1], q.pz = P.p[i3 + 2];
			q.qx = P.q[i3 + 0], q.qy = P.q[i3 + 1], q.qz = P.q[i3 + 2];
			const float md = P.maxDist ? P.maxDist[item] : kSegInf;
			// a NaN or infinite component of p or q, or a NaN or negative max_dist: not a query (dist2 = +inf)
			const bool valid = finite3(q.px, q.py, q.pz) && finite3(q.qx, q.qy, q.qz) && md >= 0;
			q.best = valid ? md * md : kSegInf;
			q.prim = -1;
			segment_lane_setup(q);
			st.reset();
			live = true;
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly segments that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished segments, while segments remain
		g_traverse(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<SegmentParams>().error);
}

void launch_segment(const SegmentParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_segment, P, P.n, numCUs, lc.perCU[kLcSegment][0], stream);
}

} // namespace tyr
