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
#include "segment_value.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

constexpr float kSegUlp = 5.9604644775390625e-8f;   // 2^-24
constexpr float kSegSlack = 64.f * kSegUlp;          // of M, on the distance: 22 needed (2.9x)
constexpr float kSegFloor = 8.470329472543003e-22f;  // 2^-70: what products that underflow can add to a distance, 8x
constexpr float kSegBig = 1.152921504606847e18f;     // 2^60: above it bound (b)'s products could overflow
constexpr float kSegTiny = 7.888609052210118e-31f;   // 2^-100: below it |d|^2 has lost precision to underflow
constexpr float kSegInf = __builtin_inff();


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
