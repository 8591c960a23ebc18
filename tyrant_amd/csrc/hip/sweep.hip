// sweep.hip -- batched swept-sphere queries on the uploaded scene (tyr_query_sweep, host/sweep.cpp): for each of the caller's
// sweeps -- a sphere of radius r whose centre moves from o along d -- the first parameter t at which it touches a triangle of
// the scene, which triangle, and where (include/tyr_c.h "Swept-sphere queries": an argmin over all triangles with no traversal
// order in it, every operation binary64 in a fixed order, so that tests/sweep_ref.py reproduces each word by brute force).
//
// One sweep to a lane on a persistent grid, with the point queries' pieces (hip/query_common.hpp, hip/traverse.hpp): the chunked
// ticket feed, the first nStaged quad records in LDS, the LdsStack with its private spill arrays, triangle_load, the flat lane
// states (interior ref | leaf ref | kRefPop | kRefDone).  The descent is the keyed one the point queries use (keyed_round,
// hip/query_common.hpp): a quad step keys each of the four slots, orders them by key, descends into the nearest and pushes
// the others farthest first; an entry is tested against the bound again when it is popped.  This unit supplies the key and
// what is done with a leaf.
//
// A slot's key is the parameter at which the segment enters the slot's box inflated by r on every axis, from a binary32 slab
// test.  At a contact the centre is within r of a point of the box, so it is inside the inflated box: the entry parameter is
// a lower bound of the value of every triangle in the box.  Pruning never changes the answer (DESIGN.md "Swept-sphere queries"
// derives the constant): every plane of the inflated box is first moved outward by
//     kSweepSlack * (|o_k| + max(|lo_k - r|, |hi_k + r|)),      kSweepSlack = 16 * 2^-24
// which is more than the slab test's roundings, the rounding of the inflated plane itself and the rounding of a value to
// binary32 can add up to (6 * 2^-24 of the same form).  A slot is skipped only when the segment misses that box, leaves it
// before 0, or enters it after `best` -- `>`: a box at exactly the bound is still visited, since ties go to the lower index
// wherever it lies.  A NaN in the slab test (0 * inf: a segment parallel to a plane it starts on) counts as "visit".
#include "sweep.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

constexpr float kSweepUlp = 5.9604644775390625e-8f; // 2^-24
constexpr float kSweepSlack = 16.f * kSweepUlp;     // of |o_k| + max(|lo_k - r|, |hi_k + r|), per plane: 6 needed (2.6x)
constexpr float kSweepInf = __builtin_inff();
constexpr double kSweepInfD = __builtin_inf();

// ---- the value of a (sweep, triangle) pair: include/tyr_c.h "Swept-sphere queries", operation by operation -------------------

struct SweepValue {
	double t; // +inf: the pair has no value
	uint32_t region;
	d3 c; // the contact
};

template <bool FULL>
__device__ __forceinline__ SweepValue sweep_value(const TriData& td, d3 o, d3 d, double r, double tmax) {
	// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
	const d3 A = mk3d((double)td.a.x, (double)td.a.y, (double)td.a.z);
	const d3 B = mk3d((double)(td.a.x + td.a.w), (double)(td.a.y + td.b.x), (double)(td.a.z + td.b.y));
	const d3 C = mk3d((double)(td.a.x + td.b.z), (double)(td.a.y + td.b.w), (double)(td.a.z + td.c.x));
	const d3 e1 = B - A, e2 = C - A;
	const d3 ap = o - A;
	const double rr = r * r;
	const double dd = dotd(d, d);
	SweepValue o_;
	o_.t = kSweepInfD, o_.region = 0u, o_.c = mk3d(0.0, 0.0, 0.0);
	auto offer = [&](bool ok, double t, uint32_t code, d3 pt) {
		if (ok && t >= 0.0 && t <= tmax && t < o_.t) { // strict: of equal t the lower region code stays
			o_.t = t;
			if (FULL)
				o_.region = code, o_.c = pt;
		}
	};
	// the face
	{
		const d3 n = crossd(e1, e2);
		const double nn = dotd(n, n);
		const double ln = __builtin_sqrt(nn);
		const double h = dotd(n, ap);
		const double s = h >= 0.0 ? 1.0 : -1.0;
		const double sdn = s * dotd(n, d);
		const double ah = __builtin_fabs(h);
		const double rl = r * ln;
		const double t = (ah - rl) / (-sdn);
		const double k = (s * r) / ln;
		const d3 q = mk3d((o.x + t * d.x) - n.x * k, (o.y + t * d.y) - n.y * k, (o.z + t * d.z) - n.z * k);
		const d3 w = q - A;
		const double bv = dotd(crossd(w, e2), n), bw = dotd(crossd(e1, w), n);
		offer(nn > 0.0 && sdn < 0.0 && ah > rl && bv >= 0.0 && bw >= 0.0 && (bv + bw) <= nn, t, 0u, q);
	}
	// the vertices
	const d3 bm = o - B, cm = o - C;
	auto vertex = [&](uint32_t code, d3 P, d3 m) {
		const double b = dotd(m, d);
		const double c = dotd(m, m) - rr;
		const double disc = b * b - dd * c;
		const double t = (-b - __builtin_sqrt(disc)) / dd;
		offer(dd > 0.0 && b < 0.0 && c > 0.0 && disc >= 0.0, t, code, P);
	};
	vertex(1u, A, ap);
	vertex(2u, B, bm);
	vertex(3u, C, cm);
	// the edges
	auto edge = [&](uint32_t code, d3 P0, d3 e, d3 m) {
		const double ee = dotd(e, e), de = dotd(d, e), me = dotd(m, e);
		const double md = dotd(m, d), mm = dotd(m, m);
		const double a = ee * dd - de * de;
		const double b = ee * md - de * me;
		const double c = ee * (mm - rr) - me * me;
		const double disc = b * b - a * c;
		const double t = (-b - __builtin_sqrt(disc)) / a;
		const double sg = (me + t * de) / ee;
		offer(ee > 0.0 && a > 0.0 && b < 0.0 && c > 0.0 && disc >= 0.0 && sg >= 0.0 && sg <= 1.0, t, code, mk3d(P0.x + e.x * sg, P0.y + e.y * sg, P0.z + e.z * sg));
	};
	edge(4u, A, e1, ap);
	edge(5u, A, e2, ap);
	edge(6u, B, C - B, bm);
	// an initial overlap comes first: Ericson's closest-point test and clamp ("Closest-point queries") in binary64
	{
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
		if (dotd(q, q) <= rr) {
			o_.t = 0.0;
			if (FULL) {
				o_.region = rule == 3u ? 4u : rule == 4u ? 3u : rule == 7u ? 0u : rule; // vertices 1 2 3, edges 4 5 6, the face 0
				o_.c = mk3d((A.x + e1.x * u2) + e2.x * v2, (A.y + e1.y * u2) + e2.y * v2, (A.z + e1.z * u2) + e2.z * v2);
			}
		}
	}
	return o_;
}

// ---- the pruning key --------------------------------------------------------------------------------------------------------

// the sweep a lane has in flight and what it has found so far
struct SweepLane {
	float ox, oy, oz, dx, dy, dz, ix, iy, iz; // origin, displacement, 1 / displacement
	float r, tmax;
	float best;   // the smallest t32 so far; tmax until a triangle is accepted
	int prim;     // its triangle, -1: none
	uint32_t ref; // the lane's state
};

// 1 / d_k for the slab test.  The slack's derivation wants a reciprocal with a relative error of 2^-24: a normal number.  For
// d_k == 0 it is the infinity the slab test handles (a segment parallel to the planes).  For a nonzero d_k whose reciprocal
// is infinite (a subnormal d_k: with a tmax near 2^128 the centre still moves along that axis) or subnormal or zero (|d_k|
// above 2^126) it is a NaN, which sweep_axis takes as "no constraint from this axis": less pruning, never a wrong answer.
__device__ __forceinline__ float sweep_recip(float d) {
	const float inv = 1.f / d;
	const bool zero = (__float_as_uint(d) & 0x7fffffffu) == 0u;
	const bool normal = fabsf(inv) >= 1.17549435e-38f && fabsf(inv) < kSweepInf; // (2^-126)
	return (zero || normal) ? inv : __uint_as_float(0x7fc00000u);
}

// one axis of the slab test on the inflated and widened box: the parameters at which the segment crosses its two planes
__device__ __forceinline__ void sweep_axis(float lo, float hi, float o, float inv, float r, float& tNear, float& tFar) {
	const float lo1 = lo - r, hi1 = hi + r;
	const float e = kSweepSlack * (fabsf(o) + __builtin_fmaxf(fabsf(lo1), fabsf(hi1)));
	const float t1 = ((lo1 - e) - o) * inv, t2 = ((hi1 + e) - o) * inv;
	const bool nan = !(t1 == t1) || !(t2 == t2); // 0 * inf: on a plane and parallel to it -- no constraint from this axis
	tNear = nan ? -kSweepInf : __builtin_fminf(t1, t2);
	tFar = nan ? kSweepInf : __builtin_fmaxf(t1, t2);
}

// A box against a lane's sweep: the pruning key (see the head of this file); +inf for a box that is skipped.
__device__ __forceinline__ float sweep_key(const SweepLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	float nx, fx, ny, fy, nz, fz;
	sweep_axis(lox, hix, q.ox, q.ix, q.r, nx, fx);
	sweep_axis(loy, hiy, q.oy, q.iy, q.r, ny, fy);
	sweep_axis(loz, hiz, q.oz, q.iz, q.r, nz, fz);
	const float tNear = __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz), tFar = __builtin_fminf(__builtin_fminf(fx, fy), fz);
	// (an unused slot's box is at +infinity: its widened planes are inf - inf)
	return (lox < kSweepInf && tNear <= tFar && tFar >= 0.f && tNear <= q.best) ? tNear : kSweepInf;
}

// a triangle of a reached leaf: the smallest pair (t32, index) so far stays
__device__ __forceinline__ void sweep_take(SweepLane& q, double t, int prim) {
	if (t < kSweepInfD) {
		const float t32 = (float)t;
		if (t32 < q.best || (t32 == q.best && (q.prim < 0 || prim < q.prim))) {
			q.best = t32;
			q.prim = prim;
		}
	}
}

// One round of the wave's traversal: the keyed descent (keyed_round, hip/query_common.hpp) on sweep_key against the lane's
// `best`, then one leaf per lane that is at one, primitives in array order.
template <class CanRefill>
__device__ __forceinline__ void s_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, SweepLane& q, CanRefill canRefill) {
	q.ref = keyed_round(
		sc, st, stagedNodes, q.ref, q.best, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return sweep_key(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			const d3 o = mk3d((double)q.ox, (double)q.oy, (double)q.oz), d = mk3d((double)q.dx, (double)q.dy, (double)q.dz);
			leaf_prims<false>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				// the triangle's own three-corner box against the bound, as a slot's: the binary64 evaluation only behind it
				const CornerBox b = tri_corner_box(cur);
				if (sweep_key(q, b.lox, b.hix, b.loy, b.hiy, b.loz, b.hiz) < kSweepInf)
					sweep_take(q, sweep_value<false>(cur, o, d, (double)q.r, (double)q.tmax).t, prim);
			});
		});
}

} // namespace

__global__ void __launch_bounds__(kBlock, 3) k_query_sweep(const SweepParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	SweepLane q = {};
	q.ref = kRefDone;
	q.prim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false, valid = false;

	// a finished sweep's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const SweepParams& P = kernarg_view<SweepParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = item;
		const d3 o = mk3d((double)q.ox, (double)q.oy, (double)q.oz), d = mk3d((double)q.dx, (double)q.dy, (double)q.dz);
		float t = valid ? q.tmax : kSweepInf;
		uint32_t region = 0u;
		// none: the end of the path; invalid: the origin as given
		float cx = q.ox, cy = q.oy, cz = q.oz;
		if (valid) {
			const double tm = (double)q.tmax;
			cx = (float)(o.x + tm * d.x), cy = (float)(o.y + tm * d.y), cz = (float)(o.z + tm * d.z);
		}
		float px = cx, py = cy, pz = cz, nx = 0.f, ny = 0.f, nz = 0.f;
		if (q.prim >= 0) {
			const SweepValue w = sweep_value<true>(triangle_load(sc.tris, (uint32_t)q.prim), o, d, (double)q.r, (double)q.tmax); // the winner's operations once more: the same value
			const d3 c = mk3d(o.x + w.t * d.x, o.y + w.t * d.y, o.z + w.t * d.z);
			const double r = (double)q.r;
			t = (float)w.t;
			region = w.region;
			cx = (float)c.x, cy = (float)c.y, cz = (float)c.z;
			px = (float)w.c.x, py = (float)w.c.y, pz = (float)w.c.z;
			if (r != 0.0)
				nx = (float)((c.x - w.c.x) / r), ny = (float)((c.y - w.c.y) / r), nz = (float)((c.z - w.c.z) / r);
		}
		P.t[i] = t;
		P.prim[i] = q.prim;
		if (P.region)
			P.region[i] = (uint8_t)region;
		if (P.point)
			P.point[3 * i + 0] = px, P.point[3 * i + 1] = py, P.point[3 * i + 2] = pz;
		if (P.center)
			P.center[3 * i + 0] = cx, P.center[3 * i + 1] = cy, P.center[3 * i + 2] = cz;
		if (P.normal)
			P.normal[3 * i + 0] = nx, P.normal[3 * i + 1] = ny, P.normal[3 * i + 2] = nz;
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<SweepParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const SweepParams& P = kernarg_view<SweepParams>();
			const size_t i3 = 3 * (size_t)item;
			q.ox = P.origins[i3 + 0], q.oy = P.origins[i3 + 1], q.oz = P.origins[i3 + 2];
			q.dx = P.directions[i3 + 0], q.dy = P.directions[i3 + 1], q.dz = P.directions[i3 + 2];
			q.r = P.radius[item];
			q.tmax = P.tmax ? P.tmax[item] : 1.f;
			q.ix = sweep_recip(q.dx), q.iy = sweep_recip(q.dy), q.iz = sweep_recip(q.dz);
			// a NaN or infinite component of o or d, a radius or tmax that is NaN, negative or infinite: not a sweep (t = +inf)
			valid = finite3(q.ox, q.oy, q.oz) && finite3(q.dx, q.dy, q.dz) && q.r >= 0 && q.r < kSweepInf && q.tmax >= 0 && q.tmax < kSweepInf;
			q.best = q.tmax;
			q.prim = -1;
			st.reset();
			live = true;
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly sweeps that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished sweeps, while sweeps remain
		s_traverse(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<SweepParams>().error);
}

void launch_sweep(const SweepParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_sweep, P, P.n, numCUs, lc.perCU[kLcSweep][0], stream);
}

} // namespace tyr
