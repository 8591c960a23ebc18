// sweep_capsule.hip -- batched swept-capsule queries on the uploaded scene (tyr_query_sweep_capsule, host/sweep_capsule.cpp): for
// each of the caller's capsules -- everything within r of the axis p -> q, both ends moving along d -- the first parameter t at
// which it touches a triangle of the scene, which triangle, and where (include/tyr_c.h "Swept-capsule queries": an argmin over
// all triangles with no traversal order in it, every operation binary64 in a fixed order, so that tests/sweep_capsule_ref.py
// reproduces each word by brute force).
//
// One capsule to a lane on a persistent grid, with the pieces of the swept spheres (hip/sweep.hip): the chunked ticket feed, the
// first nStaged quad records in LDS, the LdsStack with its private spill arrays, triangle_load, the flat lane states, the keyed
// descent (keyed_round, hip/query_common.hpp).  This unit supplies the pair value, the key and what is done with a leaf.
//
// The pair value: the capsule touches the triangle T exactly when the sphere around p + t d touches the prism
// M = { x - sigma a : x in T, sigma in [0, 1] }, a = q - p.  Twenty candidates -- M's two cap faces and three side faces, its six
// vertices and nine edges -- each by the swept sphere's formula of its kind, from shared sub-results: four normals (the caps
// share theirs), six vertex vectors m = p - V with dot(m, d) and dot(m, m) - r^2, four edge vectors (e1', e2', e3', -a) with
// dot(e, e) and dot(d, e).  The least accepted t wins, of equal t the lower feature code: a rule without an order in it, so the
// candidates are evaluated grouped by the vertex vector they use, and a candidate's division and square root only when its
// other conditions hold.  An initial overlap is the closest-segment pair value (hip/segment_value.hpp) within r.
//
// A slot's key is the parameter at which the path of p enters the slot's box grown to
//     [lo_k - (r + max(a_k, 0)),  hi_k + (r + max(-a_k, 0))]
// from the swept sphere's binary32 slab test.  At a contact p + t d is within r of a point x - sigma a with x in the box, so it
// lies in the grown box: the entry parameter is a lower bound of the value of every triangle in the box.  Every plane of the
// grown box is first moved outward by
//     kCapsuleSlack * (|p_k| + max(|lo1_k|, |hi1_k|)),      kCapsuleSlack = 32 * 2^-24
// (lo1, hi1: the grown planes), which is more than the roundings can add up to: 10 * 2^-24 of the same form, four more than the
// swept sphere's for a_k in binary32 and the growth's own add (DESIGN.md "Swept-capsule queries" derives it).  A slot is skipped
// only when the path misses that box, leaves it before 0, or enters it after `best` -- `>`: a box at exactly the bound is still
// visited, since ties go to the lower index wherever it lies.  A NaN in the slab test counts as "visit".
#include "sweep_capsule.hpp"

#include "device_common.hpp"
#include "query_common.hpp"
#include "segment_value.hpp"
#include "vecmath64.hpp"

namespace tyr {

namespace {

constexpr float kCapsuleUlp = 5.9604644775390625e-8f; // 2^-24
constexpr float kCapsuleSlack = 32.f * kCapsuleUlp;   // of |p_k| + max(|lo1_k|, |hi1_k|), per plane: 10 needed (3.2x)
constexpr float kCapsuleInf = __builtin_inff();
constexpr double kCapsuleInfD = __builtin_inf();

// ---- the value of a (capsule, triangle) pair: include/tyr_c.h "Swept-capsule queries", operation by operation ---------------

struct CapsuleValue {
	double t; // +inf: the pair has no value
	double s;
	uint32_t feature, region;
	d3 point; // on the triangle
};

template <bool FULL>
__device__ __forceinline__ CapsuleValue capsule_value(const TriData& td, d3 o, d3 P1, d3 d, double r, double tmax) {
	CapsuleValue o_;
	o_.t = kCapsuleInfD, o_.s = 0.0, o_.feature = 0u, o_.region = 0u, o_.point = mk3d(0.0, 0.0, 0.0);
	const double rr = r * r;
	// an initial overlap comes first: the axis at rest within r of the triangle
	{
		const SegValue w = segment_value<FULL>(td, o, P1);
		if (w.F <= rr) {
			o_.t = 0.0;
			if (FULL)
				o_.s = w.s, o_.region = w.region, o_.point = w.y;
			return o_;
		}
	}
	// the corners tyr_triangle_bboxes bounds: vert and the binary32 sums vert + e1, vert + e2
	const d3 A = mk3d((double)td.a.x, (double)td.a.y, (double)td.a.z);
	const d3 B = mk3d((double)(td.a.x + td.a.w), (double)(td.a.y + td.b.x), (double)(td.a.z + td.b.y));
	const d3 C = mk3d((double)(td.a.x + td.b.z), (double)(td.a.y + td.b.w), (double)(td.a.z + td.c.x));
	const d3 a = P1 - o, na = mk3d(-a.x, -a.y, -a.z);
	const d3 e1 = B - A, e2 = C - A, e3 = C - B;
	const double dd = dotd(d, d);
	// the least t, of equal t the lower feature code: the order of the offers does not matter
	auto offer = [&](double t, uint32_t feature, double s, uint32_t region, d3 pt) {
		if (t >= 0.0 && t <= tmax) {
			if (FULL) {
				if (t < o_.t || (t == o_.t && feature < o_.feature))
					o_.t = t, o_.s = s, o_.feature = feature, o_.region = region, o_.point = pt;
			} else if (t < o_.t) {
				o_.t = t;
			}
		}
	};
	// a face with the origin O (m = o - O), the edges f1, f2 and the normal n = cross(f1, f2): the sweep's face
	auto face = [&](d3 n, double nn, double ln, double nd, d3 O, d3 m, d3 f1, d3 f2, bool side, uint32_t feature, double s, uint32_t region) {
		const double h = dotd(n, m);
		const double sg = h >= 0.0 ? 1.0 : -1.0;
		const double sdn = sg * nd;
		const double ah = __builtin_fabs(h);
		const double rl = r * ln;
		if (nn > 0.0 && sdn < 0.0 && ah > rl) {
			const double t = (ah - rl) / (-sdn);
			const double k = (sg * r) / ln;
			const d3 c = mk3d((o.x + t * d.x) - n.x * k, (o.y + t * d.y) - n.y * k, (o.z + t * d.z) - n.z * k);
			const d3 w = c - O;
			const double bv = dotd(crossd(w, f2), n), bw = dotd(crossd(f1, w), n);
			if (bv >= 0.0 && bw >= 0.0 && (side ? (bv <= nn && bw <= nn) : ((bv + bw) <= nn))) {
				if (!FULL) {
					offer(t, feature, 0.0, 0u, c);
				} else if (side) {
					const double u = bv / nn, v = bw / nn;
					offer(t, feature, v, region, mk3d(O.x + f1.x * u, O.y + f1.y * u, O.z + f1.z * u));
				} else {
					offer(t, feature, s, region, s == 0.0 ? c : mk3d(c.x + a.x, c.y + a.y, c.z + a.z));
				}
			}
		}
	};
	// a vertex with the vector m = o - P: b = dot(m, d), c = dot(m, m) - rr
	auto vertex = [&](double b, double c, uint32_t feature, double s, uint32_t region, d3 P) {
		const double disc = b * b - dd * c;
		if (dd > 0.0 && b < 0.0 && c > 0.0 && disc >= 0.0)
			offer((-b - __builtin_sqrt(disc)) / dd, feature, s, region, P);
	};
	// an edge from P0 along e (ee = dot(e, e), de = dot(d, e)) with m = o - P0, md = dot(m, d), cv = dot(m, m) - rr; own: s = the
	// edge's parameter and point = V (a lateral edge), else s as given and point = V + e * sg
	auto edge = [&](d3 e, double ee, double de, d3 m, double md, double cv, uint32_t feature, double s, bool own, uint32_t region, d3 V) {
		const double me = dotd(m, e);
		const double qa = ee * dd - de * de;
		const double b = ee * md - de * me;
		const double c = ee * cv - me * me;
		const double disc = b * b - qa * c;
		if (ee > 0.0 && qa > 0.0 && b < 0.0 && c > 0.0 && disc >= 0.0) {
			const double t = (-b - __builtin_sqrt(disc)) / qa;
			const double sg = (me + t * de) / ee;
			if (sg >= 0.0 && sg <= 1.0)
				offer(t, feature, own ? sg : s, region, own ? V : mk3d(V.x + e.x * sg, V.y + e.y * sg, V.z + e.z * sg));
		}
	};
	const double ee1 = dotd(e1, e1), de1 = dotd(d, e1), ee2 = dotd(e2, e2), de2 = dotd(d, e2), ee3 = dotd(e3, e3), de3 = dotd(d, e3);
	const double eea = dotd(na, na), dea = dotd(d, na);
	const d3 n = crossd(e1, e2);
	const double nn = dotd(n, n), ln = __builtin_sqrt(nn), nd = dotd(n, d);
	{ // what uses A
		const d3 m = o - A;
		const double md = dotd(m, d), cv = dotd(m, m) - rr;
		face(n, nn, ln, nd, A, m, e1, e2, false, 0u, 0.0, 0u);
		const d3 n2 = crossd(e1, na), n3 = crossd(e2, na);
		const double nn2 = dotd(n2, n2), nn3 = dotd(n3, n3);
		face(n2, nn2, __builtin_sqrt(nn2), dotd(n2, d), A, m, e1, na, true, 2u, 0.0, 4u);
		face(n3, nn3, __builtin_sqrt(nn3), dotd(n3, d), A, m, e2, na, true, 3u, 0.0, 5u);
		vertex(md, cv, 5u, 0.0, 1u, A);
		edge(e1, ee1, de1, m, md, cv, 11u, 0.0, false, 4u, A);
		edge(e2, ee2, de2, m, md, cv, 12u, 0.0, false, 5u, A);
		edge(na, eea, dea, m, md, cv, 17u, 0.0, true, 1u, A);
	}
	{ // B
		const d3 m = o - B;
		const double md = dotd(m, d), cv = dotd(m, m) - rr;
		const d3 n4 = crossd(e3, na);
		const double nn4 = dotd(n4, n4);
		face(n4, nn4, __builtin_sqrt(nn4), dotd(n4, d), B, m, e3, na, true, 4u, 0.0, 6u);
		vertex(md, cv, 6u, 0.0, 2u, B);
		edge(e3, ee3, de3, m, md, cv, 13u, 0.0, false, 6u, B);
		edge(na, eea, dea, m, md, cv, 18u, 0.0, true, 2u, B);
	}
	{ // C
		const d3 m = o - C;
		const double md = dotd(m, d), cv = dotd(m, m) - rr;
		vertex(md, cv, 7u, 0.0, 3u, C);
		edge(na, eea, dea, m, md, cv, 19u, 0.0, true, 3u, C);
	}
	{ // A - a
		const d3 Am = A - a;
		const d3 m = o - Am;
		const double md = dotd(m, d), cv = dotd(m, m) - rr;
		face(n, nn, ln, nd, Am, m, e1, e2, false, 1u, 1.0, 0u);
		vertex(md, cv, 8u, 1.0, 1u, A);
		edge(e1, ee1, de1, m, md, cv, 14u, 1.0, false, 4u, A);
		edge(e2, ee2, de2, m, md, cv, 15u, 1.0, false, 5u, A);
	}
	{ // B - a
		const d3 m = o - (B - a);
		const double md = dotd(m, d), cv = dotd(m, m) - rr;
		vertex(md, cv, 9u, 1.0, 2u, B);
		edge(e3, ee3, de3, m, md, cv, 16u, 1.0, false, 6u, B);
	}
	{ // C - a
		const d3 m = o - (C - a);
		vertex(dotd(m, d), dotd(m, m) - rr, 10u, 1.0, 3u, C);
	}
	return o_;
}

// ---- the pruning key --------------------------------------------------------------------------------------------------------

// the capsule a lane has in flight and what it has found so far
struct CapsuleLane {
	float px, py, pz, qx, qy, qz, dx, dy, dz, ix, iy, iz; // the axis, the displacement, 1 / displacement
	float glx, gly, glz, ghx, ghy, ghz;                   // what a box grows by below and above: r + max(a_k, 0), r + max(-a_k, 0)
	float r, tmax;
	float best;   // the smallest t32 so far; tmax until a triangle is accepted
	int prim;     // its triangle, -1: none
	uint32_t ref; // the lane's state
};

// 1 / d_k for the slab test, as hip/sweep.hip's sweep_recip: the infinity for d_k == 0, a NaN ("no constraint from this axis")
// where the reciprocal of a nonzero d_k is no normal number
__device__ __forceinline__ float capsule_recip(float d) {
	const float inv = 1.f / d;
	const bool zero = (__float_as_uint(d) & 0x7fffffffu) == 0u;
	const bool normal = fabsf(inv) >= 1.17549435e-38f && fabsf(inv) < kCapsuleInf; // (2^-126)
	return (zero || normal) ? inv : __uint_as_float(0x7fc00000u);
}

__device__ __forceinline__ void capsule_lane_setup(CapsuleLane& q) {
	const float ax = q.qx - q.px, ay = q.qy - q.py, az = q.qz - q.pz;
	q.glx = q.r + __builtin_fmaxf(ax, 0.f), q.gly = q.r + __builtin_fmaxf(ay, 0.f), q.glz = q.r + __builtin_fmaxf(az, 0.f);
	q.ghx = q.r + __builtin_fmaxf(-ax, 0.f), q.ghy = q.r + __builtin_fmaxf(-ay, 0.f), q.ghz = q.r + __builtin_fmaxf(-az, 0.f);
	q.ix = capsule_recip(q.dx), q.iy = capsule_recip(q.dy), q.iz = capsule_recip(q.dz);
}

// one axis of the slab test on the grown and widened box: the parameters at which the path of p crosses its two planes
__device__ __forceinline__ void capsule_axis(float lo, float hi, float o, float inv, float gl, float gh, float& tNear, float& tFar) {
	const float lo1 = lo - gl, hi1 = hi + gh;
	const float e = kCapsuleSlack * (fabsf(o) + __builtin_fmaxf(fabsf(lo1), fabsf(hi1)));
	const float t1 = ((lo1 - e) - o) * inv, t2 = ((hi1 + e) - o) * inv;
	const bool nan = !(t1 == t1) || !(t2 == t2); // 0 * inf: on a plane and parallel to it -- no constraint from this axis
	tNear = nan ? -kCapsuleInf : __builtin_fminf(t1, t2);
	tFar = nan ? kCapsuleInf : __builtin_fmaxf(t1, t2);
}

// A box against a lane's capsule: the pruning key (see the head of this file); +inf for a box that is skipped.
__device__ __forceinline__ float capsule_key(const CapsuleLane& q, float lox, float hix, float loy, float hiy, float loz, float hiz) {
	float nx, fx, ny, fy, nz, fz;
	capsule_axis(lox, hix, q.px, q.ix, q.glx, q.ghx, nx, fx);
	capsule_axis(loy, hiy, q.py, q.iy, q.gly, q.ghy, ny, fy);
	capsule_axis(loz, hiz, q.pz, q.iz, q.glz, q.ghz, nz, fz);
	const float tNear = __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz), tFar = __builtin_fminf(__builtin_fminf(fx, fy), fz);
	// (an unused slot's box is at +infinity: its widened planes are inf - inf)
	return (lox < kCapsuleInf && tNear <= tFar && tFar >= 0.f && tNear <= q.best) ? tNear : kCapsuleInf;
}

// a triangle of a reached leaf: the smallest pair (t32, index) so far stays
__device__ __forceinline__ void capsule_take(CapsuleLane& q, double t, int prim) {
	if (t < kCapsuleInfD) {
		const float t32 = (float)t;
		if (t32 < q.best || (t32 == q.best && (q.prim < 0 || prim < q.prim))) {
			q.best = t32;
			q.prim = prim;
		}
	}
}

// One round of the wave's traversal: the keyed descent (keyed_round, hip/query_common.hpp) on capsule_key against the lane's
// `best`, then one leaf per lane that is at one, primitives in array order.
template <class CanRefill>
__device__ __forceinline__ void c_traverse(const DevScene& sc, LdsStack<kQueryStackLds, true>& st, const float4* stagedNodes, CapsuleLane& q, CanRefill canRefill) {
	q.ref = keyed_round(
		sc, st, stagedNodes, q.ref, q.best, canRefill, [&](float lox, float hix, float loy, float hiy, float loz, float hiz) { return capsule_key(q, lox, hix, loy, hiy, loz, hiz); },
		[&](uint32_t leaf) {
			const d3 o = mk3d((double)q.px, (double)q.py, (double)q.pz), P1 = mk3d((double)q.qx, (double)q.qy, (double)q.qz);
			const d3 d = mk3d((double)q.dx, (double)q.dy, (double)q.dz);
			leaf_prims<false>(sc.tris, leaf, [&](const TriData& cur, int prim) {
				// the triangle's own three-corner box against the bound, as a slot's: the binary64 evaluation only behind it
				const CornerBox b = tri_corner_box(cur);
				if (capsule_key(q, b.lox, b.hix, b.loy, b.hiy, b.loz, b.hiz) < kCapsuleInf)
					capsule_take(q, capsule_value<false>(cur, o, P1, d, (double)q.r, (double)q.tmax).t, prim);
			});
		});
}

} // namespace

__global__ void __launch_bounds__(kBlock, 2) k_query_sweep_capsule(const SweepCapsuleParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	CapsuleLane q = {};
	q.ref = kRefDone;
	q.prim = -1;
	uint32_t item = 0;
	bool live = false, overflow = false, valid = false;

	// a finished capsule's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const SweepCapsuleParams& P = kernarg_view<SweepCapsuleParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = item;
		const d3 o = mk3d((double)q.px, (double)q.py, (double)q.pz), P1 = mk3d((double)q.qx, (double)q.qy, (double)q.qz);
		const d3 d = mk3d((double)q.dx, (double)q.dy, (double)q.dz);
		float t = valid ? q.tmax : kCapsuleInf, s = 0.f;
		uint32_t feature = 0u, region = 0u;
		// none: the end of p's path; invalid: p as given
		float cx = q.px, cy = q.py, cz = q.pz;
		if (valid) {
			const double tm = (double)q.tmax;
			cx = (float)(o.x + tm * d.x), cy = (float)(o.y + tm * d.y), cz = (float)(o.z + tm * d.z);
		}
		float px = cx, py = cy, pz = cz, nx = 0.f, ny = 0.f, nz = 0.f;
		if (q.prim >= 0) {
			const CapsuleValue w = capsule_value<true>(triangle_load(sc.tris, (uint32_t)q.prim), o, P1, d, (double)q.r, (double)q.tmax); // the winner's operations once more: the same value
			const d3 a = P1 - o;
			const d3 c = mk3d((o.x + w.s * a.x) + w.t * d.x, (o.y + w.s * a.y) + w.t * d.y, (o.z + w.s * a.z) + w.t * d.z);
			const double r = (double)q.r;
			t = (float)w.t, s = (float)w.s;
			feature = w.feature, region = w.region;
			cx = (float)c.x, cy = (float)c.y, cz = (float)c.z;
			px = (float)w.point.x, py = (float)w.point.y, pz = (float)w.point.z;
			if (r != 0.0)
				nx = (float)((c.x - w.point.x) / r), ny = (float)((c.y - w.point.y) / r), nz = (float)((c.z - w.point.z) / r);
		}
		P.t[i] = t;
		P.prim[i] = q.prim;
		if (P.s)
			P.s[i] = s;
		if (P.feature)
			P.feature[i] = (uint8_t)feature;
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
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<SweepCapsuleParams>().ticket; });
		if (fresh != kNoItem) {
			item = fresh;
			const SweepCapsuleParams& P = kernarg_view<SweepCapsuleParams>();
			const size_t i3 = 3 * (size_t)item;
			q.px = P.p[i3 + 0], q.py = P.p[i3 + 1], q.pz = P.p[i3 + 2];
			q.qx = P.q[i3 + 0], q.qy = P.q[i3 + 1], q.qz = P.q[i3 + 2];
			q.dx = P.directions[i3 + 0], q.dy = P.directions[i3 + 1], q.dz = P.directions[i3 + 2];
			q.r = P.radius[item];
			q.tmax = P.tmax ? P.tmax[item] : 1.f;
			capsule_lane_setup(q);
			// a NaN or infinite component of p, q or d, a radius or tmax that is NaN, negative or infinite: not a capsule (t = +inf)
			valid = finite3(q.px, q.py, q.pz) && finite3(q.qx, q.qy, q.qz) && finite3(q.dx, q.dy, q.dz) && q.r >= 0 && q.r < kCapsuleInf && q.tmax >= 0 && q.tmax < kCapsuleInf;
			q.best = q.tmax;
			q.prim = -1;
			st.reset();
			live = true;
			q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
			if (q.ref == kRefDone)
				finish();
		}
		if (feed.top_up(live)) // mostly capsules that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished capsules, while capsules remain
		c_traverse(sc, st, stagedNodes, q, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<SweepCapsuleParams>().error);
}

void launch_sweep_capsule(const SweepCapsuleParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_sweep_capsule, P, P.n, numCUs, lc.perCU[kLcSweepCapsule][0], stream);
}

} // namespace tyr
