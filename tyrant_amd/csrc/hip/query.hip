// query.hip -- batched ray queries on the uploaded scene (tyr_query_closest / tyr_query_any, host/query.cpp): the caller's
// rays, read in place from n x 3 float arrays, answered one to a lane on a persistent grid.
//
//   closest hit  CachedBVH::intersect (bvh.h:118-161) with ray.distance = tmax; with spheres, intersect_scene
//                (kernel.cu:125-140): the seven spheres in reverse order first, then the tree, seeded with their distance
//   any hit      CachedBVH::intersectSimple(ray, closestAllowed = tmax) (bvh.h:213-256); with spheres, intersect_scene_simple
//                (kernel.cu:163-174): the tree, then the spheres with (d + epsilon) < tmax.  A boolean: the order of the two
//                halves does not change it, so the spheres are tested first and a blocked ray never enters the tree.
//
// The loop is hip/query_common.hpp's, shared with the guide passes (hip/aov.hip): the production traversal's pieces
// (hip/traverse.hpp), not its loop -- quad nodes through test_quad, the first nStaged quad nodes in LDS, the LdsStack with its
// private spill arrays, triangle_test on the leaves.  A wave is a flat per-lane state machine (interior ref | leaf ref |
// kRefPop | kRefDone) as in k_trace_flat: one pop attempt and one quad test per lane per trip, refilled from a private range of
// ray indices that it draws from one device-wide ticket word, `chunk` rays at a time.  Rays are contiguous inside a chunk, so
// a caller's coherent rays (a camera's) stay together in a wave.  This file is what a query adds: the load of a caller's ray
// and its validity test, the any-hit sphere test, and the answer's way into the caller's arrays.
#include "device_common.hpp"
#include "query.hpp"
#include "query_common.hpp"

namespace tyr {

namespace {

// Moller-Trumbore's u, v of the winning triangle: the operations of triangle_test (hip/traverse.hpp, loader.h:21-46) in
// their order, once per hit ray after the traversal
__device__ __forceinline__ float2 triangle_uv(const float4* __restrict__ tris, uint32_t prim, f3 o, f3 d) {
	const TriData td = triangle_load(tris, prim);
	const f3 vert = mk3(td.a.x, td.a.y, td.a.z);
	const f3 e1 = mk3(td.a.w, td.b.x, td.b.y);
	const f3 e2 = mk3(td.b.z, td.b.w, td.c.x);
	const f3 pvec = cross(d, e2);
	const float det = dot(e1, pvec);
	const float invDet = 1 / det;
	const f3 tvec = o - vert;
	const float u = dot(tvec, pvec) * invDet;
	const f3 qvec = cross(tvec, e1);
	const float v = dot(d, qvec) * invDet;
	return make_float2(u, v);
}

} // namespace

// ANY = false: closest hit, ANY = true: any hit.  SPHERES: also the ctx's sphere table (TYR_QUERY_SPHERES).
template <bool ANY, bool SPHERES>
__device__ __forceinline__ void query_body(const QueryParams& P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, !ANY)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	QueryRay q = {};
	q.ref = kRefDone;
	float tmax = 0.f;
	uint32_t ray = 0;
	bool live = false, overflow = false;

	// a finished ray's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const QueryParams& P = kernarg_view<QueryParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = ray;
		if (ANY) {
			P.occluded[i] = q.occluded ? 1 : 0;
		} else {
			const bool hit = q.hitTri || q.sphere >= 0;
			P.t[i] = q.dist;
			P.prim[i] = q.hitTri ? q.prim : (hit ? q.sphere : -1);
			if (P.geom)
				P.geom[i] = q.hitTri ? 1 : (hit ? 0 : -1); // GeometryType: 0 sphere, 1 triangle
			if (P.uv) {
				const float2 uv = q.hitTri ? triangle_uv(sc.tris, (uint32_t)q.prim, mk3(q.ox, q.oy, q.oz), mk3(q.dx, q.dy, q.dz)) : make_float2(0.f, 0.f);
				reinterpret_cast<float2*>(P.uv)[i] = uv;
			}
		}
		overflow = overflow || st.overflow;
		live = false;
		q.ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(P0.n);
	for (;;) {
		// ---- refill free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<QueryParams>().ticket; });
		if (fresh != kNoItem) {
			ray = fresh;
			const QueryParams& P = kernarg_view<QueryParams>();
			const size_t i3 = 3 * (size_t)ray;
			const float ox = P.origins[i3 + 0], oy = P.origins[i3 + 1], oz = P.origins[i3 + 2];
			const float dx = P.directions[i3 + 0], dy = P.directions[i3 + 1], dz = P.directions[i3 + 2];
			tmax = P.tmax ? P.tmax[ray] : kVeryFar;
			const RayConst nr = make_ray(mk3(ox, oy, oz), mk3(dx, dy, dz));
			q.start(nr, tmax);
			st.reset();
			live = true;
			// a ray with a NaN or infinite component is a miss (and never enters a box)
			const bool valid = finite3(ox, oy, oz) && finite3(dx, dy, dz);
			if (SPHERES && valid) {
				if (ANY) {
#pragma unroll
					for (int s = TYR_NUM_SPHERES; s--;) { // kernel.cu:168-172
						const float d = sphere_intersect(P.spheres[s], nr.o, nr.d);
						q.occluded = q.occluded || (d && (d + kEpsilon) < tmax);
					}
				} else {
					q_spheres_closest(P.spheres, nr, q);
				}
			}
			q.ref = (valid && !q.occluded) ? root_ref(sc, nr, q.dist) : kRefDone;
			if (q.ref != kRefDone)
				q.ref = sc.quadRootRef;
			if (q.ref == kRefDone)
				finish(); // missed the root box, blocked by a sphere, or not a ray
		}
		if (feed.top_up(live)) // mostly rays that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished rays, while rays remain
		q_traverse<ANY>(sc, st, stagedNodes, q, live, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<QueryParams>().error);
}

template <bool SPHERES>
__global__ void __launch_bounds__(kBlock, 5) k_query_closest(const QueryParams P) { query_body<false, SPHERES>(P); }
template <bool SPHERES>
__global__ void __launch_bounds__(kBlock, 5) k_query_any(const QueryParams P) { query_body<true, SPHERES>(P); }

void launch_query(const QueryParams& P, bool any, bool spheres, int numCUs, LaunchCache& lc, hipStream_t stream) {
	const auto kernel = any ? (spheres ? k_query_any<true> : k_query_any<false>) : (spheres ? k_query_closest<true> : k_query_closest<false>);
	launch_persistent(kernel, P, P.n, numCUs, lc.perCU[kLcQuery][(any ? 2 : 0) + (spheres ? 1 : 0)], stream);
}

} // namespace tyr
