// query.hip -- batched ray queries on the uploaded scene (tyr_query_closest / tyr_query_any, host/query.cpp): the caller's
// rays, read in place from n x 3 float arrays, answered one to a lane on a persistent grid.
//
//   closest hit  CachedBVH::intersect (bvh.h:118-161) with ray.distance = tmax; with spheres, intersect_scene
//                (kernel.cu:125-140): the seven spheres in reverse order first, then the tree, seeded with their distance
//   any hit      CachedBVH::intersectSimple(ray, closestAllowed = tmax) (bvh.h:213-256); with spheres, intersect_scene_simple
//                (kernel.cu:163-174): the tree, then the spheres with (d + epsilon) < tmax.  A boolean: the order of the two
//                halves does not change it, so the spheres are tested first and a blocked ray never enters the tree.
//
// The production traversal's pieces (hip/traverse.hpp), not its loop: quad nodes through test_quad, the first nStaged quad
// nodes in LDS, the LdsStack with its private spill arrays, triangle_test on the leaves.  A wave is a flat per-lane state
// machine (interior ref | leaf ref | kRefPop | kRefDone) as in k_trace_flat: one pop attempt and one quad test per lane per
// trip, refilled from a private range of ray indices that it draws from one device-wide ticket word, `chunk` rays at a time.
// Rays are contiguous inside a chunk, so a caller's coherent rays (a camera's) stay together in a wave.
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
	const uint32_t nStaged = sc.nStaged;
	for (uint32_t i = threadIdx.x; i < 7 * nStaged; i += kBlock) {
		const uint32_t v = i / nStaged, k = i - v * nStaged;
		stagedNodes[v * kStagedNodes + k] = sc.quads[8 * k + v];
	}
	__syncthreads();
	const uint32_t lane = lane_id();
	const unsigned long long below = (1ull << lane) - 1ull;
	const uint32_t n = P0.n;

	float rox = 0.f, roy = 0.f, roz = 0.f, rdx = 0.f, rdy = 0.f, rdz = 0.f, rix = 0.f, riy = 0.f, riz = 0.f;
	bool regular = true;
	float dist = 0.f, tmax = 0.f;
	uint32_t ref = kRefDone, ray = 0;
	int prim = -1, sphere = -1;
	bool hitTri = false, occluded = false, live = false, overflow = false;

	// a finished ray's answer, into the caller's arrays at its index (64-bit offsets: 3 n floats pass 2^32 bytes)
	auto finish = [&]() {
		const QueryParams& P = kernarg_view<QueryParams>(); // (read where it lies: not held in scalar registers through the descent)
		const size_t i = ray;
		if (ANY) {
			P.occluded[i] = occluded ? 1 : 0;
		} else {
			const bool hit = hitTri || sphere >= 0;
			P.t[i] = dist;
			P.prim[i] = hitTri ? prim : (hit ? sphere : -1);
			if (P.geom)
				P.geom[i] = hitTri ? 1 : (hit ? 0 : -1); // GeometryType: 0 sphere, 1 triangle
			if (P.uv) {
				const float2 uv = hitTri ? triangle_uv(sc.tris, (uint32_t)prim, mk3(rox, roy, roz), mk3(rdx, rdy, rdz)) : make_float2(0.f, 0.f);
				reinterpret_cast<float2*>(P.uv)[i] = uv;
			}
		}
		overflow = overflow || st.overflow;
		live = false;
		ref = kRefDone;
	};

	QueryFeed feed;
	feed.init(n);
	bool exhausted = (n == 0);
	for (;;) {
		// ---- refill free lanes ----
		const unsigned long long idleMask = __ballot(!live);
		const uint32_t nIdle = (uint32_t)__popcll(idleMask);
		if (!exhausted && nIdle >= kQueryRefillMinIdle) {
			const uint32_t rank = (uint32_t)__popcll(idleMask & below);
			uint32_t got = 0;
			bool fed = false;
			while (got < nIdle) {
				if (feed.next == feed.end && !feed.draw(kernarg_view<QueryParams>().ticket, n, lane)) {
					exhausted = true;
					break;
				}
				const uint32_t avail = feed.end - feed.next, room = nIdle - got;
				const uint32_t take = avail < room ? avail : room;
				if (!live && rank >= got && rank < got + take) {
					ray = feed.next + (rank - got);
					fed = true;
				}
				feed.next += take;
				got += take;
			}
			if (fed) {
				const QueryParams& P = kernarg_view<QueryParams>();
				const size_t i3 = 3 * (size_t)ray;
				const float ox = P.origins[i3 + 0], oy = P.origins[i3 + 1], oz = P.origins[i3 + 2];
				const float dx = P.directions[i3 + 0], dy = P.directions[i3 + 1], dz = P.directions[i3 + 2];
				tmax = P.tmax ? P.tmax[ray] : kVeryFar;
				const RayConst nr = make_ray(mk3(ox, oy, oz), mk3(dx, dy, dz));
				rox = nr.o.x, roy = nr.o.y, roz = nr.o.z, rdx = nr.d.x, rdy = nr.d.y, rdz = nr.d.z, rix = nr.inv.x, riy = nr.inv.y, riz = nr.inv.z;
				regular = ray_is_regular(nr);
				dist = tmax;
				prim = -1;
				sphere = -1;
				hitTri = false;
				occluded = false;
				st.reset();
				live = true;
				// a ray with a NaN or infinite component is a miss (and never enters a box)
				const bool valid = finite3(ox, oy, oz) && finite3(dx, dy, dz);
				if (SPHERES && valid) {
#pragma unroll
					for (int s = TYR_NUM_SPHERES; s--;) {
						const float d = sphere_intersect(P.spheres[s], nr.o, nr.d);
						if (ANY) {
							occluded = occluded || (d && (d + kEpsilon) < tmax); // kernel.cu:168-172
						} else if (d && d < dist) { // kernel.cu:130-135
							dist = d;
							sphere = s;
						}
					}
				}
				ref = (valid && !occluded) ? root_ref(sc, nr, dist) : kRefDone;
				if (ref != kRefDone)
					ref = sc.quadRootRef;
				if (ref == kRefDone)
					finish(); // missed the root box, blocked by a sphere, or not a ray
			}
			// mostly rays that ended at once: top the wave up again first
			if (!exhausted && (uint32_t)__popcll(__ballot(live)) < kQueryMinTraversing && (uint32_t)__popcll(__ballot(!live)) >= kQueryRefillMinIdle)
				continue;
		}
		if (__ballot(live) == 0ull) {
			if (exhausted)
				break;
			continue;
		}
		const bool allRegular = (__ballot(live && !regular) == 0ull);
		const RayConst r = { mk3(rox, roy, roz), mk3(rdx, rdy, rdz), mk3(rix, riy, riz), rix < 0, riy < 0, riz < 0 }; // bvh.h:120-121
		// ---- descent: one pop attempt + one quad test per lane per trip ----
		for (;;) {
			const uint32_t nTrav = (uint32_t)__popcll(q_traversing(ref));
			if (nTrav == 0)
				break;
			if (nTrav < kQueryMinTraversing) {
				const bool anyLeaf = q_at_leaf(ref) != 0ull;
				const bool canRefill = !exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle;
				if (anyLeaf || canRefill)
					break;
			}
			if (ref == kRefPop) {
				uint32_t pr;
				float pt;
				if (st.pop(pr, pt)) {
					if (pt < dist) // the pop-time half of Bbox.h:61 (any hit keeps no entry distance: -inf, always taken)
						ref = pr;
				} else {
					ref = kRefDone;
				}
			}
			if ((int)ref >= 0) {
				const QuadHits q = allRegular ? test_quad<true, !ANY, true>(sc.quads, ref, r, dist, stagedNodes, nStaged) : test_quad<false, !ANY, true>(sc.quads, ref, r, dist, stagedNodes, nStaged);
				const lanemask any01 = q.hit[0] | q.hit[1], any012 = any01 | q.hit[2];
				st.push3(q.hit[3] & any012, q.ref[3], q.t[3], q.hit[2] & any01, q.ref[2], q.t[2], q.hit[1] & q.hit[0], q.ref[1], q.t[1]);
				ref = lane_in(q.hit[0]) ? q.ref[0] : lane_in(q.hit[1]) ? q.ref[1] : lane_in(q.hit[2]) ? q.ref[2] : lane_in(q.hit[3]) ? q.ref[3] : kRefPop;
			}
		}
		// ---- leaves: bvh.h:129-140 (closest hit) / bvh.h:229-238 (any hit), primitives in array order ----
		if (q_is_leaf(ref)) {
			const uint32_t off = ref & (kMaxPrimOffset - 1);
			const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
			bool found = false;
			TriData tri = triangle_load(sc.tris, off);
			for (uint32_t i = 0; i < cnt && !found; ++i) {
				const TriData cur = tri; // the next primitive of the leaf is on its way while this one is tested
				if (i + 1 < cnt)
					tri = triangle_load(sc.tris, off + i + 1);
				const float t = triangle_test(cur, r);
				if (ANY) {
					found = (t > kEpsilon && ((dist - t) > kEpsilon)); // bvh.h:232-236
				} else if (t > kEpsilon && t < dist && ((dist - t) > kEpsilon)) { // bvh.h:133-137
					prim = (int)(off + i);
					dist = t;
					hitTri = true;
				}
			}
			occluded = occluded || found;
			ref = found ? kRefDone : kRefPop;
		}
		if (live && ref == kRefDone)
			finish();
	}
	if (__ballot(overflow) != 0ull && lane == 0)
		atomicOr(kernarg_view<QueryParams>().error, kQueryErrStackOverflow);
}

template <bool SPHERES>
__global__ void __launch_bounds__(kBlock, 5) k_query_closest(const QueryParams P) { query_body<false, SPHERES>(P); }
template <bool SPHERES>
__global__ void __launch_bounds__(kBlock, 5) k_query_any(const QueryParams P) { query_body<true, SPHERES>(P); }

void launch_query(const QueryParams& P, bool any, bool spheres, int numCUs, LaunchCache& lc, hipStream_t stream) {
	const Tuning t{}; // the occupancy query's answer, never a tuning override: queries do not follow the render's launch shape
	int& cached = lc.perCU[kLcQuery][(any ? 2 : 0) + (spheres ? 1 : 0)];
	if (any) {
		if (spheres)
			hipLaunchKernelGGL((k_query_any<true>), dim3(persistent_blocks(k_query_any<true>, P.n, t, numCUs, cached)), dim3(kBlock), 0, stream, P);
		else
			hipLaunchKernelGGL((k_query_any<false>), dim3(persistent_blocks(k_query_any<false>, P.n, t, numCUs, cached)), dim3(kBlock), 0, stream, P);
	} else {
		if (spheres)
			hipLaunchKernelGGL((k_query_closest<true>), dim3(persistent_blocks(k_query_closest<true>, P.n, t, numCUs, cached)), dim3(kBlock), 0, stream, P);
		else
			hipLaunchKernelGGL((k_query_closest<false>), dim3(persistent_blocks(k_query_closest<false>, P.n, t, numCUs, cached)), dim3(kBlock), 0, stream, P);
	}
}

} // namespace tyr
