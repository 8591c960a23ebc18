// aov.hip -- first-hit guide buffers for denoisers (tyr_render_aov, host/aov.cpp): per pixel the average albedo and shading
// normal of spp camera rays, their average hit distance, and sample 0's identity.
//
// Sample s of local pixel p is k_primary's camera ray for ticket index = s * nPixels + p at scan-line cursor 0: the same
// seed (camera_seed), pixel mapping and jitter / thin lens (camera_focus, camera_lens; kernel.cu:247-297).  It is traced as
// extend traces it, intersect_scene (kernel.cu:125-140): the seven spheres in reverse order, then the tree seeded with
// their distance -- k_query_closest<true>'s loop with tmax = VERY_FAR.  A hit's albedo and normal are shade's
// (kernel.cu:365-386, hip/shade.hip): a sphere's colour and (hit - position) / radius; a triangle's (1, 1, 1) or palette
// colour and normalize(cross(e1, e2)); the normal flipped unless dot(n, direction) < 0.
//
// One lane owns one pixel and runs its samples in order, accumulating in registers: fixed float32 sums, no atomics.  A
// wave draws its pixels from the launch's ticket word `chunk` at a time (contiguous pixels: coherent rays).  A sample that
// misses the spheres and fails the root box is finished where it is generated (42 % of C3's camera rays), and so is the
// pixel whose every sample does: neither holds a traversal lane.  Otherwise the loop is the query kernel's: quad nodes
// through test_quad, the first nStaged quad nodes in LDS, the LdsStack, triangle_test on the leaves.
#include "aov.hpp"
#include "device_common.hpp"
#include "query.hpp"
#include "query_common.hpp"

namespace tyr {

__global__ void __launch_bounds__(kBlock, 5) k_render_aov(const AovParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
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
	const uint32_t n = P0.nPixels;

	// the sample in flight
	float rox = 0.f, roy = 0.f, roz = 0.f, rdx = 0.f, rdy = 0.f, rdz = 0.f, rix = 0.f, riy = 0.f, riz = 0.f;
	bool regular = true;
	float dist = 0.f;
	uint32_t ref = kRefDone;
	int prim = -1, sphere = -1;
	bool hitTri = false, overflow = false;
	// the pixel: live = owned by this lane, pending = its next sample is still to be generated
	uint32_t pixel = 0, s = 0, hits = 0;
	bool live = false, pending = false;
	float ax = 0.f, ay = 0.f, az = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, tsum = 0.f;

	// the finished sample into the pixel's sums; the pixel's outputs once its last sample is in
	auto sample_done = [&]() {
		const AovParams& P = kernarg_view<AovParams>();
		const bool hit = hitTri || sphere >= 0;
		f3 alb = mk3(0.f, 0.f, 0.f), nrm = mk3(0.f, 0.f, 0.f); // a miss adds +0 (the sums' order and signs stay fixed)
		const f3 d = mk3(rdx, rdy, rdz);
		if (hit) {
			if (hitTri) {
				const TriData td = triangle_load(sc.tris, (uint32_t)prim);
				nrm = normalize(cross(mk3(td.a.w, td.b.x, td.b.y), mk3(td.b.z, td.b.w, td.c.x))); // kernel.cu:380-383
				alb = mk3(1.f, 1.f, 1.f);
				if (P.palette) { // Scene.cpp:44's `tempTriangle.color` (shade.hip, TYR_FLAG_TRIANGLE_COLORS)
					const float4 c = P.palette[2u * (__float_as_uint(td.c.z) & 255u)];
					alb = mk3(c.x, c.y, c.z);
				}
			} else {
				const tyr_sphere& object = P.spheres[sphere];
				const f3 at = mk3(rox, roy, roz) + d * dist; // kernel.cu:368
				nrm = (at - ld3(object.position)) / object.radius;
				alb = ld3(object.color);
			}
			const bool outside = dot(nrm, d) < 0; // kernel.cu:386
			nrm = outside ? nrm : nrm * -1.f;
			tsum = tsum + dist;
			++hits;
		}
		ax = ax + alb.x, ay = ay + alb.y, az = az + alb.z;
		nx = nx + nrm.x, ny = ny + nrm.y, nz = nz + nrm.z;
		const uint32_t x = pixel % P.W, yl = pixel / P.W;
		const size_t out = (size_t)(yl * P.nranks + P.rank) * P.W + x;
		if (s == 0) { // sample 0's identity in the query convention: geom 0 sphere, 1 triangle, -1 miss
			if (P.prim)
				P.prim[out] = hitTri ? prim : (hit ? sphere : -1);
			if (P.geom)
				P.geom[out] = hitTri ? 1 : (hit ? 0 : -1);
		}
		overflow = overflow || st.overflow;
		ref = kRefDone;
		if (++s < P.spp) {
			pending = true;
			return;
		}
		const float fspp = (float)P.spp;
		if (P.albedo) {
			P.albedo[3 * out + 0] = ax / fspp;
			P.albedo[3 * out + 1] = ay / fspp;
			P.albedo[3 * out + 2] = az / fspp;
		}
		if (P.normal) {
			P.normal[3 * out + 0] = nx / fspp;
			P.normal[3 * out + 1] = ny / fspp;
			P.normal[3 * out + 2] = nz / fspp;
		}
		if (P.depth)
			P.depth[out] = hits ? tsum / (float)hits : kVeryFar;
		live = false;
	};

	QueryFeed feed;
	feed.init(n);
	bool exhausted = (n == 0);
	for (;;) {
		// ---- new pixels for free lanes ----
		const unsigned long long idleMask = __ballot(!live);
		const uint32_t nIdle = (uint32_t)__popcll(idleMask);
		if (!exhausted && nIdle >= kQueryRefillMinIdle) {
			const uint32_t rank = (uint32_t)__popcll(idleMask & below);
			uint32_t got = 0;
			bool fed = false;
			while (got < nIdle) {
				if (feed.next == feed.end && !feed.draw(kernarg_view<AovParams>().ticket, n, lane)) {
					exhausted = true;
					break;
				}
				const uint32_t avail = feed.end - feed.next, room = nIdle - got;
				const uint32_t take = avail < room ? avail : room;
				if (!live && rank >= got && rank < got + take) {
					pixel = feed.next + (rank - got);
					fed = true;
				}
				feed.next += take;
				got += take;
			}
			if (fed) {
				live = pending = true;
				s = hits = 0;
				ax = ay = az = nx = ny = nz = tsum = 0.f;
			}
		}
		// ---- the next sample of every pixel that waits for one; samples that cannot enter the tree finish here ----
		while (pending) {
			const AovParams& P = kernarg_view<AovParams>();
			const uint32_t index = s * P.nPixels + pixel; // the ticket of a render's first wavefront from an empty queue
			uint32_t seed = camera_seed(P, index);
			const int x = (int)(index % P.W);
			const int yl = (int)((index / P.W) % P.localRows);
			const int y = yl * (int)P.nranks + (int)P.rank;
			const CameraRay cr = camera_lens(P, seed, camera_focus(P, seed, x, y), ld3(P.camPos), ld3(P.camRight), ld3(P.camUp));
			const RayConst nr = make_ray(cr.origin, cr.direction);
			rox = nr.o.x, roy = nr.o.y, roz = nr.o.z, rdx = nr.d.x, rdy = nr.d.y, rdz = nr.d.z, rix = nr.inv.x, riy = nr.inv.y, riz = nr.inv.z;
			regular = ray_is_regular(nr);
			dist = kVeryFar;
			prim = -1;
			sphere = -1;
			hitTri = false;
#pragma unroll
			for (int k = TYR_NUM_SPHERES; k--;) { // kernel.cu:130-135
				const float t = sphere_intersect(P.spheres[k], nr.o, nr.d);
				if (t && t < dist) {
					dist = t;
					sphere = k;
				}
			}
			ref = root_ref(sc, nr, dist);
			if (ref != kRefDone) {
				ref = sc.quadRootRef;
				st.reset();
				pending = false;
			} else {
				pending = false;
				sample_done(); // a sphere or the sky: may ask for the pixel's next sample
			}
		}
		// mostly pixels that ended at once: top the wave up again first
		if (!exhausted && (uint32_t)__popcll(__ballot(live)) < kQueryMinTraversing && (uint32_t)__popcll(__ballot(!live)) >= kQueryRefillMinIdle)
			continue;
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
				// lanes that could start work: a finished sample (its pixel's next one or a new pixel), a free lane while pixels remain
				const bool canRefill = (uint32_t)__popcll(__ballot(live ? ref == kRefDone : !exhausted)) >= kQueryRefillMinIdle;
				if (anyLeaf || canRefill)
					break;
			}
			if (ref == kRefPop) {
				uint32_t pr;
				float pt;
				if (st.pop(pr, pt)) {
					if (pt < dist) // the pop-time half of Bbox.h:61
						ref = pr;
				} else {
					ref = kRefDone;
				}
			}
			if ((int)ref >= 0) {
				const QuadHits q = allRegular ? test_quad<true, true, true>(sc.quads, ref, r, dist, stagedNodes, nStaged) : test_quad<false, true, true>(sc.quads, ref, r, dist, stagedNodes, nStaged);
				const lanemask any01 = q.hit[0] | q.hit[1], any012 = any01 | q.hit[2];
				st.push3(q.hit[3] & any012, q.ref[3], q.t[3], q.hit[2] & any01, q.ref[2], q.t[2], q.hit[1] & q.hit[0], q.ref[1], q.t[1]);
				ref = lane_in(q.hit[0]) ? q.ref[0] : lane_in(q.hit[1]) ? q.ref[1] : lane_in(q.hit[2]) ? q.ref[2] : lane_in(q.hit[3]) ? q.ref[3] : kRefPop;
			}
		}
		// ---- leaves: bvh.h:129-140, primitives in array order ----
		if (q_is_leaf(ref)) {
			const uint32_t off = ref & (kMaxPrimOffset - 1);
			const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
			TriData tri = triangle_load(sc.tris, off);
			for (uint32_t i = 0; i < cnt; ++i) {
				const TriData cur = tri;
				if (i + 1 < cnt)
					tri = triangle_load(sc.tris, off + i + 1);
				const float t = triangle_test(cur, r);
				if (t > kEpsilon && t < dist && ((dist - t) > kEpsilon)) { // bvh.h:133-137
					prim = (int)(off + i);
					dist = t;
					hitTri = true;
				}
			}
			ref = kRefPop;
		}
		if (live && !pending && ref == kRefDone)
			sample_done();
	}
	if (__ballot(overflow) != 0ull && lane == 0)
		atomicOr(kernarg_view<AovParams>().error, kQueryErrStackOverflow);
}

// ---- specular-chain guides (tyr_render_aov_chain) ---------------------------------------------------------------------
// k_render_aov's loop with one more way for a traced ray to end: on a SPEC or REFR surface, while fewer than maxChain bounces
// have been followed, the sample goes on as a new ray -- shade's reflect (shade.hip TYR_SPEC) or its refracted branch, reflect
// only on total internal reflection (shade.hip TYR_REFR without the Fresnel draw and without the absorption) -- and re-enters
// the refill path below exactly as a fresh camera ray does: the spheres, the root box, then the tree.  The lane keeps its
// pixel; the throughput T, the summed length L and the bounce count k travel with the sample.  The guides are those of the
// surface the chain ends on: albedo T * colour, its face-forwarded normal, depth L.  A kernel of its own, so that
// k_render_aov's code stays what it was.  Four blocks per CU, not k_render_aov's five: the chain's state and the surface
// arithmetic of a continuation need 103 VGPRs, and at 96 the compiler spills (DESIGN.md "Specular-chain guides": with
// max_chain 0 the fourth wave costs nothing that can be measured).
__global__ void __launch_bounds__(kBlock, 4) k_render_chain(const AovChainParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.a.scene;
	const uint32_t nStaged = sc.nStaged;
	for (uint32_t i = threadIdx.x; i < 7 * nStaged; i += kBlock) {
		const uint32_t v = i / nStaged, k = i - v * nStaged;
		stagedNodes[v * kStagedNodes + k] = sc.quads[8 * k + v];
	}
	__syncthreads();
	const uint32_t lane = lane_id();
	const unsigned long long below = (1ull << lane) - 1ull;
	const uint32_t n = P0.a.nPixels;

	// the ray in flight: a camera ray or a continuation of one
	float rox = 0.f, roy = 0.f, roz = 0.f, rdx = 0.f, rdy = 0.f, rdz = 0.f, rix = 0.f, riy = 0.f, riz = 0.f;
	bool regular = true;
	float dist = 0.f;
	uint32_t ref = kRefDone;
	int prim = -1, sphere = -1;
	bool hitTri = false, overflow = false;
	// its sample: throughput, summed length, bounces followed
	float tx = 1.f, ty = 1.f, tz = 1.f, len = 0.f;
	uint32_t bounces = 0;
	// the pixel: live = owned by this lane, pending = a ray is to be started (onward: the continuation in ro / rd, else the
	// next sample's camera ray)
	uint32_t pixel = 0, s = 0, hits = 0, firstHits = 0;
	bool live = false, pending = false, onward = false;
	float ax = 0.f, ay = 0.f, az = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, tsum = 0.f, firstSum = 0.f;

	// the traced ray into its sample: the chain goes on, or the sample ends here and goes into the pixel's sums
	auto ray_done = [&]() {
		const AovChainParams& P = kernarg_view<AovChainParams>();
		const bool hit = hitTri || sphere >= 0;
		f3 alb = mk3(0.f, 0.f, 0.f), nrm = mk3(0.f, 0.f, 0.f); // a miss adds +0 (the sums' order and signs stay fixed)
		const f3 d = mk3(rdx, rdy, rdz);
		// the pixel's place in the full frame (computed where it is needed: it is not worth registers across the shading)
		auto frame_index = [&]() {
			const uint32_t x = pixel % P.a.W, yl = pixel / P.a.W;
			return (size_t)(yl * P.a.nranks + P.a.rank) * P.a.W + x;
		};
		if (bounces == 0) { // the first segment: tyr_render_aov's ids and depth
			if (s == 0) {
				const size_t out = frame_index();
				if (P.a.prim)
					P.a.prim[out] = hitTri ? prim : (hit ? sphere : -1);
				if (P.a.geom)
					P.a.geom[out] = hitTri ? 1 : (hit ? 0 : -1);
			}
			if (hit) {
				firstSum = firstSum + dist;
				++firstHits;
			}
		}
		overflow = overflow || st.overflow;
		ref = kRefDone;
		if (hit) {
			int material = TYR_DIFF;
			f3 colour = mk3(1.f, 1.f, 1.f);
			if (hitTri) {
				const TriData td = triangle_load(sc.tris, (uint32_t)prim);
				nrm = normalize(cross(mk3(td.a.w, td.b.x, td.b.y), mk3(td.b.z, td.b.w, td.c.x))); // kernel.cu:380-383
				if (P.triMaterials) { // shade.hip, TYR_FLAG_TRIANGLE_MATERIALS: its range check admits SPEC and REFR either way
					const uint32_t m = __float_as_uint(td.c.y);
					material = m <= (uint32_t)TYR_PHONG ? (int)m : TYR_DIFF;
				}
				if (P.a.palette) { // Scene.cpp:44's `tempTriangle.color` (shade.hip, TYR_FLAG_TRIANGLE_COLORS)
					const float4 c = P.a.palette[2u * (__float_as_uint(td.c.z) & 255u)];
					colour = mk3(c.x, c.y, c.z);
				}
			} else {
				const tyr_sphere& object = P.a.spheres[sphere];
				const f3 at = mk3(rox, roy, roz) + d * dist; // kernel.cu:368
				nrm = (at - ld3(object.position)) / object.radius;
				material = object.refl;
				colour = ld3(object.color);
			}
			const bool outside = dot(nrm, d) < 0; // kernel.cu:386
			nrm = outside ? nrm : nrm * -1.f;
			len = len + dist;
			if ((material == TYR_SPEC || material == TYR_REFR) && bounces < P.maxChain) {
				f3 o = (mk3(rox, roy, roz) + d * dist) + nrm * kEpsilon, nd; // kernel.cu:368, 387
				if (material == TYR_SPEC) {
					tx = tx * colour.x, ty = ty * colour.y, tz = tz * colour.z;
					nd = reflect(d, nrm);
				} else { // kernel.cu:476-515; the refracted branch whenever there is one
					const float n1 = outside ? 1.2f : 1.0f;
					const float n2 = outside ? 1.0f : 1.2f;
					const float cosI = -dot(nrm, d);
					const float eta = n2 / n1;
					const float sinT2 = eta * eta * (1.0f - cosI * cosI);
					if (sinT2 > 1.0f) {
						nd = reflect(d, nrm);
					} else {
						o = o - (nrm * 2.f) * kEpsilon;
						const float cosT = sqrtf(1.0f - sinT2);
						nd = eta * d + (eta * cosI - cosT) * nrm;
					}
				}
				rox = o.x, roy = o.y, roz = o.z, rdx = nd.x, rdy = nd.y, rdz = nd.z;
				++bounces;
				pending = onward = true;
				return;
			}
			alb = mk3(tx, ty, tz) * colour;
			tsum = tsum + len;
			++hits;
		}
		ax = ax + alb.x, ay = ay + alb.y, az = az + alb.z;
		nx = nx + nrm.x, ny = ny + nrm.y, nz = nz + nrm.z;
		if (s == 0) { // sample 0's chain: its length, and where it ended
			const size_t out = frame_index();
			if (P.chain)
				P.chain[out] = (int32_t)bounces;
			if (P.endPrim)
				P.endPrim[out] = hitTri ? prim : (hit ? sphere : -1);
			if (P.endGeom)
				P.endGeom[out] = hitTri ? 1 : (hit ? 0 : -1);
			if (P.length0)
				P.length0[out] = hit ? len : kVeryFar;
		}
		if (++s < P.a.spp) {
			pending = true;
			return;
		}
		const float fspp = (float)P.a.spp;
		const size_t out = frame_index();
		if (P.a.albedo) {
			P.a.albedo[3 * out + 0] = ax / fspp;
			P.a.albedo[3 * out + 1] = ay / fspp;
			P.a.albedo[3 * out + 2] = az / fspp;
		}
		if (P.a.normal) {
			P.a.normal[3 * out + 0] = nx / fspp;
			P.a.normal[3 * out + 1] = ny / fspp;
			P.a.normal[3 * out + 2] = nz / fspp;
		}
		if (P.a.depth)
			P.a.depth[out] = hits ? tsum / (float)hits : kVeryFar;
		if (P.depthFirst)
			P.depthFirst[out] = firstHits ? firstSum / (float)firstHits : kVeryFar;
		live = false;
	};

	QueryFeed feed;
	feed.init(n);
	bool exhausted = (n == 0);
	for (;;) {
		// ---- new pixels for free lanes ----
		const unsigned long long idleMask = __ballot(!live);
		const uint32_t nIdle = (uint32_t)__popcll(idleMask);
		if (!exhausted && nIdle >= kQueryRefillMinIdle) {
			const uint32_t rank = (uint32_t)__popcll(idleMask & below);
			uint32_t got = 0;
			bool fed = false;
			while (got < nIdle) {
				if (feed.next == feed.end && !feed.draw(kernarg_view<AovChainParams>().a.ticket, n, lane)) {
					exhausted = true;
					break;
				}
				const uint32_t avail = feed.end - feed.next, room = nIdle - got;
				const uint32_t take = avail < room ? avail : room;
				if (!live && rank >= got && rank < got + take) {
					pixel = feed.next + (rank - got);
					fed = true;
				}
				feed.next += take;
				got += take;
			}
			if (fed) {
				live = pending = true;
				onward = false;
				s = hits = firstHits = 0;
				ax = ay = az = nx = ny = nz = tsum = firstSum = 0.f;
			}
		}
		// ---- the next ray of every pixel that waits for one; rays that cannot enter the tree finish here ----
		while (pending) {
			const AovParams& P = kernarg_view<AovChainParams>().a;
			if (!onward) { // the next sample's camera ray, as k_render_aov makes it
				const uint32_t index = s * P.nPixels + pixel;
				uint32_t seed = camera_seed(P, index);
				const int x = (int)(index % P.W);
				const int yl = (int)((index / P.W) % P.localRows);
				const int y = yl * (int)P.nranks + (int)P.rank;
				const CameraRay cr = camera_lens(P, seed, camera_focus(P, seed, x, y), ld3(P.camPos), ld3(P.camRight), ld3(P.camUp));
				rox = cr.origin.x, roy = cr.origin.y, roz = cr.origin.z, rdx = cr.direction.x, rdy = cr.direction.y, rdz = cr.direction.z;
				tx = ty = tz = 1.f;
				len = 0.f;
				bounces = 0;
			}
			onward = false;
			const RayConst nr = make_ray(mk3(rox, roy, roz), mk3(rdx, rdy, rdz));
			rix = nr.inv.x, riy = nr.inv.y, riz = nr.inv.z;
			regular = ray_is_regular(nr);
			dist = kVeryFar;
			prim = -1;
			sphere = -1;
			hitTri = false;
#pragma unroll
			for (int k = TYR_NUM_SPHERES; k--;) { // kernel.cu:130-135
				const float t = sphere_intersect(P.spheres[k], nr.o, nr.d);
				if (t && t < dist) {
					dist = t;
					sphere = k;
				}
			}
			ref = root_ref(sc, nr, dist);
			pending = false;
			if (ref != kRefDone) {
				ref = sc.quadRootRef;
				st.reset();
			} else {
				ray_done(); // a sphere or the sky: may ask for the chain's next ray or the pixel's next sample
			}
		}
		// mostly pixels that ended at once: top the wave up again first
		if (!exhausted && (uint32_t)__popcll(__ballot(live)) < kQueryMinTraversing && (uint32_t)__popcll(__ballot(!live)) >= kQueryRefillMinIdle)
			continue;
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
				// lanes that could start work: a finished ray (its chain's or pixel's next one, or a new pixel), a free lane while pixels remain
				const bool canRefill = (uint32_t)__popcll(__ballot(live ? ref == kRefDone : !exhausted)) >= kQueryRefillMinIdle;
				if (anyLeaf || canRefill)
					break;
			}
			if (ref == kRefPop) {
				uint32_t pr;
				float pt;
				if (st.pop(pr, pt)) {
					if (pt < dist) // the pop-time half of Bbox.h:61
						ref = pr;
				} else {
					ref = kRefDone;
				}
			}
			if ((int)ref >= 0) {
				const QuadHits q = allRegular ? test_quad<true, true, true>(sc.quads, ref, r, dist, stagedNodes, nStaged) : test_quad<false, true, true>(sc.quads, ref, r, dist, stagedNodes, nStaged);
				const lanemask any01 = q.hit[0] | q.hit[1], any012 = any01 | q.hit[2];
				st.push3(q.hit[3] & any012, q.ref[3], q.t[3], q.hit[2] & any01, q.ref[2], q.t[2], q.hit[1] & q.hit[0], q.ref[1], q.t[1]);
				ref = lane_in(q.hit[0]) ? q.ref[0] : lane_in(q.hit[1]) ? q.ref[1] : lane_in(q.hit[2]) ? q.ref[2] : lane_in(q.hit[3]) ? q.ref[3] : kRefPop;
			}
		}
		// ---- leaves: bvh.h:129-140, primitives in array order ----
		if (q_is_leaf(ref)) {
			const uint32_t off = ref & (kMaxPrimOffset - 1);
			const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
			TriData tri = triangle_load(sc.tris, off);
			for (uint32_t i = 0; i < cnt; ++i) {
				const TriData cur = tri;
				if (i + 1 < cnt)
					tri = triangle_load(sc.tris, off + i + 1);
				const float t = triangle_test(cur, r);
				if (t > kEpsilon && t < dist && ((dist - t) > kEpsilon)) { // bvh.h:133-137
					prim = (int)(off + i);
					dist = t;
					hitTri = true;
				}
			}
			ref = kRefPop;
		}
		if (live && !pending && ref == kRefDone)
			ray_done();
	}
	if (__ballot(overflow) != 0ull && lane == 0)
		atomicOr(kernarg_view<AovChainParams>().a.error, kQueryErrStackOverflow);
}

void launch_aov(const AovParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	const Tuning t{}; // the occupancy query's answer, as the queries' launches
	hipLaunchKernelGGL(k_render_aov, dim3(persistent_blocks(k_render_aov, P.nPixels, t, numCUs, lc.perCU[kLcQuery][4])), dim3(kBlock), 0, stream, P);
}

void launch_aov_chain(const AovChainParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	const Tuning t{};
	hipLaunchKernelGGL(k_render_chain, dim3(persistent_blocks(k_render_chain, P.a.nPixels, t, numCUs, lc.perCU[kLcQuery][5])), dim3(kBlock), 0, stream, P);
}

} // namespace tyr
