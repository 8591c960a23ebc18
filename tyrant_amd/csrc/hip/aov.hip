// aov.hip -- guide buffers for denoisers: the first-hit pass (tyr_render_aov) and the specular-chain pass
// (tyr_render_aov_chain), host/aov.cpp.  Per pixel the average albedo and shading normal of spp camera rays, their average
// hit distance, and sample 0's identity; the chain pass takes them where a sample's deterministic specular chain ends.
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
// pixel whose every sample does: neither holds a traversal lane.  Otherwise the loop is the queries', from
// hip/query_common.hpp: the feed, the descent, the leaves.  Both passes are one body, aov_body<CHAIN>, behind two kernels
// with their own __launch_bounds__.
#include "aov.hpp"
#include "device_common.hpp"
#include "query.hpp"
#include "query_common.hpp"

namespace tyr {

namespace {

// a pass's kernel argument, and the first-hit pass's part of it
template <bool CHAIN>
using AovArgs = std::conditional_t<CHAIN, AovChainParams, AovParams>;
__device__ __forceinline__ const AovParams& first_hit_args(const AovParams& p) { return p; }
__device__ __forceinline__ const AovParams& first_hit_args(const AovChainParams& p) { return p.a; }

// what a lane of the chain pass carries beyond the first-hit pass's state
struct ChainState {
	float tx = 1.f, ty = 1.f, tz = 1.f, len = 0.f; // the sample: throughput, summed length
	uint32_t bounces = 0;                          // ... and bounces followed
	bool onward = false;                           // the ray to be started is the continuation in the ray's origin and direction
	float firstSum = 0.f;                          // the pixel: first-segment depth sum and hit count
	uint32_t firstHits = 0;
};
struct NoChainState {};

} // namespace

// CHAIN = false: tyr_render_aov.  CHAIN = true: tyr_render_aov_chain -- the same loop with one more way for a traced ray to
// end: on a SPEC or REFR surface, while fewer than maxChain bounces have been followed, the sample goes on as a new ray --
// shade's reflect (shade.hip TYR_SPEC) or its refracted branch, reflect only on total internal reflection (shade.hip TYR_REFR
// without the Fresnel draw and without the absorption) -- and re-enters the refill path exactly as a fresh camera ray does:
// the spheres, the root box, then the tree.  The lane keeps its pixel; the throughput T, the summed length L and the bounce
// count travel with the sample.  The guides are those of the surface the chain ends on: albedo T * colour, its face-forwarded
// normal, depth L.  The chain's state is a ChainState that the first-hit pass does not have, so every use of it stands under `if constexpr (CHAIN)`.
template <bool CHAIN>
__device__ __forceinline__ void aov_body(const AovParams& P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	// the ray in flight: a camera ray or (CHAIN) a continuation of one
	QueryRay q = {};
	q.ref = kRefDone;
	bool overflow = false;
	std::conditional_t<CHAIN, ChainState, NoChainState> c;
	// the pixel: live = owned by this lane, pending = a ray is to be started (the next sample's camera ray, or c.onward)
	uint32_t pixel = 0, s = 0, hits = 0;
	bool live = false, pending = false;
	float ax = 0.f, ay = 0.f, az = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, tsum = 0.f;

	// the traced ray into its sample: (CHAIN) the chain goes on, or the sample ends here and goes into the pixel's sums; the
	// pixel's outputs once its last sample is in
	auto ray_done = [&]() {
		const AovArgs<CHAIN>& PC = kernarg_view<AovArgs<CHAIN>>();
		const AovParams& P = first_hit_args(PC);
		const bool hit = q.hitTri || q.sphere >= 0;
		const int id = q.hitTri ? q.prim : (hit ? q.sphere : -1), geom = q.hitTri ? 1 : (hit ? 0 : -1); // the query convention: geom 0 sphere, 1 triangle, -1 miss
		f3 alb = mk3(0.f, 0.f, 0.f), nrm = mk3(0.f, 0.f, 0.f); // a miss adds +0 (the sums' order and signs stay fixed)
		const f3 d = mk3(q.dx, q.dy, q.dz);
		// the pixel's place in the full frame (computed where it is needed: it is not worth registers across the shading)
		auto frame_index = [&]() {
			const uint32_t x = pixel % P.W, yl = pixel / P.W;
			return (size_t)(yl * P.nranks + P.rank) * P.W + x;
		};
		bool first = true;
		if constexpr (CHAIN)
			first = c.bounces == 0;
		if (first) { // the first segment: sample 0's identity, and the chain's first-hit depth
			if (s == 0) {
				const size_t out = frame_index();
				if (P.prim)
					P.prim[out] = id;
				if (P.geom)
					P.geom[out] = geom;
			}
			if constexpr (CHAIN) {
				if (hit) {
					c.firstSum = c.firstSum + q.dist;
					++c.firstHits;
				}
			}
		}
		overflow = overflow || st.overflow;
		q.ref = kRefDone;
		if (hit) {
			int material = TYR_DIFF;
			f3 colour = mk3(1.f, 1.f, 1.f);
			if (q.hitTri) {
				const TriData td = triangle_load(sc.tris, (uint32_t)q.prim);
				nrm = normalize(cross(mk3(td.a.w, td.b.x, td.b.y), mk3(td.b.z, td.b.w, td.c.x))); // kernel.cu:380-383
				if constexpr (CHAIN) {
					if (PC.triMaterials) { // shade.hip, TYR_FLAG_TRIANGLE_MATERIALS: its range check admits SPEC and REFR either way
						const uint32_t m = __float_as_uint(td.c.y);
						material = m <= (uint32_t)TYR_PHONG ? (int)m : TYR_DIFF;
					}
				}
				if (P.palette) { // Scene.cpp:44's `tempTriangle.color` (shade.hip, TYR_FLAG_TRIANGLE_COLORS)
					const float4 c = P.palette[2u * (__float_as_uint(td.c.z) & 255u)];
					colour = mk3(c.x, c.y, c.z);
				}
			} else {
				const tyr_sphere& object = P.spheres[q.sphere];
				const f3 at = mk3(q.ox, q.oy, q.oz) + d * q.dist; // kernel.cu:368
				nrm = (at - ld3(object.position)) / object.radius;
				material = object.refl;
				colour = ld3(object.color);
			}
			const bool outside = dot(nrm, d) < 0; // kernel.cu:386
			nrm = outside ? nrm : nrm * -1.f;
			if constexpr (CHAIN) {
				c.len = c.len + q.dist;
				if ((material == TYR_SPEC || material == TYR_REFR) && c.bounces < PC.maxChain) {
					f3 o = (mk3(q.ox, q.oy, q.oz) + d * q.dist) + nrm * kEpsilon, nd; // kernel.cu:368, 387
					if (material == TYR_SPEC) {
						c.tx = c.tx * colour.x, c.ty = c.ty * colour.y, c.tz = c.tz * colour.z;
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
					q.ox = o.x, q.oy = o.y, q.oz = o.z, q.dx = nd.x, q.dy = nd.y, q.dz = nd.z;
					++c.bounces;
					pending = c.onward = true;
					return;
				}
				alb = mk3(c.tx, c.ty, c.tz) * colour;
				tsum = tsum + c.len;
			} else {
				alb = colour;
				tsum = tsum + q.dist;
			}
			++hits;
		}
		ax = ax + alb.x, ay = ay + alb.y, az = az + alb.z;
		nx = nx + nrm.x, ny = ny + nrm.y, nz = nz + nrm.z;
		if constexpr (CHAIN) {
			if (s == 0) { // sample 0's chain: its length, and where it ended
				const size_t out = frame_index();
				if (PC.chain)
					PC.chain[out] = (int32_t)c.bounces;
				if (PC.endPrim)
					PC.endPrim[out] = id;
				if (PC.endGeom)
					PC.endGeom[out] = geom;
				if (PC.length0)
					PC.length0[out] = hit ? c.len : kVeryFar;
			}
		}
		if (++s < P.spp) {
			pending = true;
			return;
		}
		const float fspp = (float)P.spp;
		const size_t out = frame_index();
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
		if constexpr (CHAIN) {
			if (PC.depthFirst)
				PC.depthFirst[out] = c.firstHits ? c.firstSum / (float)c.firstHits : kVeryFar;
		}
		live = false;
	};

	QueryFeed feed;
	feed.init(P0.nPixels);
	for (;;) {
		// ---- new pixels for free lanes ----
		const uint32_t fresh = feed.refill(live, lane, [] { return first_hit_args(kernarg_view<AovArgs<CHAIN>>()).ticket; });
		if (fresh != kNoItem) {
			pixel = fresh;
			live = pending = true;
			s = hits = 0;
			ax = ay = az = nx = ny = nz = tsum = 0.f;
			if constexpr (CHAIN) {
				c.onward = false;
				c.firstHits = 0;
				c.firstSum = 0.f;
			}
		}
		// ---- the next ray of every pixel that waits for one; rays that cannot enter the tree finish here ----
		while (pending) {
			const AovParams& P = first_hit_args(kernarg_view<AovArgs<CHAIN>>());
			f3 o = mk3(q.ox, q.oy, q.oz), d = mk3(q.dx, q.dy, q.dz);
			bool camera = true;
			if constexpr (CHAIN) {
				camera = !c.onward;
				c.onward = false;
			}
			if (camera) { // the next sample's camera ray
				const uint32_t index = s * P.nPixels + pixel; // the ticket of a render's first wavefront from an empty queue
				uint32_t seed = camera_seed(P, index);
				const int x = (int)(index % P.W);
				const int yl = (int)((index / P.W) % P.localRows);
				const int y = yl * (int)P.nranks + (int)P.rank;
				const CameraRay cr = camera_lens(P, seed, camera_focus(P, seed, x, y), ld3(P.camPos), ld3(P.camRight), ld3(P.camUp));
				o = cr.origin, d = cr.direction;
				if constexpr (CHAIN) {
					c.tx = c.ty = c.tz = 1.f;
					c.len = 0.f;
					c.bounces = 0;
				}
			}
			const RayConst nr = make_ray(o, d);
			q.start(nr, kVeryFar);
			q_spheres_closest(P.spheres, nr, q);
			q.ref = root_ref(sc, nr, q.dist);
			pending = false;
			if (q.ref != kRefDone) {
				q.ref = sc.quadRootRef;
				st.reset();
			} else {
				ray_done(); // a sphere or the sky: may ask for the chain's next ray or the pixel's next sample
			}
		}
		if (feed.top_up(live)) // mostly pixels that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: a finished ray (its chain's or pixel's next one, or a new pixel), a free lane while pixels remain
		q_traverse<false>(sc, st, stagedNodes, q, live, [&](uint32_t ref) { return (uint32_t)__popcll(__ballot(live ? ref == kRefDone : !feed.exhausted)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			ray_done();
	}
	q_report_overflow(overflow, lane, first_hit_args(kernarg_view<AovArgs<CHAIN>>()).error);
}

// Five blocks per CU for the first-hit pass, four for the chain: its state and the surface arithmetic of a continuation need
// 103 VGPRs, and at 96 the compiler spills (DESIGN.md "Specular-chain guides": with max_chain 0 the fourth wave costs nothing
// that can be measured).
__global__ void __launch_bounds__(kBlock, 5) k_render_aov(const AovParams P) { aov_body<false>(P); }
__global__ void __launch_bounds__(kBlock, 4) k_render_chain(const AovChainParams P) { aov_body<true>(P.a); }

void launch_aov(const AovParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_render_aov, P, P.nPixels, numCUs, lc.perCU[kLcQuery][4], stream);
}

void launch_aov_chain(const AovChainParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_render_chain, P, P.a.nPixels, numCUs, lc.perCU[kLcQuery][5], stream);
}

} // namespace tyr
