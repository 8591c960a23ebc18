// occlusion.hip -- batched ambient-occlusion queries on the uploaded scene (tyr_query_occlusion, host/occlusion.cpp): for every
// point of a caller's batch, `samples` cosine-weighted any-hit rays over the hemisphere of its normal, made in registers and
// answered as one integer per point (include/tyr_c.h "Occlusion queries" is the contract).
//
//   k_occlusion       the any-hit loop of hip/query_common.hpp (query_body<true, SPHERES> of hip/query.hip) with a work item
//                     that is a (point, sample) pair instead of a caller's ray: item = point * samples + sample, sample
//                     fastest, so that a wave's lanes share a point or neighbouring points and the rays of a chunk start
//                     together.  An unblocked ray adds 1 to its point's count and sets its bit of the point's mask words:
//                     integer atomics, whose result does not depend on their order.
//   k_occlusion_bent  one thread per point, behind the first kernel: the sum of the visible samples' directions in sample
//                     order, the directions made again by the same device function -- no float atomics anywhere.
#include "device_common.hpp"
#include "occlusion.hpp"
#include "query_common.hpp"

namespace tyr {

namespace {

// what a point's samples share: the origin of its rays and the basis about its unit normal
struct OcclFrame {
	f3 o, w, u, v;
	bool valid; // the point and the normal are finite and the normal has a length
};

__device__ __forceinline__ OcclFrame occl_frame(f3 p, f3 nrm, float bias) {
	OcclFrame f;
	const float nn = dot(nrm, nrm);
	f.valid = finite3(p.x, p.y, p.z) && finite3(nrm.x, nrm.y, nrm.z) && fabsf(nn) < __builtin_inff() && nn > 0.f;
	f.w = normalize(nrm);
	f.o = p + f.w * bias;
	orthonormal_basis_naive(f.w, f.u, f.v);
	return f;
}

__device__ __forceinline__ uint32_t occl_hash(uint32_t x) {
	x ^= x >> 16;
	x *= 0x7feb352du;
	x ^= x >> 15;
	x *= 0x846ca68bu;
	x ^= x >> 16;
	return x;
}

// sample s of point i (its index in the caller's batch): shade's DIFF bounce (hip/shade.hip, kernel.cu:446-452) about f.w
__device__ __forceinline__ f3 occl_direction(const OcclFrame& f, uint32_t seed, uint32_t i, uint32_t s) {
	uint32_t state = occl_hash(occl_hash(seed ^ i) + s);
	const float u1 = rng_float(state);
	const float u2 = rng_float(state);
	const float r1 = (2.f * kPi) * u1;
	const float r2s = sqrtf(u2);
	float s1, c1;
	dm::sincosf_det(r1, s1, c1);
	return normalize((f.u * c1) * r2s + (f.v * s1) * r2s + f.w * sqrtf(1 - u2));
}

} // namespace

template <bool SPHERES>
__global__ void __launch_bounds__(kBlock, 5) k_occlusion(const OcclusionParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, false)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();

	QueryRay q = {};
	q.ref = kRefDone;
	uint32_t point = 0, sample = 0; // the item: the point's index in the caller's batch and the sample
	bool live = false, overflow = false;

	// a finished ray: an unblocked one counts for its point (the return-less atomics: nothing reads the old values)
	auto finish = [&]() {
		if (!q.occluded) {
			const OcclusionParams& P = kernarg_view<OcclusionParams>(); // (read where it lies: not held in scalar registers through the descent)
			atomicAdd(&P.visible[point], 1u);
			if (P.mask) {
				const size_t words = (P.samples + 31u) >> 5;
				atomicOr(&P.mask[point * words + (sample >> 5)], 1u << (sample & 31u));
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
		const uint32_t fresh = feed.refill(live, lane, [] { return kernarg_view<OcclusionParams>().ticket; });
		if (fresh != kNoItem) {
			const OcclusionParams& P = kernarg_view<OcclusionParams>();
			const uint32_t local = fresh / P.samples;
			sample = fresh - local * P.samples;
			point = P.first + local;
			const size_t p3 = 3 * (size_t)point;
			const f3 pt = mk3(P.points[p3 + 0], P.points[p3 + 1], P.points[p3 + 2]);
			const OcclFrame f = occl_frame(pt, mk3(P.normals[p3 + 0], P.normals[p3 + 1], P.normals[p3 + 2]), P.bias);
			const f3 d = f.valid ? occl_direction(f, P.seed, point, sample) : mk3(0.f, 0.f, 0.f);
			const f3 o = f.valid ? f.o : pt;
			if (P.direction) {
				const size_t d3 = 3 * ((size_t)point * P.samples + sample);
				P.direction[d3 + 0] = d.x, P.direction[d3 + 1] = d.y, P.direction[d3 + 2] = d.z;
			}
			if (P.origin && sample == 0u)
				P.origin[p3 + 0] = o.x, P.origin[p3 + 1] = o.y, P.origin[p3 + 2] = o.z;
			if (f.valid) { // (an invalid point's lanes end here: they never enter the tree and never touch the atomics)
				const float tmax = P.maxDist ? P.maxDist[point] : kVeryFar;
				const RayConst nr = make_ray(o, d);
				q.start(nr, tmax);
				st.reset();
				live = true;
				// as tyr_query_any: a ray with a NaN or infinite component is a miss (and never enters a box)
				const bool isRay = finite3(o.x, o.y, o.z) && finite3(d.x, d.y, d.z);
				if (SPHERES && isRay) {
#pragma unroll
					for (int s = TYR_NUM_SPHERES; s--;) { // kernel.cu:168-172
						const float t = sphere_intersect(P.spheres[s], nr.o, nr.d);
						q.occluded = q.occluded || (t && (t + kEpsilon) < tmax);
					}
				}
				q.ref = (isRay && !q.occluded) ? root_ref(sc, nr, q.dist) : kRefDone;
				if (q.ref != kRefDone)
					q.ref = sc.quadRootRef;
				if (q.ref == kRefDone)
					finish(); // missed the root box, blocked by a sphere, or not a ray
			}
		}
		if (feed.top_up(live)) // mostly rays that ended at once
			continue;
		if (__ballot(live) == 0ull) {
			if (feed.exhausted)
				break;
			continue;
		}
		// lanes that could start work: free ones and finished rays, while items remain
		q_traverse<true>(sc, st, stagedNodes, q, live, [&](uint32_t ref) { return !feed.exhausted && (uint32_t)__popcll(__ballot(!live || ref == kRefDone)) >= kQueryRefillMinIdle; });
		if (live && q.ref == kRefDone)
			finish();
	}
	q_report_overflow(overflow, lane, kernarg_view<OcclusionParams>().error);
}

// bent[i] = ((0 + d_s0) + d_s1) + ... over the set bits of the point's mask words, ascending
__global__ void __launch_bounds__(kBlock) k_occlusion_bent(const OcclusionBentParams P) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= P.nPoints)
		return;
	const size_t p3 = 3 * (size_t)i;
	const size_t words = (P.samples + 31u) >> 5;
	const uint32_t* row = P.mask + i * words;
	f3 sum = mk3(0.f, 0.f, 0.f);
	OcclFrame f;
	bool haveFrame = false;
	for (uint32_t w = 0; w < (uint32_t)words; ++w) {
		uint32_t bitsLeft = row[w];
		while (bitsLeft) {
			if (!haveFrame) { // (a point without a visible sample -- an invalid one among them -- reads nothing more)
				f = occl_frame(mk3(P.points[p3 + 0], P.points[p3 + 1], P.points[p3 + 2]), mk3(P.normals[p3 + 0], P.normals[p3 + 1], P.normals[p3 + 2]), P.bias);
				haveFrame = true;
			}
			const uint32_t b = (uint32_t)__builtin_ctz(bitsLeft);
			bitsLeft &= bitsLeft - 1u;
			sum = sum + occl_direction(f, P.seed, i, 32u * w + b);
		}
	}
	P.bent[p3 + 0] = sum.x, P.bent[p3 + 1] = sum.y, P.bent[p3 + 2] = sum.z;
}

void launch_occlusion(const OcclusionParams& P, bool spheres, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(spheres ? k_occlusion<true> : k_occlusion<false>, P, P.n, numCUs, lc.perCU[kLcOcclusion][spheres ? 1 : 0], stream);
}

void launch_occlusion_bent(const OcclusionBentParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(k_occlusion_bent, dim3(blocks_for(P.nPoints)), dim3(kBlock), 0, stream, P);
}

} // namespace tyr
