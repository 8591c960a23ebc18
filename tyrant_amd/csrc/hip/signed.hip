// signed.hip -- signed distances to the uploaded scene (include/tyr_c.h "Signed-distance queries"): tyr_query_signed for the
// caller's points and tyr_bake_sdf for a regular grid whose voxel centres are made here (host/signed.cpp).  A signed distance is
// the join of two contracts that exist: the closest point of tyr_query_nearest (hip/nearest_common.hpp: the value of a pair, the
// pruning key, the keyed descent) and the winding number of tyr_query_winding (hip/winding_walk.hpp: the stackless walk of the
// moment tree).  Nothing here restates either: both are the other units' texts, so each word is the one those queries answer.
//
// k_query_signed   one point to a lane on a persistent grid.  A wave takes 64 consecutive points, descends for all of them until
//                  the last is done, and then walks the moment tree for all of them together: the walk -- hundreds of binary64
//                  trips per point -- is the larger half of the work and runs with every lane.  (Refilled as k_query_nearest
//                  is, with the walk for the lanes that wait at each refill, a quarter of the lanes walk at a time: 3.5 times
//                  the time of the two separate queries, DESIGN.md "Signed distance".)
// k_sdf_bricks     the bake's first launch: the same loop with brick centres as items and reach as the bound.  A brick with a
//                  triangle within reach is near and goes to the device list; a brick without is far: its lane walks for the
//                  centre's side and the wave fills the brick's voxels, a lane to a voxel.
// k_sdf_voxels     the bake's second launch: a wave takes one near brick at a time from the list, lane = voxel
//                  (x = lane & 3, y = (lane >> 2) & 3, z = lane >> 4), 64 descents and 64 walks side by side.
// Voxel and brick centres are origin + cell * ((float)i + 0.5f) and origin + cell * (float)(4 b + 2), each operation rounded to
// binary32 (no fma: the pragma below, and -ffp-contract=off).
#include "signed.hpp"

#include "nearest_common.hpp"
#include "winding_walk.hpp"

#pragma clang fp contract(off)

namespace tyr {

namespace {

// the point a lane has in flight and what its descent has found so far (hip/nearest.hip's)
struct SignedLane {
	float px, py, pz;
	float c1;     // kSlackCoord * max |p_k|
	float best;   // the smallest value so far; bound2 until a triangle is accepted
	int prim;     // its triangle, -1: none
	uint32_t ref; // the lane's state
};

__device__ __forceinline__ void lane_start(SignedLane& q, const DevScene& sc, float px, float py, float pz, float md, bool valid) {
	q.px = px, q.py = py, q.pz = pz;
	q.best = valid ? md * md : kInf;
	q.prim = -1;
	q.c1 = kSlackCoord * __builtin_fmaxf(__builtin_fmaxf(fabsf(px), fabsf(py)), __builtin_fmaxf(fabsf(pz), 1e-30f));
	q.ref = (valid && sc.rootRef != kRefDone) ? sc.quadRootRef : kRefDone; // (rootRef == kRefDone: a scene without triangles)
}

// a triangle of a reached leaf: the smallest pair (value, index) so far stays
__device__ __forceinline__ void lane_take(SignedLane& q, float F, int prim) {
	if (F < q.best || (F == q.best && prim < q.prim)) {
		q.best = F;
		q.prim = prim;
	}
}

// tyr_query_winding's w of a point with finite coordinates
__device__ __forceinline__ float winding_of(const WindingNode* wnodes, const float4* tris, int32_t nWNodes, float accuracy, float px, float py, float pz) {
	const d3 q = mk3d((double)px, (double)py, (double)pz);
	const double B2 = (double)accuracy * (double)accuracy;
	const WindingSum s = winding_sum(wnodes, tris, (uint32_t)nWNodes, q, B2);
	return (float)(s.sum * dm::kInv4Pi);
}

// What tyr_query_signed answers for a point whose descent ended with `prim` (include/tyr_c.h "Signed-distance queries",
// operation by operation).  GRADIENT: the gradient is wanted.
struct SignedAnswer {
	float sd, w;
	int prim;
	f3 point, gradient;
};
template <bool GRADIENT>
__device__ __forceinline__ SignedAnswer signed_answer(const float4* tris, const WindingNode* wnodes, int32_t nWNodes, float accuracy, f3 p, bool valid, float md, int prim) {
	SignedAnswer o;
	o.sd = o.w = __uint_as_float(0x7fc00000u);
	o.prim = -1;
	o.point = p;
	o.gradient = mk3(0.f, 0.f, 0.f);
	if (!valid)
		return o;
	o.w = winding_of(wnodes, tris, nWNodes, accuracy, p.x, p.y, p.z);
	const bool inside = o.w > 0.5f;
	float m = md;
	if (prim >= 0) {
		const TriData td = triangle_load(tris, (uint32_t)prim);
		const NearestValue v = nearest_value<true>(td, p); // the winner's operations once more: tyr_query_nearest's dist2 and point
		m = (float)__builtin_sqrt((double)v.F);            // the correctly rounded binary32 root
		o.prim = prim;
		o.point = v.c;
		if (GRADIENT) {
			d3 g = mk3d((double)p.x - (double)v.c.x, (double)p.y - (double)v.c.y, (double)p.z - (double)v.c.z);
			const bool away = v.F > 0.f && (g.x != 0.0 || g.y != 0.0 || g.z != 0.0);
			if (away) {
				if (inside)
					g = mk3d(-g.x, -g.y, -g.z);
			} else {
				g = crossd(mk3d((double)td.a.w, (double)td.b.x, (double)td.b.y), mk3d((double)td.b.z, (double)td.b.w, (double)td.c.x));
			}
			const double len = __builtin_sqrt((g.x * g.x + g.y * g.y) + g.z * g.z);
			if (len > 0.0)
				o.gradient = mk3((float)(g.x / len), (float)(g.y / len), (float)(g.z / len));
		}
	}
	o.sd = inside ? -m : m;
	return o;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float axis_centre(float origin, float cell, uint32_t i) { return origin + cell * ((float)i + 0.5f); }
__device__ __forceinline__ float brick_centre(float origin, float cell, uint32_t b) { return origin + cell * (float)(4u * b + 2u); }

struct BrickAt {
	uint32_t bi, bj, bk;
};
__device__ __forceinline__ BrickAt brick_at(const SdfParams& P, uint32_t b) {
	BrickAt o;
	o.bi = b % P.bricks[0];
	const uint32_t r = b / P.bricks[0];
	o.bj = r % P.bricks[1];
	o.bk = r / P.bricks[1];
	return o;
}
// the voxel this lane has of brick `at`; false outside the grid
struct VoxelAt {
	uint32_t x, y, z;
	size_t index;
	bool inGrid;
};
__device__ __forceinline__ VoxelAt voxel_at(const SdfParams& P, const BrickAt& at, uint32_t lane) {
	VoxelAt o;
	o.x = 4u * at.bi + (lane & 3u), o.y = 4u * at.bj + ((lane >> 2) & 3u), o.z = 4u * at.bk + (lane >> 4);
	o.inGrid = o.x < P.dims[0] && o.y < P.dims[1] && o.z < P.dims[2];
	o.index = ((size_t)o.z * P.dims[1] + o.y) * P.dims[0] + o.x;
	return o;
}

// ---- what the two item kinds of the shared loop are ----------------------------------------------------------------------------
// load(): an item's point, bound and validity.  flush(): called by the whole wave; lanes with `mine` set hold an item whose
// descent ended with `prim` and answer it.
struct PointItems {
	typedef SignedParams Params;
	static __device__ __forceinline__ void load(const Params& P, uint32_t item, float& px, float& py, float& pz, float& md, bool& valid) {
		const size_t i3 = 3 * (size_t)item;
		px = P.points[i3 + 0], py = P.points[i3 + 1], pz = P.points[i3 + 2];
		md = P.maxDist ? P.maxDist[item] : kInf;
		// a point with a NaN or infinite coordinate, or a NaN or negative max_dist: not a query
		valid = finite3(px, py, pz) && md >= 0;
	}
	static __device__ __forceinline__ void flush(const Params& P, bool mine, uint32_t item, const SignedLane& q, uint32_t lane) {
		if (!mine)
			return;
		float px, py, pz, md;
		bool valid;
		load(P, item, px, py, pz, md, valid);
		const f3 p = mk3(px, py, pz);
		const SignedAnswer a = P.gradient ? signed_answer<true>(P.scene.tris, P.wnodes, P.nWNodes, P.accuracy, p, valid, md, q.prim)
		                                  : signed_answer<false>(P.scene.tris, P.wnodes, P.nWNodes, P.accuracy, p, valid, md, q.prim);
		const size_t i = item; // (64-bit offsets: 3 n floats pass 2^32 bytes)
		P.sd[i] = a.sd;
		if (P.prim)
			P.prim[i] = a.prim;
		if (P.w)
			P.w[i] = a.w;
		if (P.point) {
			P.point[3 * i + 0] = a.point.x;
			P.point[3 * i + 1] = a.point.y;
			P.point[3 * i + 2] = a.point.z;
		}
		if (P.gradient) {
			P.gradient[3 * i + 0] = a.gradient.x;
			P.gradient[3 * i + 1] = a.gradient.y;
			P.gradient[3 * i + 2] = a.gradient.z;
		}
	}
};

struct BrickItems {
	typedef SdfParams Params;
	static __device__ __forceinline__ void load(const Params& P, uint32_t item, float& px, float& py, float& pz, float& md, bool& valid) {
		const BrickAt at = brick_at(P, item);
		px = brick_centre(P.origin[0], P.cell, at.bi), py = brick_centre(P.origin[1], P.cell, at.bj), pz = brick_centre(P.origin[2], P.cell, at.bk);
		md = P.reach;
		valid = finite3(px, py, pz) && md >= 0;
	}
	static __device__ __forceinline__ void flush(const Params& P, bool mine, uint32_t item, const SignedLane& q, uint32_t lane) {
		const bool near = mine && q.prim >= 0, far = mine && q.prim < 0;
		if (near)
			P.nearList[1u + atomicAdd(P.nearList, 1u)] = item; // (in any order: the second launch's answers do not depend on it)
		float fill = P.band;
		if (far) {
			// the centre's side: w_c > 0.5f (an invalid centre has no winding number: outside)
			const bool valid = finite3(q.px, q.py, q.pz);
			const float w = valid ? winding_of(P.wnodes, P.scene.tris, P.nWNodes, P.accuracy, q.px, q.py, q.pz) : 0.f;
			fill = w > 0.5f ? -P.band : P.band;
		}
		// the far bricks of this round, one after the other: a lane to a voxel
		for (unsigned long long m = __ballot(far); m != 0ull; m &= m - 1ull) {
			const int src = __ffsll((long long)m) - 1;
			const uint32_t b = (uint32_t)__shfl((int)item, src);
			const float v = __shfl(fill, src);
			const VoxelAt vx = voxel_at(P, brick_at(P, b), lane);
			if (vx.inGrid) {
				P.sd[vx.index] = v;
				if (P.prim)
					P.prim[vx.index] = -1;
			}
		}
	}
};

// The loop of the points and of the bricks: a wave takes 64 consecutive items at a time from the launch's ticket, descends for
// all of them until the last is done (no refill in between: the descent is the smaller half of an item's work, and the walk
// that follows wants every lane), then answers them together.
template <class Items>
__device__ __forceinline__ void signed_items(const typename Items::Params& P0, uint32_t nItems) {
	typedef typename Items::Params Params;
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();
	bool overflow = false;
	for (;;) {
		const Params& P = kernarg_view<Params>();
		uint32_t t = 0;
		if (lane == 0)
			t = atomicAdd(P.ticket, 1u);
		t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
		const unsigned long long first = 64ull * t;
		if (first >= nItems)
			break;
		const uint32_t item = (uint32_t)first + lane;
		const bool mine = item < nItems;
		SignedLane q = {};
		q.ref = kRefDone;
		q.prim = -1;
		if (mine) {
			float px, py, pz, md;
			bool valid;
			Items::load(P, item, px, py, pz, md, valid);
			lane_start(q, sc, px, py, pz, md, valid);
		}
		st.reset();
		while (__ballot(q.ref != kRefDone) != 0ull)
			n_traverse(sc, st, stagedNodes, q, [](uint32_t) { return false; }, lane_take);
		overflow = overflow || st.overflow;
		Items::flush(P, mine, item, q, lane);
	}
	q_report_overflow(overflow, lane, kernarg_view<Params>().error);
}

} // namespace

__global__ void __launch_bounds__(kBlock, 5) k_query_signed(const SignedParams P0) { signed_items<PointItems>(P0, P0.n); }

__global__ void __launch_bounds__(kBlock, 5) k_sdf_bricks(const SdfParams P0) { signed_items<BrickItems>(P0, P0.nBricks); }

__global__ void __launch_bounds__(kBlock, 5) k_sdf_voxels(const SdfParams P0) {
	constexpr int STACK_LDS = kQueryStackLds;
	TYR_DECLARE_FLAT_STACK(st, true)
	__shared__ float4 stagedNodes[7 * kStagedNodes];
	const DevScene& sc = P0.scene;
	q_stage_nodes(stagedNodes, sc);
	const uint32_t lane = lane_id();
	// the first launch's count, written by its atomics: read past the caches that launch did not write through
	const uint32_t nNear = __hip_atomic_load(P0.nearList, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (blockIdx.x == 0 && threadIdx.x == 0 && P0.stats) {
		P0.stats[0] = nNear;
		P0.stats[1] = P0.nBricks - nNear;
	}
	bool overflow = false;
	for (;;) {
		const SdfParams& P = kernarg_view<SdfParams>();
		uint32_t t = 0;
		if (lane == 0)
			t = atomicAdd(P.ticket, 1u);
		t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
		if (t >= nNear)
			break;
		const uint32_t b = P.nearList[1u + t];
		if (b >= P.nBricks) // (never: the list holds what the first launch put there)
			continue;
		const VoxelAt vx = voxel_at(P, brick_at(P, b), lane);
		const float px = axis_centre(P.origin[0], P.cell, vx.x), py = axis_centre(P.origin[1], P.cell, vx.y), pz = axis_centre(P.origin[2], P.cell, vx.z);
		const bool valid = finite3(px, py, pz);
		SignedLane q;
		lane_start(q, sc, px, py, pz, P.band, vx.inGrid && valid);
		st.reset();
		while (__ballot(q.ref != kRefDone) != 0ull)
			n_traverse(sc, st, stagedNodes, q, [](uint32_t) { return false; }, lane_take);
		overflow = overflow || st.overflow;
		if (vx.inGrid) {
			const SignedAnswer a = signed_answer<false>(sc.tris, P.wnodes, P.nWNodes, P.accuracy, mk3(px, py, pz), valid, P.band, q.prim);
			P.sd[vx.index] = a.sd;
			if (P.prim)
				P.prim[vx.index] = a.prim;
		}
	}
	q_report_overflow(overflow, lane, kernarg_view<SdfParams>().error);
}

void launch_signed(const SignedParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_query_signed, P, P.n, numCUs, lc.perCU[kLcSigned][0], stream);
}

void launch_sdf_bricks(const SdfParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	launch_persistent(k_sdf_bricks, P, P.nBricks, numCUs, lc.perCU[kLcSigned][1], stream);
}

void launch_sdf_voxels(const SdfParams& P, int numCUs, LaunchCache& lc, hipStream_t stream) {
	// (a wave to a brick: 64 items each; the number of near bricks stays on the device, so the grid is sized for all of them)
	const unsigned long long items = 64ull * P.nBricks;
	launch_persistent(k_sdf_voxels, P, items > 0xffffffffull ? 0xffffffffu : (uint32_t)items, numCUs, lc.perCU[kLcSigned][2], stream);
}

} // namespace tyr
