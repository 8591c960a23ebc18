// temporal.hip -- motion vectors (tyr_render_motion) and the temporal reprojection of frames (tyr_temporal), host/temporal.cpp;
// both are specified operation by operation in include/tyr_c.h "Motion vectors" and "Temporal reprojection".
//
// k_render_motion regenerates each local pixel's sample-0 camera ray (camera_seed / camera_focus / camera_lens, as
// k_primary and the AOV pass make it), finds its hit point from tyr_render_aov's ids alone -- one triangle_test_uv or
// one sphere_intersect, no traversal -- moves it to the previous frame's triangle record by its barycentrics, and projects
// both points through their camera's pinhole.  k_motion_chain (tyr_render_motion_chain) does the same, except where
// tyr_render_aov_chain followed a specular chain: there it projects the virtual image point.
//
// k_temporal blends a frame's illumination into a bilinearly reprojected history that the ctx keeps ping-ponged: it reads
// history[j] and writes history[j ^ 1].  Every lane owns one pixel and sums its four taps in registers in the specified
// order: fixed float32 sums, no atomics.  A 256-lane block covers a 16 x 16 tile and each wave an 8 x 8 quarter of it (the
// mapping of hip/denoise.hip), so that a wave's taps fall on few cache lines.
#include "device_common.hpp"
#include "temporal.hpp"

namespace tyr {

namespace {

constexpr int kTile = 16; // pixels per block side: 4 waves of 8 x 8

__device__ __forceinline__ f3 load3(const float* p, uint32_t i) { return mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// the pinhole projection of X through a camera: continuous pixel coordinates (xi, yi); false when X is not in front of it
__device__ __forceinline__ bool project(f3 X, f3 O, f3 F, f3 R, f3 U, float FF, float RR, float UU, float fW, float fH, float& xi, float& yi) {
	const f3 w = X - O;
	const float f = dot(w, F);
	const float a = (dot(w, R) * FF) / (f * RR);
	const float b = (dot(w, U) * FF) / (f * UU);
	xi = (a + 0.5f) * fW;
	yi = (0.5f - b) * fH;
	return f > 0.f;
}

} // namespace

// one pixel of the motion pass.  CHAIN (tyr_render_motion_chain): where the pixel's specular chain has bounces, the point is the
// virtual image point on the camera ray at the chain's summed length, the same in both frames
template <bool CHAIN>
__device__ __forceinline__ void motion_pixel(const MotionParams& P, const int32_t* __restrict__ chain, const float* __restrict__ length0) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t x = blockIdx.x * kTile + (wave & 1u) * 8u + (lane & 7u);
	const uint32_t yl = blockIdx.y * kTile + (wave >> 1) * 8u + (lane >> 3);
	if (x >= P.W || yl >= P.localRows)
		return;
	const uint32_t y = yl * P.nranks + P.rank;
	const size_t i = static_cast<size_t>(y) * P.W + x;
	const int32_t prim = P.prim[i], geom = P.geom[i];
	float mx = 0.f, my = 0.f, pd = kVeryFar;
	const bool tri = geom == 1 && prim >= 0 && static_cast<uint32_t>(prim) < P.nPrims;
	const bool sph = geom == 0 && prim >= 0 && prim < TYR_NUM_SPHERES;
	bool through = false;
	float reach = 0.f;
	if (CHAIN) {
		through = chain[i] > 0;
		reach = length0[i];
	}
	if (through ? reach < kVeryFar : (tri || sph)) {
		// sample 0's camera ray: ticket 0 * nPixels + p (hip/aov.hip)
		uint32_t seed = camera_seed(P, yl * P.W + x);
		const CameraRay cr = camera_lens(P, seed, camera_focus(P, seed, static_cast<int>(x), static_cast<int>(y)), ld3(P.camPos), ld3(P.camRight), ld3(P.camUp));
		f3 X = mk3(0.f, 0.f, 0.f), Xp = X;
		bool hit = false;
		if (through) {
			hit = true;
			X = cr.origin + cr.direction * reach;
			Xp = X;
		} else if (tri) {
			const TriData td = triangle_load(P.tris, static_cast<uint32_t>(prim));
			float u = 0.f, v = 0.f;
			hit = triangle_test_uv(td, make_ray(cr.origin, cr.direction), u, v) != 0.f;
			X = (mk3(td.a.x, td.a.y, td.a.z) + u * mk3(td.a.w, td.b.x, td.b.y)) + v * mk3(td.b.z, td.b.w, td.c.x);
			Xp = X;
			if (P.prevPrims) {
				const float* rec = P.prevPrims + 10u * static_cast<uint32_t>(prim);
				Xp = (ld3(rec) + u * ld3(rec + 3)) + v * ld3(rec + 6);
			}
		} else {
			const float t = sphere_intersect(P.spheres[prim], cr.origin, cr.direction);
			hit = t != 0.f;
			X = cr.origin + cr.direction * t;
			Xp = X;
		}
		const float fW = static_cast<float>(P.W), fH = static_cast<float>(P.H);
		float xc, yc, xp, yp;
		const bool front = project(X, ld3(P.camPos), ld3(P.camDir), ld3(P.camRight), ld3(P.camUp), P.camFF, P.camRR, P.camUU, fW, fH, xc, yc);
		const bool frontPrev = project(Xp, ld3(P.prevPos), ld3(P.prevDir), ld3(P.prevRight), ld3(P.prevUp), P.prevFF, P.prevRR, P.prevUU, fW, fH, xp, yp);
		const float dx = xp - xc, dy = yp - yc;
		const float d = length(Xp - ld3(P.prevPos));
		if (hit && front && frontPrev && fabsf(dx) < __builtin_inff() && fabsf(dy) < __builtin_inff() && d < __builtin_inff()) {
			mx = dx;
			my = dy;
			pd = d;
		}
	}
	if (P.motion) {
		P.motion[2 * i + 0] = mx;
		P.motion[2 * i + 1] = my;
	}
	if (P.prevDepth)
		P.prevDepth[i] = pd;
}

__global__ void __launch_bounds__(kBlock) k_render_motion(const MotionParams P) { motion_pixel<false>(P, nullptr, nullptr); }

__global__ void __launch_bounds__(kBlock) k_motion_chain(const MotionParams P, const int32_t* __restrict__ chain, const float* __restrict__ length0) { motion_pixel<true>(P, chain, length0); }

__global__ void __launch_bounds__(kBlock) k_temporal(const TemporalParams P) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const int x = static_cast<int>(blockIdx.x) * kTile + static_cast<int>((wave & 1u) * 8u + (lane & 7u));
	const int y = static_cast<int>(blockIdx.y) * kTile + static_cast<int>((wave >> 1) * 8u + (lane >> 3));
	if (x >= W || y >= H)
		return;
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 a = P.accum[i];
	const float A = a.w;
	const float z = P.depth[i];
	const f3 n = load3(P.normal, i);
	float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
	float4 hu = make_float4(0.f, 0.f, 0.f, 0.f); // invalid pixels: history length 0
	if (A != 0.f) {
		const float cx = a.x / A, cy = a.y / A, cz = a.z / A;
		if (!(A > 0.f && z < kVeryFar)) {
			o = make_float4(cx, cy, cz, 1.f); // background
		} else {
			const f3 alb = load3(P.albedo, i);
			const float dx = alb.x > 0.f ? alb.x : 1.f, dy = alb.y > 0.f ? alb.y : 1.f, dz = alb.z > 0.f ? alb.z : 1.f;
			const float ux = cx / dx, uy = cy / dy, uz = cz / dz;
			float vx = ux, vy = uy, vz = uz, len = 1.f;
			if (P.haveHistory) {
				const float2 m = P.motion[i];
				const float pz = P.prevDepth[i];
				const float qx = static_cast<float>(x) + m.x, qy = static_cast<float>(y) + m.y;
				// (outside these bounds every tap is outside the frame; inside them the conversions below are exact)
				if (pz < kVeryFar && qx > -1.f && qx < static_cast<float>(W) && qy > -1.f && qy < static_cast<float>(H)) {
					const float x0f = floorf(qx), y0f = floorf(qy);
					const float fx = qx - x0f, fy = qy - y0f;
					const float gx = 1.f - fx, gy = 1.f - fy;
					const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
					const float tol = P.depthTolerance * pz;
					const float4* __restrict__ hU = P.histIn[0];
					const float4* __restrict__ hG = P.histIn[1];
					float sx = 0.f, sy = 0.f, sz = 0.f, sl = 0.f, wb = 0.f;
#pragma unroll
					for (int t = 0; t < 4; ++t) {
						const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
						if (tx < 0 || tx >= W || ty < 0 || ty >= H)
							continue;
						const uint32_t q = static_cast<uint32_t>(ty) * P.W + static_cast<uint32_t>(tx);
						const float4 h = hU[q];
						if (!(h.w > 0.f))
							continue;
						const float4 g = hG[q];
						if (!(fabsf(g.w - pz) <= tol))
							continue;
						const float dn = g.x * n.x + g.y * n.y + g.z * n.z;
						if (!(dn >= P.normalCos))
							continue;
						const float w = t == 0 ? gx * gy : (t == 1 ? fx * gy : (t == 2 ? gx * fy : fx * fy));
						sx = sx + w * h.x;
						sy = sy + w * h.y;
						sz = sz + w * h.z;
						sl = sl + w * h.w;
						wb = wb + w;
					}
					if (wb > 0.f) {
						const float hx = sx / wb, hy = sy / wb, hz = sz / wb;
						const float np1 = sl / wb + 1.f;
						len = np1 < P.maxHistory ? np1 : P.maxHistory;
						if (len > 1.f) { // (n == 1: the current frame alone, v = u exactly)
							const float k = 1.f / len;
							vx = hx + k * (ux - hx);
							vy = hy + k * (uy - hy);
							vz = hz + k * (uz - hz);
						}
					}
				}
			}
			o = make_float4(vx * dx, vy * dy, vz * dz, 1.f);
			hu = make_float4(vx, vy, vz, len);
		}
	}
	P.out[i] = o;
	if (P.lenOut)
		P.lenOut[i] = hu.w;
	P.histOut[0][i] = hu;
	P.histOut[1][i] = make_float4(n.x, n.y, n.z, z);
}

void launch_motion(const MotionParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(k_render_motion, dim3((P.W + kTile - 1) / kTile, (P.localRows + kTile - 1) / kTile), dim3(kBlock), 0, stream, P);
}

void launch_motion_chain(const MotionParams& P, const int32_t* chain, const float* length0, hipStream_t stream) {
	hipLaunchKernelGGL(k_motion_chain, dim3((P.W + kTile - 1) / kTile, (P.localRows + kTile - 1) / kTile), dim3(kBlock), 0, stream, P, chain, length0);
}

void launch_temporal(const TemporalParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(k_temporal, dim3((P.W + kTile - 1) / kTile, (P.H + kTile - 1) / kTile), dim3(kBlock), 0, stream, P);
}

} // namespace tyr
