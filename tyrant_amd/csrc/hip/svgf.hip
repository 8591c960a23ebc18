// svgf.hip -- the variance-guided spatiotemporal filter (tyr_svgf, host/svgf.cpp; specified operation by operation in
// include/tyr_c.h "SVGF").
//
// k_svgf_reproject is k_temporal (hip/temporal.hip) with two more blended quantities, the luminance moments m1 and m2, against
// a history whose colour is the filtered output of the last call's first a-trous pass.  k_svgf_variance turns the moments into
// a variance per pixel: the temporal one where the history holds at least 4 frames, a 7 x 7 spatial estimate elsewhere.  Pass j
// is one launch of k_svgf_pass, reading illum[j & 1] and writing illum[(j + 1) & 1]; pass 0 also stores its colour as the next
// call's history, and the last pass multiplies the albedo back in (and tone-maps with TYR_SVGF_RESOLVE) and writes the caller's
// frame instead.
//
// One lane owns one pixel and sums its taps in registers in the specified order: fixed float32 sums, no atomics.  A 256-lane
// block covers a 16 x 16 tile and each wave an 8 x 8 quarter of it (the mapping of hip/denoise.hip).
#include "detmath.hpp"
#include "device_common.hpp"
#include "svgf.hpp"

namespace tyr {

namespace {

constexpr int kTile = 16; // pixels per block side: 4 waves of 8 x 8

__device__ __forceinline__ float3 load3(const float* p, uint32_t i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// d_k = albedo_k > 0 ? albedo_k : 1
__device__ __forceinline__ float3 divisor(const float* albedo, uint32_t i) {
	const float3 a = load3(albedo, i);
	return make_float3(a.x > 0.f ? a.x : 1.f, a.y > 0.f ? a.y : 1.f, a.z > 0.f ? a.z : 1.f);
}

__device__ __forceinline__ float luminance(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// max(0, n_p . n_q) squared m times: the a-trous normal term (hip/denoise.hip)
__device__ __forceinline__ float normal_term(float4 gp, float4 gq, uint32_t m) {
	const float dn = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
	float g = dn > 0.f ? dn : 0.f;
	for (uint32_t k = 0; k < m; ++k)
		g = g * g;
	return g;
}

__device__ __forceinline__ bool tile_pixel(uint32_t W, uint32_t H, int& x, int& y) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	x = static_cast<int>(blockIdx.x) * kTile + static_cast<int>((wave & 1u) * 8u + (lane & 7u));
	y = static_cast<int>(blockIdx.y) * kTile + static_cast<int>((wave >> 1) * 8u + (lane >> 3));
	return x < static_cast<int>(W) && y < static_cast<int>(H);
}

} // namespace

__global__ void __launch_bounds__(kBlock) k_svgf_reproject(const SvgfParams P) {
	int x, y;
	if (!tile_pixel(P.W, P.H, x, y))
		return;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 a = P.accum[i];
	const float A = a.w;
	const float z = P.depth[i];
	const float3 n = load3(P.normal, i);
	float4 hu = make_float4(0.f, 0.f, 0.f, 0.f); // pixels that are not valid: history length 0, m2 = -1
	float2 hm = make_float2(0.f, -1.f);
	if (A > 0.f && z < kVeryFar) {
		const float3 d = divisor(P.albedo, i);
		const float ux = (a.x / A) / d.x, uy = (a.y / A) / d.y, uz = (a.z / A) / d.z;
		const float l = luminance(ux, uy, uz);
		const float l2 = l * l;
		float vx = ux, vy = uy, vz = uz, m1 = l, m2 = l2, len = 1.f;
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
				const float2* __restrict__ hM = P.histMomIn;
				float sx = 0.f, sy = 0.f, sz = 0.f, sl = 0.f, s1 = 0.f, s2 = 0.f, wb = 0.f;
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
					const float2 mq = hM[q];
					const float w = t == 0 ? gx * gy : (t == 1 ? fx * gy : (t == 2 ? gx * fy : fx * fy));
					sx = sx + w * h.x;
					sy = sy + w * h.y;
					sz = sz + w * h.z;
					sl = sl + w * h.w;
					s1 = s1 + w * mq.x;
					s2 = s2 + w * mq.y;
					wb = wb + w;
				}
				if (wb > 0.f) {
					const float hx = sx / wb, hy = sy / wb, hz = sz / wb, h1 = s1 / wb, h2 = s2 / wb;
					const float np1 = sl / wb + 1.f;
					len = np1 < P.maxHistory ? np1 : P.maxHistory;
					if (len > 1.f) { // (n == 1: the current frame alone)
						const float k = 1.f / len;
						vx = hx + k * (ux - hx);
						vy = hy + k * (uy - hy);
						vz = hz + k * (uz - hz);
						m1 = h1 + k * (l - h1);
						m2 = h2 + k * (l2 - h2);
					}
				}
			}
		}
		hu = make_float4(vx, vy, vz, len);
		hm = make_float2(m1, m2);
	}
	P.histOut[0][i] = hu; // pass 0 replaces u by its output
	P.histOut[1][i] = make_float4(n.x, n.y, n.z, z);
	P.histMomOut[i] = hm;
}

__global__ void __launch_bounds__(kBlock) k_svgf_variance(const SvgfParams P) {
	int x, y;
	if (!tile_pixel(P.W, P.H, x, y))
		return;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 hu = P.histOut[0][i];
	float4 o = make_float4(0.f, 0.f, 0.f, -1.f);
	float var = 0.f;
	if (hu.w > 0.f) {
		const float2* __restrict__ mom = P.histMomOut;
		const float len = hu.w;
		if (len >= 4.f) {
			const float2 mp = mom[i];
			const float t = mp.y - mp.x * mp.x;
			var = t > 0.f ? t : 0.f;
		} else {
			const float4* __restrict__ guide = P.histOut[1];
			const float4 gp = guide[i];
			const float izp = 1.f / gp.w;
			const float kz = P.kz;
			const uint32_t m = P.normalPowerLog2;
			float s1 = 0.f, s2 = 0.f, ws = 0.f;
#pragma unroll
			for (int dy = -3; dy <= 3; ++dy) {
				const int qy = y + dy;
				if (qy < 0 || qy >= H)
					continue;
#pragma unroll
				for (int dx = -3; dx <= 3; ++dx) {
					const int qx = x + dx;
					if (qx < 0 || qx >= W)
						continue;
					const uint32_t q = static_cast<uint32_t>(qy) * P.W + static_cast<uint32_t>(qx);
					const float2 mq = mom[q];
					if (mq.y < 0.f) // not valid
						continue;
					float w = 1.f;
					if (dx != 0 || dy != 0) {
						const float4 gq = guide[q];
						const float g = normal_term(gp, gq, m);
						const float r = (gq.w - gp.w) * izp;
						const float xz = (r * r) * kz;
						w = g / (1.f + xz);
					}
					s1 = s1 + w * mq.x;
					s2 = s2 + w * mq.y;
					ws = ws + w;
				}
			}
			const float M1 = s1 / ws, M2 = s2 / ws;
			const float t = M2 - M1 * M1;
			var = (t > 0.f ? t : 0.f) * (4.f / len);
		}
		o = make_float4(hu.x, hu.y, hu.z, var);
	}
	P.illum[0][i] = o;
	if (P.varOut)
		P.varOut[i] = var;
}

// kOut 0: an inner pass; 1: the last pass, linear output; 2: the last pass, tone-mapped.  Pass 0 also writes the history's colour.
template <int kOut>
__global__ void __launch_bounds__(kBlock) k_svgf_pass(const SvgfParams P, uint32_t j) {
	int x, y;
	if (!tile_pixel(P.W, P.H, x, y))
		return;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const float4* __restrict__ in = P.illum[j & 1u];
	const float4* __restrict__ guide = P.histOut[1];
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 up = in[i];
	float4 v = up;
	if (!(up.w < 0.f)) {
		// the variance's 3 x 3 Gaussian over valid taps
		constexpr float kG[3] = { 0.25f, 0.5f, 0.25f };
		float gs = 0.f, gw = 0.f;
#pragma unroll
		for (int dy = -1; dy <= 1; ++dy) {
			const int qy = y + dy;
			if (qy < 0 || qy >= H)
				continue;
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx) {
				const int qx = x + dx;
				if (qx < 0 || qx >= W)
					continue;
				const float vq = in[static_cast<uint32_t>(qy) * P.W + static_cast<uint32_t>(qx)].w;
				if (vq < 0.f)
					continue;
				const float k = kG[dx + 1] * kG[dy + 1];
				gs = gs + k * vq;
				gw = gw + k;
			}
		}
		const float gv = gs / gw;
		const float kl = 1.f / (P.sl2 * gv + 1e-10f);
		const float lp = luminance(up.x, up.y, up.z);
		const float4 gp = guide[i];
		const float izp = 1.f / gp.w;
		const float kz = P.kz;
		const uint32_t m = P.normalPowerLog2;
		const int s = 1 << j;
		constexpr float kH[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f };
		float sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f, ws = 0.f;
#pragma unroll
		for (int dy = -2; dy <= 2; ++dy) {
			const int qy = y + dy * s;
			if (qy < 0 || qy >= H)
				continue;
#pragma unroll
			for (int dx = -2; dx <= 2; ++dx) {
				const int qx = x + dx * s;
				if (qx < 0 || qx >= W)
					continue;
				const uint32_t q = static_cast<uint32_t>(qy) * P.W + static_cast<uint32_t>(qx);
				const float4 uq = in[q];
				if (uq.w < 0.f)
					continue;
				const float4 gq = guide[q];
				const float h = kH[dx + 2] * kH[dy + 2];
				const float dl = luminance(uq.x, uq.y, uq.z) - lp;
				const float g = normal_term(gp, gq, m);
				const float r = (gq.w - gp.w) * izp;
				const float xz = (r * r) * kz;
				const float den = (1.f + (dl * dl) * kl) * (1.f + xz);
				const float w = (h * g) / den;
				sx = sx + w * uq.x;
				sy = sy + w * uq.y;
				sz = sz + w * uq.z;
				sv = sv + (w * w) * uq.w;
				ws = ws + w;
			}
		}
		if (ws > 0.f)
			v = make_float4(sx / ws, sy / ws, sz / ws, sv / (ws * ws));
	}
	if (j == 0u) {
		float4* __restrict__ hist = P.histOut[0];
		hist[i] = make_float4(v.x, v.y, v.z, hist[i].w);
	}
	if constexpr (kOut == 0) {
		P.illum[(j + 1u) & 1u][i] = v;
	} else {
		float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
		float r = 0.f, g = 0.f, b = 0.f;
		bool any = true;
		if (!(up.w < 0.f)) {
			const float3 d = divisor(P.albedo, i);
			r = v.x * d.x;
			g = v.y * d.y;
			b = v.z * d.z;
		} else {
			const float4 a = P.accum[i];
			any = a.w != 0.f;
			if (any) { // background: c
				r = a.x / a.w;
				g = a.y / a.w;
				b = a.z / a.w;
			}
		}
		if (any) {
			if constexpr (kOut == 1) {
				o = make_float4(r, g, b, 1.f);
			} else { // k_resolve (hip/frame.hip) of (r, g, b, 1): its division by a = 1 is exact
				constexpr float inv_gamma = 1.0f / 2.2f;
				o = make_float4(dm::powf_det(r / (r + 1.f), inv_gamma), dm::powf_det(g / (g + 1.f), inv_gamma), dm::powf_det(b / (b + 1.f), inv_gamma),
					dm::powf_det(1.f / (1.f + 1.f), inv_gamma));
			}
		}
		P.out[i] = o;
	}
}

void launch_svgf(const SvgfParams& P, hipStream_t stream) {
	const dim3 grid((P.W + kTile - 1) / kTile, (P.H + kTile - 1) / kTile);
	hipLaunchKernelGGL(k_svgf_reproject, grid, dim3(kBlock), 0, stream, P);
	hipLaunchKernelGGL(k_svgf_variance, grid, dim3(kBlock), 0, stream, P);
	for (uint32_t j = 0; j + 1 < P.passes; ++j)
		hipLaunchKernelGGL(k_svgf_pass<0>, grid, dim3(kBlock), 0, stream, P, j);
	if (P.resolve)
		hipLaunchKernelGGL(k_svgf_pass<2>, grid, dim3(kBlock), 0, stream, P, P.passes - 1);
	else
		hipLaunchKernelGGL(k_svgf_pass<1>, grid, dim3(kBlock), 0, stream, P, P.passes - 1);
}

} // namespace tyr
