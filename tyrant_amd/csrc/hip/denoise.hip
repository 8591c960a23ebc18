// denoise.hip -- the edge-avoiding a-trous denoiser (tyr_denoise, host/denoise.cpp; the filter is specified in
// include/tyr_c.h "Denoiser").
//
// k_denoise_prepare turns the accumulation buffer and the guides into the illumination u = (rgb / A) / d, with its state
// (valid, background, no sample), and a packed guide (n.xyz, depth): two float4 loads per tap from then on.  Pass j is one
// launch of k_denoise_pass, reading illum[j & 1] and writing illum[(j + 1) & 1]; the last pass multiplies the albedo back in
// (and tone-maps with TYR_DENOISE_RESOLVE) and writes the caller's frame instead.
//
// One lane owns one pixel and sums its 25 taps in registers in the specified order: fixed float32 sums, no atomics, the same
// bits as a CPU that evaluates the same IEEE operations.  A 256-lane block covers a 16 x 16 tile and each wave an 8 x 8 quarter
// of it, so that a wave's taps at small steps fall on few cache lines.
#include "denoise.hpp"
#include "detmath.hpp"
#include "device_common.hpp"

namespace tyr {

namespace {

constexpr int kTile = 16; // pixels per block side: 4 waves of 8 x 8

__device__ __forceinline__ float3 load3(const float* p, uint32_t i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// d_k = albedo_k > 0 ? albedo_k : 1
__device__ __forceinline__ float3 divisor(const float* albedo, uint32_t i) {
	const float3 a = load3(albedo, i);
	return make_float3(a.x > 0.f ? a.x : 1.f, a.y > 0.f ? a.y : 1.f, a.z > 0.f ? a.z : 1.f);
}

} // namespace

__global__ void __launch_bounds__(kBlock) k_denoise_prepare(const DenoiseParams P) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= P.W * P.H)
		return;
	const float4 a = P.accum[i];
	const float A = a.w;
	const float z = P.depth[i];
	const float3 d = divisor(P.albedo, i);
	const float3 n = load3(P.normal, i);
	float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
	if (A != 0.f) {
		const float cx = a.x / A, cy = a.y / A, cz = a.z / A;
		u = make_float4(cx / d.x, cy / d.y, cz / d.z, A > 0.f && z < kVeryFar ? 1.f : -1.f);
	}
	P.illum[0][i] = u;
	P.guide[i] = make_float4(n.x, n.y, n.z, z);
}

// kOut 0: an inner pass; 1: the last pass, linear output; 2: the last pass, tone-mapped
template <int kOut>
__global__ void __launch_bounds__(kBlock) k_denoise_pass(const DenoiseParams P, uint32_t j) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const int x = static_cast<int>(blockIdx.x) * kTile + static_cast<int>((wave & 1u) * 8u + (lane & 7u));
	const int y = static_cast<int>(blockIdx.y) * kTile + static_cast<int>((wave >> 1) * 8u + (lane >> 3));
	if (x >= W || y >= H)
		return;
	const float4* __restrict__ in = P.illum[j & 1u];
	const float4* __restrict__ guide = P.guide;
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 up = in[i];
	float4 v = up;
	if (up.w > 0.f) {
		const float4 gp = guide[i];
		const float izp = 1.f / gp.w;
		const float kc = P.kc * static_cast<float>(1u << (2u * j)); // exact: a power of two
		const float kz = P.kz;
		const uint32_t m = P.normalPowerLog2;
		const int s = 1 << j;
		constexpr float kH[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f };
		float sx = 0.f, sy = 0.f, sz = 0.f, ws = 0.f;
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
				if (!(uq.w > 0.f))
					continue;
				const float4 gq = guide[q];
				const float h = kH[dx + 2] * kH[dy + 2];
				const float ex = uq.x - up.x, ey = uq.y - up.y, ez = uq.z - up.z;
				const float dc2 = ex * ex + ey * ey + ez * ez;
				const float dn = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
				float g = dn > 0.f ? dn : 0.f;
				for (uint32_t k = 0; k < m; ++k)
					g = g * g;
				const float r = (gq.w - gp.w) * izp;
				const float xz = (r * r) * kz;
				const float den = (1.f + dc2 * kc) * (1.f + xz);
				const float w = (h * g) / den;
				sx = sx + w * uq.x;
				sy = sy + w * uq.y;
				sz = sz + w * uq.z;
				ws = ws + w;
			}
		}
		if (ws > 0.f)
			v = make_float4(sx / ws, sy / ws, sz / ws, up.w);
	}
	if constexpr (kOut == 0) {
		P.illum[(j + 1u) & 1u][i] = v;
	} else {
		float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
		if (v.w != 0.f) {
			const float3 d = divisor(P.albedo, i);
			const float r = v.x * d.x, g = v.y * d.y, b = v.z * d.z;
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

void launch_denoise(const DenoiseParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(k_denoise_prepare, dim3(blocks_for(P.W * P.H)), dim3(kBlock), 0, stream, P);
	const dim3 grid((P.W + kTile - 1) / kTile, (P.H + kTile - 1) / kTile);
	for (uint32_t j = 0; j + 1 < P.passes; ++j)
		hipLaunchKernelGGL(k_denoise_pass<0>, grid, dim3(kBlock), 0, stream, P, j);
	if (P.resolve)
		hipLaunchKernelGGL(k_denoise_pass<2>, grid, dim3(kBlock), 0, stream, P, P.passes - 1);
	else
		hipLaunchKernelGGL(k_denoise_pass<1>, grid, dim3(kBlock), 0, stream, P, P.passes - 1);
}

} // namespace tyr
