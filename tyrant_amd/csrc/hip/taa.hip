// taa.hip -- temporal anti-aliasing of a resolved frame (tyr_taa, host/taa.cpp), specified operation by operation in
// include/tyr_c.h "Temporal anti-aliasing".
//
// k_taa blends a resolved frame into the ctx's reprojected output history: it reads history[j] and writes history[j ^ 1].
// Every lane owns one pixel.  One 3 x 3 loop over the current frame finds the tap nearest to the camera (whose motion the
// pixel takes) and the YCoCg statistics of the neighbourhood box; then the history is sampled with the 4 x 4 Catmull-Rom
// kernel, or with tyr_temporal's four bilinear taps where that kernel does not apply, clamped to the box and blended.  All
// sums are held in registers in the specified tap order: fixed float32 sums, no atomics, no LDS (the 3 x 3 and 4 x 4
// footprints of a wave's 8 x 8 pixels overlap almost entirely, so the taps hit L1 / L2).  A 256-lane block covers a 16 x 16
// tile and each wave an 8 x 8 quarter of it (the mapping of hip/denoise.hip).  The bilinear taps repeat hip/temporal.hip's
// rather than share them, so that unit's code stays what it is.
#include "device_common.hpp"
#include "taa.hpp"

namespace tyr {

namespace {

constexpr int kTile = 16; // pixels per block side: 4 waves of 8 x 8

struct Ycc {
	float y, co, cg;
};

__device__ __forceinline__ Ycc to_ycocg(float r, float g, float b) {
	Ycc c;
	c.y = (0.25f * r + 0.5f * g) + 0.25f * b;
	c.co = 0.5f * r - 0.5f * b;
	c.cg = (0.5f * g - 0.25f * r) - 0.25f * b;
	return c;
}

// one channel of the neighbourhood box and the clamp of the history value h to it
__device__ __forceinline__ float box_clamp(float h, float s1, float s2, float n, float mn, float mx, float gamma) {
	const float mu = s1 / n;
	const float var = s2 / n - mu * mu;
	const float sd = sqrtf(var > 0.f ? var : 0.f);
	const float e = gamma * sd;
	const float tl = mu - e, th = mu + e;
	const float l0 = tl > mn ? tl : mn, h0 = th < mx ? th : mx;
	const float lo = l0 < mx ? l0 : mx, hi = h0 > mn ? h0 : mn;
	const float t = h > lo ? h : lo;
	return t < hi ? t : hi;
}

} // namespace

__global__ void __launch_bounds__(kBlock) k_taa(const TaaParams P) {
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const int W = static_cast<int>(P.W), H = static_cast<int>(P.H);
	const int x = static_cast<int>(blockIdx.x) * kTile + static_cast<int>((wave & 1u) * 8u + (lane & 7u));
	const int y = static_cast<int>(blockIdx.y) * kTile + static_cast<int>((wave >> 1) * 8u + (lane >> 3));
	if (x >= W || y >= H)
		return;
	const uint32_t i = static_cast<uint32_t>(y) * P.W + static_cast<uint32_t>(x);
	const float4 c = P.color[i];
	float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
	if (c.w != 0.f) {
		o = make_float4(c.x, c.y, c.z, 1.f);
		if (P.haveHistory) {
			// the 3 x 3 neighbourhood of the current frame: the nearest tap, and the box statistics
			const float inf = __builtin_inff();
			float s1y = 0.f, s1o = 0.f, s1g = 0.f, s2y = 0.f, s2o = 0.f, s2g = 0.f, cnt = 0.f;
			float mny = inf, mno = inf, mng = inf, mxy = -inf, mxo = -inf, mxg = -inf;
			float bz = 0.f;
			uint32_t bq = i;
			bool first = true;
#pragma unroll
			for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
				for (int dx = -1; dx <= 1; ++dx) {
					const int tx = x + dx, ty = y + dy;
					if (tx < 0 || tx >= W || ty < 0 || ty >= H)
						continue;
					const uint32_t q = static_cast<uint32_t>(ty) * P.W + static_cast<uint32_t>(tx);
					const float4 cq = P.color[q];
					if (!(cq.w != 0.f))
						continue;
					const float zq = P.depth[q];
					if (first || zq < bz) {
						bz = zq;
						bq = q;
						first = false;
					}
					const Ycc k = to_ycocg(cq.x, cq.y, cq.z);
					s1y = s1y + k.y;
					s1o = s1o + k.co;
					s1g = s1g + k.cg;
					s2y = s2y + k.y * k.y;
					s2o = s2o + k.co * k.co;
					s2g = s2g + k.cg * k.cg;
					cnt = cnt + 1.f;
					mny = k.y < mny ? k.y : mny;
					mno = k.co < mno ? k.co : mno;
					mng = k.cg < mng ? k.cg : mng;
					mxy = k.y > mxy ? k.y : mxy;
					mxo = k.co > mxo ? k.co : mxo;
					mxg = k.cg > mxg ? k.cg : mxg;
				}
			}
			// the motion of the nearest tap; the background does not move
			float2 m = make_float2(0.f, 0.f);
			bool ok = bz == kVeryFar;
			if (bz < kVeryFar && P.prevDepth[bq] < kVeryFar) {
				m = P.motion[bq];
				ok = true;
			}
			float hx = 0.f, hy = 0.f, hz = 0.f;
			bool have = false;
			if (ok && fabsf(m.x) < inf && fabsf(m.y) < inf) {
				const float qx = static_cast<float>(x) + m.x, qy = static_cast<float>(y) + m.y;
				// (outside these bounds every tap is outside the frame; inside them the conversions below are exact)
				if (qx > -1.f && qx < static_cast<float>(W) && qy > -1.f && qy < static_cast<float>(H)) {
					const float x0f = floorf(qx), y0f = floorf(qy);
					const float fx = qx - x0f, fy = qy - y0f;
					const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
					const float4* __restrict__ hist = P.histIn;
					bool cr = !P.bilinear && x0 >= 1 && x0 + 2 < W && y0 >= 1 && y0 + 2 < H;
					if (cr) {
						float wx[4], wy[4];
						wx[0] = fx * (-0.5f + fx * (1.f - 0.5f * fx));
						wx[1] = 1.f + (fx * fx) * (-2.5f + 1.5f * fx);
						wx[2] = fx * (0.5f + fx * (2.f - 1.5f * fx));
						wx[3] = (fx * fx) * (-0.5f + 0.5f * fx);
						wy[0] = fy * (-0.5f + fy * (1.f - 0.5f * fy));
						wy[1] = 1.f + (fy * fy) * (-2.5f + 1.5f * fy);
						wy[2] = fy * (0.5f + fy * (2.f - 1.5f * fy));
						wy[3] = (fy * fy) * (-0.5f + 0.5f * fy);
						float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
						for (int j = 0; j < 4; ++j) {
#pragma unroll
							for (int k = 0; k < 4; ++k) {
								const float4 h = hist[static_cast<uint32_t>(y0 - 1 + j) * P.W + static_cast<uint32_t>(x0 - 1 + k)];
								cr = cr && h.w != 0.f;
								const float w = wx[k] * wy[j];
								sx = sx + w * h.x;
								sy = sy + w * h.y;
								sz = sz + w * h.z;
							}
						}
						hx = sx;
						hy = sy;
						hz = sz;
						have = cr;
					}
					if (!cr) {
						const float gx = 1.f - fx, gy = 1.f - fy;
						float sx = 0.f, sy = 0.f, sz = 0.f, wb = 0.f;
#pragma unroll
						for (int t = 0; t < 4; ++t) {
							const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
							if (tx < 0 || tx >= W || ty < 0 || ty >= H)
								continue;
							const float4 h = hist[static_cast<uint32_t>(ty) * P.W + static_cast<uint32_t>(tx)];
							if (!(h.w != 0.f))
								continue;
							const float w = t == 0 ? gx * gy : (t == 1 ? fx * gy : (t == 2 ? gx * fy : fx * fy));
							sx = sx + w * h.x;
							sy = sy + w * h.y;
							sz = sz + w * h.z;
							wb = wb + w;
						}
						if (wb > 0.f) {
							hx = sx / wb;
							hy = sy / wb;
							hz = sz / wb;
							have = true;
						}
					}
				}
			}
			if (have) {
				const Ycc hc = to_ycocg(hx, hy, hz);
				const Ycc cc = to_ycocg(c.x, c.y, c.z);
				const float ky = box_clamp(hc.y, s1y, s2y, cnt, mny, mxy, P.gamma);
				const float ko = box_clamp(hc.co, s1o, s2o, cnt, mno, mxo, P.gamma);
				const float kg = box_clamp(hc.cg, s1g, s2g, cnt, mng, mxg, P.gamma);
				const float oy = ky + P.alpha * (cc.y - ky);
				const float oo = ko + P.alpha * (cc.co - ko);
				const float og = kg + P.alpha * (cc.cg - kg);
				const float t = oy - og;
				o = make_float4(t + oo, oy + og, t - oo, 1.f);
			}
		}
	}
	if (P.out)
		P.out[i] = o;
	P.histOut[i] = o;
}

void launch_taa(const TaaParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(k_taa, dim3((P.W + kTile - 1) / kTile, (P.H + kTile - 1) / kTile), dim3(kBlock), 0, stream, P);
}

} // namespace tyr
