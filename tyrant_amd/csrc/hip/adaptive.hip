// adaptive.hip -- adaptive sampling (include/tyr_c.h "Adaptive sampling", DESIGN.md "Adaptive sampling"): the build of a sample
// map's sample-major ticket list, and the allocator that turns a per-pixel error estimate into a sample map with an exact total.
// (The camera rays of mapped mode are made by hip/frame.hip's k_primary_mapped.)
#include <algorithm>
#include <cfloat>

#include "adaptive.hpp"
#include "device_common.hpp"

namespace tyr {

// ======================================================================================
// The ticket list L of a sample map: pass s lists, in increasing order, the local pixels p with c[p] > s; L is the passes
// end to end.  k_map_hist reads the map once (the host then knows T, the largest count and every pass's length); pass 0 is
// the stable compaction of the pixels, pass s that of pass s - 1 (k_pass_count, k_pass_scan_blocks, k_pass_scatter: linear in
// the pass, while passes are at least a block long); the short passes at the end are all written by one block (k_pass_tail).
// ======================================================================================

// the rank of this thread's element among the block's kept ones (in thread order) and the block's count; waveCnt: LDS[4]
__device__ __forceinline__ uint32_t block_rank(bool keep, uint32_t* waveCnt, uint32_t& total) {
	const unsigned long long m = __ballot(keep);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (lane == 0)
		waveCnt[wave] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t before = 0;
	total = 0;
#pragma unroll
	for (uint32_t w = 0; w < kBlock / 64; ++w) {
		if (w < wave)
			before += waveCnt[w];
		total += waveCnt[w];
	}
	__syncthreads(); // waveCnt is reused by the next call
	return before + lanes_below(m);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
	for (int o = 32; o; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
	for (int o = 32; o; o >>= 1) {
		const uint32_t u = __shfl_xor(v, o, 64);
		v = u > v ? u : v;
	}
	return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
	for (int o = 32; o; o >>= 1) {
		const uint32_t u = __shfl_xor(v, o, 64);
		v = u < v ? u : v;
	}
	return v;
}
// full-frame index of local pixel p (rows y = yl * nranks + rank)
__device__ __forceinline__ size_t frame_index(uint32_t p, uint32_t W, uint32_t rank, uint32_t nranks) {
	const uint32_t x = p % W, y = (p / W) * nranks + rank;
	return (size_t)y * W + x;
}

// the map at the local pixels, T, the largest count, a flag for values above kMaxSpp, and the histogram of the counts >= 1.
// The block reduces first: one atomic per block for T, the maximum and the flag, and one per block for the histogram when the
// block's counts are all the same (a uniform map), else one per distinct count in each wave.
__global__ void __launch_bounds__(kBlock) k_map_hist(const SampleMapArgs A, uint32_t nPixels) {
	__shared__ uint32_t sumSh[kBlock / 64], maxSh[kBlock / 64], firstSh;
	const uint32_t p = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t c = 0;
	bool bad = false;
	if (p < nPixels) {
		c = A.map[frame_index(p, A.W, A.rank, A.nranks)];
		if (c > kMaxSpp) {
			bad = true;
			c = 0;
		}
		A.counts[p] = c;
	}
	if (threadIdx.x == 0)
		firstSh = c;
	const uint32_t sum = wave_sum_u32(c), mx = wave_max_u32(c); // (64 x 65535 fits 32 bits)
	if (lane == 0) {
		sumSh[wave] = sum;
		maxSh[wave] = mx;
	}
	const bool anyBad = __syncthreads_or(bad) != 0;
	const uint32_t first = firstSh;
	const bool uniform = __syncthreads_and(p >= nPixels || c == first) != 0;
	if (threadIdx.x == 0) {
		uint32_t bsum = 0, bmax = 0;
#pragma unroll
		for (uint32_t w = 0; w < kBlock / 64; ++w) {
			bsum += sumSh[w]; // (256 x 65535 fits 32 bits)
			bmax = maxSh[w] > bmax ? maxSh[w] : bmax;
		}
		if (bsum)
			atomicAdd(reinterpret_cast<unsigned long long*>(A.summary), (unsigned long long)bsum); // summary[0..1]: 8-byte aligned (host/adaptive.cpp)
		if (bmax)
			atomicMax(A.summary + 2, bmax);
		if (anyBad)
			atomicOr(A.summary + 3, 1u);
	}
	uint32_t* hist = A.summary + kMapSummaryWords;
	if (uniform) {
		if (threadIdx.x == 0 && first != 0u)
			atomicAdd(hist + first, (nPixels - blockIdx.x * kBlock) < kBlock ? nPixels - blockIdx.x * kBlock : kBlock);
		return;
	}
	bool pending = c != 0u;
	for (;;) {
		const unsigned long long act = __ballot(pending);
		if (act == 0ull)
			break;
		const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
		const uint32_t v = __shfl(c, (int)leader, 64);
		const unsigned long long same = __ballot(pending && c == v);
		if (lane == leader)
			atomicAdd(hist + v, (uint32_t)__popcll(same));
		if (c == v)
			pending = false;
	}
}

__device__ __forceinline__ bool pass_keep(const uint32_t* in, uint32_t e, uint32_t n, const uint32_t* counts, uint32_t s, uint32_t& pix) {
	pix = 0u;
	if (e >= n)
		return false;
	pix = in ? in[e] : e;
	return counts[pix] > s;
}
// the kept elements of each kCompactTile block of the input
__global__ void __launch_bounds__(kBlock) k_pass_count(const uint32_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ counts, uint32_t s, uint32_t* __restrict__ blockCnt) {
	__shared__ uint32_t waveCnt[kBlock / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t kept = 0;
#pragma unroll
	for (uint32_t r = 0; r < kCompactTile / kBlock; ++r) {
		uint32_t pix;
		kept += (uint32_t)__popcll(__ballot(pass_keep(in, blockIdx.x * kCompactTile + r * kBlock + threadIdx.x, n, counts, s, pix)));
	}
	if (lane == 0)
		waveCnt[wave] = kept;
	__syncthreads();
	if (threadIdx.x == 0)
		blockCnt[blockIdx.x] = waveCnt[0] + waveCnt[1] + waveCnt[2] + waveCnt[3];
}
// one block: the block counts -> exclusive prefixes, in place
__global__ void __launch_bounds__(kBlock) k_pass_scan_blocks(uint32_t* __restrict__ blockCnt, uint32_t nBlocks) {
	__shared__ uint32_t waveSum[kBlock / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for (uint32_t base = 0; base < nBlocks; base += kBlock) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < nBlocks ? blockCnt[i] : 0u;
		uint32_t incl = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t u = __shfl_up(incl, (unsigned)o, 64);
			if (lane >= (uint32_t)o)
				incl += u;
		}
		if (lane == 63u)
			waveSum[wave] = incl;
		__syncthreads();
		uint32_t before = carry, tot = 0;
#pragma unroll
		for (uint32_t w = 0; w < kBlock / 64; ++w) {
			if (w < wave)
				before += waveSum[w];
			tot += waveSum[w];
		}
		if (i < nBlocks)
			blockCnt[i] = before + incl - v;
		carry += tot;
		__syncthreads();
	}
}
// ... and written in order: behind the blocks in front (blockStart: their exclusive prefix) and the rounds in front
__global__ void __launch_bounds__(kBlock) k_pass_scatter(const uint32_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ counts, uint32_t s, uint32_t* __restrict__ out, uint32_t outLimit,
                                                         const uint32_t* __restrict__ blockStart) {
	__shared__ uint32_t waveCnt[kBlock / 64];
	uint32_t base = blockStart[blockIdx.x];
#pragma unroll
	for (uint32_t r = 0; r < kCompactTile / kBlock; ++r) {
		uint32_t pix, tot;
		const bool keep = pass_keep(in, blockIdx.x * kCompactTile + r * kBlock + threadIdx.x, n, counts, s, pix);
		const uint32_t rank = block_rank(keep, waveCnt, tot);
		if (keep && base + rank < outLimit)
			out[base + rank] = pix;
		base += tot;
	}
}

// passes that equal the one in front of them (no pixel's count ends there): copies, in one launch per run of them
__global__ void __launch_bounds__(kBlock) k_pass_repeat(uint32_t* __restrict__ list, uint32_t src, uint32_t n, uint32_t dst, uint32_t len, uint32_t total) {
	for (uint32_t idx = blockIdx.x * kBlock + threadIdx.x; idx < len; idx += gridDim.x * kBlock)
		if (dst + idx < total)
			list[dst + idx] = list[src + idx % n];
}

// Passes sFirst .. maxSpp - 1 from pass sFirst - 1 (nIn < kCompactTile entries): the block keeps the remaining pixels and their
// counts in LDS.  A pass's content only changes where some pixel's count ends, so each round compacts once and writes the
// passes up to the next such count as copies: rounds <= nIn, whatever the counts (one pixel at 65535: one round).
__global__ void __launch_bounds__(kBlock) k_pass_tail(uint32_t* __restrict__ list, const uint32_t* __restrict__ in, uint32_t nIn, const uint32_t* __restrict__ counts, uint32_t sFirst, uint32_t maxSpp,
                                                      uint32_t outOff, uint32_t total) {
	__shared__ uint32_t pixSh[2][kCompactTile], cntSh[2][kCompactTile], waveCnt[kBlock / 64], minSh[kBlock / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t j = threadIdx.x; j < nIn; j += kBlock) {
		const uint32_t pix = in[j];
		pixSh[0][j] = pix;
		cntSh[0][j] = counts[pix];
	}
	__syncthreads();
	uint32_t cur = 0, n = nIn, s = sFirst, off = outOff;
	while (s < maxSpp) {
		uint32_t kept = 0, mn = 0xffffffffu;
#pragma unroll
		for (uint32_t r = 0; r < kCompactTile / kBlock; ++r) {
			const uint32_t j = r * kBlock + threadIdx.x;
			const bool keep = j < n && cntSh[cur][j] > s;
			uint32_t tot;
			const uint32_t rank = block_rank(keep, waveCnt, tot);
			if (keep) {
				pixSh[cur ^ 1u][kept + rank] = pixSh[cur][j];
				cntSh[cur ^ 1u][kept + rank] = cntSh[cur][j];
				mn = cntSh[cur][j] < mn ? cntSh[cur][j] : mn;
			}
			kept += tot;
		}
		mn = wave_min_u32(mn);
		if (lane == 0)
			minSh[wave] = mn;
		__syncthreads();
		uint32_t sNext = minSh[0];
#pragma unroll
		for (uint32_t w = 1; w < kBlock / 64; ++w)
			sNext = minSh[w] < sNext ? minSh[w] : sNext;
		if (kept == 0u || sNext <= s || sNext > maxSpp)
			break; // (cannot happen with the host's plan: every pass below the largest count holds that count's pixels)
		cur ^= 1u;
		n = kept;
		const uint32_t len = n * (sNext - s); // passes s .. sNext - 1 hold the same n pixels
		for (uint32_t idx = threadIdx.x; idx < len; idx += kBlock)
			if (off + idx < total)
				list[off + idx] = pixSh[cur][idx % n];
		off += len;
		s = sNext;
		__syncthreads(); // minSh and the LDS lists are rewritten by the next round
	}
}

// ======================================================================================
// tyr_allocate_samples: v_p = error[p] when finite and > 0, else 0; m = max v; q_p = min(floor(v_p * (2^20 / m)), 2^20) (every
// q_p = 1 when m == 0); Q = the inclusive prefix sums of q in 64-bit integers; extra_p = floor(E Q_p / Q) - floor(E Q_{p-1} / Q)
// in 128-bit integers; c_p = min(min_spp + extra_p, max_spp).  Integer sums: the split of the reduction and of the scan does
// not change a bit of the result.
// ======================================================================================
constexpr float kQuantScale = 1048576.0f;
constexpr uint32_t kQuantMax = 1048576u;

__device__ __forceinline__ float usable_error(const AllocateArgs& A, uint32_t p) {
	const float v = A.error[frame_index(p, A.W, A.rank, A.nranks)];
	return (v > 0.0f && v <= FLT_MAX) ? v : 0.0f; // (NaN fails both tests, +inf the second)
}

__global__ void __launch_bounds__(kBlock) k_alloc_max(const AllocateArgs A) {
	const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
	const float v = p < A.localPixels ? usable_error(A, p) : 0.0f;
	const uint32_t m = wave_max_u32(__float_as_uint(v)); // non-negative floats order like their bits
	if ((threadIdx.x & 63u) == 0 && m != 0u)
		atomicMax(A.maxBits, m);
}

__global__ void __launch_bounds__(kBlock) k_alloc_scan(const AllocateArgs A) {
	__shared__ unsigned long long waveSum[kBlock / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const float m = __uint_as_float(*A.maxBits);
	const float scale = kQuantScale / m; // one binary32 division (unused when m == 0; +inf when m is below ~3.1e-33)
	unsigned long long carry = 0;
#pragma unroll
	for (uint32_t r = 0; r < kCompactTile / kBlock; ++r) {
		const uint32_t p = blockIdx.x * kCompactTile + r * kBlock + threadIdx.x;
		unsigned long long q = 0;
		if (p < A.localPixels) {
			if (m > 0.0f) {
				const float v = usable_error(A, p);
				if (scale <= FLT_MAX) {
					const float f = floorf(v * scale); // in [0, 2^20 (1 + 2^-22)]: converted only below 2^20
					q = f < kQuantScale ? (uint32_t)f : kQuantMax;
				} else {
					q = v > 0.0f ? kQuantMax : 0u; // 2^20 / m overflowed (m < ~3.1e-33): every usable error gets the full weight
				}
			} else {
				q = 1;
			}
		}
		unsigned long long incl = q;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const unsigned long long u = __shfl_up(incl, (unsigned)o, 64);
			if (lane >= (uint32_t)o)
				incl += u;
		}
		if (lane == 63u)
			waveSum[wave] = incl;
		__syncthreads();
		unsigned long long before = carry, tot = 0;
#pragma unroll
		for (uint32_t w = 0; w < kBlock / 64; ++w) {
			if (w < wave)
				before += waveSum[w];
			tot += waveSum[w];
		}
		if (p < A.localPixels)
			A.scan[p] = before + incl;
		carry += tot;
		__syncthreads();
	}
	if (threadIdx.x == 0)
		A.blockSum[blockIdx.x] = carry;
}

// one block: the blocks' totals -> exclusive prefixes, in place
__global__ void __launch_bounds__(kBlock) k_alloc_scan_blocks(const AllocateArgs A, uint32_t nBlocks) {
	__shared__ unsigned long long waveSum[kBlock / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	unsigned long long carry = 0;
	for (uint32_t base = 0; base < nBlocks; base += kBlock) {
		const uint32_t i = base + threadIdx.x;
		const unsigned long long v = i < nBlocks ? A.blockSum[i] : 0ull;
		unsigned long long incl = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const unsigned long long u = __shfl_up(incl, (unsigned)o, 64);
			if (lane >= (uint32_t)o)
				incl += u;
		}
		if (lane == 63u)
			waveSum[wave] = incl;
		__syncthreads();
		unsigned long long before = carry, tot = 0;
#pragma unroll
		for (uint32_t w = 0; w < kBlock / 64; ++w) {
			if (w < wave)
				before += waveSum[w];
			tot += waveSum[w];
		}
		if (i < nBlocks)
			A.blockSum[i] = before + incl - v;
		carry += tot;
		__syncthreads();
	}
}

__device__ __forceinline__ unsigned long long prefix_at(const AllocateArgs& A, uint32_t p) { return A.scan[p] + A.blockSum[p / kCompactTile]; }

__global__ void __launch_bounds__(kBlock) k_alloc_map(const AllocateArgs A) {
	const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
	uint32_t c = 0;
	if (p < A.localPixels) {
		const unsigned long long Q = prefix_at(A, A.localPixels - 1u); // >= 1: the largest error's weight is 2^20 (or every weight is 1)
		const unsigned long long Qp = prefix_at(A, p), Qq = p ? prefix_at(A, p - 1u) : 0ull;
		const unsigned __int128 E = A.extra;
		const unsigned long long hi = (unsigned long long)((E * Qp) / Q), lo = (unsigned long long)((E * Qq) / Q);
		const unsigned long long want = (unsigned long long)A.minSpp + (hi - lo);
		c = (uint32_t)(want < A.maxSpp ? want : A.maxSpp);
		A.mapOut[frame_index(p, A.W, A.rank, A.nranks)] = c;
	}
	const uint32_t sum = wave_sum_u32(c);
	if ((threadIdx.x & 63u) == 0 && sum)
		atomicAdd(A.totalOut, (unsigned long long)sum);
}

// ---- launch wrappers ---------------------------------------------------------------------

void launch_map_hist(const SampleMapArgs& A, uint32_t localPixels, hipStream_t stream) {
	hipLaunchKernelGGL(k_map_hist, dim3(blocks_for(localPixels)), dim3(kBlock), 0, stream, A, localPixels);
}
void launch_pass_compact(const uint32_t* in, uint32_t n, const uint32_t* counts, uint32_t s, uint32_t* out, uint32_t outLimit, uint32_t* blockCnt, hipStream_t stream) {
	if (n == 0)
		return;
	const uint32_t blocks = (n + kCompactTile - 1) / kCompactTile;
	hipLaunchKernelGGL(k_pass_count, dim3(blocks), dim3(kBlock), 0, stream, in, n, counts, s, blockCnt);
	hipLaunchKernelGGL(k_pass_scan_blocks, dim3(1), dim3(kBlock), 0, stream, blockCnt, blocks);
	hipLaunchKernelGGL(k_pass_scatter, dim3(blocks), dim3(kBlock), 0, stream, in, n, counts, s, out, outLimit, blockCnt);
}
void launch_pass_repeat(uint32_t* list, uint32_t src, uint32_t n, uint32_t dst, uint32_t copies, uint32_t total, hipStream_t stream) {
	const uint32_t len = n * copies; // (<= T < 2^32)
	if (len != 0)
		hipLaunchKernelGGL(k_pass_repeat, dim3(std::min(blocks_for(len), 8192u)), dim3(kBlock), 0, stream, list, src, n, dst, len, total);
}
void launch_pass_tail(uint32_t* list, const uint32_t* in, uint32_t nIn, const uint32_t* counts, uint32_t sFirst, uint32_t maxSpp, uint32_t outOff, uint32_t total, hipStream_t stream) {
	hipLaunchKernelGGL(k_pass_tail, dim3(1), dim3(kBlock), 0, stream, list, in, nIn, counts, sFirst, maxSpp, outOff, total);
}
void launch_allocate(const AllocateArgs& A, hipStream_t stream) {
	const uint32_t tiles = (A.localPixels + kCompactTile - 1) / kCompactTile;
	hipLaunchKernelGGL(k_alloc_max, dim3(blocks_for(A.localPixels)), dim3(kBlock), 0, stream, A);
	hipLaunchKernelGGL(k_alloc_scan, dim3(tiles), dim3(kBlock), 0, stream, A);
	hipLaunchKernelGGL(k_alloc_scan_blocks, dim3(1), dim3(kBlock), 0, stream, A, tiles);
	hipLaunchKernelGGL(k_alloc_map, dim3(blocks_for(A.localPixels)), dim3(kBlock), 0, stream, A);
}

} // namespace tyr
